// bbox_store_kernels.hip -- the appearance store of the bounding-box data association (include/obvi_bbox_store.h): the views of bbox_frontend_kernels.hip kept on the
// device between rounds.  The feature ids of all views lie in one append-only device array, the pool; the directory -- per owner the ordered views, each an
// (offset, length) into the pool -- lives on the host and holds no ids.  A round runs the kernels of bbox_kernels.h over pool segments, so it uploads the frame,
// the boxes and 16 bytes per listed view, whatever the views hold -- written into one page-locked block and sent in one copy.  Two kernels are the store's own:
//   k_bbox_view_append   one wavefront per committed box: walks the caller's feature positions in trips of 64; a lane reads its feature's bit of the box through
//                        the caller-to-sorted permutation; its slot is the popcount of the ballot below its lane plus the running total -- the ids land in the
//                        caller's feature order, which is the order the host path stores them in
//   k_bbox_pool_compact  one wavefront per live view copies its segment to its new offset in a fresh pool
// A mutating call judges its arguments first, queues its device work next and changes the directory last, after the stream has drained: a refusal or a failure
// leaves the directory as it was.  The round's device buffers belong to the store, grow on demand and are not freed between calls.
#include <algorithm>
#include <cmath>
#include <map>
#include <new>
#include <numeric>
#include <set>
#include <utility>
#include <vector>

#include "../../include/obvi_bbox_store.h"
#include "ba_device.h"
#include "bbox_kernels.h"
#include "host_util.h"

namespace obvi {
namespace {

using namespace bbox;   // NOLINT: the shared kernels and their limits

constexpr int64_t kDefaultPoolIds = 65536, kDefaultCompactMinDeadIds = 65536;
constexpr int64_t kMaxPoolIds = (int64_t)1 << 40;

struct AppendBatch {
  int64_t n_feat, n_jobs; int32_t words;
  const uint64_t* ids;        // the round's ids, ascending
  const uint32_t* inv;        // sorted position of the caller's feature i
  const uint64_t* bits;       // [n_feat][words]
  const uint64_t* jobs;       // [n_jobs][3]: box, offset of the new view in the pool, its length (the round's feats_in_box)
};

__global__ void __launch_bounds__(kBlock) k_bbox_view_append(AppendBatch a, uint64_t* pool) {
  const int lane = threadIdx.x & 63;
  const int64_t j = blockIdx.x * (int64_t)kWavesPerBlock + (threadIdx.x >> 6);
  if (j >= a.n_jobs) return;                                         // a whole wavefront leaves: the ballots below stay complete
  const uint64_t b = a.jobs[3 * j], dst = a.jobs[3 * j + 1], len = a.jobs[3 * j + 2];
  const int64_t w = (int64_t)(b >> 6);
  const int bit = (int)(b & 63);
  const unsigned long long below = ((unsigned long long)1 << lane) - 1;
  uint64_t running = 0;
  for (int64_t base = 0; base < a.n_feat; base += 64) {
    const int64_t i = base + lane;
    bool inside = false;
    uint64_t id = 0;
    if (i < a.n_feat) {
      const int64_t s = (int64_t)a.inv[i];
      inside = (a.bits[s * a.words + w] >> bit) & 1;
      id = a.ids[s];
    }
    const unsigned long long votes = __ballot(inside);
    const uint64_t slot = running + (uint64_t)__popcll(votes & below);
    if (inside && slot < len) pool[dst + slot] = id;                 // slot < len always: both come from the same bit rows; the test keeps a write inside the view
    running += (uint64_t)__popcll(votes);
  }
}

__global__ void __launch_bounds__(kBlock) k_bbox_pool_compact(int64_t n_moves, const uint64_t* moves /*[n_moves][3]: from, to, length*/, const uint64_t* from, uint64_t* to) {
  const int lane = threadIdx.x & 63;
  for (int64_t v = blockIdx.x * (int64_t)kWavesPerBlock + (threadIdx.x >> 6); v < n_moves; v += (int64_t)gridDim.x * kWavesPerBlock) {
    const uint64_t src = moves[3 * v], dst = moves[3 * v + 1], len = moves[3 * v + 2];
    for (uint64_t k = lane; k < len; k += 64) to[dst + k] = from[src + k];
  }
}

struct Seg { uint64_t off, len; };
typedef std::pair<uint64_t, uint64_t> Key;      // (frame, camera)
typedef std::map<Key, Seg> Views;

struct Pool {                                    // exactly `cap` ids: the capacity is part of the interface
  uint64_t* p = nullptr; int64_t cap = 0;
  Pool() = default;
  Pool(const Pool&) = delete;
  Pool& operator=(const Pool&) = delete;
  ~Pool() { if (p) (void)hipFree(p); }
  void alloc(int64_t n) { OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&p), (size_t)n * sizeof(uint64_t))); cap = n; }
  void swap(Pool& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
};

struct Pinned {                                  // page-locked host memory, grow-only: the staging of a round's one upload and of its read-back
  void* p = nullptr; size_t cap = 0;
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  ~Pinned() { if (p) (void)hipHostFree(p); }
  void ensure(size_t bytes) {
    if (bytes <= cap && p) return;
    if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; }
    const size_t c = bytes + bytes / 4 + 4096;
    OBVI_HIP(hipHostMalloc(&p, c, hipHostMallocDefault));
    cap = c;
  }
};

struct Round {                                   // what a successful associate leaves for commit: on the device the ids and the permutation (in d_up) and d_bits
  bool kept = false;
  int64_t n_feat = 0, n_box = 0; int32_t words = 0;
  const uint64_t* d_ids = nullptr; const uint32_t* d_inv = nullptr;
  std::vector<uint32_t> count;                   // feats_in_box
};

}  // namespace
}  // namespace obvi

struct obvi_bbox_store {
  obvi_ba_handle* h = nullptr;
  std::map<int64_t, obvi::Views> owners;         // the directory: live owners only, in token order
  int64_t next_owner = 0, views = 0, live_ids = 0, dead_ids = 0, growths = 0, compactions = 0, replaced = 0, upload_bytes = 0, compact_min_dead = 0;
  obvi::Pool pool;                               // [0, live_ids + dead_ids) in use
  obvi::Round round;
  // workspace of a round
  obvi::Pinned h_up, h_down;
  obvi::DevBuf<uint8_t> d_up, d_in, d_match; obvi::DevBuf<uint64_t> d_bits, d_jobs; obvi::DevBuf<double> d_score; obvi::DevBuf<uint32_t> d_count, d_overlap;
};

namespace obvi {
namespace {

int64_t tail(const obvi_bbox_store* s) { return s->live_ids + s->dead_ids; }

// room for `extra` more ids behind the tail: the capacity doubles until they fit
void reserve(obvi_bbox_store* s, int64_t extra, hipStream_t st) {
  const int64_t need = tail(s) + extra;
  if (need <= s->pool.cap) return;
  int64_t cap = s->pool.cap;
  while (cap < need) cap *= 2;
  Pool bigger;
  bigger.alloc(cap);
  if (tail(s) > 0) OBVI_HIP(hipMemcpyAsync(bigger.p, s->pool.p, (size_t)tail(s) * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  OBVI_HIP(hipStreamSynchronize(st));
  s->pool.swap(bigger);                          // the old array goes with `bigger`
  ++s->growths;
}

void compact(obvi_bbox_store* s) {
  OBVI_HIP(hipSetDevice(handle_device(s->h)));
  hipStream_t st = handle_stream(s->h);
  std::vector<uint64_t> moves;
  moves.reserve((size_t)(3 * s->views));
  uint64_t at = 0;
  for (const auto& o : s->owners) for (const auto& v : o.second) { moves.push_back(v.second.off); moves.push_back(at); moves.push_back(v.second.len); at += v.second.len; }
  if (at > 0) {
    Pool fresh;
    fresh.alloc(s->pool.cap);
    const int64_t n = (int64_t)moves.size() / 3;
    s->d_jobs.upload(moves, st);
    const unsigned grid = (unsigned)std::min<int64_t>((n + kWavesPerBlock - 1) / kWavesPerBlock, kOverlapMaxBlocks);
    hipLaunchKernelGGL(k_bbox_pool_compact, dim3(grid), dim3(kBlock), 0, st, n, s->d_jobs.get(), s->pool.p, fresh.p);
    OBVI_HIP(hipGetLastError());
    OBVI_HIP(hipStreamSynchronize(st));
    s->pool.swap(fresh);
  }
  size_t k = 0;
  for (auto& o : s->owners) for (auto& v : o.second) { v.second.off = moves[3 * k + 1]; ++k; }
  s->dead_ids = 0;
  ++s->compactions;
}

// the rule of the header, after a mutating call that succeeded.  The mutation stands whatever happens here: a compaction that fails leaves the pool as it was.
void compact_if_due(obvi_bbox_store* s) {
  if (s->dead_ids < s->compact_min_dead || s->dead_ids <= s->live_ids) return;
  try { compact(s); } catch (...) { (void)hipStreamSynchronize(handle_stream(s->h)); }
}

// `v` becomes the view `key` of `views`; what was there turns into dead ids
void place(obvi_bbox_store* s, Views& views, const Key& key, const Seg& v, bool count_replaced) {
  const auto ins = views.insert({key, v});
  if (!ins.second) {
    s->live_ids -= (int64_t)ins.first->second.len; s->dead_ids += (int64_t)ins.first->second.len;
    ins.first->second = v;
    if (count_replaced) ++s->replaced;
  } else {
    ++s->views;
  }
  s->live_ids += (int64_t)v.len;
}

void drop_owner(obvi_bbox_store* s, int64_t owner) {
  const auto it = s->owners.find(owner);
  for (const auto& v : it->second) { s->live_ids -= (int64_t)v.second.len; s->dead_ids += (int64_t)v.second.len; }
  s->views -= (int64_t)it->second.size();
  s->owners.erase(it);
}

int refuse(const obvi_bbox_store* s, int code, const char* msg) { return handle_fail(s->h, code, msg); }

}  // namespace
}  // namespace obvi

#define OBVI_STORE_CATCH(s)                                                                                           \
  catch (const obvi::HipError& e) { (void)hipStreamSynchronize(obvi::handle_stream((s)->h)); return obvi::refuse(s, OBVI_ERR_HIP, e.what); }        \
  catch (const std::exception& e) { (void)hipStreamSynchronize(obvi::handle_stream((s)->h)); return obvi::refuse(s, OBVI_ERR_HIP, e.what()); }      \
  catch (...) { (void)hipStreamSynchronize(obvi::handle_stream((s)->h)); return obvi::refuse(s, OBVI_ERR_HIP, "unknown host exception"); }

extern "C" {

int obvi_bbox_store_create(obvi_ba_handle* h, const obvi_bbox_store_options* opt, obvi_bbox_store** out) {
  using namespace obvi;   // NOLINT
  if (!h || !out) return OBVI_ERR_INVALID_ARGUMENT;
  if (opt && (opt->initial_pool_ids < 0 || opt->compact_min_dead_ids < 0 || opt->initial_pool_ids > kMaxPoolIds)) return handle_fail(h, OBVI_ERR_INVALID_ARGUMENT, "bbox store create: bad options");
  obvi_bbox_store* s = nullptr;
  try {
    s = new obvi_bbox_store;
    s->h = h;
    s->compact_min_dead = opt && opt->compact_min_dead_ids ? opt->compact_min_dead_ids : kDefaultCompactMinDeadIds;
    OBVI_HIP(hipSetDevice(handle_device(h)));
    s->pool.alloc(opt && opt->initial_pool_ids ? opt->initial_pool_ids : kDefaultPoolIds);
  } catch (const HipError& e) { delete s; return handle_fail(h, OBVI_ERR_HIP, e.what); }
  catch (...) { delete s; return handle_fail(h, OBVI_ERR_HIP, "bbox store create: host allocation failed"); }
  *out = s;
  return OBVI_OK;
}

void obvi_bbox_store_destroy(obvi_bbox_store* s) {
  if (!s) return;
  (void)hipSetDevice(obvi::handle_device(s->h));
  (void)hipStreamSynchronize(obvi::handle_stream(s->h));
  delete s;
}

int obvi_bbox_store_new_owners(obvi_bbox_store* s, int64_t n, int64_t* owner_out) {
  using namespace obvi;   // NOLINT
  if (!s || (n > 0 && !owner_out)) return OBVI_ERR_INVALID_ARGUMENT;
  if (n < 0) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store new_owners: negative count");
  try {
    std::map<int64_t, Views> fresh;
    for (int64_t i = 0; i < n; ++i) fresh.emplace_hint(fresh.end(), s->next_owner + i, Views());
    s->owners.merge(fresh);                      // relinks nodes: cannot fail
    for (int64_t i = 0; i < n; ++i) owner_out[i] = s->next_owner + i;
    s->next_owner += n;
    return OBVI_OK;
  } OBVI_STORE_CATCH(s)
}

int obvi_bbox_store_put_views(obvi_bbox_store* s, int64_t n_views, const int64_t* owner, const uint64_t* frame, const uint64_t* camera, const uint64_t* feat_ptr,
                              const uint64_t* view_feat) {
  using namespace obvi;   // NOLINT
  if (!s || !feat_ptr || (n_views > 0 && (!owner || !frame || !camera)) || (n_views >= 0 && feat_ptr[n_views] > 0 && !view_feat)) return OBVI_ERR_INVALID_ARGUMENT;
  if (n_views < 0) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store put_views: negative count");
  if (feat_ptr[0] != 0) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store put_views: feat_ptr must start at 0 and ascend");
  for (int64_t k = 0; k < n_views; ++k) if (feat_ptr[k + 1] < feat_ptr[k]) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store put_views: feat_ptr must start at 0 and ascend");
  const uint64_t total = feat_ptr[n_views];
  if (total > (uint64_t)kMaxPoolIds) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store put_views: too many ids");
  try {
    std::set<std::pair<int64_t, Key>> seen;
    std::vector<uint64_t> sorted;
    for (int64_t k = 0; k < n_views; ++k) {
      if (!s->owners.count(owner[k])) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store put_views: unknown or released owner");
      if (!seen.insert({owner[k], Key(frame[k], camera[k])}).second) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store put_views: the same view of an owner twice");
      sorted.assign(view_feat + feat_ptr[k], view_feat + feat_ptr[k + 1]);
      std::sort(sorted.begin(), sorted.end());
      if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store put_views: a feature id occurs twice in a view");
    }
    OBVI_HIP(hipSetDevice(handle_device(s->h)));
    hipStream_t st = handle_stream(s->h);
    reserve(s, (int64_t)total, st);
    const uint64_t base = (uint64_t)tail(s);
    if (total > 0) {
      OBVI_HIP(hipMemcpyAsync(s->pool.p + base, view_feat, (size_t)total * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      OBVI_HIP(hipStreamSynchronize(st));
    }
    for (int64_t k = 0; k < n_views; ++k) place(s, s->owners.find(owner[k])->second, Key(frame[k], camera[k]), Seg{base + feat_ptr[k], feat_ptr[k + 1] - feat_ptr[k]}, true);
    compact_if_due(s);
    return OBVI_OK;
  } OBVI_STORE_CATCH(s)
}

int obvi_bbox_store_associate(obvi_bbox_store* s, int64_t n_feat, const uint64_t* feat_id, const double* feat_pixel, int64_t n_box, const double* box_corners,
                              const int32_t* box_label, int64_t n_cand, const int64_t* cand_owner, const int32_t* cand_label, const obvi_bbox_frontend_params* prm,
                              uint8_t* in_box, uint32_t* feats_in_box, uint32_t* overlap, uint8_t* is_match, double* score) {
  using namespace obvi;   // NOLINT
  if (!s || !prm || (n_feat > 0 && (!feat_id || !feat_pixel)) || (n_box > 0 && (!box_corners || !box_label)) || (n_cand > 0 && (!cand_owner || !cand_label)))
    return OBVI_ERR_INVALID_ARGUMENT;
  if (n_feat < 0 || n_box < 0 || n_cand < 0) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store associate: bad arguments");
  if (n_feat > (int64_t)UINT32_MAX || n_box > (int64_t)INT32_MAX - 64) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store associate: too many features or boxes");
  const int64_t most = n_box > 0 ? kMaxOutputEntries / n_box : kMaxOutputEntries;
  if (n_feat > most || n_cand > most) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store associate: boxes times features, views or candidates above 2^31");
  if (!std::isfinite(prm->bounding_box_inflation_size) || !std::isfinite(prm->min_overlapping_features_for_match))
    return refuse(s, OBVI_ERR_NUMERICAL, "bbox store associate: non-finite parameter");
  for (int64_t i = 0; i < 4 * n_box; ++i) if (!std::isfinite(box_corners[i])) return refuse(s, OBVI_ERR_NUMERICAL, "bbox store associate: non-finite box corner");
  try {
    // the candidates' stored views, in candidate order, then (frame, camera) order: view_ptr and 16 bytes a view
    {
      std::vector<int64_t> listed(cand_owner, cand_owner + n_cand);
      std::sort(listed.begin(), listed.end());
      if (std::adjacent_find(listed.begin(), listed.end()) != listed.end()) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store associate: an owner listed twice");
    }
    std::vector<const Views*> cand_views((size_t)n_cand);
    int64_t n_views = 0;
    for (int64_t c = 0; c < n_cand; ++c) {
      const auto o = s->owners.find(cand_owner[c]);
      if (o == s->owners.end()) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store associate: unknown or released owner");
      cand_views[c] = &o->second;
      n_views += (int64_t)o->second.size();
    }
    if (n_views > most) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store associate: boxes times features, views or candidates above 2^31");
    OBVI_HIP(hipSetDevice(handle_device(s->h)));
    // Everything the round uploads is written into one pinned block, the 8-byte items first, and goes to the device in one copy:
    //   ids[n_feat] pix[n_feat][2] view_ptr[n_cand + 1] seg[n_views][2] corners[n_box][4] | orig[n_feat] inv[n_feat] box_label[n_box] cand_label[n_cand]
    const size_t n8 = (size_t)(3 * n_feat + (n_cand + 1) + 2 * n_views + 4 * n_box), n4 = (size_t)(2 * n_feat + n_box + n_cand);
    const size_t up_bytes = 8 * n8 + 4 * n4;
    s->h_up.ensure(up_bytes);
    auto carve = [n_feat, n_cand, n_views, n_box](uint8_t* base, auto&& take) {
      uint64_t* w = reinterpret_cast<uint64_t*>(base);
      uint64_t* ids = w; double* pix = reinterpret_cast<double*>(ids + n_feat); uint64_t* vptr = reinterpret_cast<uint64_t*>(pix + 2 * n_feat); uint64_t* seg = vptr + n_cand + 1;
      double* corners = reinterpret_cast<double*>(seg + 2 * n_views);
      uint32_t* orig = reinterpret_cast<uint32_t*>(corners + 4 * n_box); uint32_t* inv = orig + n_feat;
      int32_t* blabel = reinterpret_cast<int32_t*>(inv + n_feat); int32_t* clabel = blabel + n_box;
      take(ids, pix, vptr, seg, corners, orig, inv, blabel, clabel);
    };
    bool twice = false;
    carve(static_cast<uint8_t*>(s->h_up.p), [&](uint64_t* ids, double* pix, uint64_t* vptr, uint64_t* seg, double* corners, uint32_t* orig, uint32_t* inv, int32_t* blabel, int32_t* clabel) {
      // the frame's features in ascending id order, and both permutations
      std::iota(orig, orig + n_feat, 0u);
      std::sort(orig, orig + n_feat, [&](uint32_t a, uint32_t b) { return feat_id[a] < feat_id[b]; });
      for (int64_t k = 0; k < n_feat; ++k) {
        ids[k] = feat_id[orig[k]];
        twice = twice || (k > 0 && ids[k] == ids[k - 1]);
        pix[2 * k] = feat_pixel[2 * (int64_t)orig[k]]; pix[2 * k + 1] = feat_pixel[2 * (int64_t)orig[k] + 1];
        inv[orig[k]] = (uint32_t)k;
      }
      vptr[0] = 0;
      uint64_t v = 0;
      for (int64_t c = 0; c < n_cand; ++c) {
        for (const auto& view : *cand_views[c]) { seg[2 * v] = view.second.off; seg[2 * v + 1] = view.second.len; ++v; }
        vptr[c + 1] = v;
      }
      std::copy(box_corners, box_corners + 4 * n_box, corners);
      std::copy(box_label, box_label + n_box, blabel);
      std::copy(cand_label, cand_label + n_cand, clabel);
    });
    if (twice) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store associate: a feature id occurs twice in the frame");
    Round next;
    next.kept = true; next.n_feat = n_feat; next.n_box = n_box; next.words = (int32_t)((n_box + 63) / 64);
    if (n_box == 0) {                                                // every output has a zero dimension; a commit of no boxes may follow
      s->round = std::move(next);
      s->upload_bytes = 0;
      return OBVI_OK;
    }
    hipStream_t st = handle_stream(s->h);
    const int32_t words = next.words;
    s->round.kept = false;                                           // from here on the kept round's buffers are written over
    s->d_up.resize(up_bytes);
    OBVI_HIP(hipMemcpyAsync(s->d_up.get(), s->h_up.p, up_bytes, hipMemcpyHostToDevice, st));
    const uint64_t* d_ids = nullptr; const double* d_pix = nullptr; const uint64_t* d_vptr = nullptr; const uint64_t* d_seg = nullptr; const double* d_corners = nullptr;
    const uint32_t* d_orig = nullptr; const uint32_t* d_inv = nullptr; const int32_t* d_blabel = nullptr; const int32_t* d_clabel = nullptr;
    carve(s->d_up.get(), [&](uint64_t* ids, double* pix, uint64_t* vptr, uint64_t* seg, double* corners, uint32_t* orig, uint32_t* inv, int32_t* blabel, int32_t* clabel) {
      d_ids = ids; d_pix = pix; d_vptr = vptr; d_seg = seg; d_corners = corners; d_orig = orig; d_inv = inv; d_blabel = blabel; d_clabel = clabel;
    });
    next.d_ids = d_ids; next.d_inv = d_inv;
    s->d_count.resize((size_t)n_box); s->d_count.zero(st);
    if (n_feat > 0) {
      s->d_bits.resize((size_t)(n_feat * words));
      if (in_box) s->d_in.resize((size_t)(n_box * n_feat));
      MemberBatch m{n_feat, (int32_t)n_box, words, d_pix, d_orig, d_corners, prm->bounding_box_inflation_size};
      hipLaunchKernelGGL(k_bbox_membership, dim3((unsigned)((n_feat + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, m, s->d_bits.get(), in_box ? s->d_in.get() : nullptr, s->d_count.get());
      OBVI_HIP(hipGetLastError());
    }
    const PoolViews views{d_seg, s->pool.p};
    if (n_views > 0) {
      s->d_overlap.resize((size_t)(n_box * n_views));
      if (n_feat > 0) {
        OverlapBatch o{n_feat, n_views, (int32_t)n_box, words, d_ids, s->d_bits.get()};
        const unsigned grid = (unsigned)std::min<int64_t>((n_views + kWavesPerBlock - 1) / kWavesPerBlock, kOverlapMaxBlocks);
        if (n_feat <= kLdsFeatureLimit) hipLaunchKernelGGL((k_bbox_overlap<true, PoolViews>), dim3(grid), dim3(kBlock), 0, st, o, views, s->d_overlap.get());
        else hipLaunchKernelGGL((k_bbox_overlap<false, PoolViews>), dim3(grid), dim3(kBlock), 0, st, o, views, s->d_overlap.get());
        OBVI_HIP(hipGetLastError());
      } else {
        s->d_overlap.zero(st);                                       // no features in the frame: nothing to search in
      }
    }
    // Read back into one pinned block beside the caller's arrays (a failure leaves those untouched): score | count, overlap | is_match, in_box
    const bool want_score = n_cand > 0 && (is_match || score), want_in = in_box && n_feat > 0, want_overlap = overlap && n_views > 0;
    const size_t n_bc = (size_t)(n_box * n_cand), n_bv = (size_t)(n_box * n_views), n_bf = (size_t)(n_box * n_feat);
    s->h_down.ensure(8 * n_bc + 4 * ((size_t)n_box + n_bv) + n_bc + n_bf);
    double* h_score = static_cast<double*>(s->h_down.p);
    uint32_t* h_count = reinterpret_cast<uint32_t*>(h_score + n_bc); uint32_t* h_overlap = h_count + n_box;
    uint8_t* h_match = reinterpret_cast<uint8_t*>(h_overlap + n_bv); uint8_t* h_in = h_match + n_bc;
    if (want_score) {
      s->d_match.resize(n_bc); s->d_score.resize(n_bc);
      ScoreBatch sb{n_box, n_cand, n_views, d_blabel, d_clabel, d_vptr, s->d_overlap.get(), s->d_count.get(), prm->min_overlapping_features_for_match};
      hipLaunchKernelGGL(k_bbox_score<PoolViews>, dim3((unsigned)((n_box * n_cand + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, sb, views, s->d_match.get(), s->d_score.get());
      OBVI_HIP(hipGetLastError());
      s->d_match.download(h_match, n_bc, st);
      if (score) s->d_score.download(h_score, n_bc, st);
    }
    if (want_in) s->d_in.download(h_in, n_bf, st);
    s->d_count.download(h_count, (size_t)n_box, st);                  // the store keeps the counts: they are the lengths of the views a commit appends
    if (want_overlap) s->d_overlap.download(h_overlap, n_bv, st);
    OBVI_HIP(hipStreamSynchronize(st));
    next.count.assign(h_count, h_count + n_box);
    if (want_in) std::copy(h_in, h_in + n_bf, in_box);
    if (feats_in_box) std::copy(h_count, h_count + n_box, feats_in_box);
    if (want_overlap) std::copy(h_overlap, h_overlap + n_bv, overlap);
    if (want_score && is_match) std::copy(h_match, h_match + n_bc, is_match);
    if (want_score && score) for (size_t i = 0; i < n_bc; ++i) if (h_match[i]) score[i] = h_score[i];
    s->round = std::move(next);
    s->upload_bytes = (int64_t)up_bytes;
    return OBVI_OK;
  } OBVI_STORE_CATCH(s)
}

int obvi_bbox_store_commit(obvi_bbox_store* s, uint64_t frame_id, uint64_t camera_id, int64_t n_box, const int64_t* box_owner) {
  using namespace obvi;   // NOLINT
  if (!s || (n_box > 0 && !box_owner)) return OBVI_ERR_INVALID_ARGUMENT;
  if (!s->round.kept) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store commit: no round is kept");
  if (n_box != s->round.n_box) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store commit: n_box is not the round's");
  try {
    std::set<int64_t> seen;
    std::vector<uint64_t> jobs;
    int64_t total = 0;
    for (int64_t b = 0; b < n_box; ++b) {
      if (box_owner[b] == -1) continue;
      if (!s->owners.count(box_owner[b])) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store commit: unknown or released owner");
      if (!seen.insert(box_owner[b]).second) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store commit: an owner twice");
      jobs.push_back((uint64_t)b); jobs.push_back((uint64_t)total); jobs.push_back(s->round.count[b]);
      total += (int64_t)s->round.count[b];
    }
    const int64_t n_jobs = (int64_t)jobs.size() / 3;
    if (total > 0) {
      OBVI_HIP(hipSetDevice(handle_device(s->h)));
      hipStream_t st = handle_stream(s->h);
      reserve(s, total, st);
      for (int64_t j = 0; j < n_jobs; ++j) jobs[3 * j + 1] += (uint64_t)tail(s);
      s->d_jobs.upload(jobs, st);
      AppendBatch a{s->round.n_feat, n_jobs, s->round.words, s->round.d_ids, s->round.d_inv, s->d_bits.get(), s->d_jobs.get()};
      hipLaunchKernelGGL(k_bbox_view_append, dim3((unsigned)((n_jobs + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kBlock), 0, st, a, s->pool.p);
      OBVI_HIP(hipGetLastError());
      OBVI_HIP(hipStreamSynchronize(st));
    } else {
      for (int64_t j = 0; j < n_jobs; ++j) jobs[3 * j + 1] += (uint64_t)tail(s);
    }
    for (int64_t j = 0; j < n_jobs; ++j) place(s, s->owners.find(box_owner[jobs[3 * j]])->second, Key(frame_id, camera_id), Seg{jobs[3 * j + 1], jobs[3 * j + 2]}, true);
    s->round.kept = false;
    compact_if_due(s);
    return OBVI_OK;
  } OBVI_STORE_CATCH(s)
}

int obvi_bbox_store_merge(obvi_bbox_store* s, int64_t n, const int64_t* from, const int64_t* into) {
  using namespace obvi;   // NOLINT
  if (!s || (n > 0 && (!from || !into))) return OBVI_ERR_INVALID_ARGUMENT;
  if (n < 0) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store merge: negative count");
  try {
    std::set<int64_t> gone;
    for (int64_t i = 0; i < n; ++i) {
      if (from[i] == into[i]) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store merge: an owner onto itself");
      if (!s->owners.count(from[i]) || !s->owners.count(into[i]) || gone.count(from[i]) || gone.count(into[i]))
        return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store merge: unknown or released owner");
      gone.insert(from[i]);
    }
    for (int64_t i = 0; i < n; ++i) {
      const auto src = s->owners.find(from[i]);
      Views& dst = s->owners.find(into[i])->second;
      for (const auto& v : src->second) {                            // into[v.first] = v.second (:244-273): from's view stays where both hold the key
        s->live_ids -= (int64_t)v.second.len; --s->views;            // ... it only changes hands
        place(s, dst, v.first, v.second, false);
      }
      s->owners.erase(src);
    }
    compact_if_due(s);
    return OBVI_OK;
  } OBVI_STORE_CATCH(s)
}

int obvi_bbox_store_release(obvi_bbox_store* s, int64_t n, const int64_t* owner) {
  using namespace obvi;   // NOLINT
  if (!s || (n > 0 && !owner)) return OBVI_ERR_INVALID_ARGUMENT;
  if (n < 0) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store release: negative count");
  try {
    std::set<int64_t> seen;
    for (int64_t i = 0; i < n; ++i)
      if (!s->owners.count(owner[i]) || !seen.insert(owner[i]).second) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store release: unknown or released owner, or an owner twice");
    for (int64_t i = 0; i < n; ++i) drop_owner(s, owner[i]);
    compact_if_due(s);
    return OBVI_OK;
  } OBVI_STORE_CATCH(s)
}

int obvi_bbox_store_apply_window(obvi_bbox_store* s, uint64_t frame_id, uint64_t window, int64_t* dropped) {
  using namespace obvi;   // NOLINT
  if (!s) return OBVI_ERR_INVALID_ARGUMENT;
  int64_t n = 0;
  for (auto& o : s->owners)
    for (auto it = o.second.begin(); it != o.second.end();)
      if (it->first.first + window < frame_id) {                     // uint64_t: the sum wraps, as the host path's does
        s->live_ids -= (int64_t)it->second.len; s->dead_ids += (int64_t)it->second.len; --s->views; ++n;
        it = o.second.erase(it);
      } else {
        ++it;
      }
  if (dropped) *dropped = n;
  compact_if_due(s);
  return OBVI_OK;
}

int obvi_bbox_store_compact(obvi_bbox_store* s) {
  using namespace obvi;   // NOLINT
  if (!s) return OBVI_ERR_INVALID_ARGUMENT;
  try {
    compact(s);
    return OBVI_OK;
  } OBVI_STORE_CATCH(s)
}

int obvi_bbox_store_views(const obvi_bbox_store* s, int64_t owner, int64_t* n_views, int64_t* n_ids, uint64_t* frame, uint64_t* camera, uint64_t* feat_ptr,
                          uint64_t* view_feat) {
  using namespace obvi;   // NOLINT
  if (!s) return OBVI_ERR_INVALID_ARGUMENT;
  const auto o = s->owners.find(owner);
  if (o == s->owners.end()) return refuse(s, OBVI_ERR_INVALID_ARGUMENT, "bbox store views: unknown or released owner");
  try {
    uint64_t total = 0;
    for (const auto& v : o->second) total += v.second.len;
    std::vector<uint64_t> h_ids;
    if (view_feat && total > 0) {
      h_ids.resize((size_t)total);
      OBVI_HIP(hipSetDevice(handle_device(s->h)));
      hipStream_t st = handle_stream(s->h);
      uint64_t at = 0;
      for (const auto& v : o->second) {
        if (v.second.len) OBVI_HIP(hipMemcpyAsync(h_ids.data() + at, s->pool.p + v.second.off, (size_t)v.second.len * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        at += v.second.len;
      }
      OBVI_HIP(hipStreamSynchronize(st));
    }
    if (n_views) *n_views = (int64_t)o->second.size();
    if (n_ids) *n_ids = (int64_t)total;
    uint64_t at = 0;
    int64_t k = 0;
    for (const auto& v : o->second) {
      if (frame) frame[k] = v.first.first;
      if (camera) camera[k] = v.first.second;
      if (feat_ptr) feat_ptr[k] = at;
      at += v.second.len; ++k;
    }
    if (feat_ptr) feat_ptr[k] = at;
    std::copy(h_ids.begin(), h_ids.end(), view_feat);
    return OBVI_OK;
  } OBVI_STORE_CATCH(s)
}

int obvi_bbox_store_get_stats(const obvi_bbox_store* s, obvi_bbox_store_stats* out) {
  if (!s || !out) return OBVI_ERR_INVALID_ARGUMENT;
  *out = obvi_bbox_store_stats{(int64_t)s->owners.size(), s->views, s->live_ids, s->dead_ids, s->pool.cap, s->growths, s->compactions, s->replaced, s->upload_bytes};
  return OBVI_OK;
}

}  // extern "C"
