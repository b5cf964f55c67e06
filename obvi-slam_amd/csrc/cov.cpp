// cov.cpp -- covariance blocks of poses, features and objects by selected inversion of the reduced system's factor, and of any pair declared up front
// (include/obvi_cov.h, include/obvi_cov_pairs.h; kernels: cov_kernels.hip; shared state and helpers: ba_handle.h)
#include "ba_handle.h"
#include "../../include/obvi_cov.h"

#include <map>

namespace {

// What the inversion and the pattern test need of the symbolic plan, rebuilt when the plan was: the first scratch tile of every tile column inside its
// level (the Y tiles of a level lie one behind the other in the order of the level's columns) and the tile mask of L.  Read back from the plan's own
// device tables, so the symbolic phase of a solve carries nothing for it.
void cov_plan_tables(obvi_ba_handle* h) {
  if (h->cov_plan_serial == h->plan_serial) return;
  hipStream_t s = h->stream;
  const int32_t nt = h->nt;
  std::vector<int32_t> lvl_k((size_t)nt + 1), col_ptr((size_t)nt + 2), tiles((size_t)2 * h->ntiles + 2);
  h->d_lvl_k.download(lvl_k.data(), (size_t)nt, s); h->d_col_ptr.download(col_ptr.data(), (size_t)nt + 1, s); h->d_tiles.download(tiles.data(), (size_t)2 * h->ntiles, s);
  sync(h);
  std::vector<int32_t> ybase((size_t)nt + 1, 0);
  int64_t widest = 0;
  for (int l = 0; l < h->nlevels; ++l) {
    int64_t at = 0;
    for (int32_t x = h->h_lvl_k_ptr[l]; x < h->h_lvl_k_ptr[l + 1]; ++x) { const int32_t k = lvl_k[x]; ybase[k] = (int32_t)at; at += col_ptr[k + 1] - col_ptr[k]; }
    widest = std::max(widest, at);
  }
  h->h_cov_mask.assign((size_t)nt * nt, 0);
  for (int32_t t = 0; t < h->ntiles; ++t) h->h_cov_mask[(size_t)tiles[2 * t] * nt + tiles[2 * t + 1]] = 1;
  h->d_cov_ybase.upload(ybase, s);
  h->d_cov_ys.resize((size_t)widest * kTile * kTile + 1);
  sync(h);
  h->cov_plan_serial = h->plan_serial;
}

bool cov_ready(obvi_ba_handle* h) { return h->cov_valid && !h->dirty && !h->mask_dirty; }
const char* const kNotReady = "no covariance pass for the current state: call obvi_cov_compute (values, factors, masks, flags or priors changed, or a solve ran)";

// first row and size of a reduced block in the tile grid; row -1: constant or unused (a zero block); false: a kind the reduced system does not hold
bool block_rows(const obvi_ba_handle* h, int kind, uint32_t idx, int32_t* row, int32_t* dim) {
  if (kind == OBVI_COV_POSE) { const int32_t v = h->h_cov_pose_vid[idx]; *row = v >= 0 ? h->h_pose_row[v] : -1; *dim = 6; return true; }
  if (kind == OBVI_COV_OBJECT) { const int32_t v = h->h_obj_vid[idx]; *row = v >= 0 ? h->h_obj_row[v] : -1; *dim = h->od; return true; }
  return false;
}
int64_t block_count(const obvi_ba_handle* h, int kind) { return kind == OBVI_COV_POSE ? h->P : kind == OBVI_COV_POINT ? h->L : h->O; }
int32_t block_dim(const obvi_ba_handle* h, int kind) { return kind == OBVI_COV_POSE ? 6 : kind == OBVI_COV_POINT ? 3 : h->od; }
bool block_known(const obvi_ba_handle* h, int kind, uint32_t idx) { return kind <= OBVI_COV_OBJECT && (int64_t)idx < block_count(h, kind); }
uint64_t pair_side(int kind, uint32_t idx) { return (uint64_t)kind << 32 | idx; }
bool on_pattern(const obvi_ba_handle* h, int32_t ra, int32_t da, int32_t rb, int32_t db) {
  if (ra < 0 || rb < 0) return true;   // a zero block
  for (int32_t ta = ra / kTile; ta <= (ra + da - 1) / kTile; ++ta)
    for (int32_t tb = rb / kTile; tb <= (rb + db - 1) / kTile; ++tb)
      if (!h->h_cov_mask[(size_t)std::max(ta, tb) * h->nt + std::min(ta, tb)]) return false;
  return true;
}
// desc (4 per item) / off -> out, one launch and one wait
void gather(obvi_ba_handle* h, const std::vector<int32_t>& desc, const std::vector<int64_t>& off, int64_t extent, double* out) {
  const int64_t n = (int64_t)off.size();
  if (n == 0 || extent == 0) return;
  hipStream_t s = h->stream;
  h->d_cov_desc.upload(desc, s); h->d_cov_off.upload(off, s);
  h->d_cov_blk.resize((size_t)extent);
  OBVI_HIP(hipMemsetAsync(h->d_cov_blk.get(), 0, sizeof(double) * (size_t)extent, s));   // (gaps the caller's offsets leave)
  launch_cov_gather(s, h->d_S.get(), h->nt, n, h->d_cov_desc.get(), h->d_cov_off.get(), h->d_cov_blk.get());
  OBVI_HIP(hipGetLastError());
  std::vector<double> host((size_t)extent);
  h->d_cov_blk.download(host.data(), (size_t)extent, s);
  sync(h);
  for (int64_t i = 0; i < n; ++i) std::memcpy(out + off[i], host.data() + off[i], sizeof(double) * (size_t)(desc[4 * i + 2] * desc[4 * i + 3]));
}
int own_blocks(obvi_ba_handle* h, const char* what, int kind, int64_t n, const uint32_t* idx, double* out) {
  if (!h || n < 0 || (n > 0 && (!idx || !out))) return OBVI_ERR_INVALID_ARGUMENT;
  const int64_t cnt = kind == OBVI_COV_POSE ? h->P : h->O;
  for (int64_t i = 0; i < n; ++i) if ((int64_t)idx[i] >= cnt) return fail(h, OBVI_ERR_OUT_OF_RANGE, std::string(what) + ": index out of range");
  if (!cov_ready(h)) return fail(h, OBVI_ERR_NOT_READY, std::string(what) + ": " + kNotReady);
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  std::vector<int32_t> desc((size_t)4 * n); std::vector<int64_t> off((size_t)n);
  int32_t dim = kind == OBVI_COV_POSE ? 6 : h->od;
  for (int64_t i = 0; i < n; ++i) {
    int32_t row = -1;
    block_rows(h, kind, idx[i], &row, &dim);
    desc[4 * i] = row; desc[4 * i + 1] = row; desc[4 * i + 2] = dim; desc[4 * i + 3] = dim; off[i] = i * dim * dim;
  }
  gather(h, desc, off, n * dim * dim, out);
  return OBVI_OK;
  OBVI_API_END(h)
}
// the pairs' rows; OBVI_OK, or the status of the first pair that cannot be served (`on` given: no failure for an off-pattern pair, the answer per pair)
int pair_rows(obvi_ba_handle* h, const char* what, int64_t n, const uint8_t* ka, const uint32_t* ia, const uint8_t* kb, const uint32_t* ib, std::vector<int32_t>* desc, uint8_t* on,
              std::vector<int64_t>* src) {
  desc->resize((size_t)4 * n);
  src->assign((size_t)n, -2);
  for (int64_t i = 0; i < n; ++i) {
    if (!h->h_cov_pairs.empty() && block_known(h, ka[i], ia[i]) && block_known(h, kb[i], ib[i])) {   // a pair declared to obvi_cov_compute_pairs that this route does not serve
      const uint64_t a = pair_side(ka[i], ia[i]), b = pair_side(kb[i], ib[i]);
      const auto it = h->h_cov_pairs.find({std::min(a, b), std::max(a, b)});
      if (it != h->h_cov_pairs.end()) {
        int32_t* d = desc->data() + 4 * i;
        d[0] = d[1] = -1; d[2] = block_dim(h, ka[i]); d[3] = block_dim(h, kb[i]);
        (*src)[i] = it->second < 0 ? -1 : it->second ^ (b < a ? 1 : 0);
        if (on) on[i] = 1;
        continue;
      }
    }
    for (int side = 0; side < 2; ++side) {
      const int kind = side ? kb[i] : ka[i]; const uint32_t idx = side ? ib[i] : ia[i];
      if (kind == OBVI_COV_POINT) return fail(h, OBVI_ERR_INVALID_ARGUMENT, std::string(what) + ": cross blocks of features are not served (obvi_cov_point_blocks gives a feature's own block)");
      if (kind != OBVI_COV_POSE && kind != OBVI_COV_OBJECT) return fail(h, OBVI_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown block kind");
      if ((int64_t)idx >= (kind == OBVI_COV_POSE ? h->P : h->O)) return fail(h, OBVI_ERR_OUT_OF_RANGE, std::string(what) + ": index out of range");
    }
    int32_t* d = desc->data() + 4 * i;
    block_rows(h, ka[i], ia[i], &d[0], &d[2]); block_rows(h, kb[i], ib[i], &d[1], &d[3]);
    const bool ok = on_pattern(h, d[0], d[2], d[1], d[3]);
    if (on) on[i] = ok ? 1 : 0;
    else if (!ok) {
      char buf[320];
      std::snprintf(buf, sizeof(buf), "%s: pair %lld (%s %u, %s %u) is not on the tile pattern of the factor: its covariance is not zero, it is not computed%s", what, (long long)i,
                    ka[i] == OBVI_COV_POSE ? "pose" : "object", ia[i], kb[i] == OBVI_COV_POSE ? "pose" : "object", ib[i],
                    ka[i] == OBVI_COV_OBJECT && kb[i] == OBVI_COV_OBJECT ? " (obvi_ba_object_covariances serves any pair of objects)" : "");
      return fail(h, OBVI_ERR_INVALID_ARGUMENT, buf);
    }
  }
  return OBVI_OK;
}

// What obvi_cov_compute_pairs adds to a pass, laid out on the host before the step runs (the factor exists only between the factorisation and the
// selected inversion): the right-hand sides and block products of the reduced pairs off the pattern, the requests of the pairs with a feature and
// the operands each of them reads, and where every declared block lands in the side buffer.
struct PairPlan {
  struct Group { int32_t da = 0, db = 0; std::vector<int32_t> rows, cols, first; std::vector<int64_t> off; };   // rows: 2 per pair, the blocks' first rows
  Group groups[3];                                   // (6, 6), (6, od), (od, od)
  std::map<int32_t, int32_t> rhs_blocks;             // first row -> rows, of the distinct blocks in off-pattern pairs: ascending = elimination order
  std::map<uint64_t, int64_t> reduced;               // first row of the two blocks (a pose before an object, else the lower row first) -> offset
  std::vector<int32_t> rhs_row, slab_first, req;
  std::vector<int64_t> op_ptr{0}, ops, out_off, self_idx;
  std::vector<obvi_ba_handle::CovPairKey> self_keys;
  int64_t side = 0;                                  // doubles of the side buffer
  std::unordered_map<obvi_ba_handle::CovPairKey, int64_t, obvi_ba_handle::CovPairHash> table;
  bool empty() const { return table.empty(); }

  // where Sigma_{a, b} (rows ra.., rb.. >= 0) is read from: -1 the tiles, else offset << 1 | stored as (b, a)
  int64_t operand(const obvi_ba_handle* h, int32_t ra, int32_t da, int32_t rb, int32_t db) {
    if (on_pattern(h, ra, da, rb, db)) return -1;
    const bool swap = da > db || (da == db && ra > rb);
    if (swap) { std::swap(ra, rb); std::swap(da, db); }
    const uint64_t key = (uint64_t)(uint32_t)ra << 32 | (uint32_t)rb;
    auto it = reduced.find(key);
    if (it == reduced.end()) {
      it = reduced.emplace(key, side).first;
      Group& g = groups[da != 6 ? 2 : db != 6 ? 1 : 0];
      g.da = da; g.db = db; g.rows.push_back(ra); g.rows.push_back(rb); g.off.push_back(side);
      side += (int64_t)da * db;
      rhs_blocks[ra] = da; rhs_blocks[rb] = db;
    }
    return it->second << 1 | (swap ? 1 : 0);
  }
};
constexpr int64_t kPairYtMaxBytes = (int64_t)1 << 30;

int plan_pairs(obvi_ba_handle* h, int64_t n, const uint8_t* ka, const uint32_t* ia, const uint8_t* kb, const uint32_t* ib, PairPlan* pp) {
  hipStream_t s = h->stream;
  h->h_cov_pose_vid.assign((size_t)h->P + 1, -1);
  std::vector<uint8_t> point_var((size_t)h->L + 1, 0);
  if (h->P) h->d_pose_vid.download(h->h_cov_pose_vid.data(), (size_t)h->P, s);
  const bool points = h->num_params > 0 && h->n_rp > 0 && h->L > 0;   // else no feature is a parameter of the problem
  if (points) h->d_point_var.download(point_var.data(), (size_t)h->L, s);
  sync(h);
  if (h->m > 0 && h->nt > 0) cov_plan_tables(h);
  for (int64_t i = 0; i < n; ++i) {
    int kA = ka[i], kB = kb[i]; uint32_t iA = ia[i], iB = ib[i];
    if (pair_side(kB, iB) < pair_side(kA, iA)) { std::swap(kA, kB); std::swap(iA, iB); }
    const obvi_ba_handle::CovPairKey key{pair_side(kA, iA), pair_side(kB, iB)};
    if (pp->table.count(key)) continue;
    if (kA != OBVI_COV_POINT && kB != OBVI_COV_POINT) {
      int32_t ra, da, rb, db;
      block_rows(h, kA, iA, &ra, &da); block_rows(h, kB, iB, &rb, &db);
      if (!on_pattern(h, ra, da, rb, db)) pp->table[key] = pp->operand(h, ra, da, rb, db);   // (on the pattern: the getters' own route)
      continue;
    }
    // canonical order: pose < feature < object, so (pose, feature), (feature, feature) or (feature, object); the kernel writes (feature, other)
    const bool first_is_point = kA == OBVI_COV_POINT;
    const int64_t l = pt_internal(h, first_is_point ? iA : iB);
    const bool lvar = points && point_var[l];
    if (kA == OBVI_COV_POINT && kB == OBVI_COV_POINT) {
      const int64_t mm = pt_internal(h, iB);
      if (!lvar || !point_var[mm]) { pp->table[key] = -1; continue; }
      if (l == mm) { pp->table[key] = 0; pp->self_keys.push_back(key); pp->self_idx.push_back(l); continue; }   // (its place: below)
      const uint32_t b0 = h->h_point_ptr[mm], b1 = h->h_point_ptr[mm + 1];
      for (uint32_t a = h->h_point_ptr[l]; a < h->h_point_ptr[l + 1]; ++a)
        for (uint32_t b = b0; b < b1; ++b) {
          const int32_t ra = h->h_rp_yrow[a], rb = h->h_rp_yrow[b];
          pp->ops.push_back(ra < 0 || rb < 0 ? -1 : pp->operand(h, ra, 6, rb, 6));
        }
      pp->req.insert(pp->req.end(), {(int32_t)l, (int32_t)mm, 0, 0});
      pp->op_ptr.push_back((int64_t)pp->ops.size()); pp->out_off.push_back(pp->side);
      pp->table[key] = pp->side << 1;
      pp->side += 9;
      continue;
    }
    int32_t rx, dx;
    block_rows(h, first_is_point ? kB : kA, first_is_point ? iB : iA, &rx, &dx);
    if (!lvar || rx < 0) { pp->table[key] = -1; continue; }
    for (uint32_t a = h->h_point_ptr[l]; a < h->h_point_ptr[l + 1]; ++a) {
      const int32_t ra = h->h_rp_yrow[a];
      pp->ops.push_back(ra < 0 ? -1 : pp->operand(h, ra, 6, rx, dx));
    }
    pp->req.insert(pp->req.end(), {(int32_t)l, rx, dx, 0});
    pp->op_ptr.push_back((int64_t)pp->ops.size()); pp->out_off.push_back(pp->side);
    pp->table[key] = pp->side << 1 | (first_is_point ? 0 : 1);
    pp->side += 3 * dx;
  }
  for (size_t k = 0; k < pp->self_keys.size(); ++k) pp->table[pp->self_keys[k]] = (pp->side + 9 * (int64_t)k) << 1;   // one behind the other: k_cov_points writes them
  // right-hand sides in elimination order, 64 to a slab
  std::map<int32_t, int32_t> col_of;
  for (const auto& rb : pp->rhs_blocks) {
    col_of[rb.first] = (int32_t)pp->rhs_row.size();
    for (int32_t r = 0; r < rb.second; ++r) pp->rhs_row.push_back(rb.first + r);
  }
  const int64_t nslabs = ((int64_t)pp->rhs_row.size() + kTile - 1) / kTile;
  if (nslabs * kTile * (int64_t)h->nt * kTile * (int64_t)sizeof(double) > kPairYtMaxBytes) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), "cov_compute_pairs: the pairs off the tile pattern need %lld right-hand sides of %lld rows: more than the limit of 1 GiB",
                  (long long)pp->rhs_row.size(), (long long)h->nt * kTile);
    return fail(h, OBVI_ERR_INVALID_ARGUMENT, buf);
  }
  for (int64_t sl = 0; sl < nslabs; ++sl) pp->slab_first.push_back(pp->rhs_row[(size_t)sl * kTile] / kTile);
  for (PairPlan::Group& g : pp->groups)
    for (size_t q = 0; q < g.off.size(); ++q) {
      g.cols.push_back(col_of[g.rows[2 * q]]); g.cols.push_back(col_of[g.rows[2 * q + 1]]);
      g.first.push_back(std::max(g.rows[2 * q], g.rows[2 * q + 1]) / kTile * kTile);   // both are zero before
    }
  return OBVI_OK;
}

// the off-pattern reduced blocks, while L and L_kk^-1 are intact
void pairs_before_inversion(obvi_ba_handle* h, const PairPlan& pp, std::vector<size_t>* at32, std::vector<size_t>* at64) {
  hipStream_t s = h->stream;
  // one upload per word size: rhs_row | slab_first | req | (cols, first) per group;  op_ptr | ops | out_off | self_idx | off per group
  std::vector<int32_t> w32; std::vector<int64_t> w64;
  auto put32 = [&](const std::vector<int32_t>& v) { at32->push_back(w32.size()); w32.insert(w32.end(), v.begin(), v.end()); };
  auto put64 = [&](const std::vector<int64_t>& v) { at64->push_back(w64.size()); w64.insert(w64.end(), v.begin(), v.end()); };
  put32(pp.rhs_row); put32(pp.slab_first); put32(pp.req);
  for (const PairPlan::Group& g : pp.groups) { put32(g.cols); put32(g.first); }
  put64(pp.op_ptr); put64(pp.ops); put64(pp.out_off); put64(pp.self_idx);
  for (const PairPlan::Group& g : pp.groups) put64(g.off);
  w32.push_back(0); w64.push_back(0);
  h->d_cov_pair_i32.upload(w32, s); h->d_cov_pair_i64.upload(w64, s);
  const int64_t total = pp.side + 9 * (int64_t)pp.self_idx.size();
  h->d_cov_side.resize((size_t)total + 1);
  OBVI_HIP(hipMemsetAsync(h->d_cov_side.get(), 0, sizeof(double) * ((size_t)total + 1), s));
  if (pp.rhs_row.empty()) return;
  const int32_t* i32 = h->d_cov_pair_i32.get(); const int64_t* i64 = h->d_cov_pair_i64.get();
  const int nslabs = (int)pp.slab_first.size();
  const int64_t ldt = (int64_t)h->nt * kTile;
  h->d_cov_pair_Y.resize((size_t)nslabs * kTile * (size_t)ldt);
  launch_cov_forward(s, chol_plan(h), h->d_S.get(), h->d_Linv.get(), h->d_cov_pair_Y.get(), ldt, nslabs, i32 + (*at32)[1], i32 + (*at32)[0], (int32_t)pp.rhs_row.size());
  for (int q = 0; q < 3; ++q) {
    const PairPlan::Group& g = pp.groups[q];
    launch_cov_rhs_pairs(s, h->d_cov_pair_Y.get(), ldt, (int64_t)g.off.size(), g.da, g.db, i32 + (*at32)[3 + 2 * q], i32 + (*at32)[4 + 2 * q], i64 + (*at64)[4 + q], h->d_cov_side.get());
  }
  OBVI_HIP(hipGetLastError());
}
// the blocks with a feature, from Sigma and the side buffer; then the side buffer comes home
void pairs_after_inversion(obvi_ba_handle* h, const PairPlan& pp, const std::vector<size_t>& at32, const std::vector<size_t>& at64) {
  hipStream_t s = h->stream;
  const int32_t* i32 = h->d_cov_pair_i32.get(); const int64_t* i64 = h->d_cov_pair_i64.get();
  launch_cov_point_cross(s, h->d_S.get(), h->nt, (int64_t)pp.out_off.size(), i32 + at32[2], i64 + at64[0], i64 + at64[1], i64 + at64[2], h->d_point_ptr.get(), h->d_rp_yrow.get(),
                         h->d_Z.get(), h->d_Ci.get(), h->d_cov_side.get());
  launch_cov_points(s, h->d_S.get(), h->nt, (int64_t)pp.self_idx.size(), i64 + at64[3], h->d_point_ptr.get(), h->d_rp_yrow.get(), h->d_point_var.get(), h->d_Z.get(), h->d_Ci.get(),
                    h->d_cov_side.get() + pp.side);
  OBVI_HIP(hipGetLastError());
  const int64_t total = pp.side + 9 * (int64_t)pp.self_idx.size();
  h->h_cov_pair_blk.resize((size_t)total + 1);
  h->d_cov_side.download(h->h_cov_pair_blk.data(), (size_t)total, s);
}

// obvi_cov_compute (n = 0) and obvi_cov_compute_pairs
// `between`: handed to the step (submit_step): runs between the assembly and the factorisation (obvi_cov_debug_compute_pairs)
int cov_pass(obvi_ba_handle* h, const char* what, int64_t n, const uint8_t* ka, const uint32_t* ia, const uint8_t* kb, const uint32_t* ib,
             const std::function<void()>* between = nullptr) {
  const std::string name(what);
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, name + ": cameras not set");
  OBVI_HIP(hipSetDevice(h->device));
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  prepare(h);
  h->cov_valid = false;
  h->h_cov_pairs.clear();
  // objects shared across ranks and an exchange hook: a collective pass (include/obvi_cov.h).  Collective (0) proves the tail order; the step below issues (1), (2)
  // and (3) as in a solve, and (3) sums the failure flags, so every member takes the branch below together.
  if (exchanging(h)) {
    if (n > 0) return fail(h, OBVI_ERR_INVALID_ARGUMENT, name + ": declared pairs are not served on a handle that exchanges shared objects (the collective form is not built)");
    const int trc = prove_tail_order(h, what); if (trc != OBVI_OK) return trc;
  }
  PairPlan pp;
  if (n > 0) { const int prc = plan_pairs(h, n, ka, ia, kb, ib, &pp); if (prc != OBVI_OK) return prc; }
  hipStream_t s = h->stream;
  const double t0 = wall_s();
  h->cov_ms[0] = h->cov_ms[1] = 0.0;
  if (h->num_params > 0) {
    // the undamped system at the current point, factorised: one LM step's linearisation and factorisation with the trust-region radius at infinity
    // (obvi_ba_object_covariances takes the same route); its point pass leaves the Z and C^-1 records the feature blocks are formed from
    upload_parameter_prior_diagonals(h);
    { QuietStep quiet(h, /*use_extra=*/!h->h_pp_kind.empty()); submit_step(h, 1e300, true, true, /*keep_factor=*/true, between); }
    if (h->h_scal[SC_CHOL_FAIL] != 0.0 || h->h_scal[SC_NONFINITE] != 0.0 || !std::isfinite(h->h_scal[SC_STEPSQ]))
      return fail(h, OBVI_ERR_NUMERICAL, name + ": the normal equations are rank deficient at the current estimate");
  }
  const double t1 = wall_s();
  std::vector<size_t> at32, at64;
  if (!pp.empty()) pairs_before_inversion(h, pp, &at32, &at64);
  if (h->m > 0 && h->nt > 0) {
    cov_plan_tables(h);
    launch_selected_inverse(s, chol_plan(h), h->d_S.get(), h->d_Linv.get(), h->d_cov_ys.get(), h->d_cov_ybase.get());
    OBVI_HIP(hipGetLastError());
  }
  if (!pp.empty()) pairs_after_inversion(h, pp, at32, at64);
  h->h_cov_pose_vid.assign((size_t)h->P + 1, -1);
  if (h->P) h->d_pose_vid.download(h->h_cov_pose_vid.data(), (size_t)h->P, s);
  sync(h);
  h->cov_ms[0] = 1e3 * (t1 - t0); h->cov_ms[1] = 1e3 * (wall_s() - t1);
  h->h_cov_pairs.swap(pp.table);
  h->cov_valid = true;
  return OBVI_OK;
}

}  // namespace

extern "C" {

int obvi_cov_compute(obvi_ba_handle* h) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  OBVI_API_BEGIN
  return cov_pass(h, "cov_compute", 0, nullptr, nullptr, nullptr, nullptr);
  OBVI_API_END(h)
}

int obvi_cov_compute_pairs(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b, const uint32_t* idx_b) {
  if (!h || n < 0 || (n > 0 && (!kind_a || !idx_a || !kind_b || !idx_b))) return OBVI_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n; ++i)
    for (int side = 0; side < 2; ++side) {
      const int kind = side ? kind_b[i] : kind_a[i]; const uint32_t idx = side ? idx_b[i] : idx_a[i];
      if (kind > OBVI_COV_OBJECT) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "cov_compute_pairs: unknown block kind");
      if ((int64_t)idx >= block_count(h, kind)) return fail(h, OBVI_ERR_OUT_OF_RANGE, "cov_compute_pairs: index out of range");
    }
  OBVI_API_BEGIN
  return cov_pass(h, "cov_compute_pairs", n, kind_a, idx_a, kind_b, idx_b);
  OBVI_API_END(h)
}

// cov_pass with the `between` hook of the step, as obvi_ba_debug_reduced_solve (abi.cpp) takes it: the same checks of a given system, the same copy
int obvi_cov_debug_compute_pairs(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b, const uint32_t* idx_b, const double* lhs_in,
                                 double* lhs, int32_t* grid_row, int32_t m_cap, int32_t* m_out) {
  if (!h || !lhs || n < 0 || (n > 0 && (!kind_a || !idx_a || !kind_b || !idx_b))) return OBVI_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n; ++i)
    for (int side = 0; side < 2; ++side) {
      const int kind = side ? kind_b[i] : kind_a[i]; const uint32_t idx = side ? idx_b[i] : idx_a[i];
      if (kind > OBVI_COV_OBJECT) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "cov_debug_compute_pairs: unknown block kind");
      if ((int64_t)idx >= block_count(h, kind)) return fail(h, OBVI_ERR_OUT_OF_RANGE, "cov_debug_compute_pairs: index out of range");
    }
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, "cov_debug_compute_pairs: cameras not set");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  if (exchanging(h)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "cov_debug_compute_pairs: the handle exchanges shared objects; the entry inverts a rank's own system only");
  if (h->mask_dirty) h->dirty = true;   // (as obvi_ba_debug_reduced_system)
  prepare(h);
  if (m_out) *m_out = (int32_t)h->m_canon;
  if (h->m_canon > m_cap) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "cov_debug_compute_pairs: buffer too small");
  const int64_t mc = h->m_canon, nt = h->nt;
  if (mc == 0 || h->m == 0 || h->num_params == 0) return cov_pass(h, "cov_debug_compute_pairs", n, kind_a, idx_a, kind_b, idx_b);
  hipStream_t s = h->stream;
  constexpr int64_t TT = (int64_t)kTile * kTile;
  std::vector<double> tiles((size_t)(nt * nt * TT));
  std::vector<int32_t> tl((size_t)2 * h->ntiles);
  h->d_tiles.download(tl.data(), tl.size(), s);
  sync(h);
  std::vector<uint8_t> mk((size_t)nt * nt, 0);   // tiles outside the structural mask are never written and never read
  for (int t = 0; t < h->ntiles; ++t) mk[(size_t)tl[2 * t] * nt + tl[2 * t + 1]] = 1;
  const bool given = lhs_in != nullptr;
  if (given) {
    for (int64_t ci = 0; ci < mc; ++ci)
      for (int64_t cj = 0; cj < mc; ++cj) {
        const double v = lhs_in[ci * mc + cj], w = lhs_in[cj * mc + ci];
        if (!(v == w) && !(v != v && w != w)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "cov_debug_compute_pairs: the given system is not symmetric");
        const int64_t i = h->h_canon_row[ci], j = h->h_canon_row[cj];
        if (v != 0.0 && !mk[(size_t)(std::max(i, j) / kTile) * nt + std::min(i, j) / kTile])
          return fail(h, OBVI_ERR_INVALID_ARGUMENT, "cov_debug_compute_pairs: a non-zero entry of the given system lies outside the structural tile mask");
      }
  }
  // between the step's assembly and its factorisation: the system as the factorisation is about to see it -- or the caller's, put in its place
  const std::function<void()> between = [&] {
    h->d_S.download(tiles.data(), tiles.size(), s);
    sync(h);
    if (!given) return;
    for (int64_t ci = 0; ci < mc; ++ci) {   // real rows only: the padding rows keep the identity the step's clear gave them
      const int64_t i = h->h_canon_row[ci];
      for (int64_t cj = 0; cj < mc; ++cj) {
        const int64_t j = h->h_canon_row[cj];
        const int64_t r = std::max(i, j), c = std::min(i, j);
        const size_t tix = (size_t)(r / kTile) * nt + (c / kTile);
        if (!mk[tix]) continue;
        const double v = lhs_in[ci * mc + cj];
        tiles[tix * TT + (r % kTile) * kTile + (c % kTile)] = v;
        if (r / kTile == c / kTile) tiles[tix * TT + (c % kTile) * kTile + (r % kTile)] = v;   // diagonal tiles are kept symmetric
      }
    }
    OBVI_HIP(hipMemcpyAsync(h->d_S.get(), tiles.data(), tiles.size() * sizeof(double), hipMemcpyHostToDevice, s));
    sync(h);
  };
  const int rc = cov_pass(h, "cov_debug_compute_pairs", n, kind_a, idx_a, kind_b, idx_b, &between);
  if (rc != OBVI_OK && rc != OBVI_ERR_NUMERICAL) return rc;
  for (int64_t ci = 0; ci < mc; ++ci) {
    const int64_t i = h->h_canon_row[ci];
    if (grid_row) grid_row[ci] = (int32_t)i;
    for (int64_t cj = 0; cj < mc; ++cj) {
      const int64_t j = h->h_canon_row[cj];
      const int64_t r = std::max(i, j), c = std::min(i, j);
      const size_t tix = (size_t)(r / kTile) * nt + (c / kTile);
      lhs[ci * mc + cj] = mk[tix] ? tiles[tix * TT + (r % kTile) * kTile + (c % kTile)] : 0.0;
    }
  }
  return rc;
  OBVI_API_END(h)
}

int obvi_cov_pose_blocks(obvi_ba_handle* h, int64_t n, const uint32_t* pose_idx, double* out) { return own_blocks(h, "cov_pose_blocks", OBVI_COV_POSE, n, pose_idx, out); }
int obvi_cov_object_blocks(obvi_ba_handle* h, int64_t n, const uint32_t* obj_idx, double* out) { return own_blocks(h, "cov_object_blocks", OBVI_COV_OBJECT, n, obj_idx, out); }

int obvi_cov_point_blocks(obvi_ba_handle* h, int64_t n, const uint32_t* point_idx, double* out) {
  if (!h || n < 0 || (n > 0 && (!point_idx || !out))) return OBVI_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n; ++i) if ((int64_t)point_idx[i] >= h->L) return fail(h, OBVI_ERR_OUT_OF_RANGE, "cov_point_blocks: index out of range");
  if (!cov_ready(h)) return fail(h, OBVI_ERR_NOT_READY, std::string("cov_point_blocks: ") + kNotReady);
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  if (n == 0) return OBVI_OK;
  hipStream_t s = h->stream;
  const bool any = h->num_params > 0 && h->n_rp > 0;   // else no feature is a parameter of the problem: zero blocks
  std::vector<int64_t> idx((size_t)n);
  for (int64_t i = 0; i < n; ++i) idx[i] = any ? pt_internal(h, point_idx[i]) : -1;
  h->d_cov_off.upload(idx, s);
  h->d_cov_blk.resize((size_t)9 * n);
  launch_cov_points(s, h->d_S.get(), h->nt, n, h->d_cov_off.get(), h->d_point_ptr.get(), h->d_rp_yrow.get(), h->d_point_var.get(), h->d_Z.get(), h->d_Ci.get(), h->d_cov_blk.get());
  OBVI_HIP(hipGetLastError());
  h->d_cov_blk.download(out, (size_t)9 * n, s);
  sync(h);
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_cov_cross_blocks(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b, const uint32_t* idx_b, double* out, const int64_t* out_offset) {
  if (!h || n < 0 || (n > 0 && (!kind_a || !idx_a || !kind_b || !idx_b || !out))) return OBVI_ERR_INVALID_ARGUMENT;
  if (!cov_ready(h)) return fail(h, OBVI_ERR_NOT_READY, std::string("cov_cross_blocks: ") + kNotReady);
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  std::vector<int32_t> desc; std::vector<int64_t> src;
  { const int rc = pair_rows(h, "cov_cross_blocks", n, kind_a, idx_a, kind_b, idx_b, &desc, nullptr, &src); if (rc != OBVI_OK) return rc; }
  std::vector<int64_t> off((size_t)n);
  int64_t extent = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t sz = (int64_t)desc[4 * i + 2] * desc[4 * i + 3];
    if (out_offset && out_offset[i] < 0) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "cov_cross_blocks: negative output offset");
    off[i] = out_offset ? out_offset[i] : extent;
    extent = out_offset ? std::max(extent, off[i] + sz) : extent + sz;
  }
  gather(h, desc, off, extent, out);
  for (int64_t i = 0; i < n; ++i) {   // declared pairs: from the side buffer of the pass, as stored or transposed
    if (src[i] < 0) continue;
    const int32_t da = desc[4 * i + 2], db = desc[4 * i + 3];
    const double* blk = h->h_cov_pair_blk.data() + (src[i] >> 1);
    for (int32_t r = 0; r < da; ++r) for (int32_t c = 0; c < db; ++c) out[off[i] + r * db + c] = (src[i] & 1) ? blk[c * da + r] : blk[r * db + c];
  }
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_cov_on_pattern(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b, const uint32_t* idx_b, uint8_t* on) {
  if (!h || n < 0 || (n > 0 && (!kind_a || !idx_a || !kind_b || !idx_b || !on))) return OBVI_ERR_INVALID_ARGUMENT;
  if (!cov_ready(h)) return fail(h, OBVI_ERR_NOT_READY, std::string("cov_on_pattern: ") + kNotReady);
  OBVI_API_BEGIN
  std::vector<int32_t> desc; std::vector<int64_t> src;
  return pair_rows(h, "cov_on_pattern", n, kind_a, idx_a, kind_b, idx_b, &desc, on, &src);
  OBVI_API_END(h)
}

int obvi_cov_get_stats(const obvi_ba_handle* h, double* linearize_factor_ms, double* inversion_ms, int64_t* scratch_bytes) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  if (linearize_factor_ms) *linearize_factor_ms = h->cov_ms[0];
  if (inversion_ms) *inversion_ms = h->cov_ms[1];
  if (scratch_bytes) *scratch_bytes = (int64_t)(h->d_cov_ys.size() * sizeof(double));
  return OBVI_OK;
}

}  // extern "C"
