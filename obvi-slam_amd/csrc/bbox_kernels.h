// bbox_kernels.h -- the device code of the bounding-box data association, shared by its two launchers: the stateless round of bbox_frontend_kernels.hip
// (include/obvi_bbox_frontend.h), whose views arrive as a CSR with every call, and the round of bbox_store_kernels.hip (include/obvi_bbox_store.h), whose views
// are segments of a pool that stays on the device.  The kernels are templates over where a view's ids lie; everything else -- the membership test, the search,
// the ballots, the match rule and the arithmetic of the score -- is one piece of code, so both entries compute the same bytes.
//   k_bbox_membership  one thread per frame feature (in sorted order): which boxes hold it, as a row of ceil(n_box / 64) 64-bit words; per-box counts from
//                      wavefront ballots and one integer atomic per wavefront and box
//   k_bbox_overlap     one wavefront per view: a lane looks one id of the view up in the sorted list (binary search; the list in LDS while it fits) and fetches
//                      the bit row of the feature found; the count of a box is the popcount of the ballot of its bit
//   k_bbox_score       one thread per (box, candidate): the largest overlap and the sum of intersection over union over the candidate's views, in view order
// All integer work except the score; the only atomics are integer adds, so a deterministic handle runs the same code.
#ifndef OBVI_BBOX_KERNELS_H_
#define OBVI_BBOX_KERNELS_H_

#include <hip/hip_runtime.h>

#include <cstdint>

namespace obvi {
namespace bbox {
namespace {   // internal linkage: each of the two launchers' translation units carries its own copy of the kernels and registers it with its own code object

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kLdsFeatureLimit = 4096;      // ids of the frame kept in LDS by k_bbox_overlap: 32 KiB, five workgroups per CU
constexpr int64_t kMaxOutputEntries = (int64_t)1 << 31;   // n_box x n_feat, n_box x n_views, n_box x n_cand each: buffers below 16 GiB, the score grid below 2^23 workgroups
constexpr int kOverlapMaxBlocks = 1024;     // k_bbox_overlap strides over the views: a workgroup stages the list once for all of its views

// Where the ids of view v lie.  CSR: view_feat[feat_ptr[v] .. feat_ptr[v + 1]).  Segments: pool[seg[2 v] .. seg[2 v] + seg[2 v + 1]).
struct CsrViews {
  const uint64_t* feat_ptr; const uint64_t* view_feat;
  __device__ const uint64_t* ids(int64_t v) const { return view_feat + feat_ptr[v]; }
  __device__ uint64_t length(int64_t v) const { return feat_ptr[v + 1] - feat_ptr[v]; }
};
struct PoolViews {
  const uint64_t* seg; const uint64_t* pool;        // seg[n_views][2]: (offset, length)
  __device__ const uint64_t* ids(int64_t v) const { return pool + seg[2 * v]; }
  __device__ uint64_t length(int64_t v) const { return seg[2 * v + 1]; }
};

struct MemberBatch {
  int64_t n_feat; int32_t n_box, words;
  const double* pixel;        // [n_feat][2] in sorted-id order
  const uint32_t* orig;       // position of sorted feature s in the caller's arrays
  const double* corners;      // [n_box][4] min_x max_x min_y max_y
  double inflation;
};

__global__ void __launch_bounds__(kBlock) k_bbox_membership(MemberBatch m, uint64_t* bits, uint8_t* in_box, uint32_t* count) {
  const int64_t s = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  const bool live = s < m.n_feat;                                  // no early return: every lane takes part in the ballots
  const int lane = threadIdx.x & 63;
  const double px = live ? m.pixel[2 * s] : 0.0, py = live ? m.pixel[2 * s + 1] : 0.0;
  const int64_t o = live ? (int64_t)m.orig[s] : 0;
  for (int w = 0; w < m.words; ++w) {
    const int nb = min(64, m.n_box - 64 * w);
    uint64_t word = 0;
    for (int j = 0; j < nb; ++j) {
      const int64_t b = 64 * (int64_t)w + j;
      const double* c = m.corners + 4 * b;
      // inflateBoundingBox, then pixelInBoundingBoxClosedSet (ellipsoid_utils.h:347-361)
      const bool inside = live && (c[0] - m.inflation <= px) && (c[2] - m.inflation <= py) && (c[1] + m.inflation >= px) && (c[3] + m.inflation >= py);
      if (inside) word |= (uint64_t)1 << j;
      if (in_box && live) in_box[b * m.n_feat + o] = inside ? 1 : 0;
      const unsigned long long votes = __ballot(inside);
      if (lane == 0 && votes) atomicAdd(&count[b], (uint32_t)__popcll(votes));
    }
    if (live) bits[s * m.words + w] = word;
  }
}

struct OverlapBatch {
  int64_t n_feat, n_views; int32_t n_box, words;
  const uint64_t* ids;        // the frame's ids, ascending
  const uint64_t* bits;       // [n_feat][words]
};

// position of id in the ascending list, or -1
__device__ inline int64_t find_id(const uint64_t* list, int64_t n, uint64_t id) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (list[mid] < id) lo = mid + 1; else hi = mid;
  }
  return (lo < n && list[lo] == id) ? lo : -1;
}

template <bool kLds, class Views>
__global__ void __launch_bounds__(kBlock) k_bbox_overlap(OverlapBatch o, Views views, uint32_t* overlap) {
  __shared__ uint64_t s_ids[kLds ? kLdsFeatureLimit : 1];
  if (kLds) {
    for (int64_t i = threadIdx.x; i < o.n_feat; i += kBlock) s_ids[i] = o.ids[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t v = blockIdx.x * (int64_t)kWavesPerBlock + wave; v < o.n_views; v += (int64_t)gridDim.x * kWavesPerBlock) {
    const uint64_t* view = views.ids(v);
    const uint64_t len = views.length(v);
    for (int w = 0; w < o.words; ++w) {
      const int nb = min(64, o.n_box - 64 * w);
      uint32_t acc = 0;                                             // lane j: the count of box 64 w + j
      for (uint64_t base = 0; base < len; base += 64) {
        const uint64_t k = base + lane;
        uint64_t word = 0;
        if (k < len) {
          const uint64_t id = view[k];
          int64_t at;
          if (kLds) at = find_id(s_ids, o.n_feat, id); else at = find_id(o.ids, o.n_feat, id);
          if (at >= 0) word = o.bits[at * o.words + w];
        }
        for (int j = 0; j < nb; ++j) {
          const uint32_t c = (uint32_t)__popcll(__ballot((word >> j) & 1));
          if (lane == j) acc += c;
        }
      }
      if (lane < nb) overlap[(64 * (int64_t)w + lane) * o.n_views + v] = acc;
    }
  }
}

struct ScoreBatch {
  int64_t n_box, n_cand, n_views;
  const int32_t* box_label; const int32_t* cand_label;
  const uint64_t* view_ptr;
  const uint32_t* overlap; const uint32_t* count;
  double min_overlap;
};

template <class Views>
__global__ void __launch_bounds__(kBlock) k_bbox_score(ScoreBatch s, Views views, uint8_t* is_match, double* score) {
  const int64_t t = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  if (t >= s.n_box * s.n_cand) return;
  const int64_t b = t / s.n_cand, c = t % s.n_cand;
  uint8_t match = 0;
  double value = 0.0;
  if (s.box_label[b] == s.cand_label[c]) {
    const uint64_t v0 = s.view_ptr[c], v1 = s.view_ptr[c + 1];
    const uint64_t in_box = s.count[b];
    uint32_t best = 0;
    double sum = 0.0;
    for (uint64_t v = v0; v < v1; ++v) {
      const uint32_t n = s.overlap[b * s.n_views + (int64_t)v];
      best = max(best, n);
      if (n != 0) sum += (double)n / (double)(in_box + views.length((int64_t)v) - n);   // :467-473
    }
    if (v1 > v0 && (double)best >= s.min_overlap) {                 // :408-411; no views: not a match (the header's first departure)
      match = 1;
      value = sum / (double)(v1 - v0);                              // :476
    }
  }
  is_match[t] = match;
  score[t] = value;
}

}  // namespace
}  // namespace bbox
}  // namespace obvi
#endif  // OBVI_BBOX_KERNELS_H_
