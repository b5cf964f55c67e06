// map_merge.cpp -- include/obvi_map_merge.h: duplicate objects of a device-resident map fused into one (map_kernels.hip).  The host checks every index and
// every pair, sets up a one-group cut of the constraint rows (map_window.h: the set-up fold_window uses; the cut's object list is the drop
// list), launches into a freshly allocated, smaller map, reads the cut's status record back and hands the new map out only when nothing was refused.
#include "map_window.h"
#include "../../include/obvi_map_merge.h"

extern "C" {

int obvi_map_merge(obvi_ba_handle* h, const obvi_map* map, int64_t q, const uint32_t* drop_idx, const uint32_t* keep_idx, const double* offset, const double* noise,
                   uint32_t* new_index, obvi_map** out) {
  if (out) *out = nullptr;
  if (!h || !map || !out || q < 1 || !drop_idx || !keep_idx) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_merge: bad arguments");
  const int od = h->od;
  if (q > OBVI_MAP_GROUP_MAX_ROWS / od) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_merge: pairs of more than OBVI_MAP_GROUP_MAX_ROWS rows");
  // device, block size, the range of the drop list and an object dropped twice: the checks of every window
  { const int rc = check_window(h, map, q, drop_idx, q * od, "map_merge"); if (rc != OBVI_OK) return rc; }
  const int64_t n = map->n;
  for (int64_t r = 0; r < q; ++r) if ((int64_t)keep_idx[r] >= n) return fail(h, OBVI_ERR_OUT_OF_RANGE, "map_merge: map index out of range");
  std::vector<uint8_t> dropped((size_t)n, 0);
  for (int64_t r = 0; r < q; ++r) dropped[drop_idx[r]] = 1;
  for (int64_t r = 0; r < q; ++r) {
    if (keep_idx[r] == drop_idx[r]) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_merge: an object merged into itself");
    if (dropped[keep_idx[r]]) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_merge: an object that is dropped in one pair and kept in another (resolve chains to one survivor per group)");
  }
  const int64_t Q = q * od, nn = (int64_t)od * od;
  if (offset) for (int64_t i = 0; i < Q; ++i) if (!std::isfinite(offset[i])) return fail(h, OBVI_ERR_NUMERICAL, "map_merge: an offset that is not finite");
  if (noise) for (int64_t i = 0; i < q * nn; ++i) if (!std::isfinite(noise[i])) return fail(h, OBVI_ERR_NUMERICAL, "map_merge: a noise entry that is not finite");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  // the new map's objects, and where every old one went; all host tables are alive until the wait
  std::vector<uint32_t> kept, where((size_t)n);
  kept.reserve((size_t)(n - q));
  for (int64_t o = 0; o < n; ++o) if (!dropped[o]) { where[o] = (uint32_t)kept.size(); kept.push_back((uint32_t)o); }
  for (int64_t r = 0; r < q; ++r) where[drop_idx[r]] = where[keep_idx[r]];
  const std::vector<double> no_offset(offset ? (size_t)0 : (size_t)Q, 0.0);
  const int64_t N = n * od, NK = (n - q) * od, nQ = map_group_slabs(Q), nK = map_group_slabs(NK), tile = (int64_t)kTile * kTile;
  const MapCutDev m = window_cut(h, q, drop_idx);
  std::unique_ptr<obvi_map, MapDeleter> fresh = allocate_map(map->device, od, n - q);
  inherit_power_start(fresh.get(), map, s);
  MapMergeDev g{};
  g.od = od; g.N = (int32_t)N; g.Q = (int32_t)Q; g.NK = (int32_t)NK; g.nQ = (int32_t)nQ; g.nK = (int32_t)nK;
  g.cut = m; g.map_mean = map->d_mean; g.map_cov = map->d_cov;
  uint32_t* d_keep = nullptr; uint32_t* d_kept = nullptr; double* d_offset = nullptr; double* d_noise = nullptr;
  carve_workspace(h, [&](Carver& c) {
    d_keep = c.take<uint32_t>(q); d_kept = c.take<uint32_t>(n - q); d_offset = c.take<double>(Q);
    if (noise) d_noise = c.take<double>(q * nn);
    g.Wn = c.take<double>(nQ * nQ * tile); g.G = c.take<double>(nK * nQ * tile); g.Y = c.take<double>(nK * nQ * tile);   // whole tiles by k_mu_operands, k_mm_gather, k_mu_gemm
    g.v = c.take<double>(kTile * nQ);                                                                                   // all 64 nQ rows by k_map_wd
  });
  h2d_async(d_keep, keep_idx, sizeof(uint32_t) * (size_t)q, s); h2d_async(d_kept, kept.data(), sizeof(uint32_t) * kept.size(), s);
  h2d_async(d_offset, offset ? offset : no_offset.data(), sizeof(double) * (size_t)Q, s);
  if (noise) h2d_async(d_noise, noise, sizeof(double) * (size_t)(q * nn), s);
  g.keep = d_keep; g.kept = d_kept; g.offset = d_offset; g.noise = d_noise;
  g.out_mean = fresh->d_mean; g.out_cov = fresh->d_cov;
  launch_map_merge(s, g, map->d_x0);
  { const int rc = finish_window_call(h, true, "map_merge: the covariance of the pairs' differences is not SPD, or numerically singular (a pair that is already merged?)",
                                      "map_merge: a non-finite entry in the new map"); if (rc != OBVI_OK) return rc; }
  if (new_index) std::copy(where.begin(), where.end(), new_index);
  *out = fresh.release();
  return OBVI_OK;
  OBVI_API_END(h)
}

}  // extern "C"
