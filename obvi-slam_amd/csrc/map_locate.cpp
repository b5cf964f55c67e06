// map_locate.cpp -- include/obvi_map_locate.h: one device-resident map located in another from the constellations of their object centres (map_kernels.hip).
// The host checks the arguments, lays the workspaces out in the handle's own d_ml_* buffers, launches up to the counts and reads them back; when hypotheses
// are to be reported it launches their ranking and refinement and reads those back.  Two waits at the most.
#include "map_window.h"
#include "../../include/obvi_map_locate.h"

static_assert(OBVI_MAP_LOCATE_MAX_OBJECTS == obvi::kLocateMaxObjects && OBVI_MAP_LOCATE_MAX_SEEDS == obvi::kLocateMaxSeeds, "the header's limits are the kernels'");

extern "C" {

int obvi_map_locate(obvi_ba_handle* h, const obvi_map* a, const obvi_map* b, const int32_t* label_a, const int32_t* label_b, const obvi_map_locate_params* params,
                    int64_t capacity, uint32_t* seed, double* transform, double* transform_cov, int32_t* inliers, double* cost, int32_t* partner, int64_t* counts) {
  if (!h || !a || !b || !params || !counts || capacity < 0 || (capacity > 0 && (!seed || !transform || !inliers || !cost))) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_locate: bad arguments");
  // device and block size: the checks of every window, with no objects named
  { const int rc = check_window(h, a, 0, nullptr, 0, "map_locate"); if (rc != OBVI_OK) return rc; }
  { const int rc = check_window(h, b, 0, nullptr, 0, "map_locate"); if (rc != OBVI_OK) return rc; }
  const obvi_map_locate_params p = *params;
  if (!(std::isfinite(p.pair_min_distance) && p.pair_min_distance > 0.0)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_locate: pair_min_distance must be finite and positive");
  if (!(std::isfinite(p.pair_tolerance) && p.pair_tolerance >= 0.0)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_locate: pair_tolerance must be finite and not negative");
  if (!(std::isfinite(p.inlier_gate) && p.inlier_gate > 0.0)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_locate: the inlier gate must be finite and positive");
  if (p.min_inliers < 2) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_locate: min_inliers must be at least 2");
  if (p.refine_iterations < 0 || p.refine_iterations > 8) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_locate: refine_iterations must lie in 0 .. 8");
  const int64_t na = a->n, nb = b->n;
  if (na + nb > OBVI_MAP_LOCATE_MAX_OBJECTS) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_locate: more than OBVI_MAP_LOCATE_MAX_OBJECTS objects in the two maps");
  if (na < 2 || nb < 2) { counts[0] = counts[1] = counts[2] = 0; return OBVI_OK; }   // no seeds: nothing to launch
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int od = h->od;
  const int64_t rows = na * na, all_seeds = (na * (na - 1) / 2) * (nb * (nb - 1)), seed_cap = std::min(all_seeds, kLocateMaxSeeds), blocks = (seed_cap + 255) / 256;
  const int64_t cap = std::min(capacity, seed_cap);
  if (label_a || label_b) h->d_ml_label.resize((size_t)(na + nb));
  if (label_a) h2d_async(h->d_ml_label.get(), label_a, sizeof(int32_t) * (size_t)na, s);
  if (label_b) h2d_async(h->d_ml_label.get() + na, label_b, sizeof(int32_t) * (size_t)nb, s);
  h->d_ml_rec.resize((size_t)((na + nb) * kLocateRec)); h->d_ml_lab.resize((size_t)(na + nb));
  h->d_ml_cnt.resize((size_t)(3 * rows + 3 + 2 * blocks));
  h->d_ml_seeds.resize((size_t)(4 * seed_cap)); h->d_ml_inl.resize((size_t)seed_cap); h->d_ml_cost.resize((size_t)seed_cap);
  h->d_ml_list.resize((size_t)(seed_cap + cap + 4 * cap)); h->d_ml_dout.resize((size_t)(21 * cap)); h->d_ml_iout.resize((size_t)((1 + nb) * cap));
  MapLocateDev m{};
  m.od = od; m.na = (int32_t)na; m.nb = (int32_t)nb; m.min_inliers = p.min_inliers; m.iterations = p.refine_iterations;
  m.has_label_a = label_a ? 1 : 0; m.has_label_b = label_b ? 1 : 0;
  m.dmin = p.pair_min_distance; m.tol = p.pair_tolerance; m.gate = p.inlier_gate; m.seed_cap = seed_cap;
  m.mean_a = a->d_mean; m.cov_a = a->d_cov; m.mean_b = b->d_mean; m.cov_b = b->d_cov;
  m.label_a = h->d_ml_label.get(); m.label_b = h->d_ml_label.get() + na;
  m.rec = h->d_ml_rec.get(); m.lab = h->d_ml_lab.get();
  m.row_cnt = h->d_ml_cnt.get(); m.row_off = m.row_cnt + 2 * rows; m.totals = m.row_off + rows; m.blk_cnt = m.totals + 3; m.blk_off = m.blk_cnt + blocks;
  m.seeds = h->d_ml_seeds.get(); m.inl = h->d_ml_inl.get(); m.cost = h->d_ml_cost.get();
  m.qlist = h->d_ml_list.get(); m.sel = m.qlist + seed_cap; m.out_seed = m.sel + cap;
  m.out_T = h->d_ml_dout.get(); m.out_cov = m.out_T + 4 * cap; m.out_cost = m.out_cov + 16 * cap;
  m.out_inl = h->d_ml_iout.get(); m.out_partner = m.out_inl + cap;
  launch_map_locate_score(s, m);
  OBVI_HIP(hipGetLastError());
  int64_t totals[3];
  OBVI_HIP(hipMemcpyAsync(totals, m.totals, sizeof(totals), hipMemcpyDeviceToHost, s));
  sync(h);   // the first wait: the three counts
  if (totals[1] > seed_cap) {
    counts[0] = totals[0]; counts[1] = totals[1]; counts[2] = 0;
    return fail(h, OBVI_ERR_OUT_OF_RANGE, "map_locate: more than OBVI_MAP_LOCATE_MAX_SEEDS compatible seeds: tighten pair_tolerance or add labels");
  }
  const int64_t out = std::min(totals[2], cap);
  if (out > 0) {
    m.found = totals[2]; m.out = out;
    launch_map_locate_report(s, m);
    OBVI_HIP(hipGetLastError());
    OBVI_HIP(hipMemcpyAsync(seed, m.out_seed, sizeof(uint32_t) * 4 * out, hipMemcpyDeviceToHost, s));
    OBVI_HIP(hipMemcpyAsync(transform, m.out_T, sizeof(double) * 4 * out, hipMemcpyDeviceToHost, s));
    if (transform_cov) OBVI_HIP(hipMemcpyAsync(transform_cov, m.out_cov, sizeof(double) * 16 * out, hipMemcpyDeviceToHost, s));
    OBVI_HIP(hipMemcpyAsync(inliers, m.out_inl, sizeof(int32_t) * out, hipMemcpyDeviceToHost, s));
    OBVI_HIP(hipMemcpyAsync(cost, m.out_cost, sizeof(double) * out, hipMemcpyDeviceToHost, s));
    if (partner) OBVI_HIP(hipMemcpyAsync(partner, m.out_partner, sizeof(int32_t) * nb * out, hipMemcpyDeviceToHost, s));
    sync(h);   // the second: the hypotheses, only when there are some to report
  }
  std::copy(totals, totals + 3, counts);
  return OBVI_OK;
  OBVI_API_END(h)
}

}  // extern "C"
