// map_locate.cpp -- include/obvi_map_locate.h: one device-resident map located in another from the constellations of their object centres (map_kernels.hip).
// The host checks the arguments, carves the workspaces out of the handle's one-call workspace (map_window.h), launches up to the counts and ends in the report
// tail it shares with the match (finish_report): when hypotheses are to be reported, their ranking and refinement are launched between its two waits.
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
  MapLocateDev m{};
  m.od = od; m.na = (int32_t)na; m.nb = (int32_t)nb; m.min_inliers = p.min_inliers; m.iterations = p.refine_iterations;
  m.has_label_a = label_a ? 1 : 0; m.has_label_b = label_b ? 1 : 0;
  m.dmin = p.pair_min_distance; m.tol = p.pair_tolerance; m.gate = p.inlier_gate; m.seed_cap = seed_cap;
  m.mean_a = a->d_mean; m.cov_a = a->d_cov; m.mean_b = b->d_mean; m.cov_b = b->d_cov;
  int32_t* d_label_a = nullptr; int32_t* d_label_b = nullptr;
  carve_workspace(h, [&](Carver& c) {
    if (label_a) d_label_a = c.take<int32_t>(na);
    if (label_b) d_label_b = c.take<int32_t>(nb);
    m.rec = c.take<double>((na + nb) * kLocateRec); m.lab = c.take<int32_t>(na + nb);
    m.row_cnt = c.take<int64_t>(2 * rows); m.row_off = c.take<int64_t>(rows); m.totals = c.take<int64_t>(3);
    m.blk_cnt = c.take<int64_t>(blocks); m.blk_off = c.take<int64_t>(blocks);
    m.seeds = c.take<uint32_t>(4 * seed_cap); m.inl = c.take<int32_t>(seed_cap); m.cost = c.take<double>(seed_cap);   // entries [0, totals[1]) are written, and no other is read
    m.qlist = c.take<uint32_t>(seed_cap); m.sel = c.take<uint32_t>(cap); m.out_seed = c.take<uint32_t>(4 * cap);
    m.out_T = c.take<double>(4 * cap); m.out_cov = c.take<double>(16 * cap); m.out_cost = c.take<double>(cap);
    m.out_inl = c.take<int32_t>(cap); m.out_partner = c.take<int32_t>(nb * cap);
  });
  if (label_a) h2d_async(d_label_a, label_a, sizeof(int32_t) * (size_t)na, s);
  if (label_b) h2d_async(d_label_b, label_b, sizeof(int32_t) * (size_t)nb, s);
  m.label_a = d_label_a; m.label_b = d_label_b;
  launch_map_locate_score(s, m);
  return finish_report(h, m.totals, 2, cap,
                       {{seed, m.out_seed, sizeof(uint32_t) * 4}, {transform, m.out_T, sizeof(double) * 4}, {transform_cov, m.out_cov, sizeof(double) * 16}, {inliers, m.out_inl, sizeof(int32_t)},
                        {cost, m.out_cost, sizeof(double)}, {partner, m.out_partner, sizeof(int32_t) * (size_t)nb}},
                       counts, [&](const int64_t* totals, int64_t out) {
    if (totals[1] > seed_cap) {
      counts[0] = totals[0]; counts[1] = totals[1]; counts[2] = 0;
      return fail(h, OBVI_ERR_OUT_OF_RANGE, "map_locate: more than OBVI_MAP_LOCATE_MAX_SEEDS compatible seeds: tighten pair_tolerance or add labels");
    }
    if (out > 0) {   // the second half, between the two waits
      m.found = totals[2]; m.out = out;
      launch_map_locate_report(s, m);
      OBVI_HIP(hipGetLastError());
    }
    return (int)OBVI_OK;
  });
  OBVI_API_END(h)
}

}  // extern "C"
