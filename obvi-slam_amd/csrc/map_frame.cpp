// map_frame.cpp -- include/obvi_map_frame.h: a device-resident map moved into another frame under a transform that is itself an estimate, and two maps joined
// into one (map_kernels.hip).  The host checks the arguments, symmetrises the transform's covariance, launches into a freshly allocated map (map_window.h),
// reads the status record back and hands the new map out only when nothing was refused.  Nothing is factored: neither entry has a row limit but the map's own.
#include "map_window.h"
#include "../../include/obvi_map_frame.h"

extern "C" {

int obvi_map_transform(obvi_ba_handle* h, const obvi_map* map, const double* transform, const double* transform_cov, obvi_map** out) {
  if (out) *out = nullptr;
  if (!h || !map || !transform || !out) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_transform: bad arguments");
  // device and block size: the checks of every window, with no objects named
  { const int rc = check_window(h, map, 0, nullptr, 0, "map_transform"); if (rc != OBVI_OK) return rc; }
  const int od = h->od, dT = od == 7 ? 4 : 6, K = od - 3;
  for (int i = 0; i < dT; ++i) if (!std::isfinite(transform[i])) return fail(h, OBVI_ERR_NUMERICAL, "map_transform: a transform that is not finite");
  if (transform_cov) for (int i = 0; i < dT * dT; ++i) if (!std::isfinite(transform_cov[i])) return fail(h, OBVI_ERR_NUMERICAL, "map_transform: a transform covariance entry that is not finite");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int64_t n = map->n;
  const MapCutDev m = window_cut(h, 0, nullptr);   // the status record alone, zeroed
  std::unique_ptr<obvi_map, MapDeleter> fresh = allocate_map(map->device, od, n);
  inherit_power_start(fresh.get(), map, s);
  MapFrameDev f{};
  f.od = od; f.n = (int32_t)n; f.has_sigma = transform_cov ? 1 : 0;
  std::copy(transform, transform + dT, f.transform);
  if (transform_cov) for (int i = 0; i < dT; ++i) for (int j = 0; j < dT; ++j) f.sigma[i * dT + j] = 0.5 * (transform_cov[i * dT + j] + transform_cov[j * dT + i]);
  f.map_mean = map->d_mean; f.map_cov = map->d_cov;
  // k_mf_jac writes J of every object, and G and GS when there is a Sigma_s: they are read only then
  carve_workspace(h, [&](Carver& c) { f.J = c.take<double>(n * K * K); f.G = c.take<double>(n * K * dT); f.GS = c.take<double>(n * K * dT); });
  f.out_mean = fresh->d_mean; f.out_cov = fresh->d_cov; f.status = m.status;
  launch_map_transform(s, f);
  { const int rc = finish_window_call(h, false, "", "map_transform: a non-finite entry in the new map"); if (rc != OBVI_OK) return rc; }
  *out = fresh.release();
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_map_join(obvi_ba_handle* h, const obvi_map* a, const obvi_map* b, obvi_map** out) {
  if (out) *out = nullptr;
  if (!h || !a || !b || !out) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_join: bad arguments");
  { const int rc = check_window(h, a, 0, nullptr, 0, "map_join"); if (rc != OBVI_OK) return rc; }
  { const int rc = check_window(h, b, 0, nullptr, 0, "map_join"); if (rc != OBVI_OK) return rc; }
  if (a->n + b->n > kMapMaxRows / h->od) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_join: the joined map's covariance would exceed 1 GiB");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  std::unique_ptr<obvi_map, MapDeleter> fresh = allocate_map(a->device, a->od, a->n + b->n);
  inherit_power_start(fresh.get(), a, s);
  launch_map_join(s, a->n * a->od, a->d_mean, a->d_cov, b->n * b->od, b->d_mean, b->d_cov, fresh->d_mean, fresh->d_cov);
  OBVI_HIP(hipGetLastError());
  sync(h);   // the call's one wait
  *out = fresh.release();
  return OBVI_OK;
  OBVI_API_END(h)
}

}  // extern "C"
