// map_update.cpp -- include/obvi_map_update.h: a device-resident map read back, and conditioned on the posterior of a window's objects (map_kernels.hip).
// The host checks every index, cuts the window's objects from the map as one group (the stages of obvi_map_set_group_priors_from_map, in the handle's scratch
// buffers of that call: the handle's own groups are not touched), launches the update into a freshly allocated map, reads the cut's status record back and hands
// the new map out only when nothing was refused.
#include "map_window.h"
#include "../../include/obvi_map_update.h"

namespace {

// The update, with the posterior in d_mu_post (covariance [N_A][N_A], then mean [N_A]) on the handle's stream.  One wait.
int condition(obvi_ba_handle* h, const obvi_map* map, int64_t k, const uint32_t* map_idx, const std::string& what, obvi_map** out) {
  const int od = h->od;
  const int64_t NA = k * od, N = map->n * od, nA = map_group_slabs(NA);
  hipStream_t s = h->stream;
  const MapCutDev m = window_cut(h, k, map_idx);
  // the new map
  std::unique_ptr<obvi_map, MapDeleter> fresh(new obvi_map());
  fresh->device = map->device; fresh->od = od; fresh->n = map->n;
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_mean), sizeof(double) * N));
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_cov), sizeof(double) * N * N));
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_x0), sizeof(double) * kMapGroupMaxRows));
  OBVI_HIP(hipMemcpyAsync(fresh->d_x0, map->d_x0, sizeof(double) * kMapGroupMaxRows, hipMemcpyDeviceToDevice, s));
  const MapUpdateDev u = window_update(h, map, k, 0, m, fresh.get());
  // the condition test reads the largest eigenvalue of Lambda = Cs_AA^-1, so the cut runs whole: factor, then Lambda and the power steps
  launch_map_factor(s, m, (int)nA, map->d_mean, map->d_cov, N);
  launch_map_condition_estimate(s, m, (int)nA, map->d_x0);
  launch_map_update(s, u);
  OBVI_HIP(hipGetLastError());
  double st[kMapStatusDoubles];
  h->d_mc_status.download(st, (size_t)kMapStatusDoubles, s);
  sync(h);   // the call's one wait: either map may go away from here on, and any stream may read the new one
  if (!window_cut_spd(st)) return fail(h, OBVI_ERR_NUMERICAL, what + ": the map's covariance of the window's objects is not SPD, or numerically singular");
  if (st[MS_NONFINITE] != 0.0) return fail(h, OBVI_ERR_NUMERICAL, what + ": a non-finite entry in the posterior or in the new map");
  *out = fresh.release();
  return OBVI_OK;
}

}  // namespace

extern "C" {

int obvi_map_get(const obvi_map* map, double* mean, double* cov) {
  if (!map) return OBVI_ERR_INVALID_ARGUMENT;
  const size_t rows = (size_t)(map->n * map->od);
  if (hipSetDevice(map->device) != hipSuccess) return OBVI_ERR_HIP;
  if (mean && hipMemcpy(mean, map->d_mean, sizeof(double) * rows, hipMemcpyDeviceToHost) != hipSuccess) return OBVI_ERR_HIP;
  if (cov && hipMemcpy(cov, map->d_cov, sizeof(double) * rows * rows, hipMemcpyDeviceToHost) != hipSuccess) return OBVI_ERR_HIP;
  return OBVI_OK;
}

int obvi_map_condition(obvi_ba_handle* h, const obvi_map* map, int64_t k, const uint32_t* map_idx, const double* post_mean, const double* post_cov, obvi_map** out) {
  if (out) *out = nullptr;
  if (!h || !map || !out || k < 1 || !map_idx || !post_mean || !post_cov) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_condition: bad arguments");
  { const int rc = check_window(h, map, k, map_idx, k * h->od, "map_condition"); if (rc != OBVI_OK) return rc; }
  const int64_t NA = k * h->od;
  for (int64_t i = 0; i < NA; ++i) if (!std::isfinite(post_mean[i])) return fail(h, OBVI_ERR_NUMERICAL, "map_condition: a posterior mean that is not finite");
  for (int64_t i = 0; i < NA * NA; ++i) if (!std::isfinite(post_cov[i])) return fail(h, OBVI_ERR_NUMERICAL, "map_condition: a posterior covariance entry that is not finite");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  h->d_mu_post.resize((size_t)(NA * NA + NA));
  h2d_async(h->d_mu_post.get(), post_cov, sizeof(double) * (size_t)(NA * NA), h->stream);
  h2d_async(h->d_mu_post.get() + NA * NA, post_mean, sizeof(double) * (size_t)NA, h->stream);
  return condition(h, map, k, map_idx, "map_condition", out);
  OBVI_API_END(h)
}

int obvi_map_condition_on_handle(obvi_ba_handle* h, const obvi_map* map, int64_t k, const uint32_t* obj_idx, const uint32_t* map_idx, obvi_map** out) {
  if (out) *out = nullptr;
  if (!h || !map || !out || k < 1 || !obj_idx || !map_idx) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_condition_on_handle: bad arguments");
  { const int rc = check_window(h, map, k, map_idx, k * h->od, "map_condition_on_handle"); if (rc != OBVI_OK) return rc; }
  { const int rc = check_session_objects(h, k, obj_idx, "map_condition_on_handle"); if (rc != OBVI_OK) return rc; }
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, "map_condition_on_handle: cameras not set");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  // the posterior: the joint covariance of the window's objects, all k x k pairs, and their current estimates -- laid out on the device
  WindowPosterior keep;   // alive until condition()'s wait
  { const int rc = posterior_from_handle(h, k, obj_idx, "map_condition_on_handle", keep); if (rc != OBVI_OK) return rc; }
  return condition(h, map, k, map_idx, "map_condition_on_handle", out);
  OBVI_API_END(h)
}

}  // extern "C"
