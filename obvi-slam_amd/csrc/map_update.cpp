// map_update.cpp -- include/obvi_map_update.h: a device-resident map read back, and conditioned on the posterior of a window's objects.  The condition is the
// extension by no new object: both entries check their arguments, put the posterior on the device and call fold_window (map_window.h) with k_new = 0.
#include "map_window.h"
#include "../../include/obvi_map_update.h"

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
  OBVI_API_BEGIN
  { const int rc = upload_posterior(h, k * h->od, post_mean, post_cov, "map_condition"); if (rc != OBVI_OK) return rc; }
  return fold_window(h, map, k, map_idx, 0, "map_condition", out);
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
  WindowPosterior keep;   // alive until fold_window's wait
  { const int rc = posterior_from_handle(h, k, obj_idx, "map_condition_on_handle", keep); if (rc != OBVI_OK) return rc; }
  return fold_window(h, map, k, map_idx, 0, "map_condition_on_handle", out);
  OBVI_API_END(h)
}

}  // extern "C"
