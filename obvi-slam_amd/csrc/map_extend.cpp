// map_extend.cpp -- include/obvi_map_extend.h: a device-resident map grown by a window's new objects, born from a posterior, or gathered down to some of its
// objects (map_kernels.hip).  The extend entries check their arguments, put the posterior on the device and call fold_window (map_window.h), which the
// condition entries share; the gather copies into a freshly allocated, smaller map.
#include "map_window.h"
#include "../../include/obvi_map_extend.h"

namespace {

// what both extend entries refuse about the sizes and the map, before anything is launched or allocated
int check_extension(obvi_ba_handle* h, const obvi_map* map, int64_t k_old, const uint32_t* map_idx, int64_t k_new, const std::string& what) {
  if (k_new < 1) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": no new object (a window with nothing new conditions the map)");
  if (k_old < 0 || (k_old > 0 && (!map || !map_idx))) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": bad arguments");
  const int64_t max_k = OBVI_MAP_GROUP_MAX_ROWS / h->od;
  if (k_old > max_k || k_new > max_k || k_old + k_new > max_k) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": a window of more than OBVI_MAP_GROUP_MAX_ROWS rows");
  if (map) { const int rc = check_window(h, map, k_old, map_idx, (k_old + k_new) * h->od, what); if (rc != OBVI_OK) return rc; }
  if ((map ? map->n : 0) + k_new > kMapMaxRows / h->od) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": the grown map's covariance would exceed 1 GiB");
  return OBVI_OK;
}

}  // namespace

extern "C" {

int obvi_map_extend(obvi_ba_handle* h, const obvi_map* map, int64_t k_old, const uint32_t* map_idx, int64_t k_new, const double* post_mean, const double* post_cov,
                    obvi_map** out) {
  if (out) *out = nullptr;
  if (!h || !out || !post_mean || !post_cov) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_extend: bad arguments");
  { const int rc = check_extension(h, map, k_old, map_idx, k_new, "map_extend"); if (rc != OBVI_OK) return rc; }
  OBVI_API_BEGIN
  { const int rc = upload_posterior(h, (k_old + k_new) * h->od, post_mean, post_cov, "map_extend"); if (rc != OBVI_OK) return rc; }
  return fold_window(h, map, k_old, map_idx, k_new, "map_extend", out);
  OBVI_API_END(h)
}

int obvi_map_extend_on_handle(obvi_ba_handle* h, const obvi_map* map, int64_t k_old, const uint32_t* obj_idx_old, const uint32_t* map_idx, int64_t k_new,
                              const uint32_t* obj_idx_new, obvi_map** out) {
  if (out) *out = nullptr;
  if (!h || !out || !obj_idx_new || (k_old > 0 && !obj_idx_old)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_extend_on_handle: bad arguments");
  { const int rc = check_extension(h, map, k_old, map_idx, k_new, "map_extend_on_handle"); if (rc != OBVI_OK) return rc; }
  const int64_t k = k_old + k_new;
  std::vector<uint32_t> obj((size_t)k);   // (A, B): the order of the posterior; alive until fold_window's wait
  std::copy(obj_idx_old, obj_idx_old + k_old, obj.begin());
  std::copy(obj_idx_new, obj_idx_new + k_new, obj.begin() + k_old);
  { const int rc = check_session_objects(h, k, obj.data(), "map_extend_on_handle"); if (rc != OBVI_OK) return rc; }
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, "map_extend_on_handle: cameras not set");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  WindowPosterior keep;   // alive until fold_window's wait
  { const int rc = posterior_from_handle(h, k, obj.data(), "map_extend_on_handle", keep); if (rc != OBVI_OK) return rc; }
  return fold_window(h, map, k_old, map_idx, k_new, "map_extend_on_handle", out);
  OBVI_API_END(h)
}

int obvi_map_select(obvi_ba_handle* h, const obvi_map* map, int64_t k, const uint32_t* map_idx, obvi_map** out) {
  if (out) *out = nullptr;
  if (!h || !map || !out || k < 1 || !map_idx) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_select: bad arguments");
  if (k > map->n) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_select: more objects than the map holds");
  { const int rc = check_window(h, map, k, map_idx, 0, "map_select"); if (rc != OBVI_OK) return rc; }
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  std::unique_ptr<obvi_map, MapDeleter> fresh = allocate_map(map->device, map->od, k);
  inherit_power_start(fresh.get(), map, s);
  h->d_mc_map_idx.upload(map_idx, (size_t)k, s);
  launch_map_select(s, h->d_mc_map_idx.get(), (int32_t)k, map->od, map->d_mean, map->d_cov, map->n * map->od, fresh->d_mean, fresh->d_cov);
  OBVI_HIP(hipGetLastError());
  sync(h);   // the call's one wait
  *out = fresh.release();
  return OBVI_OK;
  OBVI_API_END(h)
}

}  // extern "C"
