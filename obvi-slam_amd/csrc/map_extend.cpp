// map_extend.cpp -- include/obvi_map_extend.h: a device-resident map grown by a window's new objects, born from a posterior, or gathered down to some of its
// objects (map_kernels.hip).  The host checks every index, cuts the window's map objects as one group (map_window.h: the set-up map_update.cpp uses), launches
// into a freshly allocated, larger map, reads the cut's status record back and hands the new map out only when nothing was refused.
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

std::unique_ptr<obvi_map, MapDeleter> allocate_map(int device, int od, int64_t n) {
  std::unique_ptr<obvi_map, MapDeleter> fresh(new obvi_map());
  fresh->device = device; fresh->od = od; fresh->n = n;
  const int64_t rows = n * od;
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_mean), sizeof(double) * rows));
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_cov), sizeof(double) * rows * rows));
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_x0), sizeof(double) * kMapGroupMaxRows));
  return fresh;
}

// The extension, with the posterior over (A, B) in d_mu_post (covariance [N_A + N_B]^2, then mean) on the handle's stream.  One wait.
int extend(obvi_ba_handle* h, const obvi_map* map, int64_t k_old, const uint32_t* map_idx, int64_t k_new, const std::string& what, obvi_map** out) {
  const int od = h->od;
  const int64_t n = map ? map->n : 0, N = n * od, NA = k_old * od, NB = k_new * od, nA = map_group_slabs(NA);
  hipStream_t s = h->stream;
  const MapCutDev m = window_cut(h, k_old, map_idx);
  std::unique_ptr<obvi_map, MapDeleter> fresh = allocate_map(h->device, od, n + k_new);
  const std::vector<double> x0 = map ? std::vector<double>() : map_power_start();   // alive until the wait
  if (map) OBVI_HIP(hipMemcpyAsync(fresh->d_x0, map->d_x0, sizeof(double) * kMapGroupMaxRows, hipMemcpyDeviceToDevice, s));
  else h2d_async(fresh->d_x0, x0.data(), sizeof(double) * x0.size(), s);
  const MapUpdateDev u = window_update(h, map, k_old, k_new, m, fresh.get());
  if (k_old > 0) {
    launch_map_factor(s, m, (int)nA, map->d_mean, map->d_cov, N);
    launch_map_condition_estimate(s, m, (int)nA, map->d_x0);
  } else if (N > 0) {
    OBVI_HIP(hipMemsetAsync(fresh->d_cov, 0, sizeof(double) * (size_t)((N + NB) * (N + NB)), s));   // no product fills the cross blocks: they are zero
  }
  launch_map_extend(s, u);
  OBVI_HIP(hipGetLastError());
  double st[kMapStatusDoubles];
  h->d_mc_status.download(st, (size_t)kMapStatusDoubles, s);
  sync(h);   // the call's one wait: either map may go away from here on, and any stream may read the new one
  if (k_old > 0 && !window_cut_spd(st)) return fail(h, OBVI_ERR_NUMERICAL, what + ": the map's covariance of the window's objects is not SPD, or numerically singular");
  if (st[MS_NONFINITE] != 0.0) return fail(h, OBVI_ERR_NUMERICAL, what + ": a non-finite entry in the posterior or in the new map");
  *out = fresh.release();
  return OBVI_OK;
}

}  // namespace

extern "C" {

int obvi_map_extend(obvi_ba_handle* h, const obvi_map* map, int64_t k_old, const uint32_t* map_idx, int64_t k_new, const double* post_mean, const double* post_cov,
                    obvi_map** out) {
  if (out) *out = nullptr;
  if (!h || !out || !post_mean || !post_cov) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_extend: bad arguments");
  { const int rc = check_extension(h, map, k_old, map_idx, k_new, "map_extend"); if (rc != OBVI_OK) return rc; }
  const int64_t NP = (k_old + k_new) * h->od;
  for (int64_t i = 0; i < NP; ++i) if (!std::isfinite(post_mean[i])) return fail(h, OBVI_ERR_NUMERICAL, "map_extend: a posterior mean that is not finite");
  for (int64_t i = 0; i < NP * NP; ++i) if (!std::isfinite(post_cov[i])) return fail(h, OBVI_ERR_NUMERICAL, "map_extend: a posterior covariance entry that is not finite");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  h->d_mu_post.resize((size_t)(NP * NP + NP));
  h2d_async(h->d_mu_post.get(), post_cov, sizeof(double) * (size_t)(NP * NP), h->stream);
  h2d_async(h->d_mu_post.get() + NP * NP, post_mean, sizeof(double) * (size_t)NP, h->stream);
  return extend(h, map, k_old, map_idx, k_new, "map_extend", out);
  OBVI_API_END(h)
}

int obvi_map_extend_on_handle(obvi_ba_handle* h, const obvi_map* map, int64_t k_old, const uint32_t* obj_idx_old, const uint32_t* map_idx, int64_t k_new,
                              const uint32_t* obj_idx_new, obvi_map** out) {
  if (out) *out = nullptr;
  if (!h || !out || !obj_idx_new || (k_old > 0 && !obj_idx_old)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_extend_on_handle: bad arguments");
  { const int rc = check_extension(h, map, k_old, map_idx, k_new, "map_extend_on_handle"); if (rc != OBVI_OK) return rc; }
  const int64_t k = k_old + k_new;
  std::vector<uint32_t> obj((size_t)k);   // (A, B): the order of the posterior; alive until extend()'s wait
  std::copy(obj_idx_old, obj_idx_old + k_old, obj.begin());
  std::copy(obj_idx_new, obj_idx_new + k_new, obj.begin() + k_old);
  { const int rc = check_session_objects(h, k, obj.data(), "map_extend_on_handle"); if (rc != OBVI_OK) return rc; }
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, "map_extend_on_handle: cameras not set");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  WindowPosterior keep;   // alive until extend()'s wait
  { const int rc = posterior_from_handle(h, k, obj.data(), "map_extend_on_handle", keep); if (rc != OBVI_OK) return rc; }
  return extend(h, map, k_old, map_idx, k_new, "map_extend_on_handle", out);
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
  OBVI_HIP(hipMemcpyAsync(fresh->d_x0, map->d_x0, sizeof(double) * kMapGroupMaxRows, hipMemcpyDeviceToDevice, s));
  h->d_mc_map_idx.upload(map_idx, (size_t)k, s);
  launch_map_select(s, h->d_mc_map_idx.get(), (int32_t)k, map->od, map->d_mean, map->d_cov, map->n * map->od, fresh->d_mean, fresh->d_cov);
  OBVI_HIP(hipGetLastError());
  sync(h);   // the call's one wait
  *out = fresh.release();
  return OBVI_OK;
  OBVI_API_END(h)
}

}  // extern "C"
