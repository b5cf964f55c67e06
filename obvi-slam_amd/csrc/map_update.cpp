// map_update.cpp -- include/obvi_map_update.h: a device-resident map read back, and conditioned on the posterior of a window's objects (map_kernels.hip).
// The host checks every index, cuts the window's objects from the map as one group (the stages of obvi_map_set_group_priors_from_map, in the handle's scratch
// buffers of that call: the handle's own groups are not touched), launches the update into a freshly allocated map, reads the cut's status record back and hands
// the new map out only when nothing was refused.
#include "ba_handle.h"
#include "../../include/obvi_map_update.h"

#include <memory>

namespace {

struct MapDeleter { void operator()(obvi_map* m) const { obvi_map_destroy(m); } };

bool twice(const uint32_t* idx, int64_t k) {
  std::vector<uint32_t> sorted(idx, idx + k);
  std::sort(sorted.begin(), sorted.end());
  return std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
}

// what both entries refuse about the map and the window's map objects, before anything is launched or allocated
int check_window(obvi_ba_handle* h, const obvi_map* map, int64_t k, const uint32_t* map_idx, const std::string& what) {
  if (map->device != h->device) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": the map lives on another device than the handle");
  if (map->od != h->od) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": the map's object block size is not the handle's");
  if (k > OBVI_MAP_GROUP_MAX_ROWS / h->od) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": a window of more than OBVI_MAP_GROUP_MAX_ROWS rows");
  for (int64_t i = 0; i < k; ++i) if ((int64_t)map_idx[i] >= map->n) return fail(h, OBVI_ERR_OUT_OF_RANGE, what + ": map index out of range");
  if (twice(map_idx, k)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": a map object twice");
  return OBVI_OK;
}

// The update, with the posterior in d_mu_post (covariance [N_A][N_A], then mean [N_A]) on the handle's stream.  One wait.
int condition(obvi_ba_handle* h, const obvi_map* map, int64_t k, const uint32_t* map_idx, const std::string& what, obvi_map** out) {
  const int od = h->od;
  const int64_t NA = k * od, N = map->n * od, nA = map_group_slabs(NA), nN = map_group_slabs(N), ld = (NA + 1) & ~(int64_t)1, tile = (int64_t)kTile * kTile;
  hipStream_t s = h->stream;
  // the window's objects as one group of a cut (MapCutDev, ba_device.h)
  const std::vector<MapCutGroup> cut{MapCutGroup{(int32_t)NA, (int32_t)nA, (int32_t)ld, 0, 0, 0, 0, 0, 0}};
  h->d_mc_groups.upload(cut, s); h->d_mc_map_idx.upload(map_idx, (size_t)k, s);
  h->d_mgn_mean.resize((size_t)NA); h->d_mgn_Lambda.resize((size_t)(NA * ld)); h->d_mgn_W.resize((size_t)(NA * NA));
  h->d_mc_A.resize((size_t)(nA * nA * tile)); h->d_mc_Wt.resize((size_t)(nA * nA * tile)); h->d_mc_Li.resize((size_t)(nA * tile));
  h->d_mc_Csym.resize((size_t)(NA * ld)); h->d_mc_x.resize((size_t)(4 * NA)); h->d_mc_partial.resize((size_t)2 * (kMapGroupMaxRows / 16));
  h->d_mc_status.resize((size_t)kMapStatusDoubles);
  h->d_mgn_W.zero(s); h->d_mgn_Lambda.zero(s); h->d_mc_status.zero(s);
  MapCutDev m;
  m.n = 1; m.od = od; m.rows = NA; m.groups = h->d_mc_groups.get(); m.map_idx = h->d_mc_map_idx.get();
  m.A = h->d_mc_A.get(); m.Li = h->d_mc_Li.get(); m.Wt = h->d_mc_Wt.get(); m.Csym = h->d_mc_Csym.get();
  m.mean = h->d_mgn_mean.get(); m.W = h->d_mgn_W.get(); m.Lambda = h->d_mgn_Lambda.get();
  m.x = h->d_mc_x.get(); m.partial = h->d_mc_partial.get(); m.status = h->d_mc_status.get();
  // the new map
  std::unique_ptr<obvi_map, MapDeleter> fresh(new obvi_map());
  fresh->device = map->device; fresh->od = od; fresh->n = map->n;
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_mean), sizeof(double) * N));
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_cov), sizeof(double) * N * N));
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_x0), sizeof(double) * kMapGroupMaxRows));
  OBVI_HIP(hipMemcpyAsync(fresh->d_x0, map->d_x0, sizeof(double) * kMapGroupMaxRows, hipMemcpyDeviceToDevice, s));
  h->d_mu_tiles.resize((size_t)((4 * nA * nA + 3 * nN * nA) * tile + kTile * nA));
  MapUpdateDev u;
  u.od = od; u.N = (int32_t)N; u.NA = (int32_t)NA; u.nN = (int32_t)nN; u.nA = (int32_t)nA;
  u.map_idx = h->d_mc_map_idx.get(); u.map_mean = map->d_mean; u.map_cov = map->d_cov;
  u.P = h->d_mu_post.get(); u.pm = h->d_mu_post.get() + NA * NA;
  u.Wt = m.Wt; u.W = m.W; u.mean_A = m.mean;
  double* t = h->d_mu_tiles.get();
  u.Wn = t; u.Ps = u.Wn + nA * nA * tile; u.U = u.Ps + nA * nA * tile; u.M = u.U + nA * nA * tile;
  u.G = u.M + nA * nA * tile; u.Y = u.G + nN * nA * tile; u.Z = u.Y + nN * nA * tile; u.v = u.Z + nN * nA * tile;
  u.out_mean = fresh->d_mean; u.out_cov = fresh->d_cov; u.status = m.status;
  // the condition test reads the largest eigenvalue of Lambda = Cs_AA^-1, so the cut runs whole: factor, then Lambda and the power steps
  launch_map_factor(s, m, (int)nA, map->d_mean, map->d_cov, N);
  launch_map_condition_estimate(s, m, (int)nA, map->d_x0);
  launch_map_update(s, u);
  OBVI_HIP(hipGetLastError());
  double st[kMapStatusDoubles];
  h->d_mc_status.download(st, (size_t)kMapStatusDoubles, s);
  sync(h);   // the call's one wait: either map may go away from here on, and any stream may read the new one
  const bool spd = st[MS_BAD] == 0.0 && st[MS_PIV_MIN] * st[MS_PIV_MIN] > 1e-13 * st[MS_PIV_MAX] * st[MS_PIV_MAX] && st[MS_EV_C] * st[MS_EV_LAMBDA] <= 1e13;
  if (!spd) return fail(h, OBVI_ERR_NUMERICAL, what + ": the map's covariance of the window's objects is not SPD, or numerically singular");
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
  { const int rc = check_window(h, map, k, map_idx, "map_condition"); if (rc != OBVI_OK) return rc; }
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
  { const int rc = check_window(h, map, k, map_idx, "map_condition_on_handle"); if (rc != OBVI_OK) return rc; }
  for (int64_t i = 0; i < k; ++i) if ((int64_t)obj_idx[i] >= h->O) return fail(h, OBVI_ERR_OUT_OF_RANGE, "map_condition_on_handle: object index out of range");
  if (twice(obj_idx, k)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_condition_on_handle: a session object twice");
  for (int64_t i = 0; i < k; ++i) if (h->h_object_const[obj_idx[i]]) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_condition_on_handle: a constant object has no posterior");
  // the flags, not the plan's list: a handle that has not planned yet exchanges as soon as it does (validate_indices refuses group priors by the same test)
  if (h->allreduce != nullptr && std::any_of(h->h_is_shared.begin(), h->h_is_shared.end(), [](uint8_t v) { return v != 0; })) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_condition_on_handle: the handle exchanges shared objects");
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, "map_condition_on_handle: cameras not set");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  prepare(h);
  for (int64_t i = 0; i < k; ++i) if (h->h_obj_vid[obj_idx[i]] < 0) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_condition_on_handle: an object that no active factor touches has no posterior");
  // the posterior: the joint covariance of the window's objects, all k x k pairs, and their current estimates -- laid out on the device
  std::vector<uint32_t> pa((size_t)(k * k)), pb((size_t)(k * k));
  for (int64_t a = 0; a < k; ++a) for (int64_t b = 0; b < k; ++b) { pa[(size_t)(a * k + b)] = obj_idx[a]; pb[(size_t)(a * k + b)] = obj_idx[b]; }
  int64_t ldt = 0;
  CovTables tables;   // alive until condition()'s wait
  { const int rc = object_cov_forward(h, k * k, "map_condition_on_handle", &ldt, tables); if (rc != OBVI_OK) return rc; }
  if (ldt == 0) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_condition_on_handle: the handle has no variable objects");
  object_cov_pair_blocks(h, k * k, pa.data(), pb.data(), ldt, tables);
  const int64_t NA = k * h->od;
  h->d_mu_obj.upload(obj_idx, (size_t)k, h->stream);
  h->d_mu_post.resize((size_t)(NA * NA + NA));
  launch_map_posterior_layout(h->stream, h->d_cov_out.get(), h->d_obj.get(), h->d_mu_obj.get(), (int32_t)k, h->od, h->d_mu_post.get(), h->d_mu_post.get() + NA * NA);
  return condition(h, map, k, map_idx, "map_condition_on_handle", out);
  OBVI_API_END(h)
}

}  // extern "C"
