// map_resident.cpp -- include/obvi_map_resident.h: a map kept on the device, and group priors cut from it and factored there (map_kernels.hip).
// The host checks every index, lays the groups out as obvi_map_set_group_priors does (upload.cpp), launches, reads one status record per group back, and swaps
// the buffers the call built into the handle only when no group was refused.
#include "map_window.h"
#include "../../include/obvi_map_resident.h"

extern "C" {

int obvi_map_create(int32_t device_id, int32_t object_block_size, int64_t n_objects, const double* mean, const double* cov, obvi_map** out) {
  if (!out) return OBVI_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  if (!mean || !cov || n_objects < 1 || (object_block_size != 0 && object_block_size != 7 && object_block_size != 9)) return OBVI_ERR_INVALID_ARGUMENT;
  const int od = object_block_size == 9 ? 9 : 7;
  if (n_objects > kMapMaxRows / od) return OBVI_ERR_INVALID_ARGUMENT;
  const int64_t rows = n_objects * od;
  for (int64_t k = 0; k < rows; ++k) if (!std::isfinite(mean[k])) return OBVI_ERR_NUMERICAL;
  for (int64_t k = 0; k < rows * rows; ++k) if (!std::isfinite(cov[k])) return OBVI_ERR_NUMERICAL;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device_id < 0 || device_id >= count) return OBVI_ERR_NO_DEVICE;
  try {
    const std::vector<double> x0 = map_power_start();
    OBVI_HIP(hipSetDevice(device_id));
    std::unique_ptr<obvi_map, MapDeleter> m = allocate_map(device_id, od, n_objects);
    OBVI_HIP(hipMemcpy(m->d_mean, mean, sizeof(double) * rows, hipMemcpyHostToDevice));
    OBVI_HIP(hipMemcpy(m->d_cov, cov, sizeof(double) * rows * rows, hipMemcpyHostToDevice));
    OBVI_HIP(hipMemcpy(m->d_x0, x0.data(), sizeof(double) * x0.size(), hipMemcpyHostToDevice));
    OBVI_HIP(hipDeviceSynchronize());   // the copies have landed: any stream of any thread may read the map from here on
    *out = m.release();
    return OBVI_OK;
  } catch (const HipError&) {   // no handle to keep the words: the code alone, and whatever was allocated is freed
    return OBVI_ERR_HIP;
  } catch (const std::bad_alloc&) {
    return OBVI_ERR_HIP;
  }
}

void obvi_map_destroy(obvi_map* map) {
  if (!map) return;
  for (double* p : {map->d_mean, map->d_cov, map->d_x0}) if (p) (void)hipFree(p);
  delete map;
}

int64_t obvi_map_num_objects(const obvi_map* map) { return map ? map->n : -1; }

int obvi_map_set_group_priors_from_map(obvi_ba_handle* h, const obvi_map* map, int64_t n_groups, const int64_t* group_ptr, const uint32_t* obj_idx,
                                       const uint32_t* map_idx, double huber) {
  if (!h || !map || n_groups < 0 || (n_groups > 0 && (!group_ptr || !obj_idx || !map_idx))) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_set_group_priors_from_map: bad arguments");
  if (map->device != h->device) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_set_group_priors_from_map: the map lives on another device than the handle");
  if (map->od != h->od) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_set_group_priors_from_map: the map's object block size is not the handle's");
  if (n_groups == 0) return obvi_map_set_group_priors(h, 0, nullptr, nullptr, nullptr, nullptr, huber);
  OBVI_API_BEGIN
  const int od = h->od;
  const int64_t n = n_groups;
  // what obvi_map_set_group_priors refuses, in its order and with its codes (upload.cpp)
  if (group_ptr[0] != 0) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_set_group_priors_from_map: group_ptr does not start at 0");
  for (int64_t g = 0; g < n; ++g) {
    if (group_ptr[g + 1] < group_ptr[g]) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_set_group_priors_from_map: group_ptr decreases");
    if (group_ptr[g + 1] == group_ptr[g]) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_set_group_priors_from_map: an empty group");
    if ((group_ptr[g + 1] - group_ptr[g]) * od > OBVI_MAP_GROUP_MAX_ROWS) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_set_group_priors_from_map: a group of more than OBVI_MAP_GROUP_MAX_ROWS rows");
  }
  const int64_t members = group_ptr[n];
  for (int64_t k = 0; k < members; ++k) if (obj_idx[k] >= h->O) return fail(h, OBVI_ERR_OUT_OF_RANGE, "map_set_group_priors_from_map: index out of range");
  {
    std::vector<uint32_t> sorted(obj_idx, obj_idx + members);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_set_group_priors_from_map: an object twice (in one group or in two)");
  }
  // ... and the map's side: no index reaches a kernel unchecked
  for (int64_t k = 0; k < members; ++k) if ((int64_t)map_idx[k] >= map->n) return fail(h, OBVI_ERR_OUT_OF_RANGE, "map_set_group_priors_from_map: map index out of range");
  {
    std::vector<uint32_t> sorted(map_idx, map_idx + members);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_set_group_priors_from_map: a map object twice");
  }
  // layout: MapGroupDev as upload.cpp lays it out, and the tile workspaces of the call (MapCutDev, ba_device.h)
  std::vector<int64_t> lam_off((size_t)n + 1, 0), w_off((size_t)n + 1, 0);
  std::vector<int32_t> slab_ptr((size_t)n + 1, 0), slab_grp, tile_ptr((size_t)n + 1, 0), tile_grp, tile_ij;
  std::vector<MapCutGroup> cut((size_t)n);
  int64_t tiles = 0, diags = 0;
  int nt_max = 0;
  for (int64_t g = 0; g < n; ++g) {
    const int64_t N = (group_ptr[g + 1] - group_ptr[g]) * od, ld = (N + 1) & ~(int64_t)1, nsl = map_group_slabs(N);
    lam_off[g + 1] = lam_off[g] + N * ld; w_off[g + 1] = w_off[g] + N * N;
    for (int64_t sl = 0; sl < nsl; ++sl) slab_grp.push_back((int32_t)g);
    for (int64_t ti = 0; ti < nsl; ++ti) for (int64_t tj = 0; tj <= ti; ++tj) { tile_grp.push_back((int32_t)g); tile_ij.push_back((int32_t)(ti << 16 | tj)); }
    slab_ptr[g + 1] = (int32_t)slab_grp.size(); tile_ptr[g + 1] = (int32_t)tile_grp.size();
    cut[g] = MapCutGroup{(int32_t)N, (int32_t)nsl, (int32_t)ld, 0, tiles, diags, group_ptr[g], lam_off[g], w_off[g]};
    tiles += nsl * nsl; diags += nsl;
    nt_max = std::max(nt_max, (int)nsl);
  }
  const int64_t rows = members * od;
  OBVI_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  std::vector<int64_t> ptr(group_ptr, group_ptr + n + 1);
  std::vector<uint32_t> obj(obj_idx, obj_idx + members);
  std::vector<uint8_t> active((size_t)n, 1);
  h->d_mgn_ptr.upload(ptr, s); h->d_mgn_obj.upload(obj, s); h->d_mgn_active.upload(active, s);
  h->d_mgn_lam_off.upload(lam_off, s); h->d_mgn_w_off.upload(w_off, s);
  h->d_mgn_slab_ptr.upload(slab_ptr, s); h->d_mgn_slab_grp.upload(slab_grp, s); h->d_mgn_tile_ptr.upload(tile_ptr, s); h->d_mgn_tile_grp.upload(tile_grp, s); h->d_mgn_tile_ij.upload(tile_ij, s);
  h->d_mc_groups.upload(cut, s); h->d_mc_map_idx.upload(map_idx, (size_t)members, s);
  h->d_mgn_mean.resize((size_t)rows); h->d_mgn_Lambda.resize((size_t)lam_off[n]); h->d_mgn_W.resize((size_t)w_off[n]);
  h->d_mc_A.resize((size_t)tiles * kTile * kTile); h->d_mc_Wt.resize((size_t)tiles * kTile * kTile); h->d_mc_Li.resize((size_t)diags * kTile * kTile);
  h->d_mc_Csym.resize((size_t)lam_off[n]); h->d_mc_x.resize((size_t)(4 * rows)); h->d_mc_partial.resize((size_t)n * 2 * (kMapGroupMaxRows / 16));
  h->d_mc_status.resize((size_t)n * kMapStatusDoubles);
  h->d_mgn_W.zero(s); h->d_mgn_Lambda.zero(s);   // W above the diagonal, the padding of Lambda's rows
  MapCutDev m;
  m.n = n; m.od = od; m.rows = rows; m.groups = h->d_mc_groups.get(); m.map_idx = h->d_mc_map_idx.get();
  m.A = h->d_mc_A.get(); m.Li = h->d_mc_Li.get(); m.Wt = h->d_mc_Wt.get(); m.Csym = h->d_mc_Csym.get();
  m.mean = h->d_mgn_mean.get(); m.W = h->d_mgn_W.get(); m.Lambda = h->d_mgn_Lambda.get();
  m.x = h->d_mc_x.get(); m.partial = h->d_mc_partial.get(); m.status = h->d_mc_status.get();
  launch_map_cut(s, m, nt_max, map->d_mean, map->d_cov, map->n * od, map->d_x0);
  OBVI_HIP(hipGetLastError());
  std::vector<double> status((size_t)n * kMapStatusDoubles);
  h->d_mc_status.download(status.data(), status.size(), s);
  sync(h);   // the call's one wait: the map may go away from here on
  for (int64_t g = 0; g < n; ++g)
    if (!window_cut_spd(&status[(size_t)g * kMapStatusDoubles])) return fail(h, OBVI_ERR_NUMERICAL, "map_set_group_priors_from_map: covariance not SPD, or numerically singular");
  // accepted: the call's buffers become the handle's
  h->d_mg_ptr.swap(h->d_mgn_ptr); h->d_mg_obj.swap(h->d_mgn_obj); h->d_mg_active.swap(h->d_mgn_active); h->d_mg_mean.swap(h->d_mgn_mean);
  h->d_mg_lam_off.swap(h->d_mgn_lam_off); h->d_mg_w_off.swap(h->d_mgn_w_off); h->d_mg_Lambda.swap(h->d_mgn_Lambda); h->d_mg_W.swap(h->d_mgn_W);
  h->d_mg_slab_ptr.swap(h->d_mgn_slab_ptr); h->d_mg_slab_grp.swap(h->d_mgn_slab_grp); h->d_mg_tile_ptr.swap(h->d_mgn_tile_ptr); h->d_mg_tile_grp.swap(h->d_mgn_tile_grp);
  h->d_mg_tile_ij.swap(h->d_mgn_tile_ij);
  h->n_mg = n; h->mg_huber = huber; h->max_mg_obj = max_index(obj_idx, members); h->mg_rows = rows;
  h->mg_slabs = (int64_t)slab_grp.size(); h->mg_tiles = (int64_t)tile_grp.size();
  h->h_mg_ptr.swap(ptr); h->h_mg_obj.swap(obj); h->h_mg_active.swap(active);
  h->d_mg_y.resize((size_t)h->mg_rows); h->d_mg_partial.resize((size_t)h->mg_slabs);
  h->dirty = true;
  return OBVI_OK;
  OBVI_API_END(h)
}

}  // extern "C"
