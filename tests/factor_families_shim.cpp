// Host build of the factor-family table (obvi-slam_amd/csrc/ba_handle.h: families(), its evaluate layout, reduce_small_families()) on a default-constructed
// handle whose host mirrors are filled here, so that the CPU test-suite can hold the bookkeeping against numpy without a GPU.  No HIP call is made: the
// handle's device buffers stay empty and free nothing.  Test infrastructure only.
#include "../obvi-slam_amd/csrc/ba_handle.h"

namespace {
void put(std::vector<uint32_t>& v, const uint32_t* p, int64_t n) { v.assign(p, p + n); }
void put(std::vector<uint8_t>& v, const uint8_t* p, int64_t n) { v.assign(p, p + n); }
}  // namespace

extern "C" {
obvi_ba_handle* ff_create(int32_t od) { obvi_ba_handle* h = new obvi_ba_handle(); h->od = od; return h; }
void ff_destroy(obvi_ba_handle* h) { delete h; }
void ff_set_blocks(obvi_ba_handle* h, int64_t P, int64_t L, int64_t O, const uint8_t* pose_const, const uint8_t* point_const, const uint8_t* object_const) {
  h->P = P; h->L = L; h->O = O;
  put(h->h_pose_const, pose_const, P); put(h->h_point_const, point_const, L); put(h->h_object_const, object_const, O);
}
// what the obvi_ba_set_* calls leave on the host for each family: count, index arrays, mask, index maxima
void ff_set_reproj(obvi_ba_handle* h, int64_t n, const uint32_t* pose, const uint32_t* point, const uint8_t* active) {
  h->n_rp = n; put(h->h_rp_pose, pose, n); put(h->h_rp_point, point, n); put(h->h_rp_active, active, n);
  h->max_rp_pose = max_index(pose, n); h->max_rp_point = max_index(point, n); h->max_rp_cam = n > 0 ? 0 : -1;
}
void ff_set_bbox(obvi_ba_handle* h, int64_t n, const uint32_t* obj, const uint32_t* pose, const uint8_t* active) {
  h->n_bb = n; put(h->h_bb_obj, obj, n); put(h->h_bb_pose, pose, n); put(h->h_bb_active, active, n);
  h->max_bb_obj = max_index(obj, n); h->max_bb_pose = max_index(pose, n); h->max_bb_cam = n > 0 ? 1 : -1;   // (every box from camera 1)
}
void ff_set_shape(obvi_ba_handle* h, int64_t n, const uint32_t* obj, const uint8_t* active) {
  h->n_sp = n; put(h->h_sp_obj, obj, n); put(h->h_sp_active, active, n); h->max_sp_obj = max_index(obj, n);
}
void ff_set_ltm(obvi_ba_handle* h, int64_t n, const uint32_t* obj, const uint8_t* active) {
  h->n_lt = n; put(h->h_lt_obj, obj, n); put(h->h_lt_active, active, n); h->max_lt_obj = max_index(obj, n);
}
void ff_set_relpose(obvi_ba_handle* h, int64_t n, const uint32_t* a, const uint32_t* b, const uint8_t* active) {
  h->n_rl = n; put(h->h_rl_a, a, n); put(h->h_rl_b, b, n); put(h->h_rl_active, active, n); h->max_rl_pose = std::max(max_index(a, n), max_index(b, n));
}
void ff_set_pairs(obvi_ba_handle* h, int64_t n, const uint32_t* a, const uint32_t* b, const uint8_t* active) {
  h->n_mp = n; put(h->h_mp_a, a, n); put(h->h_mp_b, b, n); put(h->h_mp_active, active, n); h->max_mp_obj = std::max(max_index(a, n), max_index(b, n));
}
void ff_set_groups(obvi_ba_handle* h, int64_t n, const int64_t* ptr, const uint32_t* obj, const uint8_t* active) {
  h->n_mg = n; h->h_mg_ptr.assign(ptr, ptr + n + 1); put(h->h_mg_obj, obj, ptr[n]); put(h->h_mg_active, active, n);
  h->mg_rows = h->od * ptr[n]; h->max_mg_obj = max_index(obj, ptr[n]);
}
void ff_set_shared(obvi_ba_handle* h, const uint8_t* flags) { if (flags) put(h->h_is_shared, flags, h->O); else h->h_is_shared.clear(); }

// out: type, count, residual rows, rows per factor, d0, d1, the four index maxima (pose, point, object, camera); the family's place in evaluate order, or -1 for an unknown type
int32_t ff_family(const obvi_ba_handle* h, int32_t type, int64_t* out) {
  const FamilyTable fams = families(h);
  const FactorFamily* f = fams.find(type);
  if (!f) return -1;
  const int64_t v[10] = {f->type, f->n, f->rows, f->m, f->d0, f->d1, f->max_pose, f->max_point, f->max_obj, f->max_cam};
  std::copy(v, v + 10, out);
  return fams.index(f);
}
// slot, row: [FAM_COUNT + 1] first block norm / first residual row of every family, then the totals
void ff_layout(const obvi_ba_handle* h, int64_t* slot, int64_t* row) {
  const EvalLayout l = families(h).layout();
  std::copy(l.slot, l.slot + FAM_COUNT + 1, slot); std::copy(l.row, l.row + FAM_COUNT + 1, row);
}
// The reduced program of the small families the way its two callers run it.  as_replan = 0: the full plan's fresh vectors; 1: the mask-only re-plan's
// scratch, kept in the handle between calls.  pose_used [P], obj_used [O] out; returns the residual count.
int64_t ff_reduce(obvi_ba_handle* h, int32_t as_replan, uint8_t* pose_used, uint8_t* obj_used) {
  std::vector<uint8_t> fresh_pose, fresh_obj;
  std::vector<uint8_t>& pu = as_replan ? h->scr_pose_used : fresh_pose;
  std::vector<uint8_t>& ou = as_replan ? h->scr_obj_used : fresh_obj;
  pu.assign((size_t)h->P, 0); ou.assign((size_t)h->O, 0);
  const int64_t nres = reduce_small_families(h, pu.data(), ou.data());
  std::copy(pu.begin(), pu.end(), pose_used); std::copy(ou.begin(), ou.end(), obj_used);
  return nres;
}
}
