// abi.cpp -- lifetime of a handle, evaluate, debug and profiling hooks, covariance extraction, outlier selection, state read-back, multi-GPU switches  (include/obvi_ba.h; shared state and helpers: ba_handle.h)
//
// One handle == one GPU == one HIP stream pair.  There is no CPU compute path in this library: without a HIP device obvi_ba_create fails with
// OBVI_ERR_NO_DEVICE.
#include "ba_handle.h"
#include "../../include/obvi_map_shared.h"

namespace obvi {
hipStream_t handle_stream(obvi_ba_handle* h) { return h->stream; }
int handle_device(const obvi_ba_handle* h) { return h->device; }
int handle_fail(obvi_ba_handle* h, int code, const char* msg) { return fail(h, code, msg); }
void make_dev_cam(const double* K4, const double* ext7, DevCam* out) { make_cam(K4, ext7, out); }
}  // namespace obvi

namespace obvi_lib {

// The only reader of the library's tuning knobs (ba_handle.h); obvi_ba_create calls it once per handle.
Knobs read_knobs() {
  Knobs k;
  auto set_int = [](const char* name, int& field) { if (const char* v = std::getenv(name)) field = std::atoi(v); };
  auto set_i64 = [](const char* name, int64_t& field) { if (const char* v = std::getenv(name)) field = std::atoll(v); };
  auto set_flag = [](const char* name, bool& field) { if (const char* v = std::getenv(name)) field = std::atoi(v) != 0; };
  set_int("OBVI_ND_G", k.nd_g);
  set_int("OBVI_ND_LEAF", k.nd_leaf);
  set_flag("OBVI_ND_BALANCE", k.nd_balance);
  set_flag("OBVI_TAIL_SPATIAL", k.tail_spatial);
  set_int("OBVI_PAIR_BITMAP_MAX", k.pair_bitmap_max);
  set_int("OBVI_SCHUR_WGS", k.schur_wgs);
  set_i64("OBVI_SCHUR_WIDE_BELOW", k.schur_wide_below);
  set_flag("OBVI_PLAN_SLOTS_ON_HOST", k.slots_on_host);
  set_int("OBVI_UPD_CHUNK", k.upd_chunk); k.upd_chunk = std::max(1, k.upd_chunk);
  set_int("OBVI_SLICE_MAX", k.slice_max);
  set_int("OBVI_PRE_MAX", k.pre_max); k.pre_max = std::max(0, k.pre_max);
  set_flag("OBVI_CHOL_XCD", k.chol_xcd);
  if (const char* v = std::getenv("OBVI_BACKWARD_LEVELS")) k.backward_levels = std::max(1, std::min(8, std::atoi(v)));
  set_int("OBVI_COV_ROW_TILES", k.cov_row_tiles); k.cov_row_tiles = std::max(1, k.cov_row_tiles);
  k.host_threads = std::min(16, usable_cpus()); set_int("OBVI_HOST_THREADS", k.host_threads); k.host_threads = std::max(1, k.host_threads);
  set_i64("OBVI_POINT_RENUMBER_MIN", k.point_renumber_min);
  set_flag("OBVI_SIDE", k.side);
  set_int("OBVI_SIDE_MAX_SOLVERS", k.side_max_solvers);
  set_i64("OBVI_FORK_EARLY_BELOW", k.fork_early_below);
  set_i64("OBVI_SMALL_LANES_BELOW", k.small_lanes_below);
  set_flag("OBVI_SIDE_PACKED", k.side_packed);
  if (const char* v = std::getenv("OBVI_BACKSUB_LANES")) { const int n = std::atoi(v); if (n == 1 || n == 2 || n == 4 || n == 8 || n == 16 || n == 32) k.backsub_lanes = n; }
  set_flag("OBVI_POINT_FLAT", k.point_flat);
  set_int("OBVI_DET_MIN_STRIDE", k.det_min_stride); k.det_min_stride = std::max(1, k.det_min_stride);
  set_flag("OBVI_POSE_LIN_REUSE", k.pose_lin_reuse);
  set_flag("OBVI_FUSED_POTRF", k.fused_potrf);
  set_flag("OBVI_DETERMINISTIC", k.deterministic);
  k.debug_create = std::getenv("OBVI_DEBUG_CREATE") != nullptr;
  k.debug_prepare = std::getenv("OBVI_DEBUG_PREPARE") != nullptr;
  k.debug_plan = std::getenv("OBVI_DEBUG_PLAN") != nullptr;
  return k;
}

// ... and of the three that describe the process: read at the first use of any of them
const ProcessKnobs& process_knobs() {
  static const ProcessKnobs p = [] {
    ProcessKnobs k;
    k.api_timing = std::getenv("OBVI_API_TIMING") != nullptr;
    const char* affinity = std::getenv("OBVI_HOST_AFFINITY");
    k.host_affinity = affinity != nullptr && std::atoi(affinity) == 1;
    const char* threads = std::getenv("OBVI_HOST_THREADS");
    k.pool_threads = std::max(1, threads ? std::atoi(threads) : std::min(16, usable_cpus()));
    return k;
  }();
  return p;
}

int object_cov_forward(obvi_ba_handle* h, int64_t n_pairs, const char* what, int64_t* ldt_out, CovTables& keep) {
  *ldt_out = 0;
  const int od = h->od;
  // objects shared across ranks and an exchange hook: a collective call (include/obvi_ba.h) -- a member with no pairs of its own still takes part in the step's collectives
  const bool collective = exchanging(h);
  if ((n_pairs == 0 && !collective) || h->nOv == 0 || h->m == 0) return OBVI_OK;
  if (collective) { const int trc = prove_tail_order(h, what); if (trc != OBVI_OK) return trc; }
  // the undamped reduced system S = J_c^T J_c - (Schur complement of the features) at the current point, factorised: one
  // LM step's linearisation and factorisation with the trust-region radius at infinity (its candidate point is not used)
  upload_parameter_prior_diagonals(h);
  { QuietStep quiet(h, /*use_extra=*/!h->h_pp_kind.empty()); submit_step(h, 1e300, true, true, /*keep_factor=*/true); }
  if (h->h_scal[SC_CHOL_FAIL] != 0.0 || h->h_scal[SC_NONFINITE] != 0.0 || !std::isfinite(h->h_scal[SC_STEPSQ]))
    return fail(h, OBVI_ERR_NUMERICAL, std::string(what) + ": the normal equations are rank deficient at the current estimate");
  if (n_pairs == 0) return OBVI_OK;
  hipStream_t s = h->stream;
  const int nslabs = (int)((od * h->nOv + kTile - 1) / kTile);
  const int64_t ldt = (int64_t)h->nt * kTile, nrhs = (int64_t)nslabs * kTile;   // Y = L^-1 E transposed: [nrhs][ldt]
  std::vector<int32_t>& slab_first = keep.slab_first;
  slab_first.assign(nslabs, h->nt);
  for (int64_t w = 0; w < h->nOv; ++w) {
    const int sl0 = (int)(od * w / kTile), sl1 = (int)((od * w + od - 1) / kTile);
    for (int sl = sl0; sl <= sl1; ++sl) slab_first[sl] = std::min(slab_first[sl], h->h_obj_row[w] / kTile);
  }
  h->d_cov_Y.resize((size_t)(nrhs * ldt));
  OBVI_HIP(hipMemsetAsync(h->d_cov_Y.get(), 0, sizeof(double) * (size_t)(nrhs * ldt), s));
  h->d_cov_slab.upload(slab_first, s);
  const CholPlan plan = chol_plan(h);
  launch_forward_multi(s, plan, h->d_S.get(), h->d_Linv.get(), h->d_cov_Y.get(), ldt, nslabs, h->d_cov_slab.get(), h->d_obj_row.get(), (int32_t)h->nOv, h->h_row_split.data(), od);
  *ldt_out = ldt;
  return OBVI_OK;
}

void object_cov_pair_blocks(obvi_ba_handle* h, int64_t n_pairs, const uint32_t* obj_a, const uint32_t* obj_b, int64_t ldt, CovTables& keep) {
  const int od = h->od;
  std::vector<int32_t>& cols = keep.cols; std::vector<int32_t>& first_row = keep.first_row;
  cols.assign(2 * n_pairs, 0); first_row.assign(n_pairs, 0);
  for (int64_t i = 0; i < n_pairs; ++i) {
    const int32_t va = h->h_obj_vid[obj_a[i]], vb = h->h_obj_vid[obj_b[i]];
    cols[2 * i] = va >= 0 && vb >= 0 ? od * va : -1; cols[2 * i + 1] = va >= 0 && vb >= 0 ? od * vb : -1;
    first_row[i] = va >= 0 && vb >= 0 ? std::max(h->h_obj_row[va], h->h_obj_row[vb]) / kTile * kTile : 0;   // both columns are zero above
  }
  h->d_cov_cols.upload(cols, h->stream); h->d_cov_first.upload(first_row, h->stream);
  h->d_cov_out.resize((size_t)(od * od * n_pairs));
  launch_cov_pairs(h->stream, h->d_cov_Y.get(), ldt, n_pairs, h->d_cov_cols.get(), h->d_cov_first.get(), h->d_cov_out.get(), od);
}

}  // namespace obvi_lib

extern "C" {

const char* obvi_ba_version(void) { return "obvi_ba 0.1 (gfx950)"; }
const char* obvi_ba_last_error(const obvi_ba_handle* h) { return h ? h->err.c_str() : "null handle"; }

int obvi_ba_create(const obvi_ba_options* options, obvi_ba_handle** out) {
  if (!out) return OBVI_ERR_INVALID_ARGUMENT;
  ApiTimer api_timer_(__func__);
  *out = nullptr;
  if (options && options->object_block_size != 0 && options->object_block_size != 7 && options->object_block_size != 9) return OBVI_ERR_INVALID_ARGUMENT;   // 7: yaw only (the reference's build); 9: axis-angle
  if (options && options->reprojection_variant != OBVI_REPROJECTION_AUTODIFF && options->reprojection_variant != OBVI_REPROJECTION_ANALYTIC) return OBVI_ERR_INVALID_ARGUMENT;
  const Knobs knobs = read_knobs();
  // OBVI_DEBUG_CREATE: where the time of a create goes, on stderr (the first one of a process also starts the HIP runtime)
  const bool create_times = knobs.debug_create;
  auto t_prev = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!create_times) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "create: %-44s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
    t_prev = now;
  };
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return OBVI_ERR_NO_DEVICE;
  lap("hipGetDeviceCount (runtime start)");
  const int dev = options ? options->device_id : 0;
  if (dev < 0 || dev >= count) return OBVI_ERR_NO_DEVICE;
  obvi_ba_handle* h = new (std::nothrow) obvi_ba_handle();
  if (!h) return OBVI_ERR_HIP;
  h->device = dev;
  if (options) { h->reproj_variant = options->reprojection_variant; h->deterministic = options->deterministic != 0; if (options->object_block_size == 9) h->od = 9; }
  h->knobs = knobs;
  h->fused_potrf = knobs.fused_potrf;   // 0: two launches per level from the start (CI parity run)
  if (knobs.deterministic) h->deterministic = true;   // every handle of the process (a session driven through a host that does not set the option)
  try {
    OBVI_HIP(hipSetDevice(dev));
    lap("hipSetDevice");
    OBVI_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    lap("first stream");
    // coherent (fine-grained): the host polls this page while the step is still running (wait_scalars); with a non-coherent mapping it
    // would see the device's write only at the end of the stream
    OBVI_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->h_scal), sizeof(double) * (SC_COUNT + 1), hipHostMallocCoherent));
    std::memset(h->h_scal, 0, sizeof(double) * (SC_COUNT + 1));
    lap("pinned scalar page");
    OBVI_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->staging.base), kStagingBytes, hipHostMallocDefault));
    h->staging.cap = kStagingBytes;
    lap("pinned staging arena");
    h->d_scal.resize(SC_COUNT);   // deterministic mode: grown by ensure_det_slots() to hold per-workgroup partial sums behind the block (ba_device.h)
    // the side stream (pose pass, small factor families, diagonal blocks, far pairs: beside the Schur strips)
    OBVI_HIP(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    for (auto& e : h->ev) OBVI_HIP(hipEventCreate(&e));
    for (auto& e : h->ev_end) OBVI_HIP(hipEventCreate(&e));
    OBVI_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming)); OBVI_HIP(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));   // ordering only: no timestamps
    lap("scalar block, second stream, events");
  } catch (const HipError&) {
    delete h;
    return OBVI_ERR_HIP;
  }
  *out = h;
  return OBVI_OK;
}

void obvi_ba_destroy(obvi_ba_handle* h) {
  if (!h) return;
  ApiTimer api_timer_(__func__);
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->stream2) (void)hipStreamSynchronize(h->stream2);
  for (auto& e : h->ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : h->ev_end) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : {h->ev_fork, h->ev_join}) if (e) (void)hipEventDestroy(e);
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  if (h->h_scal) (void)hipHostFree(h->h_scal);
  if (h->staging.base) (void)hipHostFree(h->staging.base);
  select_scratch_free(&h->sel_scratch);
  // DevBuf members free in ~obvi_ba_handle
  hipStream_t s = h->stream;
  delete h;
  if (s) (void)hipStreamDestroy(s);
}

int obvi_ba_reset(obvi_ba_handle* h) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  // the state obvi_ba_create leaves, with the device allocations, streams, events and pinned pages kept: no cameras, blocks or factors, no
  // parameter priors, nothing shared and no exchange hook, no snapshot, no iteration records, profiling off and its sums at zero
  int rc = obvi_ba_set_parameter_priors(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (!rc) rc = obvi_ba_set_reproj(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 1.0);
  if (!rc) rc = obvi_ba_set_bbox(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0, 1e6);
  if (!rc) rc = obvi_ba_set_shape_priors(h, 0, nullptr, nullptr, nullptr, 1.0);
  if (!rc) rc = obvi_ba_set_ltm_priors(h, 0, nullptr, nullptr, nullptr, 1.0);
  if (!rc) rc = obvi_ba_set_relpose(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0);
  if (!rc) rc = obvi_map_set_pair_priors(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1.0);
  if (!rc) rc = obvi_map_set_group_priors(h, 0, nullptr, nullptr, nullptr, nullptr, 1.0);
  if (!rc) rc = obvi_ba_set_poses(h, 0, nullptr, nullptr);
  if (!rc) rc = obvi_ba_set_points(h, 0, nullptr, nullptr);
  if (!rc) rc = obvi_ba_set_objects(h, 0, nullptr, nullptr);
  if (!rc) rc = obvi_ba_set_cameras(h, 0, nullptr, nullptr);
  if (rc) return rc;
  OBVI_API_BEGIN
  h->h_is_shared.clear(); h->h_shared_ov.clear(); h->rank = 0; h->world = 1; h->tail_t0 = -1; h->tail_level0 = -1;
  h->allreduce = nullptr; h->allreduce_user = nullptr; h->map_exchange = false;
  h->have_snapshot = false; h->use_extra = false; h->pc_valid = false; h->lin_valid = false; h->tiles_cleared = false;
  h->iterations.clear();
  h->profiling = 0; h->ck_used = 0;
  for (auto& v : h->phase_ms) v = 0.0;
  for (auto& v : h->phase_launches) v = 0;
  for (auto& v : h->ck_ms) v = 0.0;
  for (auto& v : h->ck_launches) v = 0;
  // fused_potrf / potrf_wait_timeouts stay: a wait time-out of the fused kernel is a property of the device and runtime (dispatch order), not of
  // the problem -- a pooled handle that learned it does not pay the on-device wait again at every reuse
  h->dirty = true; h->mask_dirty = false; h->cov_valid = false;
  h->err.clear();
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_prepare(obvi_ba_handle* h) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, "prepare: cameras not set");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  prepare(h);
  sync(h);   // the plan's uploads have left the host arrays they were issued from
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_evaluate(obvi_ba_handle* h, int32_t apply_loss, double* cost, double* residuals, double* block_sqnorm) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, "evaluate: cameras not set");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  prepare(h);
  hipStream_t s = h->stream;
  const EvalLayout lay = families(h).layout();
  const int64_t nres = lay.row[FAM_COUNT], nfac = lay.slot[FAM_COUNT];
  h->d_eval_res.resize((size_t)nres + 1); h->d_eval_sq.resize((size_t)nfac + 1);
  OBVI_HIP(hipMemsetAsync(h->d_scal.get(), 0, sizeof(double) * SC_COUNT, s));
  launch_pose_cache(s, h->P, h->d_pose.get(), h->d_pc.get(), h->reproj_variant == OBVI_REPROJECTION_ANALYTIC);
  launch_evaluate(s, blocks_dev(h), reproj_dev(h), h->d_rp_perm.get(), small_dev(h), h->d_cams.get(), h->d_pc.get(), h->d_pose.get(),
                  h->d_point.get(), h->d_obj.get(), apply_loss, lay, h->d_eval_res.get(), h->d_eval_sq.get(), h->d_scal.get());
  launch_map_group_eval(s, blocks_dev(h), map_group_dev(h), h->d_obj.get(), apply_loss, h->d_eval_res.get() + lay.row[FAM_MG], h->d_eval_sq.get() + lay.slot[FAM_MG], h->d_scal.get());
  if (!cost && !residuals && !block_sqnorm) return OBVI_OK;   // nothing to hand back (obvi_ba_select_outliers: its kernels follow on the same stream)
  double c = 0.0;
  OBVI_HIP(hipMemcpyAsync(&c, h->d_scal.get() + SC_COST, sizeof(double), hipMemcpyDeviceToHost, s));
  if (residuals) h->d_eval_res.download(residuals, (size_t)nres, s);
  if (block_sqnorm) h->d_eval_sq.download(block_sqnorm, (size_t)nfac, s);
  sync(h);
  if (cost) *cost = c;
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_debug_linearize(obvi_ba_handle* h, int32_t type, double* r, double* J0, double* J1) {
  if (!h || !r || !J0) return OBVI_ERR_INVALID_ARGUMENT;
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  prepare(h);
  hipStream_t s = h->stream;
  if (type == OBVI_FACTOR_MAP_GROUP_PRIOR) {   // r of all groups, J0 = W group after group (the device's own copy)
    if (h->n_mg == 0) return OBVI_OK;
    DevBuf<double> dr;
    dr.resize((size_t)h->mg_rows);
    launch_map_group_debug(s, map_group_dev(h), h->d_obj.get(), dr.get());
    dr.download(r, (size_t)h->mg_rows, s);
    size_t nw = 0;
    for (int64_t g = 0; g < h->n_mg; ++g) { const size_t N = (size_t)h->od * (size_t)(h->h_mg_ptr[g + 1] - h->h_mg_ptr[g]); nw += N * N; }
    h->d_mg_W.download(J0, nw, s);
    sync(h);
    return OBVI_OK;
  }
  const FamilyTable fams = families(h);
  const FactorFamily* f = fams.find(type);
  if (!f) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "debug_linearize: unknown factor type");
  const int m = f->m, d0 = f->d0, d1 = f->d1; const int64_t n = f->n;
  DevBuf<double> dr, dJ0, dJ1;
  dr.resize((size_t)n * m + 1); dJ0.resize((size_t)n * m * d0 + 1); dJ1.resize((size_t)n * m * d1 + 1);
  if (type == OBVI_FACTOR_REPROJECTION) {
    launch_pose_cache(s, h->P, h->d_pose.get(), h->d_pc.get(), h->reproj_variant == OBVI_REPROJECTION_ANALYTIC);
    launch_debug_linearize_reproj(s, reproj_dev(h), h->d_rp_perm.get(), h->d_cams.get(), h->d_pc.get(), h->d_point.get(), dr.get(), dJ0.get(), dJ1.get());
  } else {
    launch_debug_linearize_small(s, type, small_dev(h), h->d_cams.get(), h->d_pose.get(), h->d_obj.get(), dr.get(), dJ0.get(), dJ1.get());
  }
  dr.download(r, (size_t)n * m, s); dJ0.download(J0, (size_t)n * m * d0, s);
  if (J1 && d1) dJ1.download(J1, (size_t)n * m * d1, s);
  sync(h);
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_debug_reduced_system(obvi_ba_handle* h, double radius, double* lhs, double* rhs, int32_t m_cap, int32_t* m_out) {
  if (!h || !lhs || !rhs) return OBVI_ERR_INVALID_ARGUMENT;
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  if (h->mask_dirty) h->dirty = true;   // the canonical (caller-order) view below is that of a plan built for exactly the current masks
  prepare(h);
  if (m_out) *m_out = (int32_t)h->m_canon;
  if (h->m_canon > m_cap) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "debug_reduced_system: buffer too small");
  // the LM step's own assembly, as at a first iteration: the rank's own system (no exchange), without the parameter priors
  QuietStep quiet(h); assemble_step(h, radius, /*first_iter=*/true, /*schur=*/true, /*exchange=*/false);
  hipStream_t s = h->stream;
  const int64_t mc = h->m_canon, nt = h->nt;
  std::vector<double> tiles((size_t)nt * nt * kTile * kTile), hr((size_t)nt * kTile);
  std::vector<int32_t> tl((size_t)2 * h->ntiles);
  h->d_S.download(tiles.data(), tiles.size(), s); h->d_rhs.download(hr.data(), hr.size(), s);
  h->d_tiles.download(tl.data(), tl.size(), s);
  sync(h);
  // tiles outside the structural mask are never written: read them as zero
  std::vector<uint8_t> mk((size_t)nt * nt, 0);
  for (int t = 0; t < h->ntiles; ++t) mk[(size_t)tl[2 * t] * nt + tl[2 * t + 1]] = 1;
  // canonical order (variable poses by index, then objects) <- rows of the tile grid (elimination order)
  for (int64_t ci = 0; ci < mc; ++ci) {
    const int64_t i = h->h_canon_row[ci];
    rhs[ci] = hr[i];
    for (int64_t cj = 0; cj < mc; ++cj) {
      const int64_t j = h->h_canon_row[cj];
      const int64_t r = std::max(i, j), c = std::min(i, j);
      const size_t tix = (size_t)(r / kTile) * nt + (c / kTile);
      lhs[ci * mc + cj] = mk[tix] ? tiles[tix * (kTile * kTile) + (r % kTile) * kTile + (c % kTile)] : 0.0;
    }
  }
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_debug_reduced_solve(obvi_ba_handle* h, double radius, const double* lhs_in, const double* rhs_in, double* lhs, double* rhs, double* y,
                                int32_t* grid_row, int32_t m_cap, int32_t* m_out) {
  if (!h || !lhs || !rhs || !y || (lhs_in == nullptr) != (rhs_in == nullptr)) return OBVI_ERR_INVALID_ARGUMENT;
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, "debug_reduced_solve: cameras not set");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  if (exchanging(h)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "debug_reduced_solve: the handle exchanges shared objects; the entry solves a rank's own system only");
  if (h->mask_dirty) h->dirty = true;   // (as obvi_ba_debug_reduced_system)
  prepare(h);
  if (m_out) *m_out = (int32_t)h->m_canon;
  if (h->m_canon > m_cap) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "debug_reduced_solve: buffer too small");
  const int64_t mc = h->m_canon, nt = h->nt;
  if (mc == 0 || h->m == 0) return OBVI_OK;
  hipStream_t s = h->stream;
  constexpr int64_t TT = (int64_t)kTile * kTile;
  std::vector<double> tiles((size_t)(nt * nt * TT)), hr((size_t)nt * kTile), hy((size_t)nt * kTile);
  std::vector<int32_t> tl((size_t)2 * h->ntiles);
  h->d_tiles.download(tl.data(), tl.size(), s);
  sync(h);
  std::vector<uint8_t> mk((size_t)nt * nt, 0);   // tiles outside the structural mask are never written and never read
  for (int t = 0; t < h->ntiles; ++t) mk[(size_t)tl[2 * t] * nt + tl[2 * t + 1]] = 1;
  const bool given = lhs_in != nullptr;
  if (given) {
    for (int64_t ci = 0; ci < mc; ++ci)
      for (int64_t cj = 0; cj < mc; ++cj) {
        const double v = lhs_in[ci * mc + cj], w = lhs_in[cj * mc + ci];
        if (!(v == w) && !(v != v && w != w)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "debug_reduced_solve: the given system is not symmetric");
        const int64_t i = h->h_canon_row[ci], j = h->h_canon_row[cj];
        if (v != 0.0 && !mk[(size_t)(std::max(i, j) / kTile) * nt + std::min(i, j) / kTile])
          return fail(h, OBVI_ERR_INVALID_ARGUMENT, "debug_reduced_solve: a non-zero entry of the given system lies outside the structural tile mask");
      }
  }
  // between the step's assembly and its factorisation: the system as the factorisation is about to see it -- or the caller's, put in its place
  const std::function<void()> between = [&] {
    h->d_S.download(tiles.data(), tiles.size(), s); h->d_rhs.download(hr.data(), hr.size(), s);
    sync(h);
    if (!given) return;
    for (int64_t ci = 0; ci < mc; ++ci) {   // real rows only: the padding rows keep the identity the step's clear gave them
      const int64_t i = h->h_canon_row[ci];
      hr[i] = rhs_in[ci];
      for (int64_t cj = 0; cj < mc; ++cj) {
        const int64_t j = h->h_canon_row[cj];
        const int64_t r = std::max(i, j), c = std::min(i, j);
        const size_t tix = (size_t)(r / kTile) * nt + (c / kTile);
        if (!mk[tix]) continue;
        const double v = lhs_in[ci * mc + cj];
        tiles[tix * TT + (r % kTile) * kTile + (c % kTile)] = v;
        if (r / kTile == c / kTile) tiles[tix * TT + (c % kTile) * kTile + (r % kTile)] = v;   // diagonal tiles are kept symmetric
      }
    }
    OBVI_HIP(hipMemcpyAsync(h->d_S.get(), tiles.data(), tiles.size() * sizeof(double), hipMemcpyHostToDevice, s));
    OBVI_HIP(hipMemcpyAsync(h->d_rhs.get(), hr.data(), hr.size() * sizeof(double), hipMemcpyHostToDevice, s));
    sync(h);
  };
  // the LM step itself, as at a first iteration, with the factor kept in the tiles (nothing is cleared behind it: the next step clears)
  { QuietStep quiet(h); submit_step(h, radius, /*first_iter=*/true, /*solve=*/true, /*keep_factor=*/true, &between); }
  h->d_y.download(hy.data(), hy.size(), s);
  sync(h);
  bool finite = true;
  for (int64_t ci = 0; ci < mc; ++ci) {
    const int64_t i = h->h_canon_row[ci];
    rhs[ci] = hr[i]; y[ci] = hy[i]; finite = finite && std::isfinite(hy[i]);
    if (grid_row) grid_row[ci] = (int32_t)i;
    for (int64_t cj = 0; cj < mc; ++cj) {
      const int64_t j = h->h_canon_row[cj];
      const int64_t r = std::max(i, j), c = std::min(i, j);
      const size_t tix = (size_t)(r / kTile) * nt + (c / kTile);
      lhs[ci * mc + cj] = mk[tix] ? tiles[tix * TT + (r % kTile) * kTile + (c % kTile)] : 0.0;
    }
  }
  if (h->h_scal[SC_CHOL_FAIL] != 0.0 || h->h_scal[SC_NONFINITE] != 0.0 || !finite)
    return fail(h, OBVI_ERR_NUMERICAL, "debug_reduced_solve: the step reports a non-positive pivot or a non-finite entry");
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_object_covariances(obvi_ba_handle* h, int64_t n_pairs, const uint32_t* obj_a, const uint32_t* obj_b, double* cov49) {
  if (!h || n_pairs < 0 || (n_pairs > 0 && (!obj_a || !obj_b || !cov49))) return OBVI_ERR_INVALID_ARGUMENT;
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, "object_covariances: cameras not set");
  for (int64_t i = 0; i < n_pairs; ++i) if ((int64_t)obj_a[i] >= h->O || (int64_t)obj_b[i] >= h->O) return fail(h, OBVI_ERR_OUT_OF_RANGE, "object_covariances: object index out of range");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  prepare(h);
  const int od = h->od, od2 = od * od;
  std::fill(cov49, cov49 + od2 * n_pairs, 0.0);
  int64_t ldt = 0;
  CovTables tables;   // alive until the wait below
  { const int rc = object_cov_forward(h, n_pairs, "object_covariances", &ldt, tables); if (rc != OBVI_OK || ldt == 0) return rc; }
  hipStream_t s = h->stream;
  object_cov_pair_blocks(h, n_pairs, obj_a, obj_b, ldt, tables);
  OBVI_HIP(hipGetLastError());
  h->d_cov_out.download(cov49, (size_t)(od2 * n_pairs), s);
  sync(h);
  for (int64_t i = 0; i < od2 * n_pairs; ++i) if (!std::isfinite(cov49[i])) return fail(h, OBVI_ERR_NUMERICAL, "object_covariances: non-finite covariance");
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_set_parameter_priors(obvi_ba_handle* h, int64_t n, const uint8_t* kind, const uint32_t* block, const uint8_t* param, const double* mean, const double* std_dev) {
  if (!h || n < 0 || (n > 0 && (!kind || !block || !param || !mean || !std_dev))) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "set_parameter_priors: bad arguments");
  OBVI_API_BEGIN
  for (int64_t i = 0; i < n; ++i) {
    const int64_t cnt = kind[i] == 0 ? h->P : kind[i] == 1 ? h->L : kind[i] == 2 ? h->O : -1;
    const int dim = kind[i] == 0 ? 6 : kind[i] == 1 ? 3 : h->od;
    if (cnt < 0 || param[i] >= dim) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "set_parameter_priors: unknown block kind or parameter index");
    if ((int64_t)block[i] >= cnt) return fail(h, OBVI_ERR_OUT_OF_RANGE, "set_parameter_priors: index out of range");
    if (!(std_dev[i] > 0.0) || !std::isfinite(std_dev[i]) || !std::isfinite(mean[i])) return fail(h, OBVI_ERR_NUMERICAL, "set_parameter_priors: standard deviation must be positive and finite");
  }
  h->h_pp_kind.assign(kind, kind + n); h->h_pp_block.assign(block, block + n); h->h_pp_param.assign(param, param + n);
  h->h_pp_mean.assign(mean, mean + n); h->h_pp_std.assign(std_dev, std_dev + n);
  h->cov_valid = false;
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_column_sqnorms(obvi_ba_handle* h, double* pose6, double* point3, double* object7) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, "column_sqnorms: cameras not set");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  prepare(h);
  // one linearisation as at iteration 0: the Jacobi scale it stores is s = 1 / (1 + sqrt(c)), c the squared column norm
  { QuietStep quiet(h); if (h->num_params > 0) submit_step(h, 1e300, true, false); }
  std::vector<double> sc((size_t)h->m_canon + 1), sl((size_t)3 * h->L + 1);
  std::vector<int32_t> pose_vid((size_t)h->P + 1), obj_vid((size_t)h->O + 1);
  std::vector<uint8_t> point_var((size_t)h->L + 1);
  hipStream_t s = h->stream;
  if (h->m_canon) h->d_scale.download(sc.data(), (size_t)h->m_canon, s);
  if (h->L) { h->d_scale_l.download(sl.data(), (size_t)3 * h->L, s); h->d_point_var.download(point_var.data(), (size_t)h->L, s); }
  if (h->P) h->d_pose_vid.download(pose_vid.data(), (size_t)h->P, s);
  if (h->O) h->d_obj_vid.download(obj_vid.data(), (size_t)h->O, s);
  sync(h);
  auto colsq = [](double scale) { const double r = 1.0 / scale - 1.0; return r * r; };
  if (pose6) for (int64_t p = 0; p < h->P; ++p) for (int k = 0; k < 6; ++k) pose6[6 * p + k] = pose_vid[p] >= 0 ? colsq(sc[6 * (int64_t)pose_vid[p] + k]) : -1.0;
  if (point3) for (int64_t l = 0; l < h->L; ++l) { const int64_t li = pt_internal(h, l); for (int k = 0; k < 3; ++k) point3[3 * l + k] = point_var[li] ? colsq(sl[3 * li + k]) : -1.0; }
  if (object7) for (int64_t o = 0; o < h->O; ++o) for (int k = 0; k < h->od; ++k) object7[h->od * o + k] = obj_vid[o] >= 0 ? colsq(sc[6 * h->nPv + h->od * (int64_t)obj_vid[o] + k]) : -1.0;
  for (size_t i = 0; i < h->h_pp_kind.size(); ++i) {
    const double w = 1.0 / (h->h_pp_std[i] * h->h_pp_std[i]);
    const int64_t b = h->h_pp_block[i];
    if (h->h_pp_kind[i] == 0 && pose6 && pose_vid[b] >= 0) pose6[6 * b + h->h_pp_param[i]] += w;
    else if (h->h_pp_kind[i] == 1 && point3 && point_var[pt_internal(h, b)]) point3[3 * b + h->h_pp_param[i]] += w;
    else if (h->h_pp_kind[i] == 2 && object7 && obj_vid[b] >= 0) object7[h->od * b + h->h_pp_param[i]] += w;
  }
  return OBVI_OK;
  OBVI_API_END(h)
}

}  // extern "C"

namespace {
// the selection over `n` block norms on the device (select_kernels.hip), the mask into the caller's memory: ONE wait for the device
void run_selection(obvi_ba_handle* h, int64_t n, const double* sq, const uint8_t* act, const uint32_t* inv, double fraction, uint8_t* mask_out, int64_t* num_excluded) {
  h->d_sel_mask.resize((size_t)n + 1);
  int n_out = 0;
  // one round is four launches and one wait; a further round only when more than 4096 distinct values share the open bin's bits (24 more bits each: at most three rounds)
  for (int round = 0; round <= 2; ++round) {
    const int* result_dev = nullptr;
    OBVI_HIP(select_by_threshold(h->stream, n, sq, act, inv, fraction, h->d_sel_mask.get(), &h->sel_scratch, &result_dev, round));
    void* pinned_mask = n ? h->staging.take((size_t)n) : nullptr;
    int* pinned_result = static_cast<int*>(h->staging.take(2 * sizeof(int)));
    int pageable_result[2] = {0, 0};
    if (n) OBVI_HIP(hipMemcpyAsync(pinned_mask ? pinned_mask : mask_out, h->d_sel_mask.get(), (size_t)n, hipMemcpyDeviceToHost, h->stream));
    OBVI_HIP(hipMemcpyAsync(pinned_result ? pinned_result : pageable_result, result_dev, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    sync(h);
    const int* result = pinned_result ? pinned_result : pageable_result;
    n_out = result[0];
    if (result[1] == 0) {
      if (pinned_mask) std::memcpy(mask_out, pinned_mask, (size_t)n);
      break;
    }
    if (result[1] != round + 1 || round == 2) throw HipError{hipErrorUnknown, "outlier selection: the radix select did not finish", __FILE__, __LINE__};
  }
  if (num_excluded) *num_excluded = n_out;
}
}  // namespace

extern "C" {

int obvi_ba_select_outliers(obvi_ba_handle* h, int32_t type, double fraction, uint8_t* mask_out, int64_t* num_excluded) {
  if (!h || !mask_out) return OBVI_ERR_INVALID_ARGUMENT;
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));   // (the evaluate below is skipped when the previous call already left the norms: this path allocates and launches as well)
  // un-robustified per-block squared norms at the current estimate (object_pose_graph_optimizer.h:682-693), kept on the device; the
  // runner selects for one factor type after the other (offline_problem_runner.h:769-800): the second call finds them in place
  const uint64_t this_call = h->api_calls;
  if (h->eval_sq_call == 0 || h->eval_sq_call + 1 != this_call) {
    const int rc = obvi_ba_evaluate(h, 0, nullptr, nullptr, nullptr);
    if (rc != OBVI_OK) return rc;
  }
  const FamilyTable fams = families(h);
  const FactorFamily* f = fams.find(type);
  if (!f) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "select_outliers: unknown factor type");
  const uint32_t* inv = nullptr;   // reprojection: the norms are in the sorted order, the mask goes out in the caller's
  if (type == OBVI_FACTOR_REPROJECTION) {
    if (!h->rp_inv_on_device) { h->d_rp_inv.upload(h->h_rp_inv, h->stream); h->rp_inv_on_device = true; }
    inv = h->d_rp_inv.get();
  }
  run_selection(h, f->n, h->d_eval_sq.get() + fams.layout().slot[fams.index(f)], f->d_active->get(), inv, fraction, mask_out, num_excluded);
  h->eval_sq_call = h->api_calls;   // (the evaluate above counted as a call of its own)
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_debug_select(obvi_ba_handle* h, int64_t n, const double* sq, const uint8_t* active, double fraction, uint8_t* mask_out, int64_t* num_excluded) {
  if (!h || n < 0 || (n > 0 && (!sq || !mask_out))) return OBVI_ERR_INVALID_ARGUMENT;
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  DevBuf<double> d_sq; DevBuf<uint8_t> d_act;
  std::vector<uint8_t> ones;
  if (!active) { ones.assign((size_t)n, 1); active = ones.data(); }
  d_sq.upload(sq, (size_t)n, h->stream); d_act.upload(active, (size_t)n, h->stream);
  sync(h);
  run_selection(h, n, d_sq.get(), d_act.get(), nullptr, fraction, mask_out, num_excluded);
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_snapshot(obvi_ba_handle* h) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  copy_current(h, h->d_pose_s, h->d_point_s, h->d_obj_s);
  sync(h);
  h->have_snapshot = true;
  return OBVI_OK;
  OBVI_API_END(h)
}
int obvi_ba_restore(obvi_ba_handle* h) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  if (!h->have_snapshot) return fail(h, OBVI_ERR_NOT_READY, "restore: no snapshot");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  restore_from(h, h->d_pose_s, h->d_point_s, h->d_obj_s);
  sync(h);
  h->cov_valid = false;
  return OBVI_OK;
  OBVI_API_END(h)
}

static int get_blocks(obvi_ba_handle* h, const DevBuf<double>& d, int64_t n, int dim, double* out) {
  if (!h || (n > 0 && !out)) return OBVI_ERR_INVALID_ARGUMENT;
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  d.download(out, (size_t)n * dim, h->stream);
  sync(h);
  return OBVI_OK;
  OBVI_API_END(h)
}
int obvi_ba_get_poses(obvi_ba_handle* h, double* out) { return h ? get_blocks(h, h->d_pose, h->P, 6, out) : OBVI_ERR_INVALID_ARGUMENT; }
int obvi_ba_get_points(obvi_ba_handle* h, double* out) {
  if (!h || (h->L > 0 && !out)) return OBVI_ERR_INVALID_ARGUMENT;
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  const double* src = points_in_caller_order(h, h->d_point);
  if (h->L > 0) OBVI_HIP(hipMemcpyAsync(out, src, sizeof(double) * 3 * (size_t)h->L, hipMemcpyDeviceToHost, h->stream));
  sync(h);
  return OBVI_OK;
  OBVI_API_END(h)
}
int obvi_ba_get_objects(obvi_ba_handle* h, double* out) { return h ? get_blocks(h, h->d_obj, h->O, h->od, out) : OBVI_ERR_INVALID_ARGUMENT; }

int obvi_ba_get_state(obvi_ba_handle* h, double* poses, double* points, double* objects) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  // the three copies land in the handle's pinned arena (a copy into pageable memory blocks, one after the other), ONE wait, then out
  struct Part { double* out; const DevBuf<double>* d; size_t n; void* pinned; } parts[3] = {
      {poses, &h->d_pose, (size_t)h->P * 6, nullptr}, {points, &h->d_point, (size_t)h->L * 3, nullptr}, {objects, &h->d_obj, (size_t)h->O * (size_t)h->od, nullptr}};
  for (Part& p : parts) {
    if (!p.out || !p.n) continue;
    p.pinned = h->staging.take(p.n * sizeof(double));
    double* dst = p.pinned ? static_cast<double*>(p.pinned) : p.out;
    if (p.d == &h->d_point) OBVI_HIP(hipMemcpyAsync(dst, points_in_caller_order(h, h->d_point), p.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));   // (the caller's feature numbering)
    else p.d->download(dst, p.n, h->stream);
  }
  sync(h);
  for (Part& p : parts) if (p.pinned) std::memcpy(p.out, p.pinned, p.n * sizeof(double));
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_set_shared_objects(obvi_ba_handle* h, const uint8_t* is_shared, int32_t rank, int32_t world) {
  if (!h || world < 1 || rank < 0 || rank >= world) return OBVI_ERR_INVALID_ARGUMENT;
  OBVI_API_BEGIN
  if (is_shared) h->h_is_shared.assign(is_shared, is_shared + h->O); else h->h_is_shared.clear();
  h->rank = rank; h->world = world;
  h->dirty = true;
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_ba_set_allreduce(obvi_ba_handle* h, obvi_allreduce_fn fn, void* user) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  h->allreduce = fn; h->allreduce_user = user;
  return OBVI_OK;
}

int obvi_map_allow_exchange(obvi_ba_handle* h, int32_t on) {
  if (!h || (on != 0 && on != 1)) return OBVI_ERR_INVALID_ARGUMENT;
  // read by validate_indices and check_session_objects alone: no device call, and the plan does not depend on it
  h->map_exchange = on != 0;
  return OBVI_OK;
}

int obvi_ba_set_profiling(obvi_ba_handle* h, int32_t level) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  h->profiling = level;
  return OBVI_OK;
}

int obvi_ba_get_problem_stats(const obvi_ba_handle* h, double* out, int32_t cap) {
  if (!h || !out) return 0;
  int64_t act_rp = 0, act_bb = 0;
  for (uint8_t a : h->h_rp_active) act_rp += a != 0;
  for (uint8_t a : h->h_bb_active) act_bb += a != 0;
  const double v[23] = {(double)h->nPv, (double)h->nOv, (double)h->nLv, (double)h->m_canon, (double)h->nt, (double)h->nblk, (double)(h->npairs + h->npairs_window),
                        (double)h->ntiles, (double)h->n_trsm_jobs, (double)h->n_upd_products, h->chol_flops, (double)act_rp, (double)act_bb,
                        (double)h->nlevels, (double)h->knobs.host_threads, (double)usable_cpus(),
                        (double)h->potrf_wait_timeouts, h->fused_potrf ? 1.0 : 0.0,   // [16] LM steps re-run because a potrf workgroup of the fused level kernel timed out waiting for its jobs, [17] the fused schedule is still on
                        (double)h->n_point_waves, (double)h->n_long_points, (double)h->npairs, (double)h->nbatches,   // [18..21] how the host cut the point pass and the Schur strips (obvi_ba.h)
                        (double)(h->schur_narrow ? SchurNarrow::kGroupCols : SchurWide::kGroupCols)};   // [22] the strip geometry of the plan
  const int n = std::min<int>(cap, 23);
  for (int i = 0; i < n; ++i) out[i] = v[i];
  return n;
}

int obvi_ba_get_kernel_times(const obvi_ba_handle* h, char* names, int32_t names_cap, double* total_ms, int64_t* launches, int32_t cap) {
  if (!h || !names || !total_ms || !launches) return 0;
  int n = 0, off = 0;
  auto put = [&](const char* name, double ms, int64_t cnt) {
    const int len = (int)std::strlen(name);
    if (n >= cap || off + len + 1 > names_cap) return;
    std::memcpy(names + off, name, len + 1);
    off += len + 1;
    total_ms[n] = ms; launches[n] = cnt;
    ++n;
  };
  for (int p = 0; p < PH_COUNT; ++p) put(kPhaseNames[p], h->phase_ms[p], h->phase_launches[p]);
  static const char* kCholNames[CK_COUNT] = {"k_potrf", "k_trsm", "k_update_potrf", "k_backward"};
  for (int k = 0; k < CK_COUNT; ++k) if (h->ck_launches[k] > 0) put(kCholNames[k], h->ck_ms[k], h->ck_launches[k]);
  return n;
}

}  // extern "C"
