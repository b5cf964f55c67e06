// cov.cpp -- covariance blocks of poses, features and objects by selected inversion of the reduced system's factor  (include/obvi_cov.h; kernels: cov_kernels.hip;
// shared state and helpers: ba_handle.h)
#include "ba_handle.h"
#include "../../include/obvi_cov.h"

namespace {

// What the inversion and the pattern test need of the symbolic plan, rebuilt when the plan was: the first scratch tile of every tile column inside its
// level (the Y tiles of a level lie one behind the other in the order of the level's columns) and the tile mask of L.  Read back from the plan's own
// device tables, so the symbolic phase of a solve carries nothing for it.
void cov_plan_tables(obvi_ba_handle* h) {
  if (h->cov_plan_serial == h->plan_serial) return;
  hipStream_t s = h->stream;
  const int32_t nt = h->nt;
  std::vector<int32_t> lvl_k((size_t)nt + 1), col_ptr((size_t)nt + 2), tiles((size_t)2 * h->ntiles + 2);
  h->d_lvl_k.download(lvl_k.data(), (size_t)nt, s); h->d_col_ptr.download(col_ptr.data(), (size_t)nt + 1, s); h->d_tiles.download(tiles.data(), (size_t)2 * h->ntiles, s);
  sync(h);
  std::vector<int32_t> ybase((size_t)nt + 1, 0);
  int64_t widest = 0;
  for (int l = 0; l < h->nlevels; ++l) {
    int64_t at = 0;
    for (int32_t x = h->h_lvl_k_ptr[l]; x < h->h_lvl_k_ptr[l + 1]; ++x) { const int32_t k = lvl_k[x]; ybase[k] = (int32_t)at; at += col_ptr[k + 1] - col_ptr[k]; }
    widest = std::max(widest, at);
  }
  h->h_cov_mask.assign((size_t)nt * nt, 0);
  for (int32_t t = 0; t < h->ntiles; ++t) h->h_cov_mask[(size_t)tiles[2 * t] * nt + tiles[2 * t + 1]] = 1;
  h->d_cov_ybase.upload(ybase, s);
  h->d_cov_ys.resize((size_t)widest * kTile * kTile + 1);
  sync(h);
  h->cov_plan_serial = h->plan_serial;
}

bool cov_ready(obvi_ba_handle* h) { return h->cov_valid && !h->dirty && !h->mask_dirty; }
const char* const kNotReady = "no covariance pass for the current state: call obvi_cov_compute (values, factors, masks, flags or priors changed, or a solve ran)";

// first row and size of a reduced block in the tile grid; row -1: constant or unused (a zero block); false: a kind the reduced system does not hold
bool block_rows(const obvi_ba_handle* h, int kind, uint32_t idx, int32_t* row, int32_t* dim) {
  if (kind == OBVI_COV_POSE) { const int32_t v = h->h_cov_pose_vid[idx]; *row = v >= 0 ? h->h_pose_row[v] : -1; *dim = 6; return true; }
  if (kind == OBVI_COV_OBJECT) { const int32_t v = h->h_obj_vid[idx]; *row = v >= 0 ? h->h_obj_row[v] : -1; *dim = h->od; return true; }
  return false;
}
bool on_pattern(const obvi_ba_handle* h, int32_t ra, int32_t da, int32_t rb, int32_t db) {
  if (ra < 0 || rb < 0) return true;   // a zero block
  for (int32_t ta = ra / kTile; ta <= (ra + da - 1) / kTile; ++ta)
    for (int32_t tb = rb / kTile; tb <= (rb + db - 1) / kTile; ++tb)
      if (!h->h_cov_mask[(size_t)std::max(ta, tb) * h->nt + std::min(ta, tb)]) return false;
  return true;
}
// desc (4 per item) / off -> out, one launch and one wait
void gather(obvi_ba_handle* h, const std::vector<int32_t>& desc, const std::vector<int64_t>& off, int64_t extent, double* out) {
  const int64_t n = (int64_t)off.size();
  if (n == 0 || extent == 0) return;
  hipStream_t s = h->stream;
  h->d_cov_desc.upload(desc, s); h->d_cov_off.upload(off, s);
  h->d_cov_blk.resize((size_t)extent);
  OBVI_HIP(hipMemsetAsync(h->d_cov_blk.get(), 0, sizeof(double) * (size_t)extent, s));   // (gaps the caller's offsets leave)
  launch_cov_gather(s, h->d_S.get(), h->nt, n, h->d_cov_desc.get(), h->d_cov_off.get(), h->d_cov_blk.get());
  OBVI_HIP(hipGetLastError());
  std::vector<double> host((size_t)extent);
  h->d_cov_blk.download(host.data(), (size_t)extent, s);
  sync(h);
  for (int64_t i = 0; i < n; ++i) std::memcpy(out + off[i], host.data() + off[i], sizeof(double) * (size_t)(desc[4 * i + 2] * desc[4 * i + 3]));
}
int own_blocks(obvi_ba_handle* h, const char* what, int kind, int64_t n, const uint32_t* idx, double* out) {
  if (!h || n < 0 || (n > 0 && (!idx || !out))) return OBVI_ERR_INVALID_ARGUMENT;
  const int64_t cnt = kind == OBVI_COV_POSE ? h->P : h->O;
  for (int64_t i = 0; i < n; ++i) if ((int64_t)idx[i] >= cnt) return fail(h, OBVI_ERR_OUT_OF_RANGE, std::string(what) + ": index out of range");
  if (!cov_ready(h)) return fail(h, OBVI_ERR_NOT_READY, std::string(what) + ": " + kNotReady);
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  std::vector<int32_t> desc((size_t)4 * n); std::vector<int64_t> off((size_t)n);
  int32_t dim = kind == OBVI_COV_POSE ? 6 : h->od;
  for (int64_t i = 0; i < n; ++i) {
    int32_t row = -1;
    block_rows(h, kind, idx[i], &row, &dim);
    desc[4 * i] = row; desc[4 * i + 1] = row; desc[4 * i + 2] = dim; desc[4 * i + 3] = dim; off[i] = i * dim * dim;
  }
  gather(h, desc, off, n * dim * dim, out);
  return OBVI_OK;
  OBVI_API_END(h)
}
// the pairs' rows; OBVI_OK, or the status of the first pair that cannot be served (`on` given: no failure for an off-pattern pair, the answer per pair)
int pair_rows(obvi_ba_handle* h, const char* what, int64_t n, const uint8_t* ka, const uint32_t* ia, const uint8_t* kb, const uint32_t* ib, std::vector<int32_t>* desc, uint8_t* on) {
  desc->resize((size_t)4 * n);
  for (int64_t i = 0; i < n; ++i) {
    for (int side = 0; side < 2; ++side) {
      const int kind = side ? kb[i] : ka[i]; const uint32_t idx = side ? ib[i] : ia[i];
      if (kind == OBVI_COV_POINT) return fail(h, OBVI_ERR_INVALID_ARGUMENT, std::string(what) + ": cross blocks of features are not served (obvi_cov_point_blocks gives a feature's own block)");
      if (kind != OBVI_COV_POSE && kind != OBVI_COV_OBJECT) return fail(h, OBVI_ERR_INVALID_ARGUMENT, std::string(what) + ": unknown block kind");
      if ((int64_t)idx >= (kind == OBVI_COV_POSE ? h->P : h->O)) return fail(h, OBVI_ERR_OUT_OF_RANGE, std::string(what) + ": index out of range");
    }
    int32_t* d = desc->data() + 4 * i;
    block_rows(h, ka[i], ia[i], &d[0], &d[2]); block_rows(h, kb[i], ib[i], &d[1], &d[3]);
    const bool ok = on_pattern(h, d[0], d[2], d[1], d[3]);
    if (on) on[i] = ok ? 1 : 0;
    else if (!ok) {
      char buf[320];
      std::snprintf(buf, sizeof(buf), "%s: pair %lld (%s %u, %s %u) is not on the tile pattern of the factor: its covariance is not zero, it is not computed%s", what, (long long)i,
                    ka[i] == OBVI_COV_POSE ? "pose" : "object", ia[i], kb[i] == OBVI_COV_POSE ? "pose" : "object", ib[i],
                    ka[i] == OBVI_COV_OBJECT && kb[i] == OBVI_COV_OBJECT ? " (obvi_ba_object_covariances serves any pair of objects)" : "");
      return fail(h, OBVI_ERR_INVALID_ARGUMENT, buf);
    }
  }
  return OBVI_OK;
}

}  // namespace

extern "C" {

int obvi_cov_compute(obvi_ba_handle* h) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  if (!check_ready(h)) return fail(h, OBVI_ERR_NOT_READY, "cov_compute: cameras not set");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  prepare(h);
  h->cov_valid = false;
  // objects shared across ranks and an exchange hook: a collective pass (include/obvi_cov.h).  Collective (0) proves the tail order; the step below issues (1), (2)
  // and (3) as in a solve, and (3) sums the failure flags, so every member takes the branch below together.
  if (exchanging(h)) { const int trc = prove_tail_order(h, "cov_compute"); if (trc != OBVI_OK) return trc; }
  hipStream_t s = h->stream;
  const double t0 = wall_s();
  h->cov_ms[0] = h->cov_ms[1] = 0.0;
  if (h->num_params > 0) {
    // the undamped system at the current point, factorised: one LM step's linearisation and factorisation with the trust-region radius at infinity
    // (obvi_ba_object_covariances takes the same route); its point pass leaves the Z and C^-1 records the feature blocks are formed from
    upload_parameter_prior_diagonals(h);
    { QuietStep quiet(h, /*use_extra=*/!h->h_pp_kind.empty()); submit_step(h, 1e300, true, true, /*keep_factor=*/true); }
    if (h->h_scal[SC_CHOL_FAIL] != 0.0 || h->h_scal[SC_NONFINITE] != 0.0 || !std::isfinite(h->h_scal[SC_STEPSQ]))
      return fail(h, OBVI_ERR_NUMERICAL, "cov_compute: the normal equations are rank deficient at the current estimate");
  }
  const double t1 = wall_s();
  if (h->m > 0 && h->nt > 0) {
    cov_plan_tables(h);
    launch_selected_inverse(s, chol_plan(h), h->d_S.get(), h->d_Linv.get(), h->d_cov_ys.get(), h->d_cov_ybase.get());
    OBVI_HIP(hipGetLastError());
  }
  h->h_cov_pose_vid.assign((size_t)h->P + 1, -1);
  if (h->P) h->d_pose_vid.download(h->h_cov_pose_vid.data(), (size_t)h->P, s);
  sync(h);
  h->cov_ms[0] = 1e3 * (t1 - t0); h->cov_ms[1] = 1e3 * (wall_s() - t1);
  h->cov_valid = true;
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_cov_pose_blocks(obvi_ba_handle* h, int64_t n, const uint32_t* pose_idx, double* out) { return own_blocks(h, "cov_pose_blocks", OBVI_COV_POSE, n, pose_idx, out); }
int obvi_cov_object_blocks(obvi_ba_handle* h, int64_t n, const uint32_t* obj_idx, double* out) { return own_blocks(h, "cov_object_blocks", OBVI_COV_OBJECT, n, obj_idx, out); }

int obvi_cov_point_blocks(obvi_ba_handle* h, int64_t n, const uint32_t* point_idx, double* out) {
  if (!h || n < 0 || (n > 0 && (!point_idx || !out))) return OBVI_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n; ++i) if ((int64_t)point_idx[i] >= h->L) return fail(h, OBVI_ERR_OUT_OF_RANGE, "cov_point_blocks: index out of range");
  if (!cov_ready(h)) return fail(h, OBVI_ERR_NOT_READY, std::string("cov_point_blocks: ") + kNotReady);
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  if (n == 0) return OBVI_OK;
  hipStream_t s = h->stream;
  const bool any = h->num_params > 0 && h->n_rp > 0;   // else no feature is a parameter of the problem: zero blocks
  std::vector<int64_t> idx((size_t)n);
  for (int64_t i = 0; i < n; ++i) idx[i] = any ? pt_internal(h, point_idx[i]) : -1;
  h->d_cov_off.upload(idx, s);
  h->d_cov_blk.resize((size_t)9 * n);
  launch_cov_points(s, h->d_S.get(), h->nt, n, h->d_cov_off.get(), h->d_point_ptr.get(), h->d_rp_yrow.get(), h->d_point_var.get(), h->d_Z.get(), h->d_Ci.get(), h->d_cov_blk.get());
  OBVI_HIP(hipGetLastError());
  h->d_cov_blk.download(out, (size_t)9 * n, s);
  sync(h);
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_cov_cross_blocks(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b, const uint32_t* idx_b, double* out, const int64_t* out_offset) {
  if (!h || n < 0 || (n > 0 && (!kind_a || !idx_a || !kind_b || !idx_b || !out))) return OBVI_ERR_INVALID_ARGUMENT;
  if (!cov_ready(h)) return fail(h, OBVI_ERR_NOT_READY, std::string("cov_cross_blocks: ") + kNotReady);
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  std::vector<int32_t> desc;
  { const int rc = pair_rows(h, "cov_cross_blocks", n, kind_a, idx_a, kind_b, idx_b, &desc, nullptr); if (rc != OBVI_OK) return rc; }
  std::vector<int64_t> off((size_t)n);
  int64_t extent = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t sz = (int64_t)desc[4 * i + 2] * desc[4 * i + 3];
    if (out_offset && out_offset[i] < 0) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "cov_cross_blocks: negative output offset");
    off[i] = out_offset ? out_offset[i] : extent;
    extent = out_offset ? std::max(extent, off[i] + sz) : extent + sz;
  }
  gather(h, desc, off, extent, out);
  return OBVI_OK;
  OBVI_API_END(h)
}

int obvi_cov_on_pattern(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b, const uint32_t* idx_b, uint8_t* on) {
  if (!h || n < 0 || (n > 0 && (!kind_a || !idx_a || !kind_b || !idx_b || !on))) return OBVI_ERR_INVALID_ARGUMENT;
  if (!cov_ready(h)) return fail(h, OBVI_ERR_NOT_READY, std::string("cov_on_pattern: ") + kNotReady);
  OBVI_API_BEGIN
  std::vector<int32_t> desc;
  return pair_rows(h, "cov_on_pattern", n, kind_a, idx_a, kind_b, idx_b, &desc, on);
  OBVI_API_END(h)
}

int obvi_cov_get_stats(const obvi_ba_handle* h, double* linearize_factor_ms, double* inversion_ms, int64_t* scratch_bytes) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  if (linearize_factor_ms) *linearize_factor_ms = h->cov_ms[0];
  if (inversion_ms) *inversion_ms = h->cov_ms[1];
  if (scratch_bytes) *scratch_bytes = (int64_t)(h->d_cov_ys.size() * sizeof(double));
  return OBVI_OK;
}

}  // extern "C"
