/*
 * obvi_cov.h -- C ABI of the covariance blocks of poses, features and objects (the part of ceres::Covariance beyond
 * obvi_ba_object_covariances), by selected inversion of the reduced system's Cholesky factor.  Same library, same handle.
 *
 * The matrix is the one obvi_ba_object_covariances documents: (J^T J)^-1 over all non-constant parameter blocks that an active factor
 * touches, J robustified, no damping, the parameter priors of obvi_ba_set_parameter_priors taking part as Jacobian rows.  Blocks are
 * row-major, rows of `a` by columns of `b`, in the caller's block numbering (features included).  The block of a constant block, or of a
 * block no active factor touches, is zero.
 *
 * obvi_cov_compute linearises at the current estimate, factorises the undamped reduced system S = L L^T (one LM step's own stages with
 * the trust region at infinity) and runs the Takahashi recursion over the tile columns of L from the root of the elimination tree down:
 * that yields every entry of S^-1 ON THE TILE PATTERN OF L at about the cost of a second factorisation.  On the pattern
 * lie every pose's and every object's own block and the cross block of every pair that shares a factor or a feature; a feature's own
 * block follows from the cross blocks of the poses that observe it.  The result overwrites the factor in place and stays on the device
 * until the next call that changes values, blocks, factors, masks, flags or priors, or that linearises (solve, obvi_ba_object_covariances,
 * obvi_ba_column_sqnorms, the debug system): a getter called after such a call returns OBVI_ERR_NOT_READY.  Device memory beyond the
 * handle's own: the Y tiles of the widest level, allocated by the first obvi_cov_compute (32 KB per off-diagonal tile of that level).
 *
 * The getters are gathers: they read the device result and return; n = 0 is legal.  Nothing throws or aborts; status codes as in
 * obvi_ba.h (rank-deficient normal equations: OBVI_ERR_NUMERICAL; objects shared across ranks with an exchange hook set:
 * OBVI_ERR_INVALID_ARGUMENT, as obvi_ba_object_covariances).  Results are bit-identical from run to run on a deterministic handle.
 */
#ifndef OBVI_COV_H_
#define OBVI_COV_H_

#include <stdint.h>

#include "obvi_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

/* block kinds, as in obvi_ba_set_parameter_priors */
#define OBVI_COV_POSE 0
#define OBVI_COV_POINT 1
#define OBVI_COV_OBJECT 2

int obvi_cov_compute(obvi_ba_handle* h);

/* own blocks: out [n][36], [n][od*od] (od = obvi_ba_options.object_block_size), [n][9] */
int obvi_cov_pose_blocks(obvi_ba_handle* h, int64_t n, const uint32_t* pose_idx, double* out);
int obvi_cov_object_blocks(obvi_ba_handle* h, int64_t n, const uint32_t* obj_idx, double* out);
int obvi_cov_point_blocks(obvi_ba_handle* h, int64_t n, const uint32_t* point_idx, double* out);

/* Cross blocks of pairs of reduced blocks (pose-pose, pose-object, object-object; a pair of a block with itself is its own block).
 * Pair i is written at out + out_offset[i] (out_offset NULL: one behind the other in the order given), dim(a) x dim(b) doubles.
 * A pair whose block is not on the tile pattern of the factor is refused with OBVI_ERR_INVALID_ARGUMENT and nothing is written: off
 * the pattern the covariance is not zero, it is not computed (object pairs: obvi_ba_object_covariances serves any pair).
 * obvi_cov_on_pattern answers the question without failing: on[i] = 1 if pair i can be served.  Feature cross blocks are not served. */
int obvi_cov_cross_blocks(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b,
                          const uint32_t* idx_b, double* out, const int64_t* out_offset);
int obvi_cov_on_pattern(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b,
                        const uint32_t* idx_b, uint8_t* on);

/* wall time of the last obvi_cov_compute in milliseconds: linearisation + factorisation, selected inversion; extra device bytes it holds */
int obvi_cov_get_stats(const obvi_ba_handle* h, double* linearize_factor_ms, double* inversion_ms, int64_t* scratch_bytes);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_COV_H_ */
