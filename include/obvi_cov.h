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
 * obvi_ba.h (rank-deficient normal equations: OBVI_ERR_NUMERICAL).  Results are bit-identical from run to run on a deterministic handle.
 *
 * OBJECTS SHARED ACROSS RANKS (obvi_ba_set_shared_objects and an exchange hook, obvi_ba.h "multi-GPU"): obvi_cov_compute is then a COLLECTIVE
 * call, as obvi_ba_solve is -- every member of the job calls it, each on its own host thread, and so is obvi_ba_object_covariances.  A handle
 * without shared objects or without a hook behaves as described above.  The matrix is that of the JOINT problem of all members.  The shared
 * objects are eliminated last on every member, so the shared tail is the root of every member's elimination tree: after the members' Schur
 * complements onto it are summed, every member holds the joint factor of the tail, and the recursion from the root down needs nothing of the
 * other members' factors.
 *   Collectives per call, in this order, each issued exactly once by every member (obvi_rccl_group_stats counts four per call):
 *     (0) 2 doubles, sum: proof that every member lays the shared tail out alike (the check obvi_ba_solve runs first).  A member whose shared
 *         objects are ordered differently is refused with OBVI_ERR_INVALID_ARGUMENT -- as is every other member, since the sum is the same
 *         everywhere -- before any tile is summed.
 *     (1) (od^2 + od) doubles per shared object, sum: their diagonal blocks and gradients, with the members' parameter priors on them.
 *     (2) the lower tiles and right-hand side of the shared tail, sum: the members' Schur complements onto the shared objects.
 *     (3) the step's scalar block, sum: it carries the counts of non-positive pivots and non-finite entries, so a rank-deficient or non-finite
 *         system on ANY member makes EVERY member return OBVI_ERR_NUMERICAL from the same call; no member leaves before (3), none waits alone.
 *         (A scheduling time-out of the fused factor kernel is summed there too: all members repeat (1)-(3) together.)
 *   An error that only one member can see before (0) -- cameras not set, indices out of range -- returns on that member at once; the others are
 *   released by the group's time-out (obvi_rccl_group_set_timeout), which bounds every wait of a collective.
 *   Parameter priors (obvi_ba_set_parameter_priors) on a SHARED object follow the rule for object-only factors: exactly ONE member uploads them
 *   (any member).  They travel in (1) and reach the joint tail once per member that uploaded them: the same prior given by two members counts twice.
 *   Priors on poses, features and private objects stay with their member.
 *   Results: obvi_cov_object_blocks of a shared object is its block of the joint covariance, the same on every member (bit-identical across
 *   deterministic members of a group, which sums in member order).  Pose, feature and private-object blocks are marginals of the joint problem,
 *   not of the member's sub-problem.  obvi_cov_cross_blocks / obvi_cov_on_pattern serve the member's own poses and private objects paired with
 *   each other and with shared objects wherever the tile pattern has them, and every pair of shared objects; obvi_ba_object_covariances serves
 *   any pair among the member's private and shared objects.  Indices are per handle: a pair of blocks private to two DIFFERENT members cannot be
 *   named -- a caller who wants such pairs marks both objects as shared.
 *   Validity: invalidation is per handle, as above.  A pass describes the joint problem only while NO member has changed state since; a member
 *   cannot see that a peer did, so after any member changes values, factors, masks, flags or priors, all members call obvi_cov_compute again.
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
 * obvi_cov_on_pattern answers the question without failing: on[i] = 1 if pair i can be served.  Feature cross blocks are not served.
 * (Both serve every pair that was declared to obvi_cov_compute_pairs, features included: obvi_cov_pairs.h.) */
int obvi_cov_cross_blocks(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b,
                          const uint32_t* idx_b, double* out, const int64_t* out_offset);
int obvi_cov_on_pattern(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b,
                        const uint32_t* idx_b, uint8_t* on);

/* wall time of the last obvi_cov_compute in milliseconds: linearisation + factorisation, selected inversion; extra device bytes it holds */
int obvi_cov_get_stats(const obvi_ba_handle* h, double* linearize_factor_ms, double* inversion_ms, int64_t* scratch_bytes);

#ifdef __cplusplus
}
#endif

/* pairs off the pattern and cross blocks of features, declared up front: the entry that takes the list of wanted pairs */
#include "obvi_cov_pairs.h"

#endif /* OBVI_COV_H_ */
