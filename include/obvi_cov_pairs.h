/*
 * obvi_cov_pairs.h -- covariance blocks of any declared pair, features included (the covariance_blocks argument of ceres::Covariance::Compute).
 * Part of obvi_cov.h, which includes it: same library, same handle, same matrix, same block layout and status codes.
 *
 * obvi_cov_compute serves the pairs on the tile pattern of the factor and no cross block of a feature.  obvi_cov_compute_pairs takes the list of
 * wanted pairs up front -- the factor exists only until the selected inversion overwrites it, so a pair cannot be completed afterwards -- and
 * then serves exactly those in addition:
 *   - it does everything obvi_cov_compute does: the linearisation, the factor, the selected inverse, the stats and every getter come out as
 *     after a plain compute (bit for bit on a deterministic handle);
 *   - obvi_cov_cross_blocks writes a declared pair as dim(a) x dim(b), a feature's dimension being 3, whatever its kinds (OBVI_COV_POSE,
 *     OBVI_COV_POINT, OBVI_COV_OBJECT) and wherever it lies; it is accepted in either order, and (b, a) is the exact transpose of (a, b);
 *   - obvi_cov_on_pattern reports 1 for a declared pair ("can be served");
 *   - a pair of a block with itself is its own block, for features too; a pair with a constant block, or with a block no active factor
 *     touches, is a zero block;
 *   - an undeclared pair behaves as after obvi_cov_compute: off the pattern or with a feature it is refused, with the same messages;
 *   - the declared set lives and dies with the result: what invalidates the result drops it, and a later obvi_cov_compute clears it.
 * n = 0 is obvi_cov_compute.  An index out of range (OBVI_ERR_OUT_OF_RANGE) or an unknown kind (OBVI_ERR_INVALID_ARGUMENT) is refused before
 * any device work; rank-deficient normal equations give OBVI_ERR_NUMERICAL.
 *
 * How: a reduced pair (poses, objects) off the pattern is E_a^T S^-1 E_b = (L^-1 E_a)^T (L^-1 E_b), one forward substitution per distinct
 * block of such pairs, run between the factorisation and the selected inversion.  A pair with a feature l follows from the records of the
 * point pass and the reduced blocks of the poses that observe l; the reduced blocks it needs off the pattern join the
 * forward substitution.  Device memory, allocated by the first call that declares pairs (a handle that never does holds none of it):
 * 8 bytes x (right-hand sides, rounded up to 64) x (rows of the tile grid), and the declared blocks.  A request whose right-hand sides
 * would need more than 1 GiB is refused with OBVI_ERR_INVALID_ARGUMENT.
 *
 * NOT COLLECTIVE: on a handle that exchanges (shared objects and an exchange hook) a call with n > 0 is refused with
 * OBVI_ERR_INVALID_ARGUMENT before any collective is issued; the collective form is deliberately not built.  n = 0 is the collective
 * obvi_cov_compute.
 */
#ifndef OBVI_COV_PAIRS_H_
#define OBVI_COV_PAIRS_H_

#include <stdint.h>

#include "obvi_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

int obvi_cov_compute_pairs(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b,
                           const uint32_t* idx_b);

/* Debug / verification: obvi_cov_compute_pairs on the same pairs (n = 0: obvi_cov_compute), exposing the system the pass inverts.
 *   lhs [m][m] (row-major, canonical order: variable poses by index, then objects -- the order of obvi_ba_debug_reduced_solve): a copy of the tiles
 *       taken between the pass's assembly and its factorisation: undamped, parameter-prior diagonals included; tiles outside the structural
 *       mask read as zero.  grid_row [m] (may be null): the row of the tile grid of every canonical index.
 *   lhs_in (may be null): values put in place of the assembled tiles, which lhs then shows.  Checked as obvi_ba_debug_reduced_solve checks its
 *       own: symmetric, no non-zero entry outside the structural tile mask, else OBVI_ERR_INVALID_ARGUMENT before any device work of the pass;
 *       a non-positive pivot or a NaN gives OBVI_ERR_NUMERICAL, as the pass answers rank deficiency (lhs is written all the same).
 * m_cap: rows the buffers hold; *m_out: m.  On success the handle is in the pass's finished state: every getter serves blocks of that one
 * factorisation.  Refused on a handle that exchanges shared objects (OBVI_ERR_INVALID_ARGUMENT). */
int obvi_cov_debug_compute_pairs(obvi_ba_handle* h, int64_t n, const uint8_t* kind_a, const uint32_t* idx_a, const uint8_t* kind_b,
                                 const uint32_t* idx_b, const double* lhs_in, double* lhs, int32_t* grid_row, int32_t m_cap, int32_t* m_out);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_COV_PAIRS_H_ */
