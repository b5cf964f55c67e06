/*
 * obvi_map_locate.h -- one device-resident map (obvi_map_resident.h) located in another from the constellations of their labelled object centres, on the
 * device.  Same library, same handle and status codes as obvi_ba.h; this header includes obvi_map_resident.h, never the reverse.
 *
 * The entry that moves a map into another frame takes the transform as an argument.  This one produces it: from two resident maps and nothing else it
 * proposes, scores, ranks and refines the transforms T = T_A<-B that lay B's objects onto A's.  What fixes T is the constellation of the centres and the
 * covariance blocks that say how far a centre may be off; both live on the device alone.
 *
 * Used are the centre rows 0..2 of the means, p_o, and the symmetrised 3 x 3 centre blocks of the covariances, Cs = (C + C^T) / 2 with every entry
 * 0.5 (C[r][c] + C[c][r]): A_a of map a, B_b of map b.  Nothing else of a block is read, so the entry is the same for od 7 and od 9.  Both frames are taken to
 * share the vertical: T = (tx ty tz psi), p' = Rz(psi) p + t, the transform of the moving entry at od 7 (at od 9 that entry takes (t, 0, 0, psi)).  A TILTED
 * frame is left out.
 *
 * Seeds.  A seed is a pair a1 < a2 of A and an ordered pair b1 != b2 of B with label_a[a1] == label_b[b1] >= 0 and label_a[a2] == label_b[b2] >= 0 (a NULL
 *   label array: every object has label 0; a negative label takes an object out of every seed and out of every score).  Such a seed is TESTED.  With
 *   u = xy(p_a2 - p_a1), v = xy(p_b2 - p_b1), |u| = sqrt(ux ux + uy uy), it is COMPATIBLE if
 *       |u| >= pair_min_distance,  |v| >= pair_min_distance,  | |u| - |v| | <= pair_tolerance,  |(z_a2 - z_a1) - (z_b2 - z_b1)| <= pair_tolerance,
 *   every product, sum and difference rounded on its own.  The seed index is the place of (a1, a2, b1, b2) in lexicographic order.
 *   A compatible seed gives a hypothesis: psi = atan2(vx uy - vy ux, vx ux + vy uy); with the midpoints m_A = (p_a1 + p_a2) / 2 and m_B,
 *       (tx, ty) = xy(m_A) - Rz(psi) xy(m_B),   tz = z(m_A) - z(m_B).
 * Score.  For each object b of B with label_b[b] >= 0: p' = Rz(psi) p_b + t, and for each a with label_a[a] == label_b[b]:
 *       e = p_a - p',   S = A_a + Rz(psi) B_b Rz(psi)^T,   S = L L^T,   s = |L^-1 e|^2.
 *   Singular is a pair with a pivot of L that is not positive and finite or with p_min^2 <= 1e-13 p_max^2 (the pivot test of
 *   obvi_map_set_group_priors_from_map); a singular pair is no inlier.  b is an INLIER if the smallest s over its non-singular a is <= inlier_gate; its
 *   partner is that a, the smallest such a on ties.  inliers(h) is their number, cost(h) the sum of the minima over the inliers in ascending b.
 *   One-to-one is NOT enforced: two objects of B may have the same partner.  The host-only resolver of the entry that proposes duplicates exists for that, later in
 *   the chain.
 * Rank.  The hypotheses with inliers >= min_inliers, ordered by inliers descending, then cost ascending, then seed index ascending; the first `capacity` are
 *   reported: seed = (a1 a2 b1 b2), transform, transform_cov, inliers, cost, partner.  capacity = 0 with NULL arrays is a count-only call.
 *   counts[0]: the seeds tested; counts[1]: the compatible ones; counts[2]: the hypotheses with inliers >= min_inliers, also beyond capacity.
 * Refine.  Reported hypotheses only: refine_iterations Gauss-Newton steps on (t, psi) of sum over the inliers of e^T S^-1 e, the partners held fixed, S formed
 *   anew at each iterate's psi (its derivative is not part of the step).  With G_i = [I3 | Rz'(psi) p_b] (3 x 4):
 *       H = sum G_i^T S_i^-1 G_i,    g = sum G_i^T S_i^-1 e_i,    T <- T + H^-1 g        (a pair whose S is singular at the iterate adds nothing)
 *   transform is the last iterate and transform_cov = H^-1 formed at it; with 0 iterations transform is the seed's and transform_cov is taken there.  inliers,
 *   cost and partner are the seed's, whatever the iterations.
 *   This covariance is CORRELATED with both maps -- it is made of them -- while obvi_map_transform takes the transform's error to be independent of the map it
 *   moves.  A caller who goes on to merge the same pairs should move B with the located T as linearisation point and a WIDE Sigma, so that the merge and not
 *   the move decides where B ends.  The correlated form is left out.
 *
 * Limits.  OBVI_MAP_LOCATE_MAX_OBJECTS = 819 bounds n_a + n_b: 100 bytes an object (twelve doubles: centre, block; its label) of both maps stay in the 80 KiB
 * of local memory that let two workgroups of the scoring kernel share a compute unit.  OBVI_MAP_LOCATE_MAX_SEEDS = 2^20 bounds the compatible seeds of a call.
 *
 * What `h` lends: its device, stream, workspaces and obvi_ba_last_error.  The handle is left exactly as it was: its problem, its estimate, its group priors
 * and its covariance results.  Neither map is written.  The call waits for the device at most twice: for the counts, and, if hypotheses are reported, for them.
 *
 * Refused before any launch or device allocation, with nothing written to the outputs -- OBVI_ERR_INVALID_ARGUMENT: null h, a, b, params or counts;
 * capacity < 0; a null seed, transform, inliers or cost with capacity > 0; a map on another device or of another block size than the handle's; a parameter
 * that is not finite or outside its range below; n_a + n_b > OBVI_MAP_LOCATE_MAX_OBJECTS.
 * Refused after the first wait -- OBVI_ERR_OUT_OF_RANGE: more than OBVI_MAP_LOCATE_MAX_SEEDS compatible seeds.  counts[0] and counts[1] are written
 * (counts[2] = 0) and nothing else, so that the caller can tighten pair_tolerance or add labels.
 * n_a < 2 or n_b < 2: no seeds, OBVI_OK, counts all zero.
 *
 * No sum and no output position depends on the order in which workgroups run: the same call twice gives bit-identical outputs, on default and deterministic
 * handles alike.
 */
#ifndef OBVI_MAP_LOCATE_H_
#define OBVI_MAP_LOCATE_H_

#include <stdint.h>

#include "obvi_map_resident.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OBVI_MAP_LOCATE_MAX_OBJECTS 819
#define OBVI_MAP_LOCATE_MAX_SEEDS 1048576

typedef struct {
  double pair_min_distance;   /* > 0: a seed needs both horizontal baselines at least this long (psi is ill-determined below it) */
  double pair_tolerance;      /* >= 0: | |u| - |v| | <= tol and |dz_A - dz_B| <= tol */
  double inlier_gate;         /* > 0, finite: chi-square bar on the three centre rows */
  int32_t min_inliers;        /* >= 2: hypotheses with fewer are counted, never reported */
  int32_t refine_iterations;  /* 0 .. 8 Gauss-Newton steps on the reported hypotheses */
} obvi_map_locate_params;

int obvi_map_locate(obvi_ba_handle* h, const obvi_map* a, const obvi_map* b,
                    const int32_t* label_a /*[n_a] or NULL*/, const int32_t* label_b /*[n_b] or NULL*/,
                    const obvi_map_locate_params* params, int64_t capacity,
                    uint32_t* seed /*[capacity][4]: a1 a2 b1 b2*/, double* transform /*[capacity][4]: tx ty tz psi*/,
                    double* transform_cov /*[capacity][4][4] or NULL*/, int32_t* inliers /*[capacity]*/, double* cost /*[capacity]*/,
                    int32_t* partner /*[capacity][n_b] or NULL: A object per B object, -1 none*/,
                    int64_t* counts /*[3]: seeds tested, seeds compatible, hypotheses with >= min_inliers*/);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_MAP_LOCATE_H_ */
