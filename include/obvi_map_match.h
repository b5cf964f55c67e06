/*
 * obvi_map_match.h -- duplicate objects of a device-resident map (obvi_map_resident.h) proposed, on the device.  Same library, same handle and status codes as
 * obvi_ba.h; this header includes obvi_map_resident.h, never the reverse.
 *
 * The entry that fuses duplicates takes a list of pairs that are declared to be the same physical object.  This one says which pairs those are, by the map's
 * own uncertainty: two estimates of one chair are duplicates when their difference is small in units of the covariance of that difference, and that
 * covariance needs the cross-covariance of the two, which only the device holds.  (The reference decides by class and a 2 m centre distance at session end;
 * both tests are here as pre-filters.)
 *
 * The map is x ~ N(mu, C) over n objects, Cs = (C + C^T) / 2.  Every pair a < b is considered.
 *   Tested are the pairs with label[a] == label[b] >= 0 (label NULL: all; a negative label takes an object out of every pair) whose centres, rows 0..2 of
 *     the means, satisfy ((dx dx + dy dy) + dz dz) <= D D, D = max_centre_distance (+inf: no test).
 *   The statistic, on the rows m of row_mask (bit c: parameter c of the block; 0: all od):
 *       d = mu_b[m] - mu_a[m]        T = Cs_bb[m,m] - Cs_ba[m,m] - Cs_ab[m,m] + Cs_aa[m,m]  (summed in that order)        T = L L^T        s = |L^-1 d|^2
 *     With yaw_period > 0 (od 7 only; 0: no wrap) w = yaw_period rint((mu_b[3] - mu_a[3]) / yaw_period) and row 3 of d is (mu_b[3] - mu_a[3]) - w; w is
 *     reported in yaw_offset whether or not row 3 is in the mask -- it is row 3 of the offset the fusing entry takes for "b dropped into a".
 *   Singular is a pair with a pivot of L that is not positive and finite or with p_min^2 <= 1e-13 p_max^2, the pivot test of
 *     obvi_map_set_group_priors_from_map: two perfectly correlated copies, T = 0, are what it catches.  A singular pair is counted and never reported.
 *   Reported are the pairs with s <= gate in ascending (a, b) order, the first `capacity` of them: idx_a, idx_b, stat = s, yaw_offset = w.  The gate is the
 *     caller's, in chi-square units of the masked rows.
 *   counts[0]: all pairs with s <= gate, also beyond capacity; counts[1]: the pairs tested; counts[2]: the singular ones.  capacity = 0 with NULL arrays is a
 *     count-only call.
 *
 * What `h` lends: its device, stream, workspaces and obvi_ba_last_error.  The handle is left exactly as it was: its problem, its estimate, its group priors
 * and its covariance results.  The map is not written.  The call waits for the device at most twice: for the counts, and, if pairs are reported, for them.
 *
 * Refused before any launch or device allocation, with nothing written to the outputs -- OBVI_ERR_INVALID_ARGUMENT: null h, map or counts; capacity < 0; a
 * null output array with capacity > 0; a map on another device or of another block size than the handle's; row_mask with a bit at or above od; a gate that
 * is not finite and > 0; max_centre_distance <= 0 or NaN; yaw_period negative or not finite, or > 0 with od 9.
 *
 * No sum and no output position depends on the order in which workgroups run: the same call twice gives bit-identical outputs, on default and deterministic
 * handles alike.
 *
 * obvi_map_match_resolve is host only -- no handle, no device.  It turns candidate pairs into lists the fusing entry accepts as they are.  Candidates are
 * taken in ascending (stat, a, b) order; every object starts FREE; pair (a, b) is selected if and only if a is FREE or KEEP and b is FREE, and then a becomes
 * KEEP and b DROPPED; it stops at max_pairs selected.  drop[i] = b, keep[i] = a, sel[i] = the candidate's position in the input, *q = the number selected.  No
 * object is dropped twice and no dropped object is kept; a chain (b into a, c into b) loses its later link, and the next match on the fused map tests c
 * against a directly.  object_block_size 0 reads 7.  Refused, with nothing written -- OBVI_ERR_INVALID_ARGUMENT: a null array or q; n_pairs < 0;
 * max_pairs < 1; max_pairs od > OBVI_MAP_GROUP_MAX_ROWS; a block size other than 0, 7 or 9; a pair with a >= b.  OBVI_ERR_NUMERICAL: a stat that is negative
 * or not finite.
 */
#ifndef OBVI_MAP_MATCH_H_
#define OBVI_MAP_MATCH_H_

#include <stdint.h>

#include "obvi_map_resident.h"

#ifdef __cplusplus
extern "C" {
#endif

int obvi_map_match(obvi_ba_handle* h, const obvi_map* map, const int32_t* label /*[n] or NULL*/, uint32_t row_mask, double gate, double max_centre_distance,
                   double yaw_period, int64_t capacity, uint32_t* idx_a /*[capacity]*/, uint32_t* idx_b /*[capacity]*/, double* stat /*[capacity]*/,
                   double* yaw_offset /*[capacity]*/, int64_t* counts /*[3]: found, tested, singular*/);

int obvi_map_match_resolve(int32_t object_block_size, int64_t n_pairs, const uint32_t* idx_a, const uint32_t* idx_b, const double* stat, int64_t max_pairs,
                           uint32_t* drop /*[max_pairs]*/, uint32_t* keep /*[max_pairs]*/, uint32_t* sel /*[max_pairs]*/, int64_t* q);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_MAP_MATCH_H_ */
