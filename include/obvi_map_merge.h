/*
 * obvi_map_merge.h -- a device-resident map (obvi_map_resident.h) that shrinks: objects that are the same physical object fused into one, on the device.  Same
 * library, same handle and status codes as obvi_ba.h; this header includes obvi_map_resident.h, never the reverse.
 *
 * A map that several sessions append to gathers duplicates: two sessions each discover the same chair and each appends it, or a later window finds that its
 * "new" object is one the map already holds under another number.  Which objects are duplicates is the front end's decision (the reference takes it at session
 * end, by class and a merge distance); this entry does the algebra that follows from it.  The gather of the entries that grow a map only DROPS an object: it
 * throws away everything the map knew through the dropped estimate and leaves the survivor, and every object correlated with either, where they were.
 *
 * The map is x ~ N(mu, C) over n objects, Cs = (C + C^T) / 2, N = n od rows.  Pair r of q declares map object drop_idx[r] to be the same object as
 * keep_idx[r]; a group of m duplicates is m - 1 pairs with one keep.  The constraint is H x = d (+ noise): block row r of H has +I at the drop object and -I at
 * the keep object, d_r = offset[r] (a yaw wrap of 2 pi, or an axis swap the caller has resolved, goes there; NULL: zeros), R = blockdiag(Rs_r) with
 * Rs_r = (noise[r] + noise[r]^T) / 2 (NULL: R = 0, the constraint is exact).  With Q = q od, G = Cs H^T (N x Q), T = H G + R = L L^T, W = L^-1, Y = G W^T:
 *       mu' = mu - Y W (H mu - d)                          C' = Cs - Y Y^T
 * restricted to the n - q objects that are not dropped, which keep their old relative order.  With an exact constraint x_drop = x_keep + d holds with
 * probability one and dropping loses nothing; with noise the drop is a marginalisation of the conditioned Gaussian.  Every other object of the map moves through
 * its correlation with the pair.  Everything is computed on the map's device (fp64 tiles on the matrix cores); only a status record of a few doubles crosses to
 * the host.
 *
 * obvi_map_merge builds a NEW map on the map's device.  `map` is not written and may be destroyed before or after the new one.  The new map is exactly
 * symmetric; it is a map like any other, usable by any handle of the device from any thread once the call has returned (the call's one wait).  Its power-step
 * start vector is the old map's.  new_index (NULL: not wanted) receives, for every old object o of the n, its number in the new map -- a dropped object gets
 * its keep's new number; it is filled on the host, and only on success.
 *
 * What `h` lends: its device, stream, workspaces and obvi_ba_last_error.  The handle is left exactly as it was: its problem, its estimate, its group priors
 * and its covariance results.
 *
 * Refused before any launch or device allocation (*out = NULL on every failure) -- OBVI_ERR_INVALID_ARGUMENT: null h, map, drop_idx, keep_idx or out; q < 1; a
 * map on another device or of another block size than the handle's; q od > OBVI_MAP_GROUP_MAX_ROWS; drop_idx[r] == keep_idx[r]; an object dropped twice; an
 * object that is dropped in one pair and kept in another (chains are the caller's to resolve to one survivor per group).  OBVI_ERR_OUT_OF_RANGE: an index >= n.
 * OBVI_ERR_NUMERICAL: a non-finite entry of offset or noise.
 * Refused from what the device reports (OBVI_ERR_NUMERICAL, nothing left allocated): T fails the pivot or condition tests of
 * obvi_map_set_group_priors_from_map (the same status record, the same thresholds) -- this is what a pair that is ALREADY merged does: two perfectly correlated
 * copies give T = 0; a non-finite entry in the result.
 * NOT checked: neither the noise blocks nor the result are tested for positive definiteness.
 *
 * No sum depends on the order in which workgroups run: the same call twice gives bit-identical maps, on default and deterministic handles alike.
 */
#ifndef OBVI_MAP_MERGE_H_
#define OBVI_MAP_MERGE_H_

#include <stdint.h>

#include "obvi_map_resident.h"

#ifdef __cplusplus
extern "C" {
#endif

int obvi_map_merge(obvi_ba_handle* h, const obvi_map* map, int64_t q, const uint32_t* drop_idx /*[q]*/, const uint32_t* keep_idx /*[q]*/,
                   const double* offset /*[q][od] or NULL: zeros*/, const double* noise /*[q][od][od] or NULL: exact*/, uint32_t* new_index /*[n] or NULL*/,
                   obvi_map** out);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_MAP_MERGE_H_ */
