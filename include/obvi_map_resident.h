/*
 * obvi_map_resident.h -- a long-term map kept on the device, and group priors (factor type 10, obvi_map_group_prior.h) cut from it there.
 * Same library, same handle and status codes as obvi_ba.h; this header includes obvi_map_group_prior.h, never the reverse.
 *
 * A session solves another set of objects at every window, and the prior that fits a window is the map's Gaussian marginalised to the objects the window
 * holds.  In covariance form that marginal is a gather: the sub-block of the map's joint covariance.  The factor needs W = L^-1 and Lambda = C^-1 of the
 * sub-block, so every window needs a factorisation -- obvi_map_set_group_priors does it on the host from a host pointer; the calls below keep the map's
 * covariance on the device and cut, factor and invert every window's groups there.
 *
 * The map: n objects of od parameters (od = 7 or 9; 0 reads 7), their means [n][od] and their joint covariance [n od][n od], row-major.  It is uploaded
 * once, is immutable afterwards and lives on `device_id`; any handle on that device may use it, from any thread.  Refused before any device allocation:
 * null mean, cov or out, n_objects < 1, a block size other than 0, 7 or 9, a covariance above 1 GiB (OBVI_ERR_INVALID_ARGUMENT); a mean or covariance entry
 * that is not finite (OBVI_ERR_NUMERICAL); no such device (OBVI_ERR_NO_DEVICE).  *out is NULL on every failure.  Positive definiteness is not checked: a map
 * is only ever used through its sub-blocks.
 *
 * Group priors from the map: member k of the call is session object obj_idx[k] and map object map_idx[k]; group g holds the members
 * [group_ptr[g], group_ptr[g + 1]).  Group g's C is the map's covariance restricted to the rows and columns of its members, in the order given, symmetrised
 * ((C + C^T) / 2); its mean is the members' map means.  After a successful call the handle is in the state that
 *       obvi_map_set_group_priors(h, n_groups, group_ptr, obj_idx, mean[map_idx], cov[map_idx x map_idx], huber)
 * would have left: the same factors, masks all 1, the plan to be rebuilt -- and everything obvi_map_group_prior.h says about the factor holds.
 * n_groups = 0 clears the groups; obvi_ba_reset clears them too and does not touch the map, which the handle does not own.  The handle keeps no reference to
 * the map: the call returns after its one wait for the device, and the map may be destroyed before the solve.
 *
 * Refused before the first launch, with the codes of obvi_map_set_group_priors for what that call refuses, and: a null map, a map on another device than
 * the handle's, a map whose block size is not the handle's, a map object named twice in the call (OBVI_ERR_INVALID_ARGUMENT); a map_idx >= the map's object
 * count (OBVI_ERR_OUT_OF_RANGE).  Refused from what the device reports, after one read-back of a few doubles per group (OBVI_ERR_NUMERICAL): a Cholesky pivot
 * that is not positive and finite; (largest / smallest pivot)^2 above 1e13; the condition estimate above 1e13 -- the largest eigenvalue of C times the largest
 * of Lambda, 40 power steps each from the fixed start of the host entry.  A refused call leaves the handle's groups exactly as they were.
 *
 * Two calls with the same arguments give bit-identical W and Lambda, on default and deterministic handles alike: no sum of the device stages depends on
 * the order in which workgroups run.
 */
#ifndef OBVI_MAP_RESIDENT_H_
#define OBVI_MAP_RESIDENT_H_

#include <stdint.h>

#include "obvi_map_group_prior.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct obvi_map obvi_map;

int obvi_map_create(int32_t device_id, int32_t object_block_size, int64_t n_objects, const double* mean /*[n][od]*/, const double* cov /*[n*od][n*od]*/,
                    obvi_map** out);
void obvi_map_destroy(obvi_map* map);              /* NULL is a no-op */
int64_t obvi_map_num_objects(const obvi_map* map); /* -1 for NULL */

int obvi_map_set_group_priors_from_map(obvi_ba_handle* h, const obvi_map* map, int64_t n_groups, const int64_t* group_ptr /*[n_groups+1]*/,
                                       const uint32_t* obj_idx /*[group_ptr[n]]*/, const uint32_t* map_idx /*[group_ptr[n]]*/, double huber);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_MAP_RESIDENT_H_ */
