/*
 * obvi_map_update.h -- the way back into a device-resident map (obvi_map_resident.h): read a map, and condition it on the posterior a window ends with.
 * Same library, same handle and status codes as obvi_ba.h; this header includes obvi_map_resident.h, never the reverse.
 *
 * The loop the map exists for:   map -> prior of the window's objects -> solve -> posterior of those objects -> map.  obvi_map_set_group_priors_from_map is
 * the first arrow; the calls below are the last.  The map is x ~ N(mu, C) over n objects, Cs = (C + C^T) / 2.  A window held the map objects A (k objects,
 * N_A = k od rows, in the caller's order) with their marginal N(mu_A, Cs_AA) as its prior, and ends with the posterior N(m, P) over A.  The rest of the map meets
 * the window's measurements only through x_A, so with K = Cs[:, A] Cs_AA^-1 the joint posterior is exactly
 *       mu' = mu + K (m - mu_A)            C' = Cs - K (Cs_AA - P) K^T
 * which also updates every object the window never saw, through its correlation with A.  Everything is computed on the map's device (fp64 tiles on the matrix
 * cores); only a status record of a few doubles crosses to the host.
 *
 * obvi_map_get copies a map back: mean [n][od] and cov [n od][n od] exactly as the device holds them; either pointer may be NULL.
 *
 * obvi_map_condition builds a NEW map on the map's device from post_mean [k][od] and post_cov [k od][k od] (symmetrised: Ps = (P + P^T) / 2) of the map
 * objects map_idx[0..k).  `map` itself is not written -- maps stay immutable, other threads may be cutting priors from it -- and may be destroyed before or
 * after the new one.  The new map is exactly symmetric, its A x A block is Ps and its A means are post_mean, bit for bit; it is a map like any other: usable by
 * any handle of the device from any thread once the call has returned (the call's one wait), destroyed by obvi_map_destroy.  k may cover the whole map: the
 * result is then the posterior itself.
 *
 * obvi_map_condition_on_handle takes the posterior from the handle, on the device: m = the current estimates of the session objects obj_idx[0..k), P = their
 * joint covariance (the k x k blocks obvi_ba_object_covariances returns for all pairs).  Nothing of the posterior crosses to the host.
 *
 * What `h` lends: its device, stream, workspaces and obvi_ba_last_error.  Neither call changes its groups, factors, masks or estimate.  obvi_map_condition
 * leaves the handle exactly as it was; obvi_map_condition_on_handle has the side effects of an obvi_ba_object_covariances call and no others (it linearises, so
 * it drops an obvi_cov_* result).
 *
 * Refused before any launch or device allocation (*out = NULL on every failure) -- OBVI_ERR_INVALID_ARGUMENT: null pointers; k < 1; a map on another device or
 * of another block size than the handle's; a map object twice; k od > OBVI_MAP_GROUP_MAX_ROWS; for the handle form also a session object twice, a constant
 * session object, a handle that exchanges shared objects.  OBVI_ERR_OUT_OF_RANGE: map_idx >= n, obj_idx >= O.  OBVI_ERR_NUMERICAL: a non-finite entry of
 * post_mean / post_cov.  The handle form also returns, as obvi_ba_object_covariances does, OBVI_ERR_NOT_READY while the handle has reprojection or
 * bounding-box factors and no cameras, and the status of the problem's own validation.  It refuses a session object that no active factor touches (it is
 * no variable of the solve and has no covariance) with OBVI_ERR_INVALID_ARGUMENT once the plan is known, before anything is allocated for the new map.
 * "Exchanges shared objects" is decided from what was set -- an all-reduce hook and at least one shared object -- not from the plan: no collective is entered.
 * (With obvi_map_allow_exchange on -- obvi_map_shared.h -- the handle form runs on such a handle instead: the posterior is the joint one and the call is collective.)
 * Refused from what the device reports (OBVI_ERR_NUMERICAL, nothing left allocated): Cs_AA fails the pivot or condition tests of
 * obvi_map_set_group_priors_from_map (the same status record, the same thresholds); a non-finite entry in the result; for the handle form rank-deficient
 * normal equations, as obvi_ba_object_covariances reports them.
 *
 * NOT checked: neither P nor the result is tested for positive definiteness.  A posterior that is not below its prior (Cs_AA - P not positive semidefinite)
 * can give an indefinite map.  As before, a map is only ever used through its sub-blocks, and the cut checks those.
 *
 * No sum of the update depends on the order in which workgroups run: the same call twice gives bit-identical maps, on default and deterministic handles alike.
 */
#ifndef OBVI_MAP_UPDATE_H_
#define OBVI_MAP_UPDATE_H_

#include <stdint.h>

#include "obvi_map_resident.h"

#ifdef __cplusplus
extern "C" {
#endif

int obvi_map_get(const obvi_map* map, double* mean /*[n][od] or NULL*/, double* cov /*[n*od][n*od] or NULL*/);

int obvi_map_condition(obvi_ba_handle* h, const obvi_map* map, int64_t k, const uint32_t* map_idx /*[k]*/, const double* post_mean /*[k][od]*/,
                       const double* post_cov /*[k*od][k*od]*/, obvi_map** out);

int obvi_map_condition_on_handle(obvi_ba_handle* h, const obvi_map* map, int64_t k, const uint32_t* obj_idx /*[k]*/, const uint32_t* map_idx /*[k]*/,
                                 obvi_map** out);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_MAP_UPDATE_H_ */
