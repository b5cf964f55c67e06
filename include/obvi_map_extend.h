/*
 * obvi_map_extend.h -- a device-resident map (obvi_map_resident.h) that grows: a window's new objects appended, a first map born from a posterior, and a map
 * gathered down to some of its objects.  Same library, same handle and status codes as obvi_ba.h; this header includes obvi_map_resident.h, never the reverse.
 *
 * The map is x ~ N(mu, C) over n objects, Cs = (C + C^T) / 2.  A window held two sets of objects: A, k_old >= 0 objects of the map with their marginal
 * N(mu_A, Cs_AA) as the window's prior, and B, k_new >= 1 objects the map does not hold and that had no map prior.  It ends with the joint posterior N(m, P)
 * over (A, B) in that order, Ps = (P + P^T) / 2.  The rest of the map meets the window's measurements only through x_A, the new objects meet the map only through
 * the window, so with K = Cs[:, A] Cs_AA^-1 the joint posterior over the n + k_new objects is exactly
 *       mu'[old] = mu + K (m_A - mu_A)                     mu'[B] = m_B
 *       C'[old, old] = Cs - K (Cs_AA - Ps_AA) K^T          C'[old, B] = K Ps_AB = C'[B, old]^T          C'[B, B] = Ps_BB
 * Old objects keep their numbers; B is appended in the caller's order as objects n .. n + k_new - 1.  The old block and the old means are what the conditioning
 * entries compute for (A, m_A, P_AA), to the last bit.  Everything is computed on the map's device (fp64 tiles on the matrix cores); only a status record of a
 * few doubles crosses to the host.
 *
 * obvi_map_extend builds a NEW map on the map's device from post_mean [k_old + k_new][od] and post_cov [(k_old + k_new) od]^2 of the map objects
 * map_idx[0..k_old) followed by the new objects.  `map` is not written and may be destroyed before or after the new one.  The new map is exactly symmetric; its
 * (A u B) x (A u B) block is Ps and the means of A and B are post_mean, bit for bit; it is a map like any other, usable by any handle of the device from any
 * thread once the call has returned (the call's one wait).  Its power-step start vector is the old map's.
 *   k_old = 0: the window saw no map object; nothing is factorised, C' = blockdiag(Cs, Ps_BB), mu' = (mu, m_B).
 *   map = NULL (k_old must be 0): there is no map yet; the result is the posterior itself, on the handle's device and of its block size, with the start
 *   vector every map is created with.  This is how a first map is born on the device.
 *
 * obvi_map_extend_on_handle takes the posterior from the handle, on the device: m = the current estimates of the session objects obj_idx_old[0..k_old) (which are
 * the map objects map_idx) and obj_idx_new[0..k_new), P = their joint covariance over all (k_old + k_new)^2 pairs, as obvi_ba_object_covariances returns the
 * blocks.  Nothing of the posterior crosses to the host.
 *
 * What `h` lends: its device, stream, workspaces and obvi_ba_last_error.  obvi_map_extend leaves the handle exactly as it was; obvi_map_extend_on_handle has
 * the side effects of an obvi_ba_object_covariances call and no others (it linearises, so it drops an obvi_cov_* result).
 *
 * Refused before any launch or device allocation (*out = NULL on every failure) -- OBVI_ERR_INVALID_ARGUMENT: null h, out or posterior pointers; k_new < 1 (a
 * window with nothing new is the conditioning entries' case); k_old < 0; k_old > 0 with a null map or map_idx; a map on another device or of another block size
 * than the handle's; a map object twice; (k_old + k_new) od > OBVI_MAP_GROUP_MAX_ROWS; a result above the size obvi_map_create accepts (a covariance of 1 GiB);
 * for the handle form also null index lists, a session object twice across both lists, a constant session object, a handle that exchanges shared objects
 * (decided from what was set -- an all-reduce hook and at least one shared object -- not from the plan: no collective is entered; with obvi_map_allow_exchange
 * on -- obvi_map_shared.h -- the handle form runs on such a handle instead: the posterior is the joint one and the call is collective).  OBVI_ERR_OUT_OF_RANGE:
 * map_idx >= n, an object index >= O.  OBVI_ERR_NUMERICAL: a non-finite entry of post_mean / post_cov.  The handle form also returns OBVI_ERR_NOT_READY while
 * the handle has reprojection or bounding-box factors and no cameras, the status of the problem's own validation, and -- once the plan is known, before
 * anything is allocated for the new map -- OBVI_ERR_INVALID_ARGUMENT for a session object that no active factor touches.
 * Refused from what the device reports (OBVI_ERR_NUMERICAL, nothing left allocated): Cs_AA fails the pivot or condition tests of
 * obvi_map_set_group_priors_from_map (the same status record, the same thresholds; skipped when k_old = 0); a non-finite entry in the result; for the handle
 * form rank-deficient normal equations, as obvi_ba_object_covariances reports them.
 * NOT checked: neither P nor the result is tested for positive definiteness.
 *
 * obvi_map_select builds a new map of the objects map_idx[0..k) of `map`, in that order: a subset is their marginal, k = n a permutation.  Means and
 * covariance entries are copied exactly as the device holds them; nothing is symmetrised.  One gather on the handle's stream, one wait.  Refused: null
 * pointers, k < 1, a map on another device or of another block size, a map object twice (OBVI_ERR_INVALID_ARGUMENT); map_idx >= n (OBVI_ERR_OUT_OF_RANGE).
 * There is no row limit: k may be any 1 .. n.  This is what a bound on the map's size needs.  (Dropping a duplicate this way throws its estimate away and moves
 * nothing else; fusing duplicates is conditioning over the whole map, an entry of its own.)
 *
 * No sum depends on the order in which workgroups run: the same call twice gives bit-identical maps, on default and deterministic handles alike.
 */
#ifndef OBVI_MAP_EXTEND_H_
#define OBVI_MAP_EXTEND_H_

#include <stdint.h>

#include "obvi_map_resident.h"

#ifdef __cplusplus
extern "C" {
#endif

int obvi_map_extend(obvi_ba_handle* h, const obvi_map* map /* NULL: no map yet; k_old must be 0 */, int64_t k_old,
                    const uint32_t* map_idx /*[k_old]; may be NULL when k_old == 0*/, int64_t k_new, const double* post_mean /*[k_old + k_new][od]*/,
                    const double* post_cov /*[(k_old+k_new)*od][(k_old+k_new)*od]*/, obvi_map** out);

int obvi_map_extend_on_handle(obvi_ba_handle* h, const obvi_map* map, int64_t k_old, const uint32_t* obj_idx_old /*[k_old]*/, const uint32_t* map_idx /*[k_old]*/,
                              int64_t k_new, const uint32_t* obj_idx_new /*[k_new]*/, obvi_map** out);

int obvi_map_select(obvi_ba_handle* h, const obvi_map* map, int64_t k, const uint32_t* map_idx /*[k]*/, obvi_map** out);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_MAP_EXTEND_H_ */
