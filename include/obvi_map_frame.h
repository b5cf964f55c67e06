/*
 * obvi_map_frame.h -- a device-resident map (obvi_map_resident.h) brought into another frame under a transform that is itself an estimate, and two maps
 * joined into one, on the device.  Same library, same handle and status codes as obvi_ba.h; this header includes obvi_map_resident.h, never the reverse.
 *
 * Every other entry of the map assumes that all estimates are expressed in one frame.  Two sessions each start at their own origin, and a map written by one
 * robot is not in the frame of another.  Moving map B into map A's frame under an uncertain transform correlates every object of B through that transform;
 * after a join, the entry that proposes duplicates and the entry that fuses them pull all of B into place from a few duplicate pairs -- objects that have no
 * duplicate included: the covariance does the work.
 *
 * The map is x ~ N(mu, C) over n objects, Cs = (C + C^T) / 2, N = n od rows.  T = T_new<-old is `transform` [dT], Sigma_s = (Sigma + Sigma^T) / 2 with Sigma =
 * transform_cov [dT][dT], row-major, in the order of `transform` (NULL: T is exact).  T's error is taken to be independent of the map.
 *   od 7, block (x y z yaw dx dy dz), dT = 4: transform = (tx ty tz psi).  p' = Rz(psi) p + t, yaw' = yaw + psi -- not wrapped; the yaw period of the entry
 *     that proposes duplicates exists for that -- the dimensions unchanged.  J_o = blockdiag(Rz(psi), 1, I3) for every object; G_o = d x'_o / d(t, psi), 7 x 4:
 *     I3 and Rz'(psi) p_o in the centre rows, (0 0 0 1) in the yaw row, zeros in the dimension rows.
 *   od 9, block (x y z ax ay az dx dy dz), dT = 6: transform = (tx ty tz ax ay az), the library's pose convention (translation, axis-angle).  p' = R_T p + t,
 *     aa' = Log(R_T Exp(aa)) with the angle of the rotation log in [0, pi], the dimensions unchanged.  J_o = blockdiag(R_T, d aa' / d aa, I3); G_o, 9 x 6: I3
 *     and d(R_T p_o) / d a in the centre rows, d aa' / d a in the rotation rows, zeros in the dimension rows.  Derivatives are taken with respect to additive
 *     changes of the axis-angle vectors, as everywhere in the estimator, and of the exponential map itself: they are smooth through a = 0 and aa = 0.  They
 *     are not smooth where the composed angle reaches pi.
 *       mu'_o = g(T, mu_o)                        C' = Jt Cs Jt^T + G Sigma_s G^T,     Jt = blockdiag(J_o),  G the stacked G_o
 * This is first order in the rotation part of T; no second-order correction of the means is applied.
 *
 * obvi_map_transform builds a NEW map on the map's device.  `map` is not written and may be destroyed before or after the new one.  The new map has the same
 * n, the same object numbers and the same block size; it is exactly symmetric; it is a map like any other, usable by any handle of the device from any thread
 * once the call has returned (the call's one wait, for a status record of a few doubles).  Its power-step start vector is the old map's.
 * Exact, bit for bit: every entry of C' whose row and whose column are both dimension parameters equals Cs there, with or without Sigma; for od 7 with
 * psi = 0 and Sigma NULL, C' = Cs, the centres are p + t (each sum rounded once) and everything else of the means is unchanged.
 *
 * obvi_map_join builds a NEW map of n_a + n_b objects: mu' = (mu_a, mu_b), C' = blockdiag(C_a, C_b).  Entries are copied exactly as the device holds them:
 * nothing is symmetrised, as in the gather entry.  a's objects keep their numbers, b's follow as n_a, n_a + 1, ...  The power-step start vector is a's.  One
 * wait.  a == b is allowed (the entry that proposes duplicates will count the copies singular).  Neither a nor b is written; either may be destroyed before or
 * after the new map.  Nothing is factored: there is no row limit but the map's own 1 GiB.
 *
 * What `h` lends: its device, stream, workspaces and obvi_ba_last_error.  The handle is left exactly as it was: its problem, its estimate, its group priors
 * and its covariance results.
 *
 * Refused before any launch or device allocation (*out = NULL on every failure) --
 *   obvi_map_transform: OBVI_ERR_INVALID_ARGUMENT: null h, map, transform or out; a map on another device or of another block size than the handle's.
 *     OBVI_ERR_NUMERICAL: a non-finite entry of transform or transform_cov.
 *   obvi_map_join: OBVI_ERR_INVALID_ARGUMENT: null h, a, b or out; a map on another device or of another block size than the handle's (so two maps that
 *     differ in either); a result above the 1 GiB the create entry of obvi_map_resident.h accepts.
 * Refused from what the device reports (obvi_map_transform; OBVI_ERR_NUMERICAL, nothing left allocated): a non-finite entry in the result.
 * NOT checked: neither Sigma nor the result are tested for positive semi-definiteness.
 *
 * No sum depends on the order in which workgroups run: the same call twice gives bit-identical maps, on default and deterministic handles alike.
 */
#ifndef OBVI_MAP_FRAME_H_
#define OBVI_MAP_FRAME_H_

#include <stdint.h>

#include "obvi_map_resident.h"

#ifdef __cplusplus
extern "C" {
#endif

int obvi_map_transform(obvi_ba_handle* h, const obvi_map* map, const double* transform /*[dT]*/, const double* transform_cov /*[dT][dT] or NULL: exact*/,
                       obvi_map** out);

int obvi_map_join(obvi_ba_handle* h, const obvi_map* a, const obvi_map* b, obvi_map** out);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_MAP_FRAME_H_ */
