/*
 * obvi_map_prior.h -- joint long-term-map priors on pairs of objects: the consumer of the cross covariances of obvi_cov.h.
 * Same library, same handle and status codes as obvi_ba.h (kept out of that header: the CPU oracle mirrors obvi_ba.h and does not know this factor).
 *
 * obvi_ba_set_ltm_priors (factor type 4) takes one independent Gaussian per object: the diagonal blocks of a map's covariance.  A pair prior
 * takes the joint covariance of two objects a, b
 *       C = [[A, B], [B^T, D]]     (2od x 2od, symmetric positive definite, row-major; od = obvi_ba_options.object_block_size)
 * and the means mu_a, mu_b.  Like type 4 it is linear in the raw parameters of the ellipsoid blocks (additive, no local parameterisation), with
 * a Huber loss on |r|^2.  With d = [x_a - mu_a ; x_b - mu_b]:
 *   OBVI_MAP_PAIR_JOINT        p(x_a, x_b):  r = C^-1/2 d  (2od entries), information Lambda = C^-1.
 *   OBVI_MAP_PAIR_CONDITIONAL  p(x_b | x_a): K = B^T A^-1, S_c = D - K B; the first od entries of r are zero, the last od are
 *                              S_c^-1/2 ((x_b - mu_b) - K (x_a - mu_a)); information Lambda = G^T S_c^-1 G, G = [-K, I] (rank od).
 * Either way the cost is rho(|r|^2) / 2, the Gauss-Newton blocks are w Lambda_aa, w Lambda_bb and w Lambda_ab, the gradient is w Lambda d
 * (w = rho': Huber's rho'' < 0, so the corrector is first order as for every other factor).
 *
 * Which form -- the caller's policy, two rules that do not count information twice:
 *   - a whole map factored along a tree of its objects: a type-4 prior (obvi_ba_set_ltm_priors) on the root and a CONDITIONAL pair prior on
 *     every edge (a = parent, b = child).  For a Gaussian that is Markov on the tree this is the exact joint density;
 *   - disjoint pairs: a JOINT pair prior INSTEAD of type-4 priors on the two objects (its diagonal blocks already hold them).
 *
 * n = 0 clears the factors, and so does obvi_ba_reset.  Refused before any device work: null arguments, a == b, the same unordered pair
 * twice, an unknown form (OBVI_ERR_INVALID_ARGUMENT); an index >= the object count (OBVI_ERR_OUT_OF_RANGE); C not symmetric positive
 * definite, or numerically singular: condition number of C, A or S_c above 1e13 (OBVI_ERR_NUMERICAL).  (One factor per unordered pair: the
 * object-object block of the reduced matrix then has one writer.)
 *
 * The factor type OBVI_FACTOR_MAP_PAIR_PRIOR is accepted wherever obvi_ba.h takes a factor type: obvi_ba_set_active_mask, obvi_ba_num_factors,
 * obvi_ba_select_outliers, obvi_ba_debug_linearize (r [n][2od], J0 = d r / d a [n][2od][od], J1 = d r / d b).  obvi_ba_evaluate appends the
 * residuals (2od per factor) and block norms after the relative-pose factors; obvi_ba_num_residuals counts them.  Constness follows types 4
 * and 5: a constant a leaves b's diagonal block and gradient (d still holds a's offset); both constant: the cost is part of the fixed cost.
 *
 * NOT COLLECTIVE BY DEFAULT: a handle that exchanges shared objects (obvi_ba_set_shared_objects and an exchange hook) refuses a problem that holds pair
 * priors with OBVI_ERR_INVALID_ARGUMENT before any collective is issued -- unless the caller switched the collective form on for that handle
 * (obvi_map_allow_exchange, obvi_map_shared.h, which states its calling rules: exactly one member uploads a given prior).
 */
#ifndef OBVI_MAP_PRIOR_H_
#define OBVI_MAP_PRIOR_H_

#include <stdint.h>

#include "obvi_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { OBVI_FACTOR_MAP_PAIR_PRIOR = 9 };   /* the reference's factor types end at 8 */
enum { OBVI_MAP_PAIR_JOINT = 0, OBVI_MAP_PAIR_CONDITIONAL = 1 };

int obvi_map_set_pair_priors(obvi_ba_handle* h, int64_t n, const uint32_t* obj_a, const uint32_t* obj_b,
                             const double* mean_a /*[n][od]*/, const double* mean_b /*[n][od]*/,
                             const double* cov_joint /*[n][2od*2od]*/, const uint8_t* form /*[n] or NULL = joint*/, double huber);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_MAP_PRIOR_H_ */
