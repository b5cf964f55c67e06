/*
 * obvi_map_group_prior.h -- joint long-term-map priors on GROUPS of objects: the whole map as one Gaussian.
 * Same library, same handle and status codes as obvi_ba.h; the follow-up of obvi_map_prior.h (pairs), which this header includes.
 *
 * obvi_ba_object_covariances returns the block of every object pair, and the joint covariance of a session's objects is dense: every object
 * carries the trajectory's common drift.  A tree of conditional pair priors is exact only for a map that is Markov on that tree, disjoint joint
 * pairs throw the rest of Sigma_oo away.  A group prior takes the joint covariance of k objects o_0 .. o_{k-1}
 *       C   (k od x k od, symmetric positive definite, row-major, members in the order given; od = obvi_ba_options.object_block_size)
 * and their means.  Like types 4 and 9 it is linear in the raw parameters of the ellipsoid blocks, with a Huber loss on |r|^2:
 *       d = [x_o - mu_o] over the members,  Lambda = C^-1,  r = W d with W^T W = Lambda,
 * W the inverse of the lower Cholesky factor of C (lower triangular).  The cost is rho(|r|^2) / 2, the Gauss-Newton blocks are w Lambda_ab for every
 * member pair, the gradient is w Lambda d (w = rho', first-order corrector as for every other factor).  The Huber conventions are those of type 9.
 *
 * Policy (the caller's): a group prior holds the members' diagonal blocks, so it is given INSTEAD of type-4 priors on its members and instead of
 * pair priors among them.  A group of two equals a joint pair prior.
 *
 * Groups: group g holds the objects obj_idx[group_ptr[g] .. group_ptr[g + 1]), its means are the rows [group_ptr[g], group_ptr[g + 1]) of `mean`, and
 * `cov` holds the groups' matrices one after the other, (k_g od)^2 doubles each.  C is symmetrised ((C + C^T) / 2) as for the other priors.
 * A group has at most OBVI_MAP_GROUP_MAX_ROWS = 2048 rows (k_g od): 200 objects at either block size.
 *
 * n_groups = 0 clears the factors, and so does obvi_ba_reset.  Refused before any device work: null arguments, a group_ptr that does not start at 0
 * or decreases, an empty group, an object twice in one group or in two groups -- groups are disjoint, so every object-object block of the reduced matrix
 * has one writer among the groups -- and a group above the cap (OBVI_ERR_INVALID_ARGUMENT); an index >= the object count (OBVI_ERR_OUT_OF_RANGE);
 * C or a mean not finite, C not positive definite, or numerically singular: the squared ratio of the largest to the smallest Cholesky pivot, or the
 * condition number estimated from the largest eigenvalues of C and of C^-1, above 1e13 (OBVI_ERR_NUMERICAL).  A refused call leaves the handle's groups as they were.
 * Refused when the problem is validated (obvi_ba_prepare, obvi_ba_solve, obvi_ba_evaluate, ...; the set calls come in any order), with
 * OBVI_ERR_INVALID_ARGUMENT: a pair prior (obvi_map_prior.h) whose two objects are members of one group -- the block would have two writers, and the
 * information would count twice.
 *
 * The factor type OBVI_FACTOR_MAP_GROUP_PRIOR is accepted wherever obvi_ba.h takes a factor type: obvi_ba_set_active_mask (a flag per group),
 * obvi_ba_num_factors, obvi_ba_select_outliers (on |r|^2, as type 4), obvi_ba_debug_linearize (r concatenated over the groups, J0 = W of every group
 * one after the other, (k_g od)^2 doubles each, row-major; J1 unused).  obvi_ba_evaluate appends the residuals (k_g od per group) and one block norm per
 * group after the pair priors; obvi_ba_num_residuals counts them.  Constness follows types 4, 5 and 9: a constant member contributes no rows or columns
 * (d still holds its offset); all members constant: the cost is part of the fixed cost; a member that only a group prior touches is a variable.
 * The members of active groups are eliminated last, group after group in the caller's order.
 *
 * NOT COLLECTIVE BY DEFAULT: a handle that exchanges shared objects (obvi_ba_set_shared_objects and an exchange hook) refuses a problem that holds group
 * priors with OBVI_ERR_INVALID_ARGUMENT before any collective is issued -- unless the caller switched the collective form on for that handle
 * (obvi_map_allow_exchange, obvi_map_shared.h, which states its calling rules: exactly one member uploads a given prior).  Not built: a conditional form for groups.
 */
#ifndef OBVI_MAP_GROUP_PRIOR_H_
#define OBVI_MAP_GROUP_PRIOR_H_

#include <stdint.h>

#include "obvi_map_prior.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { OBVI_FACTOR_MAP_GROUP_PRIOR = 10 };
enum { OBVI_MAP_GROUP_MAX_ROWS = 2048 };

int obvi_map_set_group_priors(obvi_ba_handle* h, int64_t n_groups, const int64_t* group_ptr /*[n_groups+1]*/, const uint32_t* obj_idx /*[group_ptr[n]]*/,
                              const double* mean /*[group_ptr[n]][od]*/, const double* cov /* group after group, (k_g*od)^2 row-major */, double huber);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_MAP_GROUP_PRIOR_H_ */
