/*
 * obvi_map_shared.h -- the device-resident map (obvi_map_resident.h) and CONCURRENT sessions (obvi_ba.h: obvi_ba_set_shared_objects, obvi_ba_set_allreduce): joint
 * map priors on a handle that exchanges shared objects, and the joint posterior folded back into the map by every member.  Same library, same handle and status
 * codes as obvi_ba.h.  This header includes obvi_map_resident.h; the entries it speaks of in words -- the two handle forms that bring a window back into a map,
 * the conditioning one and the growing one -- are declared in their own headers, which a caller of those entries includes beside this one.
 *
 * By default a handle that exchanges shared objects (an all-reduce hook and at least one shared object were set; decided from what was set, not from the plan)
 * refuses joint map priors on pairs and groups (factor types 9 and 10) when its problem is validated, and refuses both handle forms, before any collective.
 * obvi_map_allow_exchange(h, 1) switches the collective form on for that handle; 0 switches it off again.  The switch is a flag of the handle: no device call,
 * no plan is invalidated by it, obvi_ba_reset clears it.  A null handle or a value other than 0 / 1 is OBVI_ERR_INVALID_ARGUMENT.  With the switch off every
 * entry behaves as without this header, to the text of its messages.  The collective form carries calling rules that no single member can check; switching it
 * on is the caller's statement that it keeps them.
 *
 * ---- Pair and group priors (obvi_map_set_pair_priors, obvi_map_set_group_priors, obvi_map_set_group_priors_from_map) ----
 * The rule is the one of object-only factors and parameter priors on shared objects: EXACTLY ONE member uploads a given prior.  Its members may be shared
 * objects and private objects of the uploading member, in any mix (indices are per handle).  The same prior uploaded by two members counts twice, as two
 * factors would.  A pair prior uploaded by one member whose two objects lie inside a group uploaded by another member cannot be seen by either: the refusal
 * "a map pair prior whose two objects are members of one map group prior" tests one handle's own uploads only.  Not uploading such a pair is a calling rule.
 * Nothing new crosses the members:
 *   - the prior's diagonal blocks and gradient of shared members travel with the shared blocks (the first collective of a step);
 *   - its shared x shared off-diagonal blocks are entries of the tail and travel with it (the second collective);
 *   - its cost and trial cost travel with the scalars (the third), its fixed cost with the fixed-cost all-reduce of a solve's start;
 *   - shared x private blocks stay in the uploading member's own columns: they are eliminated there, before the tail is exchanged.
 * obvi_cov_compute and obvi_ba_object_covariances stay collective as obvi_cov.h states; a pair of objects coupled only by a prior is on the pattern
 * (obvi_cov_on_pattern), whether both are shared or one is private.  Declared pairs (obvi_cov_pairs.h) stay refused on a handle that exchanges.
 *
 * ---- The handle forms, collectively ----
 * With the switch on, the conditioning and the growing handle form run on a handle that exchanges, the birth of a first map (map = NULL) included.
 *   - The posterior is the JOINT one: the four-collective sequence of obvi_ba_object_covariances (tail-order proof, shared blocks, tail, scalars) runs, issued
 *     once by every member of the job.  EVERY member enters together, as for every collective entry.
 *   - A member names shared objects and its own private objects.  Each calling member gets its own new map; the update itself is local and is the one the
 *     single-handle forms compute, to the last bit, for the same posterior.
 *   - A member with nothing to fold joins the pass through obvi_ba_object_covariances (n_pairs = 0 is allowed), whose sequence is the same.
 *   - Members that pass the same shared objects in the same order get equal maps; bit-identical where the sum across members is order-fixed (deterministic
 *     handles behind the compiled group of obvi_rccl.h, which sums in member order).
 *   - Rank-deficient normal equations on ONE member are OBVI_ERR_NUMERICAL on EVERY member, from the same call.
 *   - Argument errors a member sees before the first collective (null pointers, indices out of range, an object twice, a constant session object, a map of
 *     another device or block size, too many rows) return there at once, with the messages of the single-handle forms; the other members leave through the
 *     group's time-out.  This is the rule of every collective entry.  "An object that no active factor touches" is found after planning and before the first
 *     collective, and follows the same rule.
 * The host-pointer forms, the gather and the read-back of a map never look at the handle's exchange: they need no switch and are not changed by it.
 */
#ifndef OBVI_MAP_SHARED_H_
#define OBVI_MAP_SHARED_H_

#include <stdint.h>

#include "obvi_map_resident.h"

#ifdef __cplusplus
extern "C" {
#endif

int obvi_map_allow_exchange(obvi_ba_handle* h, int32_t on /* 0 / 1; default 0 */);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_MAP_SHARED_H_ */
