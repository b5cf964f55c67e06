/*
 * obvi_bbox_store.h -- the appearance store of the bounding-box data association: the views of obvi_bbox_frontend.h kept on the device between rounds.
 *
 * obvi_bbox_frontend_associate is stateless: every round the caller flattens every view of every candidate and the library uploads all of it.  A store keeps the
 * feature ids of the views in one device array (the pool) and a directory of the views on the host; a round then uploads the frame, the boxes and 16 bytes per
 * listed view, and the view a round leaves behind -- the frame features inside the assigned box -- is cut out of what the round already has on the device.
 *
 * Reference (include/refactoring/bounding_box_frontend/feature_based_bounding_box_front_end.h):
 *   :211-242   createObjectInfoFromSingleBb                    a box opens an owner with one view
 *   :244-273   mergeObjectAssociationInfo                      merge: into[v.first] = v.second for every view of the merged owner
 *   :275-304   mergeSingleBbContextIntoObjectAssociationInfo   a box gives its owner the view (frame, camera)
 *   :506-592   cleanupBbAssociationRound                       discarded owners, the feature validity window
 *
 * Conventions as in obvi_bbox_frontend.h: host pointers owned by the caller, 0 / negative obvi_status, nothing throws; a refusal or a failure leaves the caller's
 * outputs and the store as they were.  A NULL store or a NULL required pointer is OBVI_ERR_INVALID_ARGUMENT, answered before anything else is looked at.  A store
 * belongs to one handle (its device and its stream) and must be destroyed before it; it is not thread-safe.  Default and deterministic handles compute the same
 * bytes: nothing is summed in floating point across threads, and the append is ordered.
 *
 * An OWNER is whatever owns views: a pending object or an object.  The store hands out owner tokens, ascending from 0 and never reused.  A VIEW of an owner is
 * keyed by (frame_id, camera_id) and holds a list of unique feature ids, possibly none (an empty view still counts in the divisor of the score).  An owner's views
 * are always enumerated in ascending (frame, camera) order; that is the order the score is summed in.
 *
 * The pool is append-only and starts at initial_pool_ids entries.  An append that does not fit doubles the capacity until it does (one growth: a new array, a
 * device-to-device copy, the old one freed).  A view that is replaced, dropped by the window, merged over or released leaves its ids behind as dead ids.  After
 * every mutating call that succeeded (put_views, commit, merge, release, apply_window), if dead_ids >= compact_min_dead_ids and dead_ids > live_ids, the live
 * views are copied into a fresh array of the same capacity, in directory order (owner token, then key): dead_ids becomes 0.  obvi_bbox_store_compact does the
 * same unconditionally.  The rule is part of the interface: a caller can predict every field of obvi_bbox_store_stats.
 */
#ifndef OBVI_BBOX_STORE_H_
#define OBVI_BBOX_STORE_H_

#include <stdint.h>

#include "obvi_bbox_frontend.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct obvi_bbox_store obvi_bbox_store;

typedef struct {
  int64_t initial_pool_ids;        /* capacity of the pool at creation; 0: 65536 */
  int64_t compact_min_dead_ids;    /* no automatic compaction below this many dead ids; 0: 65536 */
} obvi_bbox_store_options;

typedef struct {
  int64_t owners, views;           /* live owners and their views */
  int64_t live_ids, dead_ids;      /* pool entries of live views / left behind; live_ids + dead_ids entries of the pool are in use */
  int64_t pool_capacity_ids, pool_growths, compactions;
  int64_t replaced_views;          /* views that put_views or commit wrote over an existing key */
  int64_t last_round_upload_bytes; /* host-to-device bytes of the last successful associate: 32 n_feat + 36 n_box + 4 n_cand + 8 (n_cand + 1) + 16 n_views
                                      (ids 8, pixels 16 and two permutations 4 + 4 per feature; corners 32 and label 4 per box; label and view_ptr per candidate;
                                      offset and length per listed view), 0 when n_box is 0.  It does not depend on how many ids the views hold. */
} obvi_bbox_store_stats;

/* opt NULL or a field 0: the defaults.  Refused: negative options.  *out is written on success only. */
int obvi_bbox_store_create(obvi_ba_handle* h, const obvi_bbox_store_options* opt, obvi_bbox_store** out);
void obvi_bbox_store_destroy(obvi_bbox_store* s);   /* NULL is a no-op */

/* n new owners without views; their tokens in owner_out[n]. */
int obvi_bbox_store_new_owners(obvi_bbox_store* s, int64_t n, int64_t* owner_out);

/* Views from the host: view k belongs to owner[k], has the key (frame[k], camera[k]) and the ids view_feat[feat_ptr[k] .. feat_ptr[k + 1]).  A view whose key the
 * owner already has replaces the old one.  Refused: the same (owner, key) twice in one call, an id twice within a view, an unknown or released owner, feat_ptr
 * that does not start at 0 or decreases. */
int obvi_bbox_store_put_views(obvi_bbox_store* s, int64_t n_views, const int64_t* owner, const uint64_t* frame, const uint64_t* camera, const uint64_t* feat_ptr,
                              const uint64_t* view_feat);

/* The round of obvi_bbox_frontend_associate over the stored views of the candidates cand_owner[n_cand], in the caller's candidate order: candidate c owns the
 * columns [sum of the view counts of the candidates before it, + its own) of overlap[n_box][n_views], in (frame, camera) order; n_views is the sum of the
 * candidates' view counts (obvi_bbox_store_views tells them).  Outputs, "any may be NULL" and "score written only where is_match is 1" as there; so are its
 * refusals.  Also refused: an unknown or released owner, an owner listed twice.  On success the store keeps the round on the device (the bit rows, the ids, the
 * permutations between the caller's and the sorted feature order) until the next associate or commit.  A refused call leaves an earlier round kept; a call that
 * fails on the device drops it. */
int obvi_bbox_store_associate(obvi_bbox_store* s, int64_t n_feat, const uint64_t* feat_id, const double* feat_pixel, int64_t n_box, const double* box_corners,
                              const int32_t* box_label, int64_t n_cand, const int64_t* cand_owner, const int32_t* cand_label, const obvi_bbox_frontend_params* params,
                              uint8_t* in_box, uint32_t* feats_in_box, uint32_t* overlap, uint8_t* is_match, double* score);

/* Gives owner box_owner[b] the view (frame_id, camera_id) holding the ids of the frame features inside box b's inflated rectangle in the kept round, in the
 * caller's feature order of that round; box_owner[b] == -1: the box leaves no view.  An existing view of that key is replaced.  Refused: no kept round, n_box
 * other than the round's, an owner twice, an unknown or released owner.  Consumes the kept round. */
int obvi_bbox_store_commit(obvi_bbox_store* s, uint64_t frame_id, uint64_t camera_id, int64_t n_box, const int64_t* box_owner);

/* Moves the views of from[i] into into[i], pair by pair in list order; where both hold a key, from's view stays.  from[i] is then released.  Refused, and nothing
 * applied: from[i] == into[i], an owner unknown, released before the call or released earlier in the list. */
int obvi_bbox_store_merge(obvi_bbox_store* s, int64_t n, const int64_t* from, const int64_t* into);

/* Drops the owners and their views.  Refused: an unknown or released owner, an owner twice. */
int obvi_bbox_store_release(obvi_bbox_store* s, int64_t n, const int64_t* owner);

/* Drops every view with view_frame + window < frame_id, evaluated in uint64_t arithmetic (the sum wraps).  *dropped (may be NULL): their number. */
int obvi_bbox_store_apply_window(obvi_bbox_store* s, uint64_t frame_id, uint64_t window, int64_t* dropped);

/* The compaction, now. */
int obvi_bbox_store_compact(obvi_bbox_store* s);

/* The owner's views in (frame, camera) order: *n_views, *n_ids (the total length), frame[n_views], camera[n_views], feat_ptr[n_views + 1], view_feat[n_ids].
 * Every output may be NULL.  With view_feat NULL the answer comes from the host directory: no device work. */
int obvi_bbox_store_views(const obvi_bbox_store* s, int64_t owner, int64_t* n_views, int64_t* n_ids, uint64_t* frame, uint64_t* camera, uint64_t* feat_ptr,
                          uint64_t* view_feat);

int obvi_bbox_store_get_stats(const obvi_bbox_store* s, obvi_bbox_store_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_BBOX_STORE_H_ */
