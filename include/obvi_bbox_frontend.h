/*
 * obvi_bbox_frontend.h -- C ABI of the bounding-box data association that sits between a detector and the object side of the
 * bundle-adjustment path: which object does a detected bounding box belong to.  A box is matched to the object whose earlier
 * boxes contained the same visual features.
 *
 * Reference (the reference's include/refactoring/bounding_box_frontend/):
 *   bounding_box_front_end.h:941-985                      getBoundingBoxAssignments: one (frame, camera) round
 *   feature_based_bounding_box_front_end.h:190-209        generateSingleBoundingBoxContextInfo: the features inside the inflated box
 *                                                         (inflateBoundingBox / pixelInBoundingBoxClosedSet, types/ellipsoid_utils.h:347-361)
 *   feature_based_bounding_box_front_end.h:917-940        getMaxFeatureIntersection: |box set n view set| for every earlier view of a candidate
 *   feature_based_bounding_box_front_end.h:357-420        pruneCandidateMatches: same class, largest intersection >= min_overlapping_features_for_match
 *   feature_based_bounding_box_front_end.h:423-479        scoreCandidateMatch: mean over the candidate's views of intersection over union
 *   bounding_box_front_end_helpers.h:125-184              greedilyAssignBoundingBoxes
 * The stateful part (which views an object keeps, pending objects, merges) is host logic.
 *
 * Conventions as in obvi_frontend.h: host pointers owned by the caller, 0 / negative obvi_status, nothing throws.  The handle
 * supplies the device and the stream; the calls do not touch the bundle-adjustment state.  Default and deterministic handles
 * compute the same bytes: the only atomics are integer counts.
 *
 * Two corners the reference leaves undefined are defined here:
 *   - a candidate with no views is not a match (the reference divides 0 by 0 there once min_overlapping_features_for_match <= 0);
 *   - the reference sums a candidate's intersection-over-union terms in the order of its hash maps; here the sum runs over the
 *     candidate's views in the order of view_ptr.
 */
#ifndef OBVI_BBOX_FRONTEND_H_
#define OBVI_BBOX_FRONTEND_H_

#include <stdint.h>

#include "obvi_frontend.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  double bounding_box_inflation_size;            /* px added on every side of a box before the membership test (:199-200) */
  double min_overlapping_features_for_match;     /* a double, as in the reference: the test is (double)count >= this (:408-411) */
} obvi_bbox_frontend_params;

/* One (frame, camera) round of getBoundingBoxAssignments up to, not including, the assignment.
 *   features   the camera's observed features in this frame: feat_id[n_feat] unique, in any order; feat_pixel[n_feat][2]
 *   boxes      the filtered boxes: box_corners[n_box][4] as (min_x, max_x, min_y, max_y) px -- the order of obvi_ba_set_bbox_factors --,
 *              box_label[n_box] the class id
 *   candidates pending objects first, then initialised ones, in the caller's order: cand_label[n_cand]
 *   views      candidate c owns the views [view_ptr[c], view_ptr[c+1]) (view_ptr[n_cand] == n_views); view k holds the feature ids
 *              view_feat[feat_ptr[k] .. feat_ptr[k+1]) (feat_ptr[n_views] == n_view_feat), unique within a view
 * Outputs (any may be NULL):
 *   in_box[n_box][n_feat]      1 where the feature's pixel lies in the closed inflated box, feats_in_box[n_box] their number
 *   overlap[n_box][n_views]    |features in box b  n  features of view k| (test hook)
 *   is_match[n_box][n_cand]    labels equal, at least one view, and the largest overlap over the candidate's views >= min_overlapping_features_for_match
 *   score[n_box][n_cand]       written ONLY where is_match is 1: (sum over views with n_k != 0 of n_k / (feats_in_box + |view_k| - n_k)) / number of views
 * Refused before any device work, outputs untouched: a NULL handle, params, view_ptr or feat_ptr, a NULL array of a non-zero count,
 * negative counts, offsets that do not start at 0, decrease or end elsewhere than the length given, non-finite box corners or
 * parameters (OBVI_ERR_NUMERICAL), a feature id that occurs twice in feat_id.  The other arguments are judged before the handle is looked at.
 * Counts of 0 are valid. */
int obvi_bbox_frontend_associate(obvi_ba_handle* h, int64_t n_feat, const uint64_t* feat_id, const double* feat_pixel, int64_t n_box,
                                 const double* box_corners, const int32_t* box_label, int64_t n_cand, const int32_t* cand_label,
                                 int64_t n_views, const uint64_t* view_ptr, int64_t n_view_feat, const uint64_t* feat_ptr,
                                 const uint64_t* view_feat, const obvi_bbox_frontend_params* params, uint8_t* in_box,
                                 uint32_t* feats_in_box, uint32_t* overlap, uint8_t* is_match, double* score);

/* The largest n_feat at which the overlap pass keeps the frame's sorted id list in LDS; above it the list is searched in global
 * memory.  Exported so that tests can stand on both sides of it. */
int64_t obvi_bbox_frontend_lds_feature_limit(void);

/* greedilyAssignBoundingBoxes.  Host only: no handle, no device.  The pairs with is_match[b][c] != 0 are ordered by score, descending
 * (the reference's std::sort leaves ties unspecified; here a tie goes by box index, then by candidate index); going down that list a
 * box without an assignment takes the candidate unless another box has claimed it.  A box left over opens a new pending object,
 * numbered from n_pending (the size of the caller's pending list) upwards in box order.
 *   assigned_cand[n_box]   the candidate index of a matched box; the number of the new pending object otherwise
 *   is_new[n_box]          1 for a box that opens a new pending object
 * Scores are read only where is_match is set; a NaN there is refused (OBVI_ERR_NUMERICAL).  Refusals leave the outputs untouched. */
int obvi_bbox_frontend_assign(int64_t n_box, int64_t n_cand, int64_t n_pending, const uint8_t* is_match, const double* score,
                              int64_t* assigned_cand, uint8_t* is_new);

#ifdef __cplusplus
}
#endif
#endif /* OBVI_BBOX_FRONTEND_H_ */
