// obvi_bounding_box_front_end.h -- host-side mirror of the reference's feature-based bounding-box front end: the stateful sequence that turns the detections
// of a (frame, camera) into object observation factors of the pose graph.  Header only.  Reference (include/refactoring/bounding_box_frontend/):
//   addBoundingBoxObservations                 bounding_box_front_end.h:78-323           the sequence of one round
//   filterBoundingBoxes                        feature_based_bounding_box_front_end.h:172-188, helpers.h:9-24 (confidence strictly above the minimum)
//   identifyCandidateMatches                   :317-353   pending objects first, then the objects of the pose graph
//   prune / score / assign                     :355-490   ONE obvi_bbox_frontend_associate call on the device and obvi_bbox_frontend_assign (include/obvi_bbox_frontend.h)
//   appearance bookkeeping                     :211-304   createObjectInfoFromSingleBb, mergeObjectAssociationInfo, mergeSingleBbContextIntoObjectAssociationInfo
//   setupInitialEstimateGeneration             :594-672
//   tryInitializeEllipsoid                     :674-692
//   searchForObjectMerges                      :742-843   with identifyMergeCandidates (bounding_box_front_end_helpers.h:29-123)
//   mergePending, mergeExistingPendingObjects  bounding_box_front_end.h:438-468, :694-740
//   cleanupBbAssociationRound                  :506-592   stale pending objects (helpers.h:186-202), the feature validity window
//   generateSingleViewEllipsoidEstimate        helpers.h:204-264 (the CONSTRAIN_ELLIPSOID_ORIENTATION branch: yaw 0)
//   covariance generator, distance scorer      bounding_box_front_end_creation_utils.h:55-102, :176-205
// The three std::function hooks of the reference stay hooks: the covariance generator (default: the edge-variance one), the geometric similarity scorer
// (default: the centre distance) and the refinement of pending estimates (default: refineInitialEstimateForPendingObjects of obvi_pending_object_estimator.h).
// Where the reference walks an unordered container and the order shows in the result, the order is defined here: candidates are the pending objects in list
// order, then the pose graph's objects in ascending id; an object's views are kept in ascending (frame, camera) order, which is the order its score is summed
// in; mergeable pending objects, their merge candidates and the pending objects that become new objects are visited in ascending id, and equal merge scores go
// by (pending index, object id).
// Store mode (useAppearanceStore, opt-in, before the first round): the views live in an obvi_bbox_store (include/obvi_bbox_store.h) on the device instead of
// observed_feats_ / object_appearance_info_, which stay empty; a pending object and an object carry an owner token of the store.  The sequence, the order of the
// views and the events are the same.
#ifndef OBVI_HOST_BOUNDING_BOX_FRONT_END_H_
#define OBVI_HOST_BOUNDING_BOX_FRONT_END_H_

#include <obvi_bbox_frontend.h>
#include <obvi_bbox_store.h>

#include <algorithm>
#include <climits>
#include <functional>
#include <iostream>
#include <map>
#include <memory>
#include <optional>
#include <set>
#include <string>
#include <tuple>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "obvi_pending_object_estimator.h"
#include "obvi_pose_graph.h"
#include "obvi_types.h"

namespace vslam_types_refactor {

static const FrameId kNoBbDiscardingConst = (FrameId)INT_MIN;   // :42, :52: INT_MIN in an unsigned FrameId -- max_frame_id_ + it wraps to a frame no session reaches, so nothing is stale

struct RawBoundingBox {                           // bounding_box_front_end.h / vslam_obj_opt_types_refactor.h
  std::string semantic_class_;
  std::pair<PixelCoord, PixelCoord> pixel_corner_locations_;   // (min_x, min_y), (max_x, max_y)
  double detection_confidence_ = 1.0;
};
inline BbCorners cornerLocationsPairToVector(const std::pair<PixelCoord, PixelCoord>& c) { return BbCorners{{c.first[0], c.second[0], c.first[1], c.second[1]}}; }

struct FeatureBasedBbAssociationParams {          // feature_based_bounding_box_front_end.h:50-63
  uint16_t min_observations_for_local_est_ = 3;
  uint16_t min_observations_ = 10;
  FrameId discard_candidate_after_num_frames_ = kNoBbDiscardingConst;
  double min_bb_confidence_ = 0.3;
  double required_min_conf_for_initialization_ = 0;
  double min_overlapping_features_for_match_ = 2;
  FrameId feature_validity_window_ = INT_MAX;
  PendingObjectEstimatorParams pending_obj_estimator_params_;
  double bounding_box_inflation_size_ = 0;
};
struct BoundingBoxCovGenParams {                  // bounding_box_front_end_creation_utils.h:14-30
  Covariance<4> bounding_box_cov_{{30.0 * 30.0, 0, 0, 0, 0, 30.0 * 30.0, 0, 0, 0, 0, 30.0 * 30.0, 0, 0, 0, 0, 30.0 * 30.0}};
  double near_edge_threshold_ = 25;
  double image_boundary_variance_ = 200.0 * 200.0;
};
struct GeometricSimilarityScorerParams {          // :32-53
  double max_merge_distance_ = 4;
  bool x_y_only_merge_ = true;
};

// the frame's observed features, in the caller's order (FeatureBasedContextInfo::observed_features_)
struct FeatureBasedContextInfo { std::vector<std::pair<FeatureId, PixelCoord>> observed_features_; };

typedef std::map<std::pair<FrameId, CameraId>, std::vector<FeatureId>> ObservedFeats;   // FeatureBasedFrontEndObjAssociationInfo::observed_feats_
struct FeatureBasedPendingObject {                // UninitializedEllispoidInfo<FeatureBasedFrontEndObjAssociationInfo, FeatureBasedFrontEndPendingObjInfo>
  ObservedFeats observed_feats_;
  double max_confidence_ = 0;
  std::optional<RawEllipsoid> object_estimate_;
  bool ready_for_merge = false;
  std::string semantic_class_;
  std::vector<ObjectObservationFactor> observation_factors_;   // object_id_ unused while pending
  FrameId min_frame_id_ = 0, max_frame_id_ = 0;
  int64_t store_owner_ = -1;                      // store mode: the owner token of its views (observed_feats_ stays empty)
};
struct AssociatedObjectIdentifier { bool initialized_ellipsoid_; ObjectId object_id_; };   // bounding_box_front_end.h:37-44
enum ObjectInitializationStatus { NOT_INITIALIZED, ENOUGH_VIEWS_FOR_MERGE, SUFFICIENT_VIEWS_FOR_NEW };

typedef std::function<Covariance<4>(const RawBoundingBox&, const FrameId&, const CameraId&, const FeatureBasedContextInfo&)> BbCovarianceGenerator;
typedef std::function<bool(const RawEllipsoid&, const RawEllipsoid&, double&)> GeometricSimilarityScorer;
// rough estimates and the pending objects they belong to, by pending index -> refined estimates (those left out keep their estimate)
typedef std::function<std::unordered_map<ObjectId, RawEllipsoid>(const std::unordered_map<ObjectId, RawEllipsoid>&, const std::unordered_map<ObjectId, FeatureBasedPendingObject>&,
                                                                 const FrameId&, const CameraId&)> PendingEstimateRefiner;

inline BbCovarianceGenerator getBoundingBoxCovarianceGenerator(const std::unordered_map<CameraId, std::pair<double, double>>& img_heights_and_widths,
                                                               const BoundingBoxCovGenParams& p) {   // creation_utils.h:55-102
  return [img_heights_and_widths, p](const RawBoundingBox& bb, const FrameId&, const CameraId& camera_id, const FeatureBasedContextInfo&) {
    Covariance<4> cov = p.bounding_box_cov_;
    if (bb.pixel_corner_locations_.first[0] < p.near_edge_threshold_) cov[0] = p.image_boundary_variance_;
    if (bb.pixel_corner_locations_.first[1] < p.near_edge_threshold_) cov[10] = p.image_boundary_variance_;
    const auto hw = img_heights_and_widths.find(camera_id);
    if (hw != img_heights_and_widths.end()) {
      if (bb.pixel_corner_locations_.second[0] > hw->second.second - p.near_edge_threshold_) cov[5] = p.image_boundary_variance_;
      if (bb.pixel_corner_locations_.second[1] > hw->second.first - p.near_edge_threshold_) cov[15] = p.image_boundary_variance_;
    }
    return cov;
  };
}
inline GeometricSimilarityScorer getDistanceSimilarityScorer(const GeometricSimilarityScorerParams& p) {   // creation_utils.h:176-205
  return [p](const RawEllipsoid& a, const RawEllipsoid& b, double& score) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = p.x_y_only_merge_ ? 0.0 : a[2] - b[2];
    const double dist = std::sqrt(dx * dx + dy * dy + dz * dz);
    if (dist > p.max_merge_distance_) return false;
    score = -1 * dist;
    return true;
  };
}

// helpers.h:204-264
template <class PoseGraphPtr>
inline bool generateSingleViewEllipsoidEstimate(const PoseGraphPtr& pose_graph, const FrameId& frame_id, const CameraId& camera_id, const std::string& semantic_class,
                                                const BbCorners& bb, RawEllipsoid& ellipsoid_est) {
  const auto& dims = pose_graph->shapePriorsBySemanticClass();
  const auto dim_it = dims.find(semantic_class);
  if (dim_it == dims.end()) { std::cerr << "Could not initialize; no mean dimension provided for class " << semantic_class << std::endl; return false; }
  const ObjectDim dim = dim_it->second.first;
  CameraIntrinsicsMat k{};
  pose_graph->getIntrinsicsForCamera(camera_id, k);
  const double depth = dim[2] * k.fy / (bb[3] - bb[2]);                                       // getObjectDepthGivenHeight
  const double u = (bb[0] + bb[1]) / 2, v = (bb[2] + bb[3]) / 2;
  const Position3d position_rel_cam{{depth * ((u - k.cx) / k.fx), depth * ((v - k.cy) / k.fy), depth}};
  const std::optional<RawPose3d> raw_robot_pose = pose_graph->getRobotPose(frame_id);
  if (!raw_robot_pose.has_value()) return false;
  CameraExtrinsics extrinsics;
  pose_graph->getExtrinsicsForCamera(camera_id, extrinsics);
  const Pose3D camera_pose = combinePoses(convertToPose3D(raw_robot_pose.value()), extrinsics);
  const Position3d g = combinePoseAndPosition(camera_pose, position_rel_cam);
  ellipsoid_est = RawEllipsoid{{g[0], g[1], g[2], 0.0, dim[0], dim[1], dim[2]}};
  return true;
}

template <class PoseGraph = ObjectAndReprojectionFeaturePoseGraph>
class FeatureBasedBoundingBoxFrontEnd {
 public:
  // `handle` supplies the device and the stream of the association round; its bundle-adjustment state is not touched
  FeatureBasedBoundingBoxFrontEnd(const std::shared_ptr<PoseGraph>& pose_graph, obvi_ba_handle* handle, const FeatureBasedBbAssociationParams& association_params,
                                  const BbCovarianceGenerator& covariance_generator, const GeometricSimilarityScorer& geometric_similarity_scorer,
                                  const PendingEstimateRefiner& refiner = PendingEstimateRefiner(), int device_id = 0)
      : pose_graph_(pose_graph), handle_(handle), association_params_(association_params), covariance_generator_(covariance_generator),
        geometric_similarity_scorer_(geometric_similarity_scorer), refiner_(refiner) {
    if (!refiner_) {
      refiner_ = [this, device_id](const std::unordered_map<ObjectId, RawEllipsoid>& rough, const std::unordered_map<ObjectId, FeatureBasedPendingObject>& infos, const FrameId& frame_id,
                                   const CameraId& camera_id) {
        std::unordered_map<ObjectId, UninitializedEllispoidInfo> slim;
        for (const auto& i : infos) slim[i.first] = UninitializedEllispoidInfo{i.second.semantic_class_, i.second.observation_factors_};
        std::unordered_map<ObjectId, RawEllipsoid> refined;
        if (!refineInitialEstimateForPendingObjects(rough, slim, pose_graph_, pose_graph_->shapePriorsBySemanticClass(), association_params_.pending_obj_estimator_params_, device_id,
                                                    &refined, nullptr, std::to_string(frame_id) + "_" + std::to_string(camera_id)))
          refined.clear();
        return refined;
      };
    }
  }
  FeatureBasedBoundingBoxFrontEnd(const FeatureBasedBoundingBoxFrontEnd&) = delete;
  FeatureBasedBoundingBoxFrontEnd& operator=(const FeatureBasedBoundingBoxFrontEnd&) = delete;
  ~FeatureBasedBoundingBoxFrontEnd() {
#if !defined(OBVI_TESTS_ORACLE_ABI_SHIM_H_) && !defined(OBVI_TESTS_LOCKSTEP_SHIM_H_)
    obvi_bbox_store_destroy(store_);             // before the handle, which the caller destroys after this object
#endif
  }

  // Store mode: from now on the views are kept in a store on the handle's device.  To be called before the first round and before
  // initializeWithLongTermMapFrontEndData; false when it comes later or the store cannot be made.
  bool useAppearanceStore(const obvi_bbox_store_options& options) {
#if !defined(OBVI_TESTS_ORACLE_ABI_SHIM_H_) && !defined(OBVI_TESTS_LOCKSTEP_SHIM_H_)
    if (store_ || !uninitialized_object_info_.empty() || !object_appearance_info_.empty()) return false;
    const int rc = obvi_bbox_store_create(handle_, &options, &store_);
    if (rc != 0) std::cerr << "obvi_bbox_store_create failed: status " << rc << " " << obvi_ba_last_error(handle_) << std::endl;
    return rc == 0;
#else
    (void)options;
    std::cerr << "the appearance store is served by libobvi_ba.so only" << std::endl;
    return false;
#endif
  }
  bool usesAppearanceStore() const { return store_ != nullptr; }

  // objects a long-term map brought: they are candidates once they have views (initializeWithLongTermMapFrontEndData: the map carries no appearance data)
  void initializeWithLongTermMapFrontEndData(const std::vector<ObjectId>& object_ids) {
    if (store_) { for (ObjectId o : object_ids) if (!object_owner_.count(o)) object_owner_[o] = newStoreOwner(); return; }
    for (ObjectId o : object_ids) object_appearance_info_[o];
  }

  bool addBoundingBoxObservations(const FrameId& frame_id, const CameraId& camera_id, const std::vector<RawBoundingBox>& bounding_boxes, const FeatureBasedContextInfo& bb_context) {
    last_assignments_.clear();
    CameraIntrinsicsMat intrinsics{};
    if (!pose_graph_->getIntrinsicsForCamera(camera_id, intrinsics)) { std::cerr << "No intrinsics found for camera with id " << camera_id << "; dropping bounding boxes for camera." << std::endl; return true; }
    CameraExtrinsics extrinsics;
    if (!pose_graph_->getExtrinsicsForCamera(camera_id, extrinsics)) { std::cerr << "No extrinsics found for camera with id " << camera_id << "; dropping bounding boxes for camera." << std::endl; return true; }
    std::vector<RawBoundingBox> boxes;                                                         // filterBoundingBoxes
    for (const RawBoundingBox& bb : bounding_boxes) if (bb.detection_confidence_ > association_params_.min_bb_confidence_) boxes.push_back(bb);

    std::vector<std::vector<FeatureId>> features_in_bb;
    std::vector<AssociatedObjectIdentifier> assignments;
    if (!getBoundingBoxAssignments(boxes, bb_context, &features_in_bb, &assignments)) return false;
    last_assignments_ = assignments;
    std::vector<int64_t> box_owner(assignments.size(), -1);                                     // store mode: whose view each box becomes

    for (size_t i = 0; i < assignments.size(); ++i) {                                          // bounding_box_front_end.h:137-202
      const RawBoundingBox& bb = boxes[i];
      const AssociatedObjectIdentifier& assoc = assignments[i];
      const Covariance<4> bb_cov = covariance_generator_(bb, frame_id, camera_id, bb_context);
      const BbCorners corners = cornerLocationsPairToVector(bb.pixel_corner_locations_);
      if (assoc.initialized_ellipsoid_) {
        addObservationForObject(frame_id, camera_id, assoc.object_id_, corners, bb_cov, bb.detection_confidence_);
        if (store_) box_owner[i] = object_owner_.at(assoc.object_id_);
        else object_appearance_info_[assoc.object_id_][{frame_id, camera_id}] = features_in_bb[i];
        continue;
      }
      ObjectObservationFactor factor;
      factor.frame_id_ = frame_id; factor.camera_id_ = camera_id; factor.object_id_ = 0; factor.bounding_box_corners_ = corners;
      factor.bounding_box_corners_covariance_ = bb_cov; factor.detection_confidence_ = bb.detection_confidence_;
      if (assoc.object_id_ >= uninitialized_object_info_.size()) {                             // createObjectInfoFromSingleBb :211-242
        FeatureBasedPendingObject fresh;
        fresh.semantic_class_ = bb.semantic_class_;
        fresh.observation_factors_.push_back(factor);
        if (store_) box_owner[i] = fresh.store_owner_ = newStoreOwner();
        else fresh.observed_feats_[{frame_id, camera_id}] = features_in_bb[i];
        fresh.max_confidence_ = bb.detection_confidence_;
        fresh.min_frame_id_ = fresh.max_frame_id_ = frame_id;
        RawEllipsoid est;
        if (generateSingleViewEllipsoidEstimate(pose_graph_, frame_id, camera_id, bb.semantic_class_, corners, est)) fresh.object_estimate_ = est;
        uninitialized_object_info_.push_back(fresh);
      } else {                                                                                  // mergeSingleBbContextIntoObjectAssociationInfo :275-304
        FeatureBasedPendingObject& p = uninitialized_object_info_[assoc.object_id_];
        p.observation_factors_.push_back(factor);
        p.max_frame_id_ = std::max(frame_id, p.max_frame_id_);
        p.min_frame_id_ = std::min(frame_id, p.min_frame_id_);
        p.max_confidence_ = std::max(p.max_confidence_, bb.detection_confidence_);
        if (store_) box_owner[i] = p.store_owner_;
        else p.observed_feats_[{frame_id, camera_id}] = features_in_bb[i];
        if (!p.object_estimate_.has_value()) {
          RawEllipsoid est;
          if (generateSingleViewEllipsoidEstimate(pose_graph_, frame_id, camera_id, bb.semantic_class_, corners, est)) p.object_estimate_ = est;
        }
      }
    }

    if (store_ && !commitStoreRound(frame_id, camera_id, box_owner)) return false;              // one commit carries the owners of all boxes

    if (!setupInitialEstimateGeneration(assignments, frame_id, camera_id)) return false;
    std::vector<ObjectId> added_pending_object_indices;
    std::unordered_set<ObjectId> existing_associated_to_objects;
    std::map<ObjectId, std::pair<ObjectInitializationStatus, RawEllipsoid>> mergable_objects_and_ests;
    for (const AssociatedObjectIdentifier& assoc : assignments) {                              // :220-251
      if (assoc.initialized_ellipsoid_) { existing_associated_to_objects.insert(assoc.object_id_); continue; }
      RawEllipsoid est{};
      const ObjectInitializationStatus status = tryInitializeEllipsoid(uninitialized_object_info_[assoc.object_id_], est);
      if (status == ENOUGH_VIEWS_FOR_MERGE || status == SUFFICIENT_VIEWS_FOR_NEW) mergable_objects_and_ests[assoc.object_id_] = {status, est};
    }
    std::vector<std::pair<ObjectId, ObjectId>> to_merge;
    std::vector<std::pair<ObjectId, RawEllipsoid>> to_add;
    searchForObjectMerges(mergable_objects_and_ests, existing_associated_to_objects, to_merge, to_add);
    const std::vector<ObjectId> merged = mergePending(to_merge);
    added_pending_object_indices.insert(added_pending_object_indices.end(), merged.begin(), merged.end());
    for (const auto& add_obj : to_add) {                                                       // :269-295
      const FeatureBasedPendingObject info = uninitialized_object_info_[add_obj.first];
      const ObjectId new_obj_id = pose_graph_->addNewEllipsoid(add_obj.second, info.semantic_class_);
      events_.push_back("new_object " + std::to_string(add_obj.first) + " " + std::to_string(new_obj_id));
      if (store_) object_owner_[new_obj_id] = info.store_owner_;                               // the token moves to the object: no store call
      else object_appearance_info_[new_obj_id] = info.observed_feats_;
      for (const ObjectObservationFactor& f : info.observation_factors_)
        addObservationForObject(f.frame_id_, f.camera_id_, new_obj_id, f.bounding_box_corners_, f.bounding_box_corners_covariance_, f.detection_confidence_);
      added_pending_object_indices.push_back(add_obj.first);
    }
    erasePending(added_pending_object_indices);
    erasePending(mergeExistingPendingObjects());
    cleanupBbAssociationRound(frame_id);
    return !store_failed_;
  }

  const std::vector<FeatureBasedPendingObject>& pendingObjects() const { return uninitialized_object_info_; }
  const std::map<ObjectId, ObservedFeats>& objectAppearanceInfo() const { return object_appearance_info_; }
  const std::vector<AssociatedObjectIdentifier>& lastAssignments() const { return last_assignments_; }
  // store mode: the owner tokens of the objects, an owner's views as (frame, camera, number of ids) in (frame, camera) order -- the host directory's answer, no
  // device work --, and the store's counters
  const std::map<ObjectId, int64_t>& objectStoreOwners() const { return object_owner_; }
  std::vector<std::tuple<FrameId, CameraId, size_t>> storedViewSizes(int64_t owner) const {
    std::vector<std::tuple<FrameId, CameraId, size_t>> out;
#if !defined(OBVI_TESTS_ORACLE_ABI_SHIM_H_) && !defined(OBVI_TESTS_LOCKSTEP_SHIM_H_)
    int64_t n_views = 0;
    if (!store_ || obvi_bbox_store_views(store_, owner, &n_views, nullptr, nullptr, nullptr, nullptr, nullptr) != 0) return out;
    std::vector<uint64_t> frame((size_t)n_views), camera((size_t)n_views), feat_ptr((size_t)n_views + 1);
    if (obvi_bbox_store_views(store_, owner, nullptr, nullptr, frame.data(), camera.data(), feat_ptr.data(), nullptr) != 0) return out;
    for (int64_t k = 0; k < n_views; ++k) out.emplace_back((FrameId)frame[k], (CameraId)camera[k], (size_t)(feat_ptr[k + 1] - feat_ptr[k]));
#else
    (void)owner;
#endif
    return out;
  }
  bool appearanceStoreStats(obvi_bbox_store_stats* stats) const {
#if !defined(OBVI_TESTS_ORACLE_ABI_SHIM_H_) && !defined(OBVI_TESTS_LOCKSTEP_SHIM_H_)
    return store_ && obvi_bbox_store_get_stats(store_, stats) == 0;
#else
    (void)stats;
    return false;
#endif
  }
  // what happened, in order: "open <pending>", "merge <pending> <object>", "new_object <pending> <object>", "discard <n>", "views_dropped <n>"
  std::vector<std::string> takeEvents() { std::vector<std::string> e; e.swap(events_); return e; }

 private:
  int32_t labelOf(const std::string& semantic_class) { return label_ids_.emplace(semantic_class, (int32_t)label_ids_.size()).first->second; }

  // ---- store mode: the calls on the store.  A failure is reported on stderr and fails the round (store_failed_).
  bool storeCall(int rc, const char* what) {
    if (rc == 0) return true;
#if !defined(OBVI_TESTS_ORACLE_ABI_SHIM_H_) && !defined(OBVI_TESTS_LOCKSTEP_SHIM_H_)
    std::cerr << what << " failed: status " << rc << " " << obvi_ba_last_error(handle_) << std::endl;
#endif
    store_failed_ = true;
    return false;
  }
  int64_t newStoreOwner() {
    int64_t owner = -1;
#if !defined(OBVI_TESTS_ORACLE_ABI_SHIM_H_) && !defined(OBVI_TESTS_LOCKSTEP_SHIM_H_)
    storeCall(obvi_bbox_store_new_owners(store_, 1, &owner), "obvi_bbox_store_new_owners");
#endif
    return owner;
  }
  bool commitStoreRound(const FrameId& frame_id, const CameraId& camera_id, const std::vector<int64_t>& box_owner) {
#if !defined(OBVI_TESTS_ORACLE_ABI_SHIM_H_) && !defined(OBVI_TESTS_LOCKSTEP_SHIM_H_)
    return !store_failed_ && storeCall(obvi_bbox_store_commit(store_, (uint64_t)frame_id, (uint64_t)camera_id, (int64_t)box_owner.size(), box_owner.data()), "obvi_bbox_store_commit");
#else
    (void)frame_id; (void)camera_id; (void)box_owner;
    return false;
#endif
  }

  // the device round plus the assignment, in place of :355-490
  bool getBoundingBoxAssignments(const std::vector<RawBoundingBox>& boxes, const FeatureBasedContextInfo& context, std::vector<std::vector<FeatureId>>* features_in_bb,
                                 std::vector<AssociatedObjectIdentifier>* assignments) {
#if !defined(OBVI_TESTS_ORACLE_ABI_SHIM_H_) && !defined(OBVI_TESTS_LOCKSTEP_SHIM_H_)
    const int64_t n_feat = (int64_t)context.observed_features_.size(), n_box = (int64_t)boxes.size();
    std::vector<uint64_t> feat_id((size_t)n_feat);
    std::vector<double> feat_pixel((size_t)(2 * n_feat)), corners((size_t)(4 * n_box));
    for (int64_t i = 0; i < n_feat; ++i) { feat_id[i] = context.observed_features_[i].first; feat_pixel[2 * i] = context.observed_features_[i].second[0]; feat_pixel[2 * i + 1] = context.observed_features_[i].second[1]; }
    std::vector<int32_t> box_label((size_t)n_box), cand_label;
    for (int64_t b = 0; b < n_box; ++b) { const BbCorners c = cornerLocationsPairToVector(boxes[b].pixel_corner_locations_); std::copy(c.begin(), c.end(), corners.begin() + 4 * b); box_label[b] = labelOf(boxes[b].semantic_class_); }
    if (store_) return getStoreAssignments(n_feat, feat_id, feat_pixel, n_box, corners, box_label, features_in_bb, assignments);
    std::vector<uint64_t> view_ptr{0}, feat_ptr{0}, view_feat;
    std::vector<ObjectId> cand_object;                                                         // of the initialised candidates
    auto add_views = [&](const ObservedFeats& views) {
      for (const auto& v : views) { view_feat.insert(view_feat.end(), v.second.begin(), v.second.end()); feat_ptr.push_back(view_feat.size()); }
      view_ptr.push_back(feat_ptr.size() - 1);
    };
    const int64_t n_pending = (int64_t)uninitialized_object_info_.size();
    for (const FeatureBasedPendingObject& p : uninitialized_object_info_) { cand_label.push_back(labelOf(p.semantic_class_)); add_views(p.observed_feats_); }
    std::unordered_map<ObjectId, std::pair<std::string, RawEllipsoid>> object_estimates;
    pose_graph_->getObjectEstimates(object_estimates);
    std::map<ObjectId, std::string> objects;
    for (const auto& o : object_estimates) objects[o.first] = o.second.first;
    for (const auto& o : objects) {
      const auto info = object_appearance_info_.find(o.first);
      if (info == object_appearance_info_.end()) continue;                                      // "Could not find appearance info for initialized object" :382-389
      cand_label.push_back(labelOf(o.second)); cand_object.push_back(o.first); add_views(info->second);
    }
    const int64_t n_cand = (int64_t)cand_label.size(), n_views = (int64_t)feat_ptr.size() - 1;
    std::vector<uint8_t> in_box((size_t)(n_box * n_feat)), is_match((size_t)(n_box * n_cand));
    std::vector<double> score((size_t)(n_box * n_cand));
    const obvi_bbox_frontend_params prm{association_params_.bounding_box_inflation_size_, association_params_.min_overlapping_features_for_match_};
    int rc = obvi_bbox_frontend_associate(handle_, n_feat, feat_id.data(), feat_pixel.data(), n_box, corners.data(), box_label.data(), n_cand, cand_label.data(), n_views, view_ptr.data(),
                                          (int64_t)view_feat.size(), feat_ptr.data(), view_feat.data(), &prm, in_box.data(), nullptr, nullptr, is_match.data(), score.data());
    if (rc != 0) { std::cerr << "obvi_bbox_frontend_associate failed: status " << rc << " " << obvi_ba_last_error(handle_) << std::endl; return false; }
    std::vector<int64_t> assigned((size_t)n_box);
    std::vector<uint8_t> is_new((size_t)n_box);
    rc = obvi_bbox_frontend_assign(n_box, n_cand, n_pending, is_match.data(), score.data(), assigned.data(), is_new.data());
    if (rc != 0) { std::cerr << "obvi_bbox_frontend_assign failed: status " << rc << std::endl; return false; }
    features_in_bb->assign((size_t)n_box, {});
    assignments->clear();
    for (int64_t b = 0; b < n_box; ++b) {
      for (int64_t i = 0; i < n_feat; ++i) if (in_box[b * n_feat + i]) (*features_in_bb)[b].push_back(feat_id[i]);
      if (is_new[b]) { assignments->push_back({false, (ObjectId)assigned[b]}); events_.push_back("open " + std::to_string(assigned[b])); }
      else if (assigned[b] < n_pending) assignments->push_back({false, (ObjectId)assigned[b]});
      else assignments->push_back({true, cand_object[(size_t)(assigned[b] - n_pending)]});
    }
    return true;
#else
    (void)boxes; (void)context; (void)features_in_bb; (void)assignments;
    std::cerr << "the bounding-box association round is served by libobvi_ba.so only" << std::endl;
    return false;
#endif
  }

#if !defined(OBVI_TESTS_ORACLE_ABI_SHIM_H_) && !defined(OBVI_TESTS_LOCKSTEP_SHIM_H_)
  // store mode: the same round over the stored views of the candidates' owners; the host needs neither the views nor, afterwards, the ids inside the boxes
  bool getStoreAssignments(int64_t n_feat, const std::vector<uint64_t>& feat_id, const std::vector<double>& feat_pixel, int64_t n_box, const std::vector<double>& corners,
                           const std::vector<int32_t>& box_label, std::vector<std::vector<FeatureId>>* features_in_bb, std::vector<AssociatedObjectIdentifier>* assignments) {
    std::vector<int32_t> cand_label;
    std::vector<int64_t> cand_owner;
    std::vector<ObjectId> cand_object;                                                         // of the initialised candidates
    const int64_t n_pending = (int64_t)uninitialized_object_info_.size();
    for (const FeatureBasedPendingObject& p : uninitialized_object_info_) { cand_label.push_back(labelOf(p.semantic_class_)); cand_owner.push_back(p.store_owner_); }
    std::unordered_map<ObjectId, std::pair<std::string, RawEllipsoid>> object_estimates;
    pose_graph_->getObjectEstimates(object_estimates);
    std::map<ObjectId, std::string> objects;
    for (const auto& o : object_estimates) objects[o.first] = o.second.first;
    for (const auto& o : objects) {
      const auto owner = object_owner_.find(o.first);
      if (owner == object_owner_.end()) continue;                                               // as in the host path: an object without appearance info is no candidate
      cand_label.push_back(labelOf(o.second)); cand_object.push_back(o.first); cand_owner.push_back(owner->second);
    }
    const int64_t n_cand = (int64_t)cand_label.size();
    std::vector<uint8_t> is_match((size_t)(n_box * n_cand));
    std::vector<double> score((size_t)(n_box * n_cand));
    const obvi_bbox_frontend_params prm{association_params_.bounding_box_inflation_size_, association_params_.min_overlapping_features_for_match_};
    if (!storeCall(obvi_bbox_store_associate(store_, n_feat, feat_id.data(), feat_pixel.data(), n_box, corners.data(), box_label.data(), n_cand, cand_owner.data(), cand_label.data(), &prm,
                                             nullptr, nullptr, nullptr, is_match.data(), score.data()), "obvi_bbox_store_associate")) return false;
    std::vector<int64_t> assigned((size_t)n_box);
    std::vector<uint8_t> is_new((size_t)n_box);
    const int rc = obvi_bbox_frontend_assign(n_box, n_cand, n_pending, is_match.data(), score.data(), assigned.data(), is_new.data());
    if (rc != 0) { std::cerr << "obvi_bbox_frontend_assign failed: status " << rc << std::endl; return false; }
    features_in_bb->assign((size_t)n_box, {});                                                  // stays empty: the commit cuts the views out of the round on the device
    assignments->clear();
    for (int64_t b = 0; b < n_box; ++b) {
      if (is_new[b]) { assignments->push_back({false, (ObjectId)assigned[b]}); events_.push_back("open " + std::to_string(assigned[b])); }
      else if (assigned[b] < n_pending) assignments->push_back({false, (ObjectId)assigned[b]});
      else assignments->push_back({true, cand_object[(size_t)(assigned[b] - n_pending)]});
    }
    return true;
  }
#endif

  void addObservationForObject(const FrameId& frame_id, const CameraId& camera_id, const ObjectId& object_id, const BbCorners& corners, const Covariance<4>& cov, const double& confidence) {
    ObjectObservationFactor f;                                                                  // bounding_box_front_end.h:563-577
    f.frame_id_ = frame_id; f.camera_id_ = camera_id; f.object_id_ = object_id; f.bounding_box_corners_ = corners; f.bounding_box_corners_covariance_ = cov; f.detection_confidence_ = confidence;
    pose_graph_->addObjectObservation(f);
  }

  bool setupInitialEstimateGeneration(const std::vector<AssociatedObjectIdentifier>& assignments, const FrameId& frame_id, const CameraId& camera_id) {   // :594-672
    std::unordered_map<ObjectId, RawEllipsoid> rough;
    std::unordered_map<ObjectId, FeatureBasedPendingObject> infos;
    for (const AssociatedObjectIdentifier& a : assignments) {
      if (a.initialized_ellipsoid_) continue;
      if (a.object_id_ >= uninitialized_object_info_.size()) { std::cerr << "No pending object for id " << a.object_id_ << std::endl; return false; }   // exit(1) in the reference
      const FeatureBasedPendingObject& p = uninitialized_object_info_[a.object_id_];
      if (p.object_estimate_.has_value()) { rough[a.object_id_] = p.object_estimate_.value(); infos[a.object_id_] = p; }
    }
    for (size_t id = 0; id < uninitialized_object_info_.size(); ++id) {
      if (rough.count(id)) continue;
      const FeatureBasedPendingObject& p = uninitialized_object_info_[id];
      if (p.ready_for_merge && p.object_estimate_.has_value()) { rough[id] = p.object_estimate_.value(); infos[id] = p; }
    }
    const std::unordered_map<ObjectId, RawEllipsoid> refined = refiner_(rough, infos, frame_id, camera_id);
    for (const auto& r : refined) {
      FeatureBasedPendingObject& p = uninitialized_object_info_[r.first];
      p.object_estimate_ = r.second;
      p.ready_for_merge = p.observation_factors_.size() >= association_params_.min_observations_for_local_est_ &&
                          p.max_confidence_ >= association_params_.required_min_conf_for_initialization_ && p.object_estimate_.has_value();
    }
    return true;
  }

  ObjectInitializationStatus tryInitializeEllipsoid(const FeatureBasedPendingObject& p, RawEllipsoid& est) const {   // :674-692
    if (!p.ready_for_merge) return NOT_INITIALIZED;
    est = p.object_estimate_.value();
    return p.observation_factors_.size() < association_params_.min_observations_ ? ENOUGH_VIEWS_FOR_MERGE : SUFFICIENT_VIEWS_FOR_NEW;
  }

  // helpers.h:29-123 with only_match_semantic_class: objects of the pending object's class that no box of this round went to and that have no observation
  // from a (frame, camera) the pending object was seen from
  void identifyMergeCandidates(const std::unordered_set<ObjectId>& existing_associated_to_objects, const std::set<ObjectId>& possible_pending, std::map<ObjectId, std::vector<ObjectId>>& merge_candidates) const {
    std::unordered_map<ObjectId, std::pair<std::string, RawEllipsoid>> object_estimates;
    pose_graph_->getObjectEstimates(object_estimates);
    std::map<ObjectId, std::string> objects;
    for (const auto& o : object_estimates) objects[o.first] = o.second.first;
    std::map<ObjectId, std::set<std::pair<FrameId, CameraId>>> sources;
    FactorInfoSet all;
    pose_graph_->getObservationFactorsBetweenFrameIdsInclusive(0, ~(FrameId)0, all);
    for (const FactorInfo& info : all) { ObjectObservationFactor f; if (pose_graph_->getObjectObservationFactor(info.second, f)) sources[f.object_id_].insert({f.frame_id_, f.camera_id_}); }
    for (const ObjectId& pending : possible_pending) {
      const FeatureBasedPendingObject& p = uninitialized_object_info_[pending];
      for (const auto& o : objects) {
        if (o.second != p.semantic_class_ || existing_associated_to_objects.count(o.first)) continue;
        bool no_overlap = true;
        for (const ObjectObservationFactor& f : p.observation_factors_) if (sources[o.first].count({f.frame_id_, f.camera_id_})) { no_overlap = false; break; }
        if (no_overlap) merge_candidates[pending].push_back(o.first);
      }
    }
  }

  void searchForObjectMerges(const std::map<ObjectId, std::pair<ObjectInitializationStatus, RawEllipsoid>>& mergable, const std::unordered_set<ObjectId>& existing_associated_to_objects,
                             std::vector<std::pair<ObjectId, ObjectId>>& to_merge, std::vector<std::pair<ObjectId, RawEllipsoid>>& to_add) const {   // :742-843
    std::set<ObjectId> possible_pending;
    for (const auto& m : mergable) possible_pending.insert(m.first);
    std::map<ObjectId, std::vector<ObjectId>> merge_candidates;
    identifyMergeCandidates(existing_associated_to_objects, possible_pending, merge_candidates);
    std::unordered_map<ObjectId, std::pair<std::string, RawEllipsoid>> object_estimates;
    pose_graph_->getObjectEstimates(object_estimates);
    std::vector<std::pair<std::pair<ObjectId, ObjectId>, double>> flattened;
    for (const auto& m : mergable)
      for (const ObjectId& cand : merge_candidates[m.first]) {
        const auto est = object_estimates.find(cand);
        double score;
        if (est != object_estimates.end() && geometric_similarity_scorer_(m.second.second, est->second.second, score)) flattened.push_back({{m.first, cand}, score});
      }
    std::sort(flattened.begin(), flattened.end(), [](const auto& l, const auto& r) { return l.second != r.second ? l.second > r.second : l.first < r.first; });
    std::set<ObjectId> unmerged = possible_pending;
    std::unordered_set<ObjectId> newly_matched_existing_objects;                              // never filled in the reference either (:808-821)
    for (const auto& pair_and_score : flattened) {
      if (!unmerged.count(pair_and_score.first.first)) continue;
      if (newly_matched_existing_objects.count(pair_and_score.first.second)) continue;
      unmerged.erase(pair_and_score.first.first);
      to_merge.push_back(pair_and_score.first);
      if (unmerged.empty()) break;
    }
    for (const ObjectId& u : unmerged) if (mergable.at(u).first == SUFFICIENT_VIEWS_FOR_NEW) to_add.push_back({u, mergable.at(u).second});
  }

  std::vector<ObjectId> mergePending(const std::vector<std::pair<ObjectId, ObjectId>>& to_merge) {   // bounding_box_front_end.h:438-468
    std::vector<ObjectId> merged;
    std::vector<int64_t> merge_from, merge_into;                                                // store mode: one merge call for the whole list
    for (const auto& m : to_merge) {
      const FeatureBasedPendingObject info = uninitialized_object_info_[m.first];
      for (const ObjectObservationFactor& f : info.observation_factors_)
        addObservationForObject(f.frame_id_, f.camera_id_, m.second, f.bounding_box_corners_, f.bounding_box_corners_covariance_, f.detection_confidence_);
      if (store_) {
        merge_from.push_back(info.store_owner_); merge_into.push_back(object_owner_.at(m.second));
      } else {
        ObservedFeats& into = object_appearance_info_.at(m.second);                             // mergeObjectAssociationInfo :244-273
        for (const auto& v : info.observed_feats_) into[v.first] = v.second;
      }
      events_.push_back("merge " + std::to_string(m.first) + " " + std::to_string(m.second));
      merged.push_back(m.first);
    }
#if !defined(OBVI_TESTS_ORACLE_ABI_SHIM_H_) && !defined(OBVI_TESTS_LOCKSTEP_SHIM_H_)
    if (store_ && !merge_from.empty()) storeCall(obvi_bbox_store_merge(store_, (int64_t)merge_from.size(), merge_from.data(), merge_into.data()), "obvi_bbox_store_merge");
#endif
    return merged;
  }

  std::vector<ObjectId> mergeExistingPendingObjects() {                                         // :694-740
    std::map<ObjectId, std::pair<ObjectInitializationStatus, RawEllipsoid>> mergable;
    for (size_t id = 0; id < uninitialized_object_info_.size(); ++id)
      if (uninitialized_object_info_[id].ready_for_merge) mergable[id] = {ENOUGH_VIEWS_FOR_MERGE, uninitialized_object_info_[id].object_estimate_.value()};
    std::vector<std::pair<ObjectId, ObjectId>> to_merge;
    std::vector<std::pair<ObjectId, RawEllipsoid>> to_add;
    searchForObjectMerges(mergable, {}, to_merge, to_add);
    return mergePending(to_merge);
  }

  void erasePending(std::vector<ObjectId> indices) {                                            // descending, so that the indices stay valid (:296-318)
    std::sort(indices.begin(), indices.end(), std::greater<ObjectId>());
    for (const ObjectId& i : indices) uninitialized_object_info_.erase(uninitialized_object_info_.begin() + (std::ptrdiff_t)i);
  }

  void cleanupBbAssociationRound(const FrameId& frame_id) {                                     // :506-592
    std::vector<FeatureBasedPendingObject> keep;
    if (association_params_.discard_candidate_after_num_frames_ > 0)
      for (const FeatureBasedPendingObject& p : uninitialized_object_info_) if (frame_id <= p.max_frame_id_ + association_params_.discard_candidate_after_num_frames_) keep.push_back(p);
    if (keep.size() != uninitialized_object_info_.size()) events_.push_back("discard " + std::to_string(uninitialized_object_info_.size() - keep.size()));
    size_t dropped = 0;
#if !defined(OBVI_TESTS_ORACLE_ABI_SHIM_H_) && !defined(OBVI_TESTS_LOCKSTEP_SHIM_H_)
    if (store_) {                                                                               // the discarded owners go, then the window over everything left
      std::set<int64_t> kept;
      for (const FeatureBasedPendingObject& p : keep) kept.insert(p.store_owner_);
      std::vector<int64_t> discarded;
      for (const FeatureBasedPendingObject& p : uninitialized_object_info_) if (!kept.count(p.store_owner_)) discarded.push_back(p.store_owner_);
      if (!discarded.empty()) storeCall(obvi_bbox_store_release(store_, (int64_t)discarded.size(), discarded.data()), "obvi_bbox_store_release");
      int64_t n = 0;
      if (storeCall(obvi_bbox_store_apply_window(store_, (uint64_t)frame_id, (uint64_t)association_params_.feature_validity_window_, &n), "obvi_bbox_store_apply_window")) dropped = (size_t)n;
    }
#endif
    auto apply_window = [&](ObservedFeats& views) {
      for (auto it = views.begin(); it != views.end();)
        if (it->first.first + association_params_.feature_validity_window_ < frame_id) { it = views.erase(it); ++dropped; } else ++it;
    };
    for (FeatureBasedPendingObject& p : keep) apply_window(p.observed_feats_);
    uninitialized_object_info_ = keep;
    for (auto& o : object_appearance_info_) apply_window(o.second);
    if (dropped) events_.push_back("views_dropped " + std::to_string(dropped));
  }

  std::shared_ptr<PoseGraph> pose_graph_;
  obvi_ba_handle* handle_;
  FeatureBasedBbAssociationParams association_params_;
  BbCovarianceGenerator covariance_generator_;
  GeometricSimilarityScorer geometric_similarity_scorer_;
  PendingEstimateRefiner refiner_;
  std::vector<FeatureBasedPendingObject> uninitialized_object_info_;
  std::map<ObjectId, ObservedFeats> object_appearance_info_;
  std::map<std::string, int32_t> label_ids_;
  std::vector<AssociatedObjectIdentifier> last_assignments_;
  std::vector<std::string> events_;
  obvi_bbox_store* store_ = nullptr;                // store mode
  std::map<ObjectId, int64_t> object_owner_;       // store mode: the objects with appearance data and their owner tokens
  bool store_failed_ = false;
};

}  // namespace vslam_types_refactor
#endif  // OBVI_HOST_BOUNDING_BOX_FRONT_END_H_
