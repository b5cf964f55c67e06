// bbox_store_replay.cpp -- the program of tests/bbox_front_end_replay.cpp with the host mirror of the feature-based bounding-box front end
// (obvi-slam_amd/host/obvi_bounding_box_front_end.h) in store mode: the views live in an obvi_bbox_store (include/obvi_bbox_store.h) whose pool starts small and
// compacts early, so that growth and compaction occur within the stream.  The same hooks, the same print-out -- the sizes of the views come from the store's
// directory through storedViewSizes -- and one more line, the store's final counters.  tests/test_gpu_bbox_store_host.py compares the print-out with the
// Python restatement the host path is held to.
//   bbox_store_replay <stream file>
// stream: "params <min_obs_local> <min_obs> <discard_after> <validity_window> <min_conf> <min_overlap> <inflation> <max_merge_distance>",
//         "classes <n>" + n x "<name> <dx> <dy> <dz>", "frames <n>" + per frame "frame <id> <n_feat> <n_box>", n_feat x "<id> <x> <y>", n_box x "<class> <x0> <y0> <x1> <y1> <conf>"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <map>
#include <string>

#include "obvi_bounding_box_front_end.h"

using namespace vslam_types_refactor;   // NOLINT

int main(int argc, char** argv) {
  if (argc < 2) { std::cerr << "usage: " << argv[0] << " <stream file>" << std::endl; return 2; }
  std::ifstream in(argv[1]);
  if (!in) { std::cerr << "cannot read " << argv[1] << std::endl; return 2; }
  std::string word;
  FeatureBasedBbAssociationParams prm;
  GeometricSimilarityScorerParams scorer;
  scorer.x_y_only_merge_ = false;
  unsigned min_local, min_obs;
  in >> word >> min_local >> min_obs >> prm.discard_candidate_after_num_frames_ >> prm.feature_validity_window_ >> prm.min_bb_confidence_ >> prm.min_overlapping_features_for_match_ >>
      prm.bounding_box_inflation_size_ >> scorer.max_merge_distance_;
  prm.min_observations_for_local_est_ = (uint16_t)min_local; prm.min_observations_ = (uint16_t)min_obs;
  size_t n_classes, n_frames;
  in >> word >> n_classes;
  std::unordered_map<std::string, std::pair<ObjectDim, Covariance<3>>> shape;
  for (size_t c = 0; c < n_classes; ++c) { std::string name; ObjectDim d; in >> name >> d[0] >> d[1] >> d[2]; shape[name] = {d, Covariance<3>{{0.01, 0, 0, 0, 0.01, 0, 0, 0, 0.01}}}; }
  auto pose_graph = std::make_shared<ObjectAndReprojectionFeaturePoseGraph>(std::unordered_map<CameraId, CameraExtrinsics>{{0, CameraExtrinsics()}},
                                                                           std::unordered_map<CameraId, CameraIntrinsicsMat>{{0, CameraIntrinsicsMat{500.0, 500.0, 320.0, 240.0}}});
  pose_graph->setShapePriorsBySemanticClass(shape);

  obvi_ba_options opt = obvi::makeHandleOptions(0);
  obvi_ba_handle* handle = nullptr;
  if (obvi_ba_create(&opt, &handle) != 0) { std::cerr << "no device" << std::endl; return 3; }
  const Covariance<4> constant_cov{{9, 0, 0, 0, 0, 9, 0, 0, 0, 0, 9, 0, 0, 0, 0, 9}};
  FeatureBasedBoundingBoxFrontEnd<> front_end(
      pose_graph, handle, prm, [constant_cov](const RawBoundingBox&, const FrameId&, const CameraId&, const FeatureBasedContextInfo&) { return constant_cov; },
      getDistanceSimilarityScorer(scorer),
      [](const std::unordered_map<ObjectId, RawEllipsoid>& rough, const std::unordered_map<ObjectId, FeatureBasedPendingObject>&, const FrameId&, const CameraId&) { return rough; });

  const obvi_bbox_store_options store_options{32, 1};
  if (!front_end.useAppearanceStore(store_options)) { std::cerr << "no store" << std::endl; return 3; }

  in >> word >> n_frames;
  for (size_t f = 0; f < n_frames; ++f) {
    FrameId frame_id; size_t n_feat, n_box;
    in >> word >> frame_id >> n_feat >> n_box;
    pose_graph->addFrame(frame_id, Pose3D());
    FeatureBasedContextInfo context;
    for (size_t i = 0; i < n_feat; ++i) { FeatureId id; PixelCoord px; in >> id >> px[0] >> px[1]; context.observed_features_.push_back({id, px}); }
    std::vector<RawBoundingBox> boxes(n_box);
    for (RawBoundingBox& b : boxes) in >> b.semantic_class_ >> b.pixel_corner_locations_.first[0] >> b.pixel_corner_locations_.first[1] >> b.pixel_corner_locations_.second[0] >> b.pixel_corner_locations_.second[1] >> b.detection_confidence_;
    if (!in) { std::cerr << "malformed stream at frame " << f << std::endl; return 2; }
    if (!front_end.addBoundingBoxObservations(frame_id, 0, boxes, context)) { std::cerr << "round failed at frame " << frame_id << std::endl; return 4; }
    std::cout << "round " << frame_id;
    for (const AssociatedObjectIdentifier& a : front_end.lastAssignments()) std::cout << " " << (a.initialized_ellipsoid_ ? "O" : "P") << a.object_id_;
    std::cout << "\n";
    for (const std::string& e : front_end.takeEvents()) std::cout << "event " << frame_id << " " << e << "\n";
  }
  std::cout.precision(12);
  for (const FeatureBasedPendingObject& p : front_end.pendingObjects()) {
    std::cout << "pending " << p.semantic_class_ << " " << p.observation_factors_.size() << " " << (p.ready_for_merge ? 1 : 0) << " " << p.min_frame_id_ << " " << p.max_frame_id_ << " " << p.max_confidence_;
    if (p.object_estimate_.has_value()) for (double v : p.object_estimate_.value()) std::cout << " " << v;
    std::cout << " views";
    if (!p.observed_feats_.empty()) { std::cerr << "observed_feats_ is not empty in store mode" << std::endl; return 5; }
    for (const auto& v : front_end.storedViewSizes(p.store_owner_)) std::cout << " " << std::get<0>(v) << ":" << std::get<2>(v);
    std::cout << "\n";
  }
  std::unordered_map<ObjectId, std::pair<std::string, RawEllipsoid>> estimates;
  pose_graph->getObjectEstimates(estimates);
  std::map<ObjectId, std::pair<std::string, RawEllipsoid>> objects(estimates.begin(), estimates.end());
  for (const auto& o : objects) {
    std::cout << "object " << o.first << " " << o.second.first;
    for (double v : o.second.second) std::cout << " " << v;
    std::cout << " views";
    const auto owner = front_end.objectStoreOwners().find(o.first);
    if (owner != front_end.objectStoreOwners().end()) for (const auto& v : front_end.storedViewSizes(owner->second)) std::cout << " " << std::get<0>(v) << ":" << std::get<2>(v);
    std::cout << "\n";
  }
  FactorInfoSet all;
  pose_graph->getObservationFactorsBetweenFrameIdsInclusive(0, ~(FrameId)0, all);
  std::map<std::pair<ObjectId, FrameId>, ObjectObservationFactor> factors;
  for (const FactorInfo& info : all) { ObjectObservationFactor fac; if (pose_graph->getObjectObservationFactor(info.second, fac)) factors[{fac.object_id_, fac.frame_id_}] = fac; }
  std::cout << "factors " << all.size() << "\n";
  for (const auto& fac : factors) {
    std::cout << "factor " << fac.first.first << " " << fac.first.second << " " << fac.second.camera_id_;
    for (double v : fac.second.bounding_box_corners_) std::cout << " " << v;
    std::cout << " " << fac.second.bounding_box_corners_covariance_[0] << " " << fac.second.detection_confidence_ << "\n";
  }
  if (!front_end.objectAppearanceInfo().empty()) { std::cerr << "object_appearance_info_ is not empty in store mode" << std::endl; return 5; }
  obvi_bbox_store_stats st;
  if (!front_end.appearanceStoreStats(&st)) { std::cerr << "no stats" << std::endl; return 5; }
  std::cout << "store owners " << st.owners << " views " << st.views << " live_ids " << st.live_ids << " dead_ids " << st.dead_ids << " capacity " << st.pool_capacity_ids << " growths "
            << st.pool_growths << " compactions " << st.compactions << " replaced " << st.replaced_views << "\n";
  return 0;
}
