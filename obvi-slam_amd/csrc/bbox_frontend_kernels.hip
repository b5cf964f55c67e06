// bbox_frontend_kernels.hip -- bounding-box data association on the device (include/obvi_bbox_frontend.h): one (frame, camera) round of the reference's
// feature-based front end (feature_based_bounding_box_front_end.h:190-209, :357-479, :917-940) up to the assignment, and the greedy assignment itself
// (bounding_box_front_end_helpers.h:125-184) on the host.  The inner work of the reference is set intersection through unordered_set look-ups: every box of the
// frame against every earlier view of every candidate of its class.  Here the frame's features are sorted by id once on the host, and the three kernels of
// bbox_kernels.h (k_bbox_membership, k_bbox_overlap, k_bbox_score; shared with the store of bbox_store_kernels.hip) run over views given as a CSR.
// All integer work except the score; the only atomics are integer adds, so a deterministic handle runs the same code.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "../../include/obvi_bbox_frontend.h"
#include "ba_device.h"
#include "bbox_kernels.h"
#include "host_util.h"

namespace obvi {
namespace {

using namespace bbox;   // NOLINT: the kernels and their limits (bbox_kernels.h)

// offsets[0] == 0, ascending, offsets[n] == total
bool csr_ok(const uint64_t* offsets, int64_t n, int64_t total) {
  if (offsets[0] != 0 || offsets[n] != (uint64_t)total) return false;
  for (int64_t i = 0; i < n; ++i) if (offsets[i + 1] < offsets[i]) return false;
  return true;
}

}  // namespace
}  // namespace obvi

extern "C" {

int64_t obvi_bbox_frontend_lds_feature_limit(void) { return obvi::kLdsFeatureLimit; }

int obvi_bbox_frontend_associate(obvi_ba_handle* h, int64_t n_feat, const uint64_t* feat_id, const double* feat_pixel, int64_t n_box, const double* box_corners,
                                 const int32_t* box_label, int64_t n_cand, const int32_t* cand_label, int64_t n_views, const uint64_t* view_ptr, int64_t n_view_feat,
                                 const uint64_t* feat_ptr, const uint64_t* view_feat, const obvi_bbox_frontend_params* prm, uint8_t* in_box, uint32_t* feats_in_box,
                                 uint32_t* overlap, uint8_t* is_match, double* score) {
  using namespace obvi;   // NOLINT
  // the arguments are judged before the handle is looked at, so that a refusal can be observed without a device; the message goes into a handle that is there
  auto refuse = [h](int code, const char* msg) { return h ? handle_fail(h, code, msg) : code; };
  if (n_feat < 0 || n_box < 0 || n_cand < 0 || n_views < 0 || n_view_feat < 0 || !prm || !view_ptr || !feat_ptr || (n_feat > 0 && (!feat_id || !feat_pixel)) ||
      (n_box > 0 && (!box_corners || !box_label)) || (n_cand > 0 && !cand_label) || (n_view_feat > 0 && !view_feat))
    return refuse(OBVI_ERR_INVALID_ARGUMENT, "bbox associate: bad arguments");
  if (n_feat > (int64_t)UINT32_MAX || n_box > (int64_t)INT32_MAX - 64) return refuse(OBVI_ERR_INVALID_ARGUMENT, "bbox associate: too many features or boxes");
  // the products that size a buffer or a grid: in_box, the bit rows, overlap, is_match / score (one thread each)
  const int64_t most = n_box > 0 ? kMaxOutputEntries / n_box : kMaxOutputEntries;
  if (n_feat > most || n_views > most || n_cand > most) return refuse(OBVI_ERR_INVALID_ARGUMENT, "bbox associate: boxes times features, views or candidates above 2^31");
  if (!csr_ok(view_ptr, n_cand, n_views)) return refuse(OBVI_ERR_INVALID_ARGUMENT, "bbox associate: view_ptr must start at 0, ascend and end at n_views");
  if (!csr_ok(feat_ptr, n_views, n_view_feat)) return refuse(OBVI_ERR_INVALID_ARGUMENT, "bbox associate: feat_ptr must start at 0, ascend and end at n_view_feat");
  if (!std::isfinite(prm->bounding_box_inflation_size) || !std::isfinite(prm->min_overlapping_features_for_match))
    return refuse(OBVI_ERR_NUMERICAL, "bbox associate: non-finite parameter");
  for (int64_t i = 0; i < 4 * n_box; ++i) if (!std::isfinite(box_corners[i])) return refuse(OBVI_ERR_NUMERICAL, "bbox associate: non-finite box corner");
  try {
    // the frame's features in ascending id order: the list the overlap pass searches, and the order of the bit rows
    std::vector<uint32_t> orig((size_t)n_feat);
    std::iota(orig.begin(), orig.end(), 0u);
    std::sort(orig.begin(), orig.end(), [&](uint32_t a, uint32_t b) { return feat_id[a] < feat_id[b]; });
    std::vector<uint64_t> ids((size_t)n_feat);
    std::vector<double> pix((size_t)(2 * n_feat));
    for (int64_t s = 0; s < n_feat; ++s) {
      ids[s] = feat_id[orig[s]];
      if (s > 0 && ids[s] == ids[s - 1]) return refuse(OBVI_ERR_INVALID_ARGUMENT, "bbox associate: a feature id occurs twice in the frame");
      pix[2 * s] = feat_pixel[2 * (int64_t)orig[s]]; pix[2 * s + 1] = feat_pixel[2 * (int64_t)orig[s] + 1];
    }
    if (!h) return OBVI_ERR_INVALID_ARGUMENT;
    if (n_box == 0) return OBVI_OK;                                 // every output has a zero dimension
    OBVI_HIP(hipSetDevice(handle_device(h)));
    hipStream_t s = handle_stream(h);
    const int32_t words = (int32_t)((n_box + 63) / 64);
    DevBuf<uint64_t> d_ids, d_bits, d_vptr, d_fptr, d_vfeat; DevBuf<double> d_pix, d_corners, d_score; DevBuf<uint32_t> d_orig, d_count, d_overlap;
    DevBuf<int32_t> d_blabel, d_clabel; DevBuf<uint8_t> d_in, d_match;
    d_count.resize((size_t)n_box); d_count.zero(s);
    if (n_feat > 0) {
      d_ids.upload(ids, s); d_pix.upload(pix, s); d_orig.upload(orig, s); d_corners.upload(box_corners, (size_t)(4 * n_box), s);
      d_bits.resize((size_t)(n_feat * words));
      if (in_box) d_in.resize((size_t)(n_box * n_feat));
      MemberBatch m{n_feat, (int32_t)n_box, words, d_pix.get(), d_orig.get(), d_corners.get(), prm->bounding_box_inflation_size};
      hipLaunchKernelGGL(k_bbox_membership, dim3((unsigned)((n_feat + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, m, d_bits.get(), in_box ? d_in.get() : nullptr, d_count.get());
      OBVI_HIP(hipGetLastError());
    }
    d_fptr.upload(feat_ptr, (size_t)n_views + 1, s);
    if (n_views > 0) {
      d_overlap.resize((size_t)(n_box * n_views));
      if (n_feat > 0) {
        d_vfeat.upload(view_feat, (size_t)n_view_feat, s);
        OverlapBatch o{n_feat, n_views, (int32_t)n_box, words, d_ids.get(), d_bits.get()};
        const CsrViews views{d_fptr.get(), d_vfeat.get()};
        const unsigned grid = (unsigned)std::min<int64_t>((n_views + kWavesPerBlock - 1) / kWavesPerBlock, kOverlapMaxBlocks);
        if (n_feat <= kLdsFeatureLimit) hipLaunchKernelGGL((k_bbox_overlap<true, CsrViews>), dim3(grid), dim3(kBlock), 0, s, o, views, d_overlap.get());
        else hipLaunchKernelGGL((k_bbox_overlap<false, CsrViews>), dim3(grid), dim3(kBlock), 0, s, o, views, d_overlap.get());
        OBVI_HIP(hipGetLastError());
      } else {
        d_overlap.zero(s);                                          // no features in the frame: nothing to search in
      }
    }
    std::vector<uint8_t> h_match;
    std::vector<double> h_score;
    if (n_cand > 0 && (is_match || score)) {
      d_blabel.upload(box_label, (size_t)n_box, s); d_clabel.upload(cand_label, (size_t)n_cand, s); d_vptr.upload(view_ptr, (size_t)n_cand + 1, s);
      d_match.resize((size_t)(n_box * n_cand)); d_score.resize((size_t)(n_box * n_cand));
      ScoreBatch sb{n_box, n_cand, n_views, d_blabel.get(), d_clabel.get(), d_vptr.get(), d_overlap.get(), d_count.get(), prm->min_overlapping_features_for_match};
      hipLaunchKernelGGL(k_bbox_score<CsrViews>, dim3((unsigned)((n_box * n_cand + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, sb, CsrViews{d_fptr.get(), d_vfeat.get()}, d_match.get(), d_score.get());
      OBVI_HIP(hipGetLastError());
      h_match.resize((size_t)(n_box * n_cand));
      d_match.download(h_match.data(), h_match.size(), s);
      if (score) { h_score.resize((size_t)(n_box * n_cand)); d_score.download(h_score.data(), h_score.size(), s); }
    }
    std::vector<uint8_t> h_in; std::vector<uint32_t> h_count, h_overlap;      // read back beside the caller's arrays: a failure leaves those untouched
    if (in_box && n_feat > 0) { h_in.resize((size_t)(n_box * n_feat)); d_in.download(h_in.data(), h_in.size(), s); }
    if (feats_in_box) { h_count.resize((size_t)n_box); d_count.download(h_count.data(), h_count.size(), s); }
    if (overlap && n_views > 0) { h_overlap.resize((size_t)(n_box * n_views)); d_overlap.download(h_overlap.data(), h_overlap.size(), s); }
    OBVI_HIP(hipStreamSynchronize(s));
    std::copy(h_in.begin(), h_in.end(), in_box);
    std::copy(h_count.begin(), h_count.end(), feats_in_box);
    std::copy(h_overlap.begin(), h_overlap.end(), overlap);
    if (is_match) std::copy(h_match.begin(), h_match.end(), is_match);
    if (score) for (size_t i = 0; i < h_score.size(); ++i) if (h_match[i]) score[i] = h_score[i];
    return OBVI_OK;
  } catch (const HipError& e) {
    if (h) (void)hipStreamSynchronize(handle_stream(h));     // copies out of the local vectors may still be queued
    return refuse(OBVI_ERR_HIP, e.what);
  } catch (const std::exception& e) {
    if (h) (void)hipStreamSynchronize(handle_stream(h));
    return refuse(OBVI_ERR_HIP, e.what());
  } catch (...) {
    if (h) (void)hipStreamSynchronize(handle_stream(h));
    return refuse(OBVI_ERR_HIP, "unknown host exception");
  }
}

int obvi_bbox_frontend_assign(int64_t n_box, int64_t n_cand, int64_t n_pending, const uint8_t* is_match, const double* score, int64_t* assigned_cand, uint8_t* is_new) {
  if (n_box < 0 || n_cand < 0 || n_pending < 0 || (n_box > 0 && (!assigned_cand || !is_new)) || (n_box > 0 && n_cand > 0 && (!is_match || !score))) return OBVI_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n_box * n_cand; ++i) if (is_match[i] && std::isnan(score[i])) return OBVI_ERR_NUMERICAL;
  try {
    std::vector<int64_t> order;
    for (int64_t i = 0; i < n_box * n_cand; ++i) if (is_match[i]) order.push_back(i);
    // descending score; i = box * n_cand + candidate, so a tie goes by box, then by candidate
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return score[x] != score[y] ? score[x] > score[y] : x < y; });
    std::vector<int64_t> taken((size_t)n_box, -1);
    std::vector<uint8_t> claimed((size_t)n_cand, 0);
    for (int64_t i : order) {
      const int64_t b = i / n_cand, c = i % n_cand;
      if (taken[b] >= 0 || claimed[c]) continue;
      taken[b] = c; claimed[c] = 1;
    }
    int64_t next = n_pending;
    for (int64_t b = 0; b < n_box; ++b) {
      is_new[b] = taken[b] < 0 ? 1 : 0;
      assigned_cand[b] = taken[b] < 0 ? next++ : taken[b];
    }
  } catch (...) { return OBVI_ERR_HIP; }
  return OBVI_OK;
}

}  // extern "C"
