// bbox_host_round.cpp -- one bounding-box association round done the plain host way, std::unordered_set look-ups as in the reference
// (feature_based_bounding_box_front_end.h:190-209, :357-479, :917-940), to have a host time beside the device's (scripts/bbox_round_time.py writes the round
// and reads the one line printed here).  Stand-alone; the script builds it: g++ -O2 -std=c++17 -o <program> scripts/bbox_host_round.cpp
//   bbox_host_round <round file> <inflation> <min_overlap> <repeats>   ->   "<median ms> <sum feats_in_box> <sum overlap> <matches> <sum score>"
// The timed part is what the reference does per round: the feature set of every box, and for every candidate of the box's class the intersection with each of
// its views, the largest, and the score.  The views' sets exist before the round (the reference keeps them per object) and are built outside the timed part;
// the reference's copies of a candidate's whole appearance map per box (:390-393, :443-446) are NOT made.  The overlap total covers every (box, view) pair, as
// the device's test hook does, and is counted in a pass of its own.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

template <class T>
static std::vector<T> read_array(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
  return v;
}

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: %s <round file> <inflation> <min_overlap> <repeats>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  const double inflation = atof(argv[2]), min_overlap = atof(argv[3]);
  const int repeats = atoi(argv[4]);
  const std::vector<int64_t> n = read_array<int64_t>(f, 5);
  const int64_t n_feat = n[0], n_box = n[1], n_cand = n[2], n_views = n[3], n_view_feat = n[4];
  const auto feat_id = read_array<uint64_t>(f, n_feat);
  const auto pixel = read_array<double>(f, 2 * n_feat);
  const auto corners = read_array<double>(f, 4 * n_box);
  const auto box_label = read_array<int32_t>(f, n_box);
  const auto cand_label = read_array<int32_t>(f, n_cand);
  const auto view_ptr = read_array<uint64_t>(f, n_cand + 1);
  const auto feat_ptr = read_array<uint64_t>(f, n_views + 1);
  const auto view_feat = read_array<uint64_t>(f, n_view_feat);
  fclose(f);

  std::unordered_map<uint64_t, std::pair<double, double>> observed;
  for (int64_t i = 0; i < n_feat; ++i) observed[feat_id[i]] = {pixel[2 * i], pixel[2 * i + 1]};
  std::vector<std::unordered_set<uint64_t>> views(n_views);
  for (int64_t v = 0; v < n_views; ++v) views[v].insert(view_feat.begin() + feat_ptr[v], view_feat.begin() + feat_ptr[v + 1]);

  int64_t sum_count = 0, matches = 0;
  double sum_score = 0.0;
  std::vector<double> ms;
  std::vector<std::unordered_set<uint64_t>> in_bb(n_box);
  for (int rep = 0; rep < repeats; ++rep) {
    sum_count = 0; matches = 0; sum_score = 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int64_t b = 0; b < n_box; ++b) {
      const double x0 = corners[4 * b] - inflation, x1 = corners[4 * b + 1] + inflation, y0 = corners[4 * b + 2] - inflation, y1 = corners[4 * b + 3] + inflation;
      in_bb[b].clear();
      for (const auto& kv : observed)
        if (x0 <= kv.second.first && y0 <= kv.second.second && x1 >= kv.second.first && y1 >= kv.second.second) in_bb[b].insert(kv.first);
      sum_count += (int64_t)in_bb[b].size();
      for (int64_t c = 0; c < n_cand; ++c) {
        if (cand_label[c] != box_label[b] || view_ptr[c + 1] == view_ptr[c]) continue;
        std::vector<int> common(view_ptr[c + 1] - view_ptr[c]);
        int best = 0;
        for (uint64_t v = view_ptr[c]; v < view_ptr[c + 1]; ++v) {
          int k = 0;
          for (const uint64_t id : views[v]) if (in_bb[b].find(id) != in_bb[b].end()) ++k;
          common[v - view_ptr[c]] = k;
          best = std::max(best, k);
        }
        if ((double)best < min_overlap) continue;
        double iou = 0.0;
        for (uint64_t v = view_ptr[c]; v < view_ptr[c + 1]; ++v) {
          const int k = common[v - view_ptr[c]];
          if (k != 0) iou += (double)k / (double)(in_bb[b].size() + views[v].size() - k);
        }
        ++matches;
        sum_score += iou / (double)(view_ptr[c + 1] - view_ptr[c]);
      }
    }
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  int64_t sum_overlap = 0;
  for (int64_t b = 0; b < n_box; ++b)
    for (int64_t v = 0; v < n_views; ++v)
      for (const uint64_t id : views[v]) if (in_bb[b].count(id)) ++sum_overlap;
  std::sort(ms.begin(), ms.end());
  printf("%.4f %lld %lld %lld %.17g\n", ms[ms.size() / 2], (long long)sum_count, (long long)sum_overlap, (long long)matches, sum_score);
  return 0;
}
