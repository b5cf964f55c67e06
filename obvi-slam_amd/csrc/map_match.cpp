// map_match.cpp -- include/obvi_map_match.h: duplicate objects of a device-resident map proposed (map_kernels.hip).  The host checks the arguments, carves the
// workspaces out of the handle's one-call workspace (map_window.h), launches, and ends in the report tail it shares with the locate (finish_report).  The
// resolver that turns the pairs into the lists of obvi_map_merge is plain host code below it.
#include "map_window.h"
#include "../../include/obvi_map_match.h"

#include <unordered_map>

extern "C" {

int obvi_map_match(obvi_ba_handle* h, const obvi_map* map, const int32_t* label, uint32_t row_mask, double gate, double max_centre_distance, double yaw_period,
                   int64_t capacity, uint32_t* idx_a, uint32_t* idx_b, double* stat, double* yaw_offset, int64_t* counts) {
  if (!h || !map || !counts || capacity < 0 || (capacity > 0 && (!idx_a || !idx_b || !stat || !yaw_offset))) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_match: bad arguments");
  const int od = h->od;
  // device and block size: the checks of every window, with no objects named
  { const int rc = check_window(h, map, 0, nullptr, 0, "map_match"); if (rc != OBVI_OK) return rc; }
  if (row_mask >> od) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_match: row_mask names a parameter the block does not have");
  if (!(std::isfinite(gate) && gate > 0.0)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_match: the gate must be finite and positive");
  if (!(max_centre_distance > 0.0)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_match: max_centre_distance must be positive (+inf: no test)");
  if (!(yaw_period >= 0.0) || !std::isfinite(yaw_period)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_match: yaw_period must be finite and not negative");
  if (yaw_period > 0.0 && od != 7) return fail(h, OBVI_ERR_INVALID_ARGUMENT, "map_match: a yaw period needs the 7-parameter block");
  OBVI_API_BEGIN
  OBVI_HIP(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int64_t n = map->n, cap = std::min(capacity, n * (n - 1) / 2);
  MapMatchDev m{};
  m.od = od; m.n = (int32_t)n; m.mask = row_mask ? row_mask : (1u << od) - 1u; m.use_dist = std::isinf(max_centre_distance) ? 0 : 1;
  m.gate = gate; m.dist2 = max_centre_distance * max_centre_distance; m.period = yaw_period; m.capacity = cap;
  m.map_mean = map->d_mean; m.map_cov = map->d_cov;
  int32_t* d_label = nullptr;
  carve_workspace(h, [&](Carver& c) {
    if (label) d_label = c.take<int32_t>(n);
    m.diag = c.take<double>(n * od * od); m.stat = c.take<double>(n * n);   // stat: k_mt_pairs writes the pairs a < b, and nothing else is read
    m.row_cnt = c.take<int64_t>(3 * n); m.row_off = c.take<int64_t>(n); m.totals = c.take<int64_t>(3);
    m.out_a = c.take<uint32_t>(cap); m.out_b = c.take<uint32_t>(cap); m.out_stat = c.take<double>(cap); m.out_yaw = c.take<double>(cap);
  });
  if (label) h2d_async(d_label, label, sizeof(int32_t) * (size_t)n, s);
  m.label = d_label;
  launch_map_match(s, m);
  return finish_report(h, m.totals, 0, cap, {{idx_a, m.out_a, sizeof(uint32_t)}, {idx_b, m.out_b, sizeof(uint32_t)}, {stat, m.out_stat, sizeof(double)}, {yaw_offset, m.out_yaw, sizeof(double)}},
                       counts, [](const int64_t*, int64_t) { return (int)OBVI_OK; });
  OBVI_API_END(h)
}

int obvi_map_match_resolve(int32_t object_block_size, int64_t n_pairs, const uint32_t* idx_a, const uint32_t* idx_b, const double* stat, int64_t max_pairs,
                           uint32_t* drop, uint32_t* keep, uint32_t* sel, int64_t* q) {
  if (!idx_a || !idx_b || !stat || !drop || !keep || !sel || !q || n_pairs < 0 || max_pairs < 1) return OBVI_ERR_INVALID_ARGUMENT;
  if (object_block_size != 0 && object_block_size != 7 && object_block_size != 9) return OBVI_ERR_INVALID_ARGUMENT;
  const int od = object_block_size ? object_block_size : 7;
  if (max_pairs > OBVI_MAP_GROUP_MAX_ROWS / od) return OBVI_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n_pairs; ++i) if (idx_a[i] >= idx_b[i]) return OBVI_ERR_INVALID_ARGUMENT;
  for (int64_t i = 0; i < n_pairs; ++i) if (!(std::isfinite(stat[i]) && stat[i] >= 0.0)) return OBVI_ERR_NUMERICAL;
  try {
    std::vector<int64_t> order((size_t)n_pairs);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
      if (stat[x] != stat[y]) return stat[x] < stat[y];
      if (idx_a[x] != idx_a[y]) return idx_a[x] < idx_a[y];
      if (idx_b[x] != idx_b[y]) return idx_b[x] < idx_b[y];
      return x < y;
    });
    enum : uint8_t { FREE = 0, KEEP, DROPPED };
    std::unordered_map<uint32_t, uint8_t> state;
    std::vector<uint32_t> out_drop, out_keep, out_sel;
    for (int64_t i : order) {
      if ((int64_t)out_drop.size() == max_pairs) break;
      uint8_t& sa = state[idx_a[i]];
      if (sa == DROPPED) continue;
      uint8_t& sb = state[idx_b[i]];
      if (sb != FREE) continue;
      sa = KEEP; sb = DROPPED;
      out_drop.push_back(idx_b[i]); out_keep.push_back(idx_a[i]); out_sel.push_back((uint32_t)i);
    }
    std::copy(out_drop.begin(), out_drop.end(), drop); std::copy(out_keep.begin(), out_keep.end(), keep); std::copy(out_sel.begin(), out_sel.end(), sel);
    *q = (int64_t)out_drop.size();
  } catch (...) { return OBVI_ERR_HIP; }
  return OBVI_OK;
}

}  // extern "C"
