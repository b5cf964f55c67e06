// map_window.h -- what the entries that make a device-resident map share (map_resident.cpp: the map created; map_update.cpp: conditioned; map_extend.cpp: grown
// or gathered; map_merge.cpp: its duplicates merged): the checks of the window's map objects, the one-group cut of those objects in the handle's scratch
// buffers, the device view of the update, allocate_map, the end of a call on the cut's status record (finish_window_call), the posterior's way to the device
// (upload_posterior, posterior_from_handle), fold_window -- the one routine that brings a window back into a map -- and the start vector a map is given at birth.
// For the entries whose device arrays live for one call (map_merge.cpp, map_match.cpp, map_frame.cpp, map_locate.cpp): carve_workspace, which lays an entry's
// arrays out in the handle's one grow-only workspace; and finish_report, the two-wait tail of the two entries that report lists (match, locate).
#ifndef OBVI_MAP_WINDOW_H_
#define OBVI_MAP_WINDOW_H_
#include "ba_handle.h"
#include "../../include/obvi_map_resident.h"

#include <initializer_list>
#include <memory>

namespace obvi_lib {

struct MapDeleter { void operator()(obvi_map* m) const { obvi_map_destroy(m); } };

// the fixed start of the power iterations, [kMapGroupMaxRows]: every map is born with the same one
inline std::vector<double> map_power_start() {
  std::vector<double> x0((size_t)kMapGroupMaxRows);
  uint64_t lcg = 0x9e3779b97f4a7c15ull;
  for (double& v : x0) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; v = 0.5 + (double)(lcg >> 11) / 9007199254740992.0; }
  return x0;
}

inline bool twice(const uint32_t* idx, int64_t k) {
  std::vector<uint32_t> sorted(idx, idx + k);
  std::sort(sorted.begin(), sorted.end());
  return std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
}

// what every entry refuses about the map and the window's map objects, before anything is launched or allocated; rows: the window's rows that count against
// OBVI_MAP_GROUP_MAX_ROWS (a gather has none: 0)
inline int check_window(obvi_ba_handle* h, const obvi_map* map, int64_t k, const uint32_t* map_idx, int64_t rows, const std::string& what) {
  if (map->device != h->device) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": the map lives on another device than the handle");
  if (map->od != h->od) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": the map's object block size is not the handle's");
  if (rows > OBVI_MAP_GROUP_MAX_ROWS) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": a window of more than OBVI_MAP_GROUP_MAX_ROWS rows");
  for (int64_t i = 0; i < k; ++i) if ((int64_t)map_idx[i] >= map->n) return fail(h, OBVI_ERR_OUT_OF_RANGE, what + ": map index out of range");
  if (twice(map_idx, k)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": a map object twice");
  return OBVI_OK;
}

// what the handle forms refuse about the window's session objects before anything is planned
inline int check_session_objects(obvi_ba_handle* h, int64_t k, const uint32_t* obj_idx, const std::string& what) {
  for (int64_t i = 0; i < k; ++i) if ((int64_t)obj_idx[i] >= h->O) return fail(h, OBVI_ERR_OUT_OF_RANGE, what + ": object index out of range");
  if (twice(obj_idx, k)) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": a session object twice");
  for (int64_t i = 0; i < k; ++i) if (h->h_object_const[obj_idx[i]]) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": a constant object has no posterior");
  // the flags, not the plan's list: a handle that has not planned yet exchanges as soon as it does (validate_indices refuses group priors by the same test);
  // with obvi_map_allow_exchange on, the posterior is the joint one and the pass is collective (include/obvi_map_shared.h)
  if (!h->map_exchange && h->allreduce != nullptr && std::any_of(h->h_is_shared.begin(), h->h_is_shared.end(), [](uint8_t v) { return v != 0; })) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": the handle exchanges shared objects");
  return OBVI_OK;
}

// The posterior of the handle forms, after the checks above and check_ready: the joint covariance of the session objects obj_idx, all k x k pairs, and their
// current estimates, laid out in d_mu_post (covariance [k od][k od], then mean [k od]) on the handle's stream.  keep: the host tables the stages upload, alive
// until the caller's wait, as obj_idx is.
struct WindowPosterior { CovTables tables; std::vector<uint32_t> pa, pb; };
inline int posterior_from_handle(obvi_ba_handle* h, int64_t k, const uint32_t* obj_idx, const std::string& what, WindowPosterior& keep) {
  { const int vrc = validate_indices(h); if (vrc != OBVI_OK) return vrc; }
  prepare(h);
  for (int64_t i = 0; i < k; ++i) if (h->h_obj_vid[obj_idx[i]] < 0) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": an object that no active factor touches has no posterior");
  CovTables& tables = keep.tables;
  std::vector<uint32_t>& pa = keep.pa; std::vector<uint32_t>& pb = keep.pb;
  pa.resize((size_t)(k * k)); pb.resize((size_t)(k * k));
  for (int64_t a = 0; a < k; ++a) for (int64_t b = 0; b < k; ++b) { pa[(size_t)(a * k + b)] = obj_idx[a]; pb[(size_t)(a * k + b)] = obj_idx[b]; }
  int64_t ldt = 0;
  { const int rc = object_cov_forward(h, k * k, what.c_str(), &ldt, tables); if (rc != OBVI_OK) return rc; }
  if (ldt == 0) return fail(h, OBVI_ERR_INVALID_ARGUMENT, what + ": the handle has no variable objects");
  object_cov_pair_blocks(h, k * k, pa.data(), pb.data(), ldt, tables);
  const int64_t NP = k * h->od;
  h->d_mu_obj.upload(obj_idx, (size_t)k, h->stream);
  h->d_mu_post.resize((size_t)(NP * NP + NP));
  launch_map_posterior_layout(h->stream, h->d_cov_out.get(), h->d_obj.get(), h->d_mu_obj.get(), (int32_t)k, h->od, h->d_mu_post.get(), h->d_mu_post.get() + NP * NP);
  return OBVI_OK;
}

// The window's k map objects as one group of a cut (MapCutDev, ba_device.h) in the handle's scratch buffers of obvi_map_set_group_priors_from_map -- the handle's
// own groups are not touched -- with the status record zeroed.  k = 0: the status record alone.
inline MapCutDev window_cut(obvi_ba_handle* h, int64_t k, const uint32_t* map_idx) {
  const int od = h->od;
  const int64_t NA = k * od, nA = map_group_slabs(NA), ld = (NA + 1) & ~(int64_t)1, tile = (int64_t)kTile * kTile;
  hipStream_t s = h->stream;
  h->d_mc_status.resize((size_t)kMapStatusDoubles);
  h->d_mc_status.zero(s);
  MapCutDev m{};
  m.n = k > 0 ? 1 : 0; m.od = od; m.rows = NA; m.status = h->d_mc_status.get();
  if (k == 0) return m;
  const std::vector<MapCutGroup> cut{MapCutGroup{(int32_t)NA, (int32_t)nA, (int32_t)ld, 0, 0, 0, 0, 0, 0}};
  h->d_mc_groups.upload(cut, s); h->d_mc_map_idx.upload(map_idx, (size_t)k, s);
  h->d_mgn_mean.resize((size_t)NA); h->d_mgn_Lambda.resize((size_t)(NA * ld)); h->d_mgn_W.resize((size_t)(NA * NA));
  h->d_mc_A.resize((size_t)(nA * nA * tile)); h->d_mc_Wt.resize((size_t)(nA * nA * tile)); h->d_mc_Li.resize((size_t)(nA * tile));
  h->d_mc_Csym.resize((size_t)(NA * ld)); h->d_mc_x.resize((size_t)(4 * NA)); h->d_mc_partial.resize((size_t)2 * (kMapGroupMaxRows / 16));
  h->d_mgn_W.zero(s); h->d_mgn_Lambda.zero(s);
  m.groups = h->d_mc_groups.get(); m.map_idx = h->d_mc_map_idx.get();
  m.A = h->d_mc_A.get(); m.Li = h->d_mc_Li.get(); m.Wt = h->d_mc_Wt.get(); m.Csym = h->d_mc_Csym.get();
  m.mean = h->d_mgn_mean.get(); m.W = h->d_mgn_W.get(); m.Lambda = h->d_mgn_Lambda.get();
  m.x = h->d_mc_x.get(); m.partial = h->d_mc_partial.get();
  return m;
}

// The device view of the update (MapUpdateDev) over that cut: `map` (NULL: none) with its k window objects and k_new objects it lacks, the posterior in
// d_mu_post, the tile operands in d_mu_tiles, the result in `fresh`.
inline MapUpdateDev window_update(obvi_ba_handle* h, const obvi_map* map, int64_t k, int64_t k_new, const MapCutDev& m, obvi_map* fresh) {
  const int od = h->od;
  const int64_t NA = k * od, NB = k_new * od, N = map ? map->n * od : 0, nA = map_group_slabs(NA), nB = map_group_slabs(NB), nN = map_group_slabs(N), tile = (int64_t)kTile * kTile;
  h->d_mu_tiles.resize((size_t)((4 * nA * nA + 3 * nN * nA + 2 * nB * nA) * tile + kTile * nA));
  MapUpdateDev u{};
  u.od = od; u.N = (int32_t)N; u.NA = (int32_t)NA; u.nN = (int32_t)nN; u.nA = (int32_t)nA;
  u.NB = (int32_t)NB; u.nB = (int32_t)nB; u.ldp = (int32_t)(NA + NB); u.ldo = (int32_t)(N + NB);
  u.map_idx = m.map_idx; u.map_mean = map ? map->d_mean : nullptr; u.map_cov = map ? map->d_cov : nullptr;
  u.P = h->d_mu_post.get(); u.pm = h->d_mu_post.get() + (NA + NB) * (NA + NB);
  u.Wt = m.Wt; u.W = m.W; u.mean_A = m.mean;
  double* t = h->d_mu_tiles.get();
  u.Wn = t; u.Ps = u.Wn + nA * nA * tile; u.U = u.Ps + nA * nA * tile; u.M = u.U + nA * nA * tile;
  u.G = u.M + nA * nA * tile; u.Y = u.G + nN * nA * tile; u.Z = u.Y + nN * nA * tile; u.v = u.Z + nN * nA * tile;
  u.Pba = u.v + kTile * nA; u.V = u.Pba + nB * nA * tile;
  u.out_mean = fresh->d_mean; u.out_cov = fresh->d_cov; u.status = m.status;
  return u;
}

// the cut's pivot and condition tests on its status record: those of obvi_map_set_group_priors_from_map
inline bool window_cut_spd(const double* st) {
  return st[MS_BAD] == 0.0 && st[MS_PIV_MIN] * st[MS_PIV_MIN] > 1e-13 * st[MS_PIV_MAX] * st[MS_PIV_MAX] && st[MS_EV_C] * st[MS_EV_LAMBDA] <= 1e13;
}

// A map of n objects with its three buffers allocated and nothing in them: the one place a map is made.  Throws HipError; the device is the current one.
inline std::unique_ptr<obvi_map, MapDeleter> allocate_map(int device, int od, int64_t n) {
  std::unique_ptr<obvi_map, MapDeleter> fresh(new obvi_map());
  fresh->device = device; fresh->od = od; fresh->n = n;
  const int64_t rows = n * od;
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_mean), sizeof(double) * rows));
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_cov), sizeof(double) * rows * rows));
  OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&fresh->d_x0), sizeof(double) * kMapGroupMaxRows));
  return fresh;
}
// ... and the start vector of the map it comes from, on the stream
inline void inherit_power_start(obvi_map* fresh, const obvi_map* from, hipStream_t s) {
  OBVI_HIP(hipMemcpyAsync(fresh->d_x0, from->d_x0, sizeof(double) * kMapGroupMaxRows, hipMemcpyDeviceToDevice, s));
}

// The end of a call that launched on a window's cut: the cut's status record read back behind the call's one wait -- either map may go away from here on, and
// any stream may read the new one -- then the cut's tests (factored: a cut was factored) and the flag of a non-finite entry, each refused in the entry's words.
inline int finish_window_call(obvi_ba_handle* h, bool factored, const std::string& not_spd, const std::string& non_finite) {
  OBVI_HIP(hipGetLastError());
  double st[kMapStatusDoubles];
  h->d_mc_status.download(st, (size_t)kMapStatusDoubles, h->stream);
  sync(h);
  if (factored && !window_cut_spd(st)) return fail(h, OBVI_ERR_NUMERICAL, not_spd);
  if (st[MS_NONFINITE] != 0.0) return fail(h, OBVI_ERR_NUMERICAL, non_finite);
  return OBVI_OK;
}

// The workspace of the entries whose device arrays live for one call -- merge, match, transform, locate; each ends in a wait, so nothing in it outlives its
// call -- carved out of the handle's d_map_ws.  An entry lists its arrays once, as take<element type>(count), in a function that runs twice: once to measure,
// once, the buffer grown to the sum, to hand the pointers out at offsets that are multiples of 256 bytes.  The regions of one call alias those of the last in
// another way every time: whatever a kernel reads must have been written on the stream by this call (the *Dev structs of ba_device.h say by whom).
struct Carver {
  char* base; size_t bytes = 0;
  template <class T> T* take(int64_t count) {
    T* p = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
    bytes += (sizeof(T) * (size_t)count + 255) & ~(size_t)255;
    return p;
  }
};
template <class List>
inline void carve_workspace(obvi_ba_handle* h, List&& list) {
  Carver measure{nullptr};
  list(measure);
  h->d_map_ws.resize(measure.bytes);
  Carver hand_out{h->d_map_ws.get()};
  list(hand_out);
}

// The end of a report entry (match, locate), after the launches that leave three int64 totals at d_totals.  The launch-error check and the totals read back
// behind the first wait; then between(totals, out), out = min(totals[found_at], cap) the entries to report: what the entry refuses on the totals (anything but
// OBVI_OK is returned as it is) and the launches that need them; then the first `out` entries of every caller array (host NULL: an optional array left out)
// and the second wait, only when out > 0; the totals into counts last.  Nothing behind entry `out` of a caller's array is written.
struct ReportArray { void* host; const void* dev; size_t entry_bytes; };
template <class Between>
inline int finish_report(obvi_ba_handle* h, const int64_t* d_totals, int found_at, int64_t cap, std::initializer_list<ReportArray> arrays, int64_t* counts, Between&& between) {
  hipStream_t s = h->stream;
  OBVI_HIP(hipGetLastError());
  int64_t totals[3];
  OBVI_HIP(hipMemcpyAsync(totals, d_totals, sizeof(totals), hipMemcpyDeviceToHost, s));
  sync(h);   // the first wait: the three totals
  const int64_t out = std::min(totals[found_at], cap);
  { const int rc = between(totals, out); if (rc != OBVI_OK) return rc; }
  if (out > 0) {
    for (const ReportArray& a : arrays) if (a.host) OBVI_HIP(hipMemcpyAsync(a.host, a.dev, a.entry_bytes * (size_t)out, hipMemcpyDeviceToHost, s));
    sync(h);   // the second: the entries, only when there are some to report
  }
  std::copy(totals, totals + 3, counts);
  return OBVI_OK;
}

// The posterior of the host-pointer forms, NP rows: refused unless every entry is finite, then copied into d_mu_post (covariance [NP][NP], then mean [NP]) on
// the handle's stream.
inline int upload_posterior(obvi_ba_handle* h, int64_t NP, const double* post_mean, const double* post_cov, const std::string& what) {
  for (int64_t i = 0; i < NP; ++i) if (!std::isfinite(post_mean[i])) return fail(h, OBVI_ERR_NUMERICAL, what + ": a posterior mean that is not finite");
  for (int64_t i = 0; i < NP * NP; ++i) if (!std::isfinite(post_cov[i])) return fail(h, OBVI_ERR_NUMERICAL, what + ": a posterior covariance entry that is not finite");
  OBVI_HIP(hipSetDevice(h->device));
  h->d_mu_post.resize((size_t)(NP * NP + NP));
  h2d_async(h->d_mu_post.get(), post_cov, sizeof(double) * (size_t)(NP * NP), h->stream);
  h2d_async(h->d_mu_post.get() + NP * NP, post_mean, sizeof(double) * (size_t)NP, h->stream);
  return OBVI_OK;
}

// One window brought back into a map -- the routine behind the condition and the extend entries -- with the posterior over (A, B) in d_mu_post (covariance
// [N_A + N_B]^2, then mean) on the handle's stream: A the window's k_old objects of `map`, cut from it as one group and factored; B its k_new objects the map
// lacks, appended.  k_new = 0 conditions the map; map NULL (k_old = 0): a first map, the posterior itself.  Launches into a freshly allocated map, reads the
// cut's status record back and hands the new map out only when nothing was refused.  One wait.
inline int fold_window(obvi_ba_handle* h, const obvi_map* map, int64_t k_old, const uint32_t* map_idx, int64_t k_new, const std::string& what, obvi_map** out) {
  const int od = h->od;
  const int64_t n = map ? map->n : 0, N = n * od, NA = k_old * od, NB = k_new * od, nA = map_group_slabs(NA);
  hipStream_t s = h->stream;
  const MapCutDev m = window_cut(h, k_old, map_idx);
  std::unique_ptr<obvi_map, MapDeleter> fresh = allocate_map(h->device, od, n + k_new);
  const std::vector<double> x0 = map ? std::vector<double>() : map_power_start();   // alive until the wait
  if (map) inherit_power_start(fresh.get(), map, s);
  else h2d_async(fresh->d_x0, x0.data(), sizeof(double) * x0.size(), s);
  const MapUpdateDev u = window_update(h, map, k_old, k_new, m, fresh.get());
  if (k_old > 0) {   // the condition test reads the largest eigenvalue of Lambda = Cs_AA^-1, so the cut runs whole: factor, then Lambda and the power steps
    launch_map_factor(s, m, (int)nA, map->d_mean, map->d_cov, N);
    launch_map_condition_estimate(s, m, (int)nA, map->d_x0);
  } else if (N > 0) {
    OBVI_HIP(hipMemsetAsync(fresh->d_cov, 0, sizeof(double) * (size_t)((N + NB) * (N + NB)), s));   // no product fills the cross blocks: they are zero
  }
  launch_map_extend(s, u);
  { const int rc = finish_window_call(h, k_old > 0, what + ": the map's covariance of the window's objects is not SPD, or numerically singular",
                                      what + ": a non-finite entry in the posterior or in the new map"); if (rc != OBVI_OK) return rc; }
  *out = fresh.release();
  return OBVI_OK;
}

}  // namespace obvi_lib
#endif  // OBVI_MAP_WINDOW_H_
