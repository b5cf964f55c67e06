// ba_device.h -- HBM layout of one bundle-adjustment problem and the kernel launch entry points.
// See DESIGN.md ("Data layout in HBM") for the rationale.
#ifndef OBVI_BA_DEVICE_H_
#define OBVI_BA_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ba_math.h"

struct obvi_ba_handle;
namespace obvi {
// what the front-end gating calls (frontend_kernels.hip) need of a handle: its device, its stream, its error slot
hipStream_t handle_stream(obvi_ba_handle* h);
int handle_device(const obvi_ba_handle* h);
int handle_fail(obvi_ba_handle* h, int code, const char* msg);
void make_dev_cam(const double* K4, const double* ext7, DevCam* out);

// Tile edge of the reduced (Schur) system.  The reduced matrix is stored as a grid of
// kTile x kTile fp64 tiles (row-major inside a tile, tiles row-major in the grid); only tiles
// in the lower triangle that are structurally non-zero after symbolic fill are ever touched.
constexpr int kTile = 64;
// k_point_pass: a wavefront assembles the part of the Z storage that belongs to its piece of the observation list (records of 18 doubles + a
// 4-double tail per point) in LDS and writes it out with coalesced 16-byte stores.  The host cuts the pieces (upload.cpp) so that an image never
// exceeds this many doubles: 64 observations + 28 points.  1264 doubles x 4 wavefronts = 40 KB per workgroup, FOUR workgroups per compute unit
// (160 KB of LDS) = 4 wavefronts per SIMD at <= 128 VGPRs; the round-1..4 layout (22 * 64 doubles, any 64 points) stopped at three (round 5).
#ifndef OBVI_POINT_IMAGE_DOUBLES
#define OBVI_POINT_IMAGE_DOUBLES 1264
#endif
constexpr int kPointImageDoubles = OBVI_POINT_IMAGE_DOUBLES;

// Slots of the device scalar block (fp64 unless noted).  One 256-byte D2H copy per LM step.
enum Scalar {
  // slots [SC_COST, SC_SUM_END) are summed across ranks in a multi-GPU solve, SC_GMAX_BITS is maximised
  SC_COST = 0,        // 0.5 sum rho(s) over the reduced program at the linearisation point
  SC_COST_CAND,       // same at the candidate point
  SC_GSQ,             // |g|^2
  SC_XSQ,             // |x|^2 over the reduced program
  SC_STEPSQ,          // |delta|^2
  SC_MODEL_CHANGE,    // -(J d)^T (r + J d / 2)
  SC_CHOL_FAIL,       // (as double) count of non-positive pivots
  SC_NONFINITE,       // (as double) count of non-finite step entries
  SC_WAIT_TIMEOUT,    // (as double) potrf workgroups of k_update_potrf whose wait for the previous level's jobs timed out: a scheduling
                      // failure, not a numerical one -- obvi_ba_solve returns OBVI_ERR_HIP (summed across ranks so that every rank does)
  SC_SUM_END,
  SC_GMAX_BITS = SC_SUM_END,  // max |g_i| (IEEE bits, via integer atomicMax; non-negative doubles order like u64)
  SC_COST_FIXED,      // residual blocks whose every parameter block is constant
  SC_TAIL_ORDER,      // multi-GPU: a 40-bit hash of this rank's order of the shared tail (as double); summed with SC_COST_FIXED at the start of a solve:
                      // every rank must find world x its own value (the tail's tiles are summed across ranks position by position)
  SC_COUNT = 32
};

// Deterministic mode (obvi_ba_options.deterministic).  The sums a solve's decisions are taken from -- costs, |g|^2, |x|^2, |delta|^2, the
// model cost change -- are then not added to the scalar block with fp64 atomics (whose order changes from run to run): workgroup b of
// a kernel stores its partial sum at scal[SC_COUNT + slot * stride + b], and a one-workgroup-per-slot kernel behind it adds them up
// in a fixed order (launch_reducing in ba_kernels.hip, which refuses a grid larger than the stride before the kernel).  stride = BlocksDev.deterministic,
// the room the handle gave the slots for the problem it holds (ensure_det_slots in ba_handle.h: det_slots_needed below, rounded up to OBVI_DET_MIN_STRIDE x 2^k).
// What stays atomic in this mode, and why the result is still the same from run to run:
//   - counters (failed pivots, non-finite entries: small integers) and the gradient maximum (integer max): exact in any order;
//   - the fp64 adds into the reduced system's tiles, right-hand side and diagonal (k_schur_window, k_schur_blocks, k_reduced_diag, the
//     small-factor gathers, the tile Cholesky's updates): every address has ONE writer per kernel -- the plan never cuts a strip, a block's
//     pair list, a target tile's products or a tile row over workgroups in this mode (prepare_plan), the small factors go through per-factor
//     scratch and a gather -- and all kernels run on one stream, so the adds reach an address in launch order.  The atomic is then only
//     the instruction the non-deterministic build shares; tests/test_gpu_deterministic.py holds reruns to bit-identity.
constexpr int kDetSlots = 7;
constexpr int64_t kDetMaxStride = 1 << 24;   // 2^24 workgroups per kernel: beyond any problem that fits the device
inline __host__ __device__ int det_slot_of(int sc) {
  return sc == SC_COST ? 0 : sc == SC_COST_CAND ? 1 : sc == SC_GSQ ? 2 : sc == SC_XSQ ? 3 : sc == SC_STEPSQ ? 4 : sc == SC_MODEL_CHANGE ? 5 : sc == SC_COST_FIXED ? 6 : -1;
}
inline __host__ __device__ int det_scalar_of(int slot) {
  return slot == 0 ? SC_COST : slot == 1 ? SC_COST_CAND : slot == 2 ? SC_GSQ : slot == 3 ? SC_XSQ : slot == 4 ? SC_STEPSQ : slot == 5 ? SC_MODEL_CHANGE : SC_COST_FIXED;
}
// The grid of every kernel that leaves partial sums, defined once: its launcher in ba_kernels.hip launches it, det_slots_needed sizes the slots by it.
// A grid made of parts adds up over them: with the other parts' counts at 0 it is one part's workgroups (the boundaries the launchers hand the kernels).
constexpr int kBaBlock = 256;   // threads per workgroup of the ba_kernels.hip kernels (kBlock there) but k_small_lin_lanes and k_eval_small (64)
// (k_bbox_lin_dense packs four workgroups of k_small_lin_lanes' bounding-box part into one and leaves their four partial sums: the grid below counts for both)
inline int64_t blocks_of(int64_t n, int64_t per) { return (n + per - 1) / per; }
inline int64_t point_pass_grid(int64_t n_waves) { return blocks_of(n_waves, kBaBlock / 64); }   // k_point_pass: a wavefront per piece of the observation list
inline int64_t point_pass_long_grid(int64_t n_long) { return blocks_of(n_long, kBaBlock); }     // k_point_pass_long: a thread per long-track point
// k_small_lin_lanes: 16 lanes per box / relative pose, one per prior; a map pair prior has 2 od rows: 16 lanes (od = 7), 32 (od = 9)
inline int64_t map_pair_per_block(int64_t od) { return od > 7 ? 2 : 4; }
inline int64_t small_lin_grid(int64_t n_bb, int64_t n_priors, int64_t n_rl, int64_t n_mp = 0, int64_t od = 7) {
  return blocks_of(n_bb, 4) + blocks_of(n_priors, 64) + blocks_of(n_rl, 4) + blocks_of(n_mp, map_pair_per_block(od));
}
inline int64_t reduced_diag_grid(int64_t P, int64_t O, int64_t od) { return blocks_of((od > 8 ? 16 : 8) * (P + O), kBaBlock); }   // k_reduced_diag: 8 threads per diagonal block, 16 if od > 8
// k_backsub_apply: `lanes` per feature on at most 2048 workgroups (8 per CU), then a thread per pose / object
inline int64_t backsub_grid(int64_t L, int64_t P, int64_t O, int lanes) { return std::min<int64_t>(blocks_of(L * lanes, kBaBlock), 2048) + blocks_of(P + O, kBaBlock); }
inline int64_t cost_grid(int64_t P, int64_t n_obs, int64_t n_small) { return (n_obs > 0 ? P : 0) + blocks_of(n_small, kBaBlock); }   // k_cost: a workgroup per pose, a thread per small factor
inline int64_t eval_reproj_grid(int64_t n_obs) { return blocks_of(n_obs, kBaBlock); }   // k_eval_reproj, k_eval_small: a thread per factor
inline int64_t eval_small_grid(int64_t n_small) { return blocks_of(n_small, 64); }
// map group priors (include/obvi_map_group_prior.h), rows N = k od of a group: k_map_group_quad and k_map_group_eval run a workgroup per 64-row slab of a group's
// matrix, k_map_group_scatter one per 64 x 64 tile of its lower triangle, k_map_group_cost one per group
inline int64_t map_group_slabs(int64_t rows) { return blocks_of(rows, 64); }
inline int64_t map_group_tiles(int64_t rows) { const int64_t t = blocks_of(rows, 64); return t * (t + 1) / 2; }
// The factor families in the order obvi_ba_evaluate lays them out (DESIGN.md "Factor families"; the table of their records: ba_handle.h), and that layout:
// per family its first block norm and its first residual row, at [FAM_COUNT] the totals
enum Family { FAM_RP = 0, FAM_BB, FAM_SP, FAM_LT, FAM_RL, FAM_MP, FAM_MG, FAM_COUNT };
struct EvalLayout { int64_t slot[FAM_COUNT + 1], row[FAM_COUNT + 1]; };
// the factors that k_cost and k_eval_small give a thread each: every family of SmallFactorsDev (c: it, or DetCounts)
template <class C>
inline int64_t num_small_factors(const C& c) { return c.n_bb + c.n_sp + c.n_lt + c.n_rl + c.n_mp; }
// the largest of those grids (launch_backsub_apply takes at most 32 lanes per feature), at least 1 for an empty problem: the stride is also the mode's flag
struct DetCounts { int64_t P, L, O, od, n_rp, n_point_waves, n_long_points, n_bb, n_sp, n_lt, n_rl, n_mp = 0, mg_tiles = 0; };   // (mg_tiles: the scatter grid, the largest of the group kernels')
inline int64_t det_slots_needed(const DetCounts& c) {
  const int64_t ns = num_small_factors(c);
  return std::max<int64_t>({1, point_pass_grid(c.n_point_waves), point_pass_long_grid(c.n_long_points), small_lin_grid(c.n_bb, c.n_sp + c.n_lt, c.n_rl, c.n_mp, c.od),
                            reduced_diag_grid(c.P, c.O, c.od), backsub_grid(c.L, c.P, c.O, 32), cost_grid(c.P, c.n_rp, ns), eval_reproj_grid(c.n_rp), eval_small_grid(ns), c.mg_tiles});
}

struct ReprojDev {          // observations sorted by (point, pose): CSC by point
  int64_t n;
  const uint32_t* pose;     // [n]
  const uint32_t* point;    // [n]
  const uint16_t* cam;      // [n]
  const double2* pixel;     // [n]
  const double* sigma;      // [n]
  const uint8_t* active;    // [n]
  const int32_t* yrow;      // [n] first row of the observing pose in the reduced system, -1 if the observation is inactive or the pose constant
  const uint32_t* point_ptr;  // [L+1] offsets into the arrays above
  double huber;
};

struct ReprojPoseDev {      // the same observations sorted by (pose, point): CSR by pose, for the pose-side pass
  int64_t n;
  const uint32_t* point;    // [n]
  const uint16_t* cam;      // [n]
  const double2* pixel;     // [n]
  const double* sigma;      // [n]
  const uint8_t* active;    // [n]
  const uint32_t* pose_ptr; // [P+1]
  double huber;
};

struct BlocksDev {          // parameter blocks + reduced-program bookkeeping
  int64_t P, L, O;
  int64_t nPv, nOv;         // variable+used poses / objects
  int64_t m;                // rows of the tile grid in use (elimination order, nodes padded to tile boundaries)
  const int32_t* pose_row;  // [nPv] reduced pose index -> first row of its 6x6 diagonal block in the tile grid
  const int32_t* obj_row;   // [nOv] reduced object index -> first row of its od x od diagonal block
  const uint8_t* obj_shared; // [nOv] or NULL: object block is shared across ranks (multi-GPU exchange)
  int32_t shared_owner;     // 1 on the rank that contributes the shared objects' diagonal blocks and scalars
  const int32_t* pose_vid;  // [P]  reduced index or -1
  const int32_t* obj_vid;   // [O]
  const uint8_t* point_var; // [L]
  int32_t analytic_rotation; // the pose caches follow the analytic-Jacobian functor (make_pose_cache, ba_math.h)
  int32_t deterministic;     // obvi_ba_options.deterministic: 0, or the stride of the per-workgroup partial sums behind the scalar block that replace the fp64 atomics
  int32_t od;                // parameters of an ellipsoid block: 7 (x y z yaw dx dy dz: the reference's build) or 9 (x y z ax ay az dx dy dz; obvi_ba_options.object_block_size)
};
// k_pose_pass runs one workgroup per pose (no slices, no atomics) above this many poses and on every deterministic handle: the form whose sums can be
// staged per pose, and that the trial cost can produce at the candidate (launch_pose_pass, launch_cost)
constexpr int64_t kPoseSliceBelow = 256;
inline bool pose_pass_unsliced(const BlocksDev& b) { return b.deterministic != 0 || b.P > kPoseSliceBelow; }

struct SmallFactorsDev {    // N <= ~3e4 each; arrays in caller order
  int32_t od;               // parameters of an ellipsoid block (BlocksDev.od)
  // bounding boxes
  int64_t n_bb; const uint32_t* bb_obj; const uint32_t* bb_pose; const uint16_t* bb_cam;
  const double* bb_rect; const double* bb_sqrt_inf; const uint8_t* bb_active; double bb_huber, bb_invalid;
  double* bb_blk;                                       // [n_bb][62] ([81] with the 9-parameter block) per-factor diagonal blocks (big problems: k_small_lin_lanes<true> / k_bbox_gather)
  int32_t bb_pairs_unique;                              // no (object, pose) pair occurs twice: the off-diagonal block of a factor is its own
  const uint32_t* bbo_ptr; const uint32_t* bbo_idx;     // factors by object: [O+1], [n_bb]
  const uint32_t* bbp_ptr; const uint32_t* bbp_idx;     // factors by pose:   [P+1], [n_bb]
  // deterministic mode: the priors and the relative-pose factors go the same way -- per-factor blocks into a scratch (slot = shape prior i,
  // then n_sp + LTM prior i, then n_sp + n_lt + relative-pose factor i; kBbBlk doubles: first block | second block), summed per target
  // block in list order by k_small_gather.  Targets: objects [0, O), then poses [O, O + P); entry = 2 slot + side (1: the slot's second block).
  // A map pair prior i takes two slots behind those, n_sp + n_lt + n_rl + 2 i (object a) and + 2 i + 1 (object b): two object blocks do not fit one
  double* sm_blk; const uint32_t* smt_ptr; const uint32_t* smt_idx;
  // shape priors
  int64_t n_sp; const uint32_t* sp_obj; const double* sp_mean; const double* sp_sqrt_inf; const uint8_t* sp_active; double sp_huber;
  // LTM priors
  int64_t n_lt; const uint32_t* lt_obj; const double* lt_mean; const double* lt_sqrt_inf; const uint8_t* lt_active; double lt_huber;
  // relative poses
  int64_t n_rl; const uint32_t* rl_a; const uint32_t* rl_b; const double* rl_t; const double* rl_R; const double* rl_sqrt_inf;
  const uint8_t* rl_active; double rl_huber;
  // map pair priors (include/obvi_map_prior.h), N = 2 od: mean [n][N] (a's, then b's), W [n][N][N] (r = W d), Lambda = W^T W [n][N][N]
  int64_t n_mp; const uint32_t* mp_a; const uint32_t* mp_b; const double* mp_mean; const double* mp_W; const double* mp_Lambda;
  const uint8_t* mp_active; double mp_huber;
};

// Map group priors (include/obvi_map_group_prior.h).  Group g: members [ptr[g], ptr[g + 1]) of obj / mean (od doubles each), N_g = od x members rows.
// Lambda_g: N_g rows of ld_g = N_g rounded up to even doubles at lam_off[g] (16-byte rows: k_map_group_quad loads pairs); W_g: lower triangular, N_g x N_g
// at w_off[g], no padding (obvi_ba_debug_linearize hands it out as it is).  Rows of all groups one after the other: row od ptr[g] + i <-> y, residuals.
// Work lists: slab (group, 64 rows) and tile (group, ti << 16 | tj, tj <= ti), group after group; slab_ptr[g] / tile_ptr[g]: a group's first.
struct MapGroupDev {
  int64_t n; int32_t od;
  const int64_t* ptr; const uint32_t* obj; const double* mean; const uint8_t* active; double huber;
  const int64_t* lam_off; const double* Lambda; const int64_t* w_off; const double* W;
  int64_t n_slabs, n_tiles;
  const int32_t* slab_ptr; const int32_t* slab_grp; const int32_t* tile_ptr; const int32_t* tile_grp; const int32_t* tile_ij;
  double* y;         // [rows] Lambda d of the last k_map_group_quad
  double* partial;   // [n_slabs] the slabs' sum d_i y_i (or sum r_i^2: k_map_group_eval)
};

// Group priors cut from a device-resident map (include/obvi_map_resident.h; map_kernels.hip).  Group g of a call: N rows in nt = ceil(N / 64) tile rows; its
// tile workspaces (A -> L and Wt: nt x nt tiles each) start at tile tile0, the inverses of its diagonal tiles at tile diag0; members [member0, member0 + N / od)
// of map_idx; Lambda / Csym (N rows of ld doubles) at lam_off, W (N x N) at w_off -- the offsets of MapGroupDev.
constexpr int kMapGroupMaxRows = 2048;   // OBVI_MAP_GROUP_MAX_ROWS
constexpr int64_t kMapMaxRows = 11585;   // floor(sqrt(2^30 / 8)): rows of a map whose covariance takes 1 GiB, the largest a map may have
constexpr int kMapPowerSteps = 40;       // power steps of the condition estimate, on C and on Lambda
enum MapStatus { MS_BAD = 0, MS_PIV_MIN, MS_PIV_MAX, MS_EV_C, MS_EV_LAMBDA, MS_NONFINITE, kMapStatusDoubles = 8 };   // one record per group, read back once per call (MS_NONFINITE: the map update's alone)
struct MapCutGroup { int32_t N, nt, ld, pad; int64_t tile0, diag0, member0, lam_off, w_off; };
struct MapCutDev {
  int64_t n; int32_t od; int64_t rows;   // groups of the call; rows of all of them
  const MapCutGroup* groups; const uint32_t* map_idx;
  double* A; double* Li; double* Wt; double* Csym;   // workspaces
  double* mean; double* W; double* Lambda;           // the outputs: the layout of MapGroupDev
  double* x; double* partial; double* status;        // power iterates [2][2][rows], Rayleigh parts [n][2][kMapGroupMaxRows / 16], status [n][kMapStatusDoubles]
};
// gather, Cholesky by tile column (three launches per column of the largest group), W = L^-1, Lambda = W^T W, kMapPowerSteps power steps, the status records.
// W and the padding of Lambda must have been zeroed on the stream.  x0: kMapGroupMaxRows doubles, the fixed start of the power iterations.
void launch_map_cut(hipStream_t s, const MapCutDev& m, int nt_max, const double* map_mean, const double* map_cov, int64_t ldc, const double* x0);
// ... its two halves, which launch_map_cut runs one after the other: gather, Cholesky and W (the factor); Lambda, the power steps and the status records (what
// the condition test reads).
void launch_map_factor(hipStream_t s, const MapCutDev& m, int nt_max, const double* map_mean, const double* map_cov, int64_t ldc);
void launch_map_condition_estimate(hipStream_t s, const MapCutDev& m, int nt_max, const double* x0);
// ... and the factor without its gather: Cholesky and W of an A (lower tiles, identity padding) that another launch filled on the stream
void launch_map_factorize(hipStream_t s, const MapCutDev& m, int nt_max);

// A map conditioned on the posterior of some of its objects (include/obvi_map_update.h; map_kernels.hip): C' = Cs - Z Y^T, mu' = mu + Y v with Y = Cs[:, A] W^T,
// Z = Y (I - W Ps W^T), v = W (m - mu_A), W = L^-1 of Cs_AA = L L^T -- the factor of a one-group cut of the window's objects A, which ran before on the stream and
// left Wt (its tiles of W^T), W (dense, N_A x N_A), mean_A and the status record.  N map rows in nN tile rows, N_A window rows in nA; every tile operand is
// [tile rows][nA] tiles of 64 x 64, tile-major (chol_tile.h), the ragged last tiles padded with zeros (Wn: with the identity, as the cut pads).
// The same launches grow the map (include/obvi_map_extend.h): the window also held N_B rows of objects B the map lacks, the posterior is over (A, B) with the
// leading dimension ldp = N_A + N_B, and the new map has ldo = N + N_B rows, B behind the old ones: C'[old, B] = Y V^T with V = Ps_BA W^T.  A map that is only
// conditioned has N_B = 0, ldp = N_A, ldo = N.  C' and mu' come from the downdate path the merge below shares (map_kernels.hip: k_map_downdate, k_map_wd,
// k_map_mean), here on the old map's own rows.
struct MapUpdateDev {
  int32_t od, N, NA, nN, nA;
  int32_t NB, nB, ldp, ldo;                                  // rows of B in nB tile rows; leading dimensions of P and of out_cov
  const uint32_t* map_idx;                                   // [N_A / od] the window's map objects
  const double* map_mean; const double* map_cov;             // the old map: [N], [N][N]
  const double* P; const double* pm;                         // the posterior: covariance [N_A][N_A] as given (not symmetrised), mean [N_A]
  const double* Wt; const double* W; const double* mean_A;   // of the cut
  double* Wn; double* Ps; double* U; double* M;              // [nA][nA] tiles: W, (P + P^T) / 2, W Ps, I - W Ps W^T
  double* G; double* Y; double* Z;                           // [nN][nA] tiles: Cs[:, A], G W^T, Y M
  double* v;                                                 // [64 nA]
  double* Pba; double* V;                                    // [nB][nA] tiles: Ps_BA, Ps_BA W^T (a map that grows)
  double* out_mean; double* out_cov;                         // the new map: [ldo], [ldo][ldo]
  double* status;                                            // the cut's record: MS_NONFINITE is set to 1 by whoever writes a non-finite entry of the new map
};
// The map conditioned and, N_B > 0, grown by B: the operands (Wn and Ps_AA, G, Y, U, M, Z), Ps_BA staged and V, v, the downdate C' and mu' on the old map's
// rows, the cross block Y V^T along the rows of both of its copies, and the window's whole (A, B) block and means scattered last.  N_B = 0 (the condition):
// Ps_BA, V and the cross block are skipped -- ten launches.  N_A = 0: the old block is symmetrised and copied (out_cov's cross blocks must have been zeroed on
// the stream); N = 0 too: the scatter alone.  No grid has a zero dimension.  status[MS_NONFINITE] must have been zeroed on the stream.
void launch_map_extend(hipStream_t s, const MapUpdateDev& u);
// out[i][j] = cov[rows(i)][rows(j)], out_mean[i] = mean[rows(i)] for the k objects idx of a map of ldc rows: a copy, nothing is symmetrised
void launch_map_select(hipStream_t s, const uint32_t* idx, int32_t k, int32_t od, const double* mean, const double* cov, int64_t ldc, double* out_mean, double* out_cov);
// Duplicate objects of a map merged (include/obvi_map_merge.h; map_kernels.hip): pair r says x[drop_r] - x[keep_r] = d_r (+ noise R_r).  With H the Q = q od
// constraint rows (+I at drop, -I at keep), G = Cs H^T, T = H G + R = L L^T, W = L^-1, Y = G W^T:  C' = Cs - Y Y^T, mu' = mu - Y W (H mu - d), on the NK rows
// of the objects `kept` (those not dropped, in their old order).  T is built in a one-group cut of Q rows (cut.A, cut.Csym; cut.mean gets H mu - d; the cut's
// map_idx is the drop list), factored and tested as any cut; G and Y are [nK][nQ] tiles of kept rows only, Wn [nQ][nQ]: W as tiles.
struct MapMergeDev {
  int32_t od, N, Q, NK, nQ, nK;                              // map rows, constraint rows, kept rows; the latter two in tiles of 64
  MapCutDev cut;                                             // the one-group cut that holds T and its factor
  const uint32_t* keep; const uint32_t* kept;                // [Q / od] the pairs' survivors; [NK / od] the objects of the new map
  const double* offset; const double* noise;                 // [Q] d (never NULL: zeros); [Q / od][od][od] as given (not symmetrised), NULL: exact
  const double* map_mean; const double* map_cov;             // the old map: [N], [N][N]
  double* Wn; double* G; double* Y; double* v;               // tiles; v [64 nQ] = W (H mu - d)
  double* out_mean; double* out_cov;                         // the new map: [NK], [NK][NK]; a non-finite entry sets MS_NONFINITE of the cut's record
};
// T and H mu - d into the cut, its factor and condition estimate (x0: the map's start vector), G, Wn, Y, then the downdate path of MapUpdateDev through the
// row table `kept` with Z = Y: C', v, mu'.  The cut's W, the padding of its Lambda and its status record must have been zeroed on the stream.
void launch_map_merge(hipStream_t s, const MapMergeDev& g, const double* x0);
// Duplicate objects of a map proposed (include/obvi_map_match.h; map_kernels.hip): every pair a < b of the n objects that passes the label and centre-distance
// tests gets s = d^T T^-1 d on the rows of `mask`, d = mu_b - mu_a (row 3 wrapped by `period`), T = Cs_bb - Cs_ba - Cs_ab + Cs_aa.  stat [n][n], upper
// triangle: s, or kMatchNotTested / kMatchSingular.  The pairs with s <= gate leave in (a, b) order, cut at `capacity`.
constexpr double kMatchNotTested = -1.0, kMatchSingular = -2.0;
struct MapMatchDev {
  int32_t od, n; uint32_t mask; int32_t use_dist;            // mask: never 0 (all rows: every bit below od); use_dist 0: no centre test
  double gate, dist2, period;                                // dist2 = D D; period 0: no wrap
  int64_t capacity;
  const double* map_mean; const double* map_cov;             // the map: [n od], [n od][n od]
  const int32_t* label;                                      // [n] or NULL
  double* diag; double* mean;                                // [n][od][od] the symmetrised diagonal blocks, [n][od] the means beside them
  double* stat;                                              // [n][n]
  int64_t* row_cnt; int64_t* row_off; int64_t* totals;       // [n][3] found, tested, singular of row a; [n] found in the rows before a; [3] the sums
  uint32_t* out_a; uint32_t* out_b; double* out_stat; double* out_yaw;   // [min(capacity, n (n - 1) / 2)] each (never read when capacity is 0)
};
// five launches: diagonal blocks, pairs, row counts, the scan of the rows (one workgroup), the scatter.  n >= 1.
void launch_map_match(hipStream_t s, const MapMatchDev& m);
// A map moved into another frame under an uncertain transform (include/obvi_map_frame.h; map_kernels.hip): x'_o = g(T, x_o) object by object,
// C' = Jt Cs Jt^T + G Sigma_s G^T with Jt = blockdiag(J_o), J_o = blockdiag(Jk_o, I3), and G the stacked G_o, whose last three rows are zero.  K = od - 3 rows
// of a block move (centre and rotation), dT = 4 (od 7: tx ty tz psi) or 6 (od 9: translation, axis-angle) parameters has the transform.
constexpr int kFrameMaxDT = 6;
struct MapFrameDev {
  int32_t od, n, has_sigma;                                  // has_sigma 0: the transform is exact, G and GS are never read
  double transform[kFrameMaxDT];                             // [dT]
  double sigma[kFrameMaxDT * kFrameMaxDT];                   // [dT][dT] Sigma_s, symmetrised by the host
  const double* map_mean; const double* map_cov;             // the old map: [n od], [n od][n od]
  double* J; double* G; double* GS;                          // [n][K][K] Jk_o, [n][K][dT] the moving rows of G_o, [n][K][dT] G_o Sigma_s
  double* out_mean; double* out_cov;                         // the new map
  double* status;                                            // MS_NONFINITE is set to 1 by whoever writes a non-finite entry of the new map; zeroed on the stream before
};
// two launches: the objects (means, Jk, G, GS: one lane each), then the covariance over object-aligned block pairs.  n >= 1.
void launch_map_transform(hipStream_t s, const MapFrameDev& f);
// out = (mean_a, mean_b), blockdiag(cov_a, cov_b), copied entry by entry: one launch.  The two maps may be the same one.
void launch_map_join(hipStream_t s, int64_t rows_a, const double* mean_a, const double* cov_a, int64_t rows_b, const double* mean_b, const double* cov_b, double* out_mean, double* out_cov);
// One map located in another from the constellations of their object centres (include/obvi_map_locate.h; map_kernels.hip).  rec: [na + nb][12] -- centre,
// the lower triangle of the symmetrised centre block (00 10 11 20 21 22), three unused -- A's objects first; lab beside it.  Rows of the seed count are
// (a1, a2) over the whole na x na square (a1 >= a2: empty), so that the scan's order is the seeds' lexicographic one.
constexpr int kLocateRec = 12, kLocateMaxObjects = 819;
constexpr int64_t kLocateMaxSeeds = 1 << 20;
struct MapLocateDev {
  int32_t od, na, nb, min_inliers, iterations, has_label_a, has_label_b;
  double dmin, tol, gate;
  int64_t seed_cap;                                          // room of seeds / inl / cost: min(all seeds, kLocateMaxSeeds); more compatible seeds: nothing behind the scan runs
  int64_t found, out;                                        // second half only: the hypotheses with >= min_inliers, and how many of them are reported
  const double* mean_a; const double* cov_a; const double* mean_b; const double* cov_b;
  const int32_t* label_a; const int32_t* label_b;            // [na], [nb]; read only with has_label_*
  double* rec; int32_t* lab;                                 // [na + nb][12], [na + nb]
  int64_t* row_cnt; int64_t* row_off; int64_t* totals;       // [na na][2] tested, compatible; [na na] compatible in the rows before; [3] the counts of the header
  uint32_t* seeds; int32_t* inl; double* cost;               // [seed_cap][4], [seed_cap], [seed_cap]
  int64_t* blk_cnt; int64_t* blk_off;                        // per 256 hypotheses: those with >= min_inliers, and those in the blocks before
  uint32_t* qlist; uint32_t* sel;                            // [found] their hypothesis numbers in ascending order; [out] the reported ones by rank
  uint32_t* out_seed; double* out_T; double* out_cov; int32_t* out_inl; double* out_cost; int32_t* out_partner;   // [out] x 4, 4, 16, 1, 1, nb
};
// first half, up to the counts: stage, count, scan, scatter, score, count and scan of the hypotheses that qualify.  na, nb >= 2.
void launch_map_locate_score(hipStream_t s, const MapLocateDev& m);
// second half, found >= out >= 1 known: the qualifying hypotheses compacted, ranked, and the first `out` refined
void launch_map_locate_report(hipStream_t s, const MapLocateDev& m);
// the posterior of the handle form: the k x k blocks of launch_cov_pairs (pair a k + b: objects a, b) -> dense P, and the objects' current values -> pm
void launch_map_posterior_layout(hipStream_t s, const double* blocks, const double* objects, const uint32_t* obj_idx, int32_t k, int32_t od, double* P, double* pm);

struct ReducedDev {         // accumulators of the reduced system
  double* Hdiag;            // pose v: 36 doubles at 36 v; object w: od^2 doubles at 36 nPv + od^2 w (row-major, lower part used)
  double* g;                // [6 nPv + od nOv] gradient J^T r (compact index: pose v at 6v, object w at 6 nPv + od w)
  double* scale;            // same index: Jacobi scaling (fixed at iteration 0)
  double* lam;              // same index: LM damping of the unscaled normal equations
  double* S;                // tile grid
  double* rhs;              // [m_pad] right-hand side -> forward-substituted z
  double* y;                // [m_pad] solution
  int32_t nt;               // tiles per dimension
  const double* extra;      // NULL, or (same compact index as g) an addition to the diagonal of the normal equations: parameter priors of the covariance extraction
};

struct PointDev {           // per eliminated point
  double* Ci;               // [L][6]  inverse Cholesky factor of (Hll + lambda), lower-tri packed (00,10,11,20,21,22)
  double* u;                // [L][3]  Ci * g_l
  double* gl;               // [L][3]  g_l = sum rho' Jl^T r
  double* lam;              // [L][3]  LM damping of the point block (unscaled normal equations)
  double* scale;            // [L][3]  Jacobi scaling
  double* Z;                // [N_r][18] 6x3 row-major:  rho' Jp^T Jl Ci^T
  const double* extra;      // NULL, or [L][3] addition to the diagonal of H_ll (parameter priors of the covariance extraction)
};

// ---- launchers (ba_kernels.hip) --------------------------------------------------------
// obvi_ba_set_reproj: the arrays only the device reads (camera, pixel, sigma), in both observation orders (by point: a -> perm[a]; by pose:
// k -> perm[rq_src[k]]), gathered from the caller's order on the device; raw_cam / raw_sigma may be null (camera 0 / one sigma for all)
void launch_reproj_gather(hipStream_t s, int64_t n, const uint32_t* perm, const uint32_t* rq_src, const uint32_t* rp_point, const uint16_t* raw_cam,
                          const double2* raw_pixel, const double* raw_sigma, double sigma_scalar, uint16_t* cam, double2* pixel, double* sigma,
                          uint32_t* q_point, uint16_t* q_cam, double2* q_pixel, double* q_sigma, uint8_t* q_active);
void launch_pose_cache(hipStream_t s, int64_t P, const double* poses, PoseCache* out, int analytic /* obvi_ba_options.reprojection_variant == OBVI_REPROJECTION_ANALYTIC */);
void launch_point_pass(hipStream_t s, const BlocksDev& b, const ReprojDev& rp, const DevCam* cams, const PoseCache* pc, const double* points,
                       const ReducedDev& rd, const PointDev& pt, double radius, int first_iter, double* scal, const uint32_t* wave_obs, int64_t n_waves,
                       const uint32_t* long_points, int64_t n_long, bool flat /* Knobs::point_flat: k_point_pass requests its loads in front of the `live` branch and of the scan */);
// lin: NULL, or (unsliced pose pass only) 27 doubles per pose that take the sums instead of Hdiag / g; launch_pose_lin_add adds such a set
void launch_pose_pass(hipStream_t s, const BlocksDev& b, const ReprojPoseDev& rq, const DevCam* cams, const PoseCache* pc,
                      const double* points, const ReducedDev& rd, double* lin = nullptr);
void launch_pose_lin_add(hipStream_t s, const BlocksDev& b, const double* lin, const ReducedDev& rd);
void launch_small_factors(hipStream_t s, const BlocksDev& b, const SmallFactorsDev& sf, const DevCam* cams,
                          const double* poses, const double* objects, const ReducedDev& rd, double* scal, int64_t lanes_below /* Knobs::small_lanes_below */,
                          bool packed /* Knobs::side_packed */);
void launch_reduced_diag(hipStream_t s, const BlocksDev& b, const double* poses, const double* objects,
                         const ReducedDev& rd, double radius, int first_iter, double* scal);
// map group priors; every launcher returns at once when there are no groups.  Linearisation: y = Lambda d and the slabs' partial sums (launch_map_group_quad,
// mode 0: groups with a variable member, mode 1: groups whose members are all constant), then w Lambda into Hdiag / S, w y into g, rho / 2 into SC_COST
// (launch_map_group_scatter: behind the small-factor gathers and in front of launch_reduced_diag, on their stream).  launch_map_group_cost: the quad kernel on
// `objects` and rho / 2 into SC_COST_CAND (mode 0) or SC_COST_FIXED (mode 1).
void launch_map_group_quad(hipStream_t s, const BlocksDev& b, const MapGroupDev& mg, const double* objects, int mode);
void launch_map_group_scatter(hipStream_t s, const BlocksDev& b, const MapGroupDev& mg, const ReducedDev& rd, double* scal);
void launch_map_group_cost(hipStream_t s, const BlocksDev& b, const MapGroupDev& mg, const double* objects, int mode, double* scal);
// r = W d of every group into `residuals` (scaled by sqrt(rho') with apply_loss; zeros for an inactive group), |r|^2 per group into `sqnorm`, the cost into SC_COST
void launch_map_group_eval(hipStream_t s, const BlocksDev& b, const MapGroupDev& mg, const double* objects, int apply_loss, double* residuals, double* sqnorm, double* scal);
// obvi_ba_debug_linearize: the raw r = W d of every group, inactive ones too; no cost, no norms
void launch_map_group_debug(hipStream_t s, const MapGroupDev& mg, const double* objects, double* residuals);
void launch_schur_blocks(hipStream_t s, int64_t nblk, const uint32_t* blk_row, const uint32_t* blk_col, const uint32_t* blk_ptr,
                         const uint32_t* pair_a, const uint32_t* pair_b, const uint32_t* obs_point, const PointDev& pt,
                         const ReducedDev& rd);
// strip geometry of k_schur_window, shared with the host code that builds the visit lists and decides which pairs
// the strip covers: row chunks of kSchurRows frames, columns = the kSchurWindowFrames frames ending with the chunk, cut
// into groups of Geom::kGroupCols 16-wide tile columns; visits are streamed through LDS in batches of at most
// kSchurBatchVisits visits / Geom::kBatchBytes of 144-byte slots
constexpr int kSchurRows = 8, kSchurWindowFrames = 40, kSchurBatchVisits = 128;
// The two strip geometries (the plan is built for one of them and the handle remembers which: obvi_ba_handle::schur_narrow).  Wide: a wavefront's accumulator is
// 3 x 5 tiles (120 registers), two wavefronts per SIMD; every deterministic handle, whose sums are partitioned by the (chunk, group) lists.  Narrow: 3 x 3 tiles
// (72 registers) and 24 KB batches, three wavefronts per SIMD and three workgroups per CU.  The chunk's own frames (8 frames = 3 tile columns) are the last group
// of either.  kVisitGroup: visits a wavefront takes together (all their LDS reads, then all their products).
struct SchurWide { static constexpr int kGroupCols = 5, kBatchBytes = 32768, kVisitGroup = 2; };
struct SchurNarrow { static constexpr int kGroupCols = 3, kBatchBytes = 24576, kVisitGroup = 2; };
// the slot tables of the strip kernel, filled on the device (plan_kernels.hip): per visit the point, its tile bits of the (chunk, group) work list
// (bit 15: two records per frame), the slot its image starts at inside its batch and the offset of its slots from the first slot of its workgroup
struct PlanVisit { uint32_t l; uint16_t twin_bits; uint16_t base; uint32_t rel; };
void launch_plan_visit_slots(hipStream_t s, bool narrow, int64_t nvis, const PlanVisit* pv, const uint32_t* wg_ptr, const uint32_t* wg_slot0, int32_t nwg, const int32_t* wg_f0, const int32_t* wg_group,
                             const uint32_t* point_ptr, const uint8_t* rp_active, const uint32_t* rp_pose, const int32_t* frame_of_pose, uint32_t zero16, uint32_t* visits, uint32_t* slot_src);
void launch_schur_window(hipStream_t s, bool narrow, int64_t nwg, int has_twins, const BlocksDev& b, const PointDev& pt, const ReducedDev& rd, const int32_t* row_of_nat,
                         const uint32_t* wg_bptr, const uint32_t* bfirst, const uint32_t* bslot, const uint32_t* visits, const uint32_t* slot_src,
                         const int32_t* wg_f0, const int32_t* wg_group);
// point back-substitution and the candidate poses / objects (with the candidate's pose cache, both layouts of launch_pose_cache), one launch
void launch_backsub_apply(hipStream_t s, const BlocksDev& b, const ReprojDev& rp, const PointDev& pt, const ReducedDev& rd, const double* points,
                          double* points_cand, const double* poses, const double* objects, double* poses_cand, double* objects_cand, PoseCache* pc_cand, double* scal,
                          int lanes /* Knobs::backsub_lanes; 0: by sightings per feature */);
// trial-point cost + model cost change.  mode 0: cost at (poses,points,objects) into SC_COST_CAND and
// model change of the step (cand - current); mode 1: cost only, split into SC_COST / SC_COST_FIXED.
void launch_cost(hipStream_t s, const BlocksDev& b, const ReprojPoseDev& rq, const SmallFactorsDev& sf, const DevCam* cams,
                 const PoseCache* pc_cur, const double* poses_cur, const double* points_cur, const double* objects_cur,
                 const PoseCache* pc_cand, const double* poses_cand, const double* points_cand, const double* objects_cand,
                 int mode, double* scal, double* lin = nullptr /* mode 0, unsliced pose pass: the pose-side sums at the candidate, 27 per pose */);
// problem->Evaluate: raw / robustified residuals of every factor in caller order, family after family as `lay` places them (the map group priors: launch_map_group_eval)
void launch_evaluate(hipStream_t s, const BlocksDev& b, const ReprojDev& rp, const uint32_t* rp_perm, const SmallFactorsDev& sf,
                     const DevCam* cams, const PoseCache* pc, const double* poses, const double* points, const double* objects,
                     int apply_loss, const EvalLayout& lay, double* residuals, double* sqnorm, double* scal);
void launch_debug_linearize_reproj(hipStream_t s, const ReprojDev& rp, const uint32_t* rp_perm, const DevCam* cams,
                                   const PoseCache* pc, const double* points, double* r, double* J0, double* J1);
void launch_debug_linearize_small(hipStream_t s, int factor_type, const SmallFactorsDev& sf, const DevCam* cams,
                                  const double* poses, const double* objects, double* r, double* J0, double* J1);
void launch_fill(hipStream_t s, double* p, int64_t n, double v);
// dst row i = src row map[i], rows of three doubles (features between the caller's numbering and the internal one)
void launch_permute_rows3(hipStream_t s, double* dst, const double* src, const uint32_t* map, int64_t n);
// multi-GPU exchange buffers: shared objects' (Hdiag 49 | g 7) and the trailing tiles [t0, nt) + rhs rows
void launch_pack_shared_blocks(hipStream_t s, const BlocksDev& b, const ReducedDev& rd, const int32_t* shared_ov, int32_t n_shared, double* buf, int unpack);
void launch_pack_tail(hipStream_t s, const ReducedDev& rd, int32_t t0, double* buf, int unpack);
// scalar sums [SC_COST, SC_SUM_END) + one gradient-maximum slot per rank: (SC_SUM_END - SC_COST) + world doubles, one all-reduce (sum)
void launch_pack_scalars(hipStream_t s, double* scal, double* buf, int32_t rank, int32_t world, int unpack);

// ---- outlier selection (select_kernels.hip) ---------------------------------------------
struct SelectScratch {
  void *tbl = nullptr, *aux = nullptr;   // hash table (keys, then representatives); histograms, counters, result, carry between rounds, candidates
  size_t tbl_slots = 0;
};
// launches only; *result_dev -> {number excluded, r} on the device: r = 0 finished, r > 0: call again with round = r (more than 4096 distinct values in the last bin; r <= 2)
hipError_t select_by_threshold(hipStream_t s, int64_t n, const double* sq, const uint8_t* active, const uint32_t* inv, double fraction,
                               uint8_t* mask_out, SelectScratch* scratch, const int** result_dev, int round = 0);
void select_scratch_free(SelectScratch* sc);

// ---- tile Cholesky (chol_kernels.hip) --------------------------------------------------
// Symbolic factorisation at tile granularity, level-scheduled: tile columns in one level of the
// tile elimination tree do not depend on each other and are processed by the same launches.
// *_ptr arrays indexed by level live on the host (they size the launches); the rest is on the device.
struct CholPlan {
  int32_t nt;
  int32_t nlevels;
  int32_t deterministic;      // column-oriented backward substitution without atomics (one launch per level)
  int32_t fused_potrf;        // 1: k_update_potrf (a level's updates + the next level's potrf in one grid, potrf workgroups wait for their jobs); 0: two launches
  const int32_t* lvl_k_ptr;   // host [nlevels+1]   tile columns of each level
  const int32_t* lvl_k;       // device
  const int32_t* trsm_ptr;    // host [nlevels+1]   trsm jobs (i,k), k in the level
  const int32_t* trsm_ik;     // device, 2 per job
  const int32_t* upd_ptr;     // host [nlevels+1]   update jobs: one per target tile (i,j) and level
  const int32_t* upd_ij;      // device, 2 per job
  const int32_t* upd_kptr;    // device [jobs+1]    the level's columns k contributing to the target
  const int32_t* upd_k;       // device
  const uint8_t* upd_flag;    // device [jobs]      1: the target's k-list is split over several jobs -> atomic accumulation
  const int32_t* rh_ptr;      // host [nlevels+1]   right-hand-side jobs: one per target tile row i and level
  const int32_t* rh_i;        // device
  const int32_t* rh_kptr;     // device [jobs+1]
  const int32_t* rh_k;        // device
  const int32_t* job_signal;  // device [update jobs + rhs jobs, per level: updates then rhs]  tile column of the next level whose potrf waits for the job, or -1
  const int32_t* k_need;      // device, parallel to lvl_k: number of jobs of the previous level that column's potrf waits for
  const int32_t* pre_ptr;     // device, parallel to lvl_k (+1): tile columns j of the previous level whose product L_kj L_kj^T (and L_kj z_j)
  const int32_t* pre_j;       // device                  the column's potrf workgroup applies itself (no job, no wait)
  int32_t* diag_done;         // device [nt] counters
  const int32_t* crit_upd;    // host [nlevels]     number of signalling update / right-hand-side jobs of the level (first in their lists)
  const int32_t* crit_rh;     // host [nlevels]
  const int32_t* slices;      // host [nlevels]     1, or 4 on thin levels (update / trsm tile products split into four row slices)
  const int32_t* col_ptr;     // device [nt+1]      column structure of L: rows i > k with L(i,k) != 0
  const int32_t* col_i;       // device
  int32_t nbw;                // launches of the backward substitution (several levels each)
  const int32_t* bw_ptr;      // host [nbw+1]       backward substitution workgroups of each launch, in the order of the forward levels
  const int32_t* bw_kj;       // device, 3 per workgroup: tile (k,j) of row k, j < k (j = -1: the workgroup that stores y_k), offset of row k's chain record
  const int32_t* bw_chains;   // device             chain records: n, the n ancestors of the row inside the launch (top first), 2 words of tile presence bits
  const int32_t* row_ptr;     // device [nt+1]      row structure of L: columns j < k with L(k,j) != 0 (forward substitution with many right-hand sides)
  const int32_t* row_j;       // device
};
void launch_copy3(hipStream_t s, double* d0, const double* s0, int64_t n0, double* d1, const double* s1, int64_t n1, double* d2, const double* s2, int64_t n2);
// small accumulators cleared at the start of an LM step, together with the tiles (one launch)
struct StepClear {
  double* hdiag; int64_t n_hdiag;
  double* g; int64_t n_g;
  double* rhs; int64_t n_rhs;
  int32_t* diag_done; int64_t n_done;   // potrf counters of k_update_potrf
  double* scal; int64_t n_scal;         // scalar block; scal[fixed_slot] = fixed_cost
  int64_t fixed_slot; double fixed_cost;
  int64_t n_max;
  double* pub_host; double pub_seq;      // not null: the workgroup that clears the scalar block first writes it to this pinned page, then pub_seq behind it (the LM loop's read-back)
};
void launch_zero_tiles(hipStream_t s, double* S, int32_t nt, const int32_t* tile_list, int32_t ntiles, const uint8_t* is_pad_row, const StepClear& c);
// optional per-kernel timing (profiling level 2): an event is recorded after every launch, tagged with the kernel class
enum CholKernel { CK_POTRF = 0, CK_TRSM, CK_UPDATE, CK_BACKWARD, CK_COUNT };
struct CholTimers {
  std::vector<hipEvent_t>* pool;   // grown on demand
  std::vector<int>* tags;          // tag of the kernel that ENDS at event i (event 0 = start, tag -1)
  int used;
};
void launch_cholesky_factor(hipStream_t s, const CholPlan& plan, int level0, int level1, double* S, double* Linv, double* rhs, double* scal, CholTimers* timers = nullptr);
void launch_cholesky_backward(hipStream_t s, const CholPlan& plan, const double* S, const double* Linv, double* rhs /* z in, overwritten */, double* y, CholTimers* timers = nullptr);

// covariance blocks: Y = L^-1 E for the unit vectors of every variable object's rows, kept transposed (Yt row-major
// [64 nslabs][ldt = 64 nt], cleared by the caller), then od x od blocks Yt[ca..] Yt[cb..]^T for pairs of row offsets (cols: 2 per
// pair, negative: zero block)
void launch_forward_multi(hipStream_t s, const CholPlan& plan, const double* S, const double* Linv, double* Yt, int64_t ldt, int nslabs,
                          const int32_t* slab_first, const int32_t* obj_row, int32_t nOv, const int32_t* row_split /* host [nlevels]: workgroups per row, or null */, int od = 7);
void launch_cov_pairs(hipStream_t s, const double* Yt, int64_t ldt, int64_t n_pairs, const int32_t* cols, const int32_t* first_row, double* out, int od = 7);


// ---- selected inversion (cov_kernels.hip; include/obvi_cov.h) ---------------------------
// Sigma = (L L^T)^-1 on the tile pattern of L, in place over the factor the LM step left in S (diagonal tiles: both triangles).  Ys: scratch for the
// Y tiles of one level (the largest level's off-diagonal tile count); ybase[k]: first scratch tile of column k inside its level.
void launch_selected_inverse(hipStream_t s, const CholPlan& plan, double* S, const double* Linv, double* Ys, const int32_t* ybase);
// blocks of Sigma by rows of the tile grid: desc = (first row, first column, rows, columns) per item, a negative row: zero block; item b goes to out + off[b]
void launch_cov_gather(hipStream_t s, const double* S, int32_t nt, int64_t n, const int32_t* desc, const int64_t* off, double* out);
// 3x3 feature blocks from Sigma and the point pass's records (Z, Ci): idx = internal feature index per item, negative: zero block; out [n][9]
void launch_cov_points(hipStream_t s, const double* S, int32_t nt, int64_t n, const int64_t* idx, const uint32_t* point_ptr, const int32_t* yrow, const uint8_t* point_var,
                       const double* Z, const double* Ci, double* out);

// declared pairs off the pattern (obvi_cov_compute_pairs), between the factorisation and the selected inversion: Yt [64 nslabs][ldt = 64 nt] = (L^-1 E)^T for
// the unit vectors of the rows rhs_row[0 .. nrhs) (ascending; cleared and seeded here), slab_first[sl] = tile row of the slab's first right-hand side
void launch_cov_forward(hipStream_t s, const CholPlan& plan, const double* S, const double* Linv, double* Yt, int64_t ldt, int nslabs, const int32_t* slab_first,
                        const int32_t* rhs_row, int32_t nrhs);
// blocks Yt[ca .. ca + da)  Yt[cb .. cb + db)^T over the columns from first[p] on -> out + off[p], da x db row-major; (da, db) one of (6, 6), (6, od), (od, od)
void launch_cov_rhs_pairs(hipStream_t s, const double* Yt, int64_t ldt, int64_t n_pairs, int da, int db, const int32_t* cols, const int32_t* first, const int64_t* off, double* out);
// Blocks with a feature.  Request g = (internal feature l, x, dx, -): dx > 0: x = first row of a reduced block of dx rows, the 3 x dx block (l, x); dx = 0: x = internal
// feature m != l, the 3 x 3 block (l, m).  ops[op_ptr[g] + e]: where Sigma_{p(a), x} (e = observation a of l) or Sigma_{p(a) p(b)} (e = a * |obs(m)| + b) comes from:
// -1 the tiles of Sigma, else offset << 1 | transposed into `side`.  Block g -> side + out_off[g].
void launch_cov_point_cross(hipStream_t s, const double* S, int32_t nt, int64_t n, const int32_t* req, const int64_t* op_ptr, const int64_t* ops, const int64_t* out_off,
                            const uint32_t* point_ptr, const int32_t* yrow, const double* Z, const double* Ci, double* side);

}  // namespace obvi
#endif  // OBVI_BA_DEVICE_H_
