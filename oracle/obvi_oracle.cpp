// obvi_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
//
// CPU oracle for the bundle-adjustment hot path: the same flat problem the C ABI in
// include/obvi_ba.h accepts, evaluated and solved on the host in scalar fp64.  Exposed as
// `oracle_*` functions with the signatures of their `obvi_ba_*` counterparts so parity tests
// feed both the same arrays.  Only tests/, __graft_entry__.smoke() and bench.py's
// cpu_baseline leg may load this library; the product (obvi-slam_amd/) never does.
//
// What it restates, and from where (all paths under /root/reference):
//   factors          -> oracle_factors.h (cites each functor)
//   evaluate         -> problem->Evaluate(apply_loss_function=false|true)
//                       include/refactoring/optimization/object_pose_graph_optimizer.h:682-693
//   solve            -> ceres::Solve with the option block at object_pose_graph_optimizer.h:651-676
//                       (SPARSE_SCHUR, HuberLoss, Levenberg-Marquardt, Jacobi scaling,
//                       non-monotonic steps).  Ceres itself is an un-vendored, un-pinned
//                       dependency (CMakeLists.txt:41-44 "Recommended to use Ceres 1.14"); the
//                       trust-region loop below restates its published algorithm
//                       (trust_region_minimizer.cc / levenberg_marquardt_strategy.cc /
//                       trust_region_step_evaluator.cc / schur_complement_solver.cc of Ceres
//                       1.14-2.x) and is marked [Ceres-doc] where it does.
//   select_outliers  -> include/refactoring/offline/offline_problem_runner.h:769-800
//   shared objects   -> no reference counterpart (the reference is one process): the exchange protocol of include/obvi_ba.h
//                       ("multi-GPU") on host buffers, so that the N > 1 path has a CPU stand-in that is held against this
//                       oracle's own solve of the joint problem (tests/test_distributed_gloo.py, world size 2 over gloo)
//
// PARITY STATUS: factor arithmetic is pinned by the two golden tuples the survey derived from
// the reference's own code (tests/golden/reference_tuples.json), the reference's simulated data
// sets (zero residual at their ground truth, tests/golden/vslam_set*.npz) plus independent numpy
// fixtures; the solver level is "parity unpinned" -- the reference holds no test or vector
// for any residual, Jacobian, cost or solve and Ceres is not installed.
#include "../include/obvi_ba.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../include/obvi_frontend.h"
#include "oracle_factors.h"
#include "oracle_frontend.h"

#ifdef OBVI_ORACLE_FACTORS_EXTENDED
// The arbiter build evaluates the FACTORS in extended precision too: the same header once more with every `double` an x87 long double
// (namespace oracle_x; every standard header it needs is already included above, so the macro touches nothing else).  Residuals and
// Jacobians are then exact to ~1e-19 for the fp64 parameter blocks and measurements they are given -- without this the arbiter would share
// the fp64 checker's own rounded factor records and count every last-digit difference of another evaluation order (the HIP kernels' closed
// forms) as that side's error, amplified by the cancellation in the reduced gradient.
#define oracle oracle_x
#define double long double
#undef OBVI_ORACLE_FACTORS_H_
#include "oracle_factors.h"
#undef double
#undef oracle
// the substitution really took effect: a factor-level type of the second inclusion carries long double members (a silent miss would give a
// "arbiter" that shares the checker's fp64 factor records)
static_assert(sizeof(oracle_x::CameraConst{}.fx) == sizeof(long double) && sizeof(oracle::CameraConst{}.fx) == sizeof(double) && sizeof(long double) > sizeof(double),
              "arbiter build: oracle_factors.h was not re-instantiated in extended precision");
#endif

namespace {
using namespace oracle;  // NOLINT

// Scalar of the solver-level sums: every accumulation of the normal equations (J^T J blocks, gradient, column norms), the Schur
// complement, the skyline factorisation, both substitutions, the model cost change and the cost sums.  `double` in libobvi_oracle.so --
// the checker.  Compiled a second time with -DOBVI_ORACLE_REAL="long double" -DOBVI_ORACLE_FACTORS_EXTENDED (libobvi_oracle_ld.so,
// `make arbiter`) the same code is the ARBITER of DESIGN.md section 6: the parameter blocks and the caller's measurements stay fp64 --
// identical inputs -- while the factor records AND everything that is summed from them carry 64 mantissa bits, so its round-off sits three
// decimal digits below both the checker's and the HIP path's; |HIP - arbiter| against |oracle - arbiter| then says which of the two
// fp64 runs is closer to the exact-arithmetic step.
#ifndef OBVI_ORACLE_REAL
#define OBVI_ORACLE_REAL double
#endif
typedef OBVI_ORACLE_REAL real;
// scalar of the factor records (residuals, Jacobians, measurement constants): fp64 in the checker, `real` in the arbiter build
#ifdef OBVI_ORACLE_FACTORS_EXTENDED
typedef real fscalar;
namespace fx = oracle_x;
#else
typedef double fscalar;
namespace fx = oracle;
#endif

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Host threads for the embarrassingly parallel parts (linearisation of the factors, trial-point cost, elimination of the points):
// bench.py's cpu_baseline leg sets min(20, hardware threads) -- 20 is the reference's own num_threads
// (object_pose_graph_optimizer.h:662) -- through oracle_set_threads().  The default, and what every parity test runs, is 1: the
// sequential code below.  With more threads every sum still adds the same terms in the same order (round 6: the points'
// Schur contributions are added row by row by one thread each, the trial cost is one running sum over per-factor values), so
// the oracle's results are bit-identical for any thread count (tests/test_oracle_solver.py).
int g_threads = 1;
template <class F>
void parallel_ranges(int64_t n, F&& fn) {   // fn(thread, begin, end), contiguous ranges in order
  const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(g_threads, n));
  if (parts == 1) { fn(0, (int64_t)0, n); return; }
  std::vector<std::thread> th;
  for (int t = 0; t < parts; ++t) th.emplace_back([&fn, n, parts, t]() { fn(t, n * t / parts, n * (t + 1) / parts); });
  for (auto& x : th) x.join();
}

struct OracleProblem {
  int reproj_variant = 0;   // obvi_ba_options.reprojection_variant: 0 = a3 (production functor), 1 = a2 (analytic-Jacobian functor)
  int od = 7;               // obvi_ba_options.object_block_size: parameters of an ellipsoid block, 7 (x y z yaw dx dy dz) or 9 (x y z ax ay az dx dy dz)
  std::vector<CameraConst> cams;       // fp64 (index checks, and the camera constants of the checker)
  std::vector<fx::CameraConst> cams_f; // the factors' camera constants
  int64_t P = 0, L = 0, O = 0;
  std::vector<double> poses, points, objects;
  std::vector<uint8_t> pose_const, point_const, object_const;
  // reprojection
  int64_t n_rp = 0;
  std::vector<uint32_t> rp_pose, rp_point; std::vector<uint16_t> rp_cam;
  std::vector<fscalar> rp_pixel, rp_sigma; double rp_huber = 1.0; std::vector<uint8_t> rp_active;
  // bbox
  int64_t n_bb = 0;
  std::vector<uint32_t> bb_obj, bb_pose; std::vector<uint16_t> bb_cam;
  std::vector<fscalar> bb_rect, bb_sqrt_inf; double bb_huber = 1.0, bb_invalid = 1e6; std::vector<uint8_t> bb_active;
  // shape prior
  int64_t n_sp = 0;
  std::vector<uint32_t> sp_obj; std::vector<fscalar> sp_mean, sp_sqrt_inf; double sp_huber = 1.0; std::vector<uint8_t> sp_active;
  // ltm prior
  int64_t n_lt = 0;
  std::vector<uint32_t> lt_obj; std::vector<fscalar> lt_mean, lt_sqrt_inf; double lt_huber = 1.0; std::vector<uint8_t> lt_active;
  // relative pose
  int64_t n_rl = 0;
  std::vector<uint32_t> rl_a, rl_b; std::vector<fscalar> rl_t, rl_R, rl_sqrt_inf; double rl_huber = 1.0; std::vector<uint8_t> rl_active;
  // parameter priors (parameter_prior.h:17-50), used by the covariance extraction only: kind 0 pose / 1 point / 2 object
  std::vector<uint8_t> pp_kind, pp_param; std::vector<uint32_t> pp_block; std::vector<double> pp_mean, pp_std;
  // snapshot
  std::vector<double> snap_poses, snap_points, snap_objects;
  // objects shared with other ranks (obvi_ba_set_shared_objects / obvi_ba_set_allreduce): the solve then runs the exchange protocol of
  // include/obvi_ba.h on host buffers
  std::vector<uint8_t> is_shared; int32_t rank = 0, world = 1;
  obvi_allreduce_fn allreduce = nullptr; void* allreduce_user = nullptr;
  // last solve
  std::vector<obvi_iteration_summary> iterations;
  // test hook (oracle_ba_debug_keep_visited): poses then points of every candidate the last solve evaluated, accepted or not
  bool keep_visited = false;
  std::vector<std::vector<double>> visited;
  std::string err;
};

// ---------------------------------------------------------------------------------------
// linearised factor record: robustified residual and Jacobians w.r.t. up to two blocks
// ---------------------------------------------------------------------------------------
enum BlockKind { KIND_POSE = 0, KIND_POINT = 1, KIND_OBJECT = 2, KIND_NONE = 3 };

struct FactorLin {
  int m = 0;                 // residual dim
  BlockKind k0 = KIND_NONE, k1 = KIND_NONE;
  int64_t i0 = -1, i1 = -1;  // block indices
  int d0 = 0, d1 = 0;        // their sizes
  fscalar r[9];
  fscalar J0[81];            // m x d0, row-major
  fscalar J1[36];            // m x d1
  fscalar cost = 0.0;        // 0.5 * rho(s)
  fscalar sqnorm = 0.0;      // un-robustified |r|^2
};

// Apply the loss the way ceres::ResidualBlock::Evaluate + Corrector do [Ceres-doc]: for
// HuberLoss rho'' <= 0 always, so the corrector reduces to scaling r and J by sqrt(rho').
void robustify(FactorLin* f, double huber_a, bool apply_loss) {
  fscalar s = 0.0;
  for (int i = 0; i < f->m; ++i) s += f->r[i] * f->r[i];
  f->sqnorm = s;
  if (!apply_loss) { f->cost = (fscalar)0.5 * s; return; }
  fscalar rho[3];
  fx::huber(s, huber_a, rho);
  f->cost = (fscalar)0.5 * rho[0];
  const fscalar w = std::sqrt(rho[1]);
  if (w != (fscalar)1.0) {
    const int d0 = f->d0, d1 = f->d1;
    for (int i = 0; i < f->m; ++i) f->r[i] *= w;
    for (int i = 0; i < f->m * d0; ++i) f->J0[i] *= w;
    for (int i = 0; i < f->m * d1; ++i) f->J1[i] *= w;
  }
}

// (the parameter blocks are fp64 in every build; the factors take them as fscalar)
template <int N> inline void load_block(const double* src, fscalar (&dst)[N]) { for (int k = 0; k < N; ++k) dst[k] = src[k]; }

void lin_reproj(const OracleProblem& pb, int64_t i, bool jac, FactorLin* f) {
  f->m = 2; f->k0 = KIND_POSE; f->k1 = KIND_POINT; f->i0 = pb.rp_pose[i]; f->i1 = pb.rp_point[i]; f->d0 = 6; f->d1 = 3;
  fscalar pose[6], pt[3];
  load_block(&pb.poses[6 * f->i0], pose); load_block(&pb.points[3 * f->i1], pt);
  const fx::CameraConst& cam = pb.cams_f[pb.rp_cam[i]];
  const bool analytic = pb.reproj_variant == OBVI_REPROJECTION_ANALYTIC;
  if (!jac) {
    if (analytic) fx::reprojection_residual_analytic<fscalar>(pose, pt, cam, &pb.rp_pixel[2 * i], pb.rp_sigma[i], f->r);
    else fx::reprojection_residual<fscalar>(pose, pt, cam, &pb.rp_pixel[2 * i], pb.rp_sigma[i], f->r);
    return;
  }
  typedef fx::Dual<9> D;
  D dp[6], dx[3], dr[2];
  for (int k = 0; k < 6; ++k) dp[k] = D::var(pose[k], k);
  for (int k = 0; k < 3; ++k) dx[k] = D::var(pt[k], 6 + k);
  if (analytic) fx::reprojection_residual_analytic<D>(dp, dx, cam, &pb.rp_pixel[2 * i], pb.rp_sigma[i], dr);
  else fx::reprojection_residual<D>(dp, dx, cam, &pb.rp_pixel[2 * i], pb.rp_sigma[i], dr);
  for (int a = 0; a < 2; ++a) {
    f->r[a] = dr[a].v;
    for (int k = 0; k < 6; ++k) f->J0[6 * a + k] = dr[a].d[k];
    for (int k = 0; k < 3; ++k) f->J1[3 * a + k] = dr[a].d[6 + k];
  }
}

template <int OD>
void lin_bbox_od(const OracleProblem& pb, int64_t i, bool jac, FactorLin* f) {
  f->m = 4; f->k0 = KIND_OBJECT; f->k1 = KIND_POSE; f->i0 = pb.bb_obj[i]; f->i1 = pb.bb_pose[i]; f->d0 = OD; f->d1 = 6;
  fscalar ell[OD], pose[6];
  load_block(&pb.objects[OD * f->i0], ell); load_block(&pb.poses[6 * f->i1], pose);
  const fx::CameraConst& cam = pb.cams_f[pb.bb_cam[i]];
  if (!jac) { fx::bbox_residual<fscalar, OD>(ell, pose, cam, &pb.bb_rect[4 * i], &pb.bb_sqrt_inf[16 * i], pb.bb_invalid, f->r); return; }
  typedef fx::Dual<OD + 6> D;
  D de[OD], dp[6], dr[4];
  for (int k = 0; k < OD; ++k) de[k] = D::var(ell[k], k);
  for (int k = 0; k < 6; ++k) dp[k] = D::var(pose[k], OD + k);
  fx::bbox_residual<D, OD>(de, dp, cam, &pb.bb_rect[4 * i], &pb.bb_sqrt_inf[16 * i], pb.bb_invalid, dr);
  for (int a = 0; a < 4; ++a) {
    f->r[a] = dr[a].v;
    for (int k = 0; k < OD; ++k) f->J0[OD * a + k] = dr[a].d[k];
    for (int k = 0; k < 6; ++k) f->J1[6 * a + k] = dr[a].d[OD + k];
  }
}
void lin_bbox(const OracleProblem& pb, int64_t i, bool jac, FactorLin* f) { if (pb.od == 9) lin_bbox_od<9>(pb, i, jac, f); else lin_bbox_od<7>(pb, i, jac, f); }

template <int OD>
void lin_shape_od(const OracleProblem& pb, int64_t i, bool jac, FactorLin* f) {
  f->m = 3; f->k0 = KIND_OBJECT; f->k1 = KIND_NONE; f->i0 = pb.sp_obj[i]; f->i1 = -1; f->d0 = OD; f->d1 = 0;
  fscalar ell[OD];
  load_block(&pb.objects[OD * f->i0], ell);
  if (!jac) { fx::shape_prior_residual<fscalar>(ell, &pb.sp_mean[3 * i], &pb.sp_sqrt_inf[9 * i], f->r, OD); return; }
  typedef fx::Dual<OD> D;
  D de[OD], dr[3];
  for (int k = 0; k < OD; ++k) de[k] = D::var(ell[k], k);
  fx::shape_prior_residual<D>(de, &pb.sp_mean[3 * i], &pb.sp_sqrt_inf[9 * i], dr, OD);
  for (int a = 0; a < 3; ++a) { f->r[a] = dr[a].v; for (int k = 0; k < OD; ++k) f->J0[OD * a + k] = dr[a].d[k]; }
}
void lin_shape(const OracleProblem& pb, int64_t i, bool jac, FactorLin* f) { if (pb.od == 9) lin_shape_od<9>(pb, i, jac, f); else lin_shape_od<7>(pb, i, jac, f); }

template <int OD>
void lin_ltm_od(const OracleProblem& pb, int64_t i, bool jac, FactorLin* f) {
  f->m = OD; f->k0 = KIND_OBJECT; f->k1 = KIND_NONE; f->i0 = pb.lt_obj[i]; f->i1 = -1; f->d0 = OD; f->d1 = 0;
  fscalar ell[OD];
  load_block(&pb.objects[OD * f->i0], ell);
  if (!jac) { fx::ltm_prior_residual<fscalar>(ell, &pb.lt_mean[OD * i], &pb.lt_sqrt_inf[OD * OD * i], f->r, OD); return; }
  typedef fx::Dual<OD> D;
  D de[OD], dr[OD];
  for (int k = 0; k < OD; ++k) de[k] = D::var(ell[k], k);
  fx::ltm_prior_residual<D>(de, &pb.lt_mean[OD * i], &pb.lt_sqrt_inf[OD * OD * i], dr, OD);
  for (int a = 0; a < OD; ++a) { f->r[a] = dr[a].v; for (int k = 0; k < OD; ++k) f->J0[OD * a + k] = dr[a].d[k]; }
}
void lin_ltm(const OracleProblem& pb, int64_t i, bool jac, FactorLin* f) { if (pb.od == 9) lin_ltm_od<9>(pb, i, jac, f); else lin_ltm_od<7>(pb, i, jac, f); }

void lin_relpose(const OracleProblem& pb, int64_t i, bool jac, FactorLin* f) {
  f->m = 6; f->k0 = KIND_POSE; f->k1 = KIND_POSE; f->i0 = pb.rl_a[i]; f->i1 = pb.rl_b[i]; f->d0 = 6; f->d1 = 6;
  fscalar pa[6], pbb[6];
  load_block(&pb.poses[6 * f->i0], pa); load_block(&pb.poses[6 * f->i1], pbb);
  if (!jac) { fx::relpose_residual<fscalar>(pa, pbb, &pb.rl_t[3 * i], &pb.rl_R[9 * i], &pb.rl_sqrt_inf[36 * i], f->r); return; }
  typedef fx::Dual<12> D;
  D da[6], db[6], dr[6];
  for (int k = 0; k < 6; ++k) { da[k] = D::var(pa[k], k); db[k] = D::var(pbb[k], 6 + k); }
  fx::relpose_residual<D>(da, db, &pb.rl_t[3 * i], &pb.rl_R[9 * i], &pb.rl_sqrt_inf[36 * i], dr);
  for (int a = 0; a < 6; ++a) {
    f->r[a] = dr[a].v;
    for (int k = 0; k < 6; ++k) { f->J0[6 * a + k] = dr[a].d[k]; f->J1[6 * a + k] = dr[a].d[6 + k]; }
  }
}

// factor families in the fixed order 0,2,3,4,5 used by evaluate()
struct Family {
  int type; int m; int64_t n; const std::vector<uint8_t>* active; double huber;
  void (*lin)(const OracleProblem&, int64_t, bool, FactorLin*);
};
std::vector<Family> families(const OracleProblem& pb) {
  return {{OBVI_FACTOR_REPROJECTION, 2, pb.n_rp, &pb.rp_active, pb.rp_huber, lin_reproj},
          {OBVI_FACTOR_BBOX, 4, pb.n_bb, &pb.bb_active, pb.bb_huber, lin_bbox},
          {OBVI_FACTOR_SHAPE_PRIOR, 3, pb.n_sp, &pb.sp_active, pb.sp_huber, lin_shape},
          {OBVI_FACTOR_LTM_PRIOR, pb.od, pb.n_lt, &pb.lt_active, pb.lt_huber, lin_ltm},
          {OBVI_FACTOR_REL_POSE, 6, pb.n_rl, &pb.rl_active, pb.rl_huber, lin_relpose}};
}

bool block_const(const OracleProblem& pb, BlockKind k, int64_t i) {
  switch (k) {
    case KIND_POSE: return pb.pose_const[i] != 0;
    case KIND_POINT: return pb.point_const[i] != 0;
    case KIND_OBJECT: return pb.object_const[i] != 0;
    default: return true;
  }
}

// ---------------------------------------------------------------------------------------
// Reduced-program bookkeeping [Ceres-doc: Program::RemoveFixedBlocks]: constant parameter
// blocks are dropped, residual blocks whose every parameter block is constant go into
// fixed_cost, parameter blocks touched by no remaining residual block are dropped too.
// ---------------------------------------------------------------------------------------
struct Reduced {
  std::vector<int32_t> pose_vid, obj_vid;  // index among variable+used blocks or -1
  std::vector<uint8_t> point_var;          // variable+used
  int64_t nPv = 0, nOv = 0, nLv = 0;
  int od = 7;                              // parameters of an ellipsoid block
  int64_t m = 0;                           // reduced (Schur) system rows = 6 nPv + od nOv
  int64_t num_params = 0, num_residuals = 0;
  double fixed_cost = 0.0;
  int64_t nOs = 0;                         // shared variable objects: the LAST nOs object blocks of the reduced system
  int64_t shared_row0 = 0;                 // first row of the shared objects (= m without any)
};

struct Workspace {
  // per-factor linearisation records of the variable part of the problem
  std::vector<FactorLin> lin;
  // skyline storage of the reduced system: row i holds columns first[i]..i
  std::vector<int64_t> first, rowptr;
  std::vector<real> S, rhs;
  // point blocks
  std::vector<real> Hll, gl;              // 9 / 3 per point
  std::vector<double> Hpp_diag;           // diag(J^T J) per reduced row (poses, objects)
  std::vector<real> colsq_c, colsq_l;     // squared column norms: reduced rows / points (3 per point)
  std::vector<real> g_c;                  // gradient, reduced rows
  std::vector<std::vector<int64_t>> point_obs;  // per point: indices into lin of its reprojection records
  std::vector<real> Wall;                       // scratch of assemble_schur: W = J_p^T J_l per factor record (kept between calls: no 400-MB allocation per LM step)
  int64_t object_row0 = 0;                // first object row of the reduced system (= 6 nPv): rows from here on form the arrow's border
};

inline int64_t pose_row(const Reduced& rd, int64_t p) { return 6 * (int64_t)rd.pose_vid[p]; }
inline int64_t obj_row(const Reduced& rd, int64_t o) { return 6 * rd.nPv + rd.od * (int64_t)rd.obj_vid[o]; }

void build_reduced(const OracleProblem& pb, Reduced* rd) {
  rd->pose_vid.assign(pb.P, -1); rd->obj_vid.assign(pb.O, -1); rd->point_var.assign(pb.L, 0);
  std::vector<uint8_t> pose_used(pb.P, 0), obj_used(pb.O, 0), point_used(pb.L, 0);
  rd->num_residuals = 0; rd->fixed_cost = 0.0;
  for (const Family& fam : families(pb)) {
    for (int64_t i = 0; i < fam.n; ++i) {
      if (!(*fam.active)[i]) continue;
      FactorLin f; fam.lin(pb, i, false, &f);
      const bool c0 = block_const(pb, f.k0, f.i0), c1 = block_const(pb, f.k1, f.i1);
      if (c0 && c1) {  // all-constant residual block -> fixed cost
        robustify(&f, fam.huber, true);
        rd->fixed_cost += f.cost;
        continue;
      }
      rd->num_residuals += fam.m;
      auto mark = [&](BlockKind k, int64_t idx) {
        if (k == KIND_POSE) pose_used[idx] = 1; else if (k == KIND_POINT) point_used[idx] = 1; else if (k == KIND_OBJECT) obj_used[idx] = 1;
      };
      if (!c0) mark(f.k0, f.i0);
      if (!c1) mark(f.k1, f.i1);
    }
  }
  rd->nPv = rd->nOv = rd->nLv = 0;
  const bool sharing = (int64_t)pb.is_shared.size() == pb.O;
  auto shared = [&](int64_t o) { return sharing && pb.is_shared[o] != 0; };
  for (int64_t o = 0; o < pb.O; ++o) if (shared(o)) obj_used[o] = 1;   // a shared object exists on every rank, observed there or not
  for (int64_t p = 0; p < pb.P; ++p) if (!pb.pose_const[p] && pose_used[p]) rd->pose_vid[p] = (int32_t)rd->nPv++;
  for (int64_t o = 0; o < pb.O; ++o) if (!pb.object_const[o] && obj_used[o] && !shared(o)) rd->obj_vid[o] = (int32_t)rd->nOv++;
  rd->nOs = 0;
  for (int64_t o = 0; o < pb.O; ++o) if (!pb.object_const[o] && obj_used[o] && shared(o)) { rd->obj_vid[o] = (int32_t)rd->nOv++; rd->nOs++; }   // eliminated last, in index order
  for (int64_t l = 0; l < pb.L; ++l) if (!pb.point_const[l] && point_used[l]) { rd->point_var[l] = 1; rd->nLv++; }
  rd->od = pb.od;
  rd->m = 6 * rd->nPv + rd->od * rd->nOv;
  rd->shared_row0 = rd->m - rd->od * rd->nOs;
  rd->num_params = rd->m + 3 * rd->nLv;
}

bool is_var(const OracleProblem& pb, const Reduced& rd, BlockKind k, int64_t i) {
  switch (k) {
    case KIND_POSE: return rd.pose_vid[i] >= 0;
    case KIND_POINT: return rd.point_var[i] != 0;
    case KIND_OBJECT: return rd.obj_vid[i] >= 0;
    default: return false;
  }
  (void)pb;
}
int64_t reduced_row(const Reduced& rd, BlockKind k, int64_t i) {
  return k == KIND_POSE ? pose_row(rd, i) : obj_row(rd, i);
}

// Cost only (trial point evaluation) over the reduced program.
double reduced_cost(const OracleProblem& pb, const Reduced& rd) {
  real cost = 0.0;
  for (const Family& fam : families(pb)) {
    // every factor's cost on the host threads, then ONE running sum in factor order: the same bits for any thread count
    std::vector<real> each((size_t)fam.n, 0.0);
    parallel_ranges(fam.n, [&](int, int64_t i0, int64_t i1) {
      for (int64_t i = i0; i < i1; ++i) {
        if (!(*fam.active)[i]) continue;
        FactorLin f; fam.lin(pb, i, false, &f);
        if (!is_var(pb, rd, f.k0, f.i0) && !is_var(pb, rd, f.k1, f.i1)) continue;
        robustify(&f, fam.huber, true);
        each[(size_t)i] = f.cost;
      }
    });
    for (real c : each) cost += c;
  }
  return (double)cost;
}

// Full linearisation at the current estimate: robustified r, J per residual block;
// squared column norms, gradient, point blocks; skyline envelope of the reduced system.
double linearize(const OracleProblem& pb, const Reduced& rd, Workspace* ws) {
  const bool timing = std::getenv("OBVI_ORACLE_TIMING") != nullptr;
  const double t_begin = now_s();
  ws->lin.clear();
  ws->point_obs.assign(pb.L, {});
  real cost = 0.0;
  for (const Family& fam : families(pb)) {
    if (g_threads > 1 && fam.n >= 1024) {
      // same records in the same order as the loop below: which factors stay is decided first (values only, cheap), then the
      // records are filled at their final positions by ranges of factors on host threads
      std::vector<int64_t> slot((size_t)fam.n, -1);
      std::vector<uint8_t> keep((size_t)fam.n, 0);
      parallel_ranges(fam.n, [&](int, int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
          if (!(*fam.active)[i]) continue;
          FactorLin f; fam.lin(pb, i, false, &f);   // block kinds / indices (and a value that is not used)
          keep[i] = is_var(pb, rd, f.k0, f.i0) || is_var(pb, rd, f.k1, f.i1);
        }
      });
      int64_t next = (int64_t)ws->lin.size();
      for (int64_t i = 0; i < fam.n; ++i) if (keep[i]) slot[i] = next++;
      ws->lin.resize((size_t)next);
      parallel_ranges(fam.n, [&](int, int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
          if (slot[i] < 0) continue;
          FactorLin& f = ws->lin[slot[i]];
          fam.lin(pb, i, true, &f);
          robustify(&f, fam.huber, true);
          if (!is_var(pb, rd, f.k0, f.i0)) std::memset(f.J0, 0, sizeof(f.J0));
          if (!is_var(pb, rd, f.k1, f.i1)) std::memset(f.J1, 0, sizeof(f.J1));
        }
      });
      for (int64_t i = 0; i < fam.n; ++i) {
        if (slot[i] < 0) continue;
        const FactorLin& f = ws->lin[slot[i]];
        cost += f.cost;
        if (fam.type == OBVI_FACTOR_REPROJECTION && is_var(pb, rd, f.k1, f.i1)) ws->point_obs[f.i1].push_back(slot[i]);
      }
      continue;
    }
    for (int64_t i = 0; i < fam.n; ++i) {
      if (!(*fam.active)[i]) continue;
      FactorLin f; fam.lin(pb, i, true, &f);
      const bool v0 = is_var(pb, rd, f.k0, f.i0), v1 = is_var(pb, rd, f.k1, f.i1);
      if (!v0 && !v1) continue;
      robustify(&f, fam.huber, true);
      cost += f.cost;
      if (!v0) { std::memset(f.J0, 0, sizeof(f.J0)); }
      if (!v1) { std::memset(f.J1, 0, sizeof(f.J1)); }
      if (fam.type == OBVI_FACTOR_REPROJECTION && v1) ws->point_obs[f.i1].push_back((int64_t)ws->lin.size());
      ws->lin.push_back(f);
    }
  }
  if (timing) std::fprintf(stderr, "oracle linearize: factor records %.3f s\n", now_s() - t_begin);
  // squared column norms and gradient
  ws->colsq_c.assign(rd.m, 0.0); ws->g_c.assign(rd.m, 0.0);
  ws->colsq_l.assign(3 * pb.L, 0.0); ws->gl.assign(3 * pb.L, 0.0); ws->Hll.assign(9 * pb.L, 0.0);
  for (const FactorLin& f : ws->lin) {
    const BlockKind ks[2] = {f.k0, f.k1}; const int64_t is[2] = {f.i0, f.i1}; const fscalar* Js[2] = {f.J0, f.J1};
    for (int b = 0; b < 2; ++b) {
      if (!is_var(pb, rd, ks[b], is[b])) continue;
      const int d = b == 0 ? f.d0 : f.d1;
      if (ks[b] == KIND_POINT) {
        real* c = &ws->colsq_l[3 * is[b]]; real* g = &ws->gl[3 * is[b]]; real* H = &ws->Hll[9 * is[b]];
        for (int a = 0; a < f.m; ++a) for (int k = 0; k < 3; ++k) {
          const real j = Js[b][3 * a + k];
          c[k] += j * j; g[k] += j * f.r[a];
          for (int k2 = 0; k2 < 3; ++k2) H[3 * k + k2] += j * Js[b][3 * a + k2];
        }
      } else {
        const int64_t row = reduced_row(rd, ks[b], is[b]);
        for (int a = 0; a < f.m; ++a) for (int k = 0; k < d; ++k) {
          const real j = Js[b][d * a + k];
          ws->colsq_c[row + k] += j * j; ws->g_c[row + k] += j * f.r[a];
        }
      }
    }
  }
  if (timing) std::fprintf(stderr, "oracle linearize: total %.3f s\n", now_s() - t_begin);
  return (double)cost;
}

// Envelope of the reduced system: block row r couples to the lowest reduced row it shares a
// residual block (relpose, bbox) or an eliminated point with.
void build_envelope(const OracleProblem& pb, const Reduced& rd, Workspace* ws) {
  ws->first.resize(rd.m);
  ws->object_row0 = 6 * rd.nPv;
  // every row of a diagonal block reaches back to the block's first row
  for (int64_t v = 0; v < rd.nPv; ++v) for (int k = 0; k < 6; ++k) ws->first[6 * v + k] = 6 * v;
  for (int64_t w = 0; w < rd.nOv; ++w) for (int k = 0; k < rd.od; ++k) ws->first[6 * rd.nPv + rd.od * w + k] = 6 * rd.nPv + rd.od * w;
  auto couple = [&](int64_t ra, int da, int64_t rb, int db) {
    if (ra < rb) { std::swap(ra, rb); std::swap(da, db); }
    for (int k = 0; k < da; ++k) ws->first[ra + k] = std::min(ws->first[ra + k], rb);
    (void)db;
  };
  for (const FactorLin& f : ws->lin) {
    if (f.k0 == KIND_POINT || f.k1 == KIND_POINT || f.k1 == KIND_NONE) continue;
    if (!is_var(pb, rd, f.k0, f.i0) || !is_var(pb, rd, f.k1, f.i1)) continue;
    couple(reduced_row(rd, f.k0, f.i0), f.d0, reduced_row(rd, f.k1, f.i1), f.d1);
  }
  for (int64_t l = 0; l < pb.L; ++l) {
    const std::vector<int64_t>& obs = ws->point_obs[l];
    int64_t lo = std::numeric_limits<int64_t>::max();
    for (int64_t idx : obs) { const FactorLin& f = ws->lin[idx]; if (rd.pose_vid[f.i0] >= 0) lo = std::min(lo, pose_row(rd, f.i0)); }
    for (int64_t idx : obs) {
      const FactorLin& f = ws->lin[idx];
      if (rd.pose_vid[f.i0] < 0) continue;
      const int64_t row = pose_row(rd, f.i0);
      for (int k = 0; k < 6; ++k) ws->first[row + k] = std::min(ws->first[row + k], lo);
    }
  }
  ws->rowptr.assign(rd.m + 1, 0);
  for (int64_t i = 0; i < rd.m; ++i) ws->rowptr[i + 1] = ws->rowptr[i] + (i - ws->first[i] + 1);
  ws->S.assign(ws->rowptr[rd.m], 0.0);
  ws->rhs.assign(rd.m, 0.0);
}
inline real& Sat(Workspace* ws, int64_t i, int64_t j) {  // i >= j >= first[i]
  return ws->S[ws->rowptr[i] + (j - ws->first[i])];
}

// Assemble the Schur complement for the per-parameter damping lambda (unscaled normal
// equations, see solve()):  (H + Lambda) y = g  with the points eliminated.
// [Ceres-doc: SchurEliminator::Eliminate]
bool assemble_schur(const OracleProblem& pb, const Reduced& rd, const std::vector<real>& lam_c,
                    const std::vector<real>& lam_l, Workspace* ws, std::vector<real>* Hll_inv) {
  std::fill(ws->S.begin(), ws->S.end(), 0.0);
  for (int64_t i = 0; i < rd.m; ++i) { ws->rhs[i] = ws->g_c[i]; Sat(ws, i, i) = lam_c[i]; }
  // camera/object blocks: J_c^T J_c (lower triangle).  A factor's two blocks are distinct
  // parameter blocks (pose/object, or two different poses), so ra != rb whenever a != b.
  for (const FactorLin& f : ws->lin) {
    const BlockKind ks[2] = {f.k0, f.k1}; const int64_t is[2] = {f.i0, f.i1}; const fscalar* Js[2] = {f.J0, f.J1};
    for (int a = 0; a < 2; ++a) {
      if (ks[a] == KIND_POINT || ks[a] == KIND_NONE || !is_var(pb, rd, ks[a], is[a])) continue;
      const int da = a == 0 ? f.d0 : f.d1; const int64_t ra = reduced_row(rd, ks[a], is[a]);
      for (int b = 0; b < 2; ++b) {
        if (ks[b] == KIND_POINT || ks[b] == KIND_NONE || !is_var(pb, rd, ks[b], is[b])) continue;
        const int db = b == 0 ? f.d0 : f.d1; const int64_t rb = reduced_row(rd, ks[b], is[b]);
        if (rb > ra || (a != b && ra == rb)) continue;
        for (int x = 0; x < da; ++x) for (int y = 0; y < db; ++y) {
          if (ra == rb && y > x) continue;
          real acc = 0.0;
          for (int q = 0; q < f.m; ++q) acc += (real)Js[a][da * q + x] * Js[b][db * q + y];
          Sat(ws, ra + x, rb + y) += acc;
        }
      }
    }
  }
  // eliminate points
  Hll_inv->assign(9 * pb.L, 0.0);
  // Host threads (g_threads > 1), in two passes so that the result does not depend on their number (round 6: an oracle whose bits change with
  // the thread count cannot back a committed end state):
  //   (A) ranges of points: H_ll^-1 and W_i = J_p,i^T J_l,i of every observation -- independent per point;
  //   (B) ranges of pose block rows: a row's right-hand side and blocks are written by ONE thread, which walks the row's observations in
  //       ascending (point, observation) order -- the order in which the one-thread loop reaches them -- so every entry subtracts the same
  //       products in the same order whatever g_threads is (1 included).
  std::vector<uint8_t> bad_part((size_t)std::max(1, g_threads), 0);
  std::vector<real>& Wall = ws->Wall;            // by factor record (every entry that is read below is written first)
  if (Wall.size() < 18 * ws->lin.size()) Wall.resize(18 * ws->lin.size());
  parallel_ranges(pb.L, [&](int tid, int64_t l_begin, int64_t l_end) {
  for (int64_t l = l_begin; l < l_end; ++l) {
    if (!rd.point_var[l]) continue;
    real H[9];
    for (int k = 0; k < 9; ++k) H[k] = ws->Hll[9 * l + k];
    for (int k = 0; k < 3; ++k) H[4 * k] += lam_l[3 * l + k];
    // 3x3 symmetric inverse via cofactors
    const real c00 = H[4] * H[8] - H[5] * H[7], c01 = H[5] * H[6] - H[3] * H[8], c02 = H[3] * H[7] - H[4] * H[6];
    const real det = H[0] * c00 + H[1] * c01 + H[2] * c02;
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) { bad_part[tid] = 1; return; }
    real* Hi = &(*Hll_inv)[9 * l];
    Hi[0] = c00 / det; Hi[1] = (H[2] * H[7] - H[1] * H[8]) / det; Hi[2] = (H[1] * H[5] - H[2] * H[4]) / det;
    Hi[3] = Hi[1];     Hi[4] = (H[0] * H[8] - H[2] * H[6]) / det; Hi[5] = (H[2] * H[3] - H[0] * H[5]) / det;
    Hi[6] = Hi[2];     Hi[7] = Hi[5];                             Hi[8] = (H[0] * H[4] - H[1] * H[3]) / det;
    // W_i = J_p,i^T J_l,i (6x3) for observations with a variable pose
    for (int64_t idx : ws->point_obs[l]) {
      const FactorLin& f = ws->lin[idx];
      if (rd.pose_vid[f.i0] < 0) continue;
      real* Wa = &Wall[18 * idx];
      for (int x = 0; x < 6; ++x) for (int k = 0; k < 3; ++k)
        Wa[3 * x + k] = (real)f.J0[x] * f.J1[k] + (real)f.J0[6 + x] * f.J1[3 + k];
    }
  }
  });
  for (uint8_t b : bad_part) if (b) return false;
  // the observations of every variable pose: (point, position in the point's list), ascending
  std::vector<std::vector<std::pair<int64_t, int32_t>>> by_pose((size_t)rd.nPv);
  for (int64_t l = 0; l < pb.L; ++l) {
    if (!rd.point_var[l]) continue;
    const std::vector<int64_t>& obs = ws->point_obs[l];
    for (size_t a = 0; a < obs.size(); ++a) {
      const int32_t vid = rd.pose_vid[ws->lin[obs[a]].i0];
      if (vid >= 0) by_pose[(size_t)vid].push_back({l, (int32_t)a});
    }
  }
  parallel_ranges(rd.nPv, [&](int, int64_t v_begin, int64_t v_end) {
  for (int64_t v = v_begin; v < v_end; ++v) {
    for (const auto& la : by_pose[(size_t)v]) {
      const int64_t l = la.first;
      const std::vector<int64_t>& obs = ws->point_obs[l];
      const FactorLin& fa = ws->lin[obs[la.second]];
      const real* Hi = &(*Hll_inv)[9 * l];
      const real* Wa = &Wall[18 * obs[la.second]];
      real Ya[18];
      for (int x = 0; x < 6; ++x) for (int k = 0; k < 3; ++k)
        Ya[3 * x + k] = Wa[3 * x] * Hi[k] + Wa[3 * x + 1] * Hi[3 + k] + Wa[3 * x + 2] * Hi[6 + k];
      const int64_t ra = pose_row(rd, fa.i0);
      for (int x = 0; x < 6; ++x)
        ws->rhs[ra + x] -= Ya[3 * x] * ws->gl[3 * l] + Ya[3 * x + 1] * ws->gl[3 * l + 1] + Ya[3 * x + 2] * ws->gl[3 * l + 2];
      for (size_t b = 0; b < obs.size(); ++b) {
        const FactorLin& fb = ws->lin[obs[b]];
        if (rd.pose_vid[fb.i0] < 0) continue;
        const int64_t rb = pose_row(rd, fb.i0);
        if (rb > ra) continue;
        const real* Wb = &Wall[18 * obs[b]];
        for (int x = 0; x < 6; ++x) for (int y = 0; y < 6; ++y) {
          if (ra == rb && y > x) continue;
          Sat(ws, ra + x, rb + y) -= Ya[3 * x] * Wb[3 * y] + Ya[3 * x + 1] * Wb[3 * y + 1] + Ya[3 * x + 2] * Wb[3 * y + 2];
        }
      }
    }
  }
  });
  return true;
}

// In-place envelope (skyline) Cholesky S = L L^T and solve.  [Ceres-doc: the reduced system
// is factorised exactly by a sparse Cholesky; the elimination order does not change the result.]
// Host threads (g_threads > 1): the same factorisation with the object rows (the border of the arrow: rows >= object_row0, whose
// envelopes reach far back into the pose band) split so that their long dot products run in parallel.  Every entry subtracts the
// same products in the same order as the sequential loop, so the factor is bit-identical:
//   band   rows < r0, sequential (narrow envelopes: a fraction of a percent of the flops)
//   (1)    entries (i, j < r0) of the border rows: need band rows only -> parallel over border rows
//   (2a)   entries (i, j >= r0): the part of the dot product over k < r0 -> parallel over border rows (reads (1) only)
//   (2b)   the remaining part over k >= r0 and the division: the dense Cholesky of the border block, sequential
bool skyline_factor_arrow(Workspace* ws, int64_t m) {
  const int64_t r0 = std::min(ws->object_row0, m);
  auto row = [&](int64_t i) { return &ws->S[ws->rowptr[i]] - ws->first[i]; };
  bool ok = true;
  for (int64_t i = 0; i < r0 && ok; ++i) {
    const int64_t fi = ws->first[i];
    real* Li = row(i);
    for (int64_t j = fi; j < i; ++j) {
      const int64_t fj = ws->first[j];
      const real* Lj = row(j);
      real s = Li[j];
      for (int64_t k = std::max(fi, fj); k < j; ++k) s -= Li[k] * Lj[k];
      Li[j] = s / Lj[j];
    }
    real s = Li[i];
    for (int64_t k = fi; k < i; ++k) s -= Li[k] * Li[k];
    if (!(s > 0.0) || !std::isfinite(s)) ok = false;
    Li[i] = std::sqrt(s);
  }
  if (!ok) return false;
  const int64_t nb = m - r0;
  // interleaved assignment of border rows to threads (their costs grow with the row index)
  auto border_rows = [&](auto&& body) {
    parallel_ranges(std::min<int64_t>(g_threads, std::max<int64_t>(nb, 1)), [&](int, int64_t t0, int64_t t1) {
      for (int64_t t = t0; t < t1; ++t) for (int64_t i = r0 + t; i < m; i += std::min<int64_t>(g_threads, std::max<int64_t>(nb, 1))) body(i);
    });
  };
  border_rows([&](int64_t i) {   // (1)
    const int64_t fi = ws->first[i];
    real* Li = row(i);
    for (int64_t j = fi; j < std::min(i, r0); ++j) {
      const int64_t fj = ws->first[j];
      const real* Lj = row(j);
      real s = Li[j];
      for (int64_t k = std::max(fi, fj); k < j; ++k) s -= Li[k] * Lj[k];
      Li[j] = s / Lj[j];
    }
  });
  border_rows([&](int64_t i) {   // (2a)
    const int64_t fi = ws->first[i];
    real* Li = row(i);
    for (int64_t j = std::max(fi, r0); j <= i; ++j) {
      const int64_t fj = ws->first[j];
      const real* Lj = row(j);
      real s = Li[j];
      for (int64_t k = std::max(fi, fj); k < std::min(j, r0); ++k) s -= Li[k] * Lj[k];
      Li[j] = s;
    }
  });
  for (int64_t i = r0; i < m; ++i) {   // (2b)
    const int64_t fi = ws->first[i];
    real* Li = row(i);
    for (int64_t j = std::max(fi, r0); j < i; ++j) {
      const int64_t fj = ws->first[j];
      const real* Lj = row(j);
      real s = Li[j];
      for (int64_t k = std::max({fi, fj, r0}); k < j; ++k) s -= Li[k] * Lj[k];
      Li[j] = s / Lj[j];
    }
    real s = Li[i];
    for (int64_t k = std::max(fi, r0); k < i; ++k) s -= Li[k] * Li[k];
    if (!(s > 0.0) || !std::isfinite(s)) return false;
    Li[i] = std::sqrt(s);
  }
  return true;
}
bool skyline_factor(Workspace* ws, int64_t m) {
  if (g_threads > 1 && ws->object_row0 < m) return skyline_factor_arrow(ws, m);
  for (int64_t i = 0; i < m; ++i) {
    const int64_t fi = ws->first[i];
    real* Li = &ws->S[ws->rowptr[i]] - fi;
    for (int64_t j = fi; j < i; ++j) {
      const int64_t fj = ws->first[j];
      const real* Lj = &ws->S[ws->rowptr[j]] - fj;
      const int64_t k0 = std::max(fi, fj);
      real s = Li[j];
      for (int64_t k = k0; k < j; ++k) s -= Li[k] * Lj[k];
      Li[j] = s / Lj[j];
    }
    real s = Li[i];
    for (int64_t k = fi; k < i; ++k) s -= Li[k] * Li[k];
    if (!(s > 0.0) || !std::isfinite(s)) return false;
    Li[i] = std::sqrt(s);
  }
  return true;
}
void skyline_solve_inplace(const Workspace* ws, int64_t m, std::vector<real>* x) {
  for (int64_t i = 0; i < m; ++i) {  // L z = b
    const int64_t fi = ws->first[i];
    const real* Li = &ws->S[ws->rowptr[i]] - fi;
    real s = (*x)[i];
    for (int64_t k = fi; k < i; ++k) s -= Li[k] * (*x)[k];
    (*x)[i] = s / Li[i];
  }
  for (int64_t i = m - 1; i >= 0; --i) {  // L^T y = z
    const int64_t fi = ws->first[i];
    const real* Li = &ws->S[ws->rowptr[i]] - fi;
    const real xi = (*x)[i] / Li[i];
    (*x)[i] = xi;
    for (int64_t k = fi; k < i; ++k) (*x)[k] -= Li[k] * xi;
  }
}
bool skyline_cholesky_solve(Workspace* ws, int64_t m, std::vector<real>* x) {
  if (!skyline_factor(ws, m)) return false;
  x->assign(ws->rhs.begin(), ws->rhs.end());
  skyline_solve_inplace(ws, m, x);
  return true;
}

// The reduced solve of a rank whose last rows belong to objects shared with other ranks (include/obvi_ba.h, exchange (2)): the rank's own
// rows A = [0, r0) are eliminated, the Schur complement onto the shared rows B and its right-hand side are summed over the ranks through the
// hook, every rank factorises the sum and back-substitutes into its own rows.  Dense (row-oriented Cholesky on the expanded envelope): this
// path exists for problems the tests hold against the joint solve.  A rank whose own block is not positive definite still takes part in the
// exchange (the ranks must stay in step) and reports the failure; the caller sums the failure flags.
bool shared_tail_solve(const OracleProblem& pb, Workspace* ws, int64_t m, int64_t r0, std::vector<real>* y) {
  const int64_t nB = m - r0;
  std::vector<real> D((size_t)m * (size_t)m, 0.0);
  for (int64_t i = 0; i < m; ++i) for (int64_t j = ws->first[i]; j <= i; ++j) D[(size_t)i * m + j] = ws->S[ws->rowptr[i] + (j - ws->first[i])];
  std::vector<real> z(ws->rhs.begin(), ws->rhs.end());
  bool ok = true;
  for (int64_t i = 0; i < m && ok; ++i) {
    real* Li = &D[(size_t)i * m];
    const int64_t jend = std::min(i, r0 - 1);
    for (int64_t j = 0; j <= jend; ++j) {            // columns of A
      const real* Lj = &D[(size_t)j * m];
      real v = Li[j];
      for (int64_t k = 0; k < j; ++k) v -= Li[k] * Lj[k];
      if (j == i) { if (!(v > 0.0)) { ok = false; break; } Li[i] = std::sqrt(v); }
      else Li[j] = v / Lj[j];
    }
    if (!ok) break;
    for (int64_t j = r0; j <= i; ++j) {              // columns of B (rows of B only): the Schur complement, not divided yet
      const real* Lj = &D[(size_t)j * m];
      real v = Li[j];
      for (int64_t k = 0; k < r0; ++k) v -= Li[k] * Lj[k];
      Li[j] = v;
    }
    real t = z[i];                                    // forward substitution through the columns of A
    for (int64_t k = 0; k < std::min(i, r0); ++k) t -= Li[k] * z[k];
    z[i] = i < r0 ? t / Li[i] : t;
  }
  std::vector<double> buf((size_t)(nB * (nB + 1) / 2 + nB), 0.0);
  if (ok) {
    size_t q = 0;
    for (int64_t i = r0; i < m; ++i) for (int64_t j = r0; j <= i; ++j) buf[q++] = (double)D[(size_t)i * m + j];
    for (int64_t i = r0; i < m; ++i) buf[q++] = (double)z[i];
  }
  if (pb.allreduce(pb.allreduce_user, buf.data(), (int64_t)buf.size(), 0, nullptr)) return false;
  if (!ok) return false;
  {
    size_t q = 0;
    for (int64_t i = r0; i < m; ++i) for (int64_t j = r0; j <= i; ++j) D[(size_t)i * m + j] = buf[q++];
    for (int64_t i = r0; i < m; ++i) z[i] = buf[q++];
  }
  for (int64_t i = r0; i < m; ++i) {                  // the summed block: the same factorisation on every rank
    real* Li = &D[(size_t)i * m];
    for (int64_t j = r0; j <= i; ++j) {
      const real* Lj = &D[(size_t)j * m];
      real v = Li[j];
      for (int64_t k = r0; k < j; ++k) v -= Li[k] * Lj[k];
      if (j == i) { if (!(v > 0.0)) return false; Li[i] = std::sqrt(v); }
      else Li[j] = v / Lj[j];
    }
    real t = z[i];
    for (int64_t k = r0; k < i; ++k) t -= Li[k] * z[k];
    z[i] = t / Li[i];
  }
  for (int64_t i = m - 1; i >= 0; --i) {              // L^T y = z
    const real yi = z[i] / D[(size_t)i * m + i];
    z[i] = yi;
    for (int64_t k = 0; k < i; ++k) z[k] -= D[(size_t)i * m + k] * yi;
  }
  y->assign(z.begin(), z.end());
  return true;
}

void copy_params(const OracleProblem& pb, std::vector<double>* a, std::vector<double>* b, std::vector<double>* c) {
  *a = pb.poses; *b = pb.points; *c = pb.objects;
}

}  // namespace

// =========================================================================================
// C interface (mirrors include/obvi_ba.h, prefix oracle_)
// =========================================================================================
extern "C" {

struct oracle_handle { OracleProblem pb; };

// host threads of the oracle's parallel parts (process-wide; 1 = the sequential reference order)
void oracle_set_threads(int32_t n) { g_threads = std::max<int32_t>(1, n); }
int32_t oracle_get_threads(void) { return g_threads; }

int oracle_ba_create(const obvi_ba_options* opt, oracle_handle** out) {
  if (!out) return OBVI_ERR_INVALID_ARGUMENT;
  if (opt && opt->object_block_size != 0 && opt->object_block_size != 7 && opt->object_block_size != 9) return OBVI_ERR_INVALID_ARGUMENT;
  if (opt && opt->reprojection_variant != OBVI_REPROJECTION_AUTODIFF && opt->reprojection_variant != OBVI_REPROJECTION_ANALYTIC) return OBVI_ERR_INVALID_ARGUMENT;
  *out = new oracle_handle();
  if (opt) { (*out)->pb.reproj_variant = opt->reprojection_variant; if (opt->object_block_size == 9) (*out)->pb.od = 9; }
  if (false) (*out)->pb.reproj_variant = 0;   // opt->deterministic: the oracle is sequential in its sums, always deterministic
  return OBVI_OK;
}
void oracle_ba_destroy(oracle_handle* h) { delete h; }
// the counterpart of obvi_ba_reset (include/obvi_ba.h): the problem a fresh handle holds, same reprojection functor
int oracle_ba_reset(oracle_handle* h) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  const int variant = h->pb.reproj_variant;
  h->pb = OracleProblem();
  h->pb.reproj_variant = variant;
  return OBVI_OK;
}

int oracle_ba_set_cameras(oracle_handle* h, int32_t n, const double* K, const double* ext) {
  if (!h || n < 0 || (n > 0 && (!K || !ext))) return OBVI_ERR_INVALID_ARGUMENT;
  h->pb.cams.resize(n); h->pb.cams_f.resize(n);
  for (int i = 0; i < n; ++i) {
    make_camera_const(K + 4 * i, ext + 7 * i, &h->pb.cams[i]);
    fscalar Kf[4], ef[7];
    for (int k = 0; k < 4; ++k) Kf[k] = K[4 * i + k];
    for (int k = 0; k < 7; ++k) ef[k] = ext[7 * i + k];
    fx::make_camera_const(Kf, ef, &h->pb.cams_f[i]);
  }
  return OBVI_OK;
}
static void set_block(std::vector<double>* dst, std::vector<uint8_t>* cdst, int64_t n, int dim, const double* v, const uint8_t* c) {
  dst->assign(v, v + n * dim);
  if (c) cdst->assign(c, c + n); else cdst->assign(n, 0);
}
int oracle_ba_set_poses(oracle_handle* h, int64_t n, const double* v, const uint8_t* c) {
  if (!h || n < 0 || (n > 0 && !v)) return OBVI_ERR_INVALID_ARGUMENT;
  h->pb.P = n; set_block(&h->pb.poses, &h->pb.pose_const, n, 6, v, c); return OBVI_OK;
}
int oracle_ba_set_points(oracle_handle* h, int64_t n, const double* v, const uint8_t* c) {
  if (!h || n < 0 || (n > 0 && !v)) return OBVI_ERR_INVALID_ARGUMENT;
  h->pb.L = n; set_block(&h->pb.points, &h->pb.point_const, n, 3, v, c); return OBVI_OK;
}
int oracle_ba_set_objects(oracle_handle* h, int64_t n, const double* v, const uint8_t* c) {
  if (!h || n < 0 || (n > 0 && !v)) return OBVI_ERR_INVALID_ARGUMENT;
  h->pb.O = n; set_block(&h->pb.objects, &h->pb.object_const, n, h->pb.od, v, c); return OBVI_OK;
}
int oracle_ba_set_const_flags(oracle_handle* h, const uint8_t* pc, const uint8_t* lc, const uint8_t* oc) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  if (pc) h->pb.pose_const.assign(pc, pc + h->pb.P);
  if (lc) h->pb.point_const.assign(lc, lc + h->pb.L);
  if (oc) h->pb.object_const.assign(oc, oc + h->pb.O);
  return OBVI_OK;
}

int oracle_ba_set_reproj(oracle_handle* h, int64_t n, const uint32_t* pose_idx, const uint32_t* point_idx,
                         const uint16_t* cam_idx, const double* pixel, const double* sigma, double sigma_scalar, double huber) {
  if (!h || n < 0 || (n > 0 && (!pose_idx || !point_idx || !pixel))) return OBVI_ERR_INVALID_ARGUMENT;
  OracleProblem& pb = h->pb;
  for (int64_t i = 0; i < n; ++i) {
    const int cam = cam_idx ? cam_idx[i] : 0;
    if (pose_idx[i] >= pb.P || point_idx[i] >= pb.L || cam >= (int)pb.cams.size()) return OBVI_ERR_OUT_OF_RANGE;
  }
  pb.n_rp = n; pb.rp_pose.assign(pose_idx, pose_idx + n); pb.rp_point.assign(point_idx, point_idx + n);
  if (cam_idx) pb.rp_cam.assign(cam_idx, cam_idx + n); else pb.rp_cam.assign(n, 0);
  pb.rp_pixel.assign(pixel, pixel + 2 * n);
  if (sigma) pb.rp_sigma.assign(sigma, sigma + n); else pb.rp_sigma.assign(n, sigma_scalar);
  pb.rp_huber = huber; pb.rp_active.assign(n, 1);
  return OBVI_OK;
}

int oracle_ba_set_bbox(oracle_handle* h, int64_t n, const uint32_t* obj_idx, const uint32_t* pose_idx, const uint16_t* cam_idx,
                       const double* corners, const double* cov, double huber, double invalid_err) {
  if (!h || n < 0 || (n > 0 && (!obj_idx || !pose_idx || !corners || !cov))) return OBVI_ERR_INVALID_ARGUMENT;
  OracleProblem& pb = h->pb;
  for (int64_t i = 0; i < n; ++i) {
    const int cam = cam_idx ? cam_idx[i] : 0;
    if (obj_idx[i] >= pb.O || pose_idx[i] >= pb.P || cam >= (int)pb.cams.size()) return OBVI_ERR_OUT_OF_RANGE;
  }
  pb.n_bb = n; pb.bb_obj.assign(obj_idx, obj_idx + n); pb.bb_pose.assign(pose_idx, pose_idx + n);
  if (cam_idx) pb.bb_cam.assign(cam_idx, cam_idx + n); else pb.bb_cam.assign(n, 0);
  pb.bb_rect.resize(4 * n); pb.bb_sqrt_inf.resize(16 * n);
  for (int64_t i = 0; i < n; ++i) {
    const fx::CameraConst& c = pb.cams_f[pb.bb_cam[i]];
    // bounding_box_factor.cpp:26-39
    fscalar si[16], cv[16];
    for (int k = 0; k < 16; ++k) cv[k] = cov[16 * i + k];
    if (!fx::spd_inverse_sqrt(cv, 4, si)) return OBVI_ERR_NUMERICAL;
    const fscalar scale[4] = {c.fx, c.fx, c.fy, c.fy};
    for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) pb.bb_sqrt_inf[16 * i + 4 * a + b] = si[4 * a + b] * scale[b];
    pb.bb_rect[4 * i + 0] = ((fscalar)corners[4 * i + 0] - c.cx) / c.fx; pb.bb_rect[4 * i + 1] = ((fscalar)corners[4 * i + 1] - c.cx) / c.fx;
    pb.bb_rect[4 * i + 2] = ((fscalar)corners[4 * i + 2] - c.cy) / c.fy; pb.bb_rect[4 * i + 3] = ((fscalar)corners[4 * i + 3] - c.cy) / c.fy;
  }
  pb.bb_huber = huber; pb.bb_invalid = invalid_err; pb.bb_active.assign(n, 1);
  return OBVI_OK;
}

int oracle_ba_set_shape_priors(oracle_handle* h, int64_t n, const uint32_t* obj_idx, const double* mean3, const double* cov9, double huber) {
  if (!h || n < 0 || (n > 0 && (!obj_idx || !mean3 || !cov9))) return OBVI_ERR_INVALID_ARGUMENT;
  OracleProblem& pb = h->pb;
  for (int64_t i = 0; i < n; ++i) if (obj_idx[i] >= pb.O) return OBVI_ERR_OUT_OF_RANGE;
  pb.n_sp = n; pb.sp_obj.assign(obj_idx, obj_idx + n); pb.sp_mean.assign(mean3, mean3 + 3 * n); pb.sp_sqrt_inf.resize(9 * n);
  for (int64_t i = 0; i < n; ++i) { fscalar cv[9]; for (int k = 0; k < 9; ++k) cv[k] = cov9[9 * i + k]; if (!fx::spd_inverse_sqrt(cv, 3, &pb.sp_sqrt_inf[9 * i])) return OBVI_ERR_NUMERICAL; }
  pb.sp_huber = huber; pb.sp_active.assign(n, 1);
  return OBVI_OK;
}

int oracle_ba_set_ltm_priors(oracle_handle* h, int64_t n, const uint32_t* obj_idx, const double* mean7, const double* cov49, double huber) {
  if (!h || n < 0 || (n > 0 && (!obj_idx || !mean7 || !cov49))) return OBVI_ERR_INVALID_ARGUMENT;
  OracleProblem& pb = h->pb;
  for (int64_t i = 0; i < n; ++i) if (obj_idx[i] >= pb.O) return OBVI_ERR_OUT_OF_RANGE;
  const int od = pb.od, od2 = od * od;
  pb.n_lt = n; pb.lt_obj.assign(obj_idx, obj_idx + n); pb.lt_mean.assign(mean7, mean7 + od * n); pb.lt_sqrt_inf.resize((size_t)od2 * n);
  for (int64_t i = 0; i < n; ++i) { fscalar cv[81]; for (int k = 0; k < od2; ++k) cv[k] = cov49[od2 * i + k]; if (!fx::spd_inverse_sqrt(cv, od, &pb.lt_sqrt_inf[od2 * i])) return OBVI_ERR_NUMERICAL; }
  pb.lt_huber = huber; pb.lt_active.assign(n, 1);
  return OBVI_OK;
}

int oracle_ba_set_relpose(oracle_handle* h, int64_t n, const uint32_t* ia, const uint32_t* ib, const double* t3, const double* aa3,
                          const double* cov36, double huber) {
  if (!h || n < 0 || (n > 0 && (!ia || !ib || !t3 || !aa3 || !cov36))) return OBVI_ERR_INVALID_ARGUMENT;
  OracleProblem& pb = h->pb;
  for (int64_t i = 0; i < n; ++i) if (ia[i] >= pb.P || ib[i] >= pb.P) return OBVI_ERR_OUT_OF_RANGE;
  // a residual block with one parameter block twice: Ceres refuses it (assemble_schur relies on two distinct blocks per factor)
  for (int64_t i = 0; i < n; ++i) if (ia[i] == ib[i]) { pb.err = "set_relpose: a factor between a pose and itself"; return OBVI_ERR_INVALID_ARGUMENT; }
  pb.n_rl = n; pb.rl_a.assign(ia, ia + n); pb.rl_b.assign(ib, ib + n); pb.rl_t.assign(t3, t3 + 3 * n);
  pb.rl_R.resize(9 * n); pb.rl_sqrt_inf.resize(36 * n);
  for (int64_t i = 0; i < n; ++i) {
    // measured_pose_deviation.orientation_.toRotationMatrix()  (relative_pose_factor.cpp:11-12)
    const fscalar a[3] = {aa3[3 * i], aa3[3 * i + 1], aa3[3 * i + 2]};
    const fscalar ang = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (ang > 0.0) { const fscalar ax[3] = {a[0] / ang, a[1] / ang, a[2] / ang}; fx::angle_axis_to_matrix(ang, ax, &pb.rl_R[9 * i]); }
    else { const fscalar ax[3] = {1, 0, 0}; fx::angle_axis_to_matrix((fscalar)0.0, ax, &pb.rl_R[9 * i]); }
    fscalar cv[36]; for (int k = 0; k < 36; ++k) cv[k] = cov36[36 * i + k];
    if (!fx::spd_inverse_sqrt(cv, 6, &pb.rl_sqrt_inf[36 * i])) return OBVI_ERR_NUMERICAL;
  }
  pb.rl_huber = huber; pb.rl_active.assign(n, 1);
  return OBVI_OK;
}

int oracle_ba_set_shared_objects(oracle_handle* h, const uint8_t* is_shared, int32_t rank, int32_t world) {
  if (!h || world < 1 || rank < 0 || rank >= world) return OBVI_ERR_INVALID_ARGUMENT;
  if (is_shared) h->pb.is_shared.assign(is_shared, is_shared + h->pb.O); else h->pb.is_shared.clear();
  h->pb.rank = rank; h->pb.world = world;
  return OBVI_OK;
}
int oracle_ba_set_allreduce(oracle_handle* h, obvi_allreduce_fn fn, void* user) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  h->pb.allreduce = fn; h->pb.allreduce_user = user;
  return OBVI_OK;
}
int oracle_ba_set_active_mask(oracle_handle* h, int32_t type, const uint8_t* mask) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  OracleProblem& pb = h->pb;
  std::vector<uint8_t>* dst; int64_t n;
  switch (type) {
    case OBVI_FACTOR_REPROJECTION: dst = &pb.rp_active; n = pb.n_rp; break;
    case OBVI_FACTOR_BBOX: dst = &pb.bb_active; n = pb.n_bb; break;
    case OBVI_FACTOR_SHAPE_PRIOR: dst = &pb.sp_active; n = pb.n_sp; break;
    case OBVI_FACTOR_LTM_PRIOR: dst = &pb.lt_active; n = pb.n_lt; break;
    case OBVI_FACTOR_REL_POSE: dst = &pb.rl_active; n = pb.n_rl; break;
    default: return OBVI_ERR_INVALID_ARGUMENT;
  }
  if (mask) dst->assign(mask, mask + n); else dst->assign(n, 1);
  return OBVI_OK;
}

int64_t oracle_ba_num_factors(const oracle_handle* h, int32_t type) {
  const OracleProblem& pb = h->pb;
  switch (type) {
    case OBVI_FACTOR_REPROJECTION: return pb.n_rp; case OBVI_FACTOR_BBOX: return pb.n_bb;
    case OBVI_FACTOR_SHAPE_PRIOR: return pb.n_sp; case OBVI_FACTOR_LTM_PRIOR: return pb.n_lt;
    case OBVI_FACTOR_REL_POSE: return pb.n_rl; default: return -1;
  }
}
int64_t oracle_ba_num_residuals(const oracle_handle* h) {
  const OracleProblem& pb = h->pb;
  return 2 * pb.n_rp + 4 * pb.n_bb + 3 * pb.n_sp + pb.od * pb.n_lt + 6 * pb.n_rl;
}

// problem->Evaluate: every active residual block (constant blocks included -- Problem::Evaluate
// works on the full program), optional loss.  object_pose_graph_optimizer.h:682-693.
int oracle_ba_evaluate(oracle_handle* h, int32_t apply_loss, double* cost, double* residuals, double* block_sqnorm) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  const OracleProblem& pb = h->pb;
  real total = 0.0; int64_t ro = 0, bo = 0;
  for (const Family& fam : families(pb)) {
    for (int64_t i = 0; i < fam.n; ++i) {
      if (!(*fam.active)[i]) {
        if (residuals) for (int a = 0; a < fam.m; ++a) residuals[ro + a] = 0.0;
        if (block_sqnorm) block_sqnorm[bo] = 0.0;
      } else {
        FactorLin f; fam.lin(pb, i, false, &f);
        // k0/k1 used by robustify only for Jacobian scaling; residual-only here
        f.k0 = KIND_NONE; f.k1 = KIND_NONE;
        robustify(&f, fam.huber, apply_loss != 0);
        total += f.cost;
        if (residuals) for (int a = 0; a < fam.m; ++a) residuals[ro + a] = (double)f.r[a];
        if (block_sqnorm) block_sqnorm[bo] = (double)f.sqnorm;
      }
      ro += fam.m; ++bo;
    }
  }
  if (cost) *cost = (double)total;
  return OBVI_OK;
}

int oracle_ba_debug_linearize(oracle_handle* h, int32_t type, double* r, double* J0, double* J1) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  const OracleProblem& pb = h->pb;
  for (const Family& fam : families(pb)) {
    if (fam.type != type) continue;
    for (int64_t i = 0; i < fam.n; ++i) {
      FactorLin f; fam.lin(pb, i, true, &f);
      const int d0 = f.d0, d1 = f.d1;
      if (r) for (int k = 0; k < fam.m; ++k) r[fam.m * i + k] = (double)f.r[k];
      if (J0) for (int k = 0; k < fam.m * d0; ++k) J0[(int64_t)fam.m * d0 * i + k] = (double)f.J0[k];
      if (J1 && d1) for (int k = 0; k < fam.m * d1; ++k) J1[(int64_t)fam.m * d1 * i + k] = (double)f.J1[k];
    }
    return OBVI_OK;
  }
  return OBVI_ERR_INVALID_ARGUMENT;
}

// Dense copy of the reduced system for LM diagonal computed from `radius` with the Jacobi
// scaling of the current point (what iteration 1 of a solve would factorise).
int oracle_ba_debug_reduced_system(oracle_handle* h, double radius, double* lhs, double* rhs, int32_t m_cap, int32_t* m_out) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  OracleProblem& pb = h->pb;
  Reduced rd; build_reduced(pb, &rd);
  if (m_out) *m_out = (int32_t)rd.m;
  if (rd.m > m_cap) return OBVI_ERR_INVALID_ARGUMENT;
  Workspace ws; linearize(pb, rd, &ws); build_envelope(pb, rd, &ws);
  std::vector<real> lam_c(rd.m), lam_l(3 * pb.L, 0.0);
  auto lam = [&](double c) {
    const double s = 1.0 / (1.0 + std::sqrt(c));
    const double d = std::min(std::max(c * s * s, 1e-6), 1e32);
    return d / radius / (s * s);
  };
  for (int64_t i = 0; i < rd.m; ++i) lam_c[i] = lam((double)ws.colsq_c[i]);
  for (int64_t l = 0; l < pb.L; ++l) if (rd.point_var[l]) for (int k = 0; k < 3; ++k) lam_l[3 * l + k] = lam((double)ws.colsq_l[3 * l + k]);
  std::vector<real> Hinv;
  if (!assemble_schur(pb, rd, lam_c, lam_l, &ws, &Hinv)) return OBVI_ERR_NUMERICAL;
  for (int64_t i = 0; i < rd.m; ++i) {
    for (int64_t j = 0; j < rd.m; ++j) lhs[i * rd.m + j] = 0.0;
    rhs[i] = (double)ws.rhs[i];
  }
  for (int64_t i = 0; i < rd.m; ++i) for (int64_t j = ws.first[i]; j <= i; ++j) { lhs[i * rd.m + j] = (double)Sat(&ws, i, j); lhs[j * rd.m + i] = (double)Sat(&ws, i, j); }
  return OBVI_OK;
}

// Mirror of obvi_ba_debug_reduced_solve: the system of oracle_ba_debug_reduced_system (or the given one) as doubles, and the y of  lhs y = rhs  by a dense
// Cholesky in long double in canonical order -- the oracle has no tile grid: grid_row is the identity.  OBVI_ERR_NUMERICAL on a pivot that is not positive
// (a NaN included), with lhs and rhs written.
int oracle_ba_debug_reduced_solve(oracle_handle* h, double radius, const double* lhs_in, const double* rhs_in, double* lhs, double* rhs, double* y,
                                  int32_t* grid_row, int32_t m_cap, int32_t* m_out) {
  if (!h || !lhs || !rhs || !y || (lhs_in == nullptr) != (rhs_in == nullptr)) return OBVI_ERR_INVALID_ARGUMENT;
  int32_t m32 = 0;
  const int rc = oracle_ba_debug_reduced_system(h, radius, lhs, rhs, m_cap, &m32);
  if (m_out) *m_out = m32;
  if (rc != OBVI_OK) return rc;
  const int64_t m = m32;
  if (lhs_in) {
    for (int64_t i = 0; i < m; ++i) for (int64_t j = 0; j < i; ++j) {
      const double v = lhs_in[i * m + j], w = lhs_in[j * m + i];
      if (!(v == w) && !(v != v && w != w)) return OBVI_ERR_INVALID_ARGUMENT;
    }
    std::copy(lhs_in, lhs_in + m * m, lhs); std::copy(rhs_in, rhs_in + m, rhs);
  }
  for (int64_t i = 0; i < m; ++i) { y[i] = 0.0; if (grid_row) grid_row[i] = (int32_t)i; }
  std::vector<long double> L((size_t)(m * m), 0.0L), z((size_t)m);
  for (int64_t j = 0; j < m; ++j) {   // column by column
    long double p = lhs[j * m + j];
    for (int64_t k = 0; k < j; ++k) p -= L[j * m + k] * L[j * m + k];
    if (!(p > 0.0L)) return OBVI_ERR_NUMERICAL;
    const long double d = std::sqrt(p);
    L[j * m + j] = d;
    for (int64_t i = j + 1; i < m; ++i) {
      long double v = lhs[i * m + j];
      for (int64_t k = 0; k < j; ++k) v -= L[i * m + k] * L[j * m + k];
      L[i * m + j] = v / d;
    }
  }
  for (int64_t i = 0; i < m; ++i) { long double v = rhs[i]; for (int64_t k = 0; k < i; ++k) v -= L[i * m + k] * z[k]; z[i] = v / L[i * m + i]; }
  for (int64_t i = m - 1; i >= 0; --i) { long double v = z[i]; for (int64_t k = i + 1; k < m; ++k) v -= L[k * m + i] * z[k]; z[i] = v / L[i * m + i]; }
  bool finite = true;
  for (int64_t i = 0; i < m; ++i) { y[i] = (double)z[i]; finite = finite && std::isfinite(y[i]); }
  return finite ? OBVI_OK : OBVI_ERR_NUMERICAL;
}

// ceres::Covariance::Compute + GetCovarianceBlock for pairs of object blocks, as the long-term-map extraction asks for them
// (long_term_object_map_extraction.cpp:419-433, long_term_object_map_extraction.h:318-340, 499-513): blocks of (J^T J)^-1 over
// the variable parameter blocks at the current point, J robustified (Covariance::Options::apply_loss_function defaults to
// true), no damping.  [Ceres-doc: Covariance; the algorithm (SPARSE_QR / DENSE_SVD) does not change a full-rank result.]
// Restated through the Schur complement: the (objects, objects) part of (J^T J)^-1 is that part of S^-1.
// A constant or unused object has no covariance: its blocks are zero.  Rank deficiency -> OBVI_ERR_NUMERICAL.
int oracle_ba_object_covariances(oracle_handle* h, int64_t n_pairs, const uint32_t* obj_a, const uint32_t* obj_b, double* cov49) {
  if (!h || n_pairs < 0 || (n_pairs > 0 && (!obj_a || !obj_b || !cov49))) return OBVI_ERR_INVALID_ARGUMENT;
  OracleProblem& pb = h->pb;
  for (int64_t i = 0; i < n_pairs; ++i) if (obj_a[i] >= (uint64_t)pb.O || obj_b[i] >= (uint64_t)pb.O) return OBVI_ERR_INVALID_ARGUMENT;
  Reduced rd; build_reduced(pb, &rd);
  Workspace ws; linearize(pb, rd, &ws); build_envelope(pb, rd, &ws);
  std::vector<real> lam_c(rd.m, 0.0), lam_l(3 * pb.L, 0.0), Hinv;
  // a ParameterPrior's Jacobian is 1 / std_dev in its parameter's column (its residual is zero at mean = estimate): 1 / std_dev^2 on the diagonal
  for (size_t i = 0; i < pb.pp_kind.size(); ++i) {
    const double w = 1.0 / (pb.pp_std[i] * pb.pp_std[i]);
    const int64_t b = pb.pp_block[i];
    if (pb.pp_kind[i] == 0 && rd.pose_vid[b] >= 0) lam_c[pose_row(rd, b) + pb.pp_param[i]] += w;
    else if (pb.pp_kind[i] == 1 && rd.point_var[b]) lam_l[3 * b + pb.pp_param[i]] += w;
    else if (pb.pp_kind[i] == 2 && rd.obj_vid[b] >= 0) lam_c[obj_row(rd, b) + pb.pp_param[i]] += w;
  }
  if (!assemble_schur(pb, rd, lam_c, lam_l, &ws, &Hinv)) return OBVI_ERR_NUMERICAL;
  if (!skyline_factor(&ws, rd.m)) return OBVI_ERR_NUMERICAL;
  std::vector<int32_t> solved_for(pb.O, -1);           // object -> slot in `cols`
  std::vector<std::vector<real>> cols;                // 7 solution vectors per object that occurs as the second of a pair
  for (int64_t i = 0; i < n_pairs; ++i) {
    const int od = pb.od;
    double* out = cov49 + od * od * i;
    std::fill(out, out + od * od, 0.0);
    const uint32_t a = obj_a[i], b = obj_b[i];
    if (rd.obj_vid[a] < 0 || rd.obj_vid[b] < 0) continue;
    if (solved_for[b] < 0) {
      solved_for[b] = (int32_t)cols.size();
      for (int k = 0; k < od; ++k) {
        std::vector<real> x(rd.m, 0.0);
        x[obj_row(rd, b) + k] = 1.0;
        skyline_solve_inplace(&ws, rd.m, &x);
        if (!std::isfinite((double)x[obj_row(rd, b) + k])) return OBVI_ERR_NUMERICAL;
        cols.push_back(std::move(x));
      }
    }
    for (int r = 0; r < od; ++r) for (int k = 0; k < od; ++k) out[od * r + k] = (double)cols[solved_for[b] + k][obj_row(rd, a) + r];
  }
  return OBVI_OK;
}

// ParameterPrior factors for the covariance extraction (long_term_object_map_extraction.cpp:764-927) and the squared column norms of
// the robustified Jacobian they are chosen from (:585-608).
int oracle_ba_set_parameter_priors(oracle_handle* h, int64_t n, const uint8_t* kind, const uint32_t* block, const uint8_t* param, const double* mean, const double* std_dev) {
  if (!h || n < 0 || (n > 0 && (!kind || !block || !param || !mean || !std_dev))) return OBVI_ERR_INVALID_ARGUMENT;
  OracleProblem& pb = h->pb;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t cnt = kind[i] == 0 ? pb.P : kind[i] == 1 ? pb.L : kind[i] == 2 ? pb.O : -1;
    const int dim = kind[i] == 0 ? 6 : kind[i] == 1 ? 3 : h->pb.od;
    if (cnt < 0 || param[i] >= dim) return OBVI_ERR_INVALID_ARGUMENT;
    if ((int64_t)block[i] >= cnt) return OBVI_ERR_OUT_OF_RANGE;
    if (!(std_dev[i] > 0.0) || !std::isfinite(std_dev[i]) || !std::isfinite(mean[i])) return OBVI_ERR_NUMERICAL;
  }
  pb.pp_kind.assign(kind, kind + n); pb.pp_block.assign(block, block + n); pb.pp_param.assign(param, param + n); pb.pp_mean.assign(mean, mean + n); pb.pp_std.assign(std_dev, std_dev + n);
  return OBVI_OK;
}
int oracle_ba_column_sqnorms(oracle_handle* h, double* pose6, double* point3, double* object7) {
  if (!h) return OBVI_ERR_INVALID_ARGUMENT;
  OracleProblem& pb = h->pb;
  Reduced rd; build_reduced(pb, &rd);
  Workspace ws; linearize(pb, rd, &ws);
  if (pose6) for (int64_t p = 0; p < pb.P; ++p) for (int k = 0; k < 6; ++k) pose6[6 * p + k] = rd.pose_vid[p] >= 0 ? (double)ws.colsq_c[pose_row(rd, p) + k] : -1.0;
  if (point3) for (int64_t l = 0; l < pb.L; ++l) for (int k = 0; k < 3; ++k) point3[3 * l + k] = rd.point_var[l] ? (double)ws.colsq_l[3 * l + k] : -1.0;
  if (object7) for (int64_t o = 0; o < pb.O; ++o) for (int k = 0; k < pb.od; ++k) object7[pb.od * o + k] = rd.obj_vid[o] >= 0 ? (double)ws.colsq_c[obj_row(rd, o) + k] : -1.0;
  for (size_t i = 0; i < pb.pp_kind.size(); ++i) {
    const double w = 1.0 / (pb.pp_std[i] * pb.pp_std[i]);
    const int64_t b = pb.pp_block[i];
    if (pb.pp_kind[i] == 0 && pose6 && rd.pose_vid[b] >= 0) pose6[6 * b + pb.pp_param[i]] += w;
    else if (pb.pp_kind[i] == 1 && point3 && rd.point_var[b]) point3[3 * b + pb.pp_param[i]] += w;
    else if (pb.pp_kind[i] == 2 && object7 && rd.obj_vid[b] >= 0) object7[pb.od * b + pb.pp_param[i]] += w;
  }
  return OBVI_OK;
}

// ceres::Solve restated.  [Ceres-doc] throughout; see header comment.
int oracle_ba_solve(oracle_handle* h, const obvi_solver_params* prm, obvi_summary* sum) {
  if (!h || !prm || !sum) return OBVI_ERR_INVALID_ARGUMENT;
  OracleProblem& pb = h->pb;
  const double t_start = now_s();
  std::memset(sum, 0, sizeof(*sum));
  pb.iterations.clear();
  pb.visited.clear();
  double t_lin = 0, t_res = 0, t_solve = 0;

  Reduced rd; build_reduced(pb, &rd);
  // Objects shared across ranks (include/obvi_ba.h "multi-GPU"): every sum the decisions are taken from runs over all ranks through the
  // hook -- here on host buffers, stream = NULL --, the shared objects' own terms (their rows of the gradient, of x and of the step) are
  // counted by rank 0 only, and the reduced solve exchanges the Schur complement onto the shared rows (shared_tail_solve).  The collectives,
  // in this order on every rank: the fixed cost once; per linearisation the shared rows' column norms and gradient (14 per object), then
  // cost / |g|^2 / |x|^2 and one gradient-maximum slot per rank; per step the shared tail, then failure flag + model cost change, then
  // |step|^2 + trial cost + its failure flag.  (The device library packs the same exchanges into three collectives per step.)
  const bool dist = pb.allreduce != nullptr && rd.nOs > 0;
  bool hook_failed = false;
  auto xsum = [&](std::vector<double>* v) { if (dist && pb.allreduce(pb.allreduce_user, v->data(), (int64_t)v->size(), 0, nullptr)) hook_failed = true; };
  const bool owner = pb.rank == 0;
  auto counted_row = [&](int64_t row) { return !dist || row < rd.shared_row0 || owner; };
  if (dist) { std::vector<double> v(1, rd.fixed_cost); xsum(&v); rd.fixed_cost = v[0]; }
  sum->fixed_cost = rd.fixed_cost;
  sum->num_parameters_reduced = (int32_t)rd.num_params;
  sum->num_residuals_reduced = (int32_t)rd.num_residuals;
  sum->reduced_system_size = (int32_t)rd.m;

  auto finish = [&](int term, const char* msg) {
    sum->termination_type = term;
    std::snprintf(sum->message, sizeof(sum->message), "%s", msg);
    sum->num_iterations = (int32_t)pb.iterations.size();
    // Solver::Summary::final_cost = min over iterations (non-monotonic steps) [Ceres-doc solver.cc]
    sum->final_cost = sum->initial_cost;
    for (const auto& it : pb.iterations) sum->final_cost = std::min(sum->final_cost, it.cost);
    sum->is_solution_usable = (term == OBVI_CONVERGENCE || term == OBVI_NO_CONVERGENCE) ? 1 : 0;
    sum->total_time_in_seconds = now_s() - t_start;
    sum->jacobian_evaluation_time_in_seconds = t_lin;
    sum->residual_evaluation_time_in_seconds = t_res;
    sum->linear_solver_time_in_seconds = t_solve;
    return OBVI_OK;
  };

  if (rd.num_params == 0) {
    // Nothing to optimise: Ceres reports CONVERGENCE with initial == final == fixed cost.
    sum->initial_cost = rd.fixed_cost;
    obvi_iteration_summary it; std::memset(&it, 0, sizeof(it)); it.cost = rd.fixed_cost; it.step_is_valid = 1; it.step_is_successful = 1;
    pb.iterations.push_back(it);
    return finish(OBVI_CONVERGENCE, "Function tolerance reached. No non-constant parameter blocks found.");
  }

  Workspace ws;
  double tt = now_s();
  double x_cost = linearize(pb, rd, &ws);
  build_envelope(pb, rd, &ws);
  t_lin += now_s() - tt;
  // the shared rows' squared column norms and gradient, summed over the ranks (exchange (1) of the protocol)
  auto share_linearisation = [&]() {
    if (!dist) return;
    std::vector<double> v((size_t)(2 * (rd.m - rd.shared_row0)));
    for (int64_t i = rd.shared_row0; i < rd.m; ++i) { v[(size_t)(2 * (i - rd.shared_row0))] = (double)ws.colsq_c[i]; v[(size_t)(2 * (i - rd.shared_row0) + 1)] = (double)ws.g_c[i]; }
    xsum(&v);
    for (int64_t i = rd.shared_row0; i < rd.m; ++i) { ws.colsq_c[i] = v[(size_t)(2 * (i - rd.shared_row0))]; ws.g_c[i] = v[(size_t)(2 * (i - rd.shared_row0) + 1)]; }
  };
  share_linearisation();

  // Jacobi scaling, computed once at iteration 0: s_j = 1 / (1 + sqrt(colsq_j))
  std::vector<real> scale_c(rd.m), scale_l(3 * pb.L, 1.0);
  for (int64_t i = 0; i < rd.m; ++i) scale_c[i] = (real)1.0 / ((real)1.0 + std::sqrt(ws.colsq_c[i]));
  for (int64_t l = 0; l < pb.L; ++l) if (rd.point_var[l]) for (int k = 0; k < 3; ++k) scale_l[3 * l + k] = (real)1.0 / ((real)1.0 + std::sqrt(ws.colsq_l[3 * l + k]));

  // (with shared objects: this rank's part -- squares, to be summed over the ranks; the shared rows by rank 0 only)
  auto grad_norms_sq = [&](double* gmax, double* gsq) {
    real mx = 0.0, sq = 0.0;
    for (int64_t i = 0; i < rd.m; ++i) if (counted_row(i)) { mx = std::max(mx, std::fabs(ws.g_c[i])); sq += ws.g_c[i] * ws.g_c[i]; }
    for (int64_t l = 0; l < pb.L; ++l) if (rd.point_var[l]) for (int k = 0; k < 3; ++k) { const real g = ws.gl[3 * l + k]; mx = std::max(mx, std::fabs(g)); sq += g * g; }
    *gmax = (double)mx; *gsq = (double)sq;
  };
  auto x_norm_sq = [&]() {
    real sq = 0.0;
    for (int64_t p = 0; p < pb.P; ++p) if (rd.pose_vid[p] >= 0) for (int k = 0; k < 6; ++k) sq += pb.poses[6 * p + k] * pb.poses[6 * p + k];
    for (int64_t o = 0; o < pb.O; ++o) if (rd.obj_vid[o] >= 0 && counted_row(obj_row(rd, o))) for (int k = 0; k < pb.od; ++k) sq += pb.objects[pb.od * o + k] * pb.objects[pb.od * o + k];
    for (int64_t l = 0; l < pb.L; ++l) if (rd.point_var[l]) for (int k = 0; k < 3; ++k) sq += pb.points[3 * l + k] * pb.points[3 * l + k];
    return (double)sq;
  };
  // cost, gradient norms and |x| of the point just linearised, over all ranks (part of exchange (3) of the protocol)
  double lin_x_norm = 0.0;
  auto point_scalars = [&](double* cost, double* gmax, double* gnorm) {
    double mx, gsq;
    grad_norms_sq(&mx, &gsq);
    double xsq = x_norm_sq();
    if (dist) {
      std::vector<double> v((size_t)(3 + pb.world), 0.0);
      v[0] = *cost; v[1] = gsq; v[2] = xsq; v[(size_t)(3 + pb.rank)] = mx;
      xsum(&v);
      *cost = v[0]; gsq = v[1]; xsq = v[2];
      for (int r = 0; r < pb.world; ++r) mx = std::max(mx, v[(size_t)(3 + r)]);
    }
    *gmax = mx; *gnorm = std::sqrt(gsq); lin_x_norm = std::sqrt(xsq);
  };
  double gmax0 = 0.0, gnorm0 = 0.0;
  point_scalars(&x_cost, &gmax0, &gnorm0);

  // LevenbergMarquardtStrategy state
  double radius = prm->initial_trust_region_radius;
  const double max_radius = prm->max_trust_region_radius;
  double decrease_factor = 2.0;
  bool reuse_diagonal = false;
  std::vector<real> diag_c(rd.m), diag_l(3 * pb.L, 0.0);
  const real kMinDiag = 1e-6, kMaxDiag = 1e32;
  const double kMinRelDecrease = 1e-3, kMinRadius = 1e-32;
  const int kMaxInvalid = 5;
  // TrustRegionStepEvaluator state
  const int max_nonmono = prm->allow_non_monotonic_steps ? 5 : 0;
  double minimum_cost = x_cost, current_cost = x_cost, reference_cost = x_cost, candidate_cost_ev = x_cost;
  double acc_ref_model = 0.0, acc_cand_model = 0.0; int num_nonmono = 0;

  // best (minimum-cost) iterate: what Ceres writes back to the user's parameter blocks
  std::vector<double> best_poses, best_points, best_objects;
  copy_params(pb, &best_poses, &best_points, &best_objects);
  double best_cost = x_cost;
  bool failed = false;   // FAILURE: the solution is not usable and Ceres leaves the user's parameter blocks as they were at entry [Ceres-doc solver.cc]
  const std::vector<double> entry_poses = best_poses, entry_points = best_points, entry_objects = best_objects;

  sum->initial_cost = x_cost + rd.fixed_cost;
  obvi_iteration_summary it; std::memset(&it, 0, sizeof(it));
  it.iteration = 0; it.cost = x_cost + rd.fixed_cost; it.step_is_valid = 1; it.step_is_successful = 1;
  it.gradient_max_norm = gmax0; it.gradient_norm = gnorm0;
  it.trust_region_radius = radius;
  double x_norm = lin_x_norm;
  int num_invalid = 0;
  double iter_t0 = now_s();
  std::vector<real> y_c, Hll_inv, lam_c(rd.m), lam_l(3 * pb.L, 0.0), delta_l(3 * pb.L, 0.0);

  for (;;) {
    // FinalizeIterationAndCheckIfMinimizerCanContinue
    it.trust_region_radius = radius;
    it.iteration_time_in_seconds = now_s() - iter_t0;
    pb.iterations.push_back(it);
    if (it.step_is_successful) sum->num_successful_steps++; else sum->num_unsuccessful_steps++;   // iteration 0 counts as a successful step [Ceres-doc]
    if (it.iteration >= prm->max_num_iterations) { finish(OBVI_NO_CONVERGENCE, "Maximum number of iterations reached."); break; }
    if (it.step_is_successful && it.gradient_max_norm <= prm->gradient_tolerance) { finish(OBVI_CONVERGENCE, "Gradient tolerance reached."); break; }
    if (radius < kMinRadius) { finish(OBVI_CONVERGENCE, "Minimum trust region radius reached."); break; }

    iter_t0 = now_s();
    const double prev_gmax = it.gradient_max_norm, prev_gnorm = it.gradient_norm;
    const int next_iter = it.iteration + 1;
    std::memset(&it, 0, sizeof(it));
    it.iteration = next_iter;

    // ---- ComputeTrustRegionStep (LevenbergMarquardtStrategy::ComputeStep) ----
    tt = now_s();
    if (!reuse_diagonal) {
      for (int64_t i = 0; i < rd.m; ++i) diag_c[i] = std::min(std::max(ws.colsq_c[i] * scale_c[i] * scale_c[i], kMinDiag), kMaxDiag);
      for (int64_t l = 0; l < pb.L; ++l) if (rd.point_var[l]) for (int k = 0; k < 3; ++k)
        diag_l[3 * l + k] = std::min(std::max(ws.colsq_l[3 * l + k] * scale_l[3 * l + k] * scale_l[3 * l + k], kMinDiag), kMaxDiag);
    }
    // scaled system (J_s^T J_s + D^2) y_s = J_s^T r, D^2 = diag/radius; in unscaled variables
    // delta = s .* y_s this is (J^T J + D^2/s^2) delta = J^T r.
    for (int64_t i = 0; i < rd.m; ++i) lam_c[i] = counted_row(i) ? diag_c[i] / radius / (scale_c[i] * scale_c[i]) : (real)0.0;   // (a shared row's damping enters the summed tail once)
    for (int64_t l = 0; l < pb.L; ++l) if (rd.point_var[l]) for (int k = 0; k < 3; ++k)
      lam_l[3 * l + k] = diag_l[3 * l + k] / radius / (scale_l[3 * l + k] * scale_l[3 * l + k]);
    const double t_asm = now_s();
    // (the shared rows' gradient is the sum over the ranks on every rank: it enters the summed tail once, through rank 0)
    std::vector<real> g_shared;
    if (dist && !owner) { g_shared.assign(ws.g_c.begin() + rd.shared_row0, ws.g_c.end()); std::fill(ws.g_c.begin() + rd.shared_row0, ws.g_c.end(), (real)0.0); }
    bool ok = assemble_schur(pb, rd, lam_c, lam_l, &ws, &Hll_inv);
    if (dist && !owner) std::copy(g_shared.begin(), g_shared.end(), ws.g_c.begin() + rd.shared_row0);
    const double t_fac = now_s();
    if (dist) { if (!shared_tail_solve(pb, &ws, rd.m, rd.shared_row0, &y_c)) ok = false; }   // (every rank takes part in the exchange, whatever its own assembly said)
    else if (ok) ok = skyline_cholesky_solve(&ws, rd.m, &y_c);
    if (!ok) y_c.assign((size_t)rd.m, 0.0);
    if (std::getenv("OBVI_ORACLE_TIMING")) std::fprintf(stderr, "oracle step: assemble_schur %.3f s, skyline factor + solve %.3f s (envelope %.1f M entries)\n", t_fac - t_asm, now_s() - t_fac, 1e-6 * (double)ws.S.size());
    // back-substitution  y_l = Hll^-1 (g_l - W^T y_c)
    if (ok) {
      for (int64_t l = 0; l < pb.L; ++l) {
        if (!rd.point_var[l]) continue;
        real b[3] = {ws.gl[3 * l], ws.gl[3 * l + 1], ws.gl[3 * l + 2]};
        for (int64_t idx : ws.point_obs[l]) {
          const FactorLin& f = ws.lin[idx];
          if (rd.pose_vid[f.i0] < 0) continue;
          const int64_t ra = pose_row(rd, f.i0);
          for (int k = 0; k < 3; ++k) {
            real acc = 0.0;  // (W^T y)_k = sum_x W[x][k] y[x], W = Jp^T Jl
            for (int x = 0; x < 6; ++x) acc += ((real)f.J0[x] * f.J1[k] + (real)f.J0[6 + x] * f.J1[3 + k]) * y_c[ra + x];
            b[k] -= acc;
          }
        }
        const real* Hi = &Hll_inv[9 * l];
        for (int k = 0; k < 3; ++k) delta_l[3 * l + k] = -(Hi[3 * k] * b[0] + Hi[3 * k + 1] * b[1] + Hi[3 * k + 2] * b[2]);
      }
    }
    reuse_diagonal = true;
    t_solve += now_s() - tt;
    bool finite = ok;
    if (ok) {
      for (int64_t i = 0; i < rd.m && finite; ++i) finite = std::isfinite((double)y_c[i]);
      for (int64_t l = 0; l < pb.L && finite; ++l) if (rd.point_var[l]) for (int k = 0; k < 3; ++k) finite = finite && std::isfinite((double)delta_l[3 * l + k]);
    }
    // model_cost_change = -(J delta)^T (r + J delta / 2)
    real model_acc = 0.0;
    if (finite) {
      for (const FactorLin& f : ws.lin) {
        real Jd[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const BlockKind ks[2] = {f.k0, f.k1}; const int64_t is[2] = {f.i0, f.i1}; const fscalar* Js[2] = {f.J0, f.J1};
        for (int b = 0; b < 2; ++b) {
          if (!is_var(pb, rd, ks[b], is[b])) continue;
          const int d = b == 0 ? f.d0 : f.d1;
          for (int k = 0; k < d; ++k) {
            const real dk = (ks[b] == KIND_POINT) ? delta_l[3 * is[b] + k] : -y_c[reduced_row(rd, ks[b], is[b]) + k];
            for (int a = 0; a < f.m; ++a) Jd[a] += Js[b][d * a + k] * dk;
          }
        }
        for (int a = 0; a < f.m; ++a) model_acc -= Jd[a] * (f.r[a] + (real)0.5 * Jd[a]);
      }
    }
    double model_cost_change = (double)model_acc;
    if (dist) {   // one decision for all ranks
      std::vector<double> v = {finite ? 0.0 : 1.0, finite ? model_cost_change : 0.0};
      xsum(&v);
      finite = v[0] == 0.0 && !hook_failed; model_cost_change = v[1];
    }
    it.step_is_valid = (finite && model_cost_change > 0.0) ? 1 : 0;
    if (!it.step_is_valid) {
      // HandleInvalidStep
      if (++num_invalid >= kMaxInvalid) {
        // the record of the step that ends the solve: not counted, but a record of an invalid step like the others (the current cost -- final_cost is the
        // minimum over the records --, the gradient norms and the radius it was tried with)
        it.cost = x_cost + rd.fixed_cost; it.gradient_max_norm = prev_gmax; it.gradient_norm = prev_gnorm; it.trust_region_radius = radius;
        pb.iterations.push_back(it);
        finish(OBVI_FAILURE, "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps");
        failed = true;
        break;
      }
      radius = radius / decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true;  // StepIsInvalid
      it.cost = x_cost + rd.fixed_cost; it.cost_change = 0.0; it.gradient_max_norm = prev_gmax; it.gradient_norm = prev_gnorm;
      it.step_norm = 0.0; it.relative_decrease = 0.0; it.step_is_successful = 0;
      continue;
    }
    num_invalid = 0;

    // ---- candidate point ----
    std::vector<double> old_poses = pb.poses, old_points = pb.points, old_objects = pb.objects;
    real step_sq = 0.0;   // (the parameter blocks are fp64 in every build: the step is rounded once, where it is added)
    for (int64_t p = 0; p < pb.P; ++p) if (rd.pose_vid[p] >= 0) for (int k = 0; k < 6; ++k) { const real d = -y_c[pose_row(rd, p) + k]; pb.poses[6 * p + k] = (double)(pb.poses[6 * p + k] + d); step_sq += d * d; }
    for (int64_t o = 0; o < pb.O; ++o) if (rd.obj_vid[o] >= 0) for (int k = 0; k < pb.od; ++k) { const real d = -y_c[obj_row(rd, o) + k]; pb.objects[pb.od * o + k] = (double)(pb.objects[pb.od * o + k] + d); if (counted_row(obj_row(rd, o))) step_sq += d * d; }
    for (int64_t l = 0; l < pb.L; ++l) if (rd.point_var[l]) for (int k = 0; k < 3; ++k) { const real d = delta_l[3 * l + k]; pb.points[3 * l + k] = (double)(pb.points[3 * l + k] + d); step_sq += d * d; }
    if (pb.keep_visited) { pb.visited.push_back(pb.poses); pb.visited.back().insert(pb.visited.back().end(), pb.points.begin(), pb.points.end()); }
    tt = now_s();
    double cand_cost = reduced_cost(pb, rd);
    t_res += now_s() - tt;
    if (dist) {
      const bool bad = !std::isfinite(cand_cost);
      std::vector<double> v = {(double)step_sq, bad ? 0.0 : cand_cost, bad ? 1.0 : 0.0};
      xsum(&v);
      step_sq = v[0]; cand_cost = v[2] == 0.0 ? v[1] : std::numeric_limits<double>::infinity();
    }
    if (!std::isfinite(cand_cost)) cand_cost = std::numeric_limits<double>::max();

    auto revert = [&]() { pb.poses = old_poses; pb.points = old_points; pb.objects = old_objects; };
    // ParameterToleranceReached
    it.step_norm = (double)std::sqrt(step_sq);
    if (it.step_norm <= prm->parameter_tolerance * (x_norm + prm->parameter_tolerance)) {
      revert();
      finish(OBVI_CONVERGENCE, "Parameter tolerance reached.");
      break;
    }
    // FunctionToleranceReached
    it.cost_change = x_cost - cand_cost;
    if (std::fabs(it.cost_change) <= prm->function_tolerance * x_cost) {
      revert();
      finish(OBVI_CONVERGENCE, "Function tolerance reached.");
      break;
    }
    // IsStepSuccessful: TrustRegionStepEvaluator::StepQuality
    {
      const double rel = (current_cost - cand_cost) / model_cost_change;
      const double hist = (reference_cost - cand_cost) / (acc_ref_model + model_cost_change);
      it.relative_decrease = (cand_cost >= std::numeric_limits<double>::max()) ? -std::numeric_limits<double>::max() : std::max(rel, hist);
    }
    if (it.relative_decrease > kMinRelDecrease) {
      // HandleSuccessfulStep
      tt = now_s();
      x_cost = linearize(pb, rd, &ws);
      t_lin += now_s() - tt;
      share_linearisation();
      point_scalars(&x_cost, &it.gradient_max_norm, &it.gradient_norm);
      x_norm = lin_x_norm;
      it.cost = x_cost + rd.fixed_cost;
      it.step_is_successful = 1;
      // strategy->StepAccepted
      radius = radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * it.relative_decrease - 1.0, 3));
      radius = std::min(max_radius, radius);
      decrease_factor = 2.0; reuse_diagonal = false;
      // step_evaluator->StepAccepted
      current_cost = cand_cost; acc_cand_model += model_cost_change; acc_ref_model += model_cost_change;
      if (cand_cost < minimum_cost) { minimum_cost = cand_cost; num_nonmono = 0; candidate_cost_ev = cand_cost; acc_cand_model = 0.0; }
      else { ++num_nonmono; if (cand_cost > candidate_cost_ev) { candidate_cost_ev = cand_cost; acc_cand_model = 0.0; } }
      if (num_nonmono == max_nonmono) { reference_cost = candidate_cost_ev; acc_ref_model = acc_cand_model; }
      if (x_cost < best_cost) { best_cost = x_cost; copy_params(pb, &best_poses, &best_points, &best_objects); }
    } else {
      revert();
      it.step_is_successful = 0;
      it.cost = cand_cost + rd.fixed_cost;   // HandleUnsuccessfulStep records the CANDIDATE's cost [Ceres-doc trust_region_minimizer.cc]
      it.gradient_max_norm = prev_gmax; it.gradient_norm = prev_gnorm;
      radius = radius / decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true;  // StepRejected
    }
  }
  if (hook_failed) { pb.poses = entry_poses; pb.points = entry_points; pb.objects = entry_objects; pb.err = "all-reduce hook failed"; return OBVI_ERR_HIP; }
  // write back the minimum-cost iterate (the entry state after a FAILURE)
  if (failed) { pb.poses = entry_poses; pb.points = entry_points; pb.objects = entry_objects; }
  else { pb.poses = best_poses; pb.points = best_points; pb.objects = best_objects; }
  return OBVI_OK;
}

int oracle_ba_get_iterations(const oracle_handle* h, obvi_iteration_summary* out, int32_t cap) {
  const int n = std::min<int>(cap, (int)h->pb.iterations.size());
  for (int i = 0; i < n; ++i) out[i] = h->pb.iterations[i];
  return n;
}

// offline_problem_runner.h:769-800: per factor type, order blocks by un-robustified |r|^2
// descending in a std::map keyed by the value (equal values collapse into one entry), take the
// first floor(size * fraction) entries.
// offline_problem_runner.h:769-800 on (value, index) pairs: std::map<double, id, greater> -- later insertions with an equal key overwrite; the
// map is filled by iterating an unordered_map, so which duplicate survives is unspecified.  We keep the highest index, and count
// distinct values like the map's size() does.  Clears mask[index] of the first floor(size * fraction) entries; returns how many.
static size_t map_rule(std::vector<std::pair<double, int64_t>>* values, double fraction, uint8_t* mask) {
  std::vector<std::pair<double, int64_t>>& v = *values;
  std::sort(v.begin(), v.end(), [](const std::pair<double, int64_t>& a, const std::pair<double, int64_t>& b) {
    return a.first > b.first || (a.first == b.first && a.second > b.second); });
  std::vector<std::pair<double, int64_t>> uniq;
  for (const auto& e : v) if (uniq.empty() || uniq.back().first != e.first) uniq.push_back(e);
  const size_t n_out = (size_t)(uniq.size() * fraction);
  for (size_t k = 0; k < n_out; ++k) mask[uniq[k].second] = 0;
  return n_out;
}
int oracle_ba_debug_select(oracle_handle* h, int64_t n, const double* sq, const uint8_t* active, double fraction, uint8_t* mask_out, int64_t* num_excluded) {
  if (!h || n < 0 || (n > 0 && (!sq || !mask_out))) return OBVI_ERR_INVALID_ARGUMENT;
  std::vector<std::pair<double, int64_t>> v;
  for (int64_t i = 0; i < n; ++i) { mask_out[i] = active ? (active[i] != 0) : 1; if (mask_out[i]) v.push_back({sq[i], i}); }
  const size_t n_out = map_rule(&v, fraction, mask_out);
  if (num_excluded) *num_excluded = (int64_t)n_out;
  return OBVI_OK;
}
int oracle_ba_select_outliers(oracle_handle* h, int32_t type, double fraction, uint8_t* mask_out, int64_t* num_excluded) {
  if (!h || !mask_out) return OBVI_ERR_INVALID_ARGUMENT;
  const OracleProblem& pb = h->pb;
  for (const Family& fam : families(pb)) {
    if (fam.type != type) continue;
    std::vector<std::pair<double, int64_t>> v;
    for (int64_t i = 0; i < fam.n; ++i) {
      mask_out[i] = (*fam.active)[i];
      if (!(*fam.active)[i]) continue;
      FactorLin f; fam.lin(pb, i, false, &f);
      double s = 0.0; for (int a = 0; a < fam.m; ++a) s += f.r[a] * f.r[a];
      v.push_back({s, i});
    }
    const size_t n_out = map_rule(&v, fraction, mask_out);
    if (num_excluded) *num_excluded = (int64_t)n_out;
    return OBVI_OK;
  }
  return OBVI_ERR_INVALID_ARGUMENT;
}

// Test hook (tests/lm_cases.py: the depths at every point a solve evaluates, of which the solve itself hands back only the best): with `on`, a solve keeps
// the poses and points of each candidate it forms, in the order of its valid steps; get_visited returns their number and, for 0 <= k < that, copies the k-th.
int oracle_ba_debug_keep_visited(oracle_handle* h, int32_t on) { h->pb.keep_visited = on != 0; if (!on) h->pb.visited.clear(); return OBVI_OK; }
int oracle_ba_debug_get_visited(oracle_handle* h, int32_t k, double* poses, double* points) {
  const int32_t n = (int32_t)h->pb.visited.size();
  if (k >= 0 && k < n && poses && points) {
    const std::vector<double>& v = h->pb.visited[(size_t)k];
    std::memcpy(poses, v.data(), sizeof(double) * 6 * h->pb.P); std::memcpy(points, v.data() + 6 * h->pb.P, sizeof(double) * 3 * h->pb.L);
  }
  return n;
}

int oracle_ba_snapshot(oracle_handle* h) { h->pb.snap_poses = h->pb.poses; h->pb.snap_points = h->pb.points; h->pb.snap_objects = h->pb.objects; return OBVI_OK; }
int oracle_ba_restore(oracle_handle* h) {
  if ((int64_t)h->pb.snap_poses.size() != 6 * h->pb.P) return OBVI_ERR_NOT_READY;
  h->pb.poses = h->pb.snap_poses; h->pb.points = h->pb.snap_points; h->pb.objects = h->pb.snap_objects; return OBVI_OK;
}
int oracle_ba_get_poses(oracle_handle* h, double* out) { std::memcpy(out, h->pb.poses.data(), sizeof(double) * h->pb.poses.size()); return OBVI_OK; }
int oracle_ba_get_points(oracle_handle* h, double* out) { std::memcpy(out, h->pb.points.data(), sizeof(double) * h->pb.points.size()); return OBVI_OK; }
int oracle_ba_get_objects(oracle_handle* h, double* out) { std::memcpy(out, h->pb.objects.data(), sizeof(double) * h->pb.objects.size()); return OBVI_OK; }
int oracle_ba_get_state(oracle_handle* h, double* poses, double* points, double* objects) {
  if (poses) oracle_ba_get_poses(h, poses);
  if (points) oracle_ba_get_points(h, points);
  if (objects) oracle_ba_get_objects(h, objects);
  return OBVI_OK;
}
int oracle_ba_update_points(oracle_handle* h, int64_t n, const double* xyz) {
  if (n != h->pb.L) return OBVI_ERR_INVALID_ARGUMENT;
  h->pb.points.assign(xyz, xyz + 3 * n); return OBVI_OK;
}

// values only, constness untouched (tests/lockstep_shim.cpp hands the oracle the other backend's result after a solve)
int oracle_ba_update_poses(oracle_handle* h, int64_t n, const double* v) {
  if (n != h->pb.P) return OBVI_ERR_INVALID_ARGUMENT;
  h->pb.poses.assign(v, v + 6 * n); return OBVI_OK;
}
int oracle_ba_update_objects(oracle_handle* h, int64_t n, const double* v) {
  if (n != h->pb.O) return OBVI_ERR_INVALID_ARGUMENT;
  h->pb.objects.assign(v, v + h->pb.od * n); return OBVI_OK;
}

// include/obvi_ba.h obvi_ba_update_state / obvi_ba_prepare as the drivers built against this library see them (tests/oracle_abi_shim.h): values only;
// the restatement has no symbolic phase to run ahead (Ceres orders and analyses inside Solve())
int oracle_ba_update_state(oracle_handle* h, const double* poses, const double* points, const double* objects) {
  if (poses) h->pb.poses.assign(poses, poses + 6 * h->pb.P);
  if (points) h->pb.points.assign(points, points + 3 * h->pb.L);
  if (objects) h->pb.objects.assign(objects, objects + h->pb.od * h->pb.O);
  return OBVI_OK;
}
int oracle_ba_prepare(oracle_handle*) { return OBVI_OK; }

// ---- factor-level entry points for golden-vector tests ---------------------------------
void oracle_reproj(const double* pose6, const double* point3, const double* K4, const double* ext7, const double* pixel2,
                   double sigma, double* r2, double* Jpose, double* Jpoint) {
  CameraConst cam; make_camera_const(K4, ext7, &cam);
  typedef Dual<9> D; D dp[6], dx[3], dr[2];
  for (int k = 0; k < 6; ++k) dp[k] = D::var(pose6[k], k);
  for (int k = 0; k < 3; ++k) dx[k] = D::var(point3[k], 6 + k);
  reprojection_residual<D>(dp, dx, cam, pixel2, sigma, dr);
  for (int a = 0; a < 2; ++a) {
    r2[a] = dr[a].v;
    if (Jpose) for (int k = 0; k < 6; ++k) Jpose[6 * a + k] = dr[a].d[k];
    if (Jpoint) for (int k = 0; k < 3; ++k) Jpoint[3 * a + k] = dr[a].d[6 + k];
  }
}
// the analytic-Jacobian functor (a2), same signature
void oracle_reproj_analytic(const double* pose6, const double* point3, const double* K4, const double* ext7, const double* pixel2,
                            double sigma, double* r2, double* Jpose, double* Jpoint) {
  CameraConst cam; make_camera_const(K4, ext7, &cam);
  typedef Dual<9> D; D dp[6], dx[3], dr[2];
  for (int k = 0; k < 6; ++k) dp[k] = D::var(pose6[k], k);
  for (int k = 0; k < 3; ++k) dx[k] = D::var(point3[k], 6 + k);
  reprojection_residual_analytic<D>(dp, dx, cam, pixel2, sigma, dr);
  for (int a = 0; a < 2; ++a) {
    r2[a] = dr[a].v;
    if (Jpose) for (int k = 0; k < 6; ++k) Jpose[6 * a + k] = dr[a].d[k];
    if (Jpoint) for (int k = 0; k < 3; ++k) Jpoint[3 * a + k] = dr[a].d[6 + k];
  }
}
int oracle_ellipsoid_corners(const double* ell7, const double* pose6, const double* K4, const double* ext7, double* corners4) {
  CameraConst cam; make_camera_const(K4, ext7, &cam);
  return ellipsoid_corners_rectified<double>(ell7, pose6, cam, corners4) ? 1 : 0;
}
int oracle_ellipsoid_corners9(const double* ell9, const double* pose6, const double* K4, const double* ext7, double* corners4) {   // the 9-parameter block
  CameraConst cam; make_camera_const(K4, ext7, &cam);
  return ellipsoid_corners_rectified<double, 9>(ell9, pose6, cam, corners4) ? 1 : 0;
}
int oracle_spd_inverse_sqrt(const double* cov, int n, double* out) { return spd_inverse_sqrt(cov, n, out) ? 1 : 0; }
void oracle_huber(double s, double a, double* rho3) { huber(s, a, rho3); }


// ---- visual-feature front-end gating (include/obvi_frontend.h; oracle_frontend.h restates the arithmetic) -------------------------
static int oracle_epipolar(int32_t n_cams, const double* K4, const double* ext7, int64_t n_poses, const double* pose6, int64_t n_cand, const uint32_t* cand_pose,
                           const uint16_t* cand_cam, const double* cand_pixel, const uint64_t* ref_ptr, const uint32_t* ref_pose, const uint16_t* ref_cam,
                           const double* ref_pixel, const uint32_t* ref_frame, const uint8_t* ref_skip, const obvi_epipolar_params* prm, uint32_t* votes,
                           uint32_t* voters, uint8_t* inlier, double* err) {
  if (n_cand < 0 || n_cams < 0 || n_poses < 0) return OBVI_ERR_INVALID_ARGUMENT;
  std::vector<oracle::Affine> cam_to_robot((size_t)n_cams), robot_to_world((size_t)n_poses);
  for (int c = 0; c < n_cams; ++c) cam_to_robot[c] = oracle::affine_from_quat_translation(ext7 + 7 * c, ext7 + 7 * c + 4);
  for (int64_t p = 0; p < n_poses; ++p) robot_to_world[p] = oracle::affine_from_pose6(pose6 + 6 * p);
  for (int64_t i = 0; i < n_cand; ++i) {
    const int c2 = cand_cam ? cand_cam[i] : 0;
    if (cand_pose[i] >= (uint64_t)n_poses || c2 >= n_cams) return OBVI_ERR_OUT_OF_RANGE;
    uint64_t v = 0, n = 0;
    for (uint64_t k = ref_ptr[i]; k < ref_ptr[i + 1]; ++k) {
      const int c1 = ref_cam ? ref_cam[k] : 0;
      if (ref_pose[k] >= (uint64_t)n_poses || c1 >= n_cams) return OBVI_ERR_OUT_OF_RANGE;
      if (!err) {
        if (prm->early_votes_return && k > ref_ptr[i] && ref_frame[k] != ref_frame[ref_ptr[i]]) break;   // :596-599
        if (ref_skip && ref_skip[k]) continue;                                                            // :551-553
      }
      double e[2];
      oracle::epipolar_error_vec(K4 + 4 * c1, K4 + 4 * c2, cam_to_robot[c1], cam_to_robot[c2], ref_pixel + 2 * k, cand_pixel + 2 * i, robot_to_world[ref_pose[k]],
                                 robot_to_world[cand_pose[i]], e);
      if (err) { err[2 * k] = e[0]; err[2 * k + 1] = e[1]; continue; }
      if (std::sqrt(e[0] * e[0] + e[1] * e[1]) < prm->inlier_epipolar_err_thresh) ++v;
      ++n;
    }
    if (err) continue;
    if (votes) votes[i] = (uint32_t)v;
    if (voters) voters[i] = (uint32_t)n;
    if (inlier) inlier[i] = (((double)v) / n) > prm->inlier_majority_percentage ? 1 : 0;
  }
  return OBVI_OK;
}
int oracle_frontend_epipolar_votes(oracle_handle*, int32_t n_cams, const double* K4, const double* ext7, int64_t n_poses, const double* pose6, int64_t n_cand,
                                   const uint32_t* cand_pose, const uint16_t* cand_cam, const double* cand_pixel, const uint64_t* ref_ptr, const uint32_t* ref_pose,
                                   const uint16_t* ref_cam, const double* ref_pixel, const uint32_t* ref_frame, const uint8_t* ref_skip, const obvi_epipolar_params* prm,
                                   uint32_t* votes, uint32_t* voters, uint8_t* inlier) {
  if (!prm) return OBVI_ERR_INVALID_ARGUMENT;
  return oracle_epipolar(n_cams, K4, ext7, n_poses, pose6, n_cand, cand_pose, cand_cam, cand_pixel, ref_ptr, ref_pose, ref_cam, ref_pixel, ref_frame, ref_skip, prm, votes, voters, inlier, nullptr);
}
int oracle_frontend_epipolar_errors(oracle_handle*, int32_t n_cams, const double* K4, const double* ext7, int64_t n_poses, const double* pose6, int64_t n_cand,
                                    const uint32_t* cand_pose, const uint16_t* cand_cam, const double* cand_pixel, const uint64_t* ref_ptr, const uint32_t* ref_pose,
                                    const uint16_t* ref_cam, const double* ref_pixel, double* err) {
  if (!err) return OBVI_ERR_INVALID_ARGUMENT;
  return oracle_epipolar(n_cams, K4, ext7, n_poses, pose6, n_cand, cand_pose, cand_cam, cand_pixel, ref_ptr, ref_pose, ref_cam, ref_pixel, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, err);
}
int oracle_frontend_parallax(oracle_handle*, int64_t n_feat, const uint64_t* frame_ptr, const uint8_t* has_pose, const double* pose6, const uint64_t* obs_ptr,
                             const double* pixel, const obvi_parallax_params* prm, uint8_t* satisfied) {
  if (n_feat < 0 || !prm) return OBVI_ERR_INVALID_ARGUMENT;
  for (int64_t f = 0; f < n_feat; ++f) {
    const uint64_t k0 = frame_ptr[f], k1 = frame_ptr[f + 1];
    bool found = false;
    if (k1 - k0 > 1)
      for (uint64_t i = k0; i + 1 < k1 && !found; ++i)
        for (uint64_t j = i + 1; j < k1 && !found; ++j) {
          bool pixel_req = false, pose_req = false;
          if (prm->enforce_min_robot_pose_parallax_requirement && has_pose[i] && has_pose[j]) {
            double tn, ang;
            oracle::relative_motion(pose6 + 6 * i, pose6 + 6 * j, &tn, &ang);
            if (tn >= prm->min_visual_feature_parallax_robot_transl_requirement || ang >= prm->min_visual_feature_parallax_robot_orient_requirement) pose_req = true;
          }
          if (prm->enforce_min_pixel_parallax_requirement)
            for (uint64_t a = obs_ptr[i]; a < obs_ptr[i + 1]; ++a)
              for (uint64_t c = obs_ptr[j]; c < obs_ptr[j + 1]; ++c) {
                const double dx = pixel[2 * a] - pixel[2 * c], dy = pixel[2 * a + 1] - pixel[2 * c + 1];
                if (std::sqrt(dx * dx + dy * dy) >= prm->min_visual_feature_parallax_pixel_requirement) pixel_req = true;
              }
          bool req;
          if (prm->enforce_min_robot_pose_parallax_requirement && !prm->enforce_min_pixel_parallax_requirement) req = pose_req;
          else if (!prm->enforce_min_robot_pose_parallax_requirement && prm->enforce_min_pixel_parallax_requirement) req = pixel_req;
          else if (prm->enforce_min_robot_pose_parallax_requirement && prm->enforce_min_pixel_parallax_requirement) req = pose_req && pixel_req;
          else req = true;
          if (req) found = true;
        }
    satisfied[f] = found ? 1 : 0;
  }
  return OBVI_OK;
}

}

