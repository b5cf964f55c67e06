// host_util.h -- small host helpers of libobvi_ba: device buffers, error plumbing, and the
// symmetric inverse square root the factor constructors of the reference apply to their
// covariances (`cov.inverse().sqrt()`: bounding_box_factor.cpp:31-33, shape_prior_factor.cpp:11,
// independent_object_map_factor.cpp:11, relative_pose_factor.cpp:13).
#ifndef OBVI_HOST_UTIL_H_
#define OBVI_HOST_UTIL_H_

#include <hip/hip_runtime.h>
#if defined(__linux__)
#include <pthread.h>
#include <sched.h>
#endif

#include <algorithm>
#include <limits>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace obvi {

struct HipError { hipError_t code; const char* what; const char* file; int line; };

#define OBVI_HIP(expr)                                                         \
  do {                                                                         \
    hipError_t e__ = (expr);                                                   \
    if (e__ != hipSuccess) throw ::obvi::HipError{e__, #expr, __FILE__, __LINE__}; \
  } while (0)

// Host -> device copies of an upload go through a pinned arena of the handle: the bytes are copied into it and the transfer is
// enqueued from there, so that it neither waits on a pageable staging copy inside the runtime (15-30 us per call, and an upload is
// some forty of them) nor needs the stream synchronised before the caller's buffer or a local vector may go away.  The arena is
// rewound whenever the stream is known to be idle (sync()); a copy that does not fit, or is too long to be worth a second pass
// over its bytes, goes the plain way and marks the arena `spilled`: the function that issued it must synchronise before it returns.
struct StagingArena {
  char* base = nullptr;
  size_t cap = 0, used = 0;
  bool spilled = false;
  void* take(size_t bytes) {
    const size_t at = (used + 255) & ~(size_t)255;
    if (base == nullptr || at + bytes > cap) return nullptr;
    used = at + bytes;
    return base + at;
  }
  void rewind() { used = 0; spilled = false; }
};
inline thread_local StagingArena* tl_staging = nullptr;   // the arena of the handle whose API call runs on this thread
constexpr size_t kStagedCopyMaxBytes = (size_t)4 << 20;

inline void h2d_async(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (bytes == 0) return;
  StagingArena* a = tl_staging;
  if (a != nullptr && bytes <= kStagedCopyMaxBytes) {
    if (void* p = a->take(bytes)) {
      std::memcpy(p, src, bytes);
      OBVI_HIP(hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s));
      return;
    }
  }
  if (a != nullptr) a->spilled = true;
  OBVI_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
}

template <class T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() { if (p_) { (void)hipFree(p_); p_ = nullptr; } n_ = 0; cap_ = 0; }
  // grow-only allocation; contents are undefined after a growing resize
  void resize(size_t n) {
    if (n > cap_) {
      if (p_) { (void)hipFree(p_); p_ = nullptr; }
      size_t c = n + n / 8 + 16;
      OBVI_HIP(hipMalloc(reinterpret_cast<void**>(&p_), c * sizeof(T)));
      cap_ = c;
    }
    n_ = n;
  }
  void upload(const T* h, size_t n, hipStream_t s) {
    resize(n);
    h2d_async(p_, h, n * sizeof(T), s);
  }
  void upload(const std::vector<T>& h, hipStream_t s) { upload(h.data(), h.size(), s); }
  // Upload without the host-side copy: stage_begin(n) sizes the buffer and hands out n elements of pinned memory from the running call's
  // arena to be filled in place (nullptr when the arena has no room: fill a vector and upload() that), stage_commit starts the copy.
  T* stage_begin(size_t n) {
    resize(n);
    StagingArena* a = tl_staging;
    if (n == 0 || a == nullptr || n * sizeof(T) > kStagedCopyMaxBytes) return nullptr;
    return static_cast<T*>(a->take(n * sizeof(T)));
  }
  void stage_commit(const T* staged, size_t n, hipStream_t s) { if (n) OBVI_HIP(hipMemcpyAsync(p_, staged, n * sizeof(T), hipMemcpyHostToDevice, s)); }
  void download(T* h, size_t n, hipStream_t s) const {
    if (n) OBVI_HIP(hipMemcpyAsync(h, p_, n * sizeof(T), hipMemcpyDeviceToHost, s));
  }
  void zero(hipStream_t s) { if (n_) OBVI_HIP(hipMemsetAsync(p_, 0, n_ * sizeof(T), s)); }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  void swap(DevBuf& o) { std::swap(p_, o.p_); std::swap(n_, o.n_); std::swap(cap_, o.cap_); }

 private:
  T* p_ = nullptr;
  size_t n_ = 0, cap_ = 0;
};

// Worker threads of the host's symbolic phase and upload sorts, started once per process: a sliding-window session builds a plan per
// window (a millisecond of work in ranges of points), and starting and joining std::threads for every range cost as much as the
// ranges themselves.  run(parts, fn) calls fn(0) ... fn(parts - 1), each exactly once, on the workers and on the calling thread, and
// returns when all are done.  Calls from different threads (one handle per thread: several sessions of one process, config #5) run
// CONCURRENTLY: every call publishes its own job, a free worker enters any published job that still has parts to hand out, and a
// caller always works on its own job, so no call waits for another one (round 4 serialised them behind one mutex: k handles planning at
// once queued).  Workers spin briefly before they sleep, so that back-to-back calls do not pay a wake-up each.
// A call is ONE immutable job record (function, part count, its own hand-out and completion counters) on the caller's stack, published
// in jobs_ under the mutex.  A worker enters a job only under that mutex (and is counted in job->inside while it holds the pointer);
// run() unpublishes the job under the same mutex and leaves only when every part is done AND no worker is inside any more, so a part
// index never travels from one job to the next and nothing of a finished job is touched after run() has returned.
class HostPool {
 public:
  explicit HostPool(int workers, bool near_caller = false) {
    for (int i = 0; i < workers; ++i) {
      try { threads_.emplace_back([this] { work(); }); }
      catch (const std::system_error&) { break; }   // fewer workers: the caller takes the rest itself
    }
    if (near_caller) keep_near_caller();
  }
  ~HostPool() {
    { std::lock_guard<std::mutex> lock(m_); stop_ = true; gen_.fetch_add(1, std::memory_order_release); }
    cv_.notify_all();
    for (auto& t : threads_) t.join();
  }
  int workers() const { return (int)threads_.size(); }
  void run(int parts, const std::function<void(int)>& fn) {
    if (parts <= 1 || threads_.empty()) { for (int i = 0; i < parts; ++i) fn(i); return; }
    Job job(&fn, parts);
    {
      std::lock_guard<std::mutex> lock(m_);
      jobs_.push_back(&job);
      published_.fetch_add(1, std::memory_order_release);
      gen_.fetch_add(1, std::memory_order_release);
    }
    cv_.notify_all();
    take(job);
    while (job.left.load(std::memory_order_acquire) != 0) std::this_thread::yield();
    {                                                                                       // nobody enters from here on
      std::lock_guard<std::mutex> lock(m_);
      for (size_t i = 0; i < jobs_.size(); ++i) if (jobs_[i] == &job) { jobs_.erase(jobs_.begin() + (std::ptrdiff_t)i); break; }
      published_.fetch_sub(1, std::memory_order_release);
    }
    while (job.inside.load(std::memory_order_acquire) != 0) std::this_thread::yield();     // ... and those who did have left
  }

 private:
  struct Job {
    Job(const std::function<void(int)>* f, int n) : fn(f), parts(n), left(n) {}
    const std::function<void(int)>* const fn;
    const int parts;
    std::atomic<int> next{0}, left, inside{0};
  };
  // The workers read what the calling thread wrote a moment ago and the caller then overwrites what they read (one problem per frame in
  // a sliding-window session).  Spread by the scheduler over a two-socket host, every such line crosses the sockets; kept on the caller's
  // block of logical CPUs (same socket, neighbouring L3 slices) it does not -- worth 2-3 % of a session on a 2 x 64-core host.  A library
  // must not change thread placement behind its host's back, so this is opt-in: OBVI_HOST_AFFINITY=1 (run_offline_ba sets it for itself).
  void keep_near_caller() {
#if defined(__linux__)
    const int cpu = sched_getcpu();
    cpu_set_t allowed;
    if (cpu < 0 || threads_.empty() || sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return;
    const int block = 16, base = cpu - cpu % block;
    cpu_set_t near;
    CPU_ZERO(&near);
    int n = 0;
    for (int c = base; c < base + block; ++c) if (CPU_ISSET(c, &allowed)) { CPU_SET(c, &near); ++n; }
    if (n < 2) return;
    for (auto& t : threads_) (void)pthread_setaffinity_np(t.native_handle(), sizeof(near), &near);
#endif
  }
  static void take(Job& job) {
    for (;;) {
      const int i = job.next.fetch_add(1, std::memory_order_acq_rel);
      if (i >= job.parts) return;
      (*job.fn)(i);
      job.left.fetch_sub(1, std::memory_order_release);
    }
  }
  void work() {
    uint64_t seen = 0;
    for (;;) {
      for (int spin = 0; spin < 20000 && gen_.load(std::memory_order_acquire) == seen; ++spin) {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
      }
      Job* job = nullptr;
      uint64_t picked_at = seen;
      {
        std::unique_lock<std::mutex> lock(m_);
        cv_.wait(lock, [&] { return gen_.load(std::memory_order_acquire) != seen; });
        if (stop_) return;
        for (Job* j : jobs_) if (j->next.load(std::memory_order_acquire) < j->parts) { job = j; break; }   // any caller's job with parts left
        picked_at = gen_.load(std::memory_order_acquire);
        if (job == nullptr) { seen = picked_at; continue; }                                               // nothing to do for this generation
        job->inside.fetch_add(1, std::memory_order_acq_rel);   // counted while the pointer is held: run() waits for zero
      }
      take(*job);
      job->inside.fetch_sub(1, std::memory_order_release);
      // another caller's job may be waiting: look again before sleeping -- but only if one is published (the common case is a single caller,
      // whose run() wants the mutex right now to take its job back: fifteen workers queueing for it cost more than the look is worth)
      if (published_.load(std::memory_order_acquire) <= 1) seen = picked_at;   // (a job published since then has moved gen_ on: it is looked at right away)
    }
  }
  std::vector<std::thread> threads_;
  std::mutex m_;
  std::condition_variable cv_;
  std::atomic<uint64_t> gen_{0};
  std::atomic<int> published_{0};   // jobs in jobs_ (read outside the mutex)
  std::vector<Job*> jobs_;   // published jobs, guarded by m_
  bool stop_ = false;
};

// out = (sym(cov))^(-1/2) for an n x n (n <= 18) symmetric positive definite matrix, row-major.  rel_floor > 0: also refuse a matrix whose smallest
// eigenvalue is not above rel_floor x the largest (numerically singular: a tiny positive pivot of rounding would become an enormous weight).
// One-sided view: eigen-decomposition by threshold-free cyclic Jacobi sweeps on a working copy,
// then out = sum_k v_k v_k^T / sqrt(lambda_k).  Returns false when cov is not finite / not SPD.
inline bool sym_inverse_sqrt(const double* cov, int n, double* out, double rel_floor = 0.0) {
  double a[18][18], v[18][18];   // n <= 18: the joint covariance of two 9-parameter ellipsoid blocks
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      a[i][j] = 0.5 * (cov[i * n + j] + cov[j * n + i]);
      v[i][j] = i == j;
      if (!std::isfinite(a[i][j])) return false;
    }
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0, tot = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) { tot += a[i][j] * a[i][j]; if (i != j) off += a[i][j] * a[i][j]; }
    if (off <= tot * 1e-32) break;
    for (int p = 0; p + 1 < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        // rotation angle that annihilates a[p][q]
        const double tau = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::hypot(1.0, tau));
        const double c = 1.0 / std::hypot(1.0, t), s = t * c;
        for (int k = 0; k < n; ++k) { const double x = a[k][p], y = a[k][q]; a[k][p] = c * x - s * y; a[k][q] = s * x + c * y; }
        for (int k = 0; k < n; ++k) { const double x = a[p][k], y = a[q][k]; a[p][k] = c * x - s * y; a[q][k] = s * x + c * y; }
        for (int k = 0; k < n; ++k) { const double x = v[k][p], y = v[k][q]; v[k][p] = c * x - s * y; v[k][q] = s * x + c * y; }
      }
  }
  double ev_max = 0.0;
  for (int k = 0; k < n; ++k) ev_max = std::max(ev_max, a[k][k]);
  for (int k = 0; k < n; ++k) if (!(a[k][k] > rel_floor * ev_max)) return false;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double acc = 0.0;
      for (int k = 0; k < n; ++k) acc += v[i][k] * v[j][k] / std::sqrt(a[k][k]);
      out[i * n + j] = acc;
    }
  return true;
}


// Map pair prior (include/obvi_map_prior.h): from the pair's joint covariance C = [[A, B], [B^T, D]] (N x N row-major, N = 2 od, symmetrised as for the
// other priors) the matrix W of r = W d and the information Lambda = W^T W.  Joint form: W = C^-1/2.  Conditional form p(b | a): K = B^T A^-1,
// S_c = D - K B, rows [0, od) of W zero, rows [od, N) = S_c^-1/2 [-K, I].  false: C is not positive definite (either form needs the whole of it), or
// numerically singular: condition number above 1e13, where an fp64 inverse keeps no more than three digits -- a joint covariance assembled from computed
// blocks can be that close to singular, and its information would be an artefact of rounding.
inline bool map_pair_weights(const double* C, int od, bool joint, double* W, double* Lambda) {
  const int N = 2 * od;
  double Ci[18 * 18];
  constexpr double kFloor = 1e-13;
  if (!sym_inverse_sqrt(C, N, Ci, kFloor)) return false;
  std::fill(W, W + N * N, 0.0);
  if (joint) {
    std::copy(Ci, Ci + N * N, W);
  } else {
    double A[81], Ais[81], Ainv[81], K[81], Sc[81], Scis[81];
    for (int x = 0; x < od; ++x) for (int y = 0; y < od; ++y) A[od * x + y] = C[N * x + y];
    if (!sym_inverse_sqrt(A, od, Ais, kFloor)) return false;
    for (int x = 0; x < od; ++x) for (int y = 0; y < od; ++y) { double acc = 0.0; for (int k = 0; k < od; ++k) acc += Ais[od * x + k] * Ais[od * k + y]; Ainv[od * x + y] = acc; }
    auto Bt = [&](int x, int k) { return 0.5 * (C[N * (od + x) + k] + C[N * k + od + x]); };   // B^T: the lower-left block
    for (int x = 0; x < od; ++x) for (int y = 0; y < od; ++y) { double acc = 0.0; for (int k = 0; k < od; ++k) acc += Bt(x, k) * Ainv[od * k + y]; K[od * x + y] = acc; }
    for (int x = 0; x < od; ++x) for (int y = 0; y < od; ++y) { double acc = 0.0; for (int k = 0; k < od; ++k) acc += K[od * x + k] * Bt(y, k); Sc[od * x + y] = C[N * (od + x) + od + y] - acc; }
    if (!sym_inverse_sqrt(Sc, od, Scis, kFloor)) return false;
    for (int x = 0; x < od; ++x)
      for (int y = 0; y < od; ++y) {
        double acc = 0.0;
        for (int k = 0; k < od; ++k) acc += Scis[od * x + k] * K[od * k + y];
        W[N * (od + x) + y] = -acc; W[N * (od + x) + od + y] = Scis[od * x + y];
      }
  }
  for (int x = 0; x < N; ++x) for (int y = 0; y <= x; ++y) { double acc = 0.0; for (int k = 0; k < N; ++k) acc += W[N * k + x] * W[N * k + y]; Lambda[N * x + y] = Lambda[N * y + x] = acc; }
  return true;
}

// Map group prior (include/obvi_map_group_prior.h): from the group's joint covariance C (N x N row-major, symmetrised as for the other priors; N up to a few
// thousand) the lower triangular W = L^-1 of r = W d (C = L L^T; N x N, zeros above the diagonal) and the information Lambda = W^T W = C^-1 (N rows of ld >= N
// doubles, both triangles, the padding zero).  Plain fp64, once per upload: a blocked right-looking Cholesky (64-column panels: the panel solve and the trailing
// update are dot products of contiguous row pieces, handed out by rows), the triangular inverse by column strips (a strip's recurrence touches no other strip),
// Lambda by rows.  par(n, fn) runs fn(i0, i1) over ranges that cover [0, n) -- on the host's workers, or in place.
// false: C is not finite, not positive definite, or numerically singular: (largest / smallest Cholesky pivot)^2, a lower bound of the condition number, above
// 1e13, or the condition number itself (largest eigenvalue of C times largest of Lambda, by power steps) above 1e13 -- the floor of map_pair_weights.
// `work`: N x N scratch.
template <class Par>
inline bool map_group_weights(const double* C, int N, double* W, double* Lambda, int ld, double* work, Par&& par) {
  constexpr int nb = 64;
  double* A = work;
  bool finite = true;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j <= i; ++j) { const double v = 0.5 * (C[(size_t)N * i + j] + C[(size_t)N * j + i]); A[(size_t)N * i + j] = v; finite = finite && std::isfinite(v); }
  if (!finite) return false;
  double piv_min = 0.0, piv_max = 0.0;
  for (int k0 = 0; k0 < N; k0 += nb) {
    const int k1 = std::min(N, k0 + nb);
    for (int j = k0; j < k1; ++j) {   // the diagonal block, unblocked
      double* Aj = A + (size_t)N * j;
      double dj = Aj[j];
      for (int t = k0; t < j; ++t) dj -= Aj[t] * Aj[t];
      if (!(dj > 0.0) || !std::isfinite(dj)) return false;
      dj = std::sqrt(dj);
      Aj[j] = dj;
      piv_min = (k0 == 0 && j == 0) ? dj : std::min(piv_min, dj); piv_max = std::max(piv_max, dj);
      for (int i = j + 1; i < k1; ++i) {
        double* Ai = A + (size_t)N * i;
        double v = Ai[j];
        for (int t = k0; t < j; ++t) v -= Ai[t] * Aj[t];
        Ai[j] = v / dj;
      }
    }
    if (k1 == N) break;
    par(N - k1, [&](int64_t i0, int64_t i1) {   // the panel below it: L_ik = A_ik L_kk^-T
      for (int64_t i = k1 + i0; i < k1 + i1; ++i) {
        double* Ai = A + (size_t)N * i;
        for (int j = k0; j < k1; ++j) {
          const double* Aj = A + (size_t)N * j;
          double v = Ai[j];
          for (int t = k0; t < j; ++t) v -= Ai[t] * Aj[t];
          Ai[j] = v / Aj[j];
        }
      }
    });
    par(N - k1, [&](int64_t i0, int64_t i1) {   // the trailing update, lower triangle
      for (int64_t i = k1 + i0; i < k1 + i1; ++i) {
        double* Ai = A + (size_t)N * i;
        for (int64_t j = k1; j <= i; ++j) {
          const double* Aj = A + (size_t)N * j;
          double v = 0.0;
          for (int t = k0; t < k1; ++t) v += Ai[t] * Aj[t];
          Ai[j] -= v;
        }
      }
    });
  }
  if (!(piv_min * piv_min > 1e-13 * piv_max * piv_max)) return false;
  // W = L^-1 in strips of 32 columns [j0, j1): row i of the strip is (e_i - sum_{j0 <= k < i} L_ik W_k) / L_ii
  std::fill(W, W + (size_t)N * N, 0.0);
  constexpr int ws = 32;
  par((N + ws - 1) / ws, [&](int64_t s0, int64_t s1) {
    for (int64_t sidx = s0; sidx < s1; ++sidx) {
      const int j0 = (int)sidx * ws, j1 = std::min(N, j0 + ws);
      for (int i = j0; i < N; ++i) {
        const double* Li = A + (size_t)N * i;
        double* Wi = W + (size_t)N * i;
        const int je = std::min(j1, i + 1);   // (lower triangular: columns up to i)
        for (int k = j0; k < i; ++k) {
          const double l = Li[k];
          const double* Wk = W + (size_t)N * k;
          const int ke = std::min(je, k + 1);
          for (int j = j0; j < ke; ++j) Wi[j] -= l * Wk[j];
        }
        if (i < j1) Wi[i] += 1.0;
        const double inv = 1.0 / Li[i];
        for (int j = j0; j < je; ++j) Wi[j] *= inv;
      }
    }
  });
  // Lambda_ij = sum_{k >= i} W_ki W_kj, j <= i: row i collects the rows k >= i of W; then the upper triangle
  par(N, [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
      double* Li = Lambda + (size_t)ld * i;
      std::fill(Li, Li + ld, 0.0);
      for (int64_t k = i; k < N; ++k) {
        const double* Wk = W + (size_t)N * k;
        const double wki = Wk[i];
        for (int64_t j = 0; j <= i; ++j) Li[j] += wki * Wk[j];
      }
    }
  });
  for (int i = 0; i < N; ++i) for (int j = 0; j < i; ++j) Lambda[(size_t)ld * j + i] = Lambda[(size_t)ld * i + j];
  // The pivot ratio is only a lower bound (a rotated matrix hides its small eigenvalues from the diagonal of L): the condition number itself, as the product
  // of the largest eigenvalues of C = L L^T and of Lambda, each by 40 power steps from a fixed start (Rayleigh quotients: lower bounds again, within a few
  // per cent after the first steps).  N^2 work per step beside the N^3 above.
  auto top_eigenvalue = [&](auto&& apply) {
    std::vector<double> x((size_t)N), y((size_t)N);
    uint64_t lcg = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < N; ++i) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; x[i] = 0.5 + (double)(lcg >> 11) / 9007199254740992.0; }
    double ev = 0.0;
    for (int it = 0; it < 40; ++it) {
      double nx = 0.0;
      for (int i = 0; i < N; ++i) nx += x[i] * x[i];
      nx = std::sqrt(nx);
      if (!(nx > 0.0) || !std::isfinite(nx)) return std::numeric_limits<double>::infinity();
      for (int i = 0; i < N; ++i) x[i] /= nx;
      apply(x.data(), y.data());
      ev = 0.0;
      for (int i = 0; i < N; ++i) ev += x[i] * y[i];
      x.swap(y);
    }
    return ev;
  };
  std::vector<double> t((size_t)N);
  const double ev_c = top_eigenvalue([&](const double* x, double* y) {   // y = L (L^T x)
    std::fill(t.begin(), t.end(), 0.0);
    for (int i = 0; i < N; ++i) { const double* Li = A + (size_t)N * i; const double xi = x[i]; for (int j = 0; j <= i; ++j) t[j] += Li[j] * xi; }
    par(N, [&](int64_t i0, int64_t i1) {
      for (int64_t i = i0; i < i1; ++i) { const double* Li = A + (size_t)N * i; double v = 0.0; for (int64_t j = 0; j <= i; ++j) v += Li[j] * t[j]; y[i] = v; }
    });
  });
  const double ev_l = top_eigenvalue([&](const double* x, double* y) {
    par(N, [&](int64_t i0, int64_t i1) {
      for (int64_t i = i0; i < i1; ++i) { const double* Li = Lambda + (size_t)ld * i; double v = 0.0; for (int j = 0; j < N; ++j) v += Li[j] * x[j]; y[i] = v; }
    });
  });
  if (!(ev_c * ev_l <= 1e13)) return false;
  return true;
}

}  // namespace obvi
#endif  // OBVI_HOST_UTIL_H_
