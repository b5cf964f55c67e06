// map_kernels.hip -- group priors cut from a device-resident map (include/obvi_map_resident.h): gather of the groups' covariance sub-blocks, blocked right-looking
// Cholesky by tile column, W = L^-1 by tile columns, Lambda = W^T W, and the two power iterations of the condition estimate.  Every group of a call shares every
// launch (grid over work item x group); launch boundaries are the only synchronisation between workgroups; no floating-point atomics: every sum has a fixed order.
// Workspace per group (MapCutGroup): nt x nt tiles of 64 x 64 doubles (tile-major, chol_tile.h), the ragged last tile padded with the identity --
//   A  : the symmetrised sub-block, lower triangle of tiles; overwritten by L
//   Li : nt tiles, the inverses of the diagonal tiles of L
//   Wt : tile (i, k), k <= i, holds (W_ik)^T -- the operand order tile_abt_mfma (C += A B^T) wants in stages 3 and 4
// and Csym, the sub-block again as N rows of ld doubles (the layout of Lambda), for the power steps on C.
// Second half of the file: the entries that write a new map.  They share ONE downdate path -- k_map_downdate (C' = Cs[rows, rows] - Z Y^T on a row table),
// k_map_wd (v = W d) and k_map_mean (mu' = mu[rows] + sign Y v) -- on the factor of a one-group cut, under the same rules, and three callers feed it: the map
// conditioned on the posterior of a window's objects (include/obvi_map_update.h, MapUpdateDev: identity rows, Z = Y (I - W Ps W^T), sign +); the map grown by
// the window's new objects, born from a posterior, or gathered down to some of its objects (include/obvi_map_extend.h: the condition's launches into a larger
// map, plus the cross block; the condition IS the extension by no object, and both end in the scatter of the window's whole block); duplicate objects of the
// map merged (include/obvi_map_merge.h: the innovation covariance of the pairs built in a one-group cut and factored as any cut, the gain tiles of the
// surviving rows alone, then the downdate through the survivors' row table with Z = Y, sign -, straight into the smaller map).  Every read of a symmetrised
// entry of a map or a posterior goes through stage_sym / sym_at.  Then the ordered compaction the two report entries share -- compact_counts (a workgroup's
// counts per thread to its sums), compact_scan (one workgroup: the exclusive scan of a strided count array, and its total), compact_place (a workgroup's hits to
// their places, by ballot) -- and its first user: duplicate objects of the map proposed (include/obvi_map_match.h): every pair's difference in units of its own
// covariance, one lane per pair, and the pairs within the gate compacted in (a, b) order.
// After it: the map moved into another frame under an uncertain transform, object-aligned block pair by block pair, and two maps joined
// (include/obvi_map_frame.h).  Last: one map located in another from the constellations of their object centres (include/obvi_map_locate.h): compatible
// seeds counted, scanned and scattered by the same three helpers, as the qualifying hypotheses are; every hypothesis scored with both maps' centres and centre blocks in local memory; the qualifying ones ranked by
// counting; the reported ones refined, one wavefront each.
#include "chol_tile.h"

namespace obvi {
namespace {

__device__ __forceinline__ double wave_sum(double v) {   // butterfly: every lane ends with the same bits
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// accumulators of tile_abt_mfma -> a row-major tile in LDS (leading dimension LDM), scaled
__device__ __forceinline__ void acc_to_lds(double* dst, const f64x4 acc[4], double scale) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) dst[(16 * rt + (lane >> 4) + 4 * r) * LDM + 16 * wv + (lane & 15)] = scale * acc[rt][r];
}
__device__ __forceinline__ void acc_to_tile(double* tile, const f64x4 acc[4]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) tile[(16 * rt + (lane >> 4) + 4 * r) * T + 16 * wv + (lane & 15)] = acc[rt][r];
}

// ---- what every part of the file shares: row tables, the symmetrised read, a tile written to both triangles ---------------------------------------
// Row w of a list of n rows, od per object -> its row of the map, idx[w / od] od + w % od (idx NULL: w itself); -1 behind the list: padding
__device__ __forceinline__ int32_t table_row(const uint32_t* idx, int od, int n, int w) { return w >= n ? -1 : (idx != nullptr ? (int32_t)idx[w / od] * od + w % od : w); }
// one tile row's 64 entries of a table, by the first 64 threads; a barrier before anyone reads them
__device__ __forceinline__ void fill_rows(int32_t* t, const uint32_t* idx, int od, int n, int tile) { if (threadIdx.x < T) t[threadIdx.x] = table_row(idx, od, n, T * tile + threadIdx.x); }
// The symmetrised two-sided read of Cs = (C + C^T) / 2 at rows ra x columns cb (two tables of 64 rows of C in LDS): both blocks of C are read along their rows,
// P[a][b] = C[ra[a]][cb[b]] and Q[a][b] = C[cb[a]][ra[b]], zero in the padding, and meet in LDS: behind a barrier Cs[ra[r]][cb[c]] = sym_at(P, Q, r, c).
// Each tile travels in two phases, as tile_fetch / tile_put do it: all of a thread's loads first, then its LDS writes (one loop of load + store waits for every
// load on its own: sixteen memory latencies per tile).
__device__ __forceinline__ void stage_sym(double* P, double* Q, const double* C, int64_t ld, const int32_t* ra, const int32_t* cb) {
  constexpr int X = T * T / kThreads;
  const int b = threadIdx.x & 63, a0 = threadIdx.x >> 6;   // element x of a thread: row a0 + 4 x, column b
  const int32_t pb = cb[b], qb = ra[b];
  double p[X], q[X];
#pragma unroll
  for (int x = 0; x < X; ++x) {
    const int32_t pa = ra[a0 + (kThreads / T) * x];
    const double c = C[(pa >= 0 && pb >= 0) ? (int64_t)pa * ld + pb : 0];   // unconditional, or every load gets a block and a wait of its own; C[0] is there
    p[x] = (pa >= 0 && pb >= 0) ? c : 0.0;
  }
#pragma unroll
  for (int x = 0; x < X; ++x) P[(a0 + (kThreads / T) * x) * LDM + b] = p[x];
#pragma unroll
  for (int x = 0; x < X; ++x) {
    const int32_t qa = cb[a0 + (kThreads / T) * x];
    const double c = C[(qa >= 0 && qb >= 0) ? (int64_t)qa * ld + qb : 0];
    q[x] = (qa >= 0 && qb >= 0) ? c : 0.0;
  }
#pragma unroll
  for (int x = 0; x < X; ++x) Q[(a0 + (kThreads / T) * x) * LDM + b] = q[x];
}
__device__ __forceinline__ double sym_at(const double* P, const double* Q, int r, int c) { return 0.5 * (P[r * LDM + c] + Q[c * LDM + r]); }
// Tile (ti, tj) of an nr x nc block, row-major in LDS, to out[T ti + r][off + T tj + c] and, transposed, to out[off + T tj + r][T ti + c]: both copies are
// written along their rows.  lower: a diagonal tile of a symmetric block -- written once, its upper half mirrored from its lower.  Returns whether an entry
// of the first copy is not finite.
__device__ __forceinline__ bool tile_to_both_triangles(const double* A, double* out, int64_t ldo, int ti, int tj, int nr, int nc, int off, bool lower) {
  bool bad = false;
  for (int e = threadIdx.x; e < T * T; e += kThreads) {
    const int r = e >> 6, c = e & 63;
    const int gi = T * ti + r, gj = T * tj + c;
    if (gi < nr && gj < nc) {
      const double x = (lower && c > r) ? A[c * LDM + r] : A[r * LDM + c];
      out[(int64_t)gi * ldo + off + gj] = x;
      bad = bad || !isfinite(x);
    }
    const int hj = T * tj + r, hi = T * ti + c;
    if (!lower && hi < nr && hj < nc) out[(int64_t)(off + hj) * ldo + hi] = A[c * LDM + r];
  }
  return bad;
}

// ---- stage 1: gather ---------------------------------------------------------------------------------------------------------------------
// workgroup (ti, tj <= ti, group): A_ij = (C[rows i][rows j] + C[rows j][rows i]^T) / 2, the symmetrised read above
__global__ void __launch_bounds__(kThreads) k_map_gather(MapCutDev m, const double* __restrict__ map_mean, const double* __restrict__ map_cov, int64_t ldc) {
  __shared__ double P[T * LDM];
  __shared__ double Q[T * LDM];
  __shared__ int32_t rows_i[T], rows_j[T];
  const int ti = blockIdx.x, tj = blockIdx.y;
  if (tj > ti) return;
  for (int64_t g = blockIdx.z; g < m.n; g += gridDim.z) {
    const MapCutGroup G = m.groups[g];
    if (ti >= G.nt) continue;
    const int od = m.od, tid = threadIdx.x;
    __syncthreads();
    fill_rows(rows_i, m.map_idx + G.member0, od, G.N, ti);
    fill_rows(rows_j, m.map_idx + G.member0, od, G.N, tj);
    __syncthreads();
    stage_sym(P, Q, map_cov, ldc, rows_i, rows_j);
    __syncthreads();
    double* tile = tile_ptr(m.A + G.tile0 * (T * T), G.nt, ti, tj);
    double* Cs = m.Csym + G.lam_off;
    for (int e = tid; e < T * T; e += kThreads) {
      const int r = e >> 6, c = e & 63, gi = T * ti + r, gj = T * tj + c;
      const bool in = gi < G.N && gj < G.N;
      const double v = in ? sym_at(P, Q, r, c) : (gi == gj ? 1.0 : 0.0);
      tile[e] = v;
      if (in) Cs[(int64_t)gi * G.ld + gj] = v;
    }
    if (ti != tj) {   // the upper triangle of Csym, written along its rows
      for (int e = tid; e < T * T; e += kThreads) {
        const int r = e >> 6, c = e & 63, gj = T * tj + r, gi = T * ti + c;
        if (gi < G.N && gj < G.N) Cs[(int64_t)gj * G.ld + gi] = sym_at(P, Q, c, r);
      }
    }
    if (tj == 0 && tid < T && rows_i[tid] >= 0) m.mean[(int64_t)od * G.member0 + T * ti + tid] = map_mean[rows_i[tid]];
  }
}

// ---- stage 2: Cholesky by tile column ------------------------------------------------------------------------------------------------------
// One workgroup per group: factor the diagonal tile k (unblocked, right-looking, in LDS), form its inverse by forward substitution, record the pivots.
// A pivot that is not positive and finite sets the flag and is replaced by 1: a select, never a branch.  Padding rows (identity) stay out of the extremes.
__global__ void __launch_bounds__(kThreads) k_map_potrf(MapCutDev m, int k) {
  __shared__ double Ls[T * LDM];
  __shared__ double X[T * LDM];
  for (int64_t g = blockIdx.x; g < m.n; g += gridDim.x) {
    const MapCutGroup G = m.groups[g];
    if (k >= G.nt) continue;
    const int tid = threadIdx.x;
    double* tile = tile_ptr(m.A + G.tile0 * (T * T), G.nt, k, k);
    __syncthreads();
    stage_tile(Ls, tile);
    double* st = m.status + kMapStatusDoubles * g;
    double bad = 0.0, pmin = INFINITY, pmax = 0.0;
    if (k > 0) { bad = st[MS_BAD]; pmin = st[MS_PIV_MIN]; pmax = st[MS_PIV_MAX]; }
    __syncthreads();
    const int row = tid >> 2, part = tid & 3;
    for (int j = 0; j < T; ++j) {
      const double d = Ls[j * LDM + j];
      const bool ok = d > 0.0 && isfinite(d);
      const double dj = sqrt(ok ? d : 1.0);
      if (T * k + j < G.N) { bad = ok ? bad : 1.0; pmin = fmin(pmin, dj); pmax = fmax(pmax, dj); }
      if (tid > j && tid < T) Ls[tid * LDM + j] = Ls[tid * LDM + j] / dj;
      __syncthreads();
      if (row > j) {   // row `row`, columns j < c <= row, c = part mod 4
        const double l = Ls[row * LDM + j];
        for (int c = j + 1 + ((part - (j + 1)) & 3); c <= row; c += 4) Ls[row * LDM + c] -= l * Ls[c * LDM + j];
      }
      __syncthreads();
    }
    if (tid < T) { const double d = Ls[tid * LDM + tid]; Ls[tid * LDM + tid] = sqrt((d > 0.0 && isfinite(d)) ? d : 1.0); }
    __syncthreads();
    // X = L^-1: column c = tid / 4, row after row; the four threads of a column split the dot product by j mod 4
    const int c = tid >> 2;
    for (int i = 0; i < T; ++i) {
      double s = 0.0;
      for (int j = (c & ~3) + part; j < i; j += 4) s += Ls[i * LDM + j] * X[j * LDM + c];
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      if (part == 0) X[i * LDM + c] = i < c ? 0.0 : ((i == c ? 1.0 : 0.0) - s) / Ls[i * LDM + i];
      __syncthreads();
    }
    double* Li = m.Li + (G.diag0 + k) * (T * T);
    for (int e = tid; e < T * T; e += kThreads) {
      const int r = e >> 6, cc = e & 63;
      tile[e] = cc <= r ? Ls[r * LDM + cc] : 0.0;
      Li[e] = X[r * LDM + cc];
    }
    if (tid == 0) { st[MS_BAD] = bad; st[MS_PIV_MIN] = pmin; st[MS_PIV_MAX] = pmax; }
  }
}

// tiles below the diagonal: A_ik <- A_ik L_kk^-T
__global__ void __launch_bounds__(kThreads) k_map_trsm(MapCutDev m, int k) {
  __shared__ double A[T * LDM];
  __shared__ double B[T * LDM];
  const int i = k + 1 + blockIdx.x;
  for (int64_t g = blockIdx.y; g < m.n; g += gridDim.y) {
    const MapCutGroup G = m.groups[g];
    if (i >= G.nt) continue;
    double* tile = tile_ptr(m.A + G.tile0 * (T * T), G.nt, i, k);
    __syncthreads();
    stage_tiles(A, tile, B, m.Li + (G.diag0 + k) * (T * T));
    __syncthreads();
    f64x4 acc[4] = {};
    tile_abt_mfma(A, B, acc);
    acc_to_tile(tile, acc);
  }
}

// trailing update, lower triangle of tiles: A_ij -= L_ik L_jk^T
__global__ void __launch_bounds__(kThreads) k_map_syrk(MapCutDev m, int k) {
  __shared__ double A[T * LDM];
  __shared__ double B[T * LDM];
  const int i = k + 1 + blockIdx.x, j = k + 1 + blockIdx.y;
  if (j > i) return;
  for (int64_t g = blockIdx.z; g < m.n; g += gridDim.z) {
    const MapCutGroup G = m.groups[g];
    if (i >= G.nt) continue;
    double* S = m.A + G.tile0 * (T * T);
    __syncthreads();
    if (i != j) stage_tiles(A, tile_ptr(S, G.nt, i, k), B, tile_ptr(S, G.nt, j, k));
    else stage_tile(A, tile_ptr(S, G.nt, i, k));
    __syncthreads();
    f64x4 acc[4] = {};
    tile_abt_mfma(A, i != j ? B : A, acc);
    double* C = tile_ptr(S, G.nt, i, j);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double v[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[rt][r] = C[(16 * rt + (lane >> 4) + 4 * r) * T + 16 * wv + (lane & 15)];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) C[(16 * rt + (lane >> 4) + 4 * r) * T + 16 * wv + (lane & 15)] = v[rt][r] - acc[rt][r];
  }
}

// ---- stage 3: W = L^-1, one workgroup per tile column ----------------------------------------------------------------------------------------
// Column k depends on no other column: Wt_kk = (L_kk^-1)^T, then for i > k:  Wt_ik = -(sum_{k <= j < i} Wt_jk L_ij^T) L_ii^-T.  The workgroup reads back the tiles of
// its own column that it wrote (behind its own barrier); W goes out row-major N x N without the padding.
__global__ void __launch_bounds__(kThreads) k_map_winv(MapCutDev m) {
  __shared__ double A[T * LDM];
  __shared__ double B[T * LDM];
  const int k = blockIdx.x, tid = threadIdx.x;
  for (int64_t g = blockIdx.y; g < m.n; g += gridDim.y) {
    const MapCutGroup G = m.groups[g];
    if (k >= G.nt) continue;
    const double* L = m.A + G.tile0 * (T * T);
    double* Wt = m.Wt + G.tile0 * (T * T);
    const double* Li = m.Li + G.diag0 * (T * T);
    double* W = m.W + G.w_off;
    const int N = G.N;
    __syncthreads();
    stage_tile(A, Li + (int64_t)k * (T * T));
    __syncthreads();
    {
      double* wt = tile_ptr(Wt, G.nt, k, k);
      for (int e = tid; e < T * T; e += kThreads) {
        const int r = e >> 6, c = e & 63, gi = T * k + r, gj = T * k + c;
        wt[e] = A[c * LDM + r];
        if (gi < N && gj < N) W[(int64_t)gi * N + gj] = A[r * LDM + c];
      }
    }
    for (int i = k + 1; i < G.nt; ++i) {
      f64x4 acc[4] = {};
      for (int j = k; j < i; ++j) {
        __syncthreads();
        stage_tiles(A, tile_ptr(Wt, G.nt, j, k), B, tile_ptr(const_cast<double*>(L), G.nt, i, j));
        __syncthreads();
        tile_abt_mfma(A, B, acc);   // (sum_j L_ij W_jk)^T
      }
      __syncthreads();
      {
        TileRegs rb;
        tile_fetch(rb, Li + (int64_t)i * (T * T));
        acc_to_lds(A, acc, -1.0);
        tile_put(B, rb);
      }
      __syncthreads();
      f64x4 w[4] = {};
      tile_abt_mfma(A, B, w);        // Wt_ik
      acc_to_tile(tile_ptr(Wt, G.nt, i, k), w);
      __syncthreads();
      acc_to_lds(A, w, 1.0);
      __syncthreads();
      for (int e = tid; e < T * T; e += kThreads) {
        const int r = e >> 6, c = e & 63, gi = T * i + r;
        if (gi < N) W[(int64_t)gi * N + T * k + c] = A[c * LDM + r];
      }
    }
  }
}

// ---- stage 4: Lambda = W^T W ---------------------------------------------------------------------------------------------------------------------
// tile (i, j <= i): sum_{k >= i} W_ki^T W_kj = sum_k Wt_ki Wt_kj^T ... with Wt_ki the tile of W_ki^T.  Both triangles, rows of ld doubles (the padding was zeroed).
__global__ void __launch_bounds__(kThreads) k_map_lambda(MapCutDev m) {
  __shared__ double A[T * LDM];
  __shared__ double B[T * LDM];
  const int i = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
  if (j > i) return;
  for (int64_t g = blockIdx.z; g < m.n; g += gridDim.z) {
    const MapCutGroup G = m.groups[g];
    if (i >= G.nt) continue;
    double* Wt = m.Wt + G.tile0 * (T * T);
    f64x4 acc[4] = {};
    for (int k = i; k < G.nt; ++k) {
      __syncthreads();
      if (i != j) stage_tiles(A, tile_ptr(Wt, G.nt, k, i), B, tile_ptr(Wt, G.nt, k, j));
      else stage_tile(A, tile_ptr(Wt, G.nt, k, i));
      __syncthreads();
      tile_abt_mfma(A, i != j ? B : A, acc);
    }
    __syncthreads();
    acc_to_lds(A, acc, 1.0);
    __syncthreads();
    double* Lam = m.Lambda + G.lam_off;
    const int N = G.N;
    for (int e = tid; e < T * T; e += kThreads) {
      const int r = e >> 6, c = e & 63;
      const int gi = T * i + r, gj = T * j + c;
      if (gi < N && gj < N) Lam[(int64_t)gi * G.ld + gj] = (i == j && c > r) ? A[c * LDM + r] : A[r * LDM + c];   // a diagonal tile: its lower triangle, mirrored
      const int hj = T * j + r, hi = T * i + c;
      if (i != j && hi < N && hj < N) Lam[(int64_t)hj * G.ld + hi] = A[c * LDM + r];
    }
  }
}

// ---- stage 5: power steps ------------------------------------------------------------------------------------------------------------------------
// One step of x <- M x / |x| on Csym (which = 0) and on Lambda (which = 1): workgroup (16 rows, group, which) normalises x itself (every workgroup the same sum in
// the same order), writes its rows of M x and its part of the Rayleigh quotient x^T M x / |x|^2.
constexpr int kPowRows = 16;
__global__ void __launch_bounds__(kThreads) k_map_power(MapCutDev m, const double* __restrict__ x0, int step) {
  __shared__ double xs[kMapGroupMaxRows];
  __shared__ double red[kThreads];
  __shared__ double part[kPowRows];
  const int which = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int64_t g = blockIdx.y; g < m.n; g += gridDim.y) {
    const MapCutGroup G = m.groups[g];
    const int N = G.N, r0 = kPowRows * blockIdx.x;
    if (r0 >= N) continue;
    const double* M = (which ? m.Lambda : m.Csym) + G.lam_off;
    const int64_t xoff = (int64_t)which * m.rows + (int64_t)m.od * G.member0;
    const double* xin = step == 0 ? x0 : m.x + (int64_t)(step & 1) * 2 * m.rows + xoff;
    double* xout = m.x + (int64_t)((step + 1) & 1) * 2 * m.rows + xoff;
    __syncthreads();
    double s = 0.0;
    for (int c = tid; c < N; c += kThreads) { const double v = xin[c]; xs[c] = v; s += v * v; }
    red[tid] = s;
    __syncthreads();
    for (int w = kThreads / 2; w >= 1; w >>= 1) { if (tid < w) red[tid] += red[tid + w]; __syncthreads(); }
    const double nx = sqrt(red[0]);
    for (int c = tid; c < N; c += kThreads) xs[c] = xs[c] / nx;
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < kPowRows / 4; ++rr) {
      const int row = r0 + 4 * wv + rr;
      double y = 0.0;
      if (row < N) for (int c = lane; c < N; c += 64) y += M[(int64_t)row * G.ld + c] * xs[c];
      y = wave_sum(y);
      if (lane == 0) { part[4 * wv + rr] = row < N ? xs[row] * y : 0.0; if (row < N) xout[row] = y; }
    }
    __syncthreads();
    if (tid == 0) {
      double e = 0.0;
      for (int q = 0; q < kPowRows; ++q) e += part[q];
      m.partial[((int64_t)g * 2 + which) * (kMapGroupMaxRows / kPowRows) + blockIdx.x] = e;
    }
  }
}
// the last step's Rayleigh quotients into the status records
__global__ void __launch_bounds__(64) k_map_power_finish(MapCutDev m) {
  const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= m.n) return;
  const int nb = (m.groups[g].N + kPowRows - 1) / kPowRows;
  for (int which = 0; which < 2; ++which) {
    double e = 0.0;
    for (int b = 0; b < nb; ++b) e += m.partial[(g * 2 + which) * (kMapGroupMaxRows / kPowRows) + b];
    m.status[kMapStatusDoubles * g + (which ? MS_EV_LAMBDA : MS_EV_C)] = e;
  }
}

// ==== the map conditioned on a window's posterior (include/obvi_map_update.h; MapUpdateDev, ba_device.h), and the downdate path ===========================
// Every kernel below writes tiles or rows that no other workgroup of its launch writes, reads only what earlier launches wrote, and sums in a fixed order.
// (ti, tj, 0): Wn_ij = (Wt_ij)^T for j <= i, zero above -- the cut's W as [nt][nt] tiles;  (ti, tj, 1), the window's alone: Ps_ij = (P + P^T) / 2 of the
// leading NA rows of the posterior, zero in the padding
__global__ void __launch_bounds__(kThreads) k_mu_operands(const double* Wt, double* Wn, int nt, const double* P, int64_t ldp, int NA, double* Ps) {
  __shared__ double A[T * LDM];
  const int ti = blockIdx.x, tj = blockIdx.y, tid = threadIdx.x;
  if (blockIdx.z == 0) {
    double* wn = tile_ptr(Wn, nt, ti, tj);
    if (tj <= ti) stage_tile(A, tile_ptr(const_cast<double*>(Wt), nt, ti, tj));
    __syncthreads();
    for (int e = tid; e < T * T; e += kThreads) wn[e] = tj <= ti ? A[(e & 63) * LDM + (e >> 6)] : 0.0;
    return;
  }
  double* ps = tile_ptr(Ps, nt, ti, tj);
  for (int e = tid; e < T * T; e += kThreads) {
    const int gi = T * ti + (e >> 6), gj = T * tj + (e & 63);
    ps[e] = (gi < NA && gj < NA) ? 0.5 * (P[gi * ldp + gj] + P[gj * ldp + gi]) : 0.0;
  }
}

// (ti, tj): G_ij = Cs[rows of tile row i][window columns of tile column j], zero in the padding
__global__ void __launch_bounds__(kThreads) k_mu_gather(MapUpdateDev u) {
  __shared__ double P[T * LDM];
  __shared__ double Q[T * LDM];
  __shared__ int32_t rows[T], cols[T];
  const int ti = blockIdx.x, tj = blockIdx.y, tid = threadIdx.x;
  fill_rows(rows, nullptr, u.od, u.N, ti);
  fill_rows(cols, u.map_idx, u.od, u.NA, tj);
  __syncthreads();
  stage_sym(P, Q, u.map_cov, u.N, rows, cols);
  __syncthreads();
  double* g = tile_ptr(u.G, u.nA, ti, tj);
  for (int e = tid; e < T * T; e += kThreads) g[e] = sym_at(P, Q, e >> 6, e & 63);
}

// C_ij = sum_k A_ik B_jk^T over tiles; kmode 0: k < kn, 1: k <= j, 2: k <= i (the lower triangular W as B, as A).  sym: C = I - sum, the tiles j <= i computed
// and mirrored, a diagonal tile from its lower triangle -- C is symmetric bit for bit.
struct MuGemm { const double* A; const double* B; double* C; int32_t nt, kn, kmode, sym; };
__global__ void __launch_bounds__(kThreads) k_mu_gemm(MuGemm g) {
  __shared__ double A[T * LDM];
  __shared__ double B[T * LDM];
  const int i = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
  if (g.sym && j > i) return;
  const int k1 = g.kmode == 0 ? g.kn : (g.kmode == 1 ? j + 1 : i + 1);
  f64x4 acc[4] = {};
  for (int k = 0; k < k1; ++k) {
    __syncthreads();
    stage_tiles(A, tile_ptr(const_cast<double*>(g.A), g.nt, i, k), B, tile_ptr(const_cast<double*>(g.B), g.nt, j, k));
    __syncthreads();
    tile_abt_mfma(A, B, acc);
  }
  __syncthreads();
  acc_to_lds(A, acc, g.sym ? -1.0 : 1.0);
  __syncthreads();
  double* c_ij = tile_ptr(g.C, g.nt, i, j);
  double* c_ji = tile_ptr(g.C, g.nt, j, i);
  for (int e = tid; e < T * T; e += kThreads) {
    const int r = e >> 6, c = e & 63;
    if (!g.sym) { c_ij[e] = A[r * LDM + c]; continue; }
    if (i == j) c_ij[e] = (r == c ? 1.0 : 0.0) + (c > r ? A[c * LDM + r] : A[r * LDM + c]);
    else { c_ij[e] = A[r * LDM + c]; c_ji[e] = A[c * LDM + r]; }
  }
}

// The hot launch, the downdate every entry ends in: the new map's block C'_ij = Cs[rows_i, rows_j] - sum_k Z_ik Y_jk^T for (ti, tj <= ti), k ascending.  The
// rows of the old map behind the block's n rows are the objects `kept` (the merge: the survivors) or, kept NULL, the rows themselves (the condition and the
// extension: the old map's block of the new one).  Z == Y (the merge): a diagonal tile stages one operand for both.  Written along the rows of both triangles,
// a diagonal tile from its lower half: C' is symmetric bit for bit.
struct MapDowndate {
  const double* Z; const double* Y; int32_t nk;   // [tile rows][nk] tiles each
  const uint32_t* kept; int32_t od, n;            // the block's rows
  int64_t ldc, ldo;
  const double* map_cov; double* out_cov; double* status;
};
__global__ void __launch_bounds__(kThreads) k_map_downdate(MapDowndate d) {
  __shared__ double A[T * LDM];
  __shared__ double B[T * LDM];
  __shared__ int32_t rows_i[T], rows_j[T];
  const int ti = blockIdx.x, tj = blockIdx.y, tid = threadIdx.x;
  if (tj > ti) return;
  fill_rows(rows_i, d.kept, d.od, d.n, ti);
  fill_rows(rows_j, d.kept, d.od, d.n, tj);
  const bool one = ti == tj && d.Z == d.Y;
  f64x4 acc[4] = {};
  for (int k = 0; k < d.nk; ++k) {
    __syncthreads();
    if (!one) stage_tiles(A, tile_ptr(const_cast<double*>(d.Z), d.nk, ti, k), B, tile_ptr(const_cast<double*>(d.Y), d.nk, tj, k));
    else stage_tile(A, tile_ptr(const_cast<double*>(d.Y), d.nk, ti, k));
    __syncthreads();
    tile_abt_mfma(A, one ? A : B, acc);
  }
  __syncthreads();
  stage_sym(A, B, d.map_cov, d.ldc, rows_i, rows_j);   // the old map's two blocks, each along its rows
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6;
  double v[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) v[rt][r] = sym_at(A, B, 16 * rt + (lane >> 4) + 4 * r, 16 * wv + (lane & 15)) - acc[rt][r];
  __syncthreads();
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) A[(16 * rt + (lane >> 4) + 4 * r) * LDM + 16 * wv + (lane & 15)] = v[rt][r];
  __syncthreads();
  if (tile_to_both_triangles(A, d.out_cov, d.ldo, ti, tj, d.n, d.n, 0, ti == tj)) d.status[MS_NONFINITE] = 1.0;
}

// v = W d, d = a - b (b NULL: d = a), W dense and lower triangular, n x n: workgroup b its 64 rows, four threads per row, the dot product split by column mod 4
template <bool DIFF>
__device__ __forceinline__ double wd_part(const double* w, const double* a, const double* b, int part, int row) {
  double s = 0.0;
  for (int c = part; c <= row; c += 4) s += w[c] * (DIFF ? a[c] - b[c] : a[c]);
  return s;
}
__global__ void __launch_bounds__(kThreads) k_map_wd(const double* W, const double* a, const double* b, int n, double* v) {
  const int row = T * blockIdx.x + (threadIdx.x >> 2), part = threadIdx.x & 3;
  double s = 0.0;
  if (row < n) s = b != nullptr ? wd_part<true>(W + (int64_t)row * n, a, b, part, row) : wd_part<false>(W + (int64_t)row * n, a, nullptr, part, row);   // (one loop with the test inside it ran 4 us longer)
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  if (part == 0) v[row] = s;
}
// mu'[row] = mu[its row of the old map] + sign (Y v)[row] on the rows of a downdate: workgroup b its 64 rows
__global__ void __launch_bounds__(kThreads) k_map_mean(MapDowndate d, const double* v, double sign, const double* map_mean, double* out_mean) {
  const int r = threadIdx.x >> 2, part = threadIdx.x & 3, row = T * blockIdx.x + r;
  double s = 0.0;
  for (int k = 0; k < d.nk; ++k) {
    const double* y = tile_ptr(const_cast<double*>(d.Y), d.nk, blockIdx.x, k) + r * T;
    for (int c = part; c < T; c += 4) s += y[c] * v[T * k + c];
  }
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  if (part == 0 && row < d.n) {
    const double x = map_mean[table_row(d.kept, d.od, d.n, row)] + sign * s;
    out_mean[row] = x;
    if (!isfinite(x)) d.status[MS_NONFINITE] = 1.0;
  }
}

// P[od a + r][od b + c] = blocks[a k + b][r][c], pm[od a + r] = objects[obj_idx[a]][r]
__global__ void __launch_bounds__(kThreads) k_mu_posterior_layout(const double* __restrict__ blocks, const double* __restrict__ objects, const uint32_t* __restrict__ obj_idx,
                                                                 int32_t k, int32_t od, double* __restrict__ P, double* __restrict__ pm) {
  const int64_t NA = (int64_t)k * od, e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= NA * NA) return;
  const int64_t i = e / NA, j = e % NA;
  P[e] = blocks[((i / od) * k + j / od) * (od * od) + (i % od) * od + j % od];
  if (j == 0) pm[i] = objects[(int64_t)obj_idx[i / od] * od + i % od];
}

// ==== the map grown by a window's new objects (include/obvi_map_extend.h) ===================================================================================
// row of the new map of row w of the posterior over (A, B): A keeps its map rows, B follows the old map
__device__ __forceinline__ int32_t window_new_row(const MapUpdateDev& u, int w) { return w < u.NA ? table_row(u.map_idx, u.od, u.NA, w) : (w < u.NA + u.NB ? u.N + (w - u.NA) : -1); }

// (bi, aj): Pba_ij = Ps[B rows of tile row i][A columns of tile column j], zero in the padding
__global__ void __launch_bounds__(kThreads) k_mx_stage(MapUpdateDev u) {
  __shared__ double P[T * LDM];
  __shared__ double Q[T * LDM];
  __shared__ int32_t ra[T], rb[T];   // rows of the posterior: A's of tile column j, B's of tile row i
  const int ti = blockIdx.x, tj = blockIdx.y, tid = threadIdx.x;
  fill_rows(ra, nullptr, u.od, u.NA, tj);
  if (tid < T) rb[tid] = T * ti + tid < u.NB ? u.NA + T * ti + tid : -1;
  __syncthreads();
  stage_sym(P, Q, u.P, u.ldp, ra, rb);
  __syncthreads();
  double* t = tile_ptr(u.Pba, u.nA, ti, tj);
  for (int e = tid; e < T * T; e += kThreads) t[e] = sym_at(P, Q, e & 63, e >> 6);   // Ps[A_c][B_r], as the scatter forms it
}

// (ti, tj): X_ij = sum_k Y_ik V_jk^T, k ascending -- rows of tile row i of the old map against the B rows of tile row j; written along the rows of both
// C'[old, B] and C'[B, old]
__global__ void __launch_bounds__(kThreads) k_mx_cross(MapUpdateDev u) {
  __shared__ double A[T * LDM];
  __shared__ double B[T * LDM];
  const int ti = blockIdx.x, tj = blockIdx.y;
  f64x4 acc[4] = {};
  for (int k = 0; k < u.nA; ++k) {
    __syncthreads();
    stage_tiles(A, tile_ptr(u.Y, u.nA, ti, k), B, tile_ptr(u.V, u.nA, tj, k));
    __syncthreads();
    tile_abt_mfma(A, B, acc);
  }
  __syncthreads();
  acc_to_lds(A, acc, 1.0);
  __syncthreads();
  if (tile_to_both_triangles(A, u.out_cov, u.ldo, ti, tj, u.N, u.NB, u.N, false)) u.status[MS_NONFINITE] = 1.0;
}

// (ti, tj) over the tiles of the posterior: the window's whole block of the new map and its means are the posterior itself, (P + P^T) / 2 and pm bit for bit.
// N_B = 0: the condition's scatter.
__global__ void __launch_bounds__(kThreads) k_mx_scatter(MapUpdateDev u) {
  __shared__ double P[T * LDM];
  __shared__ double Q[T * LDM];
  __shared__ int32_t src_i[T], src_j[T], rows[T], cols[T];   // rows of the posterior, and where they go in the new map
  const int ti = blockIdx.x, tj = blockIdx.y, tid = threadIdx.x;
  const int32_t to = tid < 2 * T ? window_new_row(u, T * (tid < T ? ti : tj) + (tid & (T - 1))) : -1;   // asked for first: map_idx arrives beside the tiles
  fill_rows(src_i, nullptr, u.od, u.NA + u.NB, ti);
  fill_rows(src_j, nullptr, u.od, u.NA + u.NB, tj);
  __syncthreads();
  stage_sym(P, Q, u.P, u.ldp, src_i, src_j);
  if (tid < 2 * T) (tid < T ? rows : cols)[tid & (T - 1)] = to;
  __syncthreads();
  bool bad = false;
  for (int e = tid; e < T * T; e += kThreads) {
    const int r = e >> 6, c = e & 63;
    if (rows[r] < 0 || cols[c] < 0) continue;
    const double x = sym_at(P, Q, r, c);
    u.out_cov[(int64_t)rows[r] * u.ldo + cols[c]] = x;
    bad = bad || !isfinite(x);
  }
  if (tj == 0 && tid < T && rows[tid] >= 0) {
    const double x = u.pm[T * ti + tid];
    u.out_mean[rows[tid]] = x;
    bad = bad || !isfinite(x);
  }
  if (bad) u.status[MS_NONFINITE] = 1.0;
}

// the objects idx of a map, in that order: workgroup (64 columns, 64 rows) copies its entries as they are
__global__ void __launch_bounds__(kThreads) k_map_select(const uint32_t* __restrict__ idx, int32_t k, int32_t od, const double* __restrict__ mean, const double* __restrict__ cov,
                                                         int64_t ldc, double* __restrict__ out_mean, double* __restrict__ out_cov) {
  __shared__ int64_t rows[T], cols[T];
  const int tid = threadIdx.x, K = k * od;
  if (tid < 2 * T) {
    const int g = T * (tid < T ? blockIdx.y : blockIdx.x) + (tid & (T - 1));
    (tid < T ? rows : cols)[tid & (T - 1)] = g < K ? (int64_t)idx[g / od] * od + g % od : -1;
  }
  __syncthreads();
  for (int e = tid; e < T * T; e += kThreads) {
    const int r = e >> 6, c = e & 63;
    if (rows[r] >= 0 && cols[c] >= 0) out_cov[(int64_t)(T * blockIdx.y + r) * K + T * blockIdx.x + c] = cov[rows[r] * ldc + cols[c]];
  }
  if (blockIdx.x == 0 && tid < T && rows[tid] >= 0) out_mean[T * blockIdx.y + tid] = mean[rows[tid]];
}

// ==== duplicate objects of the map merged (include/obvi_map_merge.h; MapMergeDev, ba_device.h) ===========================================================
// Under the rules above.  Constraint row w belongs to pair w / od: its two map rows are the drop object's (the cut's map_idx) and the keep object's; -1: padding.

// (ti, tj <= ti): T_ij = Cs[b_i, b_j] - Cs[b_i, k_j] - Cs[k_i, b_j] + Cs[k_i, k_j] + Rs, in that order, every Cs entry by the symmetrised read.  Into the cut's A
// (lower tiles, identity padding) and both triangles of Csym; a diagonal tile is taken from its lower triangle, so T is symmetric bit for bit.  Tile column 0
// also writes its rows of H mu - d into the cut's mean.
__global__ void __launch_bounds__(kThreads) k_mm_innovation(MapMergeDev g) {
  __shared__ double P[T * LDM];
  __shared__ double Qs[T * LDM];
  __shared__ int32_t ri[2][T], rj[2][T];   // [0]: drop rows, [1]: keep rows, of tile rows ti and tj
  const int ti = blockIdx.x, tj = blockIdx.y, tid = threadIdx.x;
  if (tj > ti) return;
  const MapCutGroup G = g.cut.groups[0];
  fill_rows(ri[0], g.cut.map_idx, g.od, g.Q, ti); fill_rows(ri[1], g.keep, g.od, g.Q, ti);
  fill_rows(rj[0], g.cut.map_idx, g.od, g.Q, tj); fill_rows(rj[1], g.keep, g.od, g.Q, tj);
  __syncthreads();
  double t[T * T / kThreads];
#pragma unroll
  for (int x = 0; x < T * T / kThreads; ++x) t[x] = 0.0;
#pragma unroll 1
  for (int term = 0; term < 4; ++term) {   // (drop, drop) - (drop, keep) - (keep, drop) + (keep, keep)
    const double sgn = (term == 1 || term == 2) ? -1.0 : 1.0;
    stage_sym(P, Qs, g.map_cov, g.N, ri[term >> 1], rj[term & 1]);
    __syncthreads();
#pragma unroll
    for (int x = 0; x < T * T / kThreads; ++x) {
      const int e = tid + kThreads * x;
      t[x] += sgn * sym_at(P, Qs, e >> 6, e & 63);
    }
    __syncthreads();
  }
  const int od = g.od;
#pragma unroll
  for (int x = 0; x < T * T / kThreads; ++x) {
    const int e = tid + kThreads * x, r = e >> 6, c = e & 63, gi = T * ti + r, gj = T * tj + c;
    const bool in = gi < G.N && gj < G.N;
    double v = t[x];
    if (in && g.noise != nullptr && gi / od == gj / od) {
      const double* R = g.noise + (int64_t)(gi / od) * od * od;
      v += 0.5 * (R[(gi % od) * od + gj % od] + R[(gj % od) * od + gi % od]);
    }
    P[r * LDM + c] = in ? v : (gi == gj ? 1.0 : 0.0);
  }
  __syncthreads();
  double* tile = tile_ptr(g.cut.A, G.nt, ti, tj);
  double* Cs = g.cut.Csym;
  for (int e = tid; e < T * T; e += kThreads) {
    const int r = e >> 6, c = e & 63, gi = T * ti + r, gj = T * tj + c;
    const double v = (ti == tj && c > r) ? P[c * LDM + r] : P[r * LDM + c];
    tile[e] = v;
    if (gi < G.N && gj < G.N) Cs[(int64_t)gi * G.ld + gj] = v;
  }
  if (ti != tj) {   // the upper triangle of Csym, written along its rows
    for (int e = tid; e < T * T; e += kThreads) {
      const int r = e >> 6, c = e & 63, gj = T * tj + r, gi = T * ti + c;
      if (gi < G.N && gj < G.N) Cs[(int64_t)gj * G.ld + gi] = P[c * LDM + r];
    }
  }
  if (tj == 0 && tid < T && ri[0][tid] >= 0) g.cut.mean[T * ti + tid] = (g.map_mean[ri[0][tid]] - g.map_mean[ri[1][tid]]) - g.offset[T * ti + tid];
}

// (ti, tj): G_ij = Cs[kept rows of tile row i][drop columns of tile column j] - Cs[the same rows][keep columns], zero in the padding; rows in the new map's
// order, so a dropped row is never formed
__global__ void __launch_bounds__(kThreads) k_mm_gather(MapMergeDev g) {
  __shared__ double P[T * LDM];
  __shared__ double Qs[T * LDM];
  __shared__ int32_t rows[T], cols[2][T];
  const int ti = blockIdx.x, tj = blockIdx.y, tid = threadIdx.x;
  fill_rows(rows, g.kept, g.od, g.NK, ti);
  fill_rows(cols[0], g.cut.map_idx, g.od, g.Q, tj); fill_rows(cols[1], g.keep, g.od, g.Q, tj);
  __syncthreads();
  double t[T * T / kThreads];
#pragma unroll
  for (int x = 0; x < T * T / kThreads; ++x) t[x] = 0.0;
#pragma unroll 1
  for (int term = 0; term < 2; ++term) {
    const double sgn = term ? -1.0 : 1.0;
    stage_sym(P, Qs, g.map_cov, g.N, rows, cols[term]);
    __syncthreads();
#pragma unroll
    for (int x = 0; x < T * T / kThreads; ++x) {
      const int e = tid + kThreads * x;
      t[x] += sgn * sym_at(P, Qs, e >> 6, e & 63);
    }
    __syncthreads();
  }
  double* gt = tile_ptr(g.G, g.nQ, ti, tj);
#pragma unroll
  for (int x = 0; x < T * T / kThreads; ++x) gt[tid + kThreads * x] = t[x];
}

// ==== the ordered compaction of the two report entries below: counts per row (or block), one scan, placement ===============================================
// The match compacts its found pairs, the locate its compatible seeds and its qualifying hypotheses, all three through these.

// a workgroup's K counts per thread -> its K sums at out[0 .. K); part: [K][kThreads / 64] in local memory
template <int K>
__device__ __forceinline__ void compact_counts(int32_t (&c)[K], int32_t (*part)[kThreads / 64], int64_t* out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) c[i] += __shfl_xor(c[i], x, 64);
    if ((tid & 63) == 0) part[i][tid >> 6] = c[i];
  }
  __syncthreads();
  if (tid < K) { int64_t sum = 0; for (int w = 0; w < kThreads / 64; ++w) sum += part[tid][w]; out[tid] = sum; }
}

// one workgroup: off[i] = the counts cnt[stride i] of the entries before i, and their sum; part: [kThreads + 1] in local memory
__device__ __forceinline__ int64_t compact_scan(const int64_t* cnt, int stride, int64_t n, int64_t* off, int64_t* part) {
  const int tid = threadIdx.x;
  const int64_t per = (n + kThreads - 1) / kThreads, lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  int64_t c = 0;
  for (int64_t i = lo; i < hi; ++i) c += cnt[stride * i];
  part[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int x = 0; x < kThreads; ++x) { const int64_t v = part[x]; part[x] = run; run += v; }
    part[kThreads] = run;
  }
  __syncthreads();
  int64_t o = part[tid];
  for (int64_t i = lo; i < hi; ++i) { off[i] = o; o += cnt[stride * i]; }
  return part[kThreads];
}

// where a workgroup's hits go: the hits of the threads before this one, and (all) of the whole workgroup; wcnt: [kThreads / 64] in local memory
__device__ __forceinline__ int compact_place(bool hit, int32_t* wcnt, int* all) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint64_t votes = __ballot(hit);
  __syncthreads();
  if (lane == 0) wcnt[wv] = __popcll(votes);
  __syncthreads();
  int before = __popcll(votes & ((1ull << lane) - 1ull));
  *all = 0;
  for (int w = 0; w < kThreads / 64; ++w) { before += w < wv ? wcnt[w] : 0; *all += wcnt[w]; }
  return before;
}

// ==== duplicate objects of the map proposed (include/obvi_map_match.h; MapMatchDev, ba_device.h) ==========================================================
// Under the rules above.  Every count is a sum of integers and every output position comes from the scan of the rows' counts: nothing depends on the order in
// which workgroups run.

// object o: its diagonal block, symmetrised as k_map_gather forms every entry, compacted to [o][od][od]
__global__ void __launch_bounds__(64) k_mt_diag(MapMatchDev m) {
  const int o = blockIdx.x, od = m.od, tid = threadIdx.x;
  const int64_t ldc = (int64_t)m.n * od;
  const double* C = m.map_cov + ((int64_t)o * od) * ldc + (int64_t)o * od;
  for (int e = tid; e < od * od; e += 64) {
    const int r = e / od, c = e % od;
    m.diag[(int64_t)o * od * od + e] = 0.5 * (C[r * ldc + c] + C[c * ldc + r]);
  }
}

// the wrap of a yaw difference: period * rint(dy / period), each operation rounded on its own
__device__ __forceinline__ double match_wrap(double dy, double period) { return period > 0.0 ? __dmul_rn(period, rint(dy / period)) : 0.0; }

// Workgroup (bi, bj >= bi): the pairs (a, b), a < b, of B = 64 / OD objects a of block bi and B objects b of block bj; B OD = 63 rows for both block sizes, so
// the two orientations of the cross block -- C[rows a][columns b] and C[rows b][columns a], both read along their rows -- are the two staged tiles of
// k_map_gather.  One lane per pair: label and distance tests first, then T (lower triangle, in registers; rows outside the mask replaced by the identity),
// its Cholesky with the pivot extremes of k_map_potrf over the rows of the mask, and s = |L^-1 d|^2 by forward substitution beside it.
template <int OD>
__global__ void __launch_bounds__(kThreads) k_mt_pairs(MapMatchDev m) {
  constexpr int B = T / OD, R = B * OD;
  __shared__ double P[T * LDM];   // C[rows of block bi][columns of block bj]
  __shared__ double Q[T * LDM];   // C[rows of block bj][columns of block bi]
  __shared__ double Da[B * OD * OD], Db[B * OD * OD], ma[R], mb[R];
  const int bi = blockIdx.x, bj = blockIdx.y, tid = threadIdx.x;
  if (bj < bi) return;
  const int n = m.n;
  const int na = min(B, n - bi * B), nb = min(B, n - bj * B), ra = na * OD, rb = nb * OD;
  const int64_t ldc = (int64_t)n * OD, row_a = (int64_t)bi * R, row_b = (int64_t)bj * R;
  for (int e = tid; e < T * T; e += kThreads) {
    const int r = e >> 6, c = e & 63;
    P[r * LDM + c] = (r < ra && c < rb) ? m.map_cov[(row_a + r) * ldc + row_b + c] : 0.0;
    Q[r * LDM + c] = (r < rb && c < ra) ? m.map_cov[(row_b + r) * ldc + row_a + c] : 0.0;
  }
  for (int e = tid; e < B * OD * OD; e += kThreads) {
    Da[e] = e < ra * OD ? m.diag[row_a * OD + e] : 0.0;
    Db[e] = e < rb * OD ? m.diag[row_b * OD + e] : 0.0;
  }
  if (tid < R) {
    ma[tid] = tid < ra ? m.map_mean[row_a + tid] : 0.0;
    mb[tid] = tid < rb ? m.map_mean[row_b + tid] : 0.0;
  }
  __syncthreads();
  const int al = tid / B, bl = tid % B, a = bi * B + al, b = bj * B + bl;
  if (al >= na || bl >= nb || a >= b) return;
  bool test = true;
  if (m.label != nullptr) { const int32_t la = m.label[a], lb = m.label[b]; test = la >= 0 && la == lb; }
  if (test && m.use_dist) {
    const double dx = mb[bl * OD] - ma[al * OD], dy = mb[bl * OD + 1] - ma[al * OD + 1], dz = mb[bl * OD + 2] - ma[al * OD + 2];
    test = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)) <= m.dist2;
  }
  double code = kMatchNotTested;
  if (test) {
    double t[OD * (OD + 1) / 2], d[OD], y[OD];
#pragma unroll
    for (int r = 0; r < OD; ++r) d[r] = mb[bl * OD + r] - ma[al * OD + r];
    if (OD == 7) d[3] = __dsub_rn(d[3], match_wrap(d[3], m.period));
#pragma unroll
    for (int r = 0; r < OD; ++r) {
      const bool inr = (m.mask >> r) & 1u;
      d[r] = inr ? d[r] : 0.0;
#pragma unroll
      for (int c = 0; c <= r; ++c) {
        const bool in = inr && ((m.mask >> c) & 1u);
        const double bb = Db[(bl * OD + r) * OD + c], aa = Da[(al * OD + r) * OD + c];
        const double ba = 0.5 * (Q[(bl * OD + r) * LDM + al * OD + c] + P[(al * OD + c) * LDM + bl * OD + r]);
        const double ab = 0.5 * (P[(al * OD + r) * LDM + bl * OD + c] + Q[(bl * OD + c) * LDM + al * OD + r]);
        t[r * (r + 1) / 2 + c] = in ? ((bb - ba) - ab) + aa : (r == c ? 1.0 : 0.0);
      }
    }
    double s = 0.0, pmin = INFINITY, pmax = 0.0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < OD; ++j) {   // left-looking: column j of L, then row j of the forward substitution
#pragma unroll
      for (int k = 0; k < j; ++k) {
        const double ljk = t[j * (j + 1) / 2 + k];
#pragma unroll
        for (int i = j; i < OD; ++i) t[i * (i + 1) / 2 + j] -= t[i * (i + 1) / 2 + k] * ljk;
      }
      const double p = t[j * (j + 1) / 2 + j];
      const bool ok = p > 0.0 && isfinite(p);
      const double dj = sqrt(ok ? p : 1.0);
      if ((m.mask >> j) & 1u) { bad = bad || !ok; pmin = fmin(pmin, dj); pmax = fmax(pmax, dj); }
      double acc = d[j];
#pragma unroll
      for (int k = 0; k < j; ++k) acc -= t[j * (j + 1) / 2 + k] * y[k];
      y[j] = acc / dj;
      s += y[j] * y[j];
#pragma unroll
      for (int i = j + 1; i < OD; ++i) t[i * (i + 1) / 2 + j] /= dj;
    }
    code = (bad || !(pmin * pmin > 1e-13 * pmax * pmax)) ? kMatchSingular : s;
  }
  m.stat[(int64_t)a * n + b] = code;
}

__device__ __forceinline__ bool match_found(double v, double gate) { return v >= 0.0 && v <= gate; }

// row a: its found, tested and singular pairs
__global__ void __launch_bounds__(kThreads) k_mt_count(MapMatchDev m) {
  __shared__ int32_t part[3][kThreads / 64];
  const int a = blockIdx.x, tid = threadIdx.x, n = m.n;
  int32_t c[3] = {0, 0, 0};
  for (int b = a + 1 + tid; b < n; b += kThreads) {
    const double v = m.stat[(int64_t)a * n + b];
    c[0] += match_found(v, m.gate) ? 1 : 0; c[1] += v != kMatchNotTested ? 1 : 0; c[2] += v == kMatchSingular ? 1 : 0;
  }
  compact_counts(c, part, m.row_cnt + 3 * (int64_t)a);
}

// one workgroup: row_off[a] = found pairs of the rows before a, and the three totals
__global__ void __launch_bounds__(kThreads) k_mt_scan(MapMatchDev m) {
  __shared__ int64_t part[kThreads + 1], rest[2][kThreads];
  const int tid = threadIdx.x;
  const int64_t n = m.n, per = (n + kThreads - 1) / kThreads, lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  int64_t t = 0, g = 0;
  for (int64_t a = lo; a < hi; ++a) { t += m.row_cnt[3 * a + 1]; g += m.row_cnt[3 * a + 2]; }
  rest[0][tid] = t; rest[1][tid] = g;
  const int64_t found = compact_scan(m.row_cnt, 3, n, m.row_off, part);   // its barriers stand between the sums above and below
  if (tid == 0) m.totals[0] = found;
  if (tid < 2) {
    int64_t sum = 0;
    for (int x = 0; x < kThreads; ++x) sum += rest[tid][x];
    m.totals[1 + tid] = sum;
  }
}

// row a: its found pairs to their places behind row_off[a], in the order of b, up to `capacity`
__global__ void __launch_bounds__(kThreads) k_mt_scatter(MapMatchDev m) {
  __shared__ int32_t wcnt[kThreads / 64];
  const int a = blockIdx.x, tid = threadIdx.x, n = m.n, od = m.od;
  if (m.row_cnt[3 * (int64_t)a] == 0) return;
  int64_t base = m.row_off[a];
  for (int b0 = a + 1; b0 < n && base < m.capacity; b0 += kThreads) {
    const int b = b0 + tid;
    const double v = b < n ? m.stat[(int64_t)a * n + b] : kMatchNotTested;
    const bool hit = match_found(v, m.gate);
    int all;
    const int before = compact_place(hit, wcnt, &all);
    const int64_t pos = base + before;
    if (hit && pos < m.capacity) {
      m.out_a[pos] = (uint32_t)a; m.out_b[pos] = (uint32_t)b; m.out_stat[pos] = v;
      m.out_yaw[pos] = od == 7 ? match_wrap(m.map_mean[(int64_t)b * od + 3] - m.map_mean[(int64_t)a * od + 3], m.period) : 0.0;
    }
    base += all;
  }
}

// ==== the map moved into another frame under an uncertain transform; two maps joined (include/obvi_map_frame.h; MapFrameDev, ba_device.h) ==================
// Under the rules above: no atomics, no flags between workgroups, every sum in a fixed order.

// The unit quaternion (x y z w) of an axis-angle vector, smooth through zero: (aa sin(th / 2) / th, cos(th / 2)), by series in th^2 below th = 1e-3 (the next
// terms are under 1e-22).  The estimator's own rotation (dual_forward_rotation) is a constant at and below 1e-8, which is right for a residual and wrong for
// the derivative a covariance is pushed through.
template <int N> __device__ __forceinline__ void frame_quat(const Dual<N>* aa, Dual<N>* q) {
  typedef Dual<N> D;
  const D t2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  D k, w;
  if (t2.v > 1e-6) {
    const D t = dsqrt(t2), half = t * 0.5;
    k = dsin(half) / t; w = dcos(half);
  } else {
    k = D(0.5) - t2 * (1.0 / 48.0) + t2 * t2 * (1.0 / 3840.0);
    w = D(1.0) - t2 * (1.0 / 8.0) + t2 * t2 * (1.0 / 384.0);
  }
  q[0] = k * aa[0]; q[1] = k * aa[1]; q[2] = k * aa[2]; q[3] = w;
}
// The rotation log of a unit quaternion, angle in [0, pi] -- the convention of relpose_eval_n (ba_math.h): 2 atan2(|v|, |w|) v / |v|, negated where w < 0 --
// and smooth through the identity: below |v| = 1e-3 |w| the series of atan in (|v| / w)^2.
template <int N> __device__ __forceinline__ void frame_quat_log(const Dual<N>* q, Dual<N>* aa) {
  typedef Dual<N> D;
  const D n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2], w = dabs(q[3]);
  D scale;
  if (n2.v > 1e-6 * w.v * w.v) {
    const D n = dsqrt(n2);
    scale = datan2(n, w) * 2.0 / n;
  } else {
    const D x2 = n2 / (w * w);
    scale = (D(2.0) / w) * (D(1.0) - x2 * (1.0 / 3.0) + x2 * x2 * (1.0 / 5.0) - x2 * x2 * x2 * (1.0 / 7.0));
  }
  if (q[3].v < 0.0) scale = -scale;
  for (int i = 0; i < 3; ++i) aa[i] = scale * q[i];
}

// One lane per object: mu'_o, Jk_o (the K x K block of J_o that is not the identity), the K moving rows of G_o, and GS_o = G_o Sigma_s (sums over the
// transform's parameters in their order).  A non-finite mean sets the flag of the status record.
template <int OD>
__global__ void __launch_bounds__(64) k_mf_jac(MapFrameDev f) {
  constexpr int K = OD - 3, DT = OD == 7 ? 4 : 6;
  const int o = blockIdx.x * 64 + threadIdx.x;
  if (o >= f.n) return;
  const double* m = f.map_mean + (int64_t)o * OD;
  double mu[OD], J[K * K], G[K * DT];
  for (int i = 0; i < K * K; ++i) J[i] = 0.0;
  for (int i = 0; i < K * DT; ++i) G[i] = 0.0;
  for (int i = 0; i < 3; ++i) { mu[OD - 3 + i] = m[OD - 3 + i]; G[i * DT + i] = 1.0; }
  if (OD == 7) {   // p' = Rz(psi) p + t, yaw' = yaw + psi
    const double psi = f.transform[3], c = cos(psi), s = sin(psi), x = m[0], y = m[1];
    mu[0] = c * x - s * y + f.transform[0]; mu[1] = s * x + c * y + f.transform[1]; mu[2] = m[2] + f.transform[2]; mu[3] = m[3] + psi;
    J[0] = c; J[1] = -s; J[K] = s; J[K + 1] = c; J[2 * K + 2] = 1.0; J[3 * K + 3] = 1.0;
    G[3] = -s * x - c * y; G[DT + 3] = c * x - s * y; G[3 * DT + 3] = 1.0;   // Rz'(psi) p in the centre rows, the yaw row
  } else {         // p' = R_T p + t, aa' = Log(R_T Exp(aa)); directions 0..2: the transform's axis-angle, 3..5: the object's
    typedef Dual<6> D;
    D a[3], aa[3], qt[4], qo[4], q[4], lg[3];
    for (int i = 0; i < 3; ++i) { a[i] = dvar<6>(f.transform[3 + i], i); aa[i] = dvar<6>(m[3 + i], 3 + i); }
    frame_quat(a, qt); frame_quat(aa, qo);
    q[3] = qt[3] * qo[3] - (qt[0] * qo[0] + qt[1] * qo[1] + qt[2] * qo[2]);
    q[0] = qt[3] * qo[0] + qo[3] * qt[0] + (qt[1] * qo[2] - qt[2] * qo[1]);
    q[1] = qt[3] * qo[1] + qo[3] * qt[1] + (qt[2] * qo[0] - qt[0] * qo[2]);
    q[2] = qt[3] * qo[2] + qo[3] * qt[2] + (qt[0] * qo[1] - qt[1] * qo[0]);
    frame_quat_log(q, lg);
    const D x = qt[0], y = qt[1], z = qt[2], w = qt[3];
    const D R[9] = {D(1.0) - (y * y + z * z) * 2.0, (x * y - z * w) * 2.0, (x * z + y * w) * 2.0,
                    (x * y + z * w) * 2.0, D(1.0) - (x * x + z * z) * 2.0, (y * z - x * w) * 2.0,
                    (x * z - y * w) * 2.0, (y * z + x * w) * 2.0, D(1.0) - (x * x + y * y) * 2.0};
    for (int i = 0; i < 3; ++i) {
      const D p = R[3 * i] * m[0] + R[3 * i + 1] * m[1] + R[3 * i + 2] * m[2];
      mu[i] = p.v + f.transform[i]; mu[3 + i] = lg[i].v;
      for (int j = 0; j < 3; ++j) {
        J[i * K + j] = R[3 * i + j].v; J[(3 + i) * K + 3 + j] = lg[i].d[3 + j];
        G[i * DT + 3 + j] = p.d[j]; G[(3 + i) * DT + 3 + j] = lg[i].d[j];
      }
    }
  }
  bool bad = false;
  for (int i = 0; i < OD; ++i) { f.out_mean[(int64_t)o * OD + i] = mu[i]; bad = bad || !isfinite(mu[i]); }
  for (int i = 0; i < K * K; ++i) f.J[(int64_t)o * K * K + i] = J[i];
  if (f.has_sigma) {
    for (int r = 0; r < K; ++r)
      for (int t = 0; t < DT; ++t) {
        double acc = 0.0;
        for (int u = 0; u < DT; ++u) acc += G[r * DT + u] * f.sigma[u * DT + t];
        f.G[((int64_t)o * K + r) * DT + t] = G[r * DT + t];
        f.GS[((int64_t)o * K + r) * DT + t] = acc;
      }
  }
  if (bad) f.status[MS_NONFINITE] = 1.0;
}

// Workgroup (bi, bj >= bi): the block pairs (a, b) of B = 64 / OD objects a of block bi and B objects b of block bj -- the object-aligned blocking of
// k_mt_pairs, 63 rows for both block sizes -- with both orientations of the cross block staged by stage_sym and met in P: P = Cs[rows a][columns b].  Thread
// (r, c) forms entry (r, c) of  J_a Cs_ab J_b^T + GS_a G_b^T  with J = blockdiag(Jk, I3): the inner sum over the columns of b first, then the sum over the rows
// of a, then the transform's term summed over its parameters in their order and added last; an entry whose row and column are both dimensions is Cs itself.
// The result meets in Q and leaves along the rows of both triangles, a diagonal block from its lower triangle: C' is symmetric bit for bit.  C is read once,
// C' written once.
template <int OD>
__global__ void __launch_bounds__(kThreads) k_mf_cov(MapFrameDev f) {
  constexpr int B = T / OD, R = B * OD, K = OD - 3, DT = OD == 7 ? 4 : 6, X = T * T / kThreads;
  __shared__ double P[T * LDM];
  __shared__ double Q[T * LDM];
  __shared__ double Ja[B * K * K], Jb[B * K * K], GSa[B * K * DT], Gb[B * K * DT];
  __shared__ int32_t rows_a[T], rows_b[T];
  const int bi = blockIdx.x, bj = blockIdx.y, tid = threadIdx.x;
  if (bj < bi) return;
  const int n = f.n;
  const int na = min(B, n - bi * B), nb = min(B, n - bj * B), ra = na * OD, rb = nb * OD;
  const int64_t ldc = (int64_t)n * OD, row_a = (int64_t)bi * R, row_b = (int64_t)bj * R;
  if (tid < T) { rows_a[tid] = tid < ra ? (int32_t)row_a + tid : -1; rows_b[tid] = tid < rb ? (int32_t)row_b + tid : -1; }
  for (int e = tid; e < B * K * K; e += kThreads) {
    Ja[e] = e < na * K * K ? f.J[(int64_t)bi * B * K * K + e] : 0.0;
    Jb[e] = e < nb * K * K ? f.J[(int64_t)bj * B * K * K + e] : 0.0;
  }
  if (f.has_sigma) {
    for (int e = tid; e < B * K * DT; e += kThreads) {
      GSa[e] = e < na * K * DT ? f.GS[(int64_t)bi * B * K * DT + e] : 0.0;
      Gb[e] = e < nb * K * DT ? f.G[(int64_t)bj * B * K * DT + e] : 0.0;
    }
  }
  __syncthreads();
  stage_sym(P, Q, f.map_cov, ldc, rows_a, rows_b);
  __syncthreads();
#pragma unroll
  for (int x = 0; x < X; ++x) {   // each thread symmetrises its own entries of P; Q is only read
    const int e = tid + kThreads * x, r = e >> 6, c = e & 63;
    P[r * LDM + c] = sym_at(P, Q, r, c);
  }
  __syncthreads();
#pragma unroll 1
  for (int x = 0; x < X; ++x) {
    const int e = tid + kThreads * x, r = e >> 6, c = e & 63;
    double v = 0.0;
    if (r < ra && c < rb) {
      const int al = r / OD, ri = r - al * OD, bl = c / OD, ci = c - bl * OD;
      const double* Sab = P + (al * OD) * LDM + bl * OD;   // Cs of the object pair (al, bl)
      const double* ja = Ja + (al * K + ri) * K;
      const double* jb = Jb + (bl * K + ci) * K;
      if (ri >= K && ci >= K) {
        v = P[r * LDM + c];
      } else if (ri >= K) {
#pragma unroll
        for (int l = 0; l < K; ++l) v += P[r * LDM + bl * OD + l] * jb[l];
      } else if (ci >= K) {
#pragma unroll
        for (int k = 0; k < K; ++k) v += ja[k] * P[(al * OD + k) * LDM + c];
      } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          double w = 0.0;
#pragma unroll
          for (int l = 0; l < K; ++l) w += Sab[k * LDM + l] * jb[l];
          v += ja[k] * w;
        }
        if (f.has_sigma) {
          double g = 0.0;
#pragma unroll
          for (int t = 0; t < DT; ++t) g += GSa[(al * K + ri) * DT + t] * Gb[(bl * K + ci) * DT + t];
          v += g;
        }
      }
    }
    Q[r * LDM + c] = v;
  }
  __syncthreads();
  bool bad = false;
  for (int e = tid; e < T * T; e += kThreads) {
    const int r = e >> 6, c = e & 63;
    if (r < ra && c < rb) {
      const double x = (bi == bj && c > r) ? Q[c * LDM + r] : Q[r * LDM + c];
      f.out_cov[(row_a + r) * ldc + row_b + c] = x;
      bad = bad || !isfinite(x);
    }
    if (bi != bj && r < rb && c < ra) f.out_cov[(row_b + r) * ldc + row_a + c] = Q[c * LDM + r];
  }
  if (bad) f.status[MS_NONFINITE] = 1.0;
}

// Row blockIdx.y, 256 columns of it: the entry of blockdiag(A, B), copied as the device holds it; row 0's workgroups also copy the means
__global__ void __launch_bounds__(kThreads) k_mf_join(int64_t na, const double* __restrict__ mean_a, const double* __restrict__ cov_a, int64_t nb, const double* __restrict__ mean_b,
                                                      const double* __restrict__ cov_b, double* __restrict__ out_mean, double* __restrict__ out_cov) {
  const int64_t n = na + nb, j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
    double v = 0.0;
    if (i < na && j < na) v = cov_a[i * na + j];
    else if (i >= na && j >= na) v = cov_b[(i - na) * nb + (j - na)];
    out_cov[i * n + j] = v;
  }
  if (blockIdx.y == 0) out_mean[j] = j < na ? mean_a[j] : mean_b[j - na];
}

// ==== one map located in another from the constellations of their object centres (include/obvi_map_locate.h; MapLocateDev, ba_device.h) =================
// Under the rules above.  Every count is a sum of integers, every output position comes from a scan of counts or from a rank that is a count, and the sums
// of the refinement run down one lane's objects and then through wave_sum: nothing depends on the order in which workgroups run.  What the scoring and the
// refining kernel must agree on bit for bit -- the seed's transform, a pair's statistic -- is formed by the same functions with contraction off.

// object o of either map (A's first): centre, the lower triangle of its symmetrised centre block, its label (no labels: 0)
__global__ void __launch_bounds__(64) k_ml_stage(MapLocateDev m) {
  const int o = blockIdx.x * 64 + threadIdx.x;
  if (o >= m.na + m.nb) return;
  const bool in_a = o < m.na;
  const int i = in_a ? o : o - m.na;
  const int64_t ld = (int64_t)(in_a ? m.na : m.nb) * m.od;
  const double* mu = (in_a ? m.mean_a : m.mean_b) + (int64_t)i * m.od;
  const double* C = (in_a ? m.cov_a : m.cov_b) + ((int64_t)i * m.od) * ld + (int64_t)i * m.od;
  double* r = m.rec + (int64_t)o * kLocateRec;
  r[0] = mu[0]; r[1] = mu[1]; r[2] = mu[2];
  r[3] = 0.5 * (C[0] + C[0]);
  r[4] = 0.5 * (C[ld] + C[1]); r[5] = 0.5 * (C[ld + 1] + C[ld + 1]);
  r[6] = 0.5 * (C[2 * ld] + C[2]); r[7] = 0.5 * (C[2 * ld + 1] + C[ld + 2]); r[8] = 0.5 * (C[2 * ld + 2] + C[2 * ld + 2]);
  r[9] = 0.0; r[10] = 0.0; r[11] = 0.0;
  m.lab[o] = in_a ? (m.has_label_a ? m.label_a[i] : 0) : (m.has_label_b ? m.label_b[i] : 0);
}

// a seed: 0 not tested (labels), 1 tested, 2 compatible; every operation rounded on its own, as in k_mt_pairs' distance test
__device__ __forceinline__ int ml_seed_test(const double* pa1, const double* pa2, const double* pb1, const double* pb2, int la1, int la2, int lb1, int lb2, double dmin, double tol) {
  if (!(la1 >= 0 && la1 == lb1 && la2 >= 0 && la2 == lb2)) return 0;
  const double ux = __dsub_rn(pa2[0], pa1[0]), uy = __dsub_rn(pa2[1], pa1[1]), vx = __dsub_rn(pb2[0], pb1[0]), vy = __dsub_rn(pb2[1], pb1[1]);
  const double nu = sqrt(__dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy))), nv = sqrt(__dadd_rn(__dmul_rn(vx, vx), __dmul_rn(vy, vy)));
  const double dz = __dsub_rn(__dsub_rn(pa2[2], pa1[2]), __dsub_rn(pb2[2], pb1[2]));
  return (nu >= dmin && nv >= dmin && fabs(__dsub_rn(nu, nv)) <= tol && fabs(dz) <= tol) ? 2 : 1;
}
// its transform (tx ty tz psi)
__device__ __forceinline__ void ml_hypothesis(const double* pa1, const double* pa2, const double* pb1, const double* pb2, double* T) {
  const double ux = __dsub_rn(pa2[0], pa1[0]), uy = __dsub_rn(pa2[1], pa1[1]), vx = __dsub_rn(pb2[0], pb1[0]), vy = __dsub_rn(pb2[1], pb1[1]);
  const double psi = atan2(__dsub_rn(__dmul_rn(vx, uy), __dmul_rn(vy, ux)), __dadd_rn(__dmul_rn(vx, ux), __dmul_rn(vy, uy)));
  const double c = cos(psi), s = sin(psi);
  const double ax = __dmul_rn(0.5, __dadd_rn(pa1[0], pa2[0])), ay = __dmul_rn(0.5, __dadd_rn(pa1[1], pa2[1])), az = __dmul_rn(0.5, __dadd_rn(pa1[2], pa2[2]));
  const double bx = __dmul_rn(0.5, __dadd_rn(pb1[0], pb2[0])), by = __dmul_rn(0.5, __dadd_rn(pb1[1], pb2[1])), bz = __dmul_rn(0.5, __dadd_rn(pb1[2], pb2[2]));
  T[0] = __dsub_rn(ax, __dsub_rn(__dmul_rn(c, bx), __dmul_rn(s, by)));
  T[1] = __dsub_rn(ay, __dadd_rn(__dmul_rn(s, bx), __dmul_rn(c, by)));
  T[2] = __dsub_rn(az, bz);
  T[3] = psi;
}
// the lower triangle (00 10 11 20 21 22) of Rz B Rz^T from B's
__device__ __forceinline__ void ml_rotate_block(const double* B, double c, double s, double* R) {
#pragma clang fp contract(off)
  const double m00 = c * B[0] - s * B[1], m01 = c * B[1] - s * B[2], m10 = s * B[0] + c * B[1], m11 = s * B[1] + c * B[2];
  R[0] = m00 * c - m01 * s; R[1] = m10 * c - m11 * s; R[2] = m10 * s + m11 * c;
  R[3] = B[3] * c - B[4] * s; R[4] = B[3] * s + B[4] * c; R[5] = B[5];
}
// S = A + R = L L^T by the unrolled Cholesky with k_map_potrf's pivot rule -- a select, never a branch -- and the pivot test of k_mt_pairs; false: singular
__device__ __forceinline__ bool ml_factor(const double* A, const double* R, double* L, double* d) {
#pragma clang fp contract(off)
  const double s00 = A[0] + R[0], s10 = A[1] + R[1], s11 = A[2] + R[2], s20 = A[3] + R[3], s21 = A[4] + R[4], s22 = A[5] + R[5];
  const bool ok0 = s00 > 0.0 && isfinite(s00);
  d[0] = sqrt(ok0 ? s00 : 1.0);
  L[0] = s10 / d[0]; L[1] = s20 / d[0];
  const double p1 = s11 - L[0] * L[0];
  const bool ok1 = p1 > 0.0 && isfinite(p1);
  d[1] = sqrt(ok1 ? p1 : 1.0);
  L[2] = (s21 - L[1] * L[0]) / d[1];
  const double p2 = (s22 - L[1] * L[1]) - L[2] * L[2];
  const bool ok2 = p2 > 0.0 && isfinite(p2);
  d[2] = sqrt(ok2 ? p2 : 1.0);
  const double pmin = fmin(d[0], fmin(d[1], d[2])), pmax = fmax(d[0], fmax(d[1], d[2]));
  return ok0 && ok1 && ok2 && pmin * pmin > 1e-13 * pmax * pmax;
}
// y = L^-1 e
__device__ __forceinline__ void ml_forward(const double* L, const double* d, double e0, double e1, double e2, double* y) {
#pragma clang fp contract(off)
  y[0] = e0 / d[0];
  y[1] = (e1 - L[0] * y[0]) / d[1];
  y[2] = ((e2 - L[1] * y[0]) - L[2] * y[1]) / d[2];
}
// object b of B under (T, c = cos psi, s = sin psi): the smallest statistic over the objects of A that carry its label, and which one (-1: none)
__device__ __forceinline__ int ml_partner(const double* rec, const int32_t* lab, int na, int b, const double* T, double c, double s, double* best_out) {
#pragma clang fp contract(off)
  const int32_t lb = lab[na + b];
  double best = INFINITY;
  int who = -1;
  if (lb >= 0) {
    const double* pb = rec + (int64_t)(na + b) * kLocateRec;
    const double qx = (c * pb[0] - s * pb[1]) + T[0], qy = (s * pb[0] + c * pb[1]) + T[1], qz = pb[2] + T[2];
    double R[6];
    ml_rotate_block(pb + 3, c, s, R);
    for (int a = 0; a < na; ++a) {
      if (lab[a] != lb) continue;
      const double* pa = rec + (int64_t)a * kLocateRec;
      double L[3], d[3], y[3];
      const bool ok = ml_factor(pa + 3, R, L, d);
      ml_forward(L, d, pa[0] - qx, pa[1] - qy, pa[2] - qz, y);
      const double st = (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2];
      if (ok && st < best) { best = st; who = a; }
    }
  }
  *best_out = best;
  return who;
}

// row (a1, a2) of the na x na square: its tested and its compatible seeds
__global__ void __launch_bounds__(kThreads) k_ml_count(MapLocateDev m) {
  __shared__ int32_t part[2][kThreads / 64];
  const int a1 = blockIdx.y, a2 = blockIdx.x, tid = threadIdx.x, na = m.na, nb = m.nb;
  int32_t c[2] = {0, 0};
  if (a1 < a2) {
    const double* pa1 = m.rec + (int64_t)a1 * kLocateRec; const double* pa2 = m.rec + (int64_t)a2 * kLocateRec;
    const int32_t la1 = m.lab[a1], la2 = m.lab[a2];
    for (int j = tid; j < nb * nb; j += kThreads) {
      const int b1 = j / nb, b2 = j - b1 * nb;
      if (b1 == b2) continue;
      const int code = ml_seed_test(pa1, pa2, m.rec + (int64_t)(na + b1) * kLocateRec, m.rec + (int64_t)(na + b2) * kLocateRec, la1, la2, m.lab[na + b1], m.lab[na + b2], m.dmin, m.tol);
      c[0] += code >= 1 ? 1 : 0; c[1] += code == 2 ? 1 : 0;
    }
  }
  compact_counts(c, part, m.row_cnt + 2 * ((int64_t)a1 * na + a2));
}

// one workgroup: row_off[row] = compatible seeds of the rows before it, and the totals
__global__ void __launch_bounds__(kThreads) k_ml_scan(MapLocateDev m) {
  __shared__ int64_t part[kThreads + 1], tested[kThreads];
  const int tid = threadIdx.x;
  const int64_t rows = (int64_t)m.na * m.na, per = (rows + kThreads - 1) / kThreads, lo = tid * per < rows ? tid * per : rows, hi = lo + per < rows ? lo + per : rows;
  int64_t t = 0;
  for (int64_t i = lo; i < hi; ++i) t += m.row_cnt[2 * i];
  tested[tid] = t;
  const int64_t compatible = compact_scan(m.row_cnt + 1, 2, rows, m.row_off, part);
  if (tid == 0) {
    int64_t sum = 0;
    for (int x = 0; x < kThreads; ++x) sum += tested[x];
    m.totals[0] = sum; m.totals[1] = compatible; m.totals[2] = 0;
  }
}

// row (a1, a2): its compatible seeds to their places behind row_off, in the order of (b1, b2)
__global__ void __launch_bounds__(kThreads) k_ml_scatter(MapLocateDev m) {
  __shared__ int32_t wcnt[kThreads / 64];
  const int a1 = blockIdx.y, a2 = blockIdx.x, tid = threadIdx.x, na = m.na, nb = m.nb;
  const int64_t row = (int64_t)a1 * na + a2;
  if (a1 >= a2 || m.totals[1] > m.seed_cap || m.row_cnt[2 * row + 1] == 0) return;
  const double* pa1 = m.rec + (int64_t)a1 * kLocateRec; const double* pa2 = m.rec + (int64_t)a2 * kLocateRec;
  const int32_t la1 = m.lab[a1], la2 = m.lab[a2];
  int64_t base = m.row_off[row];
  for (int j0 = 0; j0 < nb * nb; j0 += kThreads) {
    const int j = j0 + tid, b1 = j / nb, b2 = j - b1 * nb;
    const bool hit = j < nb * nb && b1 != b2 &&
                     ml_seed_test(pa1, pa2, m.rec + (int64_t)(na + b1) * kLocateRec, m.rec + (int64_t)(na + b2) * kLocateRec, la1, la2, m.lab[na + b1], m.lab[na + b2], m.dmin, m.tol) == 2;
    int all;
    const int before = compact_place(hit, wcnt, &all);
    if (hit) { uint32_t* sd = m.seeds + 4 * (base + before); sd[0] = (uint32_t)a1; sd[1] = (uint32_t)a2; sd[2] = (uint32_t)b1; sd[3] = (uint32_t)b2; }
    base += all;
  }
}

// The hot launch.  Both maps' records and labels in local memory (all of it dynamic: 100 bytes an object, 80 KiB at the object limit, two workgroups a
// compute unit).  kLocateLanes neighbouring lanes share a hypothesis: lane g walks the objects b = g, g + 16, ... of B and, for each, every a -- all lanes read
// the same record of A at the same time, a broadcast -- and after each round the sixteen minima go round the group in ascending b, so every lane of the group
// forms the same count and the same sum, in the order the header states.  (One lane a hypothesis left a 200 x 60 search with its 2 860 hypotheses on twelve
// compute units for 5.8 ms.)
constexpr int kLocateLanes = 16;
__global__ void __launch_bounds__(kThreads) k_ml_score(MapLocateDev m) {
  extern __shared__ __attribute__((aligned(16))) char ml_lds[];
  const int64_t H = m.totals[1];
  if (H > m.seed_cap || (int64_t)blockIdx.x * (kThreads / kLocateLanes) >= H) return;
  const int n = m.na + m.nb, na = m.na, nb = m.nb, tid = threadIdx.x, g = tid % kLocateLanes;
  double* rec = reinterpret_cast<double*>(ml_lds);
  int32_t* lab = reinterpret_cast<int32_t*>(rec + (int64_t)n * kLocateRec);
  for (int e = tid; e < n * kLocateRec; e += kThreads) rec[e] = m.rec[e];
  for (int e = tid; e < n; e += kThreads) lab[e] = m.lab[e];
  __syncthreads();
  const int64_t h = (int64_t)blockIdx.x * (kThreads / kLocateLanes) + tid / kLocateLanes;
  if (h >= H) return;   // whole groups leave: the exchanges below stay inside a group
  const uint32_t* sd = m.seeds + 4 * h;
  double T[4];
  ml_hypothesis(rec + sd[0] * kLocateRec, rec + sd[1] * kLocateRec, rec + (na + sd[2]) * kLocateRec, rec + (na + sd[3]) * kLocateRec, T);
  const double c = cos(T[3]), s = sin(T[3]);
  int32_t inl = 0;
  double cost = 0.0;
  for (int b0 = 0; b0 < nb; b0 += kLocateLanes) {
    double best = INFINITY;
    if (b0 + g < nb) ml_partner(rec, lab, na, b0 + g, T, c, s, &best);
#pragma unroll
    for (int x = 0; x < kLocateLanes; ++x) {
      const double v = __shfl(best, x, kLocateLanes);
      if (v <= m.gate) { ++inl; cost += v; }
    }
  }
  if (g == 0) { m.inl[h] = inl; m.cost[h] = cost; }
}

// 256 hypotheses: how many qualify
__device__ __forceinline__ bool ml_qualifies(const MapLocateDev& m, int64_t h) { const int64_t H = m.totals[1]; return H <= m.seed_cap && h < H && m.inl[h] >= m.min_inliers; }
__global__ void __launch_bounds__(kThreads) k_ml_qcount(MapLocateDev m) {
  __shared__ int32_t wcnt[kThreads / 64];
  int all;
  compact_place(ml_qualifies(m, (int64_t)blockIdx.x * kThreads + threadIdx.x), wcnt, &all);
  if (threadIdx.x == 0) m.blk_cnt[blockIdx.x] = all;
}
__global__ void __launch_bounds__(kThreads) k_ml_qscan(MapLocateDev m) {
  __shared__ int64_t part[kThreads + 1];
  const int64_t found = compact_scan(m.blk_cnt, 1, (m.seed_cap + kThreads - 1) / kThreads, m.blk_off, part);
  if (threadIdx.x == 0) m.totals[2] = found;
}
// ... and their numbers, in ascending order
__global__ void __launch_bounds__(kThreads) k_ml_qscatter(MapLocateDev m) {
  __shared__ int32_t wcnt[kThreads / 64];
  const int64_t h = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool hit = ml_qualifies(m, h);
  int all;
  const int before = compact_place(hit, wcnt, &all);
  if (hit) m.qlist[m.blk_off[blockIdx.x] + before] = (uint32_t)h;
}

// The rank of a qualifying hypothesis is the number of those that precede it -- more inliers, then the lower cost, then the lower seed index (the hypothesis
// number: the seeds were compacted in that order) -- a count, whatever order the workgroups run in.  The first `out` ranks are the report.
__global__ void __launch_bounds__(kThreads) k_ml_rank(MapLocateDev m) {
  __shared__ int32_t ki[kThreads];
  __shared__ double kc[kThreads];
  __shared__ uint32_t kh[kThreads];
  const int tid = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * kThreads + tid;
  const bool valid = q < m.found;
  const uint32_t mh = valid ? m.qlist[q] : 0u;
  const int32_t mi = valid ? m.inl[mh] : 0;
  const double mc = valid ? m.cost[mh] : 0.0;
  int64_t before = 0;
  for (int64_t t0 = 0; t0 < m.found; t0 += kThreads) {
    __syncthreads();
    const int64_t j = t0 + tid;
    const uint32_t hh = j < m.found ? m.qlist[j] : 0u;
    ki[tid] = j < m.found ? m.inl[hh] : -1; kc[tid] = j < m.found ? m.cost[hh] : 0.0; kh[tid] = hh;
    __syncthreads();
    for (int x = 0; x < kThreads; ++x) {
      const int32_t i = ki[x];
      const double cx = kc[x];
      before += (i > mi || (i == mi && (cx < mc || (cx == mc && kh[x] < mh)))) ? 1 : 0;
    }
  }
  if (valid && before < m.out) m.sel[before] = mh;
}

// One wavefront per reported hypothesis: the partners (lane l: objects l, l + 64, ... of B), then the Gauss-Newton steps on the inliers with the partners held,
// H (lower triangle, ten sums) and g (four) down each lane's objects and through wave_sum, the 4 x 4 solve on every lane alike.
__global__ void __launch_bounds__(64) k_ml_refine(MapLocateDev m) {
  const int r = blockIdx.x, lane = threadIdx.x, na = m.na, nb = m.nb;
  const uint32_t hh = m.sel[r];
  const uint32_t* sd = m.seeds + 4 * (int64_t)hh;
  double T[4];
  ml_hypothesis(m.rec + sd[0] * kLocateRec, m.rec + sd[1] * kLocateRec, m.rec + (na + sd[2]) * kLocateRec, m.rec + (na + sd[3]) * kLocateRec, T);
  int32_t* pr = m.out_partner + (int64_t)r * nb;
  {
    const double c = cos(T[3]), s = sin(T[3]);
    for (int b = lane; b < nb; b += 64) {
      double best;
      const int who = ml_partner(m.rec, m.lab, na, b, T, c, s, &best);
      pr[b] = best <= m.gate ? who : -1;
    }
  }
  double Hi[10];   // the lower triangle of H^-1, row by row
  for (int it = 0; it <= m.iterations; ++it) {
    const double c = cos(T[3]), s = sin(T[3]);
    double acc[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) acc[i] = 0.0;
    for (int b = lane; b < nb; b += 64) {
      const int a = pr[b];
      if (a < 0) continue;
      const double* pb = m.rec + (int64_t)(na + b) * kLocateRec; const double* pa = m.rec + (int64_t)a * kLocateRec;
      double R[6], L[3], d[3], y[3], z[4][3];
      ml_rotate_block(pb + 3, c, s, R);
      if (!ml_factor(pa + 3, R, L, d)) continue;
      ml_forward(L, d, pa[0] - ((c * pb[0] - s * pb[1]) + T[0]), pa[1] - ((s * pb[0] + c * pb[1]) + T[1]), pa[2] - (pb[2] + T[2]), y);
      ml_forward(L, d, 1.0, 0.0, 0.0, z[0]); ml_forward(L, d, 0.0, 1.0, 0.0, z[1]); ml_forward(L, d, 0.0, 0.0, 1.0, z[2]);
      ml_forward(L, d, -s * pb[0] - c * pb[1], c * pb[0] - s * pb[1], 0.0, z[3]);   // Rz'(psi) p_b
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int l = 0; l <= k; ++l) acc[k * (k + 1) / 2 + l] += (z[k][0] * z[l][0] + z[k][1] * z[l][1]) + z[k][2] * z[l][2];
        acc[10 + k] += (z[k][0] * y[0] + z[k][1] * y[1]) + z[k][2] * y[2];
      }
    }
#pragma unroll
    for (int i = 0; i < 14; ++i) acc[i] = wave_sum(acc[i]);
    // H = L L^T in place (the pivot rule again), then W = L^-1 and H^-1 = W^T W
    double W[10];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int k = 0; k < j; ++k) {
        const double ljk = acc[j * (j + 1) / 2 + k];
#pragma unroll
        for (int i = j; i < 4; ++i) acc[i * (i + 1) / 2 + j] -= acc[i * (i + 1) / 2 + k] * ljk;
      }
      const double p = acc[j * (j + 1) / 2 + j];
      const double dj = sqrt((p > 0.0 && isfinite(p)) ? p : 1.0);
      acc[j * (j + 1) / 2 + j] = dj;
#pragma unroll
      for (int i = j + 1; i < 4; ++i) acc[i * (i + 1) / 2 + j] /= dj;
    }
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {   // column cc of W, rows cc .. 3
#pragma unroll
      for (int i = cc; i < 4; ++i) {
        double sum = i == cc ? 1.0 : 0.0;
#pragma unroll
        for (int k = cc; k < i; ++k) sum -= acc[i * (i + 1) / 2 + k] * W[k * (k + 1) / 2 + cc];
        W[i * (i + 1) / 2 + cc] = sum / acc[i * (i + 1) / 2 + i];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double sum = 0.0;
#pragma unroll
        for (int k = i; k < 4; ++k) sum += W[k * (k + 1) / 2 + i] * W[k * (k + 1) / 2 + j];
        Hi[i * (i + 1) / 2 + j] = sum;
      }
    }
    if (it < m.iterations) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) sum += Hi[i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i] * acc[10 + j];
        T[i] += sum;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      m.out_seed[4 * (int64_t)r + i] = sd[i];
      m.out_T[4 * (int64_t)r + i] = T[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) m.out_cov[16 * (int64_t)r + 4 * i + j] = Hi[i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i];
    }
    m.out_inl[r] = m.inl[hh]; m.out_cost[r] = m.cost[hh];
  }
}

}  // namespace

void launch_map_locate_score(hipStream_t s, const MapLocateDev& m) {
  const int n = m.na + m.nb;
  const unsigned blocks = (unsigned)((m.seed_cap + kThreads - 1) / kThreads);
  const size_t lds = ((size_t)n * (kLocateRec * sizeof(double) + sizeof(int32_t)) + 15) & ~(size_t)15;
  hipLaunchKernelGGL(k_ml_stage, dim3((n + 63) / 64), dim3(64), 0, s, m);
  hipLaunchKernelGGL(k_ml_count, dim3(m.na, m.na), dim3(kThreads), 0, s, m);
  hipLaunchKernelGGL(k_ml_scan, dim3(1), dim3(kThreads), 0, s, m);
  hipLaunchKernelGGL(k_ml_scatter, dim3(m.na, m.na), dim3(kThreads), 0, s, m);
  if (lds > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_ml_score), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);   // a refusal shows as the launch's error
  hipLaunchKernelGGL(k_ml_score, dim3(blocks * kLocateLanes), dim3(kThreads), lds, s, m);
  hipLaunchKernelGGL(k_ml_qcount, dim3(blocks), dim3(kThreads), 0, s, m);
  hipLaunchKernelGGL(k_ml_qscan, dim3(1), dim3(kThreads), 0, s, m);
}
void launch_map_locate_report(hipStream_t s, const MapLocateDev& m) {
  hipLaunchKernelGGL(k_ml_qscatter, dim3((unsigned)((m.seed_cap + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, m);
  hipLaunchKernelGGL(k_ml_rank, dim3((unsigned)((m.found + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, m);
  hipLaunchKernelGGL(k_ml_refine, dim3((unsigned)m.out), dim3(64), 0, s, m);
}

void launch_map_transform(hipStream_t s, const MapFrameDev& f) {
  const int B = T / f.od, nb = (f.n + B - 1) / B;
  if (f.od == 7) {
    hipLaunchKernelGGL(k_mf_jac<7>, dim3((f.n + 63) / 64), dim3(64), 0, s, f);
    hipLaunchKernelGGL(k_mf_cov<7>, dim3(nb, nb), dim3(kThreads), 0, s, f);
  } else {
    hipLaunchKernelGGL(k_mf_jac<9>, dim3((f.n + 63) / 64), dim3(64), 0, s, f);
    hipLaunchKernelGGL(k_mf_cov<9>, dim3(nb, nb), dim3(kThreads), 0, s, f);
  }
}
void launch_map_join(hipStream_t s, int64_t rows_a, const double* mean_a, const double* cov_a, int64_t rows_b, const double* mean_b, const double* cov_b, double* out_mean, double* out_cov) {
  const int64_t n = rows_a + rows_b;
  hipLaunchKernelGGL(k_mf_join, dim3((unsigned)((n + kThreads - 1) / kThreads), (unsigned)std::min<int64_t>(n, 65535)), dim3(kThreads), 0, s, rows_a, mean_a, cov_a, rows_b, mean_b, cov_b,
                     out_mean, out_cov);
}

void launch_map_match(hipStream_t s, const MapMatchDev& m) {
  const int B = T / m.od, nb = (m.n + B - 1) / B;
  hipLaunchKernelGGL(k_mt_diag, dim3(m.n), dim3(64), 0, s, m);
  if (m.od == 7) hipLaunchKernelGGL(k_mt_pairs<7>, dim3(nb, nb), dim3(kThreads), 0, s, m);
  else hipLaunchKernelGGL(k_mt_pairs<9>, dim3(nb, nb), dim3(kThreads), 0, s, m);
  hipLaunchKernelGGL(k_mt_count, dim3(m.n), dim3(kThreads), 0, s, m);
  hipLaunchKernelGGL(k_mt_scan, dim3(1), dim3(kThreads), 0, s, m);
  if (m.capacity > 0) hipLaunchKernelGGL(k_mt_scatter, dim3(m.n), dim3(kThreads), 0, s, m);
}

void launch_map_extend(hipStream_t s, const MapUpdateDev& u) {
  const int nA = u.nA, nN = u.nN, nB = u.nB, nP = (u.NA + u.NB + T - 1) / T;
  const MapDowndate d{u.Z, u.Y, nA, nullptr, u.od, u.N, u.N, u.ldo, u.map_cov, u.out_cov, u.status};
  if (nA > 0) {
    hipLaunchKernelGGL(k_mu_operands, dim3(nA, nA, 2), dim3(kThreads), 0, s, u.Wt, u.Wn, nA, u.P, (int64_t)u.ldp, u.NA, u.Ps);
    hipLaunchKernelGGL(k_mu_gather, dim3(nN, nA), dim3(kThreads), 0, s, u);
    hipLaunchKernelGGL(k_mu_gemm, dim3(nN, nA), dim3(kThreads), 0, s, MuGemm{u.G, u.Wn, u.Y, nA, nA, 1, 0});    // Y = G W^T
    hipLaunchKernelGGL(k_mu_gemm, dim3(nA, nA), dim3(kThreads), 0, s, MuGemm{u.Wn, u.Ps, u.U, nA, nA, 2, 0});   // U = W Ps_AA (Ps = Ps^T)
    hipLaunchKernelGGL(k_mu_gemm, dim3(nA, nA), dim3(kThreads), 0, s, MuGemm{u.U, u.Wn, u.M, nA, nA, 1, 1});    // M = I - U W^T
    hipLaunchKernelGGL(k_mu_gemm, dim3(nN, nA), dim3(kThreads), 0, s, MuGemm{u.Y, u.M, u.Z, nA, nA, 0, 0});     // Z = Y M (M = M^T)
    if (nB > 0) {
      hipLaunchKernelGGL(k_mx_stage, dim3(nB, nA), dim3(kThreads), 0, s, u);
      hipLaunchKernelGGL(k_mu_gemm, dim3(nB, nA), dim3(kThreads), 0, s, MuGemm{u.Pba, u.Wn, u.V, nA, nA, 1, 0});  // V = Ps_BA W^T
    }
    hipLaunchKernelGGL(k_map_wd, dim3(nA), dim3(kThreads), 0, s, u.W, u.pm, u.mean_A, u.NA, u.v);                // v = W (m_A - mu_A)
  }
  if (nN > 0) {   // with no window rows in the map both sums are empty: the old block symmetrised, the old means copied
    hipLaunchKernelGGL(k_map_downdate, dim3(nN, nN), dim3(kThreads), 0, s, d);
    hipLaunchKernelGGL(k_map_mean, dim3(nN), dim3(kThreads), 0, s, d, u.v, 1.0, u.map_mean, u.out_mean);
  }
  if (nA > 0 && nB > 0) hipLaunchKernelGGL(k_mx_cross, dim3(nN, nB), dim3(kThreads), 0, s, u);
  hipLaunchKernelGGL(k_mx_scatter, dim3(nP, nP), dim3(kThreads), 0, s, u);   // last: the A rows of the cross block give way to Ps_AB
}
void launch_map_select(hipStream_t s, const uint32_t* idx, int32_t k, int32_t od, const double* mean, const double* cov, int64_t ldc, double* out_mean, double* out_cov) {
  const unsigned nt = (unsigned)(((int64_t)k * od + T - 1) / T);
  hipLaunchKernelGGL(k_map_select, dim3(nt, nt), dim3(kThreads), 0, s, idx, k, od, mean, cov, ldc, out_mean, out_cov);
}
void launch_map_posterior_layout(hipStream_t s, const double* blocks, const double* objects, const uint32_t* obj_idx, int32_t k, int32_t od, double* P, double* pm) {
  const int64_t n = (int64_t)k * od * k * od;
  hipLaunchKernelGGL(k_mu_posterior_layout, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, blocks, objects, obj_idx, k, od, P, pm);
}

void launch_map_cut(hipStream_t s, const MapCutDev& m, int nt_max, const double* map_mean, const double* map_cov, int64_t ldc, const double* x0) {
  launch_map_factor(s, m, nt_max, map_mean, map_cov, ldc);
  launch_map_condition_estimate(s, m, nt_max, x0);
}

void launch_map_factor(hipStream_t s, const MapCutDev& m, int nt_max, const double* map_mean, const double* map_cov, int64_t ldc) {
  if (m.n <= 0) return;
  const unsigned gz = (unsigned)std::min<int64_t>(m.n, 65535);
  hipLaunchKernelGGL(k_map_gather, dim3(nt_max, nt_max, gz), dim3(kThreads), 0, s, m, map_mean, map_cov, ldc);
  launch_map_factorize(s, m, nt_max);
}

void launch_map_factorize(hipStream_t s, const MapCutDev& m, int nt_max) {
  if (m.n <= 0) return;
  const unsigned gz = (unsigned)std::min<int64_t>(m.n, 65535);
  for (int k = 0; k < nt_max; ++k) {
    hipLaunchKernelGGL(k_map_potrf, dim3(gz), dim3(kThreads), 0, s, m, k);
    if (k + 1 == nt_max) break;
    hipLaunchKernelGGL(k_map_trsm, dim3(nt_max - k - 1, gz), dim3(kThreads), 0, s, m, k);
    hipLaunchKernelGGL(k_map_syrk, dim3(nt_max - k - 1, nt_max - k - 1, gz), dim3(kThreads), 0, s, m, k);
  }
  hipLaunchKernelGGL(k_map_winv, dim3(nt_max, gz), dim3(kThreads), 0, s, m);
}

void launch_map_condition_estimate(hipStream_t s, const MapCutDev& m, int nt_max, const double* x0) {
  if (m.n <= 0) return;
  const unsigned gz = (unsigned)std::min<int64_t>(m.n, 65535);
  hipLaunchKernelGGL(k_map_lambda, dim3(nt_max, nt_max, gz), dim3(kThreads), 0, s, m);
  const int nb = (std::min(nt_max * T, kMapGroupMaxRows) + kPowRows - 1) / kPowRows;
  for (int step = 0; step < kMapPowerSteps; ++step) hipLaunchKernelGGL(k_map_power, dim3(nb, gz, 2), dim3(kThreads), 0, s, m, x0, step);
  hipLaunchKernelGGL(k_map_power_finish, dim3((unsigned)((m.n + 63) / 64)), dim3(64), 0, s, m);
}

void launch_map_merge(hipStream_t s, const MapMergeDev& g, const double* x0) {
  const int nQ = g.nQ, nK = g.nK;
  hipLaunchKernelGGL(k_mm_innovation, dim3(nQ, nQ), dim3(kThreads), 0, s, g);
  launch_map_factorize(s, g.cut, nQ);
  launch_map_condition_estimate(s, g.cut, nQ, x0);
  hipLaunchKernelGGL(k_mu_operands, dim3(nQ, nQ, 1), dim3(kThreads), 0, s, g.cut.Wt, g.Wn, nQ, nullptr, (int64_t)0, 0, nullptr);   // Wn = W as tiles
  hipLaunchKernelGGL(k_mm_gather, dim3(nK, nQ), dim3(kThreads), 0, s, g);
  hipLaunchKernelGGL(k_mu_gemm, dim3(nK, nQ), dim3(kThreads), 0, s, MuGemm{g.G, g.Wn, g.Y, nQ, nQ, 1, 0});       // Y = G W^T
  const MapDowndate d{g.Y, g.Y, nQ, g.kept, g.od, g.NK, g.N, g.NK, g.map_cov, g.out_cov, g.cut.status};
  hipLaunchKernelGGL(k_map_downdate, dim3(nK, nK), dim3(kThreads), 0, s, d);
  hipLaunchKernelGGL(k_map_wd, dim3(nQ), dim3(kThreads), 0, s, g.cut.W, g.cut.mean, nullptr, g.Q, g.v);          // v = W (H mu - d)
  hipLaunchKernelGGL(k_map_mean, dim3(nK), dim3(kThreads), 0, s, d, g.v, -1.0, g.map_mean, g.out_mean);
}

}  // namespace obvi
