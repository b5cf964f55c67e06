// cov_kernels.hip -- selected inversion (Takahashi recursion) of the reduced system on the tile pattern of its Cholesky factor, and the
// covariance blocks read from it (include/obvi_cov.h).
//
// The LM step leaves S = L L^T in the tiles (L_ik below the diagonal, L_kk with a zero upper part) and L_kk^-1 in Linv.  With I(k) the
// off-diagonal non-zero tile rows of tile column k and Y_jk = L_jk L_kk^-1, the entries of Sigma = S^-1 on the (fill-closed) pattern are
//     Sigma_ik = - sum_{j in I(k)} Sigma_ij Y_jk        (i in I(k);  Sigma_ij = Sigma_ji^T where only the lower tile is stored)
//     Sigma_kk = L_kk^-T L_kk^-1 - sum_{j in I(k)} Y_jk^T Sigma_jk
// Every i, j in I(k) is an ancestor of k in the tile elimination tree, so with the levels taken from the root down every Sigma_ij on the
// right is final.  Sigma overwrites L in place: column k of L is last read when column k is processed, and because the workgroups of a
// column would otherwise overwrite tiles their neighbours still read, the Y tiles of one level go through a scratch first.  Per level:
//     k_selinv_y     Y_jk = L_jk L_kk^-1                       -> scratch       (one workgroup per tile)
//     k_selinv_off   Sigma_ik                                  -> tile (i, k)   (one workgroup per target tile, products in list order)
//     k_selinv_diag  Sigma_kk, symmetrised, both triangles     -> tile (k, k)   (one workgroup per column)
// One writer per tile, no atomics, no flags between workgroups: the launch boundary is the only dependency, and the same code runs on a
// default and on a deterministic handle.  All 64x64 products are on v_mfma_f64_16x16x4_f64.
// Further down: the two routes of obvi_cov_compute_pairs (include/obvi_cov_pairs.h) -- forward substitution and block products for reduced pairs off the
// pattern, run before the recursion while L is intact, and the blocks with a feature, run after it.
#include "ba_device.h"
#include "chol_tile.h"

namespace obvi {
namespace {

// C += op(A) * B with op(A) = A or A^T; both row-major 64x64 tiles in LDS (LDM).  tile_abt_mfma (chol_tile.h) multiplies by B^T; every
// product of the recursion has a plain right operand and some a transposed left one, so the operands are read in the layout the
// fragments need instead of being transposed while staging.  Fragments: A: lane l -> A[l&15][l>>4]; B: lane l -> B[l>>4][l&15].
template <bool TA>
__device__ __forceinline__ void tile_ab_mfma(const double* A, const double* B, f64x4 acc[4]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const double* Bp = B + kq * LDM + 16 * wv + r16;
  const double* Ap = TA ? A + kq * LDM + r16 : A + r16 * LDM + kq;
#pragma unroll
  for (int k0 = 0; k0 < T; k0 += 4) {
    const double bv = Bp[k0 * LDM];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      const double av = TA ? Ap[k0 * LDM + 16 * rt] : Ap[16 * rt * LDM + k0];
      acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[rt], 0, 0, 0);
    }
  }
}
__device__ __forceinline__ void store_acc(double* tile, const f64x4 acc[4], double sign) {   // accumulator layout -> row-major tile (global, ld T)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) tile[(16 * rt + (lane >> 4) + 4 * r) * T + 16 * wv + (lane & 15)] = sign * acc[rt][r];
}
// position of tile row i in the list of column k (i is in it: the jobs are the list's entries)
__device__ __forceinline__ int col_find(const int32_t* __restrict__ col_ptr, const int32_t* __restrict__ col_i, int k, int i) {
  const int e0 = col_ptr[k], e1 = col_ptr[k + 1];
  int e = e0;
  while (e + 1 < e1 && col_i[e] != i) ++e;
  return e - e0;
}

struct SelInv {
  double* S; int nt;
  const double* Linv;
  double* Ys;                 // Y tiles of the running level
  const int32_t* ybase;       // [nt] first scratch tile of column k inside its level
  const int32_t* col_ptr; const int32_t* col_i;
};

__global__ void __launch_bounds__(kThreads) k_selinv_y(SelInv p, const int32_t* __restrict__ jobs) {
  __shared__ double smem[2 * T * LDM];
  double* A = smem;
  double* B = smem + T * LDM;
  const int i = jobs[2 * blockIdx.x], k = jobs[2 * blockIdx.x + 1];
  const int x = col_find(p.col_ptr, p.col_i, k, i);
  stage_tiles(A, tile_ptr(p.S, p.nt, i, k), B, p.Linv + (int64_t)k * (T * T));
  __syncthreads();
  f64x4 acc[4] = {};
  tile_ab_mfma<false>(A, B, acc);
  store_acc(p.Ys + (int64_t)(p.ybase[k] + x) * (T * T), acc, 1.0);
}

__global__ void __launch_bounds__(kThreads) k_selinv_off(SelInv p, const int32_t* __restrict__ jobs) {
  __shared__ double smem[2 * T * LDM];
  double* A = smem;
  double* B = smem + T * LDM;
  const int i = jobs[2 * blockIdx.x], k = jobs[2 * blockIdx.x + 1];
  const int e0 = p.col_ptr[k], e1 = p.col_ptr[k + 1];
  const double* Yk = p.Ys + (int64_t)p.ybase[k] * (T * T);
  f64x4 acc[4] = {};
  for (int e = e0; e < e1; ++e) {
    const int j = p.col_i[e];
    __syncthreads();
    stage_tiles(A, i >= j ? tile_ptr(p.S, p.nt, i, j) : tile_ptr(p.S, p.nt, j, i), B, Yk + (int64_t)(e - e0) * (T * T));
    __syncthreads();
    if (i >= j) tile_ab_mfma<false>(A, B, acc);   // (the diagonal tile Sigma_ii holds both triangles)
    else tile_ab_mfma<true>(A, B, acc);
  }
  store_acc(tile_ptr(p.S, p.nt, i, k), acc, -1.0);
}

__global__ void __launch_bounds__(kThreads) k_selinv_diag(SelInv p, const int32_t* __restrict__ klist) {
  __shared__ double smem[2 * T * LDM];
  double* A = smem;
  double* B = smem + T * LDM;
  const int k = klist[blockIdx.x];
  const int e0 = p.col_ptr[k], e1 = p.col_ptr[k + 1];
  const double* Yk = p.Ys + (int64_t)p.ybase[k] * (T * T);
  stage_tile(A, p.Linv + (int64_t)k * (T * T));
  __syncthreads();
  f64x4 acc[4] = {}, sub[4] = {};
  tile_ab_mfma<true>(A, A, acc);   // L_kk^-T L_kk^-1
  for (int e = e0; e < e1; ++e) {
    __syncthreads();
    stage_tiles(A, Yk + (int64_t)(e - e0) * (T * T), B, tile_ptr(p.S, p.nt, p.col_i[e], k));
    __syncthreads();
    tile_ab_mfma<true>(A, B, sub);   // Y_jk^T Sigma_jk
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) A[(16 * rt + (lane >> 4) + 4 * r) * LDM + 16 * wv + (lane & 15)] = acc[rt][r] - sub[rt][r];
  __syncthreads();
  double* out = tile_ptr(p.S, p.nt, k, k);
  for (int e = threadIdx.x; e < T * T; e += kThreads) {
    const int r = e / T, c = e % T;
    out[e] = 0.5 * (A[r * LDM + c] + A[c * LDM + r]);
  }
}

// entry (r, c) of Sigma, rows of the tile grid: the lower tile, or the transposed entry of it
__device__ __forceinline__ double sigma_at(const double* __restrict__ S, int nt, int r, int c) {
  int tr = r / T, tc = c / T;
  if (tr < tc) { const int t = r; r = c; c = t; const int u = tr; tr = tc; tc = u; }
  return S[((int64_t)tr * nt + tc) * (T * T) + (r % T) * T + (c % T)];
}

// blocks of Sigma: item b = (first row, first column, rows, columns), row < 0: a zero block; out + off[b], row-major
__global__ void __launch_bounds__(128) k_cov_gather(const double* __restrict__ S, int nt, const int32_t* __restrict__ desc, const int64_t* __restrict__ off, double* __restrict__ out) {
  const int32_t* d = desc + 4 * (int64_t)blockIdx.x;
  const int ra = d[0], rb = d[1], da = d[2], db = d[3];
  const int t = threadIdx.x;
  if (t >= da * db) return;
  const int i = t / db, j = t % db;
  out[off[blockIdx.x] + t] = (ra < 0 || rb < 0) ? 0.0 : sigma_at(S, nt, ra + i, rb + j);
}

// Feature blocks: Cov_ll = C^-T (I + sum_{a, b in obs(l)} Z_a^T Sigma_{p(a) p(b)} Z_b) C^-1, Z_a = W_a C^-T the records of the point pass, Ci = C^-1.
// One wavefront per requested feature; lane x takes the observation pairs x, x + 64, ... (a stereo pair's two records of one frame are two
// observations; a record without a variable pose -- yrow < 0 -- is skipped), then a butterfly sum in a fixed order.
__global__ void __launch_bounds__(256) k_cov_points(const double* __restrict__ S, int nt, int64_t n, const int64_t* __restrict__ idx, const uint32_t* __restrict__ point_ptr,
                                                   const int32_t* __restrict__ yrow, const uint8_t* __restrict__ point_var, const double* __restrict__ Z,
                                                   const double* __restrict__ Ci, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n) return;
  const int64_t l = idx[g];
  if (l < 0 || !point_var[l]) { if (lane < 9) out[9 * g + lane] = 0.0; return; }
  const uint32_t beg = point_ptr[l], cnt = point_ptr[l + 1] - beg;
  double m[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) m[q] = 0.0;
  const uint32_t npair = cnt * cnt;
  for (uint32_t pr = lane; pr < npair; pr += 64) {
    const uint32_t a = beg + pr / cnt, b = beg + pr % cnt;
    const int ra = yrow[a], rb = yrow[b];
    if (ra < 0 || rb < 0) continue;
    const double* Za = Z + 18 * (int64_t)a + 4 * l;
    const double* Zb = Z + 18 * (int64_t)b + 4 * l;
    double zb[18];
#pragma unroll
    for (int q = 0; q < 18; ++q) zb[q] = Zb[q];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double sg = sigma_at(S, nt, ra + i, rb + j);
        s0 = fma(sg, zb[3 * j], s0); s1 = fma(sg, zb[3 * j + 1], s1); s2 = fma(sg, zb[3 * j + 2], s2);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double za = Za[3 * i + c];
        m[3 * c] = fma(za, s0, m[3 * c]); m[3 * c + 1] = fma(za, s1, m[3 * c + 1]); m[3 * c + 2] = fma(za, s2, m[3 * c + 2]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 9; ++q)
    for (int o = 32; o > 0; o >>= 1) m[q] += __shfl_xor(m[q], o, 64);
  if (lane == 0) {
    m[0] += 1.0; m[4] += 1.0; m[8] += 1.0;
    const double* ci = Ci + 6 * l;
    const double Cm[9] = {ci[0], 0.0, 0.0, ci[1], ci[2], 0.0, ci[3], ci[4], ci[5]};
    double t[9], c[9];
    for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) { double s = 0.0; for (int x = 0; x < 3; ++x) s += m[3 * r + x] * Cm[3 * x + q]; t[3 * r + q] = s; }
    for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) { double s = 0.0; for (int x = 0; x < 3; ++x) s += Cm[3 * x + r] * t[3 * x + q]; c[3 * r + q] = s; }
    for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) out[9 * g + 3 * r + q] = 0.5 * (c[3 * r + q] + c[3 * q + r]);
  }
}

// ---------------------------------------------------------------------------------------
// Declared pairs (obvi_cov_compute_pairs).  A reduced pair off the tile pattern is E_a^T S^-1 E_b = (L^-1 E_a)^T (L^-1 E_b), formed while the factor is
// still in the tiles: the unit vectors of the distinct blocks of such pairs, sorted by row (elimination order), are packed 64 to a slab and Y = L^-1 E is
// kept transposed, Yt [64 nslabs][ldt = 64 nt] row-major, so that the substitution of tile row k is the factorisation's update
//     Yt_k = (E_k - sum_j Yt_j L_kj^T) L_kk^-T           (64x64x64 products, tile_abt_mfma)
// One workgroup per (tile row of the level, slab), the row's products in list order: no atomics, no row splitting, one code path for default and
// deterministic handles.  A slab is zero left of the tile of its first right-hand side and skips those rows.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void block_fetch(TileRegs& r, const double* src, int64_t ld) {   // 64x64 block of a row-major matrix, the thread -> element map of tile_fetch
#pragma unroll
  for (int x = 0; x < T * T / 2 / kThreads; ++x) {
    const int e = threadIdx.x + kThreads * x, row = e / (T / 2), c2 = e % (T / 2);
    r.v[x] = *reinterpret_cast<const double2*>(src + (int64_t)row * ld + 2 * c2);
  }
}
__global__ void __launch_bounds__(64) k_cov_seed_rows(double* Yt, int64_t ldt, const int32_t* __restrict__ rhs_row, int32_t nrhs) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t < nrhs) Yt[(int64_t)t * ldt + rhs_row[t]] = 1.0;
}
__global__ void __launch_bounds__(kThreads) k_cov_forward(const double* __restrict__ S, int nt, const int32_t* __restrict__ lvl_k, const int32_t* __restrict__ row_ptr,
                                                         const int32_t* __restrict__ row_j, const double* __restrict__ Linv, double* Yt, int64_t ldt,
                                                         const int32_t* __restrict__ slab_first) {
  __shared__ double smem[2 * T * LDM];
  double* A = smem;
  double* B = smem + T * LDM;
  const int k = lvl_k[blockIdx.x], sl = blockIdx.y;
  const int first = slab_first[sl];
  if (k < first) return;                          // uniform per workgroup
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* Yslab = Yt + (int64_t)sl * T * ldt;
  f64x4 acc[4] = {};
  for (int e = row_ptr[k]; e < row_ptr[k + 1]; ++e) {
    const int j = row_j[e];
    if (j < first) continue;                      // Yt_j is zero in this slab
    TileRegs ra, rb;
    block_fetch(ra, Yslab + (int64_t)j * T, ldt);
    tile_fetch(rb, S + ((int64_t)k * nt + j) * (T * T));
    __syncthreads();
    tile_put(A, ra);
    tile_put(B, rb);
    __syncthreads();
    tile_abt_mfma(A, B, acc);
  }
  double* Yk = Yslab + (int64_t)k * T;
  __syncthreads();
  TileRegs rl;
  tile_fetch(rl, Linv + (int64_t)k * (T * T));    // L_kk^-1 carries an explicit zero upper part
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * rt + (lane >> 4) + 4 * r, col = 16 * wv + (lane & 15);
      A[row * LDM + col] = Yk[(int64_t)row * ldt + col] - acc[rt][r];   // E_k - sum, from the accumulator layout into the A operand
    }
  tile_put(B, rl);
  __syncthreads();
  f64x4 out[4] = {};
  tile_abt_mfma(A, B, out);
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) Yk[(int64_t)(16 * rt + (lane >> 4) + 4 * r) * ldt + 16 * wv + (lane & 15)] = out[rt][r];
}

// block p = Yt[ca .. ca + DA) Yt[cb .. cb + DB)^T over the columns from first[p] on (both are zero before); one workgroup per pair, a fixed-order reduction
template <int DA, int DB>
__global__ void __launch_bounds__(kThreads) k_cov_rhs_pairs(const double* __restrict__ Yt, int64_t ldt, const int32_t* __restrict__ cols, const int32_t* __restrict__ first,
                                                           const int64_t* __restrict__ off, double* __restrict__ out) {
  __shared__ double red[kThreads / 64][DA * DB];
  const int p = blockIdx.x;
  const double* ya = Yt + (int64_t)cols[2 * p] * ldt;
  const double* yb = Yt + (int64_t)cols[2 * p + 1] * ldt;
  double acc[DA * DB];
#pragma unroll
  for (int i = 0; i < DA * DB; ++i) acc[i] = 0.0;
  for (int64_t x = first[p] + threadIdx.x; x < ldt; x += kThreads) {
    double b[DB];
#pragma unroll
    for (int k = 0; k < DB; ++k) b[k] = yb[k * ldt + x];
#pragma unroll
    for (int r = 0; r < DA; ++r) {
      const double a = ya[r * ldt + x];
#pragma unroll
      for (int k = 0; k < DB; ++k) acc[DB * r + k] = fma(a, b[k], acc[DB * r + k]);
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < DA * DB; ++i) {
    double v = acc[i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) red[wv][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < DA * DB) {
    double v = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) v += red[w][threadIdx.x];
    out[off[p] + threadIdx.x] = v;
  }
}

// Pairs with a feature, from the records of the point pass (H_ll = C C^T, Ci = C^-1, Z_a = W_a C^-T):
//     Sigma_{l,x} = - C_l^-T sum_{a in obs(l)} Z_a^T Sigma_{p(a),x}                                   x a pose or an object
//     Sigma_{l,m} =   C_l^-T ( sum_{a in obs(l), b in obs(m)} Z_a^T Sigma_{p(a)p(b)} Z_b ) C_m^-1     l != m
// One wavefront per requested pair; lane e takes the observations (observation pairs) e, e + 64, ..., then a butterfly sum in a fixed order.  An
// operand block of Sigma is read entry-wise from the tiles (it may straddle tiles) or, off the pattern, from the side buffer (op >= 0: offset << 1 |
// stored transposed).  A record without a variable pose (yrow < 0: masked, or a constant pose) is skipped.
__device__ __forceinline__ double sigma_op(const double* S, int nt, const double* side, int64_t op, int ra, int da, int rb, int db, int i, int j) {
  if (op < 0) return sigma_at(S, nt, ra + i, rb + j);
  const double* b = side + (op >> 1);
  return (op & 1) ? b[j * da + i] : b[i * db + j];
}
__global__ void __launch_bounds__(256) k_cov_point_cross(const double* __restrict__ S, int nt, int64_t n, const int32_t* __restrict__ req, const int64_t* __restrict__ op_ptr,
                                                        const int64_t* __restrict__ ops, const int64_t* __restrict__ out_off, const uint32_t* __restrict__ point_ptr,
                                                        const int32_t* __restrict__ yrow, const double* __restrict__ Z, const double* __restrict__ Ci, double* side) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n) return;
  const int64_t l = req[4 * g], x = req[4 * g + 1];
  const int dx = req[4 * g + 2];
  const uint32_t beg = point_ptr[l], cnt = point_ptr[l + 1] - beg;
  const int64_t* op = ops + op_ptr[g];
  double m[27];
#pragma unroll
  for (int q = 0; q < 27; ++q) m[q] = 0.0;
  if (dx > 0) {
    for (uint32_t e = lane; e < cnt; e += 64) {
      const uint32_t a = beg + e;
      const int ra = yrow[a];
      if (ra < 0) continue;
      const double* Za = Z + 18 * (int64_t)a + 4 * l;
      const int64_t o = op[e];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double z0 = Za[3 * i], z1 = Za[3 * i + 1], z2 = Za[3 * i + 2];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          if (j < dx) {
            const double sg = sigma_op(S, nt, side, o, ra, 6, (int)x, dx, i, j);
            m[j] = fma(z0, sg, m[j]); m[9 + j] = fma(z1, sg, m[9 + j]); m[18 + j] = fma(z2, sg, m[18 + j]);
          }
        }
      }
    }
  } else {
    const uint32_t begm = point_ptr[x], cntm = point_ptr[x + 1] - begm;
    const uint32_t npair = cnt * cntm;
    for (uint32_t e = lane; e < npair; e += 64) {
      const uint32_t a = beg + e / cntm, b = begm + e % cntm;
      const int ra = yrow[a], rb = yrow[b];
      if (ra < 0 || rb < 0) continue;
      const double* Za = Z + 18 * (int64_t)a + 4 * l;
      const double* Zb = Z + 18 * (int64_t)b + 4 * x;
      const int64_t o = op[e];
      double zb[18];
#pragma unroll
      for (int q = 0; q < 18; ++q) zb[q] = Zb[q];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const double sg = sigma_op(S, nt, side, o, ra, 6, rb, 6, i, j);
          s0 = fma(sg, zb[3 * j], s0); s1 = fma(sg, zb[3 * j + 1], s1); s2 = fma(sg, zb[3 * j + 2], s2);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double za = Za[3 * i + c];
          m[3 * c] = fma(za, s0, m[3 * c]); m[3 * c + 1] = fma(za, s1, m[3 * c + 1]); m[3 * c + 2] = fma(za, s2, m[3 * c + 2]);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 27; ++q)
    for (int o = 32; o > 0; o >>= 1) m[q] += __shfl_xor(m[q], o, 64);
  if (lane != 0) return;
  const double* ci = Ci + 6 * l;
  const double Cl[9] = {ci[0], 0.0, 0.0, ci[1], ci[2], 0.0, ci[3], ci[4], ci[5]};
  double* out = side + out_off[g];
  if (dx > 0) {
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 9; ++q)
        if (q < dx) out[r * dx + q] = -(Cl[r] * m[q] + Cl[3 + r] * m[9 + q] + Cl[6 + r] * m[18 + q]);
  } else {
    const double* cm = Ci + 6 * x;
    const double Cm[9] = {cm[0], 0.0, 0.0, cm[1], cm[2], 0.0, cm[3], cm[4], cm[5]};
    double t[9];
    for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) { double s = 0.0; for (int y = 0; y < 3; ++y) s += m[3 * r + y] * Cm[3 * y + q]; t[3 * r + q] = s; }
    for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) { double s = 0.0; for (int y = 0; y < 3; ++y) s += Cl[3 * y + r] * t[3 * y + q]; out[3 * r + q] = s; }
  }
}

}  // namespace

void launch_selected_inverse(hipStream_t s, const CholPlan& p, double* S, const double* Linv, double* Ys, const int32_t* ybase) {
  const SelInv v{S, p.nt, Linv, Ys, ybase, p.col_ptr, p.col_i};
  for (int l = p.nlevels - 1; l >= 0; --l) {
    const int nk = p.lvl_k_ptr[l + 1] - p.lvl_k_ptr[l], nj = p.trsm_ptr[l + 1] - p.trsm_ptr[l];
    const int32_t* jobs = p.trsm_ik + 2 * (int64_t)p.trsm_ptr[l];   // the level's off-diagonal tiles (i, k)
    if (nj > 0) {
      hipLaunchKernelGGL(k_selinv_y, dim3(nj), dim3(kThreads), 0, s, v, jobs);
      hipLaunchKernelGGL(k_selinv_off, dim3(nj), dim3(kThreads), 0, s, v, jobs);
    }
    if (nk > 0) hipLaunchKernelGGL(k_selinv_diag, dim3(nk), dim3(kThreads), 0, s, v, p.lvl_k + p.lvl_k_ptr[l]);
  }
}
void launch_cov_gather(hipStream_t s, const double* S, int32_t nt, int64_t n, const int32_t* desc, const int64_t* off, double* out) {
  if (n > 0) hipLaunchKernelGGL(k_cov_gather, dim3((unsigned)n), dim3(128), 0, s, S, nt, desc, off, out);
}
void launch_cov_points(hipStream_t s, const double* S, int32_t nt, int64_t n, const int64_t* idx, const uint32_t* point_ptr, const int32_t* yrow, const uint8_t* point_var,
                       const double* Z, const double* Ci, double* out) {
  if (n > 0) hipLaunchKernelGGL(k_cov_points, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, S, nt, n, idx, point_ptr, yrow, point_var, Z, Ci, out);
}

void launch_cov_forward(hipStream_t s, const CholPlan& p, const double* S, const double* Linv, double* Yt, int64_t ldt, int nslabs, const int32_t* slab_first,
                        const int32_t* rhs_row, int32_t nrhs) {
  if (nrhs <= 0 || nslabs <= 0) return;
  (void)hipMemsetAsync(Yt, 0, sizeof(double) * (size_t)nslabs * T * (size_t)ldt, s);
  hipLaunchKernelGGL(k_cov_seed_rows, dim3((nrhs + 63) / 64), dim3(64), 0, s, Yt, ldt, rhs_row, nrhs);
  for (int l = 0; l < p.nlevels; ++l) {
    const int nk = p.lvl_k_ptr[l + 1] - p.lvl_k_ptr[l];
    if (nk > 0) hipLaunchKernelGGL(k_cov_forward, dim3(nk, nslabs), dim3(kThreads), 0, s, S, p.nt, p.lvl_k + p.lvl_k_ptr[l], p.row_ptr, p.row_j, Linv, Yt, ldt, slab_first);
  }
}
void launch_cov_rhs_pairs(hipStream_t s, const double* Yt, int64_t ldt, int64_t n, int da, int db, const int32_t* cols, const int32_t* first, const int64_t* off, double* out) {
  if (n <= 0) return;
  const dim3 grid((unsigned)n), block(kThreads);
  if (da == 6 && db == 6) hipLaunchKernelGGL((k_cov_rhs_pairs<6, 6>), grid, block, 0, s, Yt, ldt, cols, first, off, out);
  else if (da == 6 && db == 7) hipLaunchKernelGGL((k_cov_rhs_pairs<6, 7>), grid, block, 0, s, Yt, ldt, cols, first, off, out);
  else if (da == 6 && db == 9) hipLaunchKernelGGL((k_cov_rhs_pairs<6, 9>), grid, block, 0, s, Yt, ldt, cols, first, off, out);
  else if (da == 7 && db == 7) hipLaunchKernelGGL((k_cov_rhs_pairs<7, 7>), grid, block, 0, s, Yt, ldt, cols, first, off, out);
  else hipLaunchKernelGGL((k_cov_rhs_pairs<9, 9>), grid, block, 0, s, Yt, ldt, cols, first, off, out);
}
void launch_cov_point_cross(hipStream_t s, const double* S, int32_t nt, int64_t n, const int32_t* req, const int64_t* op_ptr, const int64_t* ops, const int64_t* out_off,
                            const uint32_t* point_ptr, const int32_t* yrow, const double* Z, const double* Ci, double* side) {
  if (n > 0) hipLaunchKernelGGL(k_cov_point_cross, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, S, nt, n, req, op_ptr, ops, out_off, point_ptr, yrow, Z, Ci, side);
}

}  // namespace obvi
