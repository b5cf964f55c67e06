// chol_tile.h -- the 64x64 fp64 tile primitives of the tile Cholesky (chol_kernels.hip) and of the selected inversion (cov_kernels.hip): tile addressing,
// global -> LDS staging with the LDM = 66 leading dimension, and the tile product on v_mfma_f64_16x16x4_f64.  Device code only; internal linkage.
#ifndef OBVI_CHOL_TILE_H_
#define OBVI_CHOL_TILE_H_
#include "ba_device.h"

namespace obvi {
namespace {

constexpr int T = kTile;        // 64
constexpr int kThreads = 256;
__device__ __forceinline__ double* tile_ptr(double* S, int nt, int i, int j) { return S + ((int64_t)i * nt + j) * (T * T); }

// ---------------------------------------------------------------------------------------
// 64x64x64 fp64 tile product  C += A * B^T  on the matrix cores: v_mfma_f64_16x16x4_f64.
// Both operands are row-major tiles staged in LDS with leading dimension LDM = 66 doubles
// (bank = (4 row + 2 col) mod 64 for the 16-row x 2-col footprint of a 32-lane group: conflict-free).
// Wavefront w owns output columns [16w, 16w+16); acc[rt] is the 16x16 tile of rows [16rt, 16rt+16).
// Fragment layout (cdna_hip_programming.md 3): A: lane l -> A[l&15][l>>4]; B: lane l -> B[l>>4][l&15];
// D: lane l, reg r -> D[(l>>4) + 4r][l&15].
// ---------------------------------------------------------------------------------------
constexpr int LDM = T + 2;
typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void tile_abt_mfma(const double* A, const double* B, f64x4 acc[4]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const double* Bp = B + (16 * wv + r16) * LDM + kq;
  const double* Ap = A + r16 * LDM + kq;
#pragma unroll
  for (int k0 = 0; k0 < T; k0 += 4) {
    const double bv = Bp[k0];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      const double av = Ap[16 * rt * LDM + k0];
      acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[rt], 0, 0, 0);
    }
  }
}
// A tile (or 16 rows of one) travels global -> registers -> LDS in two separate phases: every 16-byte load of a thread first, then the LDS
// writes.  (Written as one loop of load + store, the compiler clustered five of a tile's eight loads and waited for each of the other
// three on its own: four memory latencies per tile, eight for the two operands of a product.)
struct TileRegs { double2 v[T * T / 2 / kThreads]; };    // 8 x 16 bytes per thread of a 256-thread group
__device__ __forceinline__ void tile_fetch(TileRegs& r, const double* __restrict__ src) {
#pragma unroll
  for (int x = 0; x < T * T / 2 / kThreads; ++x) r.v[x] = reinterpret_cast<const double2*>(src)[threadIdx.x + kThreads * x];
}
__device__ __forceinline__ void tile_put(double* dst, const TileRegs& r) {   // row-major tile -> LDS with leading dimension LDM
#pragma unroll
  for (int x = 0; x < T * T / 2 / kThreads; ++x) {
    const int e = threadIdx.x + kThreads * x, row = e / (T / 2), c2 = e % (T / 2);
    dst[row * LDM + 2 * c2] = r.v[x].x; dst[row * LDM + 2 * c2 + 1] = r.v[x].y;
  }
}
__device__ __forceinline__ void stage_tile(double* dst, const double* __restrict__ src) {
  TileRegs r;
  tile_fetch(r, src);
  tile_put(dst, r);
}
// two tiles: all sixteen loads in flight together
__device__ __forceinline__ void stage_tiles(double* dstA, const double* __restrict__ srcA, double* dstB, const double* __restrict__ srcB) {
  TileRegs ra, rb;
  tile_fetch(ra, srcA);
  tile_fetch(rb, srcB);
  tile_put(dstA, ra);
  tile_put(dstB, rb);
}

}  // namespace
}  // namespace obvi
#endif  // OBVI_CHOL_TILE_H_
