// dense_cholesky_kernels.hpp -- the kernels of cse_dense_cholesky_* (DESIGN
// section 3.6h): a blocked right-looking Cholesky factorization of a row-major
// symmetric matrix, kDcNB = 64 columns per panel, in double or float, and the
// blocked substitutions and refinement kernels of its solve.
//
//   DcDiagKernel      one workgroup: the panel's NB x NB diagonal block
//       factored in LDS (the pivot test sees NaN and Inf: this TU is built
//       without -ffinite-math-only), L_kk written back and L_kk^-1 stored, so
//       that the panel below and the solve's diagonal steps are products.
//   DcPanelKernel     one workgroup per block row below: L_ik = A_ik L_kk^-T.
//   DcTrailingKernel  one workgroup per lower-triangle tile of the rest:
//       A_ij -= L_ik L_jk^T on the matrix cores (v_mfma_f64_16x16x4_f64,
//       v_mfma_f32_16x16x4_f32), four waves of 32 x 32 each.
//   DcForwardKernel, DcBackwardKernel  step k of L y = v and L^T x = y: every
//       workgroup forms the step's diagonal product itself and then updates
//       its own block row, so a step is one launch.
//   DcResidualKernel  r = rhs - A x from the lower triangle alone, one
//       workgroup per block row, tiles above the diagonal read transposed.
// Ordering between workgroups comes from kernel boundaries only; no atomics,
// every sum in a fixed order: bit-identical from run to run.  Once the flag is
// set, every later kernel of the factorization returns at once.  Ragged n and
// ld > n are bounds in the loads and stores; offsets are 64-bit.
#ifndef CSE_DENSE_CHOLESKY_KERNELS_HPP_
#define CSE_DENSE_CHOLESKY_KERNELS_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

#include "plan.hpp"

namespace cse {

constexpr int kDcNB = kDenseCholeskyNB;
constexpr int kDcThreads = 256;
constexpr int kDcTile = kDcNB * kDcNB;
constexpr int kDcPad = kDcNB + 1;    // LDS row stride of a whole tile
constexpr int kDcKChunk = 32;        // the products stage K in two halves
constexpr int kDcKStride = 36;       // their LDS row stride: conflict-free in float, 2-way in double
static_assert(kDcNB == 64 && kDcThreads == 4 * kDcNB, "the thread maps below spell these out");

typedef double DcDouble4 __attribute__((ext_vector_type(4)));
typedef float DcFloat4 __attribute__((ext_vector_type(4)));

// The 16 x 16 x 4 matrix-core product of each type.  A: lane l holds
// A[m = l % 16][k = l / 16], B: B[k = l / 16][n = l % 16]; C[Row(l, r)][l % 16].
template <typename T>
struct DcMfma;
template <>
struct DcMfma<double> {
  typedef DcDouble4 Acc;
  static __device__ __forceinline__ Acc Mma(double a, double b, Acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int Row(int lane, int r) { return (lane >> 4) + 4 * r; }
};
template <>
struct DcMfma<float> {
  typedef DcFloat4 Acc;
  static __device__ __forceinline__ Acc Mma(float a, float b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int Row(int lane, int r) { return 4 * (lane >> 4) + r; }
};

// Positive and finite; NaN fails both comparisons.
template <typename T>
__device__ __forceinline__ bool DcPivotOk(T d) {
  return d > T(0) && d <= std::numeric_limits<T>::max();
}

// The lower triangle of A in float, lower-triangle tiles folded as the
// trailing update's (R = the number of block rows).
__global__ __launch_bounds__(kDcThreads) void DcCastLowerKernel(const double* __restrict__ A, int64_t ld,
                                                                  int64_t n, float* __restrict__ out) {
  const DenseCholeskyTile tile = DenseCholeskyTrailingTile((int64_t)gridDim.x - 1, blockIdx.x, blockIdx.y);
  if (!tile.live) return;
  const int64_t r0 = tile.i * kDcNB, c0 = tile.j * kDcNB;
  for (int idx = threadIdx.x; idx < kDcTile; idx += kDcThreads) {
    const int64_t r = r0 + idx / kDcNB, c = c0 + idx % kDcNB;
    if (r < n && c <= r) out[r * n + c] = (float)A[r * ld + c];
  }
}

// Panel k's diagonal block: factor, write L_kk, store L_kk^-1 (rows and
// columns past n: the identity).  flag[0] receives the 1-based order of the
// first pivot that is not positive and finite, and nothing is written then.
template <typename T>
__global__ __launch_bounds__(kDcThreads) void DcDiagKernel(T* __restrict__ M, int64_t ld, int64_t n, int64_t k,
                                                           T* __restrict__ inv, int* __restrict__ flag) {
  if (*flag) return;
  __shared__ T a[kDcNB * kDcPad];
  __shared__ T x[kDcNB * (kDcNB + 1) / 2];  // L_kk^-1, lower triangle packed by rows
  const int t = threadIdx.x;
  const int64_t k0 = k * kDcNB;
  const int nb = (int)(n - k0 < kDcNB ? n - k0 : kDcNB);
  for (int idx = t; idx < kDcTile; idx += kDcThreads) {
    const int r = idx / kDcNB, c = idx % kDcNB;
    T v = r == c ? T(1) : T(0);
    if (c <= r) x[r * (r + 1) / 2 + c] = v;  // the identity: x becomes L^-1 as the columns go
    if (r < nb && c <= r) v = M[(k0 + r) * ld + k0 + c];
    a[r * kDcPad + c] = v;
  }
  __syncthreads();
  // Right-looking, and L X = I carried along: after column j is scaled, row j
  // of X is its right-hand side row over the pivot, and the rows below lose
  // their multiple of it, as the trailing columns of a lose theirs.
  const int c = t % kDcNB;
  for (int j = 0; j < kDcNB; ++j) {
    const T d = a[j * kDcPad + j];
    if (!DcPivotOk(d)) {  // the same value in every thread
      if (t == 0) *flag = (int)(k0 + j + 1);
      return;
    }
    const T s = sqrt(d);
    __syncthreads();
    if (t < kDcNB) {
      if (t == j)
        a[j * kDcPad + j] = s;
      else if (t > j)
        a[t * kDcPad + j] = a[t * kDcPad + j] / s;
    } else if (t < 2 * kDcNB) {
      if (c <= j) x[j * (j + 1) / 2 + c] = x[j * (j + 1) / 2 + c] / s;
    }
    __syncthreads();
    for (int r = j + 1 + t / kDcNB; r < kDcNB; r += kDcThreads / kDcNB) {
      const T l = a[r * kDcPad + j];
      if (c > j) {
        if (c <= r) a[r * kDcPad + c] -= l * a[c * kDcPad + j];
      } else {
        x[r * (r + 1) / 2 + c] -= l * x[j * (j + 1) / 2 + c];
      }
    }
    __syncthreads();
  }
  for (int idx = t; idx < kDcTile; idx += kDcThreads) {
    const int r = idx / kDcNB, cc = idx % kDcNB;
    if (r < nb && cc <= r) M[(k0 + r) * ld + k0 + cc] = a[r * kDcPad + cc];
  }
  T* out = inv + k * kDcTile;
  for (int idx = t; idx < kDcTile; idx += kDcThreads) {
    const int r = idx / kDcNB, cc = idx % kDcNB;
    out[idx] = cc <= r ? x[r * (r + 1) / 2 + cc] : T(0);
  }
}

// acc += P Q^T over K = NB: P and Q are tiles of NB columns, prow and qrow of
// their NB rows valid (the others count as zero).  Wave w takes the 32 x 32
// quadrant (w / 2, w % 2) as 2 x 2 matrix-core tiles.  ps, qs: [NB][kDcKStride].
template <typename T>
__device__ __forceinline__ void DcTileABt(const T* __restrict__ P, int64_t ldp, int prow, const T* __restrict__ Q,
                                          int64_t ldq, int qrow, T* ps, T* qs,
                                          typename DcMfma<T>::Acc (&acc)[2][2]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int lc = t % kDcKChunk, lr = t / kDcKChunk;
  for (int kc = 0; kc < kDcNB; kc += kDcKChunk) {
#pragma unroll
    for (int s = 0; s < kDcNB / (kDcThreads / kDcKChunk); ++s) {
      const int r = lr + (kDcThreads / kDcKChunk) * s;
      ps[r * kDcKStride + lc] = r < prow ? P[r * ldp + kc + lc] : T(0);
      qs[r * kDcKStride + lc] = r < qrow ? Q[r * ldq + kc + lc] : T(0);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kDcKChunk / 4; ++kk) {
      const int col = 4 * kk + (lane >> 4);
      T av[2], bv[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        av[m] = ps[(wm + 16 * m + (lane & 15)) * kDcKStride + col];
        bv[m] = qs[(wn + 16 * m + (lane & 15)) * kDcKStride + col];
      }
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[m][q] = DcMfma<T>::Mma(av[m], bv[q], acc[m][q]);
    }
    __syncthreads();
  }
}

// L_ik = A_ik L_kk^-T for block row i = k + 1 + blockIdx.x, in place.
template <typename T>
__global__ __launch_bounds__(kDcThreads) void DcPanelKernel(T* __restrict__ M, int64_t ld, int64_t n, int64_t k,
                                                            const T* __restrict__ inv, const int* __restrict__ flag) {
  if (*flag) return;
  __shared__ T ps[kDcNB * kDcKStride], qs[kDcNB * kDcKStride];
  const int64_t i0 = (k + 1 + blockIdx.x) * kDcNB, k0 = k * kDcNB;
  const int rows = (int)(n - i0 < kDcNB ? n - i0 : kDcNB);
  T* tile = M + i0 * ld + k0;
  typename DcMfma<T>::Acc acc[2][2] = {};
  DcTileABt<T>(tile, ld, rows, inv + k * kDcTile, kDcNB, kDcNB, ps, qs, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm + 16 * m + DcMfma<T>::Row(lane, r), col = wn + 16 * q + (lane & 15);
        if (row < rows) tile[row * ld + col] = acc[m][q][r];
      }
}

// A_ij -= L_ik L_jk^T for the lower-triangle tile (i, j) of the block rows
// below panel k that this workgroup's grid position folds to.
template <typename T>
__global__ __launch_bounds__(kDcThreads) void DcTrailingKernel(T* __restrict__ M, int64_t ld, int64_t n, int64_t k,
                                                               const int* __restrict__ flag) {
  if (*flag) return;
  const DenseCholeskyTile tile = DenseCholeskyTrailingTile((int64_t)gridDim.x - 1, blockIdx.x, blockIdx.y);
  if (!tile.live) return;
  __shared__ T ps[kDcNB * kDcKStride], qs[kDcNB * kDcKStride];
  const int64_t i0 = (k + 1 + tile.i) * kDcNB, j0 = (k + 1 + tile.j) * kDcNB, k0 = k * kDcNB;
  const int prow = (int)(n - i0 < kDcNB ? n - i0 : kDcNB);
  const int qrow = (int)(n - j0 < kDcNB ? n - j0 : kDcNB);
  typename DcMfma<T>::Acc acc[2][2] = {};
  DcTileABt<T>(M + i0 * ld + k0, ld, prow, M + j0 * ld + k0, ld, qrow, ps, qs, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm + 16 * m + DcMfma<T>::Row(lane, r), col = wn + 16 * q + (lane & 15);
        const int64_t gr = i0 + row, gc = j0 + col;
        if (row < prow && col < qrow && gc <= gr) M[gr * ld + gc] -= acc[m][q][r];
      }
}

// One tile times a vector through LDS, summed by one lane per output in a
// fixed order.  kDcDirect: out[r] = sum_c M[r][c] in[c]; kDcTransposed:
// out[c] = sum_r M[r][c] in[r]; kDcSymmetric: kDcDirect with M[r][c] read at
// [max][min] (a diagonal tile of a matrix given by its lower triangle).
// nr rows and nc columns of the tile are valid.  tile: [NB][kDcPad]; ends
// with a barrier, so in, tile and out may be used again at once.
enum { kDcDirect = 0, kDcTransposed = 1, kDcSymmetric = 2 };
template <typename T, int kMode>
__device__ __forceinline__ void DcTileMatVec(const T* __restrict__ M, int64_t ld, int nr, int nc, const T* in,
                                             T* tile, T* out) {
  const int t = threadIdx.x, c = t % kDcNB;
#pragma unroll 4
  for (int s = 0; s < kDcNB / 4; ++s) {
    const int r = t / kDcNB + 4 * s;
    T m = T(0);
    if (r < nr && c < nc) {
      if (kMode == kDcSymmetric)
        m = r >= c ? M[r * ld + c] : M[c * ld + r];
      else
        m = M[r * ld + c];
    }
    tile[r * kDcPad + c] = m * in[kMode == kDcTransposed ? r : c];
  }
  __syncthreads();
  if (t < kDcNB) {
    T sum = T(0);
    if (kMode == kDcTransposed) {
      for (int r = 0; r < kDcNB; ++r) sum += tile[r * kDcPad + t];
    } else {
      for (int q = 0; q < kDcNB; ++q) sum += tile[t * kDcPad + q];
    }
    out[t] = sum;
  }
  __syncthreads();
}

// Step k of L y = v: workgroup b takes block row i = k + b.  Every workgroup
// forms y_k = L_kk^-1 v_k; row k stores it, a row below subtracts L_ik y_k
// from v_i.  v and y have `padded` entries, zero past n.
template <typename T>
__global__ __launch_bounds__(kDcThreads) void DcForwardKernel(const T* __restrict__ M, int64_t ld, int64_t n,
                                                              int64_t k, const T* __restrict__ inv, T* v, T* y,
                                                              const int* __restrict__ flag) {
  if (*flag) return;
  __shared__ T tile[kDcNB * kDcPad], vin[kDcNB], yk[kDcNB], vout[kDcNB];
  const int t = threadIdx.x;
  const int64_t i = k + blockIdx.x, k0 = k * kDcNB, i0 = i * kDcNB;
  if (t < kDcNB) vin[t] = v[k0 + t];
  __syncthreads();
  DcTileMatVec<T, kDcDirect>(inv + k * kDcTile, kDcNB, kDcNB, kDcNB, vin, tile, yk);
  if (i == k) {
    if (t < kDcNB) y[k0 + t] = yk[t];
    return;
  }
  const int rows = (int)(n - i0 < kDcNB ? n - i0 : kDcNB);
  DcTileMatVec<T, kDcDirect>(M + i0 * ld + k0, ld, rows, kDcNB, yk, tile, vout);
  if (t < kDcNB) v[i0 + t] -= vout[t];
}

// Step k of L^T x = y, k descending: workgroup i in [0, k].  Every workgroup
// forms x_k = L_kk^-T y_k; row k stores it into x, a row above subtracts
// L_ki^T x_k from y_i.
template <typename T>
__global__ __launch_bounds__(kDcThreads) void DcBackwardKernel(const T* __restrict__ M, int64_t ld, int64_t n,
                                                               int64_t k, const T* __restrict__ inv, T* y, T* x,
                                                               const int* __restrict__ flag) {
  if (*flag) return;
  __shared__ T tile[kDcNB * kDcPad], yin[kDcNB], xk[kDcNB], yout[kDcNB];
  const int t = threadIdx.x;
  const int64_t i = blockIdx.x, k0 = k * kDcNB, i0 = i * kDcNB;
  if (t < kDcNB) yin[t] = y[k0 + t];
  __syncthreads();
  DcTileMatVec<T, kDcTransposed>(inv + k * kDcTile, kDcNB, kDcNB, kDcNB, yin, tile, xk);
  if (i == k) {
    if (t < kDcNB) x[k0 + t] = xk[t];
    return;
  }
  const int rows = (int)(n - k0 < kDcNB ? n - k0 : kDcNB);
  DcTileMatVec<T, kDcTransposed>(M + k0 * ld + i0, ld, rows, kDcNB, xk, tile, yout);
  if (t < kDcNB) y[i0 + t] -= yout[t];
}

// ---- The vector kernels, one entry of the padded length per thread.

// v = rhs (zero past n): the FP64 solve's start.
__global__ __launch_bounds__(kDcThreads) void DcLoadKernel(const double* __restrict__ rhs, int64_t n, int64_t padded,
                                                           double* __restrict__ v, const int* __restrict__ flag) {
  if (*flag) return;
  const int64_t idx = (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
  if (idx < padded) v[idx] = idx < n ? rhs[idx] : 0.0;
}

// x = 0, r = rhs: the refinement loop's start (dense_cholesky.cc:606-608).
__global__ __launch_bounds__(kDcThreads) void DcRefineInitKernel(const double* __restrict__ rhs, int64_t n,
                                                                 int64_t padded, double* __restrict__ x,
                                                                 double* __restrict__ r, const int* __restrict__ flag) {
  if (*flag) return;
  const int64_t idx = (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
  if (idx < padded) {
    x[idx] = 0.0;
    r[idx] = idx < n ? rhs[idx] : 0.0;
  }
}

// r32 = (float) r (:612-613).
__global__ __launch_bounds__(kDcThreads) void DcCastKernel(const double* __restrict__ r, int64_t padded,
                                                           float* __restrict__ v, const int* __restrict__ flag) {
  if (*flag) return;
  const int64_t idx = (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
  if (idx < padded) v[idx] = (float)r[idx];
}

// x += (double) c, the up-cast and the sum in one kernel (CudaDsxpy, :627-630).
__global__ __launch_bounds__(kDcThreads) void DcAccumulateKernel(const float* __restrict__ c, int64_t padded,
                                                                 double* __restrict__ x, const int* __restrict__ flag) {
  if (*flag) return;
  const int64_t idx = (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
  if (idx < padded) x[idx] += (double)c[idx];
}

// d_x = the solution, or zeros after a failed factorization.
__global__ __launch_bounds__(kDcThreads) void DcStoreKernel(const double* __restrict__ x, int64_t n,
                                                            double* __restrict__ d_x, const int* __restrict__ flag) {
  const int64_t idx = (int64_t)blockIdx.x * kDcThreads + threadIdx.x;
  if (idx < n) d_x[idx] = *flag ? 0.0 : x[idx];
}

// r = rhs - A x in FP64 (:632-635), A by its lower triangle: workgroup i sums
// block row i's tiles in column order, a tile above the diagonal as the
// transpose of its mirror.  x and r have `padded` entries.
__global__ __launch_bounds__(kDcThreads) void DcResidualKernel(const double* __restrict__ A, int64_t ld, int64_t n,
                                                               const double* __restrict__ rhs,
                                                               const double* __restrict__ x, double* __restrict__ r,
                                                               const int* __restrict__ flag) {
  if (*flag) return;
  __shared__ double tile[kDcNB * kDcPad], xin[kDcNB], part[kDcNB];
  const int t = threadIdx.x;
  const int64_t i = blockIdx.x, i0 = i * kDcNB, panels = gridDim.x;
  const int rows = (int)(n - i0 < kDcNB ? n - i0 : kDcNB);
  double sum = 0.0;
  for (int64_t j = 0; j < panels; ++j) {
    const int64_t j0 = j * kDcNB;
    const int cols = (int)(n - j0 < kDcNB ? n - j0 : kDcNB);
    if (t < kDcNB) xin[t] = x[j0 + t];
    __syncthreads();
    if (j < i)
      DcTileMatVec<double, kDcDirect>(A + i0 * ld + j0, ld, rows, cols, xin, tile, part);
    else if (j == i)
      DcTileMatVec<double, kDcSymmetric>(A + i0 * ld + i0, ld, rows, rows, xin, tile, part);
    else
      DcTileMatVec<double, kDcTransposed>(A + j0 * ld + i0, ld, cols, rows, xin, tile, part);
    if (t < kDcNB) sum += part[t];
  }
  if (t < kDcNB) r[i0 + t] = i0 + t < n ? rhs[i0 + t] - sum : 0.0;
}

}  // namespace cse

#endif  // CSE_DENSE_CHOLESKY_KERNELS_HPP_
