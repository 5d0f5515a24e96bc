// sparse_cholesky_kernels.hpp -- the kernels of cse_sparse_cholesky_* (DESIGN
// section 3.6i): a left-looking Cholesky factorization of a symmetric matrix
// of 9 x 9 blocks, one level of the elimination tree per pair of launches, and
// the level-ordered substitutions and the residual of its solve.  FP64.
//
//   ScGatherKernel    L's blocks start as P A P^T: each takes its input block,
//       transposed where the plan says so, or zeros (fill).
//   ScDiagKernel      one wave per column j of the level: A_jj - sum_k L_jk
//       L_jk^T over block row j, k ascending, on the matrix cores
//       (v_mfma_f64_16x16x4_f64, three per 9 x 9 x 9 product); the 9 x 9
//       Cholesky in LDS (the pivot test sees NaN and Inf: this TU is built
//       without -ffinite-math-only); L_jj and L_jj^-1 stored, the column's
//       status word written: 0, or 1 + the first local column whose pivot failed.
//   ScTargetKernel    one wave per off-diagonal block (i, j) of the level's
//       columns: the sorted block rows i and j are merged up to column j (the
//       walk is wave-uniform: scalar loads and branches), A_ij - sum_k L_ik
//       L_jk^T accumulated transposed, k ascending, then multiplied by
//       L_jj^-1 from the left, which is L_ij transposed, and stored.
//   ScInfoKernel      the smallest failed scalar column + 1 over the status words.
//   ScForwardKernel, ScBackwardKernel  one wave per block row / column of the
//       level, gather form: rows through the row arrays, columns through the
//       column index; the seven partial sums are added in a fixed order.
//   ScResidualKernel  r = rhs - A x from the input blocks, upper blocks through
//       the row arrays, lower ones through the input's column index.
// Ordering between waves comes from kernel boundaries only: every block a
// level reads belongs to a column on a lower level.  No atomics; every sum in
// a fixed order that does not depend on the launch geometry.  Offsets are 64-bit.
#ifndef CSE_SPARSE_CHOLESKY_KERNELS_HPP_
#define CSE_SPARSE_CHOLESKY_KERNELS_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

namespace cse {

constexpr int kScB = 9;                // block size
constexpr int kScBlock = kScB * kScB;  // doubles of a block
constexpr int kScWave = 64;
constexpr int kScThreads = 256;        // the elementwise kernels
constexpr int kScSlots = 7;            // blocks a wave of the solve works on at once: 7 x 9 lanes

typedef double ScDouble4 __attribute__((ext_vector_type(4)));

// L and the input as the kernels see them.
struct ScFactor {
  const int64_t* row_begin;
  const int32_t* block_col;
  const int32_t* block_row;
  const int64_t* col_begin;
  const int32_t* col_block;
  double* L;        // [num_factor_blocks][81]
  double* inverse;  // [N][81]: L_jj^-1, strict upper triangle zero
};

__device__ __forceinline__ void ScWaveSync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Positive and finite; NaN fails both comparisons.
__device__ __forceinline__ bool ScPivotOk(double d) { return d > 0.0 && d <= std::numeric_limits<double>::max(); }

// acc(m, n) -= sum_q X[m][q] Y[n][q] for two row-major 9 x 9 blocks.  Lane l
// holds A[m = l % 16][k = l / 16] and B[k = l / 16][n = l % 16]; the
// accumulator's entry r is C[l / 16 + 4 r][l % 16].  Rows, columns and q
// beyond 9 are zeros.
__device__ __forceinline__ ScDouble4 ScSubtractProduct(const double* X, const double* Y, ScDouble4 acc, int lane) {
  const int col = lane & 15, rsub = lane >> 4;
  double x[3], y[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int q = 4 * s + rsub;
    const bool live = col < kScB && q < kScB;
    x[s] = live ? X[col * kScB + q] : 0.0;
    y[s] = live ? Y[col * kScB + q] : 0.0;
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-x[s], y[s], acc, 0, 0, 0);
  return acc;
}

__global__ __launch_bounds__(kScThreads) void ScGatherKernel(const double* __restrict__ values,
                                                              const int32_t* __restrict__ source, int64_t entries,
                                                              double* __restrict__ L) {
  const int64_t idx = (int64_t)blockIdx.x * kScThreads + threadIdx.x;
  if (idx >= entries) return;
  const int64_t t = idx / kScBlock;
  const int e = (int)(idx - t * kScBlock);
  const int32_t src = source[t];
  double v = 0.0;
  if (src != -1) {  // the input block src, or -2 - src transposed (cse::SparseCholeskyPlan::source)
    const int at = src < 0 ? (e % kScB) * kScB + e / kScB : e;
    v = values[(int64_t)(src < 0 ? -2 - src : src) * kScBlock + at];
  }
  L[idx] = v;
}

__global__ __launch_bounds__(kScWave) void ScDiagKernel(ScFactor F, const int32_t* __restrict__ columns,
                                                        int* __restrict__ status) {
  __shared__ double a[kScBlock], x[kScBlock];
  const int lane = threadIdx.x, col = lane & 15, rsub = lane >> 4;
  const int32_t j = columns[blockIdx.x];
  const int64_t first = F.row_begin[j], diag = F.row_begin[j + 1] - 1;
  double* out = F.L + diag * kScBlock;
  ScDouble4 acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = rsub + 4 * r;
    acc[r] = (m < kScB && col < kScB) ? out[m * kScB + col] : 0.0;
  }
  for (int64_t b = first; b < diag; ++b) acc = ScSubtractProduct(F.L + b * kScBlock, F.L + b * kScBlock, acc, lane);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int m = rsub + 4 * r;
    if (m < kScB && col < kScB) a[m * kScB + col] = acc[r];
  }
  ScWaveSync();
  // The lower triangle's 45 entries, one lane each: lane -> (row, column).
  int tr = 0;
  while ((tr + 1) * (tr + 2) / 2 <= lane) ++tr;
  const int tc = lane - tr * (tr + 1) / 2;
  const bool lower = lane < kScB * (kScB + 1) / 2;
  int fail = 0;
  for (int k = 0; k < kScB; ++k) {
    const double p = a[k * kScB + k];
    if (!ScPivotOk(p) && fail == 0) fail = k + 1;
    const double s = sqrt(p);  // NaN for a negative pivot: it spreads to every block that reads this column
    ScWaveSync();
    if (lower && tc == k) a[tr * kScB + k] = tr == k ? s : a[tr * kScB + k] / s;
    ScWaveSync();
    if (lower && tc > k) a[tr * kScB + tc] -= a[tr * kScB + k] * a[tc * kScB + k];
    ScWaveSync();
  }
  // Column c of L_jj^-1 by lane c, top down.
  if (lane < kScB) {
    const int c = lane;
    for (int r = 0; r < kScB; ++r) {
      double s = 0.0;
      for (int q = 0; q < r; ++q)
        if (q >= c) s += a[r * kScB + q] * x[q * kScB + c];
      x[r * kScB + c] = r < c ? 0.0 : (r == c ? 1.0 : -s) / a[r * kScB + r];
    }
  }
  ScWaveSync();
  double* inv = F.inverse + (int64_t)j * kScBlock;
  for (int e = lane; e < kScBlock; e += kScWave) {
    out[e] = e % kScB <= e / kScB ? a[e] : 0.0;
    inv[e] = x[e];
  }
  if (lane == 0) status[j] = fail;
}

__global__ __launch_bounds__(kScWave) void ScTargetKernel(ScFactor F, const int32_t* __restrict__ targets) {
  const int lane = threadIdx.x, col = lane & 15, rsub = lane >> 4;
  const int32_t t = targets[blockIdx.x];
  const int32_t i = F.block_row[t], j = F.block_col[t];
  double* out = F.L + (int64_t)t * kScBlock;
  // The transposed target: acc(m, n) = A_ij[n][m].
  ScDouble4 acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = rsub + 4 * r;
    acc[r] = (m < kScB && col < kScB) ? out[col * kScB + m] : 0.0;
  }
  int64_t pa = F.row_begin[i], pb = F.row_begin[j];
  const int64_t ea = F.row_begin[i + 1] - 1, eb = F.row_begin[j + 1] - 1;
  while (pa < ea && pb < eb) {
    const int32_t ca = F.block_col[pa], cb = F.block_col[pb];
    if (ca >= j) break;
    if (ca == cb) {
      acc = ScSubtractProduct(F.L + pb * kScBlock, F.L + pa * kScBlock, acc, lane);
      ++pa, ++pb;
    } else if (ca < cb) {
      ++pa;
    } else {
      ++pb;
    }
  }
  // L_ij^T = L_jj^-1 (A_ij - sum)^T: the accumulator is the product's B operand as it stands.
  const double* inv = F.inverse + (int64_t)j * kScBlock;
  ScDouble4 res = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int q = 4 * s + rsub;
    const double m = (col < kScB && q < kScB) ? inv[col * kScB + q] : 0.0;
    res = __builtin_amdgcn_mfma_f64_16x16x4f64(m, acc[s], res, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int m = rsub + 4 * r;
    if (m < kScB && col < kScB) out[col * kScB + m] = res[r];
  }
}

__global__ __launch_bounds__(kScThreads) void ScInfoKernel(const int* __restrict__ status, int64_t N,
                                                            int* __restrict__ info) {
  __shared__ int best[kScThreads];
  int mine = std::numeric_limits<int>::max();
  for (int64_t j = threadIdx.x; j < N; j += kScThreads)
    if (status[j] != 0) {
      const int at = (int)(kScB * j) + status[j];
      mine = at < mine ? at : mine;
    }
  best[threadIdx.x] = mine;
  __syncthreads();
  for (int w = kScThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w && best[threadIdx.x + w] < best[threadIdx.x]) best[threadIdx.x] = best[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *info = best[0] == std::numeric_limits<int>::max() ? 0 : best[0];
}

// y[position k] = rhs[block row permutation[k]].
__global__ __launch_bounds__(kScThreads) void ScLoadKernel(const double* __restrict__ rhs,
                                                            const int32_t* __restrict__ permutation, int64_t entries,
                                                            double* __restrict__ y) {
  const int64_t idx = (int64_t)blockIdx.x * kScThreads + threadIdx.x;
  if (idx >= entries) return;
  const int64_t k = idx / kScB;
  y[idx] = rhs[(int64_t)permutation[k] * kScB + (idx - k * kScB)];
}

// dst[block row permutation[k]] (dst[k] without a permutation) = or += src[k];
// an assignment after a failed factorization stores zeros.
__global__ __launch_bounds__(kScThreads) void ScStoreKernel(const double* __restrict__ src,
                                                             const int32_t* __restrict__ permutation, int64_t entries,
                                                             const int* __restrict__ info, bool add, double* dst) {
  const int64_t idx = (int64_t)blockIdx.x * kScThreads + threadIdx.x;
  if (idx >= entries) return;
  const int64_t k = idx / kScB;
  const int64_t at = permutation ? (int64_t)permutation[k] * kScB + (idx - k * kScB) : idx;
  const double v = src[idx];
  if (add)
    dst[at] += v;
  else
    dst[at] = *info ? 0.0 : v;
}

// The seven slots' partial sums of entry e, added in slot order.
__device__ __forceinline__ double ScSlotSum(const double* part, int e) {
  double s = part[e];
#pragma unroll
  for (int q = 1; q < kScSlots; ++q) s += part[q * kScB + e];
  return s;
}

// y_i = L_ii^-1 (y_i - sum_k L_ik y_k), in place.
__global__ __launch_bounds__(kScWave) void ScForwardKernel(ScFactor F, const int32_t* __restrict__ columns,
                                                           double* y) {
  __shared__ double part[kScSlots * kScB], t[kScB];
  const int lane = threadIdx.x, slot = lane / kScB, r = lane - slot * kScB;
  const int32_t i = columns[blockIdx.x];
  const int64_t first = F.row_begin[i], diag = F.row_begin[i + 1] - 1;
  if (slot < kScSlots) {
    double s = 0.0;
    for (int64_t b = first + slot; b < diag; b += kScSlots) {
      const double* B = F.L + b * kScBlock + r * kScB;
      const double* v = y + (int64_t)F.block_col[b] * kScB;
#pragma unroll
      for (int c = 0; c < kScB; ++c) s += B[c] * v[c];
    }
    part[lane] = s;
  }
  ScWaveSync();
  if (lane < kScB) t[lane] = y[(int64_t)i * kScB + lane] - ScSlotSum(part, lane);
  ScWaveSync();
  if (lane < kScB) {
    const double* M = F.inverse + (int64_t)i * kScBlock + lane * kScB;
    double s = 0.0;
    for (int c = 0; c <= lane; ++c) s += M[c] * t[c];
    y[(int64_t)i * kScB + lane] = s;
  }
}

// x_j = L_jj^-T (y_j - sum_{i > j} L_ij^T x_i), in place.
__global__ __launch_bounds__(kScWave) void ScBackwardKernel(ScFactor F, const int32_t* __restrict__ columns,
                                                            double* y) {
  __shared__ double part[kScSlots * kScB], t[kScB];
  const int lane = threadIdx.x, slot = lane / kScB, c = lane - slot * kScB;
  const int32_t j = columns[blockIdx.x];
  if (slot < kScSlots) {
    double s = 0.0;
    for (int64_t k = F.col_begin[j] + slot; k < F.col_begin[j + 1]; k += kScSlots) {
      const int32_t b = F.col_block[k];
      const double* B = F.L + (int64_t)b * kScBlock + c;
      const double* v = y + (int64_t)F.block_row[b] * kScB;
#pragma unroll
      for (int r = 0; r < kScB; ++r) s += B[r * kScB] * v[r];
    }
    part[lane] = s;
  }
  ScWaveSync();
  if (lane < kScB) t[lane] = y[(int64_t)j * kScB + lane] - ScSlotSum(part, lane);
  ScWaveSync();
  if (lane < kScB) {
    const double* M = F.inverse + (int64_t)j * kScBlock + lane;
    double s = 0.0;
    for (int r = lane; r < kScB; ++r) s += M[r * kScB] * t[r];
    y[(int64_t)j * kScB + lane] = s;
  }
}

// The input as the residual reads it.
struct ScInput {
  const int64_t* row_begin;
  const int32_t* block_col;
  const int64_t* col_begin;
  const int32_t* col_block;
  const int32_t* col_row;
  const int32_t* position;
  const double* values;
};

// y[position of i] = rhs_i - sum_c A(i, c) x_c - sum_{r < i} A(r, i)^T x_r: one
// wave per block row of the input, each slot its upper blocks and then its
// lower ones.
__global__ __launch_bounds__(kScWave) void ScResidualKernel(ScInput A, const double* __restrict__ rhs,
                                                            const double* __restrict__ x, double* __restrict__ y) {
  __shared__ double part[kScSlots * kScB];
  const int lane = threadIdx.x, slot = lane / kScB, r = lane - slot * kScB;
  const int64_t i = blockIdx.x;
  if (slot < kScSlots) {
    double s = 0.0;
    for (int64_t b = A.row_begin[i] + slot; b < A.row_begin[i + 1]; b += kScSlots) {
      const double* B = A.values + b * kScBlock + r * kScB;
      const double* v = x + (int64_t)A.block_col[b] * kScB;
#pragma unroll
      for (int c = 0; c < kScB; ++c) s += B[c] * v[c];
    }
    for (int64_t k = A.col_begin[i] + slot; k < A.col_begin[i + 1]; k += kScSlots) {
      const double* B = A.values + (int64_t)A.col_block[k] * kScBlock + r;
      const double* v = x + (int64_t)A.col_row[k] * kScB;
#pragma unroll
      for (int c = 0; c < kScB; ++c) s += B[c * kScB] * v[c];
    }
    part[lane] = s;
  }
  ScWaveSync();
  if (lane < kScB) y[(int64_t)A.position[i] * kScB + lane] = rhs[i * kScB + lane] - ScSlotSum(part, lane);
}

}  // namespace cse

#endif  // CSE_SPARSE_CHOLESKY_KERNELS_HPP_
