// cgnr_kernels.hpp -- cse_cgnr_init's block-Jacobi preconditioner on the
// Jacobian values in HBM: BlockCRSJacobiPreconditioner::UpdateImpl
// (internal/ceres/block_jacobi_preconditioner.cc:158-224), which the reference
// runs on the CPU and copies over on every solve (cgnr_solver.cc:254-280).
//
//   Gram      G_b = sum over the cells of parameter block b of J_cell^T J_cell,
//             the upper triangle, into the block's row-major
//             tangent_size x tangent_size values (zero-filled by the host).
//             Affine groups with gradient plans: slot by slot in the three forms
//             of the squared column norm (operator_kernels.hpp) with
//             S (S + 1) / 2 sums where that has S -- a fixed order, no atomics.
//             Every other group: one lane per residual block and FP64 atomics
//             (GramBlockKernel), addressed as ColumnBlockKernel addresses.
//   Invert    per block: mirror the upper triangle, add D^2 on the diagonal,
//             Cholesky in place, M = L^-T L^-1 (:208-221, m.llt().solve(I)).
//
// linear_operators.hip's alone: it owns the plain (non-template) kernels here
// (DtDxpyKernel, GramBlockKernel).
#ifndef CSE_CGNR_KERNELS_HPP_
#define CSE_CGNR_KERNELS_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "column_kernels.hpp"
#include "operator_kernels.hpp"

namespace cse {

// y += D .* D .* x (CudaVector::DtDxpy, cgnr_solver.cc:236): cse_cgnr_multiply's.
__global__ __launch_bounds__(kBlockThreads) void DtDxpyKernel(const double* D, const double* x,
                                                              double* y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (i < n) y[i] += D[i] * D[i] * x[i];
}

constexpr int GramCount(int s) { return s * (s + 1) / 2; }

// acc (packed upper triangle, row-major) += row^T row.
template <int S>
__device__ __forceinline__ void GramAddRow(const double (&v)[S], double (&acc)[GramCount(S)]) {
  int t = 0;
#pragma unroll
  for (int r = 0; r < S; ++r)
#pragma unroll
    for (int c = r; c < S; ++c) acc[t++] += v[r] * v[c];
}

// dst (row-major S x S) upper triangle += acc.
template <int S>
__device__ __forceinline__ void GramStore(const double (&acc)[GramCount(S)], double* dst) {
  int t = 0;
#pragma unroll
  for (int r = 0; r < S; ++r)
#pragma unroll
    for (int c = r; c < S; ++c) dst[r * S + c] += acc[t++];
}

// Identity order (g.perm == null): parameter block p's cells are the blocks
// [off[p], off[p + 1]).  One wave per 64 parameter blocks; the cells of a tile
// of 64 blocks are read coalesced into LDS and each lane adds its own blocks'
// rows from there (ColumnNormRangeKernel's walk).  values: the first parameter
// block's S x S block.
template <int NR, int S>
__global__ __launch_bounds__(kWave) void GramRangeKernel(const GradArgs g, double* values) {
  constexpr int E = NR * S;
  constexpr int T = kWave;  // blocks per tile
  __shared__ double cell[T * E];
  const int lane = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * kWave;
  const int64_t p = p0 + lane;
  const int64_t pend = p0 + kWave < g.count ? p0 + kWave : g.count;
  const int64_t B0 = g.off[p0], B1 = g.off[pend];
  const int64_t my0 = p < g.count ? g.off[p] : B1, my1 = p < g.count ? g.off[p + 1] : B1;
  double acc[GramCount(S)];
#pragma unroll
  for (int t = 0; t < GramCount(S); ++t) acc[t] = 0.0;
  for (int64_t t0 = B0; t0 < B1; t0 += T) {
    const int nb = B1 - t0 < T ? (int)(B1 - t0) : T;
#pragma unroll
    for (int it = 0; it < E; ++it) {
      const int t = it * kWave + lane;  // element t of the tile
      const int bm = t / E, e = t - bm * E, k = e / S, cc = e - k * S;
      double v = 0.0;
      if (bm < nb) v = g.jac[g.jrow[k] + g.jstride * (t0 + bm) + cc];
      cell[t] = v;
    }
    __syncthreads();
    const int64_t lo = my0 > t0 ? my0 : t0, hi = my1 < t0 + nb ? my1 : t0 + nb;
    for (int64_t b = lo; b < hi; ++b) {
      const int bm = (int)(b - t0);
#pragma unroll
      for (int k = 0; k < NR; ++k) {
        double v[S];
#pragma unroll
        for (int cc = 0; cc < S; ++cc) v[cc] = cell[bm * E + k * S + cc];
        GramAddRow<S>(v, acc);
      }
    }
    __syncthreads();
  }
  if (p < g.count) GramStore<S>(acc, values + (int64_t)(S * S) * p);
}

// One wave per chunk of at most kGradChunk blocks of one parameter block:
// lane per block, a fixed xor-butterfly, the chunk's partial
// (ch.partial: [nchunks][S (S + 1) / 2], a buffer of cse_cgnr_init's own).
template <int NR, int S>
__global__ __launch_bounds__(kBlockThreads) void GramLanesKernel(const GradArgs g, const GradChunks ch) {
  constexpr int K = GramCount(S);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t cid = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  if (cid >= ch.nchunks) return;
  const int64_t q1 = ch.begin[cid + 1];
  double acc[K];
#pragma unroll
  for (int t = 0; t < K; ++t) acc[t] = 0.0;
  for (int64_t q = ch.begin[cid] + lane; q < q1; q += kWave) {
    const int64_t b = g.perm ? (int64_t)g.perm[q] : q;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const double* row = g.jac + g.jrow[k] + g.jstride * b;
      double v[S];
#pragma unroll
      for (int c = 0; c < S; ++c) v[c] = row[c];
      GramAddRow<S>(v, acc);
    }
  }
#pragma unroll
  for (int t = 0; t < K; ++t)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[t] += __shfl_xor(acc[t], off, kWave);
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < K; ++t) ch.partial[cid * K + t] = acc[t];
  }
}

// Each parameter block adds its chunks' partials in chunk order.
template <int S>
__global__ __launch_bounds__(kBlockThreads) void GramChunkReduceKernel(const GradArgs g, const GradChunks ch,
                                                                      double* values) {
  constexpr int K = GramCount(S);
  const int64_t p = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (p >= g.count || ch.chunk_off[p] == ch.chunk_off[p + 1]) return;
  double acc[K];
#pragma unroll
  for (int t = 0; t < K; ++t) acc[t] = 0.0;
  for (int64_t q = ch.chunk_off[p]; q < ch.chunk_off[p + 1]; ++q)
#pragma unroll
    for (int t = 0; t < K; ++t) acc[t] += ch.partial[q * K + t];
  GramStore<S>(acc, values + (int64_t)(S * S) * p);
}

// One lane per parameter block (few blocks each, not in block order).
template <int NR, int S>
__global__ __launch_bounds__(kBlockThreads) void GramSlotKernel(const GradArgs g, double* values) {
  const int64_t p = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (p >= g.count) return;
  double acc[GramCount(S)];
#pragma unroll
  for (int t = 0; t < GramCount(S); ++t) acc[t] = 0.0;
  for (int64_t q = g.off[p]; q < g.off[p + 1]; ++q) {
    const int64_t b = g.perm ? (int64_t)g.perm[q] : q;
#pragma unroll
    for (int k = 0; k < NR; ++k) {
      const double* row = g.jac + g.jrow[k] + g.jstride * b;
      double v[S];
#pragma unroll
      for (int c = 0; c < S; ++c) v[c] = row[c];
      GramAddRow<S>(v, acc);
    }
  }
  GramStore<S>(acc, values + (int64_t)(S * S) * p);
}

// The table entry whose columns start at `delta` (the table is sorted by
// delta_offset and has one entry per non-constant block), or -1.
__device__ __forceinline__ int64_t FindCgnrBlockDev(const CgnrBlock* tab, int64_t ntab, int64_t delta) {
  int64_t lo = 0, hi = ntab;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (tab[mid].delta_offset < delta)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < ntab && tab[lo].delta_offset == delta ? lo : -1;
}

// One lane per residual block, FP64 atomics: the table path, held cameras,
// shapes without an affine norm kernel and affine groups without a gradient
// plan (ColumnBlockKernel's addressing, column_kernels.hpp).
__global__ __launch_bounds__(kBlockThreads) void GramBlockKernel(const ColumnBlockArgs a, const double* jac,
                                                                 const CgnrBlock* tab, int64_t ntab,
                                                                 double* values) {
  const int64_t i = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= a.n) return;
  int64_t q = 0;
  if (!a.affine) q = a.jac_layout[a.gindex ? a.gindex[i] : a.first + i];
  for (int j = 0; j < a.nb; ++j) {
    const int32_t id = a.ids[i * a.nb + j];
    int64_t col0;
    int cols = a.sz[j];
    if (a.affine) {
      col0 = a.delta_base[j] + (int64_t)cols * id;
    } else {
      const PbDev pb = a.pbs[id];
      if (pb.is_constant) continue;
      col0 = pb.delta_offset;
      cols = pb.tangent_size < cols ? pb.tangent_size : cols;
    }
    const int64_t q0 = q;
    if (!a.affine) q += a.nr;
    const int64_t e = FindCgnrBlockDev(tab, ntab, col0);
    if (e < 0) continue;
    const CgnrBlock blk = tab[e];
    if (cols > blk.tangent_size) cols = blk.tangent_size;
    double* dst = values + blk.value_offset;
    for (int r = 0; r < cols; ++r)
      for (int c = r; c < cols; ++c) {
        double s = 0.0;
        for (int k = 0; k < a.nr; ++k) {
          const double* row = jac + (a.affine ? a.jac_base[j][k] + a.jac_stride[j] * i : a.jac_offsets[q0 + k]);
          s += row[r] * row[c];
        }
        unsafeAtomicAdd(dst + r * blk.tangent_size + c, s);
      }
  }
}

// m: row-major S x S in global memory whose upper triangle holds G; d: the
// block's entries of D, or null.  Writes M = (G + diag(d^2))^-1, both
// triangles, by the Cholesky factor; false (and m = 0) when a pivot is not
// positive and finite (PivotOk, operator_kernels.hpp).  A holds L below the
// diagonal, 1 / L_jj on it and L^-1 transposed above it.
template <int S>
__device__ __forceinline__ bool InvertSpdBlock(double* m, const double* d) {
  double A[S][S];
#pragma unroll
  for (int r = 0; r < S; ++r)
#pragma unroll
    for (int c = r; c < S; ++c) {
      double v = m[r * S + c];
      if (r == c && d) v += d[r] * d[r];
      A[c][r] = v;  // the lower triangle
    }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    double p = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) p -= A[j][k] * A[j][k];
    ok = ok && PivotOk(p);
    const double inv = 1.0 / sqrt(p);
    A[j][j] = inv;
#pragma unroll
    for (int i = j + 1; i < S; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= A[i][k] * A[j][k];
      A[i][j] = s * inv;
    }
  }
  if (!ok) {
#pragma unroll
    for (int t = 0; t < S * S; ++t) m[t] = 0.0;
    return false;
  }
  // L^-1, column by column: X_jj = 1 / L_jj, X_ij = -(sum_{j <= k < i} L_ik X_kj) / L_ii,
  // X_ij kept at A[j][i].
#pragma unroll
  for (int j = 0; j < S; ++j)
#pragma unroll
    for (int i = j + 1; i < S; ++i) {
      double s = A[i][j] * A[j][j];
#pragma unroll
      for (int k = j + 1; k < i; ++k) s += A[i][k] * A[j][k];
      A[j][i] = -s * A[i][i];
    }
  // M = X^T X: M_rc = sum_{k >= max(r, c)} X_kr X_kc.
#pragma unroll
  for (int r = 0; r < S; ++r)
#pragma unroll
    for (int c = r; c < S; ++c) {
      double s = 0.0;
#pragma unroll
      for (int k = c; k < S; ++k) s += A[r][k] * A[c][k];
      m[r * S + c] = s;
      m[c * S + r] = s;
    }
  return true;
}

// The same for a run-time size up to kCgnrMaxBlockColumns (sizes above 10).
__device__ inline bool InvertSpdBlockAny(int S, double* m, const double* d) {
  double A[kCgnrMaxBlockColumns][kCgnrMaxBlockColumns];
  for (int r = 0; r < S; ++r)
    for (int c = r; c < S; ++c) {
      double v = m[r * S + c];
      if (r == c && d) v += d[r] * d[r];
      A[c][r] = v;
    }
  bool ok = true;
  for (int j = 0; j < S; ++j) {
    double p = A[j][j];
    for (int k = 0; k < j; ++k) p -= A[j][k] * A[j][k];
    ok = ok && PivotOk(p);
    const double inv = 1.0 / sqrt(p);
    A[j][j] = inv;
    for (int i = j + 1; i < S; ++i) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s -= A[i][k] * A[j][k];
      A[i][j] = s * inv;
    }
  }
  if (!ok) {
    for (int t = 0; t < S * S; ++t) m[t] = 0.0;
    return false;
  }
  for (int j = 0; j < S; ++j)
    for (int i = j + 1; i < S; ++i) {
      double s = A[i][j] * A[j][j];
      for (int k = j + 1; k < i; ++k) s += A[i][k] * A[j][k];
      A[j][i] = -s * A[i][i];
    }
  for (int r = 0; r < S; ++r)
    for (int c = r; c < S; ++c) {
      double s = 0.0;
      for (int k = c; k < S; ++k) s += A[r][k] * A[c][k];
      m[r * S + c] = s;
      m[c * S + r] = s;
    }
  return true;
}

// AddDiagonalAndInvert: one parameter block per lane.  Sizes 1 to 10 in
// registers; kAny adds the run-time loop for 11 to kCgnrMaxBlockColumns (the
// host launches it only when the table has such a block).  A block whose
// factorisation fails is left zero and raises the status word cse_wait reads,
// as cse_schur_init's.
template <bool kAny>
__global__ __launch_bounds__(kWave) void CgnrInvertKernel(const CgnrBlock* tab, int64_t ntab, const double* D,
                                                          double* values, int* status) {
  const int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (i >= ntab) return;
  const CgnrBlock blk = tab[i];
  double* m = values + blk.value_offset;
  const double* d = D ? D + blk.delta_offset : nullptr;
  bool ok = true;
  switch (blk.tangent_size) {
    case 1: ok = InvertSpdBlock<1>(m, d); break;
    case 2: ok = InvertSpdBlock<2>(m, d); break;
    case 3: ok = InvertSpdBlock<3>(m, d); break;
    case 4: ok = InvertSpdBlock<4>(m, d); break;
    case 5: ok = InvertSpdBlock<5>(m, d); break;
    case 6: ok = InvertSpdBlock<6>(m, d); break;
    case 7: ok = InvertSpdBlock<7>(m, d); break;
    case 8: ok = InvertSpdBlock<8>(m, d); break;
    case 9: ok = InvertSpdBlock<9>(m, d); break;
    case 10: ok = InvertSpdBlock<10>(m, d); break;
    default:
      if constexpr (kAny) {
        ok = InvertSpdBlockAny(blk.tangent_size, m, d);
      } else {
        // The host launches kAny when the table has such a block; one that
        // arrives here all the same is left zero and reported.
        for (int t = 0; t < blk.tangent_size * blk.tangent_size; ++t) m[t] = 0.0;
        ok = false;
      }
      break;
  }
  if (!ok) *status = 1;
}

}  // namespace cse

#endif  // CSE_CGNR_KERNELS_HPP_
