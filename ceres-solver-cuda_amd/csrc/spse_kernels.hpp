// spse_kernels.hpp -- the vector kernels of cse_schur_power_series: the
// reference's PowerSeriesExpansionPreconditioner (internal/ceres/power_series_
// expansion_preconditioner.cc:51-72) with every vector, norm and the stop test
// on the device.
//
//   y = P^-1 x;  prev = y;  threshold = tolerance |y|            SpseZeroKernel
//   for i = 1, 2, ...:
//     t = Q prev        the kSchurSeries point pass and the contribution
//                       reduce (schur_kernels.hpp), into a zeroed t
//     term = P^-1 t;  y += term;  prev = term;  |term|;          SpseTermKernel
//     stop if i >= max_num_iterations or |term| < threshold
// with P = blockdiag(F^T F + D_f^2), Q = F^T E (E^T E + D_e^2)^-1 E^T F.
//
// One workgroup of kCgThreads lanes per kernel for every vector length, as the
// PCG's vector kernels (cg_kernels.hpp) and for their reason: the norm's order
// depends on n alone, there is no second launch shape.  Lane 0 runs the
// transitions of spse_state.hpp on the state in device memory.
//
// Frozen after termination: SpseTermKernel returns at once when state->done is
// set, so the terms the host enqueued past the end leave y as it was (the
// point passes between them write t and the contribution records only).
//
// The block apply is SchurPrecondApplyKernel's sum, product by product in the
// same order and contracted as the compiler contracts that kernel's (fma), so
// the zeroth term is cse_schur_precondition's under a JACOBI init.
//
// Included by cg_kernels.hip alone (it uses cg_kernels.hpp's CgBlockSum).
#ifndef CSE_SPSE_KERNELS_HPP_
#define CSE_SPSE_KERNELS_HPP_

#include "cg_kernels.hpp"

namespace cse {

// Entry k of P^-1 v: row k of its camera's block, or 0 outside the blocks'
// entries [pre_off, pre_off + pre_n).
__device__ __forceinline__ double SpseBlockApply(const SpseArgs& a, const double* v, int64_t k) {
  const int64_t j = k - a.pre_off;
  if (j < 0 || j >= a.pre_n) return 0.0;
  const int64_t blk = j / 9;
  const int row = (int)(j - 9 * blk);
  const double* m = a.blocks + 81 * blk + 9 * row;
  const double* vb = v + a.pre_off + 9 * blk;
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < 9; ++c) s = __builtin_fma(m[c], vb[c], s);
  return s;
}

// kAccumulate: y += P^-1 x (cse_schur_precondition's contract) instead of
// y = P^-1 x.
template <bool kAccumulate>
__global__ __launch_bounds__(kCgThreads) void SpseZeroKernel(const SpseArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[1][kCgWaves];
  double acc[1] = {0.0};
  for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) {
    const double v = SpseBlockApply(a, a.x, k);
    a.prev[k] = v;
    a.y[k] = kAccumulate ? a.y[k] + v : v;
    acc[0] += v * v;
  }
  CgBlockSum<1>(acc, lds);
  if (threadIdx.x == 0) SpseBegin(a.state, sqrt(acc[0]), a.tolerance);
}

__global__ __launch_bounds__(kCgThreads) void SpseTermKernel(const SpseArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[1][kCgWaves];
  if (a.state->done) return;
  double acc[1] = {0.0};
  for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) {
    const double v = SpseBlockApply(a, a.t, k);
    a.prev[k] = v;
    a.y[k] = a.y[k] + v;
    acc[0] += v * v;
  }
  CgBlockSum<1>(acc, lds);
  if (threadIdx.x == 0) SpseTerm(a.state, sqrt(acc[0]), a.max_num_iterations);
}

// The PCG's direction step (conjugate_gradients_solver.h:162-190) with z as
// given: rho = r'z, the rho / beta tests, p = z + beta p.  CgDirectionKernel
// without its block apply, for a preconditioner that wrote z itself.
__global__ __launch_bounds__(kCgThreads) void CgDirectionGivenKernel(const CgArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[1][kCgWaves];
  __shared__ double beta_s;
  __shared__ int go;  // 0: stop, 1: p = z, 2: p = z + beta p
  if (a.state->done) return;
  double acc[1] = {0.0};
  for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) acc[0] += a.r[k] * a.z[k];
  CgBlockSum<1>(acc, lds);
  if (threadIdx.x == 0) {
    const bool cont = CgDirection(a.state, acc[0]);
    go = !cont ? 0 : a.state->iteration == 1 ? 1 : 2;
    beta_s = a.state->beta;
  }
  __syncthreads();
  if (go == 0) return;
  if (go == 1) {
    for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) a.p[k] = a.z[k];
  } else {
    const double beta = beta_s;
    for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) a.p[k] = a.z[k] + beta * a.p[k];
  }
}

}  // namespace cse

#endif  // CSE_SPSE_KERNELS_HPP_
