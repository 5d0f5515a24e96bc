// cg_kernels.hpp -- the vector algebra of cse_schur_solve: ConjugateGradients-
// Solver (internal/ceres/conjugate_gradients_solver.h:108-305) with every
// vector, scalar and stopping test on the device.
//
// Two kernels per iteration besides the operator's product:
//   CgDirectionKernel  z = M^-1 r, rho = r'z, the rho / beta tests, p = z + beta p
//   CgUpdateKernel     pq = p'q and its tests, alpha, x += alpha p,
//                      r -= alpha q, Q1 = -x'(rhs + r), zeta, |r|, the three
//                      stopping tests
// and on a residual-reset iteration the update in two halves around the extra
// product tmp = S x (kCgUpdateX, then kCgUpdateReset).  Lane 0 of wave 0 runs
// the transitions of cg_state.hpp on the state in device memory with ordinary
// stores; the host never computes a scalar of the iteration.
//
// One workgroup of kCgThreads lanes per kernel, for every vector length: a
// reduction is per-lane strided sums, WaveSumLane0's butterfly, then the waves
// in wave order through LDS -- an order that depends on n alone, with no
// second launch shape and no combination across workgroups.  The vectors are
// short against the operator (n = 9 cameras; 1.2e5 entries at 13,682 cameras,
// where one product moves three orders of magnitude more bytes).
//
// Frozen after termination: every kernel returns at once when state->done is
// set, so iterations enqueued past the end leave x, r, p and the state as they
// were (the operator launches between them write z and tmp only).
//
// Contraction is off inside the kernels: x + alpha p is a product and a sum,
// as the reference's Axpby, so that only the reductions' order differs from a
// plain host restatement.
//
// Included by cg_kernels.hip alone, which is built without -ffinite-math-only:
// under that flag the compiler takes every sum for finite and folds the
// reference's tests for an infinite rho, beta, pq and alpha away.
#ifndef CSE_CG_KERNELS_HPP_
#define CSE_CG_KERNELS_HPP_

#include <hip/hip_runtime.h>

#include "cg_kernels.h"
#include "kernel_common.hpp"

namespace cse {

// The workgroup's sums of v[0..N), in every lane.
template <int N>
__device__ __forceinline__ void CgBlockSum(double (&v)[N], double (*lds)[kCgWaves]) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double w = WaveSumLane0(v[i]);
    if (lane == 0) lds[i][wave] = w;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kCgWaves; ++w) t += lds[i][w];
    v[i] = t;
  }
  __syncthreads();
}

// :125-136, and with zero_guess the rest of the preamble for x = 0: r = rhs,
// |r| = |b|, Q0 = 0, without the product.
__global__ __launch_bounds__(kCgThreads) void CgInitKernel(const CgArgs a, int zero_guess) {
#pragma clang fp contract(off)
  __shared__ double lds[1][kCgWaves];
  __shared__ int go;
  double acc[1] = {0.0};
  for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) acc[0] += a.rhs[k] * a.rhs[k];
  CgBlockSum<1>(acc, lds);
  const double norm_rhs = sqrt(acc[0]);
  if (threadIdx.x == 0) go = CgBegin(a.state, norm_rhs) ? 1 : 0;
  __syncthreads();
  if (!go) {
    for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) a.x[k] = 0.0;
    return;
  }
  if (!zero_guess) return;
  for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) {
    a.x[k] = 0.0;
    a.r[k] = a.rhs[k];
  }
  if (threadIdx.x == 0) CgInitialResidual(a.state, a.params, norm_rhs, 0.0);
}

// :143-159 after tmp = S x: r = rhs - tmp, |r|, Q0 = -x'(rhs + r).
__global__ __launch_bounds__(kCgThreads) void CgInitialResidualKernel(const CgArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[2][kCgWaves];
  if (a.state->done) return;
  double acc[2] = {0.0, 0.0};
  for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) {
    const double b = a.rhs[k];
    const double r = b - a.tmp[k];
    a.r[k] = r;
    acc[0] += a.x[k] * (b + r);
    acc[1] += r * r;
  }
  CgBlockSum<2>(acc, lds);
  if (threadIdx.x == 0) CgInitialResidual(a.state, a.params, sqrt(acc[1]), acc[0]);
}

// :162-190.
__global__ __launch_bounds__(kCgThreads) void CgDirectionKernel(const CgArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[1][kCgWaves];
  __shared__ double beta_s;
  __shared__ int go;  // 0: stop, 1: p = z, 2: p = z + beta p
  if (a.state->done) return;
  double acc[1] = {0.0};
  for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) {
    const double rk = a.r[k];
    double zk = rk;
    if (a.precond) {
      zk = 0.0;
      const int64_t j = k - a.pre_off;
      if (j >= 0 && j < a.pre_n) {
        const int64_t blk = j / 9;
        const int row = (int)(j - 9 * blk);
        const double* m = a.precond + 81 * blk + 9 * row;
        const double* rb = a.r + a.pre_off + 9 * blk;
#pragma unroll
        for (int c = 0; c < 9; ++c) zk += m[c] * rb[c];
      }
    }
    a.z[k] = zk;
    acc[0] += rk * zk;
  }
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

// :195-301 after q = S p (in z).  kCgUpdateX stops after x += alpha p, for the
// product tmp = S x of a reset iteration; kCgUpdateReset resumes there with
// r = rhs - tmp.
template <int kMode>
__global__ __launch_bounds__(kCgThreads) void CgUpdateKernel(const CgArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[2][kCgWaves];
  __shared__ double alpha_s;
  __shared__ int go;
  if (a.state->done) return;
  double alpha = 0.0;
  if constexpr (kMode != kCgUpdateReset) {
    double pq[1] = {0.0};
    for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) pq[0] += a.p[k] * a.z[k];
    CgBlockSum<1>(pq, lds);
    if (threadIdx.x == 0) {
      go = CgStep(a.state, pq[0]) ? 1 : 0;
      alpha_s = a.state->alpha;
    }
    __syncthreads();
    if (!go) return;
    alpha = alpha_s;
  }
  if constexpr (kMode == kCgUpdateX) {
    for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) a.x[k] = a.x[k] + alpha * a.p[k];
    return;
  }
  double acc[2] = {0.0, 0.0};
  for (int64_t k = threadIdx.x; k < a.n; k += kCgThreads) {
    const double b = a.rhs[k];
    double xk, rk;
    if constexpr (kMode == kCgUpdateFull) {
      xk = a.x[k] + alpha * a.p[k];
      rk = a.r[k] - alpha * a.z[k];
      a.x[k] = xk;
    } else {
      xk = a.x[k];
      rk = b - a.tmp[k];
    }
    a.r[k] = rk;
    acc[0] += xk * (b + rk);
    acc[1] += rk * rk;
  }
  CgBlockSum<2>(acc, lds);
  if (threadIdx.x == 0) CgTests(a.state, a.params, acc[0], acc[1]);
}

}  // namespace cse

#endif  // CSE_CG_KERNELS_HPP_
