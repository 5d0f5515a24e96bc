// cg_sliced_kernels.hpp -- the vector algebra of cse_cgnr_solve: the same
// ConjugateGradientsSolver (internal/ceres/conjugate_gradients_solver.h:108-305)
// and the same transitions (cg_state.hpp) as cg_kernels.hpp, for vectors of any
// length: num_effective_parameters entries, 13.5 million at problem-13682,
// where one workgroup per kernel is no longer a choice.
//
// The vector is cut into slices of kCgSliceEntries entries, one workgroup
// each; the slice count depends on n alone.  A reduction is: per-lane sums over
// the lane's kCgSliceEntries / kCgSliceThreads entries in index order,
// WaveSumLane0's butterfly, the waves in wave order through LDS -- the slice's
// partial -- and then the slice partials in a fixed order by the workgroup that
// finishes last (CgSliceHandOver), which also runs the transition on the state
// with ordinary stores.  The order depends on n alone, so repeats and every
// check_period give the same bits.
//
// The scalar of a reduction is known only when its grid ends, so each of
// cg_kernels.hpp's two kernels is two here:
//   direction-reduce  rho = r'z, CgDirection        (z = M^-1 r: CgnrApplyBlocksKernel
//   direction-apply   p = z, or p = z + beta p       before it; IDENTITY reads r)
//   step-reduce       pq = p'q, CgStep
//   update            x += alpha p, r -= alpha q, Q1, |r|, CgTests
// and on a residual-reset iteration the update's X half, the product tmp = A x,
// and its reset half.  The init kernels are split the same way.
//
// Every workgroup reads state->done (and alpha, beta) before it adds to the
// hand-over counter and only the last adder writes the state, so all
// workgroups of a grid see the same state.  A kernel returns at once when
// `done` is set: iterations enqueued past the end change nothing.
//
// Contraction is off, as in cg_kernels.hpp; included by cg_kernels.hip alone
// (no -ffinite-math-only: the tests for infinite scalars survive).
#ifndef CSE_CG_SLICED_KERNELS_HPP_
#define CSE_CG_SLICED_KERNELS_HPP_

#include <hip/hip_runtime.h>

#include "cg_kernels.h"
#include "kernel_common.hpp"

namespace cse {

// The slice's sums of v[0..N), in every lane.
template <int N>
__device__ __forceinline__ void CgSliceSum(double (&v)[N], double (*lds)[kCgSliceWaves]) {
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
    for (int w = 0; w < kCgSliceWaves; ++w) t += lds[i][w];
    v[i] = t;
  }
  __syncthreads();
}

__device__ __forceinline__ double CgLoadSc1(const double* p) {
  double v;
  asm volatile("global_load_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}

// Four loads in flight (a dependent wait per load is a round trip to L2 each:
// 6,588 slice partials at problem-13682, 26 per lane and sum).
__device__ __forceinline__ void CgLoadSc1x4(const double* p0, const double* p1, const double* p2,
                                            const double* p3, double (&v)[4]) {
  asm volatile(
      "global_load_dwordx2 %0, %4, off sc1\n\t"
      "global_load_dwordx2 %1, %5, off sc1\n\t"
      "global_load_dwordx2 %2, %6, off sc1\n\t"
      "global_load_dwordx2 %3, %7, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
      : "v"(p0), "v"(p1), "v"(p2), "v"(p3)
      : "memory");
}

// The grid's sums from the per-lane sums v.  Every workgroup reduces its slice
// and hands the partial(s) over; returns true in the workgroup that finished
// last, with the totals in v (every lane).  The hand-over is
// ReduceFinalizeKernel's (evaluation_kernels.hpp; MI355X visibility table, one
// lane per storing workgroup, one unsharded counter): lane 0 stores the
// partials write-through (sc1) and drains them (vmcnt(0)) before its
// agent-scope add; the workgroup whose add came last runs an agent-scope
// acquire after that add has returned, then a workgroup barrier, and only then
// reads the partials.  ReduceFinalizeKernel reads them with sc1 loads in the
// acquire's place, which the table covers at one workgroup per compute unit;
// these grids have up to thousands of workgroups, several resident per compute
// unit, so the acquire is kept here (the loads stay sc1; with the acquire plain
// loads would do as well).  The counter is left at 0 for the next launch.  Slice partial i of slice s is at
// partial[i * nslices + s]; the last workgroup adds them lane-strided in slice
// order, then as CgSliceSum.
template <int N>
__device__ __forceinline__ bool CgSliceHandOver(double (&v)[N], double* partial, int* counter,
                                                double (*lds)[kCgSliceWaves], int* last) {
#pragma clang fp contract(off)
  CgSliceSum<N>(v, lds);
  const int nslices = (int)gridDim.x;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double* dst = partial + (int64_t)i * nslices + blockIdx.x;
      asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(dst), "v"(v[i]) : "memory");
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int old = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *last = old == nslices - 1;
    if (old == nslices - 1) {
      // The consumer's agent-scope acquire (it invalidates this compute unit's
      // L1, where every wave of this workgroup runs), complete before the
      // barrier lets the other waves load.  Once per kernel, in one workgroup.
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!*last) return false;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double* src = partial + (int64_t)i * nslices;
    double t = 0.0;
    int s = threadIdx.x;
    for (; s + 3 * kCgSliceThreads < nslices; s += 4 * kCgSliceThreads) {
      double x[4];
      CgLoadSc1x4(src + s, src + s + kCgSliceThreads, src + s + 2 * kCgSliceThreads,
                  src + s + 3 * kCgSliceThreads, x);
      t += x[0];
      t += x[1];
      t += x[2];
      t += x[3];
    }
    for (; s < nslices; s += kCgSliceThreads) t += CgLoadSc1(src + s);
    v[i] = t;
  }
  CgSliceSum<N>(v, lds);
  if (threadIdx.x == 0) *counter = 0;
  return true;
}

// The lane's entries of its slice: k = slice base + lane + u kCgSliceThreads.
#define CSE_CG_SLICE_LOOP(k, a)                                                              \
  for (int64_t k = (int64_t)blockIdx.x * kCgSliceEntries + threadIdx.x,                      \
               k##_end = ((int64_t)blockIdx.x + 1) * kCgSliceEntries < (a).n                 \
                             ? ((int64_t)blockIdx.x + 1) * kCgSliceEntries                   \
                             : (a).n;                                                        \
       k < k##_end; k += kCgSliceThreads)

// :125-136: |rhs|, CgBegin; with zero_guess the rest of the preamble for x = 0
// too (|r| = |b|, Q0 = 0, no product).  The vectors follow in
// CgSlicedInitApplyKernel.  Reads no `done`: it is the previous solve's.
__global__ __launch_bounds__(kCgSliceThreads) void CgSlicedInitKernel(const CgSlicedArgs a, int zero_guess) {
#pragma clang fp contract(off)
  __shared__ double lds[1][kCgSliceWaves];
  __shared__ int last;
  double acc[1] = {0.0};
  CSE_CG_SLICE_LOOP(k, a) acc[0] += a.rhs[k] * a.rhs[k];
  if (!CgSliceHandOver<1>(acc, a.partial, a.counter, lds, &last)) return;
  if (threadIdx.x == 0) {
    const double norm_rhs = sqrt(acc[0]);
    if (CgBegin(a.state, norm_rhs) && zero_guess) CgInitialResidual(a.state, a.params, norm_rhs, 0.0);
  }
}

// x = 0 when the solve starts there or |b| = 0 ended it; r = rhs from a zero start.
__global__ __launch_bounds__(kCgSliceThreads) void CgSlicedInitApplyKernel(const CgSlicedArgs a, int zero_guess) {
  const bool zero = zero_guess || (a.state->done && a.state->reason == kCgZeroRhs);
  CSE_CG_SLICE_LOOP(k, a) {
    if (zero) a.x[k] = 0.0;
    if (zero_guess) a.r[k] = a.rhs[k];
  }
}

// :143-159 after tmp = A x: r = rhs - tmp, |r|, Q0 = -x'(rhs + r).
__global__ __launch_bounds__(kCgSliceThreads) void CgSlicedInitialResidualKernel(const CgSlicedArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[2][kCgSliceWaves];
  __shared__ int last;
  if (a.state->done) return;
  double acc[2] = {0.0, 0.0};
  CSE_CG_SLICE_LOOP(k, a) {
    const double b = a.rhs[k];
    const double r = b - a.tmp[k];
    a.r[k] = r;
    acc[0] += a.x[k] * (b + r);
    acc[1] += r * r;
  }
  if (!CgSliceHandOver<2>(acc, a.partial, a.counter, lds, &last)) return;
  if (threadIdx.x == 0) CgInitialResidual(a.state, a.params, sqrt(acc[1]), acc[0]);
}

// :162-172: rho = r'z and its tests (a.zr: z, or r under IDENTITY).
__global__ __launch_bounds__(kCgSliceThreads) void CgSlicedDirectionReduceKernel(const CgSlicedArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[1][kCgSliceWaves];
  __shared__ int last;
  if (a.state->done) return;
  double acc[1] = {0.0};
  CSE_CG_SLICE_LOOP(k, a) acc[0] += a.r[k] * a.zr[k];
  if (!CgSliceHandOver<1>(acc, a.partial, a.counter, lds, &last)) return;
  if (threadIdx.x == 0) CgDirection(a.state, acc[0]);
}

// :174-190: p = z in iteration 1, p = z + beta p after it.
__global__ __launch_bounds__(kCgSliceThreads) void CgSlicedDirectionApplyKernel(const CgSlicedArgs a) {
#pragma clang fp contract(off)
  if (a.state->done) return;
  if (a.state->iteration == 1) {
    CSE_CG_SLICE_LOOP(k, a) a.p[k] = a.zr[k];
  } else {
    const double beta = a.state->beta;
    CSE_CG_SLICE_LOOP(k, a) a.p[k] = a.zr[k] + beta * a.p[k];
  }
}

// :195-216 after q = A p (in z): pq = p'q, alpha and their tests.
__global__ __launch_bounds__(kCgSliceThreads) void CgSlicedStepReduceKernel(const CgSlicedArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[1][kCgSliceWaves];
  __shared__ int last;
  if (a.state->done) return;
  double acc[1] = {0.0};
  CSE_CG_SLICE_LOOP(k, a) acc[0] += a.p[k] * a.z[k];
  if (!CgSliceHandOver<1>(acc, a.partial, a.counter, lds, &last)) return;
  if (threadIdx.x == 0) CgStep(a.state, acc[0]);
}

// :218-301.  kCgUpdateFull: x += alpha p, r -= alpha q, then Q1, |r| and the
// stopping tests; kCgUpdateX: x += alpha p alone, for the product tmp = A x of
// a reset iteration; kCgUpdateReset: r = rhs - tmp and the tests.
template <int kMode>
__global__ __launch_bounds__(kCgSliceThreads) void CgSlicedUpdateKernel(const CgSlicedArgs a) {
#pragma clang fp contract(off)
  __shared__ double lds[2][kCgSliceWaves];
  __shared__ int last;
  if (a.state->done) return;
  const double alpha = a.state->alpha;
  if constexpr (kMode == kCgUpdateX) {
    CSE_CG_SLICE_LOOP(k, a) a.x[k] = a.x[k] + alpha * a.p[k];
    return;
  }
  double acc[2] = {0.0, 0.0};
  CSE_CG_SLICE_LOOP(k, a) {
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
  if (!CgSliceHandOver<2>(acc, a.partial, a.counter, lds, &last)) return;
  if (threadIdx.x == 0) CgTests(a.state, a.params, acc[0], acc[1]);
}

#undef CSE_CG_SLICE_LOOP

// y = M x (kAssign) or y += M x over the block table of cse_cgnr_init: one
// parameter block per lane, its row-major tangent_size x tangent_size block at
// value_offset (CudaJacobiPreconditioner::RightMultiplyAndAccumulate,
// cgnr_solver.cc:272-274).  state: null, or the solve's (frozen when done).
template <bool kAssign>
__global__ __launch_bounds__(kBlockThreads) void CgnrApplyBlocksKernel(const CgnrBlock* tab, int64_t ntab,
                                                                       const double* values, const double* x,
                                                                       double* y, const CgState* state) {
#pragma clang fp contract(off)
  if (state && state->done) return;
  const int64_t i = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= ntab) return;
  const CgnrBlock blk = tab[i];
  const int S = blk.tangent_size;
  const double* m = values + blk.value_offset;
  const double* xb = x + blk.delta_offset;
  double* yb = y + blk.delta_offset;
  for (int r = 0; r < S; ++r) {
    double s = 0.0;
    for (int c = 0; c < S; ++c) s += m[r * S + c] * xb[c];
    yb[r] = kAssign ? s : yb[r] + s;
  }
}

}  // namespace cse

#endif  // CSE_CG_SLICED_KERNELS_HPP_
