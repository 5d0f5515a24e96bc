// evaluation_kernels.hpp -- the plain (non-template) kernels around one
// evaluation: Program::Plus, the held-camera sector fix-up, the cost reduction
// and the slot-0 repack.  cse_evaluator.hip owns them: it is the one TU of the
// library that includes this header (a plain kernel included by two TUs is
// defined twice at link time).
#ifndef CSE_EVALUATION_KERNELS_HPP_
#define CSE_EVALUATION_KERNELS_HPP_

#include "kernel_common.hpp"

namespace cse {

// Program::Plus for manifold-free blocks: runs of consecutive state entries
// whose delta offset is a constant shift away (PlusRun, host_shared.hpp).
__global__ __launch_bounds__(kBlockThreads) void PlusKernel(const double* x, const double* delta,
                                                            double* out, const PlusRun* runs,
                                                            int num_runs) {
  for (int r = 0; r < num_runs; ++r) {
    const PlusRun run = runs[r];
    for (int64_t t = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x; t < run.length;
         t += (int64_t)gridDim.x * kBlockThreads) {
      const int64_t i = run.state_begin + t;
      out[i] = x[i] + delta[i - run.delta_shift];
    }
  }
}

// Program::Plus of the CSE_MANIFOLD_QUATERNION_EUCLIDEAN blocks, one block
// per thread: ProductManifold<QuaternionManifold, EuclideanManifold<n>>::Plus,
// i.e. QuaternionPlusImpl (internal/ceres/manifold.cc:28-59: the quaternion
// exp(delta) on the left of x, x unchanged when |delta| is zero) and x + delta
// for the Euclidean tail (QuatPlusBlock, host_shared.hpp).
__global__ __launch_bounds__(kBlockThreads) void QuaternionPlusKernel(const double* x,
                                                                      const double* delta,
                                                                      double* out,
                                                                      const QuatPlusBlock* blocks,
                                                                      int64_t n) {
  const int64_t b = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (b >= n) return;
  const QuatPlusBlock B = blocks[b];
  const double* q = x + B.state_offset;
  const double* d = delta + B.delta_offset;
  double* o = out + B.state_offset;
  // |delta| as std::hypot(d0, d1, d2) (manifold.cc:33), in libstdc++'s
  // scaled form: no underflow for tiny steps (|d| < 1e-154 would square to
  // zero and be skipped), no overflow for huge ones; zero exactly when the
  // three components are (the FP_ZERO test, :35).
  const double a0 = fabs(d[0]), a1 = fabs(d[1]), a2 = fabs(d[2]);
  const double m = fmax(a0, fmax(a1, a2));
  if (m == 0.0) {
    o[0] = q[0];
    o[1] = q[1];
    o[2] = q[2];
    o[3] = q[3];
  } else {
    double nd;
    {
#pragma clang fp contract(off)
      const double r0 = a0 / m, r1 = a1 / m, r2 = a2 / m;
      nd = m * sqrt(r0 * r0 + r1 * r1 + r2 * r2);
    }
    double sn, cs;
    sincos(nd, &sn, &cs);
    const double sbd = sn / nd;
    const double w = cs, a = sbd * d[0], bq = sbd * d[1], c = sbd * d[2];
    o[0] = w * q[0] - a * q[1] - bq * q[2] - c * q[3];
    o[1] = w * q[1] + a * q[0] + bq * q[3] - c * q[2];
    o[2] = w * q[2] - a * q[3] + bq * q[0] + c * q[1];
    o[3] = w * q[3] + a * q[2] - bq * q[1] + c * q[0];
  }
  for (int k = 4; k < B.size; ++k) o[k] = q[k] + d[k - 1];
}

// Held-camera groups (Tune::kConst0 Jacobian kernels): after a held block
// the packed F cells (BSM) or row blocks (CRS) of a chunk start inside a
// 64-byte sector.  Each full chunk stored only the whole sectors of its
// segment and put its head pieces (slots 0-3: at their positions in the
// sector before its first whole one) and its tail pieces (slots 4-7: at their
// positions in the sector after its last) into side[16 c ..]; here thread
// 4 c + pos assembles position pos of the sector chunk c shares with the
// previous chunk that has a segment (prev[c]): the tail of that chunk, then
// the head of c, each only if that chunk was full (c < nfull; a ragged last
// chunk writes its whole segment itself), so each such sector is written as
// one 64-byte piece instead of two partial writes.  The group's first
// segment wrote its head itself.
__global__ __launch_bounds__(kBlockThreads) void HeldSectorFixupKernel(double* jac, const int64_t* fbase,
                                                                       const double* side,
                                                                       const int32_t* prev,
                                                                       int64_t nchunks, int64_t nfull) {
  const int64_t t = (int64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  const int64_t c = t >> 2;
  const int pos = (int)(t & 3);
  if (c >= nchunks || c == 0) return;
  const int64_t f0 = fbase[c];
  if (fbase[c + 1] == f0 || f0 == fbase[0]) return;  // no segment, or the first one
  const uintptr_t A0 = reinterpret_cast<uintptr_t>(jac + f0);
  const int hp = (int)(((64 - (A0 & 63)) & 63) >> 4);  // head pieces of c
  if (hp == 0) return;                                    // starts on a sector
  const int64_t pc = prev[c];
  const double* src = nullptr;
  if (pos < 4 - hp) {
    if (pc >= 0 && pc < nfull) src = side + 16 * pc + 8 + 2 * pos;
  } else if (c < nfull) {
    src = side + 16 * c + 2 * pos;
  }
  if (src) {
    double* S = reinterpret_cast<double*>(A0 & ~(uintptr_t)63);
    *reinterpret_cast<double2*>(S + 2 * pos) = *reinterpret_cast<const double2*>(src);
  }
}

// Sums the per-workgroup partials of every group in a fixed order, writes
// the cost, publishes the evaluation status and re-arms the status word
// for the next evaluation (replaces thrust::reduce + the abort-flag round
// trip, autodiff_residual_block_cuda_evaluator.h:241-265).
__global__ __launch_bounds__(1024) void FinalizeKernel(const double* partials, int64_t n,
                                                       double* cost, int* status,
                                                       int* status_out) {
  __shared__ double wsum[1024 / kWave];
  // Four independent accumulators per thread keep several loads in flight.
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  const int64_t step = blockDim.x;
  int64_t k = threadIdx.x;
  for (; k + 3 * step < n; k += 4 * step) {
    v0 += partials[k];
    v1 += partials[k + step];
    v2 += partials[k + 2 * step];
    v3 += partials[k + 3 * step];
  }
  for (; k < n; k += step) v0 += partials[k];
  double v = (v0 + v1) + (v2 + v3);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x / kWave); ++w) t += wsum[w];
    const int s = *status;
    *cost = s ? 0.0 : t;
    *status_out = s;
    *status = 0;
  }
}

// Many partials, one launch: workgroup b sums partials [b*per, (b+1)*per)
// in a fixed order and hands its sum over to
// whichever workgroup finishes last, which adds the G slice sums in slice
// order and finalises as FinalizeKernel does -- the same value, bit for bit,
// as a slice pass followed by FinalizeKernel over the 128 slice sums.  Hand-over (MI355X_MICROARCH.md, valid
// forms: one lane per storing workgroup, agent-scope atomic add, the last
// adder told by the returned value): the slice sum is stored write-through
// (sc1) and drained (vmcnt(0)) before the add; the last workgroup reads the
// sums with sc1 loads only after its add has returned.  The counter is left
// at 0 for the next launch.
__global__ __launch_bounds__(kBlockThreads) void ReduceFinalizeKernel(
    const double* partials, int64_t n, int64_t per, double* slices, int* counter, double* cost,
    int* status, int* status_out) {
  __shared__ double lds_sum[kWavesPerBlock];
  __shared__ int last;
  const int64_t begin = (int64_t)blockIdx.x * per;
  const int64_t end = begin + per < n ? begin + per : n;
  // The slice's values in the same order as one load per step, but eight
  // loads in flight at a time (a dependent load per add cost ~0.5 us each:
  // 7 us for the 14 per thread of problem-13682's 452,931 partials).
  double v = 0.0;
  int64_t k = begin + threadIdx.x;
  for (; k + 7 * kBlockThreads < end; k += 8 * kBlockThreads) {
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = partials[k + u * kBlockThreads];
#pragma unroll
    for (int u = 0; u < 8; ++u) v += x[u];
  }
  for (; k < end; k += kBlockThreads) v += partials[k];
  const double t = WorkgroupSum(v, lds_sum);
  if (threadIdx.x == 0) {
    double* dst = slices + blockIdx.x;
    asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" ::"v"(dst), "v"(t)
                 : "memory");
    const int old = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = old == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  double s = 0.0;
  if (threadIdx.x < gridDim.x) {
    const double* src = slices + threadIdx.x;
    asm volatile("global_load_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(s) : "v"(src)
                 : "memory");
  }
  __syncthreads();  // lds_sum is reused
  const double total = WorkgroupSum(s, lds_sum);
  if (threadIdx.x == 0) {
    const int st = *status;
    *cost = st ? 0.0 : total;
    *status_out = st;
    *status = 0;
    *counter = 0;
  }
}

// Copies slot-0 parameter blocks [lo, lo + count) of the state into the
// packed table (once per evaluation: 13,682 cameras = 1.1 MB for BAL
// problem-13682), one 16-byte piece per thread: the first `pieces` pieces of
// each row of `stride` doubles (the LDS-DMA gather reads no others).
// With src_off (groups with constant slot-0 blocks): row b comes from
// state + src_off[b] (active) or cstate + (-1 - src_off[b]) (constant).
__global__ __launch_bounds__(256) void RepackSlot0Kernel(const double* state, int64_t state_base,
                                                         int size, int stride, int pieces, int32_t lo,
                                                         int64_t count, double* packed,
                                                         const int64_t* src_off, const double* cstate) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t b = t / pieces;
  const int k = 2 * (int)(t - b * pieces);
  if (b >= count) return;
  const double* src;
  if (src_off) {
    const int64_t o = src_off[b];
    src = o >= 0 ? state + o : cstate + (-1 - o);
  } else {
    src = state + state_base + (int64_t)size * (lo + b);
  }
  const double x = src[k];
  // The padding double of an odd-sized row marks a constant block (1.0):
  // the constant-aware kernels read it with the row (AffineInputs::x0pad).
  const double y = k + 1 < size ? src[k + 1] : (src_off && src_off[b] < 0 ? 1.0 : 0.0);
  *reinterpret_cast<double2*>(packed + (int64_t)stride * b + k) = make_double2(x, y);
}

}  // namespace cse

#endif  // CSE_EVALUATION_KERNELS_HPP_
