// cg_kernels.hip -- cse_schur_solve's vector kernels (cg_kernels.hpp),
// cse_schur_power_series' (spse_kernels.hpp), cse_cgnr_solve's
// (cg_sliced_kernels.hpp) and their launchers, built without
// -ffinite-math-only (cg_kernels.h says why).
#include "cg_kernels.h"

#include "cg_kernels.hpp"
#include "cg_sliced_kernels.hpp"
#include "spse_kernels.hpp"

namespace cse {

static_assert(kCgThreads == kCgWaves * kWave, "cg_kernels.h spells the wave size out");
static_assert(kCgSliceThreads == kCgSliceWaves * kWave, "cg_kernels.h spells the wave size out");
static_assert(kCgSliceEntries % kCgSliceThreads == 0, "every lane takes the same number of entries");

void LaunchCgInit(const CgArgs& a, bool zero_guess, hipStream_t s) {
  hipLaunchKernelGGL(CgInitKernel, dim3(1), dim3(kCgThreads), 0, s, a, zero_guess ? 1 : 0);
}

void LaunchCgInitialResidual(const CgArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(CgInitialResidualKernel, dim3(1), dim3(kCgThreads), 0, s, a);
}

void LaunchCgDirection(const CgArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(CgDirectionKernel, dim3(1), dim3(kCgThreads), 0, s, a);
}

void LaunchCgUpdate(CgUpdateMode mode, const CgArgs& a, hipStream_t s) {
  switch (mode) {
    case kCgUpdateFull: hipLaunchKernelGGL((CgUpdateKernel<kCgUpdateFull>), dim3(1), dim3(kCgThreads), 0, s, a); break;
    case kCgUpdateX: hipLaunchKernelGGL((CgUpdateKernel<kCgUpdateX>), dim3(1), dim3(kCgThreads), 0, s, a); break;
    case kCgUpdateReset: hipLaunchKernelGGL((CgUpdateKernel<kCgUpdateReset>), dim3(1), dim3(kCgThreads), 0, s, a); break;
  }
}

void LaunchSpseZero(const SpseArgs& a, bool accumulate, hipStream_t s) {
  if (accumulate)
    hipLaunchKernelGGL(SpseZeroKernel<true>, dim3(1), dim3(kCgThreads), 0, s, a);
  else
    hipLaunchKernelGGL(SpseZeroKernel<false>, dim3(1), dim3(kCgThreads), 0, s, a);
}

void LaunchSpseTerm(const SpseArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(SpseTermKernel, dim3(1), dim3(kCgThreads), 0, s, a);
}

void LaunchCgDirectionGiven(const CgArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(CgDirectionGivenKernel, dim3(1), dim3(kCgThreads), 0, s, a);
}

// One workgroup per slice.
#define CSE_CG_SLICED(kernel, a, s, ...) \
  hipLaunchKernelGGL(kernel, dim3((unsigned)CgSliceCount((a).n)), dim3(kCgSliceThreads), 0, s, a, ##__VA_ARGS__)

void LaunchCgSlicedInit(const CgSlicedArgs& a, bool zero_guess, hipStream_t s) {
  CSE_CG_SLICED(CgSlicedInitKernel, a, s, zero_guess ? 1 : 0);
  CSE_CG_SLICED(CgSlicedInitApplyKernel, a, s, zero_guess ? 1 : 0);
}

void LaunchCgSlicedInitialResidual(const CgSlicedArgs& a, hipStream_t s) {
  CSE_CG_SLICED(CgSlicedInitialResidualKernel, a, s);
}

void LaunchCgSlicedDirection(const CgSlicedArgs& a, hipStream_t s) {
  if (a.tab) LaunchCgnrApplyBlocks(a.tab, a.ntab, a.precond, a.r, a.z, true, a.state, s);
  CSE_CG_SLICED(CgSlicedDirectionReduceKernel, a, s);
  CSE_CG_SLICED(CgSlicedDirectionApplyKernel, a, s);
}

void LaunchCgSlicedUpdate(CgUpdateMode mode, const CgSlicedArgs& a, hipStream_t s) {
  switch (mode) {
    case kCgUpdateFull:
      CSE_CG_SLICED(CgSlicedStepReduceKernel, a, s);
      CSE_CG_SLICED(CgSlicedUpdateKernel<kCgUpdateFull>, a, s);
      break;
    case kCgUpdateX:
      CSE_CG_SLICED(CgSlicedStepReduceKernel, a, s);
      CSE_CG_SLICED(CgSlicedUpdateKernel<kCgUpdateX>, a, s);
      break;
    case kCgUpdateReset: CSE_CG_SLICED(CgSlicedUpdateKernel<kCgUpdateReset>, a, s); break;
  }
}

#undef CSE_CG_SLICED

void LaunchCgnrApplyBlocks(const CgnrBlock* tab, int64_t ntab, const double* values, const double* x,
                           double* y, bool assign, const CgState* state, hipStream_t s) {
  if (ntab <= 0) return;
  const dim3 grid((unsigned)((ntab + kBlockThreads - 1) / kBlockThreads));
  if (assign)
    hipLaunchKernelGGL(CgnrApplyBlocksKernel<true>, grid, dim3(kBlockThreads), 0, s, tab, ntab, values, x, y, state);
  else
    hipLaunchKernelGGL(CgnrApplyBlocksKernel<false>, grid, dim3(kBlockThreads), 0, s, tab, ntab, values, x, y, state);
}

}  // namespace cse
