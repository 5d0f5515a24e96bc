// cg_kernels.hip -- cse_schur_solve's vector kernels (cg_kernels.hpp) and their
// launchers, built without -ffinite-math-only (cg_kernels.h says why).
#include "cg_kernels.h"

#include "cg_kernels.hpp"

namespace cse {

static_assert(kCgThreads == kCgWaves * kWave, "cg_kernels.h spells the wave size out");

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

}  // namespace cse
