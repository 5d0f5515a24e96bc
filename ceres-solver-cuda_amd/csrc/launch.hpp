// launch.hpp -- host-side launches of the evaluator kernels for one functor
// kind, in their shipped settings (grid, workgroup size, tuning struct).
//
// Shared by the library (cse_evaluator.hip) and by user functor kinds, whose
// kernels are instantiated in the user's hipcc TU
// (include/ceres_amd/autodiff_cuda.h) the way the reference instantiates
// EvaluateKernel<CostFunctor, LossFunctionCUDA, kR, Ns...> in the user's nvcc
// TU (include/ceres/internal/autodiff_residual_block_cuda_evaluator.h:
// 183-271, cuda_evaluator_kernel.h:297-422).  Every function here launches
// exactly the kernel the library launches for the same (kind, loss, layout,
// outputs); the Snavely camera's specialised kernels (group store, fused
// gradient, held cameras) are chosen in cse_evaluator.hip and never reach
// these.  The launches of the evaluation kernels themselves are in
// launch_eval.hpp (TUs that instantiate only those include it alone).
#ifndef CSE_LAUNCH_HPP_
#define CSE_LAUNCH_HPP_

#include <hip/hip_runtime.h>

#include "launch_eval.hpp"
#include "operator_kernels.hpp"

namespace cse {

// J x (affine or table) and J^T x (table; affine groups use the gradient
// post-pass for it).  which: 0 = J x affine, 1 = J x table, 2 = J^T x table.
template <class K>
void LaunchMultiplyKernel(const GroupArgs& a, int which, const double* x, double* y, hipStream_t s) {
  const dim3 grid((unsigned)((a.n + kBlockThreads - 1) / kBlockThreads));
  if constexpr (KindTraits<K>::NB <= 2) {
    if (which == 0) {
      hipLaunchKernelGGL(RightMultiplyAffineKernel<K>, grid, dim3(kBlockThreads), 0, s, a, x, y);
      return;
    }
  }
  if (which == 2)
    hipLaunchKernelGGL((MultiplyTableKernel<K, true>), grid, dim3(kBlockThreads), 0, s, a, x, y);
  else
    hipLaunchKernelGGL((MultiplyTableKernel<K, false>), grid, dim3(kBlockThreads), 0, s, a, x, y);
}

// The gradient post-pass over one slot (GradArgs; NR residuals, S columns):
// form 0 = identity order, contiguous block ranges (points); 1 = chunks of
// at most kGradChunk blocks, one wave each, then the ordered chunk reduce
// (cameras); 2 = one lane per parameter block.
enum GradForm { kGradRange = 0, kGradChunked = 1, kGradPerBlock = 2 };
template <int NR, int S>
void LaunchGradientSlot(const GradArgs& ga, const GradChunks& ch, int form, hipStream_t s) {
  if (form == kGradRange) {
    hipLaunchKernelGGL((GradientRangeKernel<NR, S>), dim3((unsigned)((ga.count + kWave - 1) / kWave)),
                       dim3(kWave), 0, s, ga);
  } else if (form == kGradChunked) {
    const dim3 grid((unsigned)((ch.nchunks + kWavesPerBlock - 1) / kWavesPerBlock));
    if (ch.nchunks > 0)
      hipLaunchKernelGGL((GradientLanesKernel<NR, S>), grid, dim3(kBlockThreads), 0, s, ga, ch);
    hipLaunchKernelGGL((GradientChunkReduceKernel<S>),
                       dim3((unsigned)((ga.count + kBlockThreads - 1) / kBlockThreads)),
                       dim3(kBlockThreads), 0, s, ga, ch);
  } else {
    hipLaunchKernelGGL((GradientSlotKernel<NR, S, false>),
                       dim3((unsigned)((ga.count + kBlockThreads - 1) / kBlockThreads)),
                       dim3(kBlockThreads), 0, s, ga);
  }
}

}  // namespace cse

#endif  // CSE_LAUNCH_HPP_
