// per_block_loss_kernels.h -- launchers of the evaluation kernels with
// per-block loss parameters (cse_residual_group.loss_data_size == 2): the
// kernels of evaluate_kernel.hpp and group_store_kernel.hpp instantiated with
// the per-block loss kinds (loss.hpp, kLossPerBlock), picked by the same
// functions as their uniform twins (kernel_pickers.hpp).  They are
// instantiated in their own TU (per_block_loss_kernels.hip), compiled beside
// cse_evaluator.hip.  loss: the group's cse_loss_kind (Huber, Cauchy, or the
// scaled trivial loss).
#ifndef CSE_PER_BLOCK_LOSS_KERNELS_H_
#define CSE_PER_BLOCK_LOSS_KERNELS_H_

#include <hip/hip_runtime.h>

#include "evaluate_kernel.hpp"

namespace cse {

using PerBlockLaunchFn = void (*)(const GroupArgs&, int64_t num_wg, hipStream_t);

// As Pick and PickFused of cse_evaluator.hip, for a group whose blocks carry
// their own (a, scale): null where the uniform pickers return null.
PerBlockLaunchFn PerBlockPick(int kind, int loss, bool jac, int policy, bool dma, bool const0);
PerBlockLaunchFn PerBlockPickFused(int kind, int loss, int policy, bool points, bool const0);
// CameraGradientKernel (the Snavely camera, or kKindQuaternionTangent), one
// chunk per wave, kPerBlockCamGradWaves waves per workgroup.
constexpr int kPerBlockCamGradWaves = kWavesPerBlock;
void LaunchPerBlockCameraGradient(int kind, int loss, const CamGradArgs& g, hipStream_t s);

}  // namespace cse

#endif  // CSE_PER_BLOCK_LOSS_KERNELS_H_
