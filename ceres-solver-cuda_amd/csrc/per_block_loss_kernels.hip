// per_block_loss_kernels.hip -- the evaluation kernels of groups with
// per-block loss parameters: every kernel family the pickers can hand a
// uniform group of a library kind (group store, two-round BSM and CRS, the
// chunk kernels, fused and fused-points, the held-camera forms, the table
// kernel, CameraGradientKernel), instantiated with the per-block loss kinds.
// Same kernels, same store tails, same settings as cse_evaluator.hip's; only
// where the loss parameters come from differs (BlockLoss, kernel_common.hpp).
// One TU of its own so both compile in parallel.
#include "per_block_loss_kernels.h"

#include "kernel_pickers.hpp"

namespace cse {

PerBlockLaunchFn PerBlockPick(int kind, int loss, bool jac, int policy, bool dma, bool const0) {
  return Pick<PerBlockLosses>(kind, loss, jac, policy, dma, const0);
}

PerBlockLaunchFn PerBlockPickFused(int kind, int loss, int policy, bool points, bool const0) {
  return PickFused<PerBlockLosses>(kind, loss, policy, points, const0);
}

void LaunchPerBlockCameraGradient(int kind, int loss, const CamGradArgs& g, hipStream_t s) {
  LaunchCameraGradientOf<PerBlockLosses, kPerBlockCamGradWaves>(kind, loss, g, s);
}

}  // namespace cse
