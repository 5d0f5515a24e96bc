// launch_eval.hpp -- the launches of launch.hpp that name only the evaluation
// kernels (evaluate_kernel.hpp), for the TUs that instantiate those alone:
// operator_kernels.hpp defines plain (non-template) kernels, which only one TU
// of the library may hold.
#ifndef CSE_LAUNCH_EVAL_HPP_
#define CSE_LAUNCH_EVAL_HPP_

#include <hip/hip_runtime.h>

#include "evaluate_kernel.hpp"

namespace cse {

inline int64_t Chunks(int64_t n) { return (n + kWave - 1) / kWave; }

// The general kernel: one residual block per lane, offsets through the
// descriptor's tables (EvaluateTableKernel).
template <class K, int L, bool J>
void LaunchTableKernel(const GroupArgs& a, int64_t num_wg, hipStream_t s) {
  hipLaunchKernelGGL((EvaluateTableKernel<K, L, J>), dim3((unsigned)num_wg), dim3(kBlockThreads), 0, s,
                     a);
}

// The affine kernel: one 64-block chunk per wave, 4 waves per workgroup.
// kCoop 2: slot 0 by LDS-DMA from the repacked table; 1: 8-byte pieces from
// the state.
template <class K, int L, bool J, bool Crs, int kCoop, class T = ShippedTune>
void LaunchAffineChunks(const GroupArgs& a, int64_t num_wg, hipStream_t s) {
  hipLaunchKernelGGL((EvaluateAffineChunks<K, L, J, Crs, kCoop, T>), dim3((unsigned)num_wg),
                     dim3(kBlockThreads), 0, s, a);
}

// The residual+Jacobian evaluation of two-slot kinds with the LDS-DMA
// gather: two half-wave staging rounds, one wave per workgroup
// (BlockSparseMatrix: EvaluateAffineChunksTwoRoundW1; CompressedRow:
// EvaluateAffineChunksTwoRoundCrsW1).
template <class K, int L, int kCoop, class T = ShippedTune>
void LaunchTwoRoundW1(const GroupArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((EvaluateAffineChunksTwoRoundW1<K, L, kCoop, T>), dim3((unsigned)Chunks(a.n)),
                     dim3(kWave), 0, s, a);
}
template <class K, int L, int kCoop, class T = ShippedTune>
void LaunchTwoRoundCrsW1(const GroupArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((EvaluateAffineChunksTwoRoundCrsW1<K, L, kCoop, T>), dim3((unsigned)Chunks(a.n)),
                     dim3(kWave), 0, s, a);
}

// The affine evaluation of a (non-Snavely) kind: the kernel the library's
// Pick chooses for (layout, outputs, gather).
template <class K, int L, bool Crs, bool J, bool kDma>
void LaunchAffine(const GroupArgs& a, int64_t num_wg, hipStream_t s) {
  if constexpr (J && kDma && !Crs && kTwoRoundBsm<K>) {
    LaunchTwoRoundW1<K, L, 2>(a, s);
  } else if constexpr (J && kDma && Crs) {
    LaunchTwoRoundCrsW1<K, L, 2>(a, s);
  } else {
    LaunchAffineChunks<K, L, J, Crs, kDma ? 2 : 1>(a, num_wg, s);
  }
}

// The fused gradient (gradient_mode 0) of a two-slot kind whose slot 1 has
// 3 parameters, the form the library's Snavely kinds take: the Jacobian
// kernel that also sums the slot-1 rows of its sorted blocks
// (EvaluateAffineChunksFusedPointsW1, one wave per workgroup), and the
// slot-0 rows by re-evaluation in slot-0 order (CameraGradientKernel).
template <class K>
constexpr bool kFusedGradShape = KindTraits<K>::NB == 2 && KindTraits<K>::S1 == 3;

template <class K, int L, bool Crs>
void LaunchFusedPointsKernel(const GroupArgs& a, hipStream_t s) {
  hipLaunchKernelGGL((EvaluateAffineChunksFusedPointsW1<K, L, Crs>), dim3((unsigned)Chunks(a.n)), dim3(kWave),
                     0, s, a);
}

template <class K, int L>
void LaunchCameraGradient(const CamGradArgs& g, int64_t nslots, hipStream_t s) {
  constexpr int W = kWavesPerBlock;
  hipLaunchKernelGGL((CameraGradientKernel<K, L, W>), dim3((unsigned)((nslots + W - 1) / W)), dim3(W * kWave), 0,
                     s, g);
}

}  // namespace cse

#endif  // CSE_LAUNCH_EVAL_HPP_
