// kernel_pickers.hpp -- which evaluation kernel a residual group launches:
// the library's functor kinds (VisitKind), the kernels' loss template argument
// (UniformLosses, PerBlockLosses) and the pickers from (kind, loss, outputs,
// layout policy, gather) to a launch function.  Host code, templates only:
// cse_evaluator.hip instantiates the pickers with UniformLosses and
// per_block_loss_kernels.hip with PerBlockLosses, each TU compiling the
// kernels its pickers name; linear_operators.hip takes VisitKind alone.
#ifndef CSE_KERNEL_PICKERS_HPP_
#define CSE_KERNEL_PICKERS_HPP_

#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "../../include/cse.h"
#include "group_store_kernel.hpp"
#include "launch.hpp"
#include "plan.hpp"

namespace cse {

using LaunchFn = void (*)(const GroupArgs&, int64_t num_wg, hipStream_t);

// The functor kinds the library is built for.  Visit(kind, f) calls
// f(K{}) with the kind's functor type; returns false for an unknown kind.
using TestLinear3_234 = LinearTestKind<3, 2, 3, 4>;
using TestLinear3_432 = LinearTestKind<3, 4, 3, 2>;
using TestLinear2_23 = LinearTestKind<2, 2, 3>;
using TestLinear3_24 = LinearTestKind<3, 2, 4>;
using TestLinear4_34 = LinearTestKind<4, 3, 4>;

// (kKindQuaternionTangent, plan.hpp: the internal kernel kind of a group
// whose slot-0 blocks are on CSE_MANIFOLD_QUATERNION_EUCLIDEAN.)
template <class F>
bool VisitKind(int kind, F&& f) {
  switch (kind) {
    case kKindQuaternionTangent: f(SnavelyQuaternionTangentKind{}); return true;
    case CSE_FUNCTOR_SNAVELY_2_9_3: f(SnavelyKind{}); return true;
    case CSE_FUNCTOR_SNAVELY_NO_DISTORTION_2_7_3: f(SnavelyNoDistortionKind{}); return true;
    case CSE_FUNCTOR_SNAVELY_QUATERNION_2_10_3: f(SnavelyQuaternionKind{}); return true;
    case CSE_FUNCTOR_POINT_DISPLACEMENT_3_3: f(PointDisplacementKind{}); return true;
    case CSE_FUNCTOR_TEST_LINEAR_3_2_3_4: f(TestLinear3_234{}); return true;
    case CSE_FUNCTOR_TEST_LINEAR_3_4_3_2: f(TestLinear3_432{}); return true;
    case CSE_FUNCTOR_TEST_LINEAR_2_2_3: f(TestLinear2_23{}); return true;
    case CSE_FUNCTOR_TEST_LINEAR_3_2_4: f(TestLinear3_24{}); return true;
    case CSE_FUNCTOR_TEST_LINEAR_4_3_4: f(TestLinear4_34{}); return true;
    case CSE_FUNCTOR_TEST_BILINEAR_1_2_2: f(BilinearTestKind{}); return true;
    case CSE_FUNCTOR_TEST_TEN_PARAMETER_1_x10: f(TenParameterTestKind{}); return true;
    case CSE_FUNCTOR_TEST_PARTIAL_OUTPUT_2_1: f(PartialOutputTestKind{}); return true;
    default: return false;
  }
}

template <class K, int L, bool J>
void LaunchTable(const GroupArgs& a, int64_t num_wg, hipStream_t s) {
  LaunchTableKernel<K, L, J>(a, num_wg, s);
}

// The affine kernel: one 64-block chunk per wave, 4 waves per workgroup
// (the residual-only and cost-only evaluations; one wave per workgroup
// measured 1 % slower for them, profiles/round3/w1).
template <class K, int L, bool J, bool Crs, int Co, class T = ShippedTune>
void LaunchChunks(const GroupArgs& a, int64_t num_wg, hipStream_t s) {
  LaunchAffineChunks<K, L, J, Crs, Co, T>(a, num_wg, s);
}

// The BSM residual+Jacobian evaluation of two-slot kinds: one wave per
// workgroup (EvaluateAffineChunksTwoRoundW1); the Snavely camera's, when
// its outputs sit on 64-byte sectors, four-wave workgroups storing long
// runs (EvaluateAffineChunksGroupStore, group_store_kernel.hpp).
template <class K, class T>
constexpr bool kGroupStore = std::is_same<K, SnavelyKind>::value &&
                             std::is_same<T, ShippedTune>::value;

template <class K, int L, int Co, class T = ShippedTune>
void LaunchTwoRound(const GroupArgs& a, int64_t num_wg, hipStream_t s) {
  (void)num_wg;
  if constexpr (kGroupStore<K, T> && Co == 2) {
    if (GroupStoreEligible(a)) {
      const int64_t chunks = Chunks(a.n);
      hipLaunchKernelGGL((EvaluateAffineChunksGroupStore<K, L>),
                         dim3((unsigned)((chunks + kQuadWaves - 1) / kQuadWaves)),
                         dim3(kQuadWaves * kWave), 0, s, a);
      return;
    }
  }
  LaunchTwoRoundW1<K, L, Co, T>(a, s);
}

// The CRS residual+Jacobian evaluation: one wave per workgroup.
template <class K, int L, int Co, class T = ShippedTune>
void LaunchTwoRoundCrs(const GroupArgs& a, int64_t num_wg, hipStream_t s) {
  (void)num_wg;
  LaunchTwoRoundCrsW1<K, L, Co, T>(a, s);
}

// The affine kernel with the fused gradient (Snavely groups): with the
// slot-0 contributions (gradient_mode 3) or points only (gradient_mode 0,
// slot 0 from CameraGradientKernel; one wave per workgroup).
template <class K, int L, bool Crs, class T = ShippedTune>
void LaunchFused(const GroupArgs& a, int64_t num_wg, hipStream_t s) {
  hipLaunchKernelGGL((EvaluateAffineChunksFused<K, L, Crs, T>), dim3((unsigned)num_wg),
                     dim3(kBlockThreads), 0, s, a);
}
template <class K, int L, bool Crs, class T = PointsOnlyTune>
void LaunchFusedPoints(const GroupArgs& a, int64_t num_wg, hipStream_t s) {
  (void)num_wg;
  hipLaunchKernelGGL((EvaluateAffineChunksFusedPointsW1<K, L, Crs, T>), dim3((unsigned)Chunks(a.n)),
                     dim3(kWave), 0, s, a);
}

// f(std::integral_constant<int, s0>) for the slot-0 sizes the fused
// gradient's tail is built for (1..16, the affine kernels' bound).
template <class F>
bool VisitSlot0Size(int s0, F&& f) {
  switch (s0) {
#define CSE_S0_CASE(n) \
  case n: f(std::integral_constant<int, n>{}); return true;
    CSE_S0_CASE(1) CSE_S0_CASE(2) CSE_S0_CASE(3) CSE_S0_CASE(4) CSE_S0_CASE(5) CSE_S0_CASE(6)
    CSE_S0_CASE(7) CSE_S0_CASE(8) CSE_S0_CASE(9) CSE_S0_CASE(10) CSE_S0_CASE(11) CSE_S0_CASE(12)
    CSE_S0_CASE(13) CSE_S0_CASE(14) CSE_S0_CASE(15) CSE_S0_CASE(16)
#undef CSE_S0_CASE
    default: return false;
  }
}

// The kernels' loss template argument of a cse_loss kind, as a visitor:
// Visit(loss, f) calls f(std::integral_constant<int, L>).  UniformLosses:
// Huber, Cauchy, and the trivial loss for every other kind (the group's
// parameters in GroupArgs::loss).  PerBlockLosses: their per-block forms
// (loss.hpp: parameters from GroupArgs::loss_data).  Every picker below takes
// the visitor as its first template argument and is otherwise the same
// function for both, so a per-block group gets the kernel family of its
// uniform twin.
struct UniformLosses {
  static constexpr bool kPerBlock = false;
  template <class F>
  static auto Visit(int loss, F&& f) {
    switch (loss) {
      case CSE_LOSS_HUBER: return f(std::integral_constant<int, kLossHuber>{});
      case CSE_LOSS_CAUCHY: return f(std::integral_constant<int, kLossCauchy>{});
      default: return f(std::integral_constant<int, kLossTrivial>{});
    }
  }
};
struct PerBlockLosses {
  static constexpr bool kPerBlock = true;
  template <class F>
  static auto Visit(int loss, F&& f) {
    switch (loss) {
      case CSE_LOSS_HUBER: return f(std::integral_constant<int, kLossHuberPerBlock>{});
      case CSE_LOSS_CAUCHY: return f(std::integral_constant<int, kLossCauchyPerBlock>{});
      default: return f(std::integral_constant<int, kLossTrivialPerBlock>{});
    }
  }
};

template <class LV, class K>
LaunchFn PickFusedK(int loss, bool crs, bool points) {
  return LV::Visit(loss, [&](auto l) -> LaunchFn {
    constexpr int L = decltype(l)::value;
    return points ? (crs ? &LaunchFusedPoints<K, L, true> : &LaunchFusedPoints<K, L, false>)
                  : (crs ? &LaunchFused<K, L, true> : &LaunchFused<K, L, false>);
  });
}

template <class LV, class K, bool Crs>
LaunchFn PickFusedC0(int loss, bool points) {
  using TP = PointsOnlyTuneC0;
  using TF = ShippedTuneC0;
  return LV::Visit(loss, [&](auto l) -> LaunchFn {
    constexpr int L = decltype(l)::value;
    return points ? &LaunchFusedPoints<K, L, Crs, TP> : &LaunchFused<K, L, Crs, TF>;
  });
}

// points = true: the slot-1 rows only (gradient_mode 0, slot 0 from
// CameraGradientKernel); false: with the slot-0 contributions (mode 3).
// const0: groups with constant slot-0 blocks (BSM).
template <class LV>
LaunchFn PickFused(int kind, int loss, int policy, bool points, bool const0 = false) {
  const bool crs = policy == kAffineCrs;
  if (const0) {
    if (kind == kKindQuaternionTangent)
      return crs ? PickFusedC0<LV, SnavelyQuaternionTangentKind, true>(loss, points)
                 : PickFusedC0<LV, SnavelyQuaternionTangentKind, false>(loss, points);
    return crs ? PickFusedC0<LV, SnavelyKind, true>(loss, points)
               : PickFusedC0<LV, SnavelyKind, false>(loss, points);
  }
  if (kind == kKindQuaternionTangent)
    return PickFusedK<LV, SnavelyQuaternionTangentKind>(loss, crs, points);
  return PickFusedK<LV, SnavelyKind>(loss, crs, points);
}

// Affine kernels: cooperative slot-0 gather by LDS-DMA from the repacked
// table (dma = true) or by 8-byte pieces straight from the state.
template <class K, int L, bool Crs>
LaunchFn PickAffine(bool jac, bool dma) {
  if constexpr (!Crs && kTwoRoundBsm<K>) {
    // (the 8-byte-piece gather of kCoop 1 would spill at 128 VGPRs)
    if (jac && dma) return &LaunchTwoRound<K, L, 2>;
  }
  if constexpr (Crs) {
    // 1778 CRS 0.298 -> 0.285 ms, 13682 CRS 1.540 -> 1.480 ms (profiles/round2/s5k)
    if (jac && dma) return &LaunchTwoRoundCrs<K, L, 2>;
  }
  if (dma) return jac ? &LaunchChunks<K, L, true, Crs, 2> : &LaunchChunks<K, L, false, Crs, 2>;
  return jac ? &LaunchChunks<K, L, true, Crs, 1> : &LaunchChunks<K, L, false, Crs, 1>;
}

template <class K, int L>
LaunchFn PickJP(bool jac, int policy, bool dma) {
  if constexpr (KindTraits<K>::NB <= 2 && KindTraits<K>::NR <= 3) {
    switch (policy) {
      case kAffinePacked: return PickAffine<K, L, false>(jac, dma);
      case kAffineCrs: return PickAffine<K, L, true>(jac, dma);
      default: break;
    }
  }
  return jac ? &LaunchTable<K, L, true> : &LaunchTable<K, L, false>;
}

// const0: the group has constant slot-0 blocks (FusedKind kinds, the
// repacked table; DetectAffine): the Jacobian kernel with the packed F cells
// (BSM) or the packed row blocks of two widths (CRS).
template <class LV>
LaunchFn PickConst0(int kind, int loss, bool jac, bool crs) {
  auto pick = [&](auto kd) -> LaunchFn {
    using K = decltype(kd);
    using T = ShippedTuneC0;
    if (!jac) return nullptr;  // residual/cost kernels write no Jacobian: the usual ones
    return LV::Visit(loss, [&](auto l) -> LaunchFn {
      constexpr int L = decltype(l)::value;
      return crs ? &LaunchTwoRoundCrs<K, L, 2, T> : &LaunchTwoRound<K, L, 2, T>;
    });
  };
  if (kind == kKindQuaternionTangent) return pick(SnavelyQuaternionTangentKind{});
  if (kind == CSE_FUNCTOR_SNAVELY_2_9_3) return pick(SnavelyKind{});
  return nullptr;
}

template <class LV>
LaunchFn Pick(int kind, int loss, bool jac, int policy, bool dma, bool const0 = false) {
  if (const0 && jac)
    return (policy == kAffinePacked || policy == kAffineCrs) && dma
               ? PickConst0<LV>(kind, loss, jac, policy == kAffineCrs)
               : nullptr;
  LaunchFn fn = nullptr;
  VisitKind(kind, [&](auto kd) {
    using K = decltype(kd);
    if constexpr (AffineOnly<K>::value) {
      if (policy == kAffinePacked || policy == kAffineCrs)
        fn = LV::Visit(loss, [&](auto l) -> LaunchFn {
          constexpr int L = decltype(l)::value;
          return policy == kAffineCrs ? PickAffine<K, L, true>(jac, dma) : PickAffine<K, L, false>(jac, dma);
        });
    } else if constexpr (TestOnly<K>::value) {
      if constexpr (!LV::kPerBlock)  // (cse_create refuses per-block parameters on the test kinds)
        if (loss == CSE_LOSS_TRIVIAL)
          fn = jac ? &LaunchTable<K, kLossTrivial, true> : &LaunchTable<K, kLossTrivial, false>;
    } else {
      fn = LV::Visit(loss, [&](auto l) -> LaunchFn { return PickJP<K, decltype(l)::value>(jac, policy, dma); });
    }
  });
  return fn;
}

// CameraGradientKernel of a fused-gradient library kind (the Snavely camera,
// or the quaternion camera on its manifold), W waves per workgroup.
template <class LV, int W>
void LaunchCameraGradientOf(int kind, int loss, const CamGradArgs& cg, hipStream_t s) {
  const dim3 grid((unsigned)((cg.nslots + W - 1) / W));
  auto launch = [&](auto kd) {
    using K = decltype(kd);
    LV::Visit(loss, [&](auto l) {
      hipLaunchKernelGGL((CameraGradientKernel<K, decltype(l)::value, W>), grid, dim3(W * kWave), 0, s, cg);
    });
  };
  if (kind == kKindQuaternionTangent) launch(SnavelyQuaternionTangentKind{});
  else launch(SnavelyKind{});
}

}  // namespace cse

#endif  // CSE_KERNEL_PICKERS_HPP_
