// cse_evaluator.hip -- the C ABI (include/cse.h) over the gfx950 kernels:
// the user-kind registry, create and upload, the evaluation and Plus.  The
// calls a linear solver makes on the same evaluator (evaluator.hpp) are in
// linear_operators.hip.
//
// Host side of the evaluator: uploads the Program once
// (RegisteredCUDAEvaluators::Init, internal/ceres/registered_cuda_evaluators.cc:226-280)
// as the host-only planner laid it out (plan.hpp: descriptor validation, the
// layout policy of each residual group, its gradient plans and tables), and
// runs one fused kernel per group plus one finalize kernel per evaluation
// (RegisteredCUDAEvaluators::Evaluate, :46-103).
//
// The library reads no environment variable and has no build-time
// alternatives: every kernel it can launch is the shipped one for its
// (functor, loss, outputs, layout).  The settings measured and not shipped
// are recorded in DESIGN.md §4.4 (and the git history before round 6).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/cse.h"
#include "evaluation_kernels.hpp"
#include "evaluator.hpp"
#include "group_store_kernel.hpp"
#include "jet_kernels.h"
#include "kernel_pickers.hpp"
#include "launch.hpp"
#include "multi_device.h"
#include "per_block_loss_kernels.h"
#include "plan.hpp"

namespace cse {
std::string& LastError();  // layout.cpp: one per thread (cse_last_error reads it here)
}  // namespace cse

namespace {

using cse::DevBuf;
using cse::Fail;
using cse::Group;
using cse::kAffineCrs;
using cse::kAffinePacked;
using cse::kKindQuaternionTangent;
using cse::kTable;
using cse::KindShape;
using cse::LaunchFn;
using cse::VisitKind;
using cse::VisitSlot0Size;
using TestLinear3_234 = cse::TestLinear3_234;
using TestLinear3_432 = cse::TestLinear3_432;
using TestLinear2_23 = cse::TestLinear2_23;
using TestLinear3_24 = cse::TestLinear3_24;
using TestLinear4_34 = cse::TestLinear4_34;

// The uniform-loss pickers (kernel_pickers.hpp); a group with per-block loss
// parameters takes cse::PerBlockPick / PerBlockPickFused instead.
LaunchFn Pick(int kind, int loss, bool jac, int policy, bool dma, bool const0 = false) {
  return cse::Pick<cse::UniformLosses>(kind, loss, jac, policy, dma, const0);
}
LaunchFn PickFused(int kind, int loss, int policy, bool points, bool const0 = false) {
  return cse::PickFused<cse::UniformLosses>(kind, loss, policy, points, const0);
}

// The planner's shape table (plan.hpp, cse::kKindRows) row by row against
// the functor types the kernels are instantiated with.
template <class K>
constexpr bool KindRowMatches(int kind) {
  using Tr = cse::KindTraits<K>;
  const cse::KindRow* r = cse::KindRowOf(kind);
  if (!r || r->nr != Tr::NR || r->nb != Tr::NB || r->data != Tr::D || r->x0 != Tr::X0) return false;
  for (int j = 0; j < cse::kMaxSlots; ++j)
    if (r->sz[j] != (j < Tr::NB ? K::kSizes[j] : 0)) return false;
  return true;
}
#define CSE_KIND_ROW(kind, K) static_assert(KindRowMatches<K>(kind), "plan.hpp: kKindRows row of " #kind)
CSE_KIND_ROW(kKindQuaternionTangent, cse::SnavelyQuaternionTangentKind);
CSE_KIND_ROW(CSE_FUNCTOR_SNAVELY_2_9_3, cse::SnavelyKind);
CSE_KIND_ROW(CSE_FUNCTOR_SNAVELY_NO_DISTORTION_2_7_3, cse::SnavelyNoDistortionKind);
CSE_KIND_ROW(CSE_FUNCTOR_SNAVELY_QUATERNION_2_10_3, cse::SnavelyQuaternionKind);
CSE_KIND_ROW(CSE_FUNCTOR_POINT_DISPLACEMENT_3_3, cse::PointDisplacementKind);
CSE_KIND_ROW(CSE_FUNCTOR_TEST_LINEAR_3_2_3_4, TestLinear3_234);
CSE_KIND_ROW(CSE_FUNCTOR_TEST_LINEAR_3_4_3_2, TestLinear3_432);
CSE_KIND_ROW(CSE_FUNCTOR_TEST_LINEAR_2_2_3, TestLinear2_23);
CSE_KIND_ROW(CSE_FUNCTOR_TEST_LINEAR_3_2_4, TestLinear3_24);
CSE_KIND_ROW(CSE_FUNCTOR_TEST_LINEAR_4_3_4, TestLinear4_34);
CSE_KIND_ROW(CSE_FUNCTOR_TEST_BILINEAR_1_2_2, cse::BilinearTestKind);
CSE_KIND_ROW(CSE_FUNCTOR_TEST_TEN_PARAMETER_1_x10, cse::TenParameterTestKind);
CSE_KIND_ROW(CSE_FUNCTOR_TEST_PARTIAL_OUTPUT_2_1, cse::PartialOutputTestKind);
#undef CSE_KIND_ROW
static_assert(sizeof(cse::kKindRows) / sizeof(cse::kKindRows[0]) == 13, "one assert per kKindRows row");

// ---- User functor kinds (cse_register_functor): the kernels live in the
// user's TU (include/ceres_amd/autodiff_cuda.h); the library holds their
// launch tables.  Entries are never removed, so a pointer to one stays valid.
struct UserKindEntry {
  cse_functor_ops ops;
  std::string name;
};
std::mutex g_user_mu;
std::vector<UserKindEntry*> g_user_kinds;

const cse_functor_ops* UserOps(int kind) {
  if (kind < CSE_FUNCTOR_USER_FIRST) return nullptr;
  std::lock_guard<std::mutex> lock(g_user_mu);
  const size_t i = (size_t)(kind - CSE_FUNCTOR_USER_FIRST);
  return i < g_user_kinds.size() ? &g_user_kinds[i]->ops : nullptr;
}

bool IsUserKind(int kind) { return UserOps(kind) != nullptr; }

}  // namespace

// A registered user kind's launch table and name (cse::UserLookup).
const cse_functor_ops* CseUserKind(int kind, std::string* name) {
  if (kind < CSE_FUNCTOR_USER_FIRST) return nullptr;
  std::lock_guard<std::mutex> lock(g_user_mu);
  const size_t i = (size_t)(kind - CSE_FUNCTOR_USER_FIRST);
  if (i >= g_user_kinds.size()) return nullptr;
  *name = g_user_kinds[i]->name;
  return &g_user_kinds[i]->ops;
}

namespace {

bool ShapeOf(int kind, KindShape* k) { return cse::ShapeOf(kind, UserOps(kind), k); }

// Cost reduction: above this many per-wave partials, kPartialBlocks
// workgroups sum slices and the last of them finalises
// (ReduceFinalizeKernel); below, one FinalizeKernel.
constexpr int64_t kPartialsTwoPass = 4096;
constexpr int kPartialBlocks = 128;

// The post-pass form of a plan (cse::GradForm) and its chunk table.
int GradFormOf(const cse::GradArgs& ga, const Group::GradPlan& P) {
  if (ga.perm == nullptr) return cse::kGradRange;  // identity order: contiguous ranges (points)
  return P.wave ? cse::kGradChunked : cse::kGradPerBlock;  // many blocks per parameter block: chunks
}
cse::GradChunks GradChunksOf(const Group::GradPlan& P) {
  return cse::GradChunks{P.chunk_begin.p, P.chunk_off.p, P.chunk_partial.p, P.nchunks};
}

}  // namespace

// evaluator.hpp's functions, which linear_operators.hip calls too.
namespace cse {

bool LaunchGradPass(int nr, int size, const cse::GradArgs& ga, const Group::GradPlan& P,
                    hipStream_t s, const cse_functor_ops* user, int slot) {
  const int form = GradFormOf(ga, P);
  const cse::GradChunks ch = GradChunksOf(P);
  if (user) {
    if (!user->gradient[slot]) return false;
    user->gradient[slot](&ga, &ch, form, s);
    return true;
  }
  if (nr == 2 && size == 9) return cse::LaunchGradientSlot<2, 9>(ga, ch, form, s), true;
  if (nr == 2 && size == 3) return cse::LaunchGradientSlot<2, 3>(ga, ch, form, s), true;
  if (nr == 2 && size == 7) return cse::LaunchGradientSlot<2, 7>(ga, ch, form, s), true;
  if (nr == 2 && size == 10) return cse::LaunchGradientSlot<2, 10>(ga, ch, form, s), true;
  if (nr == 3 && size == 3) return cse::LaunchGradientSlot<3, 3>(ga, ch, form, s), true;
  return false;
}

cse::GroupArgs MakeArgs(cse_evaluator* ev, Group& G, const double* state, double* res,
                        double* jac, double* grad) {
  cse::GroupArgs a{};
  a.n = G.n;
  a.ids = G.ids.p;
  a.data = G.data.p;
  a.state = state;
  a.cstate = ev->cstate.p;
  a.pbs = ev->pbs.p;
  a.plus_jacobians = ev->plus_jac.p;
  for (int j = 0; j < 2; ++j) {
    a.state_base[j] = G.state_base[j];
    a.delta_base[j] = G.delta_base[j];
    a.jac_stride[j] = G.jac_stride[j];
    for (int r = 0; r < 3; ++r) a.jac_base[j][r] = G.jac_base[j][r];
  }
  a.res_base = G.res_base;
  a.packed0 = G.packed0.p;
  a.packed0_lo = G.slot0_lo;
  a.packed0_stride = G.packed_stride;
  a.act0_bits = G.act0.p;
  a.fbase = G.fbase.p;
  a.side = G.side.p;
  a.delta0 = G.delta0.p;
  a.gindex = G.gindex.p;
  a.first = G.first;
  a.residual_layout = ev->res_layout.p;
  a.jac_layout = ev->jac_layout.p;
  a.jac_offsets = ev->jac_offsets.p;
  a.residuals = res;
  a.jacobian = jac;
  a.gradient = grad;
  a.partials = ev->partials.p + G.partial_offset;
  a.status = ev->status.p;
  a.loss.a = G.loss.a;
  a.loss.scale = G.loss.scale;
  a.loss.scaled = G.loss.scaled;
  static_assert(sizeof(a.user_loss) == sizeof(G.loss.user), "user loss bytes");
  std::memcpy(a.user_loss, G.loss.user, sizeof(a.user_loss));
  a.apply_loss = ev->opts.apply_loss_function;
  a.check_finite = ev->opts.check_finite;
  a.table_runs = G.runs.p;
  a.plain0 = G.plain0 ? 1 : 0;
  a.plain0_state_base = G.plain0_state_base;
  a.plain0_delta_base = G.plain0_delta_base;
  a.loss_data = G.loss_data.p;
  return a;
}

cse::GradArgs SlotGradArgs(const Group& G, int j, const double* jac, const double* res, double* grad) {
  const Group::GradPlan& P = G.grad[j];
  cse::GradArgs ga{};
  ga.jac = jac;
  for (int r = 0; r < G.shape.nr && r < 3; ++r) ga.jrow[r] = G.jac_base[j][r];
  ga.jstride = G.jac_stride[j];
  ga.res = res;
  ga.res_base = G.res_base;
  ga.perm = P.perm.p;
  ga.off = P.off.p;
  ga.count = P.count;
  ga.lo = P.lo;
  ga.grad = grad;
  ga.delta_base = G.delta_base[j];
  return ga;
}

int LaunchContribReduce(const Group::GradPlan& P, const double* gcontrib, const cse::GradArgs& ga,
                        hipStream_t s) {
  const cse::GradChunks ch = GradChunksOf(P);
  if (P.nchunks > 0)
    hipLaunchKernelGGL((cse::GradientContribKernel<9, 10>),
                       dim3((unsigned)((P.nchunks + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
                       dim3(cse::kBlockThreads), 0, s, gcontrib, P.perm.p, ch, P.chunk_order.p);
  hipLaunchKernelGGL((cse::GradientChunkReduceKernel<9>),
                     dim3((unsigned)((ga.count + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                     dim3(cse::kBlockThreads), 0, s, ga, ch);
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

int LaunchFusedGradTail(const Group& G, double* out, hipStream_t s) {
  const int64_t entries = 2 * ((G.n + cse::kWave - 1) / cse::kWave);
  hipLaunchKernelGGL((cse::GradientBoundaryKernel<3>),
                     dim3((unsigned)((entries + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                     dim3(cse::kBlockThreads), 0, s, G.gside.p, entries, out, G.delta_base[1]);
  const Group::GradPlan& P = G.grad[0];
  cse::GradArgs ga{};
  ga.count = P.count;
  ga.lo = P.lo;
  ga.grad = out;
  ga.delta_base = G.delta_base[0];
  ga.delta_tab = G.const0 ? G.delta0.p + (P.lo - G.slot0_lo) : nullptr;
  return LaunchContribReduce(P, G.gcontrib.p, ga, s);
}

}  // namespace cse

namespace {

int FoldTiming(cse_evaluator* ev) {
  for (auto& pr : ev->pending) {
    float ms = 0.f;
    CSE_HIP(hipEventSynchronize(pr.second));
    CSE_HIP(hipEventElapsedTime(&ms, pr.first, pr.second));
    ev->last_ms = ms;
    ev->total_ms += ms;
    ev->launches += 1;
    ev->pool.push_back(pr);
  }
  ev->pending.clear();
  return CSE_OK;
}

// gradient_mode 0: the slot-1 boundary entries as LaunchFusedGradTail's, and
// the slot-0 sums by re-evaluation in camera order (CameraGradientKernel), then
// GradientChunkReduceKernel.  The sorted inputs are built on first use
// (CamGradSortedInputs, on the evaluator's stream).
int CamGradSortedInputs(Group& G, hipStream_t s) {
  const Group::GradPlan& P = G.grad[0];
  const int D = G.shape.data;
  int rc;
  if (!G.sorted_ready) {  // set only once the copies have been queued
    if (D != 2 && !UserFused(G))
      return Fail(CSE_ERR_UNSUPPORTED, "camera-order gradient: 2 data doubles per block");
    if ((rc = G.sdata.alloc((size_t)G.n * D))) return rc;
    if ((rc = G.sid1.alloc((size_t)G.n))) return rc;
    const dim3 grid((unsigned)((G.n + cse::kBlockThreads - 1) / cse::kBlockThreads));
    if (D == 2)
      hipLaunchKernelGGL((cse::SortSlot0InputsKernel<2>), grid, dim3(cse::kBlockThreads), 0, s, G.ids.p,
                         G.data.p, P.perm.p, P.nperm, G.sdata.p, G.sid1.p);
    else
      hipLaunchKernelGGL((cse::SortSlot0InputsAnyKernel<>), grid, dim3(cse::kBlockThreads), 0, s, G.ids.p,
                         G.data.p, D, P.perm.p, P.nperm, G.sdata.p, G.sid1.p);
    CSE_HIP(hipGetLastError());
    G.sorted_ready = true;
  }
  return CSE_OK;
}

// Waves per workgroup of CameraGradientKernel (one chunk per wave).
constexpr int kCamGradWavesPerWg = cse::kWavesPerBlock;

// CameraGradientKernel: the per-chunk slot-0 sums into P.chunk_partial.
int LaunchCameraGradKernel(cse_evaluator* ev, Group& G, const double* state, hipStream_t s) {
  const Group::GradPlan& P = G.grad[0];
  cse::CamGradArgs cg{};
  cg.state = state;
  cg.state_base0 = G.state_base[0];
  cg.state_base1 = G.state_base[1];
  cg.sdata = G.sdata.p;
  cg.sid1 = G.sid1.p;
  cg.chunk_pb = P.chunk_pb.p;
  cg.chunk_begin = P.chunk_begin.p;
  cg.chunk_order = P.chunk_order.p;
  cg.partial = P.chunk_partial.p;
  cg.nchunks = P.nchunks;
  cg.nslots = P.nchunks;
  cg.loss.a = G.loss.a;
  cg.loss.scale = G.loss.scale;
  cg.loss.scaled = G.loss.scaled;
  cg.apply_loss = ev->opts.apply_loss_function;
  cg.loss_data = G.loss_data.p;  // records in the blocks' original order: through the plan's perm
  cg.perm = P.perm.p;
  if (G.const0) {  // active cameras' state offsets need not be affine
    cg.packed0 = G.packed0.p;
    cg.packed_lo = G.slot0_lo;
    cg.packed_stride = G.packed_stride;
  }
  if (G.user) {  // the kind's own CameraGradientKernel (its TU), with its loss object
    static_assert(sizeof(cg.user_loss) == sizeof(G.loss.user), "user loss bytes");
    std::memcpy(cg.user_loss, G.loss.user, sizeof(cg.user_loss));
    if (P.nchunks > 0) G.user->camera_gradient(&cg, cg.nslots, s);
    CSE_HIP(hipGetLastError());
    return CSE_OK;
  }
  constexpr int W = kCamGradWavesPerWg;
  static_assert(W == cse::kPerBlockCamGradWaves, "the per-block launch takes the same workgroups");
  if (P.nchunks > 0) {
    if (G.jet) cse::LaunchJetCameraGradient(G.loss.kind, cg, cg.nslots, s);
    else if (G.loss_data_size) cse::LaunchPerBlockCameraGradient(G.kind, G.loss.kind, cg, s);
    else cse::LaunchCameraGradientOf<cse::UniformLosses, W>(G.kind, G.loss.kind, cg, s);
  }
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

// After the points kernel and CameraGradientKernel: the slot-1 boundary
// entries, then the slot-0 rows from the chunk sums, in a fixed order.
// assign (grad_exact): the rows are written, not added to.  The boundary
// entries and the camera rows in one launch (GradientTailKernel).
int LaunchCameraGradReduce(Group& G, double* out, hipStream_t s, bool assign = false) {
  const Group::GradPlan& P = G.grad[0];
  const int64_t entries = 2 * ((G.n + cse::kWave - 1) / cse::kWave);
  const int64_t bwg = (entries + cse::kBlockThreads - 1) / cse::kBlockThreads;
  cse::GradArgs ga{};
  ga.count = P.count;
  ga.lo = P.lo;
  ga.grad = out;
  ga.delta_base = G.delta_base[0];
  ga.delta_tab = G.const0 ? G.delta0.p + (P.lo - G.slot0_lo) : nullptr;
  const cse::GradChunks ch{P.chunk_begin.p, P.chunk_off.p, P.chunk_partial.p, P.nchunks};
  const int64_t cwg = (ga.count + cse::kBlockThreads - 1) / cse::kBlockThreads;
  const dim3 grid((unsigned)(bwg + cwg));
  auto tail = [&](auto s0) {
    constexpr int S0 = decltype(s0)::value;
    if (assign)
      hipLaunchKernelGGL((cse::GradientTailKernel<3, S0, true>), grid, dim3(cse::kBlockThreads), 0, s, G.gside.p,
                         entries, G.delta_base[1], bwg, ga, ch);
    else
      hipLaunchKernelGGL((cse::GradientTailKernel<3, S0, false>), grid, dim3(cse::kBlockThreads), 0, s,
                         G.gside.p, entries, G.delta_base[1], bwg, ga, ch);
  };
  if (!VisitSlot0Size(G.shape.s0, tail))
    return Fail(CSE_ERR_UNSUPPORTED, "fused gradient: slot 0 of " + std::to_string(G.shape.s0) + " parameters");
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

// One planned group's tables to the device (cse::PlanGroup made T), its ids
// and functor data, and the buffers the plan sizes.  Returns once every copy
// has completed, so the caller may release T.
int UploadGroup(const cse_residual_group& g, const cse::GroupTables& T, Group* Gp, hipStream_t s) {
  Group& G = *Gp;
  const KindShape& k = G.shape;
  int rc;
  if (G.repack0 && (rc = G.packed0.alloc((size_t)G.slot0_count * G.packed_stride))) return rc;
  if ((rc = G.act0.upload(T.bits.data(), T.bits.size(), s))) return rc;
  if ((rc = G.src0.upload(T.src.data(), T.src.size(), s))) return rc;
  if ((rc = G.delta0.upload(T.dlt.data(), T.dlt.size(), s))) return rc;
  if ((rc = G.fbase.upload(T.fbase.data(), T.fbase.size(), s))) return rc;
  if ((rc = G.prev_seg.upload(T.prev_seg.data(), T.prev_seg.size(), s))) return rc;
  if ((rc = G.side.alloc(T.prev_seg.size() * 16))) return rc;
  for (int j = 0; j < 2; ++j) {
    Group::GradPlan& D = G.grad[j];
    const cse::GradTables& H = T.grad[j];
    static_cast<cse::GradPlanInfo&>(D) = T.grad_info[j];
    if ((rc = D.perm.upload(H.perm.data(), H.perm.size(), s))) return rc;
    if ((rc = D.off.upload(H.off.data(), H.off.size(), s))) return rc;
    if ((rc = D.chunk_order.upload(H.chunk_order.data(), H.chunk_order.size(), s))) return rc;
    if ((rc = D.chunk_begin.upload(H.chunk_begin.data(), H.chunk_begin.size(), s))) return rc;
    if ((rc = D.chunk_off.upload(H.chunk_off.data(), H.chunk_off.size(), s))) return rc;
    if ((rc = D.chunk_pb.upload(H.chunk_pb.data(), H.chunk_pb.size(), s))) return rc;
    const int size = j == 0 ? k.s0 : k.s1;
    if (D.ready && !D.sorted &&
        (rc = D.chunk_partial.alloc((size_t)std::max<int64_t>(1, D.nchunks) * size)))
      return rc;
  }
  if ((rc = G.runs.upload(T.runs.data(), T.runs.size(), s))) return rc;
  if ((rc = G.ids.upload(g.parameter_block_ids, (size_t)g.num_blocks * k.nb, s))) return rc;
  // Per-block loss parameters: the rows de-interleaved, so that the kernels'
  // functor data keeps its [n][D] form and the (a, scale) records are one
  // aligned 16-byte load each.  (The host copies live until the wait below.)
  std::vector<double> rows, records;
  if (G.loss_data_size) {
    const int64_t n = g.num_blocks, D = k.data, W = D + G.loss_data_size;
    rows.resize((size_t)(n * D));
    records.resize((size_t)(n * 2));
    for (int64_t i = 0; i < n; ++i) {
      for (int64_t c = 0; c < D; ++c) rows[i * D + c] = g.functor_data[i * W + c];
      records[2 * i] = g.functor_data[i * W + D];
      records[2 * i + 1] = g.functor_data[i * W + D + 1];
    }
    if ((rc = G.data.upload(rows.data(), rows.size(), s))) return rc;
    if ((rc = G.loss_data.upload(records.data(), records.size(), s))) return rc;
  } else if ((rc = G.data.upload(g.functor_data, (size_t)g.num_blocks * k.data, s))) {
    return rc;
  }
  if ((!G.affine || G.const0) && g.residual_block_index &&
      (rc = G.gindex.upload(g.residual_block_index, (size_t)g.num_blocks, s)))
    return rc;
  if (hipStreamSynchronize(s) != hipSuccess) return Fail(CSE_ERR_HIP, "upload failed");
  return CSE_OK;
}

// How a group's gradient is summed in one evaluation (cse_options.
// gradient_mode, cse.h): grad_pass = a deterministic post-pass over the
// written residuals and Jacobian (the group has plans for all its slots),
// else in-kernel FP64 atomics (as the reference); fused = the fused form
// (FusedGrad); recompute = its slot-0 rows by CameraGradientKernel (modes 0
// and 1 on held-camera groups) rather than written contributions (mode 3).
struct GradPath {
  bool grad_pass = false, fused = false, recompute = false;
};
// Does gradient_mode give a fused-eligible group the fused form?
// Mode 1 (post-pass) has no form over the packed F cells of a group with
// constant slot-0 blocks: it takes mode 0's fused form (also fixed order).
// The Jet form has no mode-3 kernel (contributions in block order): the
// post-pass instead, as for groups without a fused form.
bool FusedGradMode(const cse_evaluator* ev, const Group& G) {
  const int mode = ev->opts.gradient_mode;
  return G.fuse_ok && (mode == 0 || (!G.user && ((mode == 3 && !G.jet) || (mode == 1 && G.const0))));
}
GradPath GradPathOf(const cse_evaluator* ev, const Group& G, bool grad, bool res, bool jac) {
  GradPath p;
  p.grad_pass = grad && res && jac && G.affine && ev->opts.gradient_mode != 2;
  for (int j = 0; j < G.shape.nb; ++j) p.grad_pass = p.grad_pass && G.grad[j].ready;
  p.fused = p.grad_pass && FusedGradMode(ev, G);
  // Constant slot-0 blocks: no post-pass over the packed F cells (in-kernel
  // atomics instead, active cameras only).
  if (G.const0 && !p.fused) p.grad_pass = false;
  p.recompute = p.fused && ev->opts.gradient_mode != 3;
  return p;
}

// Enqueue one evaluation on ev->stream.
// same_point (CSE_EVAL_SAME_POINT): the state equals the previous
// evaluation's, so the packed slot-0 tables it built are still valid and the
// repack launches are skipped.
int Enqueue(cse_evaluator* ev, const double* d_state, double* d_cost, double* d_res,
            double* d_grad, double* d_jac, bool same_point = false) {
  if (d_jac && !ev->has_layout)
    return Fail(CSE_ERR_INVALID, "Jacobian requested but the descriptor had no Jacobian layout");
  const bool repack = !(same_point && ev->point_current);
  ev->point_current = false;  // set again once every launch below is queued
  const bool jets = d_jac || d_grad;
  std::pair<hipEvent_t, hipEvent_t> timing{nullptr, nullptr};
  if (ev->opts.profile) {
    if (ev->pool.empty()) {
      // Timing only: no system-scope fence (cache write-back and
      // invalidation) at either event, which cost ~7-10 us per evaluation
      // at the 8-way shard and problem-16 (profiles/round3/ov0).
      CSE_HIP(hipEventCreateWithFlags(&timing.first, hipEventDisableSystemFence));
      CSE_HIP(hipEventCreateWithFlags(&timing.second, hipEventDisableSystemFence));
    } else {
      timing = ev->pool.back();
      ev->pool.pop_back();
    }
    if (ev->pending.size() > 4096) {
      int rc = FoldTiming(ev);
      if (rc) return rc;
    }
  }
  // One grad_exact group whose gradient takes the fused form with the
  // camera rows recomputed (the fused points kernel, the camera rows and the
  // boundary rows then write every row exactly once): no zeroing pass, the
  // tail kernels assign.  The same predicate as the group loop below.
  const bool grad_assign =
      d_grad && ev->groups.size() == 1 && ev->groups[0].grad_exact &&
      GradPathOf(ev, ev->groups[0], d_grad != nullptr, d_res != nullptr, d_jac != nullptr).recompute;
  if (d_grad && ev->num_effective > 0 && !grad_assign)
    CSE_HIP(hipMemsetAsync(d_grad, 0, ev->num_effective * sizeof(double), ev->stream));
  if (d_jac && !ev->jac_covered && ev->num_jacobian_values > 0)
    CSE_HIP(hipMemsetAsync(d_jac, 0, ev->num_jacobian_values * sizeof(double), ev->stream));
  if (d_res && !ev->res_covered && ev->num_residuals > 0)
    CSE_HIP(hipMemsetAsync(d_res, 0, ev->num_residuals * sizeof(double), ev->stream));
  for (size_t g = 0; g < ev->groups.size(); ++g) {
    Group& G = ev->groups[g];
    if (G.n == 0) continue;
    const bool dma = G.packed0.p != nullptr;
    LaunchFn fn = nullptr;
    cse_kernel_launch_fn ufn = nullptr;  // a user kind's kernel (its own TU)
    if (G.user) {
      ufn = G.policy == kTable ? G.user->table[jets ? 1 : 0]
                               : G.user->affine[G.policy == kAffineCrs][jets ? 1 : 0][dma ? 1 : 0];
      if (!ufn) return Fail(CSE_ERR_UNSUPPORTED, "user functor kind " + G.user_name + " has no such kernel");
    } else {
      fn = G.loss_data_size ? cse::PerBlockPick(G.kind, G.loss.kind, jets, G.policy, dma, G.const0)
                            : Pick(G.kind, G.loss.kind, jets, G.policy, dma, G.const0);
      if (G.jet && jets)  // the Jet<double, 12> instantiations (cse_create kept only these shapes)
        fn = G.policy == kTable ? cse::JetSnavelyTable(G.loss.kind)
                                : cse::JetSnavelyJacobian(G.loss.kind, G.policy == kAffineCrs);
      if (!fn) return Fail(CSE_ERR_UNSUPPORTED, "no kernel for functor kind " + std::to_string(G.kind));
    }
    const GradPath gp = GradPathOf(ev, G, d_grad != nullptr, d_res != nullptr, d_jac != nullptr);
    const bool grad_pass = gp.grad_pass, fused = gp.fused, recompute = gp.recompute;
    cse::GroupArgs a = MakeArgs(ev, G, d_state, d_res, d_jac, grad_pass ? nullptr : d_grad);
    if (fused) {
      const int64_t chunks = (G.n + cse::kWave - 1) / cse::kWave;
      int rc;
      if ((rc = G.gside.ensure((size_t)(2 * chunks * 4)))) return rc;
      if (!recompute && (rc = G.gcontrib.ensure((size_t)G.n * G.slot0_stride))) return rc;
      a.gfused = d_grad;
      a.gside = G.gside.p;
      a.gcontrib = G.gcontrib.p;
      if (G.user)
        ufn = G.user->fused_points[G.policy == kAffineCrs];
      else
        fn = G.loss_data_size ? cse::PerBlockPickFused(G.kind, G.loss.kind, G.policy, recompute, G.const0)
                              : PickFused(G.kind, G.loss.kind, G.policy, recompute, G.const0);
      if (G.jet) fn = cse::JetSnavelyFusedPoints(G.loss.kind, G.policy == kAffineCrs);
    }
    if (timing.first && g == 0) CSE_HIP(hipEventRecord(timing.first, ev->stream));
    if (dma && repack) {
      const int pieces = (G.shape.x0 + 1) / 2;
      const int64_t total = G.slot0_count * pieces;
      hipLaunchKernelGGL(cse::RepackSlot0Kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                         ev->stream, d_state, G.state_base[0], G.shape.x0, G.packed_stride, pieces,
                         G.slot0_lo, G.slot0_count, G.packed0.p, G.src0.p, ev->cstate.p);
    }
    if (recompute) {
      const int rc = CamGradSortedInputs(G, ev->stream);
      if (rc) return rc;
    }
    if (ufn)
      ufn(&a, G.num_wg, ev->stream);
    else
      fn(a, G.num_wg, ev->stream);
    CSE_HIP(hipGetLastError());
    if (G.const0 && jets && d_jac && G.side.p) {
      // The 64-byte sectors two held-camera chunks share (the full chunks
      // stored their heads and tails in side slots), when the full chunks
      // took that tail: the same base alignment test as the kernel.
      if (cse::HeldWindowsAligned(d_res, G.res_base, d_jac, G.jac_base[1][0], G.fbase0)) {
        const int64_t nchunks = (G.n + cse::kWave - 1) / cse::kWave;
        const int64_t threads = 4 * nchunks;
        hipLaunchKernelGGL(cse::HeldSectorFixupKernel,
                           dim3((unsigned)((threads + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                           dim3(cse::kBlockThreads), 0, ev->stream, d_jac, G.fbase.p, G.side.p,
                           G.prev_seg.p, nchunks, G.n / cse::kWave);
        CSE_HIP(hipGetLastError());
      }
    }
    if (recompute) {
      // After the points kernel on the same stream (beside it on a second
      // stream measured 3.9 % slower, 2.23 vs 2.15 ms: profiles/round3/s2).
      int rc;
      if ((rc = LaunchCameraGradKernel(ev, G, d_state, ev->stream))) return rc;
      if ((rc = LaunchCameraGradReduce(G, d_grad, ev->stream, grad_assign))) return rc;
    } else if (fused) {
      const int rc = LaunchFusedGradTail(G, d_grad, ev->stream);
      if (rc) return rc;
    } else if (grad_pass) {
      const int sizes[2] = {G.shape.s0, G.shape.s1};
      for (int j = 0; j < G.shape.nb; ++j) {
        const cse::GradArgs ga = SlotGradArgs(G, j, d_jac, d_res, d_grad);
        if (!LaunchGradPass(G.shape.nr, sizes[j], ga, G.grad[j], ev->stream, G.user, j))
          return Fail(CSE_ERR_UNSUPPORTED, "no gradient pass for this shape");
        CSE_HIP(hipGetLastError());
      }
    }
  }
  if (timing.first) {
    if (ev->groups.empty()) CSE_HIP(hipEventRecord(timing.first, ev->stream));
    CSE_HIP(hipEventRecord(timing.second, ev->stream));
    ev->pending.push_back(timing);
  }
  const double* parts = ev->partials.p;
  const int64_t nparts = ev->total_wg;
  if (nparts > kPartialsTwoPass) {
    // Fixed-order slices summed by kPartialBlocks workgroups, the last of
    // which adds the slice sums: one launch (ReduceFinalizeKernel).
    const int64_t per = (nparts + kPartialBlocks - 1) / kPartialBlocks;
    hipLaunchKernelGGL(cse::ReduceFinalizeKernel, dim3(kPartialBlocks), dim3(cse::kBlockThreads), 0,
                       ev->stream, parts, nparts, per, ev->partials2.p, ev->status.p + 2, d_cost,
                       ev->status.p, ev->status.p + 1);
  } else {
    hipLaunchKernelGGL(cse::FinalizeKernel, dim3(1), dim3(1024), 0, ev->stream, parts, nparts,
                       d_cost, ev->status.p, ev->status.p + 1);
  }
  CSE_HIP(hipGetLastError());
  ev->point_current = true;
  return CSE_OK;
}

}  // namespace

extern "C" {

void cse_default_options(cse_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->device = -1;
  o->check_finite = 1;
  o->apply_loss_function = 1;
}

const char* cse_last_error(void) { return cse::LastError().c_str(); }

int cse_abi_version(void) { return CSE_ABI_VERSION; }

const char* cse_build_info(void) {
#define CSE_STR2_(x) #x
#define CSE_STR_(x) CSE_STR2_(x)
  return "cse abi=" CSE_STR_(CSE_ABI_VERSION) " target=gfx950 built " __DATE__ " " __TIME__;
}

int cse_create(const cse_problem_desc* d, const cse_options* options, cse_evaluator** out) {
  if (!out) return Fail(CSE_ERR_INVALID, "null out");
  *out = nullptr;
  // Validation comes in two parts, so that every refusal keeps its place in
  // the order callers know: the descriptor's own fields before the options,
  // the groups and their blocks (ValidateGroups) after the device is picked.
  int rc = cse::Validate(d);
  if (rc) return rc;
  cse_evaluator* ev = new (std::nothrow) cse_evaluator();
  if (!ev) return Fail(CSE_ERR_OOM, "host allocation failed");
  if (options) ev->opts = *options; else cse_default_options(&ev->opts);
  auto bail = [&](int code) { cse_destroy(ev); return code; };
  if (ev->opts.gradient_mode < 0 || ev->opts.gradient_mode > 3)
    return bail(Fail(CSE_ERR_INVALID, "gradient_mode " + std::to_string(ev->opts.gradient_mode) +
                                          " is not one of 0..3"));
  if (ev->opts.jacobian_form != CSE_JACOBIAN_CLOSED_FORM && ev->opts.jacobian_form != CSE_JACOBIAN_JET)
    return bail(Fail(CSE_ERR_INVALID, "jacobian_form " + std::to_string(ev->opts.jacobian_form) +
                                          " is not a cse_jacobian_form"));
  // (before the device is picked: a descriptor these refuse needs no GPU)
  if ((rc = cse::ValidateLossData(d, &ev->opts))) return bail(rc);

  if (ev->opts.device >= 0) {
    const hipError_t e = hipSetDevice(ev->opts.device);
    if (e != hipSuccess)
      return bail(Fail(CSE_ERR_HIP, "hipSetDevice(" + std::to_string(ev->opts.device) +
                                        ") failed: " + hipGetErrorString(e)));
    ev->device = ev->opts.device;
  } else {
    if (hipGetDevice(&ev->device) != hipSuccess) return bail(Fail(CSE_ERR_HIP, "no HIP device"));
  }
  if (hipDeviceGetAttribute(&ev->num_cus, hipDeviceAttributeMultiprocessorCount, ev->device) !=
      hipSuccess)
    return bail(Fail(CSE_ERR_HIP, "hipDeviceGetAttribute failed"));
  if (ev->opts.stream || ev->opts.use_stream) {
    ev->stream = (hipStream_t)ev->opts.stream;
  } else {
    if (hipStreamCreateWithFlags(&ev->stream, hipStreamNonBlocking) != hipSuccess)
      return bail(Fail(CSE_ERR_HIP, "hipStreamCreate failed"));
    ev->own_stream = true;
  }
  hipStream_t s = ev->stream;
  ev->num_parameter_blocks = d->num_parameter_blocks;
  ev->num_parameters = d->num_parameters;
  ev->num_effective = d->num_effective_parameters;
  ev->num_constant = d->num_constant_parameters;
  ev->num_residual_blocks = d->num_residual_blocks;
  ev->num_residuals = d->num_residuals;
  ev->num_jacobian_values = d->num_jacobian_values;
  ev->num_plus_jacobian_values = d->num_plus_jacobian_values;

  // Validate, then plan and upload one group at a time: a group's host
  // tables (UploadGroup waits for their copies) die before the next is planned.
  cse::ProgramPlan P;
  if ((rc = cse::ValidateGroups(d, &CseUserKind, &P, &ev->opts))) return bail(rc);
  ev->has_layout = P.has_layout;
  ev->groups.resize((size_t)d->num_groups);
  // The one group's tables outlive the loop when it has held cameras: the
  // Schur structure of such a group is planned from them.
  cse::GroupTables held_tables;
  bool have_held_tables = false;
  for (int gi = 0; gi < d->num_groups; ++gi) {
    Group& G = ev->groups[gi];
    const cse_residual_group& g = d->groups[gi];
    cse::GroupTables T;
    cse::PlanGroup(d, ev->opts, gi, &P, &G, &T);
    G.user_name = P.user_names[gi];
    if ((rc = UploadGroup(g, T, &G, s))) return bail(rc);
    if (d->num_groups == 1 && G.const0) {
      held_tables = std::move(T);
      have_held_tables = true;
    }
  }
  cse::PlanProgram(d, d->num_groups == 1 ? &ev->groups[0] : nullptr, &P,
                   have_held_tables ? &held_tables : nullptr);
  held_tables = cse::GroupTables{};
  ev->res_covered = P.res_covered;
  ev->jac_covered = P.jac_covered;
  ev->bytes_res = P.bytes_res;
  ev->bytes_jac = P.bytes_jac;
  ev->total_wg = P.total_wg;
  ev->any_general = P.any_general;
  ev->plus_supported = P.plus_supported;
  ev->plus_runs_host = std::move(P.plus_runs);
  ev->plus_quat_host = std::move(P.plus_quat);
  static_cast<cse::SchurPlan&>(ev->schur) = P.schur;
  // cse_cgnr_init's block table, as runs (a pass over the parameter blocks and
  // a few bytes; the first JACOBI init expands and uploads it).
  if (ev->has_layout) cse::PlanCgnrBlocks(d, &ev->cgnr.plan);

  // Program-level device state.
  if ((rc = ev->schur.chunk_begin.upload(P.schur_chunk_begin.data(), P.schur_chunk_begin.size(), s)))
    return bail(rc);
  if ((rc = ev->schur.big.upload(P.schur_big.data(), P.schur_big.size(), s))) return bail(rc);
  if (ev->schur.held) {
    auto& S = ev->schur;
    if ((rc = S.chunk_held.upload(P.schur_chunk_held.data(), P.schur_chunk_held.size(), s))) return bail(rc);
    if ((rc = S.big_rank.upload(P.schur_big_rank.data(), P.schur_big_rank.size(), s))) return bail(rc);
    if ((rc = S.fcell.upload(P.schur_fcell.data(), P.schur_fcell.size(), s))) return bail(rc);
    if ((rc = S.cam_rank.upload(P.schur_cam_rank.data(), P.schur_cam_rank.size(), s))) return bail(rc);
  }
  if ((rc = ev->cstate.upload(d->constant_state, (size_t)d->num_constant_parameters, s))) return bail(rc);
  if ((rc = ev->plus_jac.upload(d->plus_jacobians, (size_t)d->num_plus_jacobian_values, s))) return bail(rc);
  if (ev->any_general) {
    if ((rc = ev->pbs.upload(P.pbs.data(), P.pbs.size(), s))) return bail(rc);
    if ((rc = ev->res_layout.upload(d->residual_layout, (size_t)d->num_residual_blocks, s))) return bail(rc);
    if (ev->has_layout) {
      if ((rc = ev->jac_layout.upload(d->jacobian_per_residual_layout, (size_t)d->num_residual_blocks, s)))
        return bail(rc);
      if ((rc = ev->jac_offsets.upload(d->jacobian_per_residual_offsets,
                                       (size_t)d->num_jacobian_per_residual_offsets, s)))
        return bail(rc);
    }
  }
  if ((rc = ev->partials.alloc(std::max<int64_t>(ev->total_wg, 1)))) return bail(rc);
  // Slots of groups that launch nothing (empty groups) must read as zero.
  if (hipMemsetAsync(ev->partials.p, 0, ev->partials.n * sizeof(double), s) != hipSuccess)
    return bail(Fail(CSE_ERR_HIP, "hipMemsetAsync failed"));
  if ((rc = ev->partials2.alloc(kPartialBlocks))) return bail(rc);
  // [0] running flag, [1] last status, [2] ReduceFinalizeKernel's counter
  if ((rc = ev->status.alloc(3))) return bail(rc);
  if (hipMemsetAsync(ev->status.p, 0, 3 * sizeof(int), s) != hipSuccess)
    return bail(Fail(CSE_ERR_HIP, "memset failed"));
  if (hipHostMalloc(&ev->status_host, sizeof(int)) != hipSuccess)
    return bail(Fail(CSE_ERR_HIP, "hipHostMalloc failed"));
  // The copies read P's tables: wait before P goes out of scope.
  if (hipStreamSynchronize(s) != hipSuccess) return bail(Fail(CSE_ERR_HIP, "upload failed"));
  *out = ev;
  return CSE_OK;
}

int cse_evaluate_device_ex(cse_evaluator* ev, const double* d_state, double* d_cost,
                           double* d_residuals, double* d_gradient, double* d_jacobian_values,
                           uint32_t flags) {
  if (!ev || !d_cost) return Fail(CSE_ERR_INVALID, "null evaluator or cost");
  CSE_SINGLE_DEVICE(ev, "cse_evaluate_device");
  if (flags & ~(uint32_t)CSE_EVAL_SAME_POINT) return Fail(CSE_ERR_INVALID, "unknown evaluate flags");
  if (ev->num_parameters > 0 && !d_state) return Fail(CSE_ERR_INVALID, "null state");
  if (hipSetDevice(ev->device) != hipSuccess) return Fail(CSE_ERR_HIP, "hipSetDevice failed");
  ev->host_state_current = false;
  return Enqueue(ev, d_state, d_cost, d_residuals, d_gradient, d_jacobian_values,
                 (flags & CSE_EVAL_SAME_POINT) != 0);
}

int cse_evaluate_device(cse_evaluator* ev, const double* d_state, double* d_cost,
                        double* d_residuals, double* d_gradient, double* d_jacobian_values) {
  return cse_evaluate_device_ex(ev, d_state, d_cost, d_residuals, d_gradient, d_jacobian_values, 0);
}

int cse_wait(cse_evaluator* ev) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  if (ev->multi) return CSE_OK;  // cse_evaluate on it is synchronous
  CSE_HIP(hipMemcpyAsync(ev->status_host, ev->status.p + 1, sizeof(int), hipMemcpyDeviceToHost,
                         ev->stream));
  CSE_HIP(hipStreamSynchronize(ev->stream));
  if (ev->opts.profile) {
    int rc = FoldTiming(ev);
    if (rc) return rc;
  }
  return *ev->status_host ? CSE_EVALUATION_FAILED : CSE_OK;
}

int cse_evaluate_ex(cse_evaluator* ev, const double* state, double* cost, double* residuals,
                    double* gradient, double* jacobian_values, uint32_t flags) {
  if (!ev || !cost) return Fail(CSE_ERR_INVALID, "null evaluator or cost");
  if (flags & ~(uint32_t)CSE_EVAL_SAME_POINT) return Fail(CSE_ERR_INVALID, "unknown evaluate flags");
  const bool same_point = (flags & CSE_EVAL_SAME_POINT) != 0;
  if (ev->multi) {
    if (!state) return Fail(CSE_ERR_INVALID, "null state");
    return MultiEvaluate(ev->multi, state, cost, residuals, gradient, jacobian_values, same_point);
  }
  if (ev->num_parameters > 0 && !state) return Fail(CSE_ERR_INVALID, "null state");
  CSE_HIP(hipSetDevice(ev->device));
  int rc;
  if (!ev->h_state.p && (rc = ev->h_state.alloc(std::max<int64_t>(ev->num_parameters, 1)))) return rc;
  if (!ev->h_cost.p && (rc = ev->h_cost.alloc(1))) return rc;
  if (residuals && !ev->h_res.p && (rc = ev->h_res.alloc(std::max<int64_t>(ev->num_residuals, 1)))) return rc;
  if (gradient && !ev->h_grad.p && (rc = ev->h_grad.alloc(std::max<int64_t>(ev->num_effective, 1)))) return rc;
  if (jacobian_values && !ev->h_jac.p &&
      (rc = ev->h_jac.alloc(std::max<int64_t>(ev->num_jacobian_values, 1))))
    return rc;
  // At the same point the state uploaded for the previous host-pointer
  // evaluation is still in h_state (Evaluator::EvaluateOptions::
  // new_evaluation_point == false, trust_region_minimizer.cc:826).
  if (ev->num_parameters > 0 && !(same_point && ev->host_state_current)) {
    ev->host_state_current = false;
    CSE_HIP(hipMemcpyAsync(ev->h_state.p, state, ev->num_parameters * sizeof(double),
                           hipMemcpyHostToDevice, ev->stream));
  }
  rc = Enqueue(ev, ev->h_state.p, ev->h_cost.p, residuals ? ev->h_res.p : nullptr,
               gradient ? ev->h_grad.p : nullptr, jacobian_values ? ev->h_jac.p : nullptr, same_point);
  if (rc) return rc;
  ev->host_state_current = true;
  rc = cse_wait(ev);
  if (rc < 0) return rc;
  if (rc == CSE_EVALUATION_FAILED) return rc;
  CSE_HIP(hipMemcpy(cost, ev->h_cost.p, sizeof(double), hipMemcpyDeviceToHost));
  if (residuals && ev->num_residuals > 0)
    CSE_HIP(hipMemcpy(residuals, ev->h_res.p, ev->num_residuals * sizeof(double), hipMemcpyDeviceToHost));
  if (gradient && ev->num_effective > 0)
    CSE_HIP(hipMemcpy(gradient, ev->h_grad.p, ev->num_effective * sizeof(double), hipMemcpyDeviceToHost));
  if (jacobian_values && ev->num_jacobian_values > 0)
    CSE_HIP(hipMemcpy(jacobian_values, ev->h_jac.p, ev->num_jacobian_values * sizeof(double),
                      hipMemcpyDeviceToHost));
  return CSE_OK;
}

int cse_evaluate(cse_evaluator* ev, const double* state, double* cost, double* residuals,
                 double* gradient, double* jacobian_values) {
  return cse_evaluate_ex(ev, state, cost, residuals, gradient, jacobian_values, 0);
}

int cse_set_plus_jacobians(cse_evaluator* ev, const double* plus_jacobians) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  if (ev->multi) return MultiSetPlusJacobians(ev->multi, plus_jacobians);
  if (ev->num_plus_jacobian_values == 0) return CSE_OK;
  if (!plus_jacobians) return Fail(CSE_ERR_INVALID, "null plus_jacobians");
  CSE_HIP(hipSetDevice(ev->device));
  CSE_HIP(hipMemcpyAsync(ev->plus_jac.p, plus_jacobians, ev->num_plus_jacobian_values * sizeof(double),
                         hipMemcpyHostToDevice, ev->stream));
  CSE_HIP(hipStreamSynchronize(ev->stream));
  return CSE_OK;
}

int cse_plus_device(cse_evaluator* ev, const double* d_state, const double* d_delta,
                    double* d_state_plus_delta) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_plus_device");
  if (!ev->plus_supported)
    return Fail(CSE_ERR_UNSUPPORTED,
                "Plus on device: an active parameter block has an explicit plus-Jacobian manifold");
  if (ev->plus_runs_host.empty() && ev->plus_quat_host.empty()) return CSE_OK;
  if (!d_state || !d_delta || !d_state_plus_delta) return Fail(CSE_ERR_INVALID, "null pointer");
  CSE_HIP(hipSetDevice(ev->device));
  if (!ev->plus_runs_host.empty()) {
    if (!ev->plus_runs.p) {
      int rc = ev->plus_runs.upload(ev->plus_runs_host.data(), ev->plus_runs_host.size(), ev->stream);
      if (rc) return rc;
    }
    const int64_t n = ev->num_parameters;
    const unsigned grid = (unsigned)std::max<int64_t>(
        1, std::min<int64_t>((n + cse::kBlockThreads - 1) / cse::kBlockThreads, 8LL * ev->num_cus));
    hipLaunchKernelGGL(cse::PlusKernel, dim3(grid), dim3(cse::kBlockThreads), 0, ev->stream, d_state,
                       d_delta, d_state_plus_delta, ev->plus_runs.p, (int)ev->plus_runs_host.size());
  }
  if (!ev->plus_quat_host.empty()) {
    if (!ev->plus_quat.p) {
      int rc = ev->plus_quat.upload(ev->plus_quat_host.data(), ev->plus_quat_host.size(), ev->stream);
      if (rc) return rc;
    }
    const int64_t nq = (int64_t)ev->plus_quat_host.size();
    hipLaunchKernelGGL(cse::QuaternionPlusKernel,
                       dim3((unsigned)((nq + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                       dim3(cse::kBlockThreads), 0, ev->stream, d_state, d_delta, d_state_plus_delta,
                       ev->plus_quat.p, nq);
  }
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

int cse_plus(cse_evaluator* ev, const double* state, const double* delta,
             double* state_plus_delta) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  if (ev->multi) return MultiPlus(ev->multi, state, delta, state_plus_delta);
  if (!ev->plus_supported)
    return Fail(CSE_ERR_UNSUPPORTED,
                "Plus on device: an active parameter block has an explicit plus-Jacobian manifold");
  if (ev->num_parameters == 0) return CSE_OK;
  if (!state || !delta || !state_plus_delta) return Fail(CSE_ERR_INVALID, "null pointer");
  CSE_HIP(hipSetDevice(ev->device));
  int rc;
  if ((rc = ev->h_state.ensure(ev->num_parameters))) return rc;
  if ((rc = ev->h_delta.ensure(std::max<int64_t>(1, ev->num_effective)))) return rc;
  if ((rc = ev->h_plus.ensure(ev->num_parameters))) return rc;
  CSE_HIP(hipMemcpyAsync(ev->h_state.p, state, ev->num_parameters * sizeof(double),
                         hipMemcpyHostToDevice, ev->stream));
  CSE_HIP(hipMemcpyAsync(ev->h_delta.p, delta, ev->num_effective * sizeof(double),
                         hipMemcpyHostToDevice, ev->stream));
  double* out = ev->h_plus.p;
  if ((rc = cse_plus_device(ev, ev->h_state.p, ev->h_delta.p, out))) return rc;
  CSE_HIP(hipMemcpyAsync(state_plus_delta, out, ev->num_parameters * sizeof(double),
                         hipMemcpyDeviceToHost, ev->stream));
  CSE_HIP(hipStreamSynchronize(ev->stream));
  return CSE_OK;
}

void cse_destroy(cse_evaluator* ev) {
  if (!ev) return;
  if (ev->multi) {
    MultiDestroy(ev->multi);
    delete ev;
    return;
  }
  (void)hipSetDevice(ev->device);
  if (ev->stream) (void)hipStreamSynchronize(ev->stream);
  if (ev->status_host) (void)hipHostFree(ev->status_host);
  if (ev->cg.state_host) (void)hipHostFree(ev->cg.state_host);
  if (ev->spse.state_host) (void)hipHostFree(ev->spse.state_host);
  for (auto& pr : ev->pending) ev->pool.push_back(pr);
  for (auto& pr : ev->pool) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  if (ev->own_stream && ev->stream) (void)hipStreamDestroy(ev->stream);
  delete ev;  // every DevBuf (groups, plans, tables, scratch) frees itself
}

int cse_create_multi(const cse_problem_desc* d, const cse_options* options, const int32_t* devices,
                     int32_t num_devices, cse_evaluator** out) {
  if (!out) return Fail(CSE_ERR_INVALID, "null out");
  *out = nullptr;
  int rc = cse::Validate(d);
  if (rc) return rc;
  if (options && (options->gradient_mode < 0 || options->gradient_mode > 3))
    return Fail(CSE_ERR_INVALID, "gradient_mode " + std::to_string(options->gradient_mode) +
                                     " is not one of 0..3");
  cse_evaluator* ev = new (std::nothrow) cse_evaluator();
  if (!ev) return Fail(CSE_ERR_OOM, "host allocation failed");
  if ((rc = MultiCreate(d, options, devices, num_devices, &ev->multi))) {
    delete ev;
    return rc;
  }
  ev->device = devices[0];
  *out = ev;
  return CSE_OK;
}

int cse_shard_info(cse_evaluator* ev, int32_t* num_shards, int64_t* first_block, int32_t* devices) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  if (ev->multi) return MultiShardInfo(ev->multi, num_shards, first_block, devices);
  if (num_shards) *num_shards = 1;
  if (first_block) {
    first_block[0] = 0;
    first_block[1] = ev->num_residual_blocks;
  }
  if (devices) devices[0] = ev->device;
  return CSE_OK;
}

int cse_shard_transfer_bytes(cse_evaluator* ev, int64_t* state_h2d_bytes, int64_t* strips_d2h_bytes) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  if (ev->multi) return MultiTransferBytes(ev->multi, state_h2d_bytes, strips_d2h_bytes);
  if (state_h2d_bytes) state_h2d_bytes[0] = ev->num_parameters * (int64_t)sizeof(double);
  if (strips_d2h_bytes)
    strips_d2h_bytes[0] = (ev->num_residuals + ev->num_jacobian_values) * (int64_t)sizeof(double);
  return CSE_OK;
}

int cse_host_register(void* p, size_t bytes) { return CseHostRegister(p, bytes); }

int cse_host_unregister(void* p) { return CseHostUnregister(p); }

// Registration compares whole tables bytewise: no padding inside.
static_assert(offsetof(cse_functor_ops, kernel_args_tag) == 80 && sizeof(cse_functor_ops) == 224,
              "cse_functor_ops layout");

int cse_register_functor(const cse_functor_ops* ops, int32_t* kind) {
  if (!ops || !kind) return Fail(CSE_ERR_INVALID, "null functor table or kind");
  const std::string name = ops->name ? ops->name : "(unnamed)";
  if (ops->abi_version != CSE_ABI_VERSION)
    return Fail(CSE_ERR_INVALID, "functor " + name + ": built against ABI " +
                                     std::to_string(ops->abi_version) + ", the library is " +
                                     std::to_string(CSE_ABI_VERSION));
  if (ops->kernel_args_size != (int32_t)sizeof(cse::GroupArgs) ||
      ops->gradient_args_size != (int32_t)sizeof(cse::GradArgs) ||
      ops->kernel_args_tag != cse::kGroupArgsTag)
    return Fail(CSE_ERR_INVALID, "functor " + name +
                                     ": kernel argument layout differs from the library's (build "
                                     "the functor against the same ceres-solver-cuda_amd headers)");
  const bool fused = ops->fused_points[0] || ops->fused_points[1] || ops->camera_gradient;
  if (fused && (!ops->fused_points[0] || !ops->fused_points[1] || !ops->camera_gradient ||
                ops->camera_gradient_args_size != (int32_t)sizeof(cse::CamGradArgs)))
    return Fail(CSE_ERR_INVALID, "functor " + name +
                                     ": the fused gradient's launches come as all three, with the "
                                     "library's camera-gradient argument size");
  const int nb = ops->num_parameter_blocks;
  if (ops->num_residuals < 1 || nb < 1 || nb > CSE_MAX_PARAMETER_BLOCKS || ops->data_size < 1)
    return Fail(CSE_ERR_INVALID, "functor " + name + ": bad shape");
  for (int j = 0; j < nb; ++j)
    if (ops->parameter_block_sizes[j] < 1)
      return Fail(CSE_ERR_INVALID, "functor " + name + ": parameter block size < 1");
  if (ops->loss_kind < CSE_LOSS_TRIVIAL || ops->loss_kind > CSE_LOSS_USER ||
      (ops->loss_kind == CSE_LOSS_USER &&
       (ops->loss_size < 1 || ops->loss_size > CSE_USER_LOSS_BYTES)))
    return Fail(CSE_ERR_INVALID, "functor " + name + ": bad loss kind or size");
  if (!ops->table[0] || !ops->table[1])
    return Fail(CSE_ERR_INVALID, "functor " + name + ": the general kernels are required");
  bool any_affine = false;
  for (int c = 0; c < 2; ++c)
    for (int j = 0; j < 2; ++j)
      for (int d = 0; d < 2; ++d) any_affine = any_affine || ops->affine[c][j][d];
  if (any_affine && (!cse::UserAffine(ops) || nb > 2 || ops->num_residuals > 3))
    return Fail(CSE_ERR_INVALID, "functor " + name + ": affine kernels must come as all eight, "
                                                     "for at most two blocks and three residuals");
  if (fused && (!any_affine || nb != 2 || ops->parameter_block_sizes[1] != 3 ||
                ops->parameter_block_sizes[0] > 16))
    return Fail(CSE_ERR_INVALID, "functor " + name + ": the fused gradient is for affine kinds of two "
                                                     "blocks, the second of 3 parameters");
  std::lock_guard<std::mutex> lock(g_user_mu);
  for (size_t i = 0; i < g_user_kinds.size(); ++i) {
    const UserKindEntry& e = *g_user_kinds[i];
    cse_functor_ops a = e.ops, b = *ops;
    a.name = b.name = nullptr;
    if (e.name == name && std::memcmp(&a, &b, sizeof(a)) == 0) {
      *kind = CSE_FUNCTOR_USER_FIRST + (int32_t)i;
      return CSE_OK;
    }
  }
  UserKindEntry* e = new (std::nothrow) UserKindEntry{*ops, name};
  if (!e) return Fail(CSE_ERR_OOM, "host allocation failed");
  e->ops.name = nullptr;  // the copy in e->name serves
  g_user_kinds.push_back(e);
  *kind = CSE_FUNCTOR_USER_FIRST + (int32_t)(g_user_kinds.size() - 1);
  return CSE_OK;
}

int cse_functor_shape(int32_t kind, int32_t* num_residuals, int32_t* num_parameter_blocks,
                      int32_t* parameter_block_sizes, int32_t* data_size) {
  KindShape k;
  if (!ShapeOf(kind, &k)) return Fail(CSE_ERR_UNSUPPORTED, "unknown functor kind " + std::to_string(kind));
  if (num_residuals) *num_residuals = k.nr;
  if (num_parameter_blocks) *num_parameter_blocks = k.nb;
  if (parameter_block_sizes)
    for (int j = 0; j < k.nb; ++j) parameter_block_sizes[j] = k.sz[j];
  if (data_size) *data_size = k.data;
  return CSE_OK;
}

int cse_get_info(cse_evaluator* ev, cse_info* info) {
  if (!ev || !info) return Fail(CSE_ERR_INVALID, "null argument");
  if (ev->multi) return MultiInfo(ev->multi, info);
  std::memset(info, 0, sizeof(*info));
  info->num_residual_blocks = ev->num_residual_blocks;
  info->num_residuals = ev->num_residuals;
  info->num_parameters = ev->num_parameters;
  info->num_effective_parameters = ev->num_effective;
  info->num_jacobian_values = ev->num_jacobian_values;
  info->num_groups = (int32_t)ev->groups.size();
  for (auto& G : ev->groups) {
    info->num_affine_groups += G.affine ? 1 : 0;
    info->num_fused_gradient_groups += FusedGradMode(ev, G) ? 1 : 0;
  }
  info->device = ev->device;
  info->bytes_jacobian_eval = ev->bytes_jac;
  info->bytes_residual_eval = ev->bytes_res;
  return CSE_OK;
}

int cse_kernel_stats(cse_evaluator* ev, double* last_ms, double* total_ms, int64_t* launches) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  if (ev->multi) return MultiKernelStats(ev->multi, last_ms, total_ms, launches);
  if (!ev->opts.profile) return Fail(CSE_ERR_INVALID, "evaluator created without options.profile");
  int rc = FoldTiming(ev);
  if (rc) return rc;
  if (last_ms) *last_ms = ev->last_ms;
  if (total_ms) *total_ms = ev->total_ms;
  if (launches) *launches = ev->launches;
  return CSE_OK;
}

int cse_reset_kernel_stats(cse_evaluator* ev) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  if (ev->multi) return MultiResetKernelStats(ev->multi);
  int rc = FoldTiming(ev);
  if (rc) return rc;
  ev->last_ms = ev->total_ms = 0.0;
  ev->launches = 0;
  return CSE_OK;
}

}  // extern "C"
