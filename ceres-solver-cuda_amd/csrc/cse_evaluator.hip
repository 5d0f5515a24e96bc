// cse_evaluator.hip -- the C ABI (include/cse.h) over the gfx950 kernels.
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
#include "group_store_kernel.hpp"
#include "jet_kernels.h"
#include "kernel_pickers.hpp"
#include "launch.hpp"
#include "multi_device.h"
#include "per_block_loss_kernels.h"
#include "plan.hpp"
#include "schur_kernels.hpp"
#include "schur_complement_kernels.hpp"
#include "cg_kernels.h"

namespace cse {
std::string& LastError();  // layout.cpp: one per thread (cse_last_error reads it here)
}  // namespace cse

namespace {

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

int Fail(int code, const std::string& msg) { return CseFail(code, msg); }

// Entry points whose arguments are device pointers of one device.
#define CSE_SINGLE_DEVICE(ev, what)                                                         \
  do {                                                                                     \
    if ((ev) && (ev)->multi)                                                               \
      return Fail(CSE_ERR_UNSUPPORTED, std::string(what) +                                 \
                                           ": not available on a multi-device evaluator " \
                                           "(cse_create_multi): its outputs span devices"); \
  } while (0)

#define CSE_HIP(call)                                                              \
  do {                                                                             \
    hipError_t e_ = (call);                                                        \
    if (e_ != hipSuccess)                                                          \
      return Fail(CSE_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)


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

// Device buffer, move-only, freed on destruction.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, n = o.n;
      o.p = nullptr, o.n = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  int alloc(size_t count) {
    release();
    if (count == 0) return CSE_OK;
    if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) {
      p = nullptr;
      return Fail(CSE_ERR_OOM, "hipMalloc of " + std::to_string(count * sizeof(T)) + " bytes failed");
    }
    n = count;
    return CSE_OK;
  }
  // Allocate on first use / grow; keeps the buffer when large enough.
  int ensure(size_t count) {
    if (p && n >= count) return CSE_OK;
    return alloc(count);
  }
  int upload(const T* h, size_t count, hipStream_t s) {
    int rc = alloc(count);
    if (rc) return rc;
    if (count && hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s) != hipSuccess)
      return Fail(CSE_ERR_HIP, "hipMemcpyAsync H2D failed");
    return CSE_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

// A residual group on the device: the planner's decisions (cse::GroupPlan,
// plan.hpp) and the buffers its tables were uploaded to.
struct Group : cse::GroupPlan {
  std::string user_name;
  DevBuf<int32_t> ids;
  DevBuf<double> data;       // [n][D]: the functor constants alone
  DevBuf<double> loss_data;  // [n][2] (a, scale) records: per-block loss parameters only
  DevBuf<int64_t> gindex;  // only when not contiguous
  DevBuf<double> packed0;  // repacked slot-0 table (repack0)
  // Gradient post-pass plan per slot (cse::GradPlanInfo, cse::GradTables).
  struct GradPlan : cse::GradPlanInfo {
    DevBuf<int32_t> perm;  // empty = identity
    DevBuf<int64_t> off;
    DevBuf<int64_t> chunk_begin, chunk_off;
    DevBuf<int32_t> chunk_pb;
    DevBuf<int32_t> chunk_order;
    DevBuf<double> chunk_partial;
  } grad[2];
  // const0 (cse::GroupTables): the active bits, repack sources, delta
  // offsets and per-chunk first cells.
  DevBuf<uint32_t> act0;
  DevBuf<int64_t> src0, fbase, delta0;
  // Held-camera sectors (HeldSectorFixupKernel): each chunk's two side
  // slots and the previous chunk with F cells (BSM) or row blocks (CRS).
  DevBuf<double> side;
  DevBuf<int32_t> prev_seg;
  // Fused gradient (cse::FusedGrad): the slot-1 boundary entries and slot-0
  // contributions of eligible groups (allocated on first use).
  DevBuf<double> gside, gcontrib;
  // Slot-0-sorted functor data and slot-1 ids (CameraGradientKernel; built
  // on first use).
  DevBuf<double> sdata;
  DevBuf<int32_t> sid1;
  bool sorted_ready = false;
  // Table policy: each 64-block chunk's store runs.
  DevBuf<int64_t> runs;
};


// Waves per workgroup of the CGNR and Schur chunk kernels (one chunk per
// wave either way); one wave per workgroup, as the Jacobian kernels are
// launched, measured slower: S x 2.363 -> 2.410 ms, CGNR 2.596 -> 2.614 ms
// (profiles/round3/w1c).
constexpr int kOperatorWavesPerWg = cse::kWavesPerBlock;

// Cost reduction: above this many per-wave partials, kPartialBlocks
// workgroups sum slices and the last of them finalises
// (ReduceFinalizeKernel); below, one FinalizeKernel.
constexpr int64_t kPartialsTwoPass = 4096;
constexpr int kPartialBlocks = 128;

using cse::FusedKind;
bool SnavelyShaped(const Group& G) { return cse::SnavelyShaped(G.shape); }
bool UserFused(const Group& G) { return cse::UserFused(G.user, G.shape); }


}  // namespace

struct cse_evaluator {
  // A multi-device evaluator (cse_create_multi) is a shell around CseMulti;
  // everything below is unused then.
  CseMulti* multi = nullptr;
  int device = 0;
  int num_cus = 256;  // compute units (grid caps of the Plus kernels)
  hipStream_t stream = nullptr;
  bool own_stream = false;
  cse_options opts{};
  int64_t num_parameter_blocks = 0, num_parameters = 0, num_effective = 0, num_constant = 0;
  int64_t num_residual_blocks = 0, num_residuals = 0, num_jacobian_values = 0;
  int64_t num_plus_jacobian_values = 0;
  bool has_layout = false;
  bool jac_covered = true;  // every Jacobian value is written by some block
  bool res_covered = true;
  int64_t bytes_jac = 0, bytes_res = 0;
  std::vector<Group> groups;
  int64_t total_wg = 0;
  bool any_general = false;
  DevBuf<cse::PbDev> pbs;
  DevBuf<double> cstate, plus_jac;
  DevBuf<int64_t> res_layout, jac_layout, jac_offsets;
  DevBuf<double> partials, partials2;
  // Program::Plus (cse_plus_device): runs of manifold-free state entries.
  bool plus_supported = true;
  std::vector<cse::PlusRun> plus_runs_host;
  DevBuf<cse::PlusRun> plus_runs;
  // CSE_MANIFOLD_QUATERNION_EUCLIDEAN blocks: Plus one block per thread.
  std::vector<cse::QuatPlusBlock> plus_quat_host;
  DevBuf<cse::QuatPlusBlock> plus_quat;
  DevBuf<double> h_delta, h_plus;
  DevBuf<int> status;  // [0] running flag, [1] last status, [2] reduce counter
  // Host-path buffers (allocated on first use).
  DevBuf<double> h_state, h_cost, h_res, h_jac, h_grad;
  DevBuf<double> cg_z;  // cse_cgnr_multiply's z = J x when it cannot fuse
  int* status_host = nullptr;  // pinned
  // Evaluate at the same point (CSE_EVAL_SAME_POINT): the packed slot-0
  // tables hold the state of the last evaluation queued without error, and
  // h_state the last host state uploaded (cleared by a device-pointer call).
  bool point_current = false;
  bool host_state_current = false;
  // Profiling: one (start, stop) event pair per evaluation around its
  // group kernels, folded lazily so timing never stalls the launch queue.
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending, pool;
  double last_ms = 0.0, total_ms = 0.0;
  int64_t launches = 0;
  // The implicit Schur complement (cse_schur_*): structure found at create
  // time, values and vectors bound by cse_schur_init.
  struct Schur : cse::SchurPlan {
    DevBuf<int64_t> chunk_begin, big;
    DevBuf<double> ete_inv, precond, partial, ub;
    bool ready = false;
    int preconditioner = CSE_SCHUR_IDENTITY;
    const double *jac = nullptr, *D = nullptr, *b = nullptr;
    // The explicit complement's pair plan (cse::PlanSchurPairs): counted on
    // the first plan query, built and uploaded on the first
    // cse_schur_complement; structure only, so it outlives every init.
    struct Pairs : cse::SchurPairCounts {
      bool counted = false, uploaded = false;
      DevBuf<int32_t> block_row, block_col, chunk_block, pairs;
      DevBuf<int64_t> pair_begin, chunk_off;
      DevBuf<double> partial;
    } pairs;
    // The block-sparse complement's structure (cse::PlanSchurSparse), cached
    // the same way; row_begin and block_col stay on the host too, for
    // cse_schur_complement_sparse_structure.
    struct Sparse : cse::SchurSparseCounts {
      bool counted = false, uploaded = false;
      int64_t num_finish = 0;
      std::vector<int64_t> h_row_begin;
      std::vector<int32_t> h_block_col;
      DevBuf<int64_t> row_begin, col_begin;
      DevBuf<int32_t> block_col, plan_block, sparse_of_plan, finish, col_block;
      DevBuf<double> contrib;  // [num_blocks][9]: the product's column contributions
    } sparse;
  } schur;
  // cse_schur_solve's scratch (cg_kernels.hpp): the four vectors p, r, z, tmp
  // in one buffer and the state, allocated by the first solve.
  struct Cg {
    DevBuf<double> vectors;
    DevBuf<cse::CgState> state;
    cse::CgState* state_host = nullptr;  // pinned
  } cg;
};

namespace {

// The post-pass form of a plan (cse::GradForm) and its chunk table.
int GradFormOf(const cse::GradArgs& ga, const Group::GradPlan& P) {
  if (ga.perm == nullptr) return cse::kGradRange;  // identity order: contiguous ranges (points)
  return P.wave ? cse::kGradChunked : cse::kGradPerBlock;  // many blocks per parameter block: chunks
}
cse::GradChunks GradChunksOf(const Group::GradPlan& P) {
  return cse::GradChunks{P.chunk_begin.p, P.chunk_off.p, P.chunk_partial.p, P.nchunks};
}

// The post-pass kernels of the built-in shapes (the planner's GradSupported
// names the same ones); a user kind brings its own (cse_functor_ops.gradient).
bool LaunchGradPass(int nr, int size, const cse::GradArgs& ga, const Group::GradPlan& P,
                    hipStream_t s, const cse_functor_ops* user = nullptr, int slot = 0) {
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

// After a fused kernel (the evaluator's FusedGrad or CgnrMultiplyKernel):
// add the slot-1 boundary entries and the slot-0 contributions, per
// parameter block in a fixed order, into out (delta offsets).
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
  const cse::GradChunks ch{P.chunk_begin.p, P.chunk_off.p, P.chunk_partial.p, P.nchunks};
  if (P.nchunks > 0)
    hipLaunchKernelGGL((cse::GradientContribKernel<9, 10>),
                       dim3((unsigned)((P.nchunks + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
                       dim3(cse::kBlockThreads), 0, s, G.gcontrib.p, P.perm.p, ch,
                       P.chunk_order.p);
  hipLaunchKernelGGL((cse::GradientChunkReduceKernel<9>),
                     dim3((unsigned)((ga.count + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                     dim3(cse::kBlockThreads), 0, s, ga, ch);
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

// gradient_mode 0: the slot-1 boundary entries as above, and the slot-0
// sums by re-evaluation in camera order (CameraGradientKernel), then
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
        const Group::GradPlan& P = G.grad[j];
        cse::GradArgs ga{};
        ga.jac = d_jac;
        for (int r = 0; r < G.shape.nr && r < 3; ++r) ga.jrow[r] = G.jac_base[j][r];
        ga.jstride = G.jac_stride[j];
        ga.res = d_res;
        ga.res_base = G.res_base;
        ga.perm = P.perm.p;
        ga.off = P.off.p;
        ga.count = P.count;
        ga.lo = P.lo;
        ga.grad = d_grad;
        ga.delta_base = G.delta_base[j];
        if (!LaunchGradPass(G.shape.nr, sizes[j], ga, P, ev->stream, G.user, j))
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
  for (int gi = 0; gi < d->num_groups; ++gi) {
    Group& G = ev->groups[gi];
    const cse_residual_group& g = d->groups[gi];
    cse::GroupTables T;
    cse::PlanGroup(d, ev->opts, gi, &P, &G, &T);
    G.user_name = P.user_names[gi];
    if ((rc = UploadGroup(g, T, &G, s))) return bail(rc);
  }
  cse::PlanProgram(d, d->num_groups == 1 ? &ev->groups[0] : nullptr, &P);
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

  // Program-level device state.
  if ((rc = ev->schur.chunk_begin.upload(P.schur_chunk_begin.data(), P.schur_chunk_begin.size(), s)))
    return bail(rc);
  if ((rc = ev->schur.big.upload(P.schur_big.data(), P.schur_big.size(), s))) return bail(rc);
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

extern "C++" {
namespace {

bool DispatchMultiply(int kind, const cse::GroupArgs& a, bool affine, bool left, const double* x,
                      double* y, hipStream_t s) {
  const int which = affine && !left ? 0 : left ? 2 : 1;
  return VisitKind(kind, [&](auto kd) { cse::LaunchMultiplyKernel<decltype(kd)>(a, which, x, y, s); });
}

int JacobianMultiply(cse_evaluator* ev, const double* J, const double* x, double* y, bool left) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_jacobian_multiply");
  if (!ev->has_layout)
    return Fail(CSE_ERR_INVALID, "the descriptor had no Jacobian layout");
  if (!J || !x || !y) return Fail(CSE_ERR_INVALID, "null pointer");
  CSE_HIP(hipSetDevice(ev->device));
  for (auto& G : ev->groups) {
    if (G.n == 0) continue;
    // Groups with constant slot-0 blocks take the table kernels (their F
    // cells are not at affine offsets).
    const bool affine = G.affine && !G.const0;
    bool plans = affine;
    for (int j = 0; j < G.shape.nb; ++j) plans = plans && G.grad[j].ready;
    // MakeArgs wants non-const outputs; the kernels only read a.jacobian.
    cse::GroupArgs a = MakeArgs(ev, G, nullptr, nullptr, const_cast<double*>(J), nullptr);
    if (left && plans) {
      const int sizes[2] = {G.shape.s0, G.shape.s1};
      for (int j = 0; j < G.shape.nb; ++j) {
        const Group::GradPlan& P = G.grad[j];
        cse::GradArgs ga{};
        ga.jac = J;
        for (int r = 0; r < G.shape.nr && r < 3; ++r) ga.jrow[r] = G.jac_base[j][r];
        ga.jstride = G.jac_stride[j];
        ga.res = x;
        ga.res_base = G.res_base;
        ga.perm = P.perm.p;
        ga.off = P.off.p;
        ga.count = P.count;
        ga.lo = P.lo;
        ga.grad = y;
        ga.delta_base = G.delta_base[j];
        if (!LaunchGradPass(G.shape.nr, sizes[j], ga, P, ev->stream, G.user, j))
          return Fail(CSE_ERR_UNSUPPORTED, "no J^T x pass for this shape");
      }
    } else {
      if (!G.affine && !ev->any_general)
        return Fail(CSE_ERR_UNSUPPORTED, "table-path tables were not uploaded");
      if (G.user) {
        if (!G.user->multiply)
          return Fail(CSE_ERR_UNSUPPORTED, "user functor kind " + G.user_name + " has no multiply kernel");
        G.user->multiply(&a, affine && !left ? 0 : left ? 2 : 1, x, y, ev->stream);
      } else if (!DispatchMultiply(G.kind, a, affine, left, x, y, ev->stream))
        return Fail(CSE_ERR_UNSUPPORTED, "no multiply kernel for functor kind " +
                                             std::to_string(G.kind));
    }
    CSE_HIP(hipGetLastError());
  }
  return CSE_OK;
}

}  // namespace
}  // extern "C++"

int cse_jacobian_right_multiply(cse_evaluator* ev, const double* d_jacobian_values,
                                const double* d_x, double* d_y) {
  return JacobianMultiply(ev, d_jacobian_values, d_x, d_y, false);
}

int cse_jacobian_left_multiply(cse_evaluator* ev, const double* d_jacobian_values,
                               const double* d_x, double* d_y) {
  return JacobianMultiply(ev, d_jacobian_values, d_x, d_y, true);
}

int cse_cgnr_multiply(cse_evaluator* ev, const double* d_jacobian_values, const double* d_D,
                      const double* d_x, double* d_y) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_cgnr_multiply");
  if (!ev->has_layout) return Fail(CSE_ERR_INVALID, "the descriptor had no Jacobian layout");
  if (!d_jacobian_values || !d_x || !d_y) return Fail(CSE_ERR_INVALID, "null pointer");
  CSE_HIP(hipSetDevice(ev->device));
  hipStream_t s = ev->stream;
  if (d_D && ev->num_effective > 0)
    hipLaunchKernelGGL(cse::DtDxpyKernel,
                       dim3((unsigned)((ev->num_effective + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                       dim3(cse::kBlockThreads), 0, s, d_D, d_x, d_y, ev->num_effective);
  bool fused = true;
  for (auto& G : ev->groups) fused = fused && (G.n == 0 || (G.fuse_ok && !G.const0 && SnavelyShaped(G)));
  if (!fused) {
    // z = J x, then y += J^T z: the two products of CudaCgnrLinearOperator.
    int rc;
    if ((rc = ev->cg_z.ensure((size_t)std::max<int64_t>(ev->num_residuals, 1)))) return rc;
    CSE_HIP(hipMemsetAsync(ev->cg_z.p, 0, ev->num_residuals * sizeof(double), s));
    if ((rc = JacobianMultiply(ev, d_jacobian_values, d_x, ev->cg_z.p, false))) return rc;
    return JacobianMultiply(ev, d_jacobian_values, ev->cg_z.p, d_y, true);
  }
  for (auto& G : ev->groups) {
    if (G.n == 0) continue;
    const int64_t chunks = (G.n + cse::kWave - 1) / cse::kWave;
    int rc;
    if ((rc = G.gside.ensure((size_t)(2 * chunks * 4)))) return rc;
    if ((rc = G.gcontrib.ensure((size_t)G.n * G.slot0_stride))) return rc;
    cse::GroupArgs a = MakeArgs(ev, G, nullptr, nullptr, const_cast<double*>(d_jacobian_values),
                                nullptr);
    a.gside = G.gside.p;
    a.gcontrib = G.gcontrib.p;
    constexpr int W = kOperatorWavesPerWg;
    const dim3 grid((unsigned)((chunks + W - 1) / W));
    if (G.policy == kAffineCrs)
      hipLaunchKernelGGL((cse::CgnrMultiplyKernel<cse::SnavelyKind, true, W>), grid,
                         dim3(W * cse::kWave), 0, s, a, d_x, d_y);
    else
      hipLaunchKernelGGL((cse::CgnrMultiplyKernel<cse::SnavelyKind, false, W>), grid,
                         dim3(W * cse::kWave), 0, s, a, d_x, d_y);
    CSE_HIP(hipGetLastError());
    if ((rc = LaunchFusedGradTail(G, d_y, s))) return rc;
  }
  return CSE_OK;
}

// ---------------------------------------------------------------------------
// ITERATIVE_SCHUR on the device (schur_kernels.hpp)
// ---------------------------------------------------------------------------
extern "C++" {
namespace {

cse::SchurArgs MakeSchurArgs(cse_evaluator* ev, const double* x, double* y) {
  const Group& G = ev->groups[0];
  const auto& S = ev->schur;
  cse::SchurArgs a{};
  a.n = G.n;
  a.ids = G.ids.p;
  a.jac = S.jac;
  a.f_base = G.jac_base[0][0];
  a.e_base = G.jac_base[1][0];
  a.f_col_base = S.f_col_base;
  a.e_col_base = G.delta_base[1];
  a.e_cols = S.e_cols;
  a.D = S.D;
  a.b = S.b;
  a.b_base = G.res_base;
  a.x = x;
  a.ete_inv = S.ete_inv.p;
  a.contrib = G.gcontrib.p;
  a.y = y;
  a.chunk_begin = S.chunk_begin.p;
  a.nchunks = S.nchunks;
  a.big = S.big.p;
  a.nbig = S.nbig;
  a.status = ev->status.p + 1;  // read by cse_wait
  return a;
}

template <int kMode, bool kGrad = false>
void LaunchSchurPass(const cse::SchurArgs& a, hipStream_t s) {
  constexpr int W = kOperatorWavesPerWg;
  if (a.nchunks > 0)
    hipLaunchKernelGGL((cse::SchurChunkKernel<9, kMode, W, kGrad>), dim3((unsigned)((a.nchunks + W - 1) / W)),
                       dim3(W * cse::kWave), 0, s, a);
  if (a.nbig > 0)
    hipLaunchKernelGGL((cse::SchurBigKernel<9, kMode, kGrad>),
                       dim3((unsigned)((a.nbig + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
                       dim3(cse::kBlockThreads), 0, s, a);
}

// y (f vector) += the per-f-block sums of the contributions just written.
int SchurFTail(cse_evaluator* ev, double* y, hipStream_t s) {
  const Group& G = ev->groups[0];
  const Group::GradPlan& P = G.grad[0];
  cse::GradArgs ga{};
  ga.count = P.count;
  ga.lo = P.lo;
  ga.grad = y;
  ga.delta_base = ev->schur.f_col_base;
  const cse::GradChunks ch{P.chunk_begin.p, P.chunk_off.p, P.chunk_partial.p, P.nchunks};
  if (P.nchunks > 0)
    hipLaunchKernelGGL((cse::GradientContribKernel<9, 10>),
                       dim3((unsigned)((P.nchunks + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
                       dim3(cse::kBlockThreads), 0, s, G.gcontrib.p, P.perm.p, ch,
                       P.chunk_order.p);
  hipLaunchKernelGGL((cse::GradientChunkReduceKernel<9>),
                     dim3((unsigned)((ga.count + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                     dim3(cse::kBlockThreads), 0, s, ga, ch);
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

// The init's camera-order pass and the per-camera finish (schur_kernels.hpp).
struct SchurCameraLaunch {
  cse::SchurArgs a;
  const Group::GradPlan* P;
  cse::GradChunks ch;
  const double* D;
  int64_t d_off;  // D index of the plan's first camera's first column
  double* precond;
  int* status;
  double* rhs;   // rhs row of the plan's first camera
  double* grad;  // gradient row of the plan's first camera (null: no gradient)
};

template <int kDiag, bool kGrad>
void LaunchSchurCameraPass(const SchurCameraLaunch& L, hipStream_t s) {
  const Group::GradPlan& P = *L.P;
  if (P.nchunks > 0)
    hipLaunchKernelGGL((cse::SchurCameraPassKernel<9, kDiag, kGrad>),
                       dim3((unsigned)((P.nchunks + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
                       dim3(cse::kBlockThreads), 0, s, L.a, P.perm.p, L.ch, P.chunk_order.p);
  if (P.count > 0)
    hipLaunchKernelGGL((cse::SchurCameraFinishKernel<9, kDiag, kGrad>),
                       dim3((unsigned)((P.count + 63) / 64)), dim3(64), 0, s, L.ch, P.count, L.D,
                       L.d_off, L.precond, L.status, L.rhs, L.grad);
}

int SchurCheck(cse_evaluator* ev, bool need_ready) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_schur");
  if (!ev->schur.eligible)
    return Fail(CSE_ERR_UNSUPPORTED,
                "implicit Schur complement: needs one Snavely-shaped group (2 residuals, blocks of 9 and 3) "
                "on the affine BlockSparse path "
                "with its points (slot 1) as the leading e columns and its cameras after them");
  if (need_ready && !ev->schur.ready) return Fail(CSE_ERR_INVALID, "cse_schur_init has not run");
  CSE_HIP(hipSetDevice(ev->device));
  return CSE_OK;
}

}  // namespace
}  // extern "C++"

int cse_schur_structure(cse_evaluator* ev, int64_t* num_cols_e, int64_t* num_cols_f) {
  int rc = SchurCheck(ev, false);
  if (rc) return rc;
  if (num_cols_e) *num_cols_e = ev->schur.e_cols;
  if (num_cols_f) *num_cols_f = ev->schur.f_cols;
  return CSE_OK;
}

extern "C++" {
namespace {
int SchurInit(cse_evaluator* ev, const double* d_jacobian_values, const double* d_D, const double* d_b,
              double* d_rhs, int preconditioner, double* d_gradient) {
  int rc = SchurCheck(ev, false);
  if (rc) return rc;
  if (!d_jacobian_values || !d_b || !d_rhs) return Fail(CSE_ERR_INVALID, "null pointer");
  auto& S = ev->schur;
  if (preconditioner != CSE_SCHUR_IDENTITY && preconditioner != CSE_SCHUR_JACOBI &&
      preconditioner != CSE_SCHUR_SCHUR_JACOBI)
    return Fail(CSE_ERR_INVALID, "unknown preconditioner");
  if (preconditioner == CSE_SCHUR_SCHUR_JACOBI && S.duplicates)
    return Fail(CSE_ERR_UNSUPPORTED,
                "SCHUR_JACOBI: an e block sees one f block in two residual blocks");
  Group& G = ev->groups[0];
  hipStream_t s = ev->stream;
  const bool grad = d_gradient != nullptr;
  if ((rc = S.ete_inv.ensure((size_t)2 * S.e_cols))) return rc;
  if ((rc = G.gcontrib.ensure((size_t)G.n * G.slot0_stride))) return rc;  // the multiplies'
  if ((rc = S.ub.ensure((size_t)G.n * (grad ? 4 : 2)))) return rc;
  S.jac = d_jacobian_values;
  S.D = d_D;
  S.b = d_b;
  S.preconditioner = preconditioner;
  // Point order: M_p, u_b = b_b - E_b M_p E_b^T b (and the gradient's e
  // rows); then camera order: rhs = F^T u, the gradient's f rows -F^T b and
  // the preconditioner's F^T Q F, each F cell read once.  The status word
  // read by cse_wait reports a non-positive pivot (schur_kernels.hpp, PivotOk).
  CSE_HIP(hipMemsetAsync(ev->status.p + 1, 0, sizeof(int), s));
  CSE_HIP(hipMemsetAsync(d_rhs, 0, S.f_cols * sizeof(double), s));
  if (grad)  // rows of blocks without residual blocks stay 0
    CSE_HIP(hipMemsetAsync(d_gradient, 0, ev->num_effective * sizeof(double), s));
  cse::SchurArgs a = MakeSchurArgs(ev, nullptr, nullptr);
  a.ub = S.ub.p;
  a.grad = d_gradient;
  if (grad)
    LaunchSchurPass<cse::kSchurInit, true>(a, s);
  else
    LaunchSchurPass<cse::kSchurInit>(a, s);
  CSE_HIP(hipGetLastError());
  const Group::GradPlan& P = G.grad[0];
  const int diag = preconditioner == CSE_SCHUR_IDENTITY ? 0 : preconditioner == CSE_SCHUR_JACOBI ? 1 : 2;
  const int parts = (diag ? cse::SymCount<9>() : 0) + 9 * (grad ? 2 : 1);
  if ((rc = S.partial.ensure((size_t)std::max<int64_t>(1, P.nchunks) * parts))) return rc;
  if (diag && (rc = S.precond.ensure((size_t)81 * P.count))) return rc;
  const cse::GradChunks ch{P.chunk_begin.p, P.chunk_off.p, S.partial.p, P.nchunks};
  // d_off: D index of camera lo + p = e_cols + f index = e_cols + f_col_base + 9 (lo + p).
  const int64_t d_off = S.e_cols + S.f_col_base + 9LL * P.lo;
  double* rhs_p = d_rhs + S.f_col_base + 9LL * P.lo;
  double* grad_p = grad ? d_gradient + G.delta_base[0] + 9LL * P.lo : nullptr;
  int* status = ev->status.p + 1;
  const SchurCameraLaunch L{a, &P, ch, d_D, d_off, S.precond.p, status, rhs_p, grad_p};
  switch (diag * 2 + (grad ? 1 : 0)) {
    case 0: LaunchSchurCameraPass<0, false>(L, s); break;
    case 1: LaunchSchurCameraPass<0, true>(L, s); break;
    case 2: LaunchSchurCameraPass<1, false>(L, s); break;
    case 3: LaunchSchurCameraPass<1, true>(L, s); break;
    case 4: LaunchSchurCameraPass<2, false>(L, s); break;
    default: LaunchSchurCameraPass<2, true>(L, s); break;
  }
  CSE_HIP(hipGetLastError());
  S.ready = true;
  return CSE_OK;
}
}  // namespace
}  // extern "C++"

int cse_schur_init(cse_evaluator* ev, const double* d_jacobian_values, const double* d_D,
                   const double* d_b, double* d_rhs, int preconditioner) {
  return SchurInit(ev, d_jacobian_values, d_D, d_b, d_rhs, preconditioner, nullptr);
}

int cse_schur_init_gradient(cse_evaluator* ev, const double* d_jacobian_values, const double* d_D,
                            const double* d_b, double* d_rhs, int preconditioner,
                            double* d_gradient) {
  if (!d_gradient) return Fail(CSE_ERR_INVALID, "null gradient");
  return SchurInit(ev, d_jacobian_values, d_D, d_b, d_rhs, preconditioner, d_gradient);
}

int cse_schur_multiply(cse_evaluator* ev, const double* d_x, double* d_y) {
  int rc = SchurCheck(ev, true);
  if (rc) return rc;
  if (!d_x || !d_y) return Fail(CSE_ERR_INVALID, "null pointer");
  const auto& S = ev->schur;
  hipStream_t s = ev->stream;
  hipLaunchKernelGGL(cse::SchurDiagKernel,
                     dim3((unsigned)((S.f_cols + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                     dim3(cse::kBlockThreads), 0, s, S.D, S.e_cols, d_x, d_y, S.f_cols);
  LaunchSchurPass<cse::kSchurMultiply>(MakeSchurArgs(ev, d_x, nullptr), s);
  CSE_HIP(hipGetLastError());
  return SchurFTail(ev, d_y, s);
}

int cse_schur_precondition(cse_evaluator* ev, const double* d_x, double* d_y) {
  int rc = SchurCheck(ev, true);
  if (rc) return rc;
  if (!d_x || !d_y) return Fail(CSE_ERR_INVALID, "null pointer");
  const auto& S = ev->schur;
  hipStream_t s = ev->stream;
  const unsigned grid = (unsigned)((S.f_cols + cse::kBlockThreads - 1) / cse::kBlockThreads);
  if (S.preconditioner == CSE_SCHUR_IDENTITY) {  // IdentityPreconditioner: y += x
    hipLaunchKernelGGL(cse::AxpyKernel, dim3(grid), dim3(cse::kBlockThreads), 0, s, d_x, d_y,
                       S.f_cols);
    CSE_HIP(hipGetLastError());
    return CSE_OK;
  }
  const Group::GradPlan& P = ev->groups[0].grad[0];
  // The cameras' f rows start at f index f_col_base + 9 lo.
  const int64_t off = S.f_col_base + 9LL * P.lo;
  hipLaunchKernelGGL((cse::SchurPrecondApplyKernel<9>), dim3(grid), dim3(cse::kBlockThreads), 0, s,
                     S.precond.p, d_x + off, d_y + off, 9LL * P.count);
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

int cse_schur_back_substitute(cse_evaluator* ev, const double* d_x, double* d_y) {
  int rc = SchurCheck(ev, true);
  if (rc) return rc;
  if (!d_x || !d_y) return Fail(CSE_ERR_INVALID, "null pointer");
  const auto& S = ev->schur;
  hipStream_t s = ev->stream;
  // e part: (E^T E + D_e^2)^-1 E^T (b - F x); f part: x.
  CSE_HIP(hipMemsetAsync(d_y, 0, S.e_cols * sizeof(double), s));
  LaunchSchurPass<cse::kSchurBack>(MakeSchurArgs(ev, d_x, d_y), s);
  CSE_HIP(hipGetLastError());
  CSE_HIP(hipMemcpyAsync(d_y + S.e_cols, d_x, S.f_cols * sizeof(double), hipMemcpyDeviceToDevice, s));
  return CSE_OK;
}

extern "C++" {
namespace {
// The pair plan of the explicit complement, from the group's ids as they were
// uploaded (the descriptor is gone after cse_create).
int SchurIds(cse_evaluator* ev, std::vector<int32_t>* ids) {
  const Group& G = ev->groups[0];
  ids->resize((size_t)(2 * G.n));
  CSE_HIP(hipStreamSynchronize(ev->stream));
  if (G.n > 0) CSE_HIP(hipMemcpy(ids->data(), G.ids.p, ids->size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  return CSE_OK;
}

// keep: receives the host tables of a plan built by this call (the
// block-sparse structure is made from them); have_ids: the ids, when the
// caller has downloaded them already.
int SchurPairPlanOf(cse_evaluator* ev, bool upload, cse::SchurPairPlan* keep = nullptr,
                    const std::vector<int32_t>* have_ids = nullptr) {
  auto& Q = ev->schur.pairs;
  if (upload ? Q.uploaded : Q.counted) return CSE_OK;
  const Group& G = ev->groups[0];
  std::vector<int32_t> own;
  int rc = have_ids ? CSE_OK : SchurIds(ev, &own);
  if (rc) return rc;
  const std::vector<int32_t>& ids = have_ids ? *have_ids : own;
  cse::SchurPairPlan P;
  rc = cse::PlanSchurPairs(ids.data(), G.n, !upload, &P);
  if (rc) return rc;
  static_cast<cse::SchurPairCounts&>(Q) = P;
  Q.counted = true;
  if (!upload) return CSE_OK;
  hipStream_t s = ev->stream;
  rc = Q.block_row.upload(P.block_row.data(), P.block_row.size(), s);
  if (!rc) rc = Q.block_col.upload(P.block_col.data(), P.block_col.size(), s);
  if (!rc) rc = Q.pair_begin.upload(P.pair_begin.data(), P.pair_begin.size(), s);
  if (!rc) rc = Q.chunk_off.upload(P.chunk_off.data(), P.chunk_off.size(), s);
  if (!rc) rc = Q.chunk_block.upload(P.chunk_block.data(), P.chunk_block.size(), s);
  if (!rc) rc = Q.pairs.upload(P.pairs.data(), P.pairs.size(), s);
  if (!rc) rc = Q.partial.alloc((size_t)(P.num_chunks * cse::kSchurBlockDoubles));
  // The copies read P's tables: wait before P goes out of scope.
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = Fail(CSE_ERR_HIP, "plan upload failed");
  if (rc) {
    for (DevBuf<int32_t>* b : {&Q.block_row, &Q.block_col, &Q.chunk_block, &Q.pairs}) b->release();
    Q.pair_begin.release();
    Q.chunk_off.release();
    Q.partial.release();
    return rc;
  }
  Q.uploaded = true;
  if (keep) *keep = std::move(P);  // the host tables, for the block-sparse structure
  return CSE_OK;
}
}  // namespace
}  // extern "C++"

int cse_schur_complement_plan(cse_evaluator* ev, int64_t* num_blocks, int64_t* num_pairs,
                              int64_t* plan_bytes) {
  int rc = SchurCheck(ev, false);
  if (rc) return rc;
  if ((rc = SchurPairPlanOf(ev, false))) return rc;
  const auto& Q = ev->schur.pairs;
  if (num_blocks) *num_blocks = Q.num_blocks;
  if (num_pairs) *num_pairs = Q.num_pairs;
  if (plan_bytes) *plan_bytes = Q.plan_bytes;
  return CSE_OK;
}

extern "C++" {
namespace {
// The block-sparse structure over the pair plan (both built and uploaded when
// upload; counts alone otherwise).
int SchurSparsePlanOf(cse_evaluator* ev, bool upload) {
  auto& Z = ev->schur.sparse;
  if (upload ? Z.uploaded : Z.counted) return CSE_OK;
  const Group& G = ev->groups[0];
  std::vector<int32_t> ids;
  int rc = SchurIds(ev, &ids);
  if (rc) return rc;
  cse::SchurPairPlan P;
  if ((rc = SchurPairPlanOf(ev, upload, &P, &ids))) return rc;
  // f index of f block id = f_col_base + 9 id, and camera 0 is f index 0.
  const int32_t first_id = (int32_t)(-ev->schur.f_col_base / 9);
  const int64_t C = ev->schur.f_cols / 9;
  if (upload && P.pair_begin.empty()) {
    // An earlier call uploaded the pair plan: the block-level tables that the
    // structure is made from come back from the device.
    const auto& Q = ev->schur.pairs;
    try {
      P.block_row.resize((size_t)Q.num_blocks);
      P.block_col.resize((size_t)Q.num_blocks);
      P.chunk_off.resize((size_t)Q.num_blocks + 1);
    } catch (const std::bad_alloc&) {
      return Fail(CSE_ERR_OOM, "block-sparse Schur complement: host allocation failed");
    }
    if (Q.num_blocks > 0) {
      CSE_HIP(hipMemcpy(P.block_row.data(), Q.block_row.p, P.block_row.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      CSE_HIP(hipMemcpy(P.block_col.data(), Q.block_col.p, P.block_col.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    CSE_HIP(hipMemcpy(P.chunk_off.data(), Q.chunk_off.p, P.chunk_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  }
  static_cast<cse::SchurPairCounts&>(P) = ev->schur.pairs;
  cse::SchurSparsePlan Y;
  if ((rc = cse::PlanSchurSparse(ids.data(), G.n, P, first_id, C, !upload, &Y))) return rc;
  static_cast<cse::SchurSparseCounts&>(Z) = Y;
  Z.counted = true;
  if (!upload) return CSE_OK;
  hipStream_t s = ev->stream;
  rc = Z.row_begin.upload(Y.row_begin.data(), Y.row_begin.size(), s);
  if (!rc) rc = Z.col_begin.upload(Y.col_begin.data(), Y.col_begin.size(), s);
  if (!rc) rc = Z.block_col.upload(Y.block_col.data(), Y.block_col.size(), s);
  if (!rc) rc = Z.plan_block.upload(Y.plan_block.data(), Y.plan_block.size(), s);
  if (!rc) rc = Z.sparse_of_plan.upload(Y.sparse_of_plan.data(), Y.sparse_of_plan.size(), s);
  if (!rc) rc = Z.finish.upload(Y.finish.data(), Y.finish.size(), s);
  if (!rc) rc = Z.col_block.upload(Y.col_block.data(), Y.col_block.size(), s);
  if (!rc) rc = Z.contrib.alloc((size_t)(9 * Y.num_blocks));
  // The copies read Y's tables: wait before Y goes out of scope.
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = Fail(CSE_ERR_HIP, "structure upload failed");
  if (rc) {
    for (DevBuf<int32_t>* b : {&Z.block_col, &Z.plan_block, &Z.sparse_of_plan, &Z.finish, &Z.col_block})
      b->release();
    Z.row_begin.release();
    Z.col_begin.release();
    Z.contrib.release();
    return rc;
  }
  Z.num_finish = (int64_t)Y.finish.size();
  Z.h_row_begin = std::move(Y.row_begin);
  Z.h_block_col = std::move(Y.block_col);
  Z.uploaded = true;
  return CSE_OK;
}

cse::SchurPairArgs MakeSchurPairArgs(cse_evaluator* ev) {
  const auto& S = ev->schur;
  const Group& G = ev->groups[0];
  const auto& Q = S.pairs;
  cse::SchurPairArgs a{};
  a.ids = G.ids.p;
  a.jac = S.jac;
  a.f_base = G.jac_base[0][0];
  a.e_base = G.jac_base[1][0];
  a.f_col_base = S.f_col_base;
  a.e_col_base = G.delta_base[1];
  a.e_cols = S.e_cols;
  a.D = S.D;
  a.ete_inv = S.ete_inv.p;
  a.block_row = Q.block_row.p;
  a.block_col = Q.block_col.p;
  a.pair_begin = Q.pair_begin.p;
  a.chunk_off = Q.chunk_off.p;
  a.chunk_block = Q.chunk_block.p;
  a.pairs = Q.pairs.p;
  a.nblocks = Q.num_blocks;
  a.nchunks = Q.num_chunks;
  a.partial = Q.partial.p;
  return a;
}
}  // namespace
}  // extern "C++"

int cse_schur_complement_sparse_structure(cse_evaluator* ev, int64_t* num_block_rows, int64_t* num_blocks,
                                          int64_t* device_bytes, int64_t* row_begin, int32_t* block_col) {
  int rc = SchurCheck(ev, false);
  if (rc) return rc;
  if ((rc = SchurSparsePlanOf(ev, row_begin || block_col))) return rc;
  const auto& Z = ev->schur.sparse;
  if (num_block_rows) *num_block_rows = Z.num_block_rows;
  if (num_blocks) *num_blocks = Z.num_blocks;
  if (device_bytes) *device_bytes = Z.device_bytes;
  if (row_begin) std::copy(Z.h_row_begin.begin(), Z.h_row_begin.end(), row_begin);
  if (block_col) std::copy(Z.h_block_col.begin(), Z.h_block_col.end(), block_col);
  return CSE_OK;
}

int cse_schur_complement_sparse(cse_evaluator* ev, double* d_values) {
  int rc = SchurCheck(ev, true);
  if (rc) return rc;
  if (!d_values) return Fail(CSE_ERR_INVALID, "null pointer");
  if ((rc = SchurSparsePlanOf(ev, true))) return rc;
  const auto& Q = ev->schur.pairs;
  const auto& Z = ev->schur.sparse;
  hipStream_t s = ev->stream;
  cse::SchurPairArgs a = MakeSchurPairArgs(ev);
  a.sparse_of_plan = Z.sparse_of_plan.p;
  a.plan_block = Z.plan_block.p;
  a.sparse_col = Z.block_col.p;
  a.finish = Z.finish.p;
  a.nfinish = Z.num_finish;
  a.values = d_values;
  if (Q.num_chunks > 0)
    hipLaunchKernelGGL((cse::SchurPairChunkKernel<9, true>),
                       dim3((unsigned)((Q.num_chunks + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
                       dim3(cse::kBlockThreads), 0, s, a);
  if (Z.num_finish > 0) {
    const int64_t entries = Z.num_finish * cse::kSchurBlockDoubles;
    hipLaunchKernelGGL((cse::SchurSparseFinishKernel<9>),
                       dim3((unsigned)((entries + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                       dim3(cse::kBlockThreads), 0, s, a);
  }
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

int cse_schur_explicit_multiply(cse_evaluator* ev, const double* d_values, const double* d_x, double* d_y) {
  int rc = SchurCheck(ev, true);
  if (rc) return rc;
  if (!d_values || !d_x || !d_y) return Fail(CSE_ERR_INVALID, "null pointer");
  // Workgroups assign y while others still read x: the two may not overlap.
  if (d_x < d_y + ev->schur.f_cols && d_y < d_x + ev->schur.f_cols)
    return Fail(CSE_ERR_INVALID, "cse_schur_explicit_multiply: x and y overlap");
  if ((rc = SchurSparsePlanOf(ev, true))) return rc;
  const auto& Z = ev->schur.sparse;
  cse::SchurExplicitArgs a{};
  a.row_begin = Z.row_begin.p;
  a.col_begin = Z.col_begin.p;
  a.block_col = Z.block_col.p;
  a.col_block = Z.col_block.p;
  a.values = d_values;
  a.x = d_x;
  a.y = d_y;
  a.C = Z.num_block_rows;
  if (Z.num_block_rows > 0) {
    // The rows' pass leaves each block's column contribution; the columns'
    // pass adds them to y in the transposed index's order.
    hipLaunchKernelGGL((cse::SchurExplicitRowKernel<9>), dim3((unsigned)Z.num_block_rows),
                       dim3(cse::kSchurExplicitWaves * cse::kWave), 0, ev->stream, a, Z.contrib.p);
    hipLaunchKernelGGL((cse::SchurExplicitColumnKernel<9>), dim3((unsigned)Z.num_block_rows),
                       dim3(cse::kBlockThreads), 0, ev->stream, a, (const double*)Z.contrib.p);
  }
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

// ---------------------------------------------------------------------------
// cse_schur_solve: the reference's conjugate gradients on the device
// (cg_state.hpp, cg_kernels.hpp)
// ---------------------------------------------------------------------------
void cse_cg_default_options(cse_cg_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->min_num_iterations = 1;
  o->max_num_iterations = 500;
  o->residual_reset_period = 10;
  o->check_period = 1;
  o->r_tolerance = -1.0;
  o->q_tolerance = 0.0;
}

extern "C++" {
namespace {

// The loop of conjugate_gradients_solver.h:108-305 over any operator: `op(x, y)`
// enqueues y = A x on the stream `s` and returns a cse status; the
// preconditioner is the one described in `a` (applied inside
// CgDirectionKernel).  The host enqueues check_period iterations, copies the
// state to pinned memory, waits once and stops or goes on; it computes no
// scalar of the iteration.  Nothing is allocated here.
template <class Op>
int CgSolve(const cse::CgArgs& a, const cse_cg_options& o, cse::CgState* state_host, hipStream_t s,
            Op&& op, cse_cg_summary* summary) {
  int rc;
  int32_t syncs = 0, enqueued = 0;
  auto look = [&]() -> int {
    CSE_HIP(hipMemcpyAsync(state_host, a.state, sizeof(cse::CgState), hipMemcpyDeviceToHost, s));
    CSE_HIP(hipStreamSynchronize(s));
    ++syncs;
    return CSE_OK;
  };
  const bool zero_guess = (o.flags & CSE_CG_ZERO_INITIAL_GUESS) != 0;
  cse::LaunchCgInit(a, zero_guess, s);
  if (!zero_guess) {
    if ((rc = op((const double*)a.x, a.tmp))) return rc;
    cse::LaunchCgInitialResidual(a, s);
  }
  CSE_HIP(hipGetLastError());
  // |b| = 0 and convergence before the first iteration end here.
  if ((rc = look())) return rc;
  for (int32_t it = 1; !state_host->done && it <= o.max_num_iterations; ++it) {
    cse::LaunchCgDirection(a, s);
    if ((rc = op((const double*)a.p, a.z))) return rc;
    if (it % o.residual_reset_period == 0) {
      cse::LaunchCgUpdate(cse::kCgUpdateX, a, s);
      if ((rc = op((const double*)a.x, a.tmp))) return rc;
      cse::LaunchCgUpdate(cse::kCgUpdateReset, a, s);
    } else {
      cse::LaunchCgUpdate(cse::kCgUpdateFull, a, s);
    }
    CSE_HIP(hipGetLastError());
    ++enqueued;
    if (enqueued % o.check_period == 0 || it == o.max_num_iterations)
      if ((rc = look())) return rc;
  }
  const cse::CgState& st = *state_host;
  if (!st.done) return Fail(CSE_ERR_HIP, "cse_schur_solve: the device state did not terminate");
  summary->termination_type = st.termination_type;
  summary->reason = st.reason;
  summary->num_iterations = st.iteration;
  summary->num_iterations_enqueued = enqueued;
  summary->num_synchronizations = syncs;
  summary->reserved = 0;
  summary->norm_rhs = st.norm_rhs;
  summary->norm_r = st.norm_r;
  summary->q = st.Q1;
  summary->zeta = st.zeta;
  summary->rho = st.rho;
  summary->pq = st.pq;
  return CSE_OK;
}

}  // namespace
}  // extern "C++"

int cse_schur_solve(cse_evaluator* ev, const cse_cg_options* options, const double* d_S_values,
                    const double* d_rhs, double* d_x, double* d_step, cse_cg_summary* summary) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_schur_solve");
  if (!options || !summary || !d_rhs || !d_x)
    return Fail(CSE_ERR_INVALID, "cse_schur_solve: null options, summary, d_rhs or d_x");
  const cse_cg_options& o = *options;
  if (o.check_period < 1) return Fail(CSE_ERR_INVALID, "cse_schur_solve: check_period is below 1");
  if (o.residual_reset_period < 1)
    return Fail(CSE_ERR_INVALID, "cse_schur_solve: residual_reset_period is below 1");
  if (o.max_num_iterations < 1)
    return Fail(CSE_ERR_INVALID, "cse_schur_solve: max_num_iterations is below 1");
  if (o.min_num_iterations < 0)
    return Fail(CSE_ERR_INVALID, "cse_schur_solve: min_num_iterations is negative");
  if (o.reserved != 0) return Fail(CSE_ERR_INVALID, "cse_schur_solve: options.reserved is not 0");
  if (o.flags & ~CSE_CG_ZERO_INITIAL_GUESS) return Fail(CSE_ERR_INVALID, "cse_schur_solve: unknown flags");
  int rc = SchurCheck(ev, true);
  if (rc) return rc;
  auto& S = ev->schur;
  const int64_t n = S.f_cols;
  if (d_rhs < d_x + n && d_x < d_rhs + n) return Fail(CSE_ERR_INVALID, "cse_schur_solve: d_x overlaps d_rhs");
  if (d_S_values && !S.sparse.uploaded)
    return Fail(CSE_ERR_INVALID,
                "cse_schur_solve: d_S_values without the block-sparse structure "
                "(cse_schur_complement_sparse_structure, cse_schur_complement_sparse)");
  auto& W = ev->cg;
  if ((rc = W.vectors.ensure((size_t)4 * (size_t)std::max<int64_t>(n, 1)))) return rc;
  if ((rc = W.state.ensure(1))) return rc;
  if (!W.state_host) CSE_HIP(hipHostMalloc((void**)&W.state_host, sizeof(cse::CgState)));
  cse::CgArgs a{};
  a.n = n;
  a.rhs = d_rhs;
  a.x = d_x;
  a.p = W.vectors.p;
  a.r = a.p + n;
  a.z = a.r + n;
  a.tmp = a.z + n;
  if (S.preconditioner != CSE_SCHUR_IDENTITY) {
    // The cameras' inverse blocks start at f index f_col_base + 9 lo
    // (cse_schur_precondition).
    const Group::GradPlan& P = ev->groups[0].grad[0];
    a.precond = S.precond.p;
    a.pre_off = S.f_col_base + 9LL * P.lo;
    a.pre_n = 9LL * P.count;
    if (a.pre_off < 0 || a.pre_off + a.pre_n > n || (size_t)(9 * a.pre_n) > S.precond.n)
      return Fail(CSE_ERR_INVALID, "cse_schur_solve: the preconditioner's blocks do not fit the f columns");
  }
  a.state = W.state.p;
  a.params = cse::CgParams{o.min_num_iterations, o.max_num_iterations, o.r_tolerance, o.q_tolerance};
  std::memset(summary, 0, sizeof(*summary));
  if (d_S_values)
    rc = CgSolve(a, o, W.state_host, ev->stream,
                 [&](const double* x, double* y) { return cse_schur_explicit_multiply(ev, d_S_values, x, y); },
                 summary);
  else
    rc = CgSolve(a, o, W.state_host, ev->stream,
                 [&](const double* x, double* y) { return cse_schur_multiply(ev, x, y); }, summary);
  if (rc) return rc;
  if (d_step && summary->termination_type != CSE_CG_FAILURE) return cse_schur_back_substitute(ev, d_x, d_step);
  return CSE_OK;
}

int cse_schur_complement(cse_evaluator* ev, double* d_S, int64_t ld) {
  int rc = SchurCheck(ev, true);
  if (rc) return rc;
  auto& S = ev->schur;
  if (!d_S) return Fail(CSE_ERR_INVALID, "null pointer");
  if (ld < S.f_cols) return Fail(CSE_ERR_INVALID, "cse_schur_complement: ld is smaller than num_cols_f");
  if ((rc = SchurPairPlanOf(ev, true))) return rc;
  const auto& Q = S.pairs;
  hipStream_t s = ev->stream;
  // Blocks of cameras that share no point stay zero; the rows' padding
  // [f_cols, ld) is not touched.
  if (S.f_cols > 0)
    CSE_HIP(hipMemset2DAsync(d_S, (size_t)ld * sizeof(double), 0, (size_t)S.f_cols * sizeof(double),
                             (size_t)S.f_cols, s));
  if (S.D && S.f_cols > 0)
    hipLaunchKernelGGL(cse::SchurDiagonalFillKernel,
                       dim3((unsigned)((S.f_cols + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                       dim3(cse::kBlockThreads), 0, s, S.D, S.e_cols, d_S, ld, S.f_cols);
  cse::SchurPairArgs a = MakeSchurPairArgs(ev);
  a.S = d_S;
  a.ld = ld;
  if (Q.num_chunks > 0) {
    hipLaunchKernelGGL((cse::SchurPairChunkKernel<9>),
                       dim3((unsigned)((Q.num_chunks + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
                       dim3(cse::kBlockThreads), 0, s, a);
    const int64_t entries = Q.num_blocks * cse::kSchurBlockDoubles;
    hipLaunchKernelGGL((cse::SchurPairFinishKernel<9>),
                       dim3((unsigned)((entries + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                       dim3(cse::kBlockThreads), 0, s, a);
  }
  CSE_HIP(hipGetLastError());
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

// The asan build keeps the per-block loss kernels in this object (its link
// line, tests/cpp/Makefile, lists the objects of ABI 5).
#ifdef CSE_PER_BLOCK_LOSS_IN_THIS_TU
#include "per_block_loss_kernels.hip"
#include "cg_kernels.hip"  // with this unit's flags there: no sanitizer run reaches an infinite scalar
#endif
