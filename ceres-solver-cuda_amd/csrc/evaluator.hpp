// evaluator.hpp -- the evaluator's host-side state (struct cse_evaluator and
// the device buffers of its groups), shared by cse_evaluator.hip (create,
// upload, evaluation, Plus), linear_operators.hip (the Jacobian-level calls of
// a linear solver) and schur_operators.hip (cse_schur_*).  A HIP host header:
// it defines no kernel.
#ifndef CSE_EVALUATOR_HPP_
#define CSE_EVALUATOR_HPP_

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/cse.h"
#include "cg_state.hpp"
#include "spse_state.hpp"
#include "plan.hpp"

struct CseMulti;  // multi_device.h

namespace cse {

struct GroupArgs;      // kernel_common.hpp
struct GradArgs;       // operator_kernels.hpp
struct SchurPairArgs;  // schur_complement_kernels.hpp

inline int Fail(int code, const std::string& msg) { return CseFail(code, msg); }

// Entry points whose arguments are device pointers of one device.
#define CSE_SINGLE_DEVICE(ev, what)                                                         \
  do {                                                                                     \
    if ((ev) && (ev)->multi)                                                               \
      return ::cse::Fail(CSE_ERR_UNSUPPORTED, std::string(what) +                          \
                                                  ": not available on a multi-device evaluator " \
                                                  "(cse_create_multi): its outputs span devices"); \
  } while (0)

#define CSE_HIP(call)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return ::cse::Fail(CSE_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

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

// A pair plan (cse::SchurPairPlan) on the device: its six tables and the chunk
// partials.  One rule for every holder: each buffer is allocated at exactly
// the plan's size, the partials at num_chunks blocks (what plan_bytes counts),
// and after a failure the tables are empty: Upload releases what it had
// allocated, and a caller whose stream synchronize fails calls Release.  The
// caller synchronizes before the host plan the copies read goes out of scope.
struct SchurPairTables {
  int64_t num_blocks = 0, num_chunks = 0;
  DevBuf<int32_t> block_row, block_col, chunk_block, pairs;
  DevBuf<int64_t> pair_begin, chunk_off;
  DevBuf<double> partial;
  int Upload(const SchurPairPlan& P, hipStream_t s) {
    int rc = block_row.upload(P.block_row.data(), P.block_row.size(), s);
    if (!rc) rc = block_col.upload(P.block_col.data(), P.block_col.size(), s);
    if (!rc) rc = pair_begin.upload(P.pair_begin.data(), P.pair_begin.size(), s);
    if (!rc) rc = chunk_off.upload(P.chunk_off.data(), P.chunk_off.size(), s);
    if (!rc) rc = chunk_block.upload(P.chunk_block.data(), P.chunk_block.size(), s);
    if (!rc) rc = pairs.upload(P.pairs.data(), P.pairs.size(), s);
    if (!rc) rc = partial.alloc((size_t)(P.num_chunks * kSchurBlockDoubles));
    if (rc) {
      Release();
      return rc;
    }
    num_blocks = P.num_blocks;
    num_chunks = P.num_chunks;
    return CSE_OK;
  }
  void Release() { *this = SchurPairTables{}; }
  // The table pointers, nblocks, nchunks and partial of a (schur_operators.hip).
  void Bind(SchurPairArgs* a) const;
};

// Waves per workgroup of the CGNR and Schur chunk kernels (one chunk per
// wave either way); one wave per workgroup, as the Jacobian kernels are
// launched, measured slower: S x 2.363 -> 2.410 ms, CGNR 2.596 -> 2.614 ms
// (profiles/round3/w1c).
constexpr int kOperatorWavesPerWg = cse::kWavesPerBlock;

inline bool SnavelyShaped(const Group& G) { return cse::SnavelyShaped(G.shape); }
inline bool UserFused(const Group& G) { return cse::UserFused(G.user, G.shape); }

}  // namespace cse

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
  std::vector<cse::Group> groups;
  int64_t total_wg = 0;
  bool any_general = false;
  cse::DevBuf<cse::PbDev> pbs;
  cse::DevBuf<double> cstate, plus_jac;
  cse::DevBuf<int64_t> res_layout, jac_layout, jac_offsets;
  cse::DevBuf<double> partials, partials2;
  // Program::Plus (cse_plus_device): runs of manifold-free state entries.
  bool plus_supported = true;
  std::vector<cse::PlusRun> plus_runs_host;
  cse::DevBuf<cse::PlusRun> plus_runs;
  // CSE_MANIFOLD_QUATERNION_EUCLIDEAN blocks: Plus one block per thread.
  std::vector<cse::QuatPlusBlock> plus_quat_host;
  cse::DevBuf<cse::QuatPlusBlock> plus_quat;
  cse::DevBuf<double> h_delta, h_plus;
  cse::DevBuf<int> status;  // [0] running flag, [1] last status, [2] reduce counter
  // Host-path buffers (allocated on first use).
  cse::DevBuf<double> h_state, h_cost, h_res, h_jac, h_grad;
  cse::DevBuf<double> cg_z;  // cse_cgnr_multiply's z = J x when it cannot fuse
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
    cse::DevBuf<int64_t> chunk_begin, big;
    // held (cse::ProgramPlan::schur_chunk_held and the others): a block's F
    // cell and a camera's f rows by rank.
    cse::DevBuf<int64_t> chunk_held, big_rank;
    cse::DevBuf<int32_t> fcell, cam_rank;
    cse::DevBuf<double> ete_inv, precond, partial, ub;
    bool ready = false;
    int preconditioner = CSE_SCHUR_IDENTITY;
    const double *jac = nullptr, *D = nullptr, *b = nullptr;
    bool ub_grad = false;  // ub holds [n][4] records (the init wrote the gradient)
    // max_num_spse_iterations of the POWER_SERIES preconditioner
    // (cse_schur_set_spse_iterations; linear_solver.h:172).
    int32_t spse_iterations = 5;
    // The explicit complement's pair plan (cse::PlanSchurPairs): counted on
    // the first plan query, built and uploaded on the first
    // cse_schur_complement; structure only, so it outlives every init.
    struct Pairs : cse::SchurPairCounts {
      bool counted = false, uploaded = false;
      cse::SchurPairTables tables;
    } pairs;
    // The block-sparse complement's structure (cse::PlanSchurSparse), cached
    // the same way; row_begin and block_col stay on the host too, for
    // cse_schur_complement_sparse_structure.
    struct Sparse : cse::SchurSparseCounts {
      bool counted = false, uploaded = false;
      int64_t num_finish = 0;
      std::vector<int64_t> h_row_begin;
      std::vector<int32_t> h_block_col;
      cse::DevBuf<int64_t> row_begin, col_begin;
      cse::DevBuf<int32_t> block_col, plan_block, sparse_of_plan, finish, col_block;
      cse::DevBuf<double> contrib;  // [num_blocks][9]: the product's column contributions
    } sparse;
    // CLUSTER_JACOBI (cse_schur_set_clusters, cse_schur_cluster_jacobi): the
    // partition as given, the cluster-filtered pair plan with its tile layout
    // (cse::PlanSchurClusters; built and uploaded when the partition
    // changes), the unfactored tiles, the factor.  `active` from a
    // build until the next init: cse_schur_precondition and cse_schur_solve
    // then apply the factor instead of the init's preconditioner.
    struct Cluster : cse::SchurClusterCounts {
      bool set = false, uploaded = false, active = false;
      std::vector<int32_t> labels;
      int32_t num_labels = 0;
      int64_t num_finish = 0;
      cse::SchurPairTables tables;  // the filtered plan
      cse::DevBuf<int32_t> tile_of_plan, plan_of_tile, tile_camera, finish;
      cse::DevBuf<int32_t> camera_begin, cameras;
      cse::DevBuf<int64_t> first_tile, value_begin;
      cse::DevBuf<double> tiles, factor, inv_diag;
    } cluster;
    // CLUSTER_TRIDIAGONAL (cse_schur_set_cluster_forest,
    // cse_schur_cluster_tridiagonal): the forest as given over `cluster`'s
    // partition, its own filtered plan and tiles (cse::PlanSchurTridiagonal;
    // CLUSTER_JACOBI's plan is not touched), the factor, the apply's scratch
    // and the first pass's failure flag.  A changed partition drops the forest.
    struct Tridiagonal : cse::SchurTridiagonalCounts {
      bool set = false, uploaded = false, active = false;
      std::vector<int32_t> edges;
      int64_t num_finish = 0;
      cse::SchurPairTables tables;
      cse::DevBuf<int32_t> tile_of_plan, plan_of_tile, tile_camera, finish;
      cse::DevBuf<int32_t> camera_begin, cameras, d_edges, path_begin, path_cluster, path_edge;
      cse::DevBuf<int64_t> first_tile, value_begin, edge_tile, edge_value;
      cse::DevBuf<double> tiles, factor, inv_diag, scratch;
      cse::DevBuf<int> failed;
    } tridiagonal;
  } schur;
  // cse_schur_solve's scratch (cg_kernels.hpp): the four vectors p, r, z, tmp
  // in one buffer and the state, allocated by the first solve.
  struct Cg {
    cse::DevBuf<double> vectors;
    cse::DevBuf<cse::CgState> state;
    cse::CgState* state_host = nullptr;  // pinned
  } cg;
  // cse_schur_power_series' scratch (spse_kernels.hpp), allocated by the first
  // series: the last term and Q times it, the state, its pinned copy, and --
  // after an init that built no (F^T F + D_f^2)^-1 blocks (IDENTITY,
  // SCHUR_JACOBI) -- blocks of its own with the camera pass's scratch (chunk
  // partials, the rhs and gradient rows that pass writes beside them).
  struct Spse {
    cse::DevBuf<double> vectors;
    cse::DevBuf<cse::SpseState> state;
    cse::SpseState* state_host = nullptr;  // pinned
    cse::DevBuf<double> blocks, partial, rows;
    bool blocks_ready = false;  // blocks are those of the current init
  } spse;
  // CGNR on the device (cse_cgnr_init, cse_cgnr_precondition, cse_cgnr_solve).
  // `plan` is the block table as cse_create planned it from the descriptor, in
  // runs; the first JACOBI init expands it, uploads it and looks each affine
  // slot's first block up (value_base).  The solve shares cg.state with
  // cse_schur_solve and has vectors of its own (num_effective_parameters each).
  struct Cgnr {
    cse::CgnrBlockPlan plan;
    bool uploaded = false;
    int64_t ntab = 0;
    cse::DevBuf<cse::CgnrBlock> blocks;
    // Per group, per slot: the value offset of parameter block `lo` of the
    // slot's gradient plan when the plan's blocks are consecutive table entries
    // of the slot's size; -1 otherwise (that group takes GramBlockKernel).
    std::vector<int64_t> value_base;
    cse::DevBuf<double> values;         // the inverse blocks
    cse::DevBuf<double> chunk_partial;  // the Gram's chunk partials (largest wave plan)
    cse::DevBuf<double> vectors, partial;
    cse::DevBuf<int> counter;
    bool ready = false;
    int preconditioner = CSE_CGNR_IDENTITY;
    const double *jac = nullptr, *D = nullptr;
  } cgnr;
  // The dense Cholesky factorization (cse_dense_cholesky_*, dense_cholesky.hip):
  // the workspace cse::PlanDenseCholesky lays out, kept and grown across
  // calls, and what the last factorize bound.
  struct DenseCholesky {
    cse::DevBuf<unsigned char> workspace;
    cse::DenseCholeskyPlan plan;
    bool factored = false;
    double* A = nullptr;  // the caller's matrix: L in FP64, read by a refining solve in FP32
    int64_t ld = 0;
  } dense;
  // The block-sparse Cholesky factorization (cse_sparse_cholesky_*,
  // sparse_cholesky.hip): the host plan of the last analyze
  // (cse::PlanSparseCholesky) and its tables on the device; L, the inverses of
  // its diagonal blocks, the two solve vectors and the status words, allocated
  // by the first factorize after an analyze; the values the last factorize bound.
  struct SparseCholesky {
    cse::SparseCholeskyPlan plan;
    bool analyzed = false, factored = false;
    cse::DevBuf<int32_t> permutation, position, block_col, block_row, col_block, source, level_columns, level_targets;
    cse::DevBuf<int32_t> in_block_col, in_col_block, in_col_row;
    cse::DevBuf<int64_t> row_begin, col_begin, in_row_begin, in_col_begin;
    cse::DevBuf<double> L, inverse, y, x;
    cse::DevBuf<int> status;  // [N] per column, then info
    const double* values = nullptr;
  } sparse;
};

namespace cse {

// Defined in cse_evaluator.hip, so that every kernel these launch is
// instantiated there alone.
GroupArgs MakeArgs(cse_evaluator* ev, Group& G, const double* state, double* res, double* jac,
                   double* grad);
// The post-pass of slot j, grad += J_j^T res: its arguments, and its kernels
// for the built-in shapes (the planner's GradSupported names the same ones);
// a user kind brings its own (cse_functor_ops.gradient).
GradArgs SlotGradArgs(const Group& G, int j, const double* jac, const double* res, double* grad);
bool LaunchGradPass(int nr, int size, const GradArgs& ga, const Group::GradPlan& P, hipStream_t s,
                    const cse_functor_ops* user = nullptr, int slot = 0);
// ga.grad += the slot-0 contributions [n][10], summed per parameter block in
// a fixed order (GradientContribKernel<9, 10>, GradientChunkReduceKernel<9>).
int LaunchContribReduce(const Group::GradPlan& P, const double* gcontrib, const GradArgs& ga,
                        hipStream_t s);
// After a fused kernel (the evaluator's FusedGrad or CgnrMultiplyKernel):
// add the slot-1 boundary entries and the slot-0 contributions, per
// parameter block in a fixed order, into out (delta offsets).
int LaunchFusedGradTail(const Group& G, double* out, hipStream_t s);
// y += x over n > 0 entries (AxpyKernel, schur_operators.hip's: CGNR comes here for it).
void LaunchAxpy(const double* x, double* y, int64_t n, hipStream_t s);

}  // namespace cse

#endif  // CSE_EVALUATOR_HPP_
