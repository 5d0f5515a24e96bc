// schur_operators.hip -- the cse_schur_* calls of the C ABI (include/cse.h) on
// the evaluator (evaluator.hpp): the implicit Schur complement and the power
// series (schur_kernels.hpp), the pair, sparse and cluster plans, the explicit
// complements (schur_complement_kernels.hpp), CLUSTER_JACOBI and
// CLUSTER_TRIDIAGONAL (cluster_kernels.hpp) and cse_schur_solve (cg_solve.hpp; the vector kernels
// through cg_kernels.h).  The per-camera sums are launched through
// evaluator.hpp's LaunchContribReduce: their kernels stay instantiated in
// cse_evaluator.hip.
#include <algorithm>
#include <cstring>
#include <new>

#include "cg_solve.hpp"
#include "cluster_kernels.hpp"
#include "launch.hpp"
#include "schur_complement_kernels.hpp"
#include "schur_kernels.hpp"

namespace cse {

void SchurPairTables::Bind(SchurPairArgs* a) const {
  a->block_row = block_row.p;
  a->block_col = block_col.p;
  a->pair_begin = pair_begin.p;
  a->chunk_off = chunk_off.p;
  a->chunk_block = chunk_block.p;
  a->pairs = pairs.p;
  a->nblocks = num_blocks;
  a->nchunks = num_chunks;
  a->partial = partial.p;
}

void LaunchAxpy(const double* x, double* y, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(AxpyKernel, Blocks(n), dim3(kBlockThreads), 0, s, x, y, n);
}

}  // namespace cse

namespace {

using cse::Blocks;
using cse::CgArgumentCheck;
using cse::CgSolve;
using cse::Fail;
using cse::Group;
using cse::kOperatorWavesPerWg;

// ---------------------------------------------------------------------------
// ITERATIVE_SCHUR on the device (schur_kernels.hpp)
// ---------------------------------------------------------------------------
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

// The kHeld kernels' tables; all null without held cameras.
cse::SchurHeldArgs MakeSchurHeldArgs(cse_evaluator* ev) {
  const auto& S = ev->schur;
  cse::SchurHeldArgs h{};
  if (S.held) {
    h.chunk_held = S.chunk_held.p;
    h.big_rank = S.big_rank.p;
    h.cam_rank = S.cam_rank.p;
    h.cam_lo = ev->groups[0].grad[0].lo;
  }
  return h;
}

// held (multiply and back substitution of a group with held cameras): the
// kHeld kernels; the init's point-order pass reads no F cell and is the same
// kernel either way.
template <int kMode, bool kGrad = false, bool kHeld = false>
void LaunchSchurPass(const cse::SchurArgs& a, hipStream_t s, const cse::SchurHeldArgs& h = {}) {
  constexpr int W = kOperatorWavesPerWg;
  if (a.nchunks > 0)
    hipLaunchKernelGGL((cse::SchurChunkKernel<9, kMode, W, kGrad, kHeld>), Blocks(a.nchunks, W),
                       dim3(W * cse::kWave), 0, s, a, h);
  if (a.nbig > 0)
    hipLaunchKernelGGL((cse::SchurBigKernel<9, kMode, kGrad, kHeld>), Blocks(a.nbig, cse::kWavesPerBlock),
                       dim3(cse::kBlockThreads), 0, s, a, h);
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
  if (ev->schur.held) {
    // The rows through the group's delta-offset table (an active camera's is
    // e_cols + 9 rank; a held camera has no chunk and its entry is not read).
    ga.grad = y - ev->schur.e_cols;
    ga.delta_tab = G.delta0.p + (P.lo - G.slot0_lo);
  }
  return LaunchContribReduce(P, G.gcontrib.p, ga, s);
}

// The inverse blocks' entries of an f vector: the cameras' f rows start at f
// index f_col_base + 9 lo; with held cameras the blocks are the active
// cameras', from f index 0.
void SchurBlockRange(const cse_evaluator* ev, int64_t* off, int64_t* n) {
  const auto& S = ev->schur;
  const Group::GradPlan& P = ev->groups[0].grad[0];
  *off = S.held ? 0 : S.f_col_base + 9LL * P.lo;
  *n = S.held ? S.f_cols : 9LL * P.count;
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
  // held cameras (null otherwise): the F cell of each perm entry, each camera's active rank
  const int32_t* fcell;
  const int32_t* cam_rank;
};

// The pass over the u_b records the init left in S.ub, with `partial` for its
// chunk partials; the inverse blocks go to precond, the rows to rhs and grad.
SchurCameraLaunch MakeSchurCameraLaunch(cse_evaluator* ev, double* partial, double* precond, double* rhs,
                                        double* grad) {
  const auto& S = ev->schur;
  const Group::GradPlan& P = ev->groups[0].grad[0];
  // d_off: D index of camera lo + p = e_cols + f index = e_cols + f_col_base + 9 (lo + p).
  // Held cameras: the finish writes camera lo + p at its active rank, from
  // the first f column.
  int64_t off, n;
  SchurBlockRange(ev, &off, &n);
  SchurCameraLaunch L{};
  L.a = MakeSchurArgs(ev, nullptr, nullptr);
  L.a.ub = S.ub.p;
  L.P = &P;
  L.ch = cse::GradChunks{P.chunk_begin.p, P.chunk_off.p, partial, P.nchunks};
  L.D = S.D;
  L.d_off = S.e_cols + off;
  L.precond = precond;
  L.status = ev->status.p + 1;
  L.rhs = rhs;
  L.grad = grad;
  L.fcell = S.held ? S.fcell.p : nullptr;
  L.cam_rank = S.held ? S.cam_rank.p : nullptr;
  return L;
}

template <int kDiag, bool kGrad, bool kHeld>
void LaunchSchurCameraPassAs(const SchurCameraLaunch& L, hipStream_t s) {
  const Group::GradPlan& P = *L.P;
  if (P.nchunks > 0)
    hipLaunchKernelGGL((cse::SchurCameraPassKernel<9, kDiag, kGrad, kHeld>), Blocks(P.nchunks, cse::kWavesPerBlock),
                       dim3(cse::kBlockThreads), 0, s, L.a, P.perm.p, L.ch, P.chunk_order.p, L.fcell);
  if (P.count > 0)
    hipLaunchKernelGGL((cse::SchurCameraFinishKernel<9, kDiag, kGrad, kHeld>), Blocks(P.count, 64), dim3(64), 0, s,
                       L.ch, P.count, L.D, L.d_off, L.precond, L.status, L.rhs, L.grad, L.cam_rank);
}

template <int kDiag, bool kGrad>
void LaunchSchurCameraPass(const SchurCameraLaunch& L, hipStream_t s) {
  if (L.cam_rank)  // held cameras
    LaunchSchurCameraPassAs<kDiag, kGrad, true>(L, s);
  else
    LaunchSchurCameraPassAs<kDiag, kGrad, false>(L, s);
}

// what: the name a multi-device refusal carries.
int SchurCheck(cse_evaluator* ev, bool need_ready, const char* what = "cse_schur") {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, what);
  if (!ev->schur.eligible)
    return Fail(CSE_ERR_UNSUPPORTED,
                "implicit Schur complement: needs one Snavely-shaped group (2 residuals, blocks of 9 and 3) "
                "on the affine BlockSparse path "
                "with its points (slot 1) as the leading e columns and its cameras after them");
  if (need_ready && !ev->schur.ready) return Fail(CSE_ERR_INVALID, "cse_schur_init has not run");
  CSE_HIP(hipSetDevice(ev->device));
  return CSE_OK;
}

// The explicit complements: their pair plan addresses F cells by block index.
int SchurExplicitCheck(cse_evaluator* ev, bool need_ready, const char* what) {
  const int rc = SchurCheck(ev, need_ready);
  if (rc) return rc;
  if (ev->schur.held)
    return Fail(CSE_ERR_UNSUPPORTED,
                std::string(what) + ": the explicit Schur complement is not available with held cameras "
                                    "(constant slot-0 blocks); the implicit operator is");
  return CSE_OK;
}

int SchurInit(cse_evaluator* ev, const double* d_jacobian_values, const double* d_D, const double* d_b,
              double* d_rhs, int preconditioner, double* d_gradient) {
  int rc = SchurCheck(ev, false);
  if (rc) return rc;
  if (!d_jacobian_values || !d_b || !d_rhs) return Fail(CSE_ERR_INVALID, "null pointer");
  auto& S = ev->schur;
  if (preconditioner != CSE_SCHUR_IDENTITY && preconditioner != CSE_SCHUR_JACOBI &&
      preconditioner != CSE_SCHUR_SCHUR_JACOBI && preconditioner != CSE_SCHUR_POWER_SERIES_EXPANSION)
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
  S.ub_grad = grad;
  ev->spse.blocks_ready = false;  // cse_schur_power_series builds its own after IDENTITY / SCHUR_JACOBI
  S.cluster.active = false;       // the init's own preconditioner is back
  S.tridiagonal.active = false;
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
  // POWER_SERIES_EXPANSION is JACOBI's init: the series' blocks are (F^T F + D_f^2)^-1.
  const int diag = preconditioner == CSE_SCHUR_IDENTITY ? 0 : preconditioner == CSE_SCHUR_SCHUR_JACOBI ? 2 : 1;
  const int parts = (diag ? cse::SymCount<9>() : 0) + 9 * (grad ? 2 : 1);
  if ((rc = S.partial.ensure((size_t)std::max<int64_t>(1, P.nchunks) * parts))) return rc;
  if (diag && (rc = S.precond.ensure((size_t)81 * (S.held ? S.num_active : P.count)))) return rc;
  // The rows of the plan's first camera (held: of the first active one).
  double* rhs_p = S.held ? d_rhs : d_rhs + S.f_col_base + 9LL * P.lo;
  double* grad_p = !grad ? nullptr : S.held ? d_gradient + S.e_cols : d_gradient + G.delta_base[0] + 9LL * P.lo;
  const SchurCameraLaunch L = MakeSchurCameraLaunch(ev, S.partial.p, S.precond.p, rhs_p, grad_p);
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

// ---------------------------------------------------------------------------
// SCHUR_POWER_SERIES_EXPANSION (spse_kernels.hpp; the kSchurSeries point pass
// of schur_kernels.hpp)
// ---------------------------------------------------------------------------
bool SchurInitBuiltFtfBlocks(const cse_evaluator* ev) {
  const int pc = ev->schur.preconditioner;
  return pc == CSE_SCHUR_JACOBI || pc == CSE_SCHUR_POWER_SERIES_EXPANSION;
}

// The series' scratch, and -- after an init that built no (F^T F + D_f^2)^-1
// blocks -- blocks of its own, by the pass a JACOBI init runs
// (SchurCameraPassKernel<9, 1>, SchurCameraFinishKernel) over the u_b records
// the init left in S.ub: the same kernels on the same inputs, so the blocks
// are a JACOBI init's bit for bit.  The rhs (and gradient) rows that pass
// writes go to scratch.
int SpseEnsure(cse_evaluator* ev) {
  auto& S = ev->schur;
  auto& Z = ev->spse;
  const int64_t n = S.f_cols;
  int rc;
  if ((rc = Z.vectors.ensure((size_t)2 * (size_t)std::max<int64_t>(n, 1)))) return rc;
  if ((rc = Z.state.ensure(1))) return rc;
  if (!Z.state_host) CSE_HIP(hipHostMalloc((void**)&Z.state_host, sizeof(cse::SpseState)));
  if (SchurInitBuiltFtfBlocks(ev) || Z.blocks_ready) return CSE_OK;
  const Group::GradPlan& P = ev->groups[0].grad[0];
  const bool grad = S.ub_grad;
  const int64_t blocks = S.held ? S.num_active : P.count;
  const int parts = cse::SymCount<9>() + 9 * (grad ? 2 : 1);
  if ((rc = Z.partial.ensure((size_t)std::max<int64_t>(1, P.nchunks) * parts))) return rc;
  if ((rc = Z.blocks.ensure((size_t)81 * (size_t)std::max<int64_t>(blocks, 1)))) return rc;
  if ((rc = Z.rows.ensure((size_t)18 * (size_t)std::max<int64_t>(blocks, 1)))) return rc;
  const SchurCameraLaunch L =
      MakeSchurCameraLaunch(ev, Z.partial.p, Z.blocks.p, Z.rows.p, grad ? Z.rows.p + 9 * blocks : nullptr);
  if (grad)
    LaunchSchurCameraPass<1, true>(L, ev->stream);
  else
    LaunchSchurCameraPass<1, false>(L, ev->stream);
  CSE_HIP(hipGetLastError());
  Z.blocks_ready = true;
  return CSE_OK;
}

// Enqueues the whole series on the evaluator's stream, no host wait:
// y = (accumulate: y +) sum_{i <= m} (P^-1 Q)^i P^-1 x, m the number of terms
// the state's stop test admits (power_series_expansion_preconditioner.cc:51-72).
// SpseEnsure has run.  Writes the series' own scratch, the contribution
// records and y alone.
int SpseEnqueue(cse_evaluator* ev, int32_t max_num_iterations, double tolerance, const double* x, double* y,
                bool accumulate) {
  const auto& S = ev->schur;
  auto& Z = ev->spse;
  hipStream_t s = ev->stream;
  const int64_t n = S.f_cols;
  cse::SpseArgs a{};
  a.n = n;
  a.blocks = SchurInitBuiltFtfBlocks(ev) ? S.precond.p : Z.blocks.p;
  SchurBlockRange(ev, &a.pre_off, &a.pre_n);
  if (a.pre_off < 0 || a.pre_off + a.pre_n > n)
    return Fail(CSE_ERR_INVALID, "cse_schur_power_series: the inverse blocks do not fit the f columns");
  a.x = x;
  a.y = y;
  a.prev = Z.vectors.p;
  double* t = Z.vectors.p + std::max<int64_t>(n, 1);
  a.t = t;
  a.state = Z.state.p;
  a.max_num_iterations = max_num_iterations;
  a.tolerance = tolerance;
  cse::LaunchSpseZero(a, accumulate, s);
  const cse::SchurArgs pass = MakeSchurArgs(ev, a.prev, nullptr);
  const cse::SchurHeldArgs held = MakeSchurHeldArgs(ev);
  for (int32_t i = 1; i <= max_num_iterations; ++i) {
    // t = Q prev: the point pass, then the per-camera sums into a zeroed t.
    if (S.held)
      LaunchSchurPass<cse::kSchurSeries, false, true>(pass, s, held);
    else
      LaunchSchurPass<cse::kSchurSeries>(pass, s);
    if (n > 0) CSE_HIP(hipMemsetAsync(t, 0, n * sizeof(double), s));
    int rc = SchurFTail(ev, t, s);
    if (rc) return rc;
    cse::LaunchSpseTerm(a, s);
  }
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

// ---------------------------------------------------------------------------
// The explicit complements' plans (cse::PlanSchurPairs, cse::PlanSchurSparse)
// ---------------------------------------------------------------------------
// The pair plan of the explicit complement, from the group's ids as they were
// uploaded (the descriptor is gone after cse_create).
int SchurIds(cse_evaluator* ev, std::vector<int32_t>* ids) {
  const Group& G = ev->groups[0];
  ids->resize((size_t)(2 * G.n));
  CSE_HIP(hipStreamSynchronize(ev->stream));
  if (G.n > 0) CSE_HIP(hipMemcpy(ids->data(), G.ids.p, ids->size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  return CSE_OK;
}

// The f block id of camera 0 and the number of cameras: the f index of f
// block id is f_col_base + 9 id, and camera 0 is f index 0.
void SchurCameraIndex(const cse_evaluator* ev, int32_t* first_id, int64_t* num_cameras) {
  *first_id = (int32_t)(-ev->schur.f_col_base / 9);
  *num_cameras = ev->schur.f_cols / 9;
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
  rc = Q.tables.Upload(P, s);
  // The copies read P's tables: wait before P goes out of scope.
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = Fail(CSE_ERR_HIP, "plan upload failed");
  if (rc) {
    Q.tables.Release();
    return rc;
  }
  Q.uploaded = true;
  if (keep) *keep = std::move(P);  // the host tables, for the block-sparse structure
  return CSE_OK;
}

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
  int32_t first_id;
  int64_t C;
  SchurCameraIndex(ev, &first_id, &C);
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
    const auto& T = Q.tables;
    if (Q.num_blocks > 0) {
      CSE_HIP(hipMemcpy(P.block_row.data(), T.block_row.p, P.block_row.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      CSE_HIP(hipMemcpy(P.block_col.data(), T.block_col.p, P.block_col.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    CSE_HIP(hipMemcpy(P.chunk_off.data(), T.chunk_off.p, P.chunk_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
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
    for (cse::DevBuf<int32_t>* b : {&Z.block_col, &Z.plan_block, &Z.sparse_of_plan, &Z.finish, &Z.col_block})
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

// The pair kernels' arguments over the pair plan in `tables`.
cse::SchurPairArgs MakeSchurPairArgs(cse_evaluator* ev, const cse::SchurPairTables& tables) {
  const auto& S = ev->schur;
  const Group& G = ev->groups[0];
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
  tables.Bind(&a);
  return a;
}

// The block store (kSparse kernels): every chunk, then the finish list.
void LaunchSchurBlockStore(const cse::SchurPairArgs& a, hipStream_t s) {
  if (a.nchunks > 0)
    hipLaunchKernelGGL((cse::SchurPairChunkKernel<9, true>), Blocks(a.nchunks, cse::kWavesPerBlock),
                       dim3(cse::kBlockThreads), 0, s, a);
  if (a.nfinish > 0)
    hipLaunchKernelGGL((cse::SchurSparseFinishKernel<9>), Blocks(a.nfinish * cse::kSchurBlockDoubles),
                       dim3(cse::kBlockThreads), 0, s, a);
}

// ---------------------------------------------------------------------------
// CLUSTER_JACOBI (cluster_kernels.hpp; cse::PlanSchurClusters)
// ---------------------------------------------------------------------------
int SchurClusterCheck(cse_evaluator* ev, const char* what) {
  const int rc = SchurCheck(ev, false, what);
  if (rc) return rc;
  if (ev->schur.held)
    return Fail(CSE_ERR_UNSUPPORTED,
                std::string(what) + ": CLUSTER_JACOBI is not available with held cameras (constant slot-0 "
                                    "blocks): the pair plan addresses F cells by block index");
  return CSE_OK;
}

// The filtered plan and the tile layout of the partition, built and uploaded
// once per partition (by cse_schur_set_clusters); the buffers beside the pair
// tables are kept (and grown when a later partition needs more).
int SchurClusterPlanOf(cse_evaluator* ev) {
  auto& K = ev->schur.cluster;
  if (K.uploaded) return CSE_OK;
  const Group& G = ev->groups[0];
  std::vector<int32_t> ids;
  int rc = SchurIds(ev, &ids);
  if (rc) return rc;
  int32_t first_id;
  int64_t C;
  SchurCameraIndex(ev, &first_id, &C);
  cse::SchurClusterPlan P;
  if ((rc = cse::PlanSchurClusters(ids.data(), G.n, first_id, C, K.labels.data(), K.num_labels, false, &P)))
    return rc;
  hipStream_t s = ev->stream;
  rc = K.tables.Upload(P.pairs, s);
  if (!rc) rc = K.tile_of_plan.upload(P.tile_of_plan.data(), P.tile_of_plan.size(), s);
  if (!rc) rc = K.plan_of_tile.upload(P.plan_of_tile.data(), P.plan_of_tile.size(), s);
  if (!rc) rc = K.tile_camera.upload(P.tile_camera.data(), P.tile_camera.size(), s);
  if (!rc) rc = K.finish.upload(P.finish.data(), P.finish.size(), s);
  if (!rc) rc = K.camera_begin.upload(P.camera_begin.data(), P.camera_begin.size(), s);
  if (!rc) rc = K.cameras.upload(P.cameras.data(), P.cameras.size(), s);
  if (!rc) rc = K.first_tile.upload(P.first_tile.data(), P.first_tile.size(), s);
  if (!rc) rc = K.value_begin.upload(P.value_begin.data(), P.value_begin.size(), s);
  if (!rc) rc = K.tiles.ensure((size_t)std::max<int64_t>(1, P.num_tiles * cse::kSchurBlockDoubles));
  if (!rc) rc = K.factor.ensure((size_t)std::max<int64_t>(1, P.num_tiles * cse::kSchurBlockDoubles));
  if (!rc) rc = K.inv_diag.ensure((size_t)std::max<int64_t>(1, 9 * C));
  // The copies read P's tables: wait before P goes out of scope.
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = Fail(CSE_ERR_HIP, "cluster plan upload failed");
  if (rc) {
    K.tables.Release();
    return rc;
  }
  static_cast<cse::SchurClusterCounts&>(K) = P;
  K.num_finish = (int64_t)P.finish.size();
  // One cluster in one workgroup's LDS: above 64 KiB the kernels need the
  // limit raised.
  CSE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&cse::ClusterFactorKernel<9>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)cse::ClusterFactorLds(cse::kSchurMaxClusterCameras)));
  CSE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&cse::ClusterApplyKernel<9>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)cse::ClusterApplyLds(cse::kSchurMaxClusterCameras)));
  K.uploaded = true;
  return CSE_OK;
}

cse::ClusterArgs MakeClusterArgs(cse_evaluator* ev) {
  const auto& K = ev->schur.cluster;
  cse::ClusterArgs a{};
  a.camera_begin = K.camera_begin.p;
  a.cameras = K.cameras.p;
  a.first_tile = K.first_tile.p;
  a.value_begin = K.value_begin.p;
  a.tiles = K.tiles.p;
  a.factor = K.factor.p;
  a.inv_diag = K.inv_diag.p;
  a.status = ev->status.p + 1;
  return a;
}

// y (+)= M^-1 x over every cluster; every f entry belongs to one cluster, so
// without `accumulate` y is assigned whole.
void LaunchClusterApply(cse_evaluator* ev, const double* x, double* y, bool accumulate) {
  const auto& K = ev->schur.cluster;
  if (K.num_clusters <= 0) return;
  hipLaunchKernelGGL((cse::ClusterApplyKernel<9>), dim3((unsigned)K.num_clusters), dim3(cse::kClusterThreads),
                     cse::ClusterApplyLds(K.max_cameras), ev->stream, MakeClusterArgs(ev), x, y,
                     accumulate ? 1 : 0);
}

// ---------------------------------------------------------------------------
// CLUSTER_TRIDIAGONAL (cluster_kernels.hpp; cse::PlanSchurTridiagonal)
// ---------------------------------------------------------------------------
// The forest's filtered plan, tile layout and paths, built and uploaded once
// per forest (by cse_schur_set_cluster_forest).
int SchurTridiagonalPlanOf(cse_evaluator* ev) {
  auto& T = ev->schur.tridiagonal;
  const auto& K = ev->schur.cluster;
  if (T.uploaded) return CSE_OK;
  const Group& G = ev->groups[0];
  std::vector<int32_t> ids;
  int rc = SchurIds(ev, &ids);
  if (rc) return rc;
  int32_t first_id;
  int64_t C;
  SchurCameraIndex(ev, &first_id, &C);
  cse::SchurTridiagonalPlan P;
  if ((rc = cse::PlanSchurTridiagonal(ids.data(), G.n, first_id, C, K.labels.data(), K.num_labels, T.edges.data(),
                                      (int32_t)(T.edges.size() / 2), false, &P)))
    return rc;
  hipStream_t s = ev->stream;
  rc = T.tables.Upload(P.pairs, s);
  if (!rc) rc = T.tile_of_plan.upload(P.tile_of_plan.data(), P.tile_of_plan.size(), s);
  if (!rc) rc = T.plan_of_tile.upload(P.plan_of_tile.data(), P.plan_of_tile.size(), s);
  if (!rc) rc = T.tile_camera.upload(P.tile_camera.data(), P.tile_camera.size(), s);
  if (!rc) rc = T.finish.upload(P.finish.data(), P.finish.size(), s);
  if (!rc) rc = T.camera_begin.upload(P.camera_begin.data(), P.camera_begin.size(), s);
  if (!rc) rc = T.cameras.upload(P.cameras.data(), P.cameras.size(), s);
  if (!rc) rc = T.first_tile.upload(P.first_tile.data(), P.first_tile.size(), s);
  if (!rc) rc = T.value_begin.upload(P.value_begin.data(), P.value_begin.size(), s);
  if (!rc) rc = T.d_edges.upload(P.edges.data(), P.edges.size(), s);
  if (!rc) rc = T.edge_tile.upload(P.edge_tile.data(), P.edge_tile.size(), s);
  if (!rc) rc = T.edge_value.upload(P.edge_value.data(), P.edge_value.size(), s);
  if (!rc) rc = T.path_begin.upload(P.paths.path_begin.data(), P.paths.path_begin.size(), s);
  if (!rc) rc = T.path_cluster.upload(P.paths.path_cluster.data(), P.paths.path_cluster.size(), s);
  if (!rc) rc = T.path_edge.upload(P.paths.path_edge.data(), P.paths.path_edge.size(), s);
  if (!rc) rc = T.tiles.ensure((size_t)std::max<int64_t>(1, P.num_tiles * cse::kSchurBlockDoubles));
  if (!rc) rc = T.factor.ensure((size_t)std::max<int64_t>(1, P.num_tiles * cse::kSchurBlockDoubles));
  if (!rc) rc = T.inv_diag.ensure((size_t)std::max<int64_t>(1, 9 * C));
  if (!rc) rc = T.scratch.ensure((size_t)std::max<int64_t>(1, 9 * C));
  if (!rc) rc = T.failed.ensure(1);
  // The copies read P's tables: wait before P goes out of scope.
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = Fail(CSE_ERR_HIP, "tridiagonal plan upload failed");
  if (rc) {
    T.tables.Release();
    return rc;
  }
  static_cast<cse::SchurTridiagonalCounts&>(T) = P;
  T.num_finish = (int64_t)P.finish.size();
  // One step in one workgroup's LDS: above 64 KiB the kernels need the limit raised.
  CSE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&cse::TridiagonalFactorKernel<9>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)cse::ClusterFactorLds(cse::kSchurMaxClusterCameras)));
  CSE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&cse::TridiagonalApplyKernel<9>),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)cse::TridiagonalApplyLds(cse::kSchurMaxClusterCameras)));
  T.uploaded = true;
  return CSE_OK;
}

cse::TridiagonalArgs MakeTridiagonalArgs(cse_evaluator* ev) {
  const auto& T = ev->schur.tridiagonal;
  cse::TridiagonalArgs a{};
  a.camera_begin = T.camera_begin.p;
  a.cameras = T.cameras.p;
  a.first_tile = T.first_tile.p;
  a.value_begin = T.value_begin.p;
  a.edges = T.d_edges.p;
  a.edge_tile = T.edge_tile.p;
  a.edge_value = T.edge_value.p;
  a.path_begin = T.path_begin.p;
  a.path_cluster = T.path_cluster.p;
  a.path_edge = T.path_edge.p;
  a.tiles = T.tiles.p;
  a.factor = T.factor.p;
  a.inv_diag = T.inv_diag.p;
  a.scratch = T.scratch.p;
  a.failed = T.failed.p;
  a.status = ev->status.p + 1;
  a.max_step = (int)T.max_step_cameras;
  return a;
}

// y (+)= M^-1 x over every path; every f entry belongs to one path.
void LaunchTridiagonalApply(cse_evaluator* ev, const double* x, double* y, bool accumulate) {
  const auto& T = ev->schur.tridiagonal;
  if (T.num_paths <= 0) return;
  hipLaunchKernelGGL((cse::TridiagonalApplyKernel<9>), dim3((unsigned)T.num_paths), dim3(cse::kClusterThreads),
                     cse::TridiagonalApplyLds(T.max_step_cameras), ev->stream, MakeTridiagonalArgs(ev), x, y,
                     accumulate ? 1 : 0);
}

// Whichever cluster preconditioner is active.
void LaunchActiveClusterApply(cse_evaluator* ev, const double* x, double* y, bool accumulate) {
  if (ev->schur.tridiagonal.active)
    LaunchTridiagonalApply(ev, x, y, accumulate);
  else
    LaunchClusterApply(ev, x, y, accumulate);
}

// ---------------------------------------------------------------------------
// cse_schur_solve (cg_solve.hpp)
// ---------------------------------------------------------------------------
// cg_kernels.hpp's one-workgroup kernels, and how z = M^-1 r is produced, a
// constant of the solve: inside CgDirectionKernel (the init's inverse blocks,
// or none), or by the series or the cluster apply enqueued first and the step
// that takes z as given.  The series' enqueue can only fail in a launch, which
// CgSolve's hipGetLastError after the iteration reports.
struct SchurCgLaunch {
  enum Preconditioner { kInKernel, kSeries, kClusters };
  cse::CgArgs a;
  cse_evaluator* ev;
  Preconditioner how;
  void Init(bool zero_guess, hipStream_t s) const { cse::LaunchCgInit(a, zero_guess, s); }
  void InitialResidual(hipStream_t s) const { cse::LaunchCgInitialResidual(a, s); }
  void Direction(hipStream_t s) const {
    switch (how) {
      case kInKernel: cse::LaunchCgDirection(a, s); return;
      case kSeries: (void)SpseEnqueue(ev, ev->schur.spse_iterations, 0.0, a.r, a.z, false); break;
      case kClusters: LaunchActiveClusterApply(ev, a.r, a.z, false); break;
    }
    cse::LaunchCgDirectionGiven(a, s);
  }
  void Update(cse::CgUpdateMode mode, hipStream_t s) const { cse::LaunchCgUpdate(mode, a, s); }
};

}  // namespace

extern "C" {

int cse_schur_structure(cse_evaluator* ev, int64_t* num_cols_e, int64_t* num_cols_f) {
  int rc = SchurCheck(ev, false);
  if (rc) return rc;
  if (num_cols_e) *num_cols_e = ev->schur.e_cols;
  if (num_cols_f) *num_cols_f = ev->schur.f_cols;
  return CSE_OK;
}

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
  hipLaunchKernelGGL(cse::SchurDiagKernel, Blocks(S.f_cols), dim3(cse::kBlockThreads), 0, s, S.D, S.e_cols, d_x,
                     d_y, S.f_cols);
  if (S.held)
    LaunchSchurPass<cse::kSchurMultiply, false, true>(MakeSchurArgs(ev, d_x, nullptr), s, MakeSchurHeldArgs(ev));
  else
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
  if (S.cluster.active || S.tridiagonal.active) {  // CLUSTER_JACOBI / _TRIDIAGONAL: y += M^-1 x by the factor
    LaunchActiveClusterApply(ev, d_x, d_y, true);
    CSE_HIP(hipGetLastError());
    return CSE_OK;
  }
  if (S.preconditioner == CSE_SCHUR_IDENTITY) {  // IdentityPreconditioner: y += x
    cse::LaunchAxpy(d_x, d_y, S.f_cols, s);
    CSE_HIP(hipGetLastError());
    return CSE_OK;
  }
  if (S.preconditioner == CSE_SCHUR_POWER_SERIES_EXPANSION) {
    // y += series(x), all spse_iterations terms (tolerance 0:
    // iterative_schur_complement_solver.cc:186-189).
    if (d_x < d_y + S.f_cols && d_y < d_x + S.f_cols)
      return Fail(CSE_ERR_INVALID, "cse_schur_precondition: x and y overlap (POWER_SERIES_EXPANSION)");
    if ((rc = SpseEnsure(ev))) return rc;
    return SpseEnqueue(ev, S.spse_iterations, 0.0, d_x, d_y, true);
  }
  int64_t off, n;
  SchurBlockRange(ev, &off, &n);
  hipLaunchKernelGGL((cse::SchurPrecondApplyKernel<9>), Blocks(S.f_cols), dim3(cse::kBlockThreads), 0, s,
                     S.precond.p, d_x + off, d_y + off, n);
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

int cse_schur_set_spse_iterations(cse_evaluator* ev, int32_t max_num_iterations) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_schur_set_spse_iterations");
  if (max_num_iterations < 1)
    return Fail(CSE_ERR_INVALID, "cse_schur_set_spse_iterations: max_num_iterations is below 1");
  ev->schur.spse_iterations = max_num_iterations;
  return CSE_OK;
}

int cse_schur_power_series(cse_evaluator* ev, int32_t max_num_iterations, double tolerance, const double* d_x,
                           double* d_y, cse_spse_summary* summary) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_schur_power_series");
  if (!d_x || !d_y) return Fail(CSE_ERR_INVALID, "cse_schur_power_series: null d_x or d_y");
  if (max_num_iterations < 1)
    return Fail(CSE_ERR_INVALID, "cse_schur_power_series: max_num_iterations is below 1");
  // solver.cc:277-281; spelled with the bits, this unit is built with -ffinite-math-only.
  const uint64_t tol_bits = __builtin_bit_cast(uint64_t, tolerance);
  const bool negative = (tol_bits >> 63) != 0 && (tol_bits << 1) != 0;  // -0.0 is 0
  if (negative || ((tol_bits >> 52) & 0x7ff) == 0x7ff)
    return Fail(CSE_ERR_INVALID, "cse_schur_power_series: tolerance is negative or not finite");
  int rc = SchurCheck(ev, true);
  if (rc) return rc;
  const int64_t n = ev->schur.f_cols;
  if (d_x < d_y + n && d_y < d_x + n) return Fail(CSE_ERR_INVALID, "cse_schur_power_series: d_x overlaps d_y");
  if ((rc = SpseEnsure(ev))) return rc;
  if ((rc = SpseEnqueue(ev, max_num_iterations, tolerance, d_x, d_y, false))) return rc;
  if (!summary) return CSE_OK;
  auto& Z = ev->spse;
  CSE_HIP(hipMemcpyAsync(Z.state_host, Z.state.p, sizeof(cse::SpseState), hipMemcpyDeviceToHost, ev->stream));
  CSE_HIP(hipStreamSynchronize(ev->stream));
  summary->num_terms = Z.state_host->num_terms;
  summary->reserved = 0;
  summary->norm_first = Z.state_host->norm_first;
  summary->norm_last = Z.state_host->norm_last;
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
  if (S.held)
    LaunchSchurPass<cse::kSchurBack, false, true>(MakeSchurArgs(ev, d_x, d_y), s, MakeSchurHeldArgs(ev));
  else
    LaunchSchurPass<cse::kSchurBack>(MakeSchurArgs(ev, d_x, d_y), s);
  CSE_HIP(hipGetLastError());
  CSE_HIP(hipMemcpyAsync(d_y + S.e_cols, d_x, S.f_cols * sizeof(double), hipMemcpyDeviceToDevice, s));
  return CSE_OK;
}

int cse_schur_complement_plan(cse_evaluator* ev, int64_t* num_blocks, int64_t* num_pairs,
                              int64_t* plan_bytes) {
  int rc = SchurExplicitCheck(ev, false, "cse_schur_complement_plan");
  if (rc) return rc;
  if ((rc = SchurPairPlanOf(ev, false))) return rc;
  const auto& Q = ev->schur.pairs;
  if (num_blocks) *num_blocks = Q.num_blocks;
  if (num_pairs) *num_pairs = Q.num_pairs;
  if (plan_bytes) *plan_bytes = Q.plan_bytes;
  return CSE_OK;
}

int cse_schur_complement(cse_evaluator* ev, double* d_S, int64_t ld) {
  int rc = SchurExplicitCheck(ev, true, "cse_schur_complement");
  if (rc) return rc;
  auto& S = ev->schur;
  if (!d_S) return Fail(CSE_ERR_INVALID, "null pointer");
  if (ld < S.f_cols) return Fail(CSE_ERR_INVALID, "cse_schur_complement: ld is smaller than num_cols_f");
  if ((rc = SchurPairPlanOf(ev, true))) return rc;
  hipStream_t s = ev->stream;
  // Blocks of cameras that share no point stay zero; the rows' padding
  // [f_cols, ld) is not touched.
  if (S.f_cols > 0)
    CSE_HIP(hipMemset2DAsync(d_S, (size_t)ld * sizeof(double), 0, (size_t)S.f_cols * sizeof(double),
                             (size_t)S.f_cols, s));
  if (S.D && S.f_cols > 0)
    hipLaunchKernelGGL(cse::SchurDiagonalFillKernel, Blocks(S.f_cols), dim3(cse::kBlockThreads), 0, s, S.D,
                       S.e_cols, d_S, ld, S.f_cols);
  cse::SchurPairArgs a = MakeSchurPairArgs(ev, S.pairs.tables);
  a.S = d_S;
  a.ld = ld;
  if (a.nchunks > 0) {
    hipLaunchKernelGGL((cse::SchurPairChunkKernel<9>), Blocks(a.nchunks, cse::kWavesPerBlock),
                       dim3(cse::kBlockThreads), 0, s, a);
    hipLaunchKernelGGL((cse::SchurPairFinishKernel<9>), Blocks(a.nblocks * cse::kSchurBlockDoubles),
                       dim3(cse::kBlockThreads), 0, s, a);
  }
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

int cse_schur_complement_sparse_structure(cse_evaluator* ev, int64_t* num_block_rows, int64_t* num_blocks,
                                          int64_t* device_bytes, int64_t* row_begin, int32_t* block_col) {
  int rc = SchurExplicitCheck(ev, false, "cse_schur_complement_sparse_structure");
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
  int rc = SchurExplicitCheck(ev, true, "cse_schur_complement_sparse");
  if (rc) return rc;
  if (!d_values) return Fail(CSE_ERR_INVALID, "null pointer");
  if ((rc = SchurSparsePlanOf(ev, true))) return rc;
  const auto& Z = ev->schur.sparse;
  cse::SchurPairArgs a = MakeSchurPairArgs(ev, ev->schur.pairs.tables);
  a.sparse_of_plan = Z.sparse_of_plan.p;
  a.plan_block = Z.plan_block.p;
  a.sparse_col = Z.block_col.p;
  a.finish = Z.finish.p;
  a.nfinish = Z.num_finish;
  a.values = d_values;
  LaunchSchurBlockStore(a, ev->stream);
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

int cse_schur_explicit_multiply(cse_evaluator* ev, const double* d_values, const double* d_x, double* d_y) {
  int rc = SchurExplicitCheck(ev, true, "cse_schur_explicit_multiply");
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

int cse_schur_set_clusters(cse_evaluator* ev, const int32_t* cluster_of_camera, int64_t num_cameras,
                           int32_t num_clusters) {
  int rc = SchurClusterCheck(ev, "cse_schur_set_clusters");
  if (rc) return rc;
  auto& K = ev->schur.cluster;
  if (!cluster_of_camera) return Fail(CSE_ERR_INVALID, "cse_schur_set_clusters: null cluster_of_camera");
  if (num_cameras != ev->schur.f_cols / 9)
    return Fail(CSE_ERR_INVALID, "cse_schur_set_clusters: num_cameras is " + std::to_string(num_cameras) +
                                     ", the program has " + std::to_string(ev->schur.f_cols / 9) +
                                     " (num_cols_f / 9)");
  if ((rc = cse::ValidateSchurClusters(cluster_of_camera, num_cameras, num_clusters))) return rc;
  // The structure is rebuilt only when the partition changes.
  if (K.set && K.num_labels == num_clusters && (int64_t)K.labels.size() == num_cameras &&
      std::equal(K.labels.begin(), K.labels.end(), cluster_of_camera))
    return CSE_OK;
  try {
    K.labels.assign(cluster_of_camera, cluster_of_camera + num_cameras);
  } catch (const std::bad_alloc&) {
    K.set = false;
    return Fail(CSE_ERR_OOM, "cse_schur_set_clusters: host allocation failed");
  }
  K.num_labels = num_clusters;
  K.uploaded = false;
  K.active = false;  // a factor of the earlier partition
  // The forest was one over the earlier partition's clusters: dropped.
  auto& T = ev->schur.tridiagonal;
  T.set = T.uploaded = T.active = false;
  T.edges.clear();
  // The filtered plan and the tile layout now, on the host, so that no linear
  // solve pays for them.
  K.set = true;
  if ((rc = SchurClusterPlanOf(ev))) K.set = false;
  return rc;
}

int cse_schur_cluster_jacobi(cse_evaluator* ev, double* d_matrices) {
  int rc = SchurClusterCheck(ev, "cse_schur_cluster_jacobi");
  if (rc) return rc;
  auto& S = ev->schur;
  auto& K = S.cluster;
  if (!S.ready) return Fail(CSE_ERR_INVALID, "cse_schur_cluster_jacobi: cse_schur_init has not run");
  if (!K.set) return Fail(CSE_ERR_INVALID, "cse_schur_cluster_jacobi: cse_schur_set_clusters has not run");
  if ((rc = SchurClusterPlanOf(ev))) return rc;
  hipStream_t s = ev->stream;
  // The cluster's cells by the explicit complement's kernels over the filtered
  // plan, stored tile by tile; the tiles no block writes are zero.
  cse::SchurPairArgs a = MakeSchurPairArgs(ev, K.tables);
  a.sparse_of_plan = K.tile_of_plan.p;
  a.plan_block = K.plan_of_tile.p;
  a.sparse_col = K.tile_camera.p;
  a.finish = K.finish.p;
  a.nfinish = K.num_finish;
  a.values = K.tiles.p;
  if (K.num_tiles > 0)
    CSE_HIP(hipMemsetAsync(K.tiles.p, 0, (size_t)K.num_tiles * cse::kSchurBlockDoubles * sizeof(double), s));
  LaunchSchurBlockStore(a, s);
  if (K.num_clusters > 0) {
    cse::ClusterArgs c = MakeClusterArgs(ev);
    c.matrices = d_matrices;
    hipLaunchKernelGGL((cse::ClusterFactorKernel<9>), dim3((unsigned)K.num_clusters),
                       dim3(cse::kClusterThreads), cse::ClusterFactorLds(K.max_cameras), s, c);
  }
  CSE_HIP(hipGetLastError());
  K.active = true;
  S.tridiagonal.active = false;  // the latest build is the active one
  return CSE_OK;
}

int cse_schur_set_cluster_forest(cse_evaluator* ev, const int32_t* edges, int32_t num_edges) {
  int rc = SchurClusterCheck(ev, "cse_schur_set_cluster_forest");
  if (rc) return rc;
  auto& K = ev->schur.cluster;
  auto& T = ev->schur.tridiagonal;
  if (!K.set) return Fail(CSE_ERR_INVALID, "cse_schur_set_cluster_forest: cse_schur_set_clusters has not run");
  if (num_edges < 0) return Fail(CSE_ERR_INVALID, "cse_schur_set_cluster_forest: negative num_edges");
  if (num_edges > 0 && !edges) return Fail(CSE_ERR_INVALID, "cse_schur_set_cluster_forest: null edges");
  // Refusals first, so that a refused forest leaves the one in place as it is.
  try {
    std::vector<int32_t> size((size_t)K.num_labels, 0);
    for (int32_t l : K.labels) ++size[(size_t)l];
    cse::SchurForestPaths paths;
    if ((rc = cse::ValidateSchurForest(edges, num_edges, size.data(), K.num_labels, &paths))) return rc;
    if (T.set && (int64_t)T.edges.size() == 2LL * num_edges && std::equal(T.edges.begin(), T.edges.end(), edges))
      return CSE_OK;
    T.edges.assign(edges, edges + 2 * (size_t)num_edges);
  } catch (const std::bad_alloc&) {
    T.set = false;
    return Fail(CSE_ERR_OOM, "cse_schur_set_cluster_forest: host allocation failed");
  }
  T.uploaded = false;
  T.active = false;  // a factor over the earlier forest
  T.set = true;
  if ((rc = SchurTridiagonalPlanOf(ev))) T.set = false;
  return rc;
}

int cse_schur_cluster_tridiagonal(cse_evaluator* ev, double* d_matrices, int32_t* d_scaled) {
  int rc = SchurClusterCheck(ev, "cse_schur_cluster_tridiagonal");
  if (rc) return rc;
  auto& S = ev->schur;
  auto& T = S.tridiagonal;
  if (!S.ready) return Fail(CSE_ERR_INVALID, "cse_schur_cluster_tridiagonal: cse_schur_init has not run");
  if (!S.cluster.set)
    return Fail(CSE_ERR_INVALID, "cse_schur_cluster_tridiagonal: cse_schur_set_clusters has not run");
  if (!T.set)
    return Fail(CSE_ERR_INVALID,
                "cse_schur_cluster_tridiagonal: cse_schur_set_cluster_forest has not run for this partition "
                "(a changed partition drops the forest)");
  if ((rc = SchurTridiagonalPlanOf(ev))) return rc;
  hipStream_t s = ev->stream;
  // The cells, off-diagonal ones included, by the explicit complement's
  // kernels over the filtered plan; the tiles no block writes are zero.
  cse::SchurPairArgs a = MakeSchurPairArgs(ev, T.tables);
  a.sparse_of_plan = T.tile_of_plan.p;
  a.plan_block = T.plan_of_tile.p;
  a.sparse_col = T.tile_camera.p;
  a.finish = T.finish.p;
  a.nfinish = T.num_finish;
  a.values = T.tiles.p;
  if (T.num_tiles > 0)
    CSE_HIP(hipMemsetAsync(T.tiles.p, 0, (size_t)T.num_tiles * cse::kSchurBlockDoubles * sizeof(double), s));
  CSE_HIP(hipMemsetAsync(T.failed.p, 0, sizeof(int), s));
  LaunchSchurBlockStore(a, s);
  if (T.num_paths > 0) {
    cse::TridiagonalArgs c = MakeTridiagonalArgs(ev);
    c.matrices = d_matrices;
    // M as it is; then, only when a pivot failed, every path again with its
    // edges halved: the second launch decides on the device.
    for (int scaled = 0; scaled < 2; ++scaled)
      hipLaunchKernelGGL((cse::TridiagonalFactorKernel<9>), dim3((unsigned)T.num_paths), dim3(cse::kClusterThreads),
                         cse::ClusterFactorLds(T.max_step_cameras), s, c, scaled);
  }
  CSE_HIP(hipGetLastError());
  if (d_scaled) CSE_HIP(hipMemcpyAsync(d_scaled, T.failed.p, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  T.active = true;
  S.cluster.active = false;  // the latest build is the active one
  return CSE_OK;
}

int cse_schur_solve(cse_evaluator* ev, const cse_cg_options* options, const double* d_S_values,
                    const double* d_rhs, double* d_x, double* d_step, cse_cg_summary* summary) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_schur_solve");
  int rc = CgArgumentCheck("cse_schur_solve", options, d_rhs, d_x, summary);
  if (rc) return rc;
  const cse_cg_options& o = *options;
  if ((rc = SchurCheck(ev, true))) return rc;
  auto& S = ev->schur;
  const int64_t n = S.f_cols;
  if (d_rhs < d_x + n && d_x < d_rhs + n) return Fail(CSE_ERR_INVALID, "cse_schur_solve: d_x overlaps d_rhs");
  if (d_S_values && S.held)
    return Fail(CSE_ERR_UNSUPPORTED,
                "cse_schur_solve: d_S_values (the explicit Schur complement) is not available with held "
                "cameras (constant slot-0 blocks); pass NULL for the implicit operator");
  const bool clusters = S.cluster.active || S.tridiagonal.active;
  const bool series = !clusters && S.preconditioner == CSE_SCHUR_POWER_SERIES_EXPANSION;
  const auto how = clusters ? SchurCgLaunch::kClusters
                   : series         ? SchurCgLaunch::kSeries
                                    : SchurCgLaunch::kInKernel;
  if (d_S_values && series)
    return Fail(CSE_ERR_UNSUPPORTED,
                "cse_schur_solve: d_S_values (the explicit Schur complement) with a POWER_SERIES_EXPANSION "
                "init; the explicit complement takes SCHUR_JACOBI alone (solver.cc:262-275)");
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
  if (series) {
    if ((rc = SpseEnsure(ev))) return rc;
  } else if (how == SchurCgLaunch::kInKernel && S.preconditioner != CSE_SCHUR_IDENTITY) {
    a.precond = S.precond.p;
    SchurBlockRange(ev, &a.pre_off, &a.pre_n);
    if (a.pre_off < 0 || a.pre_off + a.pre_n > n || (size_t)(9 * a.pre_n) > S.precond.n)
      return Fail(CSE_ERR_INVALID, "cse_schur_solve: the preconditioner's blocks do not fit the f columns");
  }
  a.state = W.state.p;
  a.params = cse::CgParams{o.min_num_iterations, o.max_num_iterations, o.r_tolerance, o.q_tolerance};
  std::memset(summary, 0, sizeof(*summary));
  // The operator: the block-sparse values when given, else the implicit one.
  rc = CgSolve("cse_schur_solve", SchurCgLaunch{a, ev, how}, o, W.state_host, ev->stream,
               [&](const double* x, double* y) {
                 return d_S_values ? cse_schur_explicit_multiply(ev, d_S_values, x, y) : cse_schur_multiply(ev, x, y);
               },
               summary);
  if (rc) return rc;
  if (d_step && summary->termination_type != CSE_CG_FAILURE) return cse_schur_back_substitute(ev, d_x, d_step);
  return CSE_OK;
}

}  // extern "C"
