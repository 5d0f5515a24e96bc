// linear_operators.hip -- the calls of the C ABI (include/cse.h) that a linear
// solver makes on the evaluator (evaluator.hpp): J x, J^T x and CGNR
// (operator_kernels.hpp), the column norms and ScaleColumns
// (column_kernels.hpp), the implicit Schur complement (schur_kernels.hpp),
// the explicit one (schur_complement_kernels.hpp), CLUSTER_JACOBI
// (cluster_kernels.hpp), cse_schur_solve and CGNR on
// the device (cgnr_kernels.hpp; the vector kernels through cg_kernels.h).  The
// gradient post-pass kernels are launched through evaluator.hpp's functions:
// they stay instantiated in cse_evaluator.hip.
#include <algorithm>
#include <cstring>
#include <new>

#include "cg_kernels.h"
#include "cgnr_kernels.hpp"
#include "cluster_kernels.hpp"
#include "column_kernels.hpp"
#include "evaluator.hpp"
#include "kernel_pickers.hpp"
#include "schur_complement_kernels.hpp"
#include "schur_kernels.hpp"

namespace {

using cse::DevBuf;
using cse::Fail;
using cse::Group;
using cse::kOperatorWavesPerWg;

bool DispatchMultiply(int kind, const cse::GroupArgs& a, bool affine, bool left, const double* x,
                      double* y, hipStream_t s) {
  const int which = affine && !left ? 0 : left ? 2 : 1;
  return cse::VisitKind(kind, [&](auto kd) { cse::LaunchMultiplyKernel<decltype(kd)>(a, which, x, y, s); });
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
        const cse::GradArgs ga = SlotGradArgs(G, j, J, x, y);
        if (!LaunchGradPass(G.shape.nr, sizes[j], ga, G.grad[j], ev->stream, G.user, j))
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

// ---------------------------------------------------------------------------
// SquaredColumnNorm and ScaleColumns (column_kernels.hpp, operator_kernels.hpp)
// ---------------------------------------------------------------------------
// The norm of slot j through its gradient plan, in the plan's form (as
// LaunchGradientSlot): identity order = contiguous block ranges; chunks of at
// most kGradChunk blocks and the ordered chunk reduce; one lane per parameter
// block.  P.chunk_partial is the plan's own (nchunks x S).
template <int NR, int S>
void LaunchColumnNormSlot(const cse::GradArgs& ga, const Group::GradPlan& P, hipStream_t s) {
  if (ga.count <= 0) return;
  if (ga.perm == nullptr) {
    hipLaunchKernelGGL((cse::ColumnNormRangeKernel<NR, S>), dim3((unsigned)((ga.count + cse::kWave - 1) / cse::kWave)),
                       dim3(cse::kWave), 0, s, ga);
  } else if (P.wave) {
    const cse::GradChunks ch{P.chunk_begin.p, P.chunk_off.p, P.chunk_partial.p, P.nchunks};
    if (P.nchunks > 0)
      hipLaunchKernelGGL((cse::ColumnNormLanesKernel<NR, S>),
                         dim3((unsigned)((P.nchunks + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
                         dim3(cse::kBlockThreads), 0, s, ga, ch);
    hipLaunchKernelGGL((cse::ColumnNormChunkReduceKernel<S>),
                       dim3((unsigned)((ga.count + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                       dim3(cse::kBlockThreads), 0, s, ga, ch);
  } else {
    hipLaunchKernelGGL((cse::ColumnNormSlotKernel<NR, S>),
                       dim3((unsigned)((ga.count + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                       dim3(cse::kBlockThreads), 0, s, ga);
  }
}

// Every shape an affine group can have (DetectAffine: at most 3 residuals)
// with blocks of up to 10 columns; false for a larger block.
template <int NR>
bool LaunchColumnNormSize(int size, const cse::GradArgs& ga, const Group::GradPlan& P, hipStream_t s) {
  switch (size) {
    case 1: LaunchColumnNormSlot<NR, 1>(ga, P, s); return true;
    case 2: LaunchColumnNormSlot<NR, 2>(ga, P, s); return true;
    case 3: LaunchColumnNormSlot<NR, 3>(ga, P, s); return true;
    case 4: LaunchColumnNormSlot<NR, 4>(ga, P, s); return true;
    case 5: LaunchColumnNormSlot<NR, 5>(ga, P, s); return true;
    case 6: LaunchColumnNormSlot<NR, 6>(ga, P, s); return true;
    case 7: LaunchColumnNormSlot<NR, 7>(ga, P, s); return true;
    case 8: LaunchColumnNormSlot<NR, 8>(ga, P, s); return true;
    case 9: LaunchColumnNormSlot<NR, 9>(ga, P, s); return true;
    case 10: LaunchColumnNormSlot<NR, 10>(ga, P, s); return true;
    default: return false;
  }
}

bool ColumnNormShape(int nr, int size) { return nr >= 1 && nr <= 3 && size >= 1 && size <= 10; }

void LaunchColumnNormPass(int nr, int size, const cse::GradArgs& ga, const Group::GradPlan& P, hipStream_t s) {
  if (nr == 1) LaunchColumnNormSize<1>(size, ga, P, s);
  if (nr == 2) LaunchColumnNormSize<2>(size, ga, P, s);
  if (nr == 3) LaunchColumnNormSize<3>(size, ga, P, s);
}

// The block-per-lane kernels' arguments: table addressing, or the affine
// parameters of a group whose tables were not uploaded.
cse::ColumnBlockArgs MakeColumnBlockArgs(cse_evaluator* ev, const Group& G, bool affine) {
  cse::ColumnBlockArgs a{};
  a.n = G.n;
  a.ids = G.ids.p;
  a.nr = G.shape.nr;
  a.nb = G.shape.nb;
  for (int j = 0; j < cse::kMaxSlots; ++j) a.sz[j] = G.shape.sz[j];
  a.affine = affine ? 1 : 0;
  a.pbs = ev->pbs.p;
  a.gindex = G.gindex.p;
  a.first = G.first;
  a.jac_layout = ev->jac_layout.p;
  a.jac_offsets = ev->jac_offsets.p;
  if (affine) {
    // The Jacobian's columns of slot 0 (s0) are the tangent's on a manifold kind.
    a.sz[0] = G.shape.s0;
    a.sz[1] = G.shape.s1;
    for (int j = 0; j < 2; ++j) {
      a.delta_base[j] = G.delta_base[j];
      a.jac_stride[j] = G.jac_stride[j];
      for (int r = 0; r < 3; ++r) a.jac_base[j][r] = G.jac_base[j][r];
    }
  }
  return a;
}

template <bool kScale>
void LaunchColumnBlocks(const cse::ColumnBlockArgs& a, double* jac, const double* scale, double* out,
                        hipStream_t s) {
  hipLaunchKernelGGL((cse::ColumnBlockKernel<kScale>),
                     dim3((unsigned)((a.n + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                     dim3(cse::kBlockThreads), 0, s, a, jac, scale, out);
}

int ColumnOpCheck(cse_evaluator* ev, const char* what, const void* p0, const void* p1) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, what);
  if (!ev->has_layout) return Fail(CSE_ERR_INVALID, "the descriptor had no Jacobian layout");
  if (!p0 || !p1) return Fail(CSE_ERR_INVALID, "null pointer");
  CSE_HIP(hipSetDevice(ev->device));
  return CSE_OK;
}

// The chunk runs of an affine group without held cameras (ScaleStreamArgs).
cse::ScaleStreamArgs MakeScaleStreamArgs(const Group& G) {
  const int nr = G.shape.nr, nb = G.shape.nb;
  const int sz[2] = {G.shape.s0, nb > 1 ? G.shape.s1 : 0};
  cse::ScaleStreamArgs a{};
  a.n = G.n;
  a.ids = G.ids.p;
  a.nb = nb;
  a.ntab = sz[0] + sz[1];
  for (int j = 0; j < nb; ++j) {
    a.sz[j] = sz[j];
    a.delta_base[j] = G.delta_base[j];
  }
  if (G.policy == cse::kAffineCrs) {
    // Rows of ntab doubles from row0; each slot at its column of the row.
    int64_t row0 = G.jac_base[0][0];
    for (int j = 0; j < nb; ++j) row0 = std::min(row0, G.jac_base[j][0]);
    for (int j = 0; j < nb; ++j) a.tab_off[j] = (int)(G.jac_base[j][0] - row0);
    a.nruns = 1;
    a.run_base[0] = row0;
    a.run_cell[0] = nr * a.ntab;
    a.run_s[0] = a.ntab;
    a.run_tab[0] = 0;
  } else {
    a.nruns = nb;
    for (int j = 0; j < nb; ++j) {
      a.tab_off[j] = j == 0 ? 0 : sz[0];
      a.run_base[j] = G.jac_base[j][0];
      a.run_cell[j] = nr * sz[j];
      a.run_s[j] = sz[j];
      a.run_tab[j] = a.tab_off[j];
    }
  }
  return a;
}

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
    hipLaunchKernelGGL((cse::SchurChunkKernel<9, kMode, W, kGrad, kHeld>),
                       dim3((unsigned)((a.nchunks + W - 1) / W)), dim3(W * cse::kWave), 0, s, a, h);
  if (a.nbig > 0)
    hipLaunchKernelGGL((cse::SchurBigKernel<9, kMode, kGrad, kHeld>),
                       dim3((unsigned)((a.nbig + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
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

template <int kDiag, bool kGrad, bool kHeld>
void LaunchSchurCameraPassAs(const SchurCameraLaunch& L, hipStream_t s) {
  const Group::GradPlan& P = *L.P;
  if (P.nchunks > 0)
    hipLaunchKernelGGL((cse::SchurCameraPassKernel<9, kDiag, kGrad, kHeld>),
                       dim3((unsigned)((P.nchunks + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
                       dim3(cse::kBlockThreads), 0, s, L.a, P.perm.p, L.ch, P.chunk_order.p, L.fcell);
  if (P.count > 0)
    hipLaunchKernelGGL((cse::SchurCameraFinishKernel<9, kDiag, kGrad, kHeld>),
                       dim3((unsigned)((P.count + 63) / 64)), dim3(64), 0, s, L.ch, P.count, L.D,
                       L.d_off, L.precond, L.status, L.rhs, L.grad, L.cam_rank);
}

template <int kDiag, bool kGrad>
void LaunchSchurCameraPass(const SchurCameraLaunch& L, hipStream_t s) {
  if (L.cam_rank)  // held cameras
    LaunchSchurCameraPassAs<kDiag, kGrad, true>(L, s);
  else
    LaunchSchurCameraPassAs<kDiag, kGrad, false>(L, s);
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
  const cse::GradChunks ch{P.chunk_begin.p, P.chunk_off.p, S.partial.p, P.nchunks};
  // d_off: D index of camera lo + p = e_cols + f index = e_cols + f_col_base + 9 (lo + p).
  // Held cameras: the finish writes camera lo + p at its active rank, from
  // the first f column.
  const int64_t d_off = S.held ? S.e_cols : S.e_cols + S.f_col_base + 9LL * P.lo;
  double* rhs_p = S.held ? d_rhs : d_rhs + S.f_col_base + 9LL * P.lo;
  double* grad_p = !grad ? nullptr : S.held ? d_gradient + S.e_cols : d_gradient + G.delta_base[0] + 9LL * P.lo;
  int* status = ev->status.p + 1;
  const SchurCameraLaunch L{a,      &P,    ch,     d_D, d_off, S.precond.p,
                            status, rhs_p, grad_p, S.held ? S.fcell.p : nullptr,
                            S.held ? S.cam_rank.p : nullptr};
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
// The inverse blocks' entries of an f vector (cse_schur_precondition): the
// cameras' f rows start at f index f_col_base + 9 lo; with held cameras the
// blocks are the active cameras', from f index 0.
void SchurBlockRange(const cse_evaluator* ev, int64_t* off, int64_t* n) {
  const auto& S = ev->schur;
  const Group::GradPlan& P = ev->groups[0].grad[0];
  *off = S.held ? 0 : S.f_col_base + 9LL * P.lo;
  *n = S.held ? S.f_cols : 9LL * P.count;
}

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
  Group& G = ev->groups[0];
  const Group::GradPlan& P = G.grad[0];
  const bool grad = S.ub_grad;
  const int64_t blocks = S.held ? S.num_active : P.count;
  const int parts = cse::SymCount<9>() + 9 * (grad ? 2 : 1);
  if ((rc = Z.partial.ensure((size_t)std::max<int64_t>(1, P.nchunks) * parts))) return rc;
  if ((rc = Z.blocks.ensure((size_t)81 * (size_t)std::max<int64_t>(blocks, 1)))) return rc;
  if ((rc = Z.rows.ensure((size_t)18 * (size_t)std::max<int64_t>(blocks, 1)))) return rc;
  cse::SchurArgs a = MakeSchurArgs(ev, nullptr, nullptr);
  a.ub = S.ub.p;
  const cse::GradChunks ch{P.chunk_begin.p, P.chunk_off.p, Z.partial.p, P.nchunks};
  const int64_t d_off = S.held ? S.e_cols : S.e_cols + S.f_col_base + 9LL * P.lo;  // as SchurInit
  const SchurCameraLaunch L{a,
                            &P,
                            ch,
                            S.D,
                            d_off,
                            Z.blocks.p,
                            ev->status.p + 1,
                            Z.rows.p,
                            grad ? Z.rows.p + 9 * blocks : nullptr,
                            S.held ? S.fcell.p : nullptr,
                            S.held ? S.cam_rank.p : nullptr};
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

// cse_schur_solve under a POWER_SERIES init: SchurCgLaunch with the direction
// step in two parts, z = series(r) enqueued, then the step that takes z as
// given.  The series' enqueue can only fail in a launch, which CgSolve's
// hipGetLastError after the iteration reports.
struct SchurSpseCgLaunch {
  cse::CgArgs a;
  cse_evaluator* ev;
  void Init(bool zero_guess, hipStream_t s) const { cse::LaunchCgInit(a, zero_guess, s); }
  void InitialResidual(hipStream_t s) const { cse::LaunchCgInitialResidual(a, s); }
  void Direction(hipStream_t s) const {
    (void)SpseEnqueue(ev, ev->schur.spse_iterations, 0.0, a.r, a.z, false);
    cse::LaunchCgDirectionGiven(a, s);
  }
  void Update(cse::CgUpdateMode mode, hipStream_t s) const { cse::LaunchCgUpdate(mode, a, s); }
};

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

// ---------------------------------------------------------------------------
// CLUSTER_JACOBI (cluster_kernels.hpp; cse::PlanSchurClusters)
// ---------------------------------------------------------------------------
int SchurClusterCheck(cse_evaluator* ev, const char* what) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, what);
  const int rc = SchurCheck(ev, false);
  if (rc) return rc;
  if (ev->schur.held)
    return Fail(CSE_ERR_UNSUPPORTED,
                std::string(what) + ": CLUSTER_JACOBI is not available with held cameras (constant slot-0 "
                                    "blocks): the pair plan addresses F cells by block index");
  return CSE_OK;
}

// The filtered plan and the tile layout of the partition, built and uploaded
// once per partition (by cse_schur_set_clusters); every buffer is kept (and
// grown when a later partition needs more).
int SchurClusterPlanOf(cse_evaluator* ev) {
  auto& K = ev->schur.cluster;
  if (K.uploaded) return CSE_OK;
  const Group& G = ev->groups[0];
  std::vector<int32_t> ids;
  int rc = SchurIds(ev, &ids);
  if (rc) return rc;
  const int32_t first_id = (int32_t)(-ev->schur.f_col_base / 9);  // as SchurSparsePlanOf
  const int64_t C = ev->schur.f_cols / 9;
  cse::SchurClusterPlan P;
  if ((rc = cse::PlanSchurClusters(ids.data(), G.n, first_id, C, K.labels.data(), K.num_labels, false, &P)))
    return rc;
  hipStream_t s = ev->stream;
  const cse::SchurPairPlan& Q = P.pairs;
  rc = K.block_row.upload(Q.block_row.data(), Q.block_row.size(), s);
  if (!rc) rc = K.block_col.upload(Q.block_col.data(), Q.block_col.size(), s);
  if (!rc) rc = K.pair_begin.upload(Q.pair_begin.data(), Q.pair_begin.size(), s);
  if (!rc) rc = K.chunk_off.upload(Q.chunk_off.data(), Q.chunk_off.size(), s);
  if (!rc) rc = K.chunk_block.upload(Q.chunk_block.data(), Q.chunk_block.size(), s);
  if (!rc) rc = K.pairs.upload(Q.pairs.data(), Q.pairs.size(), s);
  if (!rc) rc = K.partial.ensure((size_t)std::max<int64_t>(1, Q.num_chunks * cse::kSchurBlockDoubles));
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
  if (rc) return rc;
  static_cast<cse::SchurClusterCounts&>(K) = P;
  K.num_finish = (int64_t)P.finish.size();
  K.num_plan_blocks = Q.num_blocks;
  K.num_plan_chunks = Q.num_chunks;
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

// cse_schur_solve under the cluster preconditioner: as SchurSpseCgLaunch, the
// direction step in two parts, z = M^-1 r by the apply kernel, then the step
// that takes z as given.
struct SchurClusterCgLaunch {
  cse::CgArgs a;
  cse_evaluator* ev;
  void Init(bool zero_guess, hipStream_t s) const { cse::LaunchCgInit(a, zero_guess, s); }
  void InitialResidual(hipStream_t s) const { cse::LaunchCgInitialResidual(a, s); }
  void Direction(hipStream_t s) const {
    LaunchClusterApply(ev, a.r, a.z, false);
    cse::LaunchCgDirectionGiven(a, s);
  }
  void Update(cse::CgUpdateMode mode, hipStream_t s) const { cse::LaunchCgUpdate(mode, a, s); }
};

// ---------------------------------------------------------------------------
// cse_schur_solve: the reference's conjugate gradients on the device
// (cg_state.hpp, cg_kernels.hpp)
// ---------------------------------------------------------------------------
// The loop of conjugate_gradients_solver.h:108-305 over any operator and either
// set of vector kernels: `op(x, y)` enqueues y = A x on the stream `s` and
// returns a cse status; `L` launches the vector kernels over its arguments
// L.a (SchurCgLaunch: cg_kernels.hpp's one-workgroup kernels, the
// preconditioner applied inside CgDirectionKernel; CgnrCgLaunch:
// cg_sliced_kernels.hpp's).  The host enqueues check_period iterations, copies
// the state to pinned memory, waits once and stops or goes on; it computes no
// scalar of the iteration.  Nothing is allocated here.
struct SchurCgLaunch {
  cse::CgArgs a;
  void Init(bool zero_guess, hipStream_t s) const { cse::LaunchCgInit(a, zero_guess, s); }
  void InitialResidual(hipStream_t s) const { cse::LaunchCgInitialResidual(a, s); }
  void Direction(hipStream_t s) const { cse::LaunchCgDirection(a, s); }
  void Update(cse::CgUpdateMode mode, hipStream_t s) const { cse::LaunchCgUpdate(mode, a, s); }
};

struct CgnrCgLaunch {
  cse::CgSlicedArgs a;
  void Init(bool zero_guess, hipStream_t s) const { cse::LaunchCgSlicedInit(a, zero_guess, s); }
  void InitialResidual(hipStream_t s) const { cse::LaunchCgSlicedInitialResidual(a, s); }
  void Direction(hipStream_t s) const { cse::LaunchCgSlicedDirection(a, s); }
  void Update(cse::CgUpdateMode mode, hipStream_t s) const { cse::LaunchCgSlicedUpdate(mode, a, s); }
};

template <class Launch, class Op>
int CgSolve(const char* what, const Launch& L, const cse_cg_options& o, cse::CgState* state_host,
            hipStream_t s, Op&& op, cse_cg_summary* summary) {
  const auto& a = L.a;
  int rc;
  int32_t syncs = 0, enqueued = 0;
  auto look = [&]() -> int {
    CSE_HIP(hipMemcpyAsync(state_host, a.state, sizeof(cse::CgState), hipMemcpyDeviceToHost, s));
    CSE_HIP(hipStreamSynchronize(s));
    ++syncs;
    return CSE_OK;
  };
  const bool zero_guess = (o.flags & CSE_CG_ZERO_INITIAL_GUESS) != 0;
  L.Init(zero_guess, s);
  if (!zero_guess) {
    if ((rc = op((const double*)a.x, a.tmp))) return rc;
    L.InitialResidual(s);
  }
  CSE_HIP(hipGetLastError());
  // |b| = 0 and convergence before the first iteration end here.
  if ((rc = look())) return rc;
  for (int32_t it = 1; !state_host->done && it <= o.max_num_iterations; ++it) {
    L.Direction(s);
    if ((rc = op((const double*)a.p, a.z))) return rc;
    if (it % o.residual_reset_period == 0) {
      L.Update(cse::kCgUpdateX, s);
      if ((rc = op((const double*)a.x, a.tmp))) return rc;
      L.Update(cse::kCgUpdateReset, s);
    } else {
      L.Update(cse::kCgUpdateFull, s);
    }
    CSE_HIP(hipGetLastError());
    ++enqueued;
    if (enqueued % o.check_period == 0 || it == o.max_num_iterations)
      if ((rc = look())) return rc;
  }
  const cse::CgState& st = *state_host;
  if (!st.done) return Fail(CSE_ERR_HIP, std::string(what) + ": the device state did not terminate");
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

// The argument checks cse_schur_solve and cse_cgnr_solve share.
int CgArgumentCheck(const char* what, const cse_cg_options* options, const double* d_rhs, const double* d_x,
                    const cse_cg_summary* summary) {
  const std::string w = std::string(what) + ": ";
  if (!options || !summary || !d_rhs || !d_x)
    return Fail(CSE_ERR_INVALID, w + "null options, summary, d_rhs or d_x");
  const cse_cg_options& o = *options;
  if (o.check_period < 1) return Fail(CSE_ERR_INVALID, w + "check_period is below 1");
  if (o.residual_reset_period < 1) return Fail(CSE_ERR_INVALID, w + "residual_reset_period is below 1");
  if (o.max_num_iterations < 1) return Fail(CSE_ERR_INVALID, w + "max_num_iterations is below 1");
  if (o.min_num_iterations < 0) return Fail(CSE_ERR_INVALID, w + "min_num_iterations is negative");
  if (o.reserved != 0) return Fail(CSE_ERR_INVALID, w + "options.reserved is not 0");
  if (o.flags & ~CSE_CG_ZERO_INITIAL_GUESS) return Fail(CSE_ERR_INVALID, w + "unknown flags");
  return CSE_OK;
}

// ---------------------------------------------------------------------------
// CGNR on the device: the block-Jacobi preconditioner (cgnr_kernels.hpp) and
// cse_cgnr_solve (cg_sliced_kernels.hpp through cg_kernels.h)
// ---------------------------------------------------------------------------
// The Gram of slot j through its gradient plan, in the plan's form (as
// LaunchColumnNormSlot).  values: the S x S block of the plan's first
// parameter block; partial: cse_cgnr_init's own chunk partials.
template <int NR, int S>
void LaunchGramSlot(const cse::GradArgs& ga, const Group::GradPlan& P, double* values, double* partial,
                    hipStream_t s) {
  if (ga.count <= 0) return;
  if (ga.perm == nullptr) {
    hipLaunchKernelGGL((cse::GramRangeKernel<NR, S>), dim3((unsigned)((ga.count + cse::kWave - 1) / cse::kWave)),
                       dim3(cse::kWave), 0, s, ga, values);
  } else if (P.wave) {
    const cse::GradChunks ch{P.chunk_begin.p, P.chunk_off.p, partial, P.nchunks};
    if (P.nchunks > 0)
      hipLaunchKernelGGL((cse::GramLanesKernel<NR, S>),
                         dim3((unsigned)((P.nchunks + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
                         dim3(cse::kBlockThreads), 0, s, ga, ch);
    hipLaunchKernelGGL((cse::GramChunkReduceKernel<S>),
                       dim3((unsigned)((ga.count + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                       dim3(cse::kBlockThreads), 0, s, ga, ch, values);
  } else {
    hipLaunchKernelGGL((cse::GramSlotKernel<NR, S>),
                       dim3((unsigned)((ga.count + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                       dim3(cse::kBlockThreads), 0, s, ga, values);
  }
}

template <int NR>
void LaunchGramSize(int size, const cse::GradArgs& ga, const Group::GradPlan& P, double* values,
                    double* partial, hipStream_t s) {
  switch (size) {
    case 1: LaunchGramSlot<NR, 1>(ga, P, values, partial, s); break;
    case 2: LaunchGramSlot<NR, 2>(ga, P, values, partial, s); break;
    case 3: LaunchGramSlot<NR, 3>(ga, P, values, partial, s); break;
    case 4: LaunchGramSlot<NR, 4>(ga, P, values, partial, s); break;
    case 5: LaunchGramSlot<NR, 5>(ga, P, values, partial, s); break;
    case 6: LaunchGramSlot<NR, 6>(ga, P, values, partial, s); break;
    case 7: LaunchGramSlot<NR, 7>(ga, P, values, partial, s); break;
    case 8: LaunchGramSlot<NR, 8>(ga, P, values, partial, s); break;
    case 9: LaunchGramSlot<NR, 9>(ga, P, values, partial, s); break;
    case 10: LaunchGramSlot<NR, 10>(ga, P, values, partial, s); break;
    default: break;  // ColumnNormShape
  }
}

void LaunchGramPass(int nr, int size, const cse::GradArgs& ga, const Group::GradPlan& P, double* values,
                    double* partial, hipStream_t s) {
  if (nr == 1) LaunchGramSize<1>(size, ga, P, values, partial, s);
  if (nr == 2) LaunchGramSize<2>(size, ga, P, values, partial, s);
  if (nr == 3) LaunchGramSize<3>(size, ga, P, values, partial, s);
}

// An affine group's Gram goes through its gradient plans when every slot has
// one in a form the kernels take (as the column norm) and its parameter blocks
// are consecutive entries of the block table (CgnrUpload's value_base).
bool GramThroughPlans(const cse_evaluator* ev, size_t gi) {
  const Group& G = ev->groups[gi];
  if (!G.affine || G.const0) return false;
  const int sizes[2] = {G.shape.s0, G.shape.s1};
  for (int j = 0; j < G.shape.nb; ++j) {
    const Group::GradPlan& P = G.grad[j];
    if (j >= 2 || !P.ready || !ColumnNormShape(G.shape.nr, sizes[j])) return false;
    if (!P.sorted && P.wave && !(P.chunk_begin.p && P.chunk_off.p)) return false;
    if (ev->cgnr.value_base[2 * gi + j] < 0) return false;
  }
  return true;
}

// First JACOBI init: every affine slot's first block is looked up in the
// plan's runs, and the table is expanded and uploaded (the host copy lives
// for this call only).
int CgnrUpload(cse_evaluator* ev) {
  auto& C = ev->cgnr;
  if (C.uploaded) return CSE_OK;
  C.value_base.assign(2 * ev->groups.size(), -1);
  int64_t chunk_doubles = 1;
  for (size_t gi = 0; gi < ev->groups.size(); ++gi) {
    const Group& G = ev->groups[gi];
    if (!G.affine || G.const0) continue;
    const int sizes[2] = {G.shape.s0, G.shape.s1};
    for (int j = 0; j < G.shape.nb && j < 2; ++j) {
      const Group::GradPlan& P = G.grad[j];
      if (!P.ready || P.count <= 0) continue;
      const int S = sizes[j];
      // Blocks lo .. lo + count - 1 are consecutive entries of size S when
      // the first is in a run of that size that holds count more.
      const cse::CgnrRun* run = nullptr;
      const int64_t first = cse::FindCgnrBlock(C.plan, G.delta_base[j] + (int64_t)S * P.lo, &run);
      if (first < 0 || run->tangent_size != S || first + P.count > run->first_block + run->count) continue;
      C.value_base[2 * gi + j] = run->value_offset + (first - run->first_block) * (int64_t)S * S;
      if (P.wave) chunk_doubles = std::max<int64_t>(chunk_doubles, P.nchunks * cse::GramCount(S));
    }
  }
  int rc;
  if ((rc = C.chunk_partial.ensure((size_t)chunk_doubles))) return rc;
  if ((rc = C.values.ensure((size_t)std::max<int64_t>(C.plan.num_values, 1)))) return rc;
  std::vector<cse::CgnrBlock> table;
  try {
    cse::ExpandCgnrBlocks(C.plan, &table);
  } catch (const std::bad_alloc&) {
    return Fail(CSE_ERR_OOM, "cse_cgnr_init: host allocation of the block table failed");
  }
  if ((rc = C.blocks.upload(table.data(), table.size(), ev->stream))) return rc;
  // The copy reads the host table: wait before it goes out of scope.
  CSE_HIP(hipStreamSynchronize(ev->stream));
  C.ntab = (int64_t)table.size();
  C.uploaded = true;
  return CSE_OK;
}

int CgnrCheck(cse_evaluator* ev, const char* what, bool need_ready) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, what);
  if (!ev->has_layout) return Fail(CSE_ERR_INVALID, "the descriptor had no Jacobian layout");
  if (need_ready && !ev->cgnr.ready) return Fail(CSE_ERR_INVALID, std::string(what) + ": cse_cgnr_init has not run");
  CSE_HIP(hipSetDevice(ev->device));
  return CSE_OK;
}

}  // namespace

extern "C" {

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
    if (G.policy == cse::kAffineCrs)
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

int cse_jacobian_squared_column_norm(cse_evaluator* ev, const double* d_jacobian_values, double* d_x) {
  int rc = ColumnOpCheck(ev, "cse_jacobian_squared_column_norm", d_jacobian_values, d_x);
  if (rc) return rc;
  hipStream_t s = ev->stream;
  // Assigned: zero, then every group adds (groups may share columns, and a
  // column without cells reads 0).
  if (ev->num_effective > 0) CSE_HIP(hipMemsetAsync(d_x, 0, ev->num_effective * sizeof(double), s));
  for (auto& G : ev->groups) {
    if (G.n == 0) continue;
    // Held cameras (const0): the table kernel, as the products.
    const bool affine = G.affine && !G.const0;
    const int sizes[2] = {G.shape.s0, G.shape.s1};
    bool plans = affine;
    for (int j = 0; j < G.shape.nb; ++j)
      plans = plans && G.grad[j].ready && ColumnNormShape(G.shape.nr, sizes[j]) &&
              (G.grad[j].sorted || !G.grad[j].wave || G.grad[j].chunk_partial.p);
    if (plans) {
      for (int j = 0; j < G.shape.nb; ++j)
        LaunchColumnNormPass(G.shape.nr, sizes[j], SlotGradArgs(G, j, d_jacobian_values, nullptr, d_x),
                             G.grad[j], s);
    } else {
      if (!affine && !ev->any_general)
        return Fail(CSE_ERR_UNSUPPORTED, "table-path tables were not uploaded");
      LaunchColumnBlocks<false>(MakeColumnBlockArgs(ev, G, affine), const_cast<double*>(d_jacobian_values),
                                nullptr, d_x, s);
    }
    CSE_HIP(hipGetLastError());
  }
  return CSE_OK;
}

int cse_jacobian_scale_columns(cse_evaluator* ev, double* d_jacobian_values, const double* d_scale) {
  int rc = ColumnOpCheck(ev, "cse_jacobian_scale_columns", d_jacobian_values, d_scale);
  if (rc) return rc;
  hipStream_t s = ev->stream;
  for (auto& G : ev->groups) {
    if (G.n == 0) continue;
    if (G.affine && !G.const0) {
      const cse::ScaleStreamArgs a = MakeScaleStreamArgs(G);
      constexpr int W = kOperatorWavesPerWg;
      const int64_t chunks = (G.n + cse::kWave - 1) / cse::kWave;
      hipLaunchKernelGGL((cse::ScaleColumnsStreamKernel<W>), dim3((unsigned)((chunks + W - 1) / W)),
                         dim3(W * cse::kWave), (size_t)W * cse::kWave * a.ntab * sizeof(double), s, a,
                         d_jacobian_values, d_scale);
    } else {
      // Held cameras (compacted F cells, two row widths) and the table path.
      if (!ev->any_general) return Fail(CSE_ERR_UNSUPPORTED, "table-path tables were not uploaded");
      LaunchColumnBlocks<true>(MakeColumnBlockArgs(ev, G, false), d_jacobian_values, d_scale, nullptr, s);
    }
    CSE_HIP(hipGetLastError());
  }
  return CSE_OK;
}

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
  hipLaunchKernelGGL(cse::SchurDiagKernel,
                     dim3((unsigned)((S.f_cols + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                     dim3(cse::kBlockThreads), 0, s, S.D, S.e_cols, d_x, d_y, S.f_cols);
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
  const unsigned grid = (unsigned)((S.f_cols + cse::kBlockThreads - 1) / cse::kBlockThreads);
  if (S.cluster.active) {  // CLUSTER_JACOBI: y += M^-1 x by the factor
    LaunchClusterApply(ev, d_x, d_y, true);
    CSE_HIP(hipGetLastError());
    return CSE_OK;
  }
  if (S.preconditioner == CSE_SCHUR_IDENTITY) {  // IdentityPreconditioner: y += x
    hipLaunchKernelGGL(cse::AxpyKernel, dim3(grid), dim3(cse::kBlockThreads), 0, s, d_x, d_y,
                       S.f_cols);
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
  const Group::GradPlan& P = ev->groups[0].grad[0];
  // The cameras' f rows start at f index f_col_base + 9 lo; with held
  // cameras the blocks are the active cameras', from f index 0.
  const int64_t off = S.held ? 0 : S.f_col_base + 9LL * P.lo;
  hipLaunchKernelGGL((cse::SchurPrecondApplyKernel<9>), dim3(grid), dim3(cse::kBlockThreads), 0, s,
                     S.precond.p, d_x + off, d_y + off, S.held ? S.f_cols : 9LL * P.count);
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
  cse::SchurPairArgs a = MakeSchurPairArgs(ev);
  a.block_row = K.block_row.p;
  a.block_col = K.block_col.p;
  a.pair_begin = K.pair_begin.p;
  a.chunk_off = K.chunk_off.p;
  a.chunk_block = K.chunk_block.p;
  a.pairs = K.pairs.p;
  a.nblocks = K.num_plan_blocks;
  a.nchunks = K.num_plan_chunks;
  a.partial = K.partial.p;
  a.sparse_of_plan = K.tile_of_plan.p;
  a.plan_block = K.plan_of_tile.p;
  a.sparse_col = K.tile_camera.p;
  a.finish = K.finish.p;
  a.nfinish = K.num_finish;
  a.values = K.tiles.p;
  if (K.num_tiles > 0)
    CSE_HIP(hipMemsetAsync(K.tiles.p, 0, (size_t)K.num_tiles * cse::kSchurBlockDoubles * sizeof(double), s));
  if (K.num_plan_chunks > 0)
    hipLaunchKernelGGL((cse::SchurPairChunkKernel<9, true>),
                       dim3((unsigned)((K.num_plan_chunks + cse::kWavesPerBlock - 1) / cse::kWavesPerBlock)),
                       dim3(cse::kBlockThreads), 0, s, a);
  if (K.num_finish > 0) {
    const int64_t entries = K.num_finish * cse::kSchurBlockDoubles;
    hipLaunchKernelGGL((cse::SchurSparseFinishKernel<9>),
                       dim3((unsigned)((entries + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                       dim3(cse::kBlockThreads), 0, s, a);
  }
  if (K.num_clusters > 0) {
    cse::ClusterArgs c = MakeClusterArgs(ev);
    c.matrices = d_matrices;
    hipLaunchKernelGGL((cse::ClusterFactorKernel<9>), dim3((unsigned)K.num_clusters),
                       dim3(cse::kClusterThreads), cse::ClusterFactorLds(K.max_cameras), s, c);
  }
  CSE_HIP(hipGetLastError());
  K.active = true;
  return CSE_OK;
}

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
  const bool clusters = S.cluster.active;
  const bool series = !clusters && S.preconditioner == CSE_SCHUR_POWER_SERIES_EXPANSION;
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
  } else if (clusters) {
    // z = M^-1 r outside the direction kernel (SchurClusterCgLaunch).
  } else if (S.preconditioner != CSE_SCHUR_IDENTITY) {
    // The cameras' inverse blocks start at f index f_col_base + 9 lo
    // (cse_schur_precondition).
    const Group::GradPlan& P = ev->groups[0].grad[0];
    a.precond = S.precond.p;
    a.pre_off = S.held ? 0 : S.f_col_base + 9LL * P.lo;
    a.pre_n = S.held ? S.f_cols : 9LL * P.count;
    if (a.pre_off < 0 || a.pre_off + a.pre_n > n || (size_t)(9 * a.pre_n) > S.precond.n)
      return Fail(CSE_ERR_INVALID, "cse_schur_solve: the preconditioner's blocks do not fit the f columns");
  }
  a.state = W.state.p;
  a.params = cse::CgParams{o.min_num_iterations, o.max_num_iterations, o.r_tolerance, o.q_tolerance};
  std::memset(summary, 0, sizeof(*summary));
  if (series)
    rc = CgSolve("cse_schur_solve", SchurSpseCgLaunch{a, ev}, o, W.state_host, ev->stream,
                 [&](const double* x, double* y) { return cse_schur_multiply(ev, x, y); }, summary);
  else if (clusters && d_S_values)
    rc = CgSolve("cse_schur_solve", SchurClusterCgLaunch{a, ev}, o, W.state_host, ev->stream,
                 [&](const double* x, double* y) { return cse_schur_explicit_multiply(ev, d_S_values, x, y); },
                 summary);
  else if (clusters)
    rc = CgSolve("cse_schur_solve", SchurClusterCgLaunch{a, ev}, o, W.state_host, ev->stream,
                 [&](const double* x, double* y) { return cse_schur_multiply(ev, x, y); }, summary);
  else if (d_S_values)
    rc = CgSolve("cse_schur_solve", SchurCgLaunch{a}, o, W.state_host, ev->stream,
                 [&](const double* x, double* y) { return cse_schur_explicit_multiply(ev, d_S_values, x, y); },
                 summary);
  else
    rc = CgSolve("cse_schur_solve", SchurCgLaunch{a}, o, W.state_host, ev->stream,
                 [&](const double* x, double* y) { return cse_schur_multiply(ev, x, y); }, summary);
  if (rc) return rc;
  if (d_step && summary->termination_type != CSE_CG_FAILURE) return cse_schur_back_substitute(ev, d_x, d_step);
  return CSE_OK;
}

int cse_cgnr_init(cse_evaluator* ev, const double* d_jacobian_values, const double* d_D, const double* d_b,
                  double* d_rhs, int preconditioner) {
  int rc = CgnrCheck(ev, "cse_cgnr_init", false);
  if (rc) return rc;
  if (!d_jacobian_values) return Fail(CSE_ERR_INVALID, "cse_cgnr_init: null d_jacobian_values");
  if ((d_b == nullptr) != (d_rhs == nullptr))
    return Fail(CSE_ERR_INVALID, "cse_cgnr_init: d_b and d_rhs go together (both NULL, or both given)");
  if (preconditioner != CSE_CGNR_IDENTITY && preconditioner != CSE_CGNR_JACOBI)
    return Fail(CSE_ERR_INVALID, "cse_cgnr_init: unknown preconditioner");
  auto& C = ev->cgnr;
  if (preconditioner == CSE_CGNR_JACOBI) {
    if (!C.plan.tiles)
      return Fail(CSE_ERR_UNSUPPORTED,
                  "cse_cgnr_init: JACOBI needs the non-constant parameter blocks to tile "
                  "[0, num_effective_parameters) exactly (a gap or an overlap in the delta offsets)");
    if (!C.plan.fits)
      return Fail(CSE_ERR_UNSUPPORTED, "cse_cgnr_init: JACOBI takes blocks of at most " +
                                           std::to_string(cse::kCgnrMaxBlockColumns) +
                                           " tangent columns; the largest here has " +
                                           std::to_string(C.plan.max_size));
  }
  hipStream_t s = ev->stream;
  C.ready = false;
  if (d_rhs) {
    // rhs = J^T b (cgnr_solver.cc:365-367).
    if (ev->num_effective > 0) CSE_HIP(hipMemsetAsync(d_rhs, 0, ev->num_effective * sizeof(double), s));
    if ((rc = JacobianMultiply(ev, d_jacobian_values, d_b, d_rhs, true))) return rc;
  }
  if (preconditioner == CSE_CGNR_JACOBI) {
    if ((rc = CgnrUpload(ev))) return rc;
    // The status word read by cse_wait reports a pivot that is not positive.
    CSE_HIP(hipMemsetAsync(ev->status.p + 1, 0, sizeof(int), s));
    // Zero, then every group adds its cells' J^T J in group order.
    CSE_HIP(hipMemsetAsync(C.values.p, 0, C.values.n * sizeof(double), s));
    for (size_t gi = 0; gi < ev->groups.size(); ++gi) {
      Group& G = ev->groups[gi];
      if (G.n == 0) continue;
      if (GramThroughPlans(ev, gi)) {
        const int sizes[2] = {G.shape.s0, G.shape.s1};
        for (int j = 0; j < G.shape.nb; ++j)
          LaunchGramPass(G.shape.nr, sizes[j], SlotGradArgs(G, j, d_jacobian_values, nullptr, nullptr), G.grad[j],
                         C.values.p + C.value_base[2 * gi + j], C.chunk_partial.p, s);
      } else {
        const bool affine = G.affine && !G.const0;
        if (!affine && !ev->any_general)
          return Fail(CSE_ERR_UNSUPPORTED, "table-path tables were not uploaded");
        const cse::ColumnBlockArgs a = MakeColumnBlockArgs(ev, G, affine);
        hipLaunchKernelGGL(cse::GramBlockKernel, dim3((unsigned)((a.n + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                           dim3(cse::kBlockThreads), 0, s, a, d_jacobian_values, C.blocks.p, C.ntab, C.values.p);
      }
      CSE_HIP(hipGetLastError());
    }
    if (C.ntab > 0) {
      const dim3 grid((unsigned)((C.ntab + cse::kWave - 1) / cse::kWave));
      if (C.plan.max_size > 10)
        hipLaunchKernelGGL(cse::CgnrInvertKernel<true>, grid, dim3(cse::kWave), 0, s, C.blocks.p, C.ntab, d_D,
                           C.values.p, ev->status.p + 1);
      else
        hipLaunchKernelGGL(cse::CgnrInvertKernel<false>, grid, dim3(cse::kWave), 0, s, C.blocks.p, C.ntab, d_D,
                           C.values.p, ev->status.p + 1);
      CSE_HIP(hipGetLastError());
    }
  }
  C.jac = d_jacobian_values;
  C.D = d_D;
  C.preconditioner = preconditioner;
  C.ready = true;
  return CSE_OK;
}

int cse_cgnr_precondition(cse_evaluator* ev, const double* d_x, double* d_y) {
  int rc = CgnrCheck(ev, "cse_cgnr_precondition", true);
  if (rc) return rc;
  if (!d_x || !d_y) return Fail(CSE_ERR_INVALID, "cse_cgnr_precondition: null pointer");
  const int64_t n = ev->num_effective;
  if (d_x < d_y + n && d_y < d_x + n) return Fail(CSE_ERR_INVALID, "cse_cgnr_precondition: x and y overlap");
  const auto& C = ev->cgnr;
  hipStream_t s = ev->stream;
  if (C.preconditioner == CSE_CGNR_IDENTITY) {  // CudaIdentityPreconditioner: y += x
    if (n > 0)
      hipLaunchKernelGGL(cse::AxpyKernel, dim3((unsigned)((n + cse::kBlockThreads - 1) / cse::kBlockThreads)),
                         dim3(cse::kBlockThreads), 0, s, d_x, d_y, n);
  } else {
    cse::LaunchCgnrApplyBlocks(C.blocks.p, C.ntab, C.values.p, d_x, d_y, false, nullptr, s);
  }
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

int cse_cgnr_solve(cse_evaluator* ev, const cse_cg_options* options, const double* d_rhs, double* d_x,
                   cse_cg_summary* summary) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_cgnr_solve");
  int rc = CgArgumentCheck("cse_cgnr_solve", options, d_rhs, d_x, summary);
  if (rc) return rc;
  const cse_cg_options& o = *options;
  if ((rc = CgnrCheck(ev, "cse_cgnr_solve", true))) return rc;
  const int64_t n = ev->num_effective;
  if (d_rhs < d_x + n && d_x < d_rhs + n) return Fail(CSE_ERR_INVALID, "cse_cgnr_solve: d_x overlaps d_rhs");
  auto& C = ev->cgnr;
  auto& W = ev->cg;
  const int64_t nslices = cse::CgSliceCount(n);
  if ((rc = C.vectors.ensure((size_t)4 * (size_t)std::max<int64_t>(n, 1)))) return rc;
  if ((rc = C.partial.ensure((size_t)(2 * nslices)))) return rc;
  if (!C.counter.p) {
    if ((rc = C.counter.alloc(1))) return rc;
    CSE_HIP(hipMemsetAsync(C.counter.p, 0, sizeof(int), ev->stream));
  }
  if ((rc = W.state.ensure(1))) return rc;
  if (!W.state_host) CSE_HIP(hipHostMalloc((void**)&W.state_host, sizeof(cse::CgState)));
  cse::CgSlicedArgs a{};
  a.n = n;
  a.rhs = d_rhs;
  a.x = d_x;
  a.p = C.vectors.p;
  a.r = a.p + n;
  a.z = a.r + n;
  a.tmp = a.z + n;
  a.zr = a.r;
  if (C.preconditioner == CSE_CGNR_JACOBI) {
    a.zr = a.z;
    a.tab = C.blocks.p;
    a.ntab = C.ntab;
    a.precond = C.values.p;
  }
  a.state = W.state.p;
  a.params = cse::CgParams{o.min_num_iterations, o.max_num_iterations, o.r_tolerance, o.q_tolerance};
  a.partial = C.partial.p;
  a.counter = C.counter.p;
  std::memset(summary, 0, sizeof(*summary));
  // CudaCgnrLinearOperator (cgnr_solver.cc:226-237) accumulates: y is zeroed first.
  return CgSolve("cse_cgnr_solve", CgnrCgLaunch{a}, o, W.state_host, ev->stream,
                 [&](const double* x, double* y) -> int {
                   if (n > 0) CSE_HIP(hipMemsetAsync(y, 0, n * sizeof(double), ev->stream));
                   return cse_cgnr_multiply(ev, C.jac, C.D, x, y);
                 },
                 summary);
}

}  // extern "C"
