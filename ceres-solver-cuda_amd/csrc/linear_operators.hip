// linear_operators.hip -- the Jacobian-level calls of the C ABI (include/cse.h)
// that a linear solver makes on the evaluator (evaluator.hpp): J x, J^T x and
// CGNR's normal operator (operator_kernels.hpp), the column norms and
// ScaleColumns (column_kernels.hpp), and CGNR on the device (cgnr_kernels.hpp,
// cg_solve.hpp; the vector kernels through cg_kernels.h).  The cse_schur_*
// calls are schur_operators.hip's.  The gradient post-pass kernels are
// launched through evaluator.hpp's functions: they stay instantiated in
// cse_evaluator.hip.
#include <algorithm>
#include <cstring>
#include <new>
#include <type_traits>
#include <utility>

#include "cg_solve.hpp"
#include "cgnr_kernels.hpp"
#include "column_kernels.hpp"
#include "kernel_pickers.hpp"

namespace {

using cse::Blocks;
using cse::CgArgumentCheck;
using cse::CgSolve;
using cse::Chunks;
using cse::Fail;
using cse::Group;
using cse::kOperatorWavesPerWg;

// What every entry point here checks first, in this order.
int LayoutCheck(cse_evaluator* ev, const char* what) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, what);
  if (!ev->has_layout) return Fail(CSE_ERR_INVALID, "the descriptor had no Jacobian layout");
  return CSE_OK;
}

// pointers: every pointer argument of the call is given.
int OperandCheck(cse_evaluator* ev, const char* what, bool pointers) {
  const int rc = LayoutCheck(ev, what);
  if (rc) return rc;
  if (!pointers) return Fail(CSE_ERR_INVALID, "null pointer");
  CSE_HIP(hipSetDevice(ev->device));
  return CSE_OK;
}

bool DispatchMultiply(int kind, const cse::GroupArgs& a, bool affine, bool left, const double* x,
                      double* y, hipStream_t s) {
  const int which = affine && !left ? 0 : left ? 2 : 1;
  return cse::VisitKind(kind, [&](auto kd) { cse::LaunchMultiplyKernel<decltype(kd)>(a, which, x, y, s); });
}

int JacobianMultiply(cse_evaluator* ev, const double* J, const double* x, double* y, bool left) {
  const int rc = OperandCheck(ev, "cse_jacobian_multiply", J && x && y);
  if (rc) return rc;
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
// Every shape a slot of an affine group can have (DetectAffine: at most 3
// residuals) with blocks of up to 10 columns: calls f(NR, S), both as
// std::integral_constant<int, .>, for nr in 1..3 and size in 1..10; false, and
// no call, for any other.  What f instantiates exists for these 30 shapes.
template <class F, int... I>
bool VisitSlotShapeAt(int index, F&& f, std::integer_sequence<int, I...>) {
  return ((index == I &&
           (f(std::integral_constant<int, I / 10 + 1>{}, std::integral_constant<int, I % 10 + 1>{}), true)) ||
          ...);
}

template <class F>
bool VisitSlotShape(int nr, int size, F&& f) {
  if (nr < 1 || nr > 3 || size < 1 || size > 10) return false;
  return VisitSlotShapeAt(10 * (nr - 1) + size - 1, f, std::make_integer_sequence<int, 30>{});
}

bool ColumnNormShape(int nr, int size) {
  return VisitSlotShape(nr, size, [](auto, auto) {});
}

// The norm of slot j through its gradient plan, in the plan's form (as
// LaunchGradientSlot): identity order = contiguous block ranges; chunks of at
// most kGradChunk blocks and the ordered chunk reduce; one lane per parameter
// block.  P.chunk_partial is the plan's own (nchunks x S).
template <int NR, int S>
void LaunchColumnNormSlot(const cse::GradArgs& ga, const Group::GradPlan& P, hipStream_t s) {
  if (ga.count <= 0) return;
  if (ga.perm == nullptr) {
    hipLaunchKernelGGL((cse::ColumnNormRangeKernel<NR, S>), Blocks(ga.count, cse::kWave), dim3(cse::kWave), 0, s, ga);
  } else if (P.wave) {
    const cse::GradChunks ch{P.chunk_begin.p, P.chunk_off.p, P.chunk_partial.p, P.nchunks};
    if (P.nchunks > 0)
      hipLaunchKernelGGL((cse::ColumnNormLanesKernel<NR, S>), Blocks(P.nchunks, cse::kWavesPerBlock),
                         dim3(cse::kBlockThreads), 0, s, ga, ch);
    hipLaunchKernelGGL((cse::ColumnNormChunkReduceKernel<S>), Blocks(ga.count), dim3(cse::kBlockThreads), 0, s, ga,
                       ch);
  } else {
    hipLaunchKernelGGL((cse::ColumnNormSlotKernel<NR, S>), Blocks(ga.count), dim3(cse::kBlockThreads), 0, s, ga);
  }
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
  hipLaunchKernelGGL((cse::ColumnBlockKernel<kScale>), Blocks(a.n), dim3(cse::kBlockThreads), 0, s, a, jac, scale,
                     out);
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
// CGNR on the device: the block-Jacobi preconditioner (cgnr_kernels.hpp) and
// cse_cgnr_solve (cg_solve.hpp; cg_sliced_kernels.hpp through cg_kernels.h)
// ---------------------------------------------------------------------------
// The Gram of slot j through its gradient plan, in the plan's form (as
// LaunchColumnNormSlot).  values: the S x S block of the plan's first
// parameter block; partial: cse_cgnr_init's own chunk partials.
template <int NR, int S>
void LaunchGramSlot(const cse::GradArgs& ga, const Group::GradPlan& P, double* values, double* partial,
                    hipStream_t s) {
  if (ga.count <= 0) return;
  if (ga.perm == nullptr) {
    hipLaunchKernelGGL((cse::GramRangeKernel<NR, S>), Blocks(ga.count, cse::kWave), dim3(cse::kWave), 0, s, ga,
                       values);
  } else if (P.wave) {
    const cse::GradChunks ch{P.chunk_begin.p, P.chunk_off.p, partial, P.nchunks};
    if (P.nchunks > 0)
      hipLaunchKernelGGL((cse::GramLanesKernel<NR, S>), Blocks(P.nchunks, cse::kWavesPerBlock),
                         dim3(cse::kBlockThreads), 0, s, ga, ch);
    hipLaunchKernelGGL((cse::GramChunkReduceKernel<S>), Blocks(ga.count), dim3(cse::kBlockThreads), 0, s, ga, ch,
                       values);
  } else {
    hipLaunchKernelGGL((cse::GramSlotKernel<NR, S>), Blocks(ga.count), dim3(cse::kBlockThreads), 0, s, ga, values);
  }
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
  const int rc = LayoutCheck(ev, what);
  if (rc) return rc;
  if (need_ready && !ev->cgnr.ready) return Fail(CSE_ERR_INVALID, std::string(what) + ": cse_cgnr_init has not run");
  CSE_HIP(hipSetDevice(ev->device));
  return CSE_OK;
}

// cg_sliced_kernels.hpp's kernels over their arguments (CgSolve's Launch).
struct CgnrCgLaunch {
  cse::CgSlicedArgs a;
  void Init(bool zero_guess, hipStream_t s) const { cse::LaunchCgSlicedInit(a, zero_guess, s); }
  void InitialResidual(hipStream_t s) const { cse::LaunchCgSlicedInitialResidual(a, s); }
  void Direction(hipStream_t s) const { cse::LaunchCgSlicedDirection(a, s); }
  void Update(cse::CgUpdateMode mode, hipStream_t s) const { cse::LaunchCgSlicedUpdate(mode, a, s); }
};

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
  int rc = OperandCheck(ev, "cse_cgnr_multiply", d_jacobian_values && d_x && d_y);
  if (rc) return rc;
  hipStream_t s = ev->stream;
  if (d_D && ev->num_effective > 0)
    hipLaunchKernelGGL(cse::DtDxpyKernel, Blocks(ev->num_effective), dim3(cse::kBlockThreads), 0, s, d_D, d_x, d_y,
                       ev->num_effective);
  bool fused = true;
  for (auto& G : ev->groups) fused = fused && (G.n == 0 || (G.fuse_ok && !G.const0 && SnavelyShaped(G)));
  if (!fused) {
    // z = J x, then y += J^T z: the two products of CudaCgnrLinearOperator.
    if ((rc = ev->cg_z.ensure((size_t)std::max<int64_t>(ev->num_residuals, 1)))) return rc;
    CSE_HIP(hipMemsetAsync(ev->cg_z.p, 0, ev->num_residuals * sizeof(double), s));
    if ((rc = JacobianMultiply(ev, d_jacobian_values, d_x, ev->cg_z.p, false))) return rc;
    return JacobianMultiply(ev, d_jacobian_values, ev->cg_z.p, d_y, true);
  }
  for (auto& G : ev->groups) {
    if (G.n == 0) continue;
    const int64_t chunks = Chunks(G.n);
    if ((rc = G.gside.ensure((size_t)(2 * chunks * 4)))) return rc;
    if ((rc = G.gcontrib.ensure((size_t)G.n * G.slot0_stride))) return rc;
    cse::GroupArgs a = MakeArgs(ev, G, nullptr, nullptr, const_cast<double*>(d_jacobian_values),
                                nullptr);
    a.gside = G.gside.p;
    a.gcontrib = G.gcontrib.p;
    constexpr int W = kOperatorWavesPerWg;
    if (G.policy == cse::kAffineCrs)
      hipLaunchKernelGGL((cse::CgnrMultiplyKernel<cse::SnavelyKind, true, W>), Blocks(chunks, W),
                         dim3(W * cse::kWave), 0, s, a, d_x, d_y);
    else
      hipLaunchKernelGGL((cse::CgnrMultiplyKernel<cse::SnavelyKind, false, W>), Blocks(chunks, W),
                         dim3(W * cse::kWave), 0, s, a, d_x, d_y);
    CSE_HIP(hipGetLastError());
    if ((rc = LaunchFusedGradTail(G, d_y, s))) return rc;
  }
  return CSE_OK;
}

int cse_jacobian_squared_column_norm(cse_evaluator* ev, const double* d_jacobian_values, double* d_x) {
  int rc = OperandCheck(ev, "cse_jacobian_squared_column_norm", d_jacobian_values && d_x);
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
      for (int j = 0; j < G.shape.nb; ++j) {
        const cse::GradArgs ga = SlotGradArgs(G, j, d_jacobian_values, nullptr, d_x);
        VisitSlotShape(G.shape.nr, sizes[j], [&](auto nr, auto size) {
          LaunchColumnNormSlot<decltype(nr)::value, decltype(size)::value>(ga, G.grad[j], s);
        });
      }
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
  int rc = OperandCheck(ev, "cse_jacobian_scale_columns", d_jacobian_values && d_scale);
  if (rc) return rc;
  hipStream_t s = ev->stream;
  for (auto& G : ev->groups) {
    if (G.n == 0) continue;
    if (G.affine && !G.const0) {
      const cse::ScaleStreamArgs a = MakeScaleStreamArgs(G);
      constexpr int W = kOperatorWavesPerWg;
      hipLaunchKernelGGL((cse::ScaleColumnsStreamKernel<W>), Blocks(Chunks(G.n), W), dim3(W * cse::kWave),
                         (size_t)W * cse::kWave * a.ntab * sizeof(double), s, a, d_jacobian_values, d_scale);
    } else {
      // Held cameras (compacted F cells, two row widths) and the table path.
      if (!ev->any_general) return Fail(CSE_ERR_UNSUPPORTED, "table-path tables were not uploaded");
      LaunchColumnBlocks<true>(MakeColumnBlockArgs(ev, G, false), d_jacobian_values, d_scale, nullptr, s);
    }
    CSE_HIP(hipGetLastError());
  }
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
        for (int j = 0; j < G.shape.nb; ++j) {
          const cse::GradArgs ga = SlotGradArgs(G, j, d_jacobian_values, nullptr, nullptr);
          VisitSlotShape(G.shape.nr, sizes[j], [&](auto nr, auto size) {
            LaunchGramSlot<decltype(nr)::value, decltype(size)::value>(
                ga, G.grad[j], C.values.p + C.value_base[2 * gi + j], C.chunk_partial.p, s);
          });
        }
      } else {
        const bool affine = G.affine && !G.const0;
        if (!affine && !ev->any_general)
          return Fail(CSE_ERR_UNSUPPORTED, "table-path tables were not uploaded");
        const cse::ColumnBlockArgs a = MakeColumnBlockArgs(ev, G, affine);
        hipLaunchKernelGGL(cse::GramBlockKernel, Blocks(a.n), dim3(cse::kBlockThreads), 0, s, a, d_jacobian_values,
                           C.blocks.p, C.ntab, C.values.p);
      }
      CSE_HIP(hipGetLastError());
    }
    if (C.ntab > 0) {
      const dim3 grid = Blocks(C.ntab, cse::kWave);
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
    if (n > 0) cse::LaunchAxpy(d_x, d_y, n, s);
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
