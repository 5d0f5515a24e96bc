// sparse_cholesky.hip -- cse_sparse_cholesky_*: the SparseCholesky behind
// SPARSE_SCHUR (sparse_cholesky.h:72-113, schur_complement_solver.cc:290-333)
// over the plan of cse::PlanSparseCholesky and the kernels of
// sparse_cholesky_kernels.hpp.  Built without -ffinite-math-only, as
// cg_kernels.hip: the pivot test must see NaN and Inf.
#include "sparse_cholesky_kernels.hpp"
#include "evaluator.hpp"

namespace {

using cse::Fail;
using cse::kScB;
using cse::kScBlock;
using cse::kScThreads;
using cse::kScWave;
using Sparse = cse_evaluator::SparseCholesky;

dim3 ElementGrid(int64_t entries) { return dim3((unsigned)((entries + kScThreads - 1) / kScThreads)); }

cse::ScFactor FactorArgs(Sparse& S) {
  return cse::ScFactor{S.row_begin.p, S.block_col.p, S.block_row.p, S.col_begin.p, S.col_block.p, S.L.p, S.inverse.p};
}

template <typename T>
int Upload(cse::DevBuf<T>& buf, const std::vector<T>& host, hipStream_t s) {
  return buf.upload(host.data(), host.size(), s);
}

void Release(Sparse& S) {
  S = Sparse{};
}

// y = L^-T L^-1 y, a launch per level each way.
void EnqueueSubstitutions(Sparse& S, hipStream_t s) {
  const cse::SparseCholeskyPlan& P = S.plan;
  const cse::ScFactor F = FactorArgs(S);
  for (int32_t l = 0; l < P.num_levels; ++l) {
    const int64_t b = P.level_begin[(size_t)l], n = P.level_begin[(size_t)l + 1] - b;
    hipLaunchKernelGGL(cse::ScForwardKernel, dim3((unsigned)n), dim3(kScWave), 0, s, F,
                       (const int32_t*)S.level_columns.p + b, S.y.p);
  }
  for (int32_t l = P.num_levels - 1; l >= 0; --l) {
    const int64_t b = P.level_begin[(size_t)l], n = P.level_begin[(size_t)l + 1] - b;
    hipLaunchKernelGGL(cse::ScBackwardKernel, dim3((unsigned)n), dim3(kScWave), 0, s, F,
                       (const int32_t*)S.level_columns.p + b, S.y.p);
  }
}

}  // namespace

extern "C" {

int cse_sparse_cholesky_analyze(cse_evaluator* ev, int64_t num_block_rows, const int64_t* row_begin,
                                const int32_t* block_col, int32_t ordering, const int32_t* permutation,
                                cse_sparse_cholesky_summary* summary) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_sparse_cholesky_analyze");
  cse::SparseCholeskyPlan P;
  int rc = cse::PlanSparseCholesky(num_block_rows, row_begin, block_col, ordering, permutation, &P);
  if (rc) return rc;
  CSE_HIP(hipSetDevice(ev->device));
  Sparse& S = ev->sparse;
  // The factor of the structure before goes with it; work still queued on the
  // old tables ends first.
  CSE_HIP(hipStreamSynchronize(ev->stream));
  Release(S);
  hipStream_t s = ev->stream;
  S.plan = std::move(P);
  const cse::SparseCholeskyPlan& Q = S.plan;
  rc = Upload(S.permutation, Q.permutation, s);
  if (!rc) rc = Upload(S.position, Q.position, s);
  if (!rc) rc = Upload(S.row_begin, Q.row_begin, s);
  if (!rc) rc = Upload(S.block_col, Q.block_col, s);
  if (!rc) rc = Upload(S.block_row, Q.block_row, s);
  if (!rc) rc = Upload(S.col_begin, Q.col_begin, s);
  if (!rc) rc = Upload(S.col_block, Q.col_block, s);
  if (!rc) rc = Upload(S.source, Q.source, s);
  if (!rc) rc = Upload(S.level_columns, Q.level_columns, s);
  if (!rc) rc = Upload(S.level_targets, Q.level_targets, s);
  if (!rc) rc = Upload(S.in_row_begin, Q.in_row_begin, s);
  if (!rc) rc = Upload(S.in_block_col, Q.in_block_col, s);
  if (!rc) rc = Upload(S.in_col_begin, Q.in_col_begin, s);
  if (!rc) rc = Upload(S.in_col_block, Q.in_col_block, s);
  if (!rc) rc = Upload(S.in_col_row, Q.in_col_row, s);
  if (rc) {
    (void)hipGetLastError();  // the failed hipMalloc's: the next call's check must not see it
    (void)hipStreamSynchronize(s);
    Release(S);
    return rc;
  }
  if (hipStreamSynchronize(s) != hipSuccess) {
    Release(S);
    return Fail(CSE_ERR_HIP, "cse_sparse_cholesky_analyze: the upload of the tables failed");
  }
  S.analyzed = true;
  if (summary) {
    summary->num_block_rows = Q.num_block_rows;
    summary->num_input_blocks = Q.num_input_blocks;
    summary->num_factor_blocks = Q.num_factor_blocks;
    summary->num_block_products = Q.num_block_products;
    summary->device_bytes = Q.device_bytes;
    summary->num_levels = Q.num_levels;
    summary->max_level_columns = Q.max_level_columns;
  }
  return CSE_OK;
}

int cse_sparse_cholesky_structure(cse_evaluator* ev, int32_t* permutation, int64_t* factor_row_begin,
                                  int32_t* factor_block_col, int32_t* parent, int32_t* level) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_sparse_cholesky_structure");
  if (!ev->sparse.analyzed)
    return Fail(CSE_ERR_INVALID, "cse_sparse_cholesky_structure: no cse_sparse_cholesky_analyze before it");
  const cse::SparseCholeskyPlan& P = ev->sparse.plan;
  if (permutation) std::copy(P.permutation.begin(), P.permutation.end(), permutation);
  if (factor_row_begin) std::copy(P.row_begin.begin(), P.row_begin.end(), factor_row_begin);
  if (factor_block_col) std::copy(P.block_col.begin(), P.block_col.end(), factor_block_col);
  if (parent) std::copy(P.parent.begin(), P.parent.end(), parent);
  if (level) std::copy(P.level.begin(), P.level.end(), level);
  return CSE_OK;
}

int cse_sparse_cholesky_factorize(cse_evaluator* ev, const double* d_values) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_sparse_cholesky_factorize");
  if (!d_values) return Fail(CSE_ERR_INVALID, "cse_sparse_cholesky_factorize: null pointer");
  Sparse& S = ev->sparse;
  if (!S.analyzed)
    return Fail(CSE_ERR_INVALID, "cse_sparse_cholesky_factorize: no cse_sparse_cholesky_analyze before it");
  CSE_HIP(hipSetDevice(ev->device));
  const cse::SparseCholeskyPlan& P = S.plan;
  const int64_t N = P.num_block_rows;
  S.factored = false;
  int rc = S.L.ensure((size_t)(P.num_factor_blocks * kScBlock));
  if (!rc) rc = S.inverse.ensure((size_t)(N * kScBlock));
  if (!rc) rc = S.y.ensure((size_t)(N * kScB));
  if (!rc) rc = S.x.ensure((size_t)(N * kScB));
  if (!rc) rc = S.status.ensure((size_t)(N + 1));
  if (rc) {
    (void)hipGetLastError();
    return rc;
  }
  S.values = d_values;
  hipStream_t s = ev->stream;
  const int64_t entries = P.num_factor_blocks * kScBlock;
  hipLaunchKernelGGL(cse::ScGatherKernel, ElementGrid(entries), dim3(kScThreads), 0, s, d_values,
                     (const int32_t*)S.source.p, entries, S.L.p);
  const cse::ScFactor F = FactorArgs(S);
  for (int32_t l = 0; l < P.num_levels; ++l) {
    const int64_t cb = P.level_begin[(size_t)l], cn = P.level_begin[(size_t)l + 1] - cb;
    const int64_t tb = P.target_begin[(size_t)l], tn = P.target_begin[(size_t)l + 1] - tb;
    hipLaunchKernelGGL(cse::ScDiagKernel, dim3((unsigned)cn), dim3(kScWave), 0, s, F,
                       (const int32_t*)S.level_columns.p + cb, S.status.p);
    if (tn > 0)
      hipLaunchKernelGGL(cse::ScTargetKernel, dim3((unsigned)tn), dim3(kScWave), 0, s, F,
                         (const int32_t*)S.level_targets.p + tb);
  }
  hipLaunchKernelGGL(cse::ScInfoKernel, dim3(1), dim3(kScThreads), 0, s, (const int*)S.status.p, N, S.status.p + N);
  CSE_HIP(hipGetLastError());
  S.factored = true;
  return CSE_OK;
}

int cse_sparse_cholesky_factor_values(cse_evaluator* ev, double* d_L) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_sparse_cholesky_factor_values");
  if (!d_L) return Fail(CSE_ERR_INVALID, "cse_sparse_cholesky_factor_values: null pointer");
  Sparse& S = ev->sparse;
  if (!S.factored)
    return Fail(CSE_ERR_INVALID, "cse_sparse_cholesky_factor_values: no cse_sparse_cholesky_factorize before it");
  CSE_HIP(hipSetDevice(ev->device));
  CSE_HIP(hipMemcpyAsync(d_L, S.L.p, (size_t)(S.plan.num_factor_blocks * kScBlock) * sizeof(double),
                         hipMemcpyDeviceToDevice, ev->stream));
  return CSE_OK;
}

int cse_sparse_cholesky_solve(cse_evaluator* ev, const double* d_rhs, double* d_x,
                              int32_t max_num_refinement_iterations) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_sparse_cholesky_solve");
  if (!d_rhs || !d_x) return Fail(CSE_ERR_INVALID, "cse_sparse_cholesky_solve: null pointer");
  if (max_num_refinement_iterations < 0)
    return Fail(CSE_ERR_INVALID, "cse_sparse_cholesky_solve: max_num_refinement_iterations is negative");
  Sparse& S = ev->sparse;
  if (!S.factored)
    return Fail(CSE_ERR_INVALID, "cse_sparse_cholesky_solve: no cse_sparse_cholesky_factorize before it");
  const cse::SparseCholeskyPlan& P = S.plan;
  const int64_t n = P.num_block_rows * kScB;
  if (d_x != d_rhs && d_x < d_rhs + n && d_rhs < d_x + n)
    return Fail(CSE_ERR_INVALID, "cse_sparse_cholesky_solve: d_x overlaps d_rhs partially");
  CSE_HIP(hipSetDevice(ev->device));
  hipStream_t s = ev->stream;
  const dim3 wg(kScThreads), grid = ElementGrid(n);
  const int* info = S.status.p + P.num_block_rows;
  const int32_t* perm = S.permutation.p;
  hipLaunchKernelGGL(cse::ScLoadKernel, grid, wg, 0, s, d_rhs, perm, n, S.y.p);
  EnqueueSubstitutions(S, s);
  if (max_num_refinement_iterations == 0) {
    hipLaunchKernelGGL(cse::ScStoreKernel, grid, wg, 0, s, (const double*)S.y.p, perm, n, info, false, d_x);
  } else {
    // SparseIterativeRefiner's loop on a vector of the evaluator's: d_x may be
    // d_rhs, which every residual reads.
    hipLaunchKernelGGL(cse::ScStoreKernel, grid, wg, 0, s, (const double*)S.y.p, perm, n, info, false, S.x.p);
    const cse::ScInput A{S.in_row_begin.p, S.in_block_col.p, S.in_col_begin.p, S.in_col_block.p,
                         S.in_col_row.p,   S.position.p,     S.values};
    for (int32_t i = 0; i < max_num_refinement_iterations; ++i) {
      hipLaunchKernelGGL(cse::ScResidualKernel, dim3((unsigned)P.num_block_rows), dim3(kScWave), 0, s, A, d_rhs,
                         (const double*)S.x.p, S.y.p);
      EnqueueSubstitutions(S, s);
      hipLaunchKernelGGL(cse::ScStoreKernel, grid, wg, 0, s, (const double*)S.y.p, perm, n, info, true, S.x.p);
    }
    hipLaunchKernelGGL(cse::ScStoreKernel, grid, wg, 0, s, (const double*)S.x.p, (const int32_t*)nullptr, n, info,
                       false, d_x);
  }
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

int cse_sparse_cholesky_info(cse_evaluator* ev, int32_t* info) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_sparse_cholesky_info");
  if (!info) return Fail(CSE_ERR_INVALID, "cse_sparse_cholesky_info: null pointer");
  Sparse& S = ev->sparse;
  if (!S.factored)
    return Fail(CSE_ERR_INVALID, "cse_sparse_cholesky_info: no cse_sparse_cholesky_factorize before it");
  CSE_HIP(hipSetDevice(ev->device));
  int flag = 0;
  CSE_HIP(hipMemcpyAsync(&flag, S.status.p + S.plan.num_block_rows, sizeof(int), hipMemcpyDeviceToHost, ev->stream));
  CSE_HIP(hipStreamSynchronize(ev->stream));
  *info = flag;
  return CSE_OK;
}

}  // extern "C"
