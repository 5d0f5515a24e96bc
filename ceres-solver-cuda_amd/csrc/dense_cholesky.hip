// dense_cholesky.hip -- cse_dense_cholesky_*: DenseCholesky's device forms
// (dense_cholesky.h:195-302) over the kernels of dense_cholesky_kernels.hpp.
// Built without -ffinite-math-only, as cg_kernels.hip: the pivot test must see
// NaN and Inf.
#include "dense_cholesky_kernels.hpp"
#include "evaluator.hpp"

namespace {

using cse::Fail;
using cse::kDcThreads;

// The workspace's segments (cse::DenseCholeskyPlan's offsets) as pointers.
template <typename T>
struct DcWorkspace {
  T *matrix, *inverse, *v, *y;
  double *x, *r;
  int* flag;
  DcWorkspace(unsigned char* base, const cse::DenseCholeskyPlan& P)
      : matrix(reinterpret_cast<T*>(base + P.matrix_off)),
        inverse(reinterpret_cast<T*>(base + P.inverse_off)),
        v(reinterpret_cast<T*>(base + P.v_off)),
        y(reinterpret_cast<T*>(base + P.y_off)),
        x(reinterpret_cast<double*>(base + P.x_off)),
        r(reinterpret_cast<double*>(base + P.r_off)),
        flag(reinterpret_cast<int*>(base + P.flag_off)) {}
};

dim3 VectorGrid(int64_t entries) { return dim3((unsigned)((entries + kDcThreads - 1) / kDcThreads)); }

// The factorization of M (ld), panel by panel.
template <typename T>
void EnqueueFactor(T* M, int64_t ld, const cse::DenseCholeskyPlan& P, T* inverse, int* flag, hipStream_t s) {
  const dim3 wg(kDcThreads);
  for (int64_t k = 0; k < P.num_panels; ++k) {
    hipLaunchKernelGGL(cse::DcDiagKernel<T>, dim3(1), wg, 0, s, M, ld, P.n, k, inverse, flag);
    const int64_t R = cse::DenseCholeskyRowsBelow(P.num_panels, k);
    if (R == 0) break;
    hipLaunchKernelGGL(cse::DcPanelKernel<T>, dim3((unsigned)R), wg, 0, s, M, ld, P.n, k, (const T*)inverse,
                       (const int*)flag);
    hipLaunchKernelGGL(cse::DcTrailingKernel<T>,
                       dim3((unsigned)cse::DenseCholeskyTrailingGridX(R), (unsigned)cse::DenseCholeskyTrailingGridY(R)),
                       wg, 0, s, M, ld, P.n, k, (const int*)flag);
  }
}

// x = L^-T L^-1 v: v is consumed, y is scratch, the result lands in v.
template <typename T>
void EnqueueSubstitutions(const T* M, int64_t ld, const cse::DenseCholeskyPlan& P, const T* inverse, T* v, T* y,
                          const int* flag, hipStream_t s) {
  const dim3 wg(kDcThreads);
  for (int64_t k = 0; k < P.num_panels; ++k)
    hipLaunchKernelGGL(cse::DcForwardKernel<T>, dim3((unsigned)(P.num_panels - k)), wg, 0, s, M, ld, P.n, k, inverse,
                       v, y, flag);
  for (int64_t k = P.num_panels - 1; k >= 0; --k)
    hipLaunchKernelGGL(cse::DcBackwardKernel<T>, dim3((unsigned)(k + 1)), wg, 0, s, M, ld, P.n, k, inverse, y, v,
                       flag);
}

}  // namespace

extern "C" {

int cse_dense_cholesky_workspace(int64_t n, int32_t precision, int64_t* device_bytes) {
  if (!device_bytes) return Fail(CSE_ERR_INVALID, "cse_dense_cholesky_workspace: null pointer");
  cse::DenseCholeskyPlan P;
  int rc = cse::PlanDenseCholesky(n, precision, &P);
  if (rc) return rc;
  *device_bytes = P.workspace_bytes;
  return CSE_OK;
}

int cse_dense_cholesky_factorize(cse_evaluator* ev, int64_t n, double* d_A, int64_t ld, int32_t precision) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_dense_cholesky_factorize");
  if (!d_A) return Fail(CSE_ERR_INVALID, "cse_dense_cholesky_factorize: null pointer");
  cse::DenseCholeskyPlan P;
  int rc = cse::PlanDenseCholesky(n, precision, &P);
  if (rc) return rc;
  if (ld < n) return Fail(CSE_ERR_INVALID, "cse_dense_cholesky_factorize: ld is smaller than n");
  CSE_HIP(hipSetDevice(ev->device));
  auto& D = ev->dense;
  D.factored = false;
  if ((rc = D.workspace.ensure((size_t)P.workspace_bytes))) {
    (void)hipGetLastError();  // the failed hipMalloc's: the next call's check must not see it
    return rc;
  }
  D.plan = P;
  D.A = d_A;
  D.ld = ld;
  hipStream_t s = ev->stream;
  if (precision == CSE_DENSE_CHOLESKY_FP64) {
    DcWorkspace<double> W(D.workspace.p, P);
    CSE_HIP(hipMemsetAsync(W.flag, 0, cse::kDenseCholeskyAlign, s));
    EnqueueFactor<double>(d_A, ld, P, W.inverse, W.flag, s);
  } else {
    DcWorkspace<float> W(D.workspace.p, P);
    CSE_HIP(hipMemsetAsync(W.flag, 0, cse::kDenseCholeskyAlign, s));
    hipLaunchKernelGGL(cse::DcCastLowerKernel,
                       dim3((unsigned)cse::DenseCholeskyTrailingGridX(P.num_panels),
                            (unsigned)cse::DenseCholeskyTrailingGridY(P.num_panels)),
                       dim3(kDcThreads), 0, s, (const double*)d_A, ld, n, W.matrix);
    EnqueueFactor<float>(W.matrix, n, P, W.inverse, W.flag, s);
  }
  CSE_HIP(hipGetLastError());
  D.factored = true;
  return CSE_OK;
}

int cse_dense_cholesky_solve(cse_evaluator* ev, const double* d_rhs, double* d_x,
                             int32_t max_num_refinement_iterations) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_dense_cholesky_solve");
  if (!d_rhs || !d_x) return Fail(CSE_ERR_INVALID, "cse_dense_cholesky_solve: null pointer");
  if (max_num_refinement_iterations < 0)
    return Fail(CSE_ERR_INVALID, "cse_dense_cholesky_solve: max_num_refinement_iterations is negative");
  auto& D = ev->dense;
  if (!D.factored) return Fail(CSE_ERR_INVALID, "cse_dense_cholesky_solve: no cse_dense_cholesky_factorize before it");
  const cse::DenseCholeskyPlan& P = D.plan;
  const int64_t n = P.n;
  if (d_x != d_rhs && d_x < d_rhs + n && d_rhs < d_x + n)
    return Fail(CSE_ERR_INVALID, "cse_dense_cholesky_solve: d_x overlaps d_rhs partially");
  if (P.precision == CSE_DENSE_CHOLESKY_FP64 && max_num_refinement_iterations != 0)
    return Fail(CSE_ERR_UNSUPPORTED,
                "cse_dense_cholesky_solve: refinement needs an FP32 factorization (the FP64 factor has "
                "overwritten the matrix a residual would read)");
  CSE_HIP(hipSetDevice(ev->device));
  hipStream_t s = ev->stream;
  const dim3 wg(kDcThreads);
  if (P.precision == CSE_DENSE_CHOLESKY_FP64) {
    DcWorkspace<double> W(D.workspace.p, P);
    const int* flag = W.flag;
    hipLaunchKernelGGL(cse::DcLoadKernel, VectorGrid(P.padded), wg, 0, s, d_rhs, n, P.padded, W.v, flag);
    EnqueueSubstitutions<double>(D.A, D.ld, P, W.inverse, W.v, W.y, flag, s);
    hipLaunchKernelGGL(cse::DcStoreKernel, VectorGrid(n), wg, 0, s, (const double*)W.v, n, d_x, flag);
  } else {
    DcWorkspace<float> W(D.workspace.p, P);
    const int* flag = W.flag;
    hipLaunchKernelGGL(cse::DcRefineInitKernel, VectorGrid(P.padded), wg, 0, s, d_rhs, n, P.padded, W.x, W.r, flag);
    for (int32_t i = 0; i <= max_num_refinement_iterations; ++i) {
      hipLaunchKernelGGL(cse::DcCastKernel, VectorGrid(P.padded), wg, 0, s, (const double*)W.r, P.padded, W.v, flag);
      EnqueueSubstitutions<float>(W.matrix, n, P, W.inverse, W.v, W.y, flag, s);
      hipLaunchKernelGGL(cse::DcAccumulateKernel, VectorGrid(P.padded), wg, 0, s, (const float*)W.v, P.padded, W.x,
                         flag);
      if (i < max_num_refinement_iterations)
        hipLaunchKernelGGL(cse::DcResidualKernel, dim3((unsigned)P.num_panels), wg, 0, s, (const double*)D.A, D.ld,
                           n, d_rhs, (const double*)W.x, W.r, flag);
    }
    hipLaunchKernelGGL(cse::DcStoreKernel, VectorGrid(n), wg, 0, s, (const double*)W.x, n, d_x, flag);
  }
  CSE_HIP(hipGetLastError());
  return CSE_OK;
}

int cse_dense_cholesky_info(cse_evaluator* ev, int32_t* info) {
  if (!ev) return Fail(CSE_ERR_INVALID, "null evaluator");
  CSE_SINGLE_DEVICE(ev, "cse_dense_cholesky_info");
  if (!info) return Fail(CSE_ERR_INVALID, "cse_dense_cholesky_info: null pointer");
  auto& D = ev->dense;
  if (!D.factored) return Fail(CSE_ERR_INVALID, "cse_dense_cholesky_info: no cse_dense_cholesky_factorize before it");
  CSE_HIP(hipSetDevice(ev->device));
  int flag = 0;
  CSE_HIP(hipMemcpyAsync(&flag, D.workspace.p + D.plan.flag_off, sizeof(int), hipMemcpyDeviceToHost, ev->stream));
  CSE_HIP(hipStreamSynchronize(ev->stream));
  *info = flag;
  return CSE_OK;
}

}  // extern "C"
