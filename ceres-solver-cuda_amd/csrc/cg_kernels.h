// cg_kernels.h -- the launchers of cse_schur_solve's vector kernels
// (cg_kernels.hpp), a translation unit of their own (cg_kernels.hip): it is
// built without -ffinite-math-only, which the evaluation kernels' unit needs
// and under which ConjugateGradientsSolver's tests for infinite scalars
// (conjugate_gradients_solver.h:116-118, :196, :208) would be folded away.
#ifndef CSE_CG_KERNELS_H_
#define CSE_CG_KERNELS_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cg_state.hpp"

namespace cse {

constexpr int kCgWaves = 16;
constexpr int kCgThreads = kCgWaves * 64;

struct CgArgs {
  int64_t n;          // num_cols_f
  const double* rhs;
  double* x;          // the solution
  double *p, *r, *z, *tmp;  // the reference's four scratch vectors (q is z)
  // The preconditioner: null = IDENTITY, else [pre_n / 9][9][9] inverse blocks
  // for the entries [pre_off, pre_off + pre_n); z = 0 outside them.
  const double* precond;
  int64_t pre_off, pre_n;
  CgState* state;
  CgParams params;
};

enum CgUpdateMode { kCgUpdateFull = 0, kCgUpdateX = 1, kCgUpdateReset = 2 };

// One workgroup each, on stream s.  zero_guess: x = 0, r = rhs, no product.
void LaunchCgInit(const CgArgs& a, bool zero_guess, hipStream_t s);
void LaunchCgInitialResidual(const CgArgs& a, hipStream_t s);
void LaunchCgDirection(const CgArgs& a, hipStream_t s);
void LaunchCgUpdate(CgUpdateMode mode, const CgArgs& a, hipStream_t s);

}  // namespace cse

#endif  // CSE_CG_KERNELS_H_
