// cg_kernels.h -- the launchers of cse_schur_solve's vector kernels
// (cg_kernels.hpp), of cse_schur_power_series' (spse_kernels.hpp) and of
// cse_cgnr_solve's (cg_sliced_kernels.hpp), a
// translation unit of their own (cg_kernels.hip): it is
// built without -ffinite-math-only, which the evaluation kernels' unit needs
// and under which ConjugateGradientsSolver's tests for infinite scalars
// (conjugate_gradients_solver.h:116-118, :196, :208) would be folded away.
#ifndef CSE_CG_KERNELS_H_
#define CSE_CG_KERNELS_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cg_state.hpp"
#include "host_shared.hpp"
#include "spse_state.hpp"

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

// ---- cse_schur_power_series' vector kernels (spse_kernels.hpp), one workgroup
// each as the kernels above.
struct SpseArgs {
  int64_t n;             // num_cols_f
  const double* blocks;  // [pre_n / 9][9][9] inverse blocks of F^T F + D_f^2 for the
  int64_t pre_off, pre_n;  // entries [pre_off, pre_off + pre_n); P^-1 is 0 outside them
  const double* x;       // the zeroth kernel's input
  double* y;             // the series' sum
  double* prev;          // the last term
  const double* t;       // Q prev, what the term kernel applies the blocks to
  SpseState* state;
  int32_t max_num_iterations;
  double tolerance;
};

// y = P^-1 x (accumulate: y += P^-1 x), prev = that term, the state begun.
void LaunchSpseZero(const SpseArgs& a, bool accumulate, hipStream_t s);
// term = P^-1 t, y += term, prev = term, |term| and the stop test; nothing
// once the state is done.
void LaunchSpseTerm(const SpseArgs& a, hipStream_t s);
// CgDirectionKernel with z as given (a preconditioner that wrote a.z itself).
void LaunchCgDirectionGiven(const CgArgs& a, hipStream_t s);

// ---- cse_cgnr_solve's vector kernels (cg_sliced_kernels.hpp): any length, one
// workgroup of kCgSliceThreads lanes per slice of kCgSliceEntries entries.
constexpr int kCgSliceEntries = 2048;
constexpr int kCgSliceWaves = 4;
constexpr int kCgSliceThreads = kCgSliceWaves * 64;

inline int64_t CgSliceCount(int64_t n) { return n > 0 ? (n + kCgSliceEntries - 1) / kCgSliceEntries : 1; }

struct CgSlicedArgs {
  int64_t n;          // num_effective_parameters
  const double* rhs;
  double* x;
  double *p, *r, *z, *tmp;  // the reference's four scratch vectors (q is z)
  const double* zr;   // what the direction kernels read as z: z = M^-1 r, or r under IDENTITY
  CgState* state;
  CgParams params;
  double* partial;    // [2][CgSliceCount(n)]: the slices' partial sums
  int* counter;       // the hand-over counter, 0 between launches
  // The block-Jacobi preconditioner (null tab: IDENTITY).
  const CgnrBlock* tab;
  int64_t ntab;
  const double* precond;
};

void LaunchCgSlicedInit(const CgSlicedArgs& a, bool zero_guess, hipStream_t s);
void LaunchCgSlicedInitialResidual(const CgSlicedArgs& a, hipStream_t s);
// z = M^-1 r (JACOBI), rho and its tests, then p.
void LaunchCgSlicedDirection(const CgSlicedArgs& a, hipStream_t s);
// Full and X: p'q and its tests first.
void LaunchCgSlicedUpdate(CgUpdateMode mode, const CgSlicedArgs& a, hipStream_t s);
// y = M x (assign) or y += M x, one parameter block per lane; state: null, or
// the solve's (nothing is written once it is done).
void LaunchCgnrApplyBlocks(const CgnrBlock* tab, int64_t ntab, const double* values, const double* x,
                           double* y, bool assign, const CgState* state, hipStream_t s);

}  // namespace cse

#endif  // CSE_CG_KERNELS_H_
