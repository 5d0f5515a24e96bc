// cg_state.hpp -- the scalar logic of ConjugateGradientsSolver
// (internal/ceres/conjugate_gradients_solver.h:108-305) as transitions of one
// small struct, in plain C++ for the host and the device alike.
//
// cse_schur_solve keeps this struct in device memory: lane 0 of the vector
// kernels (cg_kernels.hpp) calls a transition after each reduction, the other
// lanes read alpha, beta and `done` from it, and the host only copies it back
// to look at `done`.  tests/cpp/cg_state_driver.cpp drives the same functions
// with host loops.
//
// Once `done` is set every transition returns without touching the state: the
// iterations the host enqueued past the end change nothing (the frozen rule).
#ifndef CSE_CG_STATE_HPP_
#define CSE_CG_STATE_HPP_

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CSE_CG_HD __host__ __device__ inline
#else
#define CSE_CG_HD inline
#endif

namespace cse {

// LinearSolverTerminationType (linear_solver.h:57-74); = cse_cg_termination.
enum CgTermination : int32_t { kCgSuccess = 0, kCgNoConvergence = 1, kCgFailure = 2 };

// The statement of the reference that ended the solve; = cse_cg_reason.
enum CgReason : int32_t {
  kCgMaxIterations = 0,    // :299-301 (and the initial summary, :126-128)
  kCgZeroRhs = 1,          // :131-136  |b| = 0
  kCgInitialResidual = 2,  // :147-152  |r| <= tol_r before the first iteration
  kCgRho = 3,              // :168-172  rho = r'z is 0 or infinite
  kCgBeta = 4,             // :178-187  beta is 0 or infinite
  kCgIndefinite = 5,       // :196-205  p'q <= 0 or infinite
  kCgAlpha = 6,            // :208-216  alpha is infinite
  kCgQTolerance = 7,       // :273-283  zeta < q_tolerance
  kCgRTolerance = 8        // :288-297  |r| <= tol_r
};

// The options the transitions read (ConjugateGradientsSolverOptions).
struct CgParams {
  int32_t min_num_iterations;
  int32_t max_num_iterations;
  double r_tolerance;
  double q_tolerance;
};

struct CgState {
  double rho, last_rho, pq, alpha, beta, Q0, Q1, norm_rhs, norm_r, zeta;
  int32_t iteration;  // summary.num_iterations
  int32_t termination_type, reason;
  int32_t done;
};

// std::isinf, spelled with the bits.  A unit built with -ffinite-math-only
// folds either spelling to false when it sees the sum that made x, which is
// why the kernels that call these transitions have a unit of their own
// (cg_kernels.h).
CSE_CG_HD bool CgIsInfinity(double x) {
  return (__builtin_bit_cast(uint64_t, x) & 0x7fffffffffffffffull) == 0x7ff0000000000000ull;
}

CSE_CG_HD bool CgIsZeroOrInfinity(double x) { return x == 0.0 || CgIsInfinity(x); }  // :116-118

CSE_CG_HD void CgStop(CgState* s, int32_t type, int32_t reason) {
  s->termination_type = type;
  s->reason = reason;
  s->done = 1;
}

// :125-136.  Returns true when the solve goes on; on false (|b| = 0) the
// caller sets the solution to zero.
CSE_CG_HD bool CgBegin(CgState* s, double norm_rhs) {
  s->rho = s->last_rho = s->pq = s->alpha = s->beta = 0.0;
  s->Q0 = s->Q1 = s->norm_r = s->zeta = 0.0;
  s->norm_rhs = norm_rhs;
  s->iteration = 0;
  s->termination_type = kCgNoConvergence;
  s->reason = kCgMaxIterations;
  s->done = 0;
  if (norm_rhs == 0.0) {
    CgStop(s, kCgSuccess, kCgZeroRhs);
    return false;
  }
  return true;
}

// :146-159, after r = rhs - A x: norm_r = |r|, x_dot = x'(rhs + r).
CSE_CG_HD void CgInitialResidual(CgState* s, const CgParams& o, double norm_r, double x_dot) {
  if (s->done) return;
  const double tol_r = o.r_tolerance * s->norm_rhs;
  s->norm_r = norm_r;
  if (o.min_num_iterations == 0 && norm_r <= tol_r) {
    CgStop(s, kCgSuccess, kCgInitialResidual);
    return;
  }
  s->rho = 1.0;
  s->Q0 = -x_dot;
}

// :161-190, after z = M^-1 r: rho = r'z.  Starts iteration
// summary.num_iterations.  Returns true when p is to be updated: p = z in
// iteration 1, p = z + beta p after it.
CSE_CG_HD bool CgDirection(CgState* s, double rho) {
  if (s->done) return false;
  s->iteration += 1;
  s->last_rho = s->rho;
  s->rho = rho;
  if (CgIsZeroOrInfinity(rho)) {
    CgStop(s, kCgFailure, kCgRho);
    return false;
  }
  if (s->iteration == 1) return true;
  s->beta = s->rho / s->last_rho;
  if (CgIsZeroOrInfinity(s->beta)) {
    CgStop(s, kCgFailure, kCgBeta);
    return false;
  }
  return true;
}

// :195-216, after q = A p: pq = p'q.  Returns true when x (and r) are to be
// updated with alpha.
CSE_CG_HD bool CgStep(CgState* s, double pq) {
  if (s->done) return false;
  s->pq = pq;
  if (pq <= 0 || CgIsInfinity(pq)) {
    CgStop(s, kCgNoConvergence, kCgIndefinite);
    return false;
  }
  s->alpha = s->rho / pq;
  if (CgIsInfinity(s->alpha)) {
    CgStop(s, kCgFailure, kCgAlpha);
    return false;
  }
  return true;
}

// :244-301, after the updates of x and r: x_dot = x'(rhs + r), r_dot = r'r.
// norm_r is stored before the quadratic test (the reference computes it there
// for its message only).
CSE_CG_HD void CgTests(CgState* s, const CgParams& o, double x_dot, double r_dot) {
  if (s->done) return;
  const double tol_r = o.r_tolerance * s->norm_rhs;
  s->Q1 = -x_dot;
  s->norm_r = std::sqrt(r_dot);
  s->zeta = s->iteration * (s->Q1 - s->Q0) / s->Q1;
  if (s->zeta < o.q_tolerance && s->iteration >= o.min_num_iterations) {
    CgStop(s, kCgSuccess, kCgQTolerance);
    return;
  }
  s->Q0 = s->Q1;
  if (s->norm_r <= tol_r && s->iteration >= o.min_num_iterations) {
    CgStop(s, kCgSuccess, kCgRTolerance);
    return;
  }
  if (s->iteration >= o.max_num_iterations) CgStop(s, kCgNoConvergence, kCgMaxIterations);
}

}  // namespace cse

#endif  // CSE_CG_STATE_HPP_
