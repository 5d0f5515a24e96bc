// cg_state_driver.cpp -- the transitions of csrc/cg_state.hpp on the host,
// under AddressSanitizer + UBSan (tests/test_schur_solve.py, cg_state.mk).
//
// 1. Plain host loops drive the transitions in the order cse_schur_solve's
//    kernels do (cg_kernels.hpp) on small dense SPD systems -- the two known
//    answers of conjugate_gradients_solver_test.cc:47-152 among them -- and the
//    results are compared with closed-form solutions.
// 2. Crafted scalars go through every branch of
//    conjugate_gradients_solver.h:116-301; the termination type, reason and
//    iteration count are the ones the reference's text gives.
// 3. After `done`, further transitions change nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../ceres-solver-cuda_amd/csrc/cg_state.hpp"

using cse::CgParams;
using cse::CgState;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

namespace {

using Vec = std::vector<double>;
const double kInf = std::numeric_limits<double>::infinity();

double Dot(const Vec& a, const Vec& b) {
  double s = 0.0;
  for (size_t i = 0; i < a.size(); ++i) s += a[i] * b[i];
  return s;
}

struct System {
  int n;
  Vec A;       // row-major
  Vec minv;    // diagonal preconditioner's inverse; empty: identity
  void Multiply(const Vec& x, Vec* y) const {
    for (int i = 0; i < n; ++i) {
      double s = 0.0;
      for (int j = 0; j < n; ++j) s += A[(size_t)i * n + j] * x[j];
      (*y)[i] = s;
    }
  }
};

struct Options {
  CgParams params;
  int reset_period;
  bool zero_guess;
};

// The sequence of cse_schur_solve: CgInitKernel, (product,
// CgInitialResidualKernel), then per iteration CgDirectionKernel, product,
// CgUpdateKernel -- `extra` more iterations are driven past the end, as a
// check_period above 1 enqueues them.
CgState Solve(const System& S, const Vec& b, Vec* x, const Options& o, int extra = 0) {
  const int n = S.n;
  Vec p(n, NAN), r(n, NAN), z(n, NAN), tmp(n, NAN);
  CgState st;
  std::memset(&st, 0xab, sizeof(st));
  const double norm_rhs = std::sqrt(Dot(b, b));
  if (!cse::CgBegin(&st, norm_rhs)) {
    for (double& v : *x) v = 0.0;
  } else if (o.zero_guess) {
    for (double& v : *x) v = 0.0;
    r = b;
    cse::CgInitialResidual(&st, o.params, norm_rhs, 0.0);
  }
  if (!o.zero_guess && !st.done) {
    S.Multiply(*x, &tmp);
    double xd = 0.0, rd = 0.0;
    for (int i = 0; i < n; ++i) {
      r[i] = b[i] - tmp[i];
      xd += (*x)[i] * (b[i] + r[i]);
      rd += r[i] * r[i];
    }
    cse::CgInitialResidual(&st, o.params, std::sqrt(rd), xd);
  }
  int budget = -1;
  for (int it = 1; it <= o.params.max_num_iterations; ++it) {
    if (st.done && budget < 0) budget = extra;
    if (st.done && budget-- == 0) break;
    // direction
    if (!st.done) {
      for (int i = 0; i < n; ++i) z[i] = S.minv.empty() ? r[i] : S.minv[i] * r[i];
      if (cse::CgDirection(&st, Dot(r, z))) {
        for (int i = 0; i < n; ++i) p[i] = st.iteration == 1 ? z[i] : z[i] + st.beta * p[i];
      }
    } else {
      CHECK(!cse::CgDirection(&st, 123.0));
    }
    S.Multiply(p, &z);  // the operator runs whatever the state: scratch only
    // update
    if (st.done) {
      CHECK(!cse::CgStep(&st, 1.0));
      cse::CgTests(&st, o.params, 1.0, 1.0);
      continue;
    }
    if (!cse::CgStep(&st, Dot(p, z))) continue;
    double xd = 0.0, rd = 0.0;
    const bool reset = it % o.reset_period == 0;
    for (int i = 0; i < n; ++i) (*x)[i] = (*x)[i] + st.alpha * p[i];
    if (reset) S.Multiply(*x, &tmp);
    for (int i = 0; i < n; ++i) {
      r[i] = reset ? b[i] - tmp[i] : r[i] - st.alpha * z[i];
      xd += (*x)[i] * (b[i] + r[i]);
      rd += r[i] * r[i];
    }
    cse::CgTests(&st, o.params, xd, rd);
  }
  return st;
}

Options MakeOptions(int min_it, int max_it, int reset, double r_tol, double q_tol, bool zero) {
  return Options{CgParams{min_it, max_it, r_tol, q_tol}, reset, zero};
}

void KnownAnswers() {
  // Solves3x3IdentitySystem
  {
    System S{3, {1, 0, 0, 0, 1, 0, 0, 0, 1}, {}};
    Vec b{1, 2, 3}, x{1, 1, 1};
    const CgState st = Solve(S, b, &x, MakeOptions(1, 10, 20, 1e-9, 0.0, false));
    CHECK(st.termination_type == cse::kCgSuccess && st.iteration == 1);
    CHECK(st.reason == cse::kCgRTolerance);
    CHECK(x[0] == 1.0 && x[1] == 2.0 && x[2] == 3.0);
  }
  // Solves3x3SymmetricSystem
  for (int extra : {0, 5}) {
    System S{3, {2, -1, 0, -1, 2, -1, 0, -1, 2}, {}};
    Vec b{-1, 0, 3}, x{1, 1, 1};
    const CgState st = Solve(S, b, &x, MakeOptions(1, 10, 20, 1e-9, 0.0, false), extra);
    CHECK(st.termination_type == cse::kCgSuccess && st.done);
    CHECK(std::fabs(x[0]) <= 1e-15 && std::fabs(x[1] - 1.0) <= 1e-15 && std::fabs(x[2] - 2.0) <= 1e-15);
  }
}

void ClosedForms() {
  // A diagonal system: x_i = b_i / d_i after at most n iterations.
  {
    const int n = 5;
    System S{n, Vec(n * n, 0.0), {}};
    Vec b(n), x(n, NAN);
    for (int i = 0; i < n; ++i) S.A[i * n + i] = 1.0 + i, b[i] = 2.0 * i - 3.0;
    const CgState st = Solve(S, b, &x, MakeOptions(1, 50, 3, 1e-13, 0.0, true));
    CHECK(st.termination_type == cse::kCgSuccess && st.reason == cse::kCgRTolerance);
    CHECK(st.iteration <= n + 1);
    for (int i = 0; i < n; ++i) CHECK(std::fabs(x[i] - b[i] / (1.0 + i)) <= 1e-12);
    // ... and in one iteration with its own inverse as the preconditioner
    System P = S;
    P.minv.resize(n);
    for (int i = 0; i < n; ++i) P.minv[i] = 1.0 / (1.0 + i);
    Vec y(n, NAN);
    const CgState sp = Solve(P, b, &y, MakeOptions(1, 50, 10, 1e-13, 0.0, true));
    CHECK(sp.termination_type == cse::kCgSuccess && sp.iteration == 1);
    for (int i = 0; i < n; ++i) CHECK(std::fabs(y[i] - b[i] / (1.0 + i)) <= 1e-14);
  }
  // tridiag(-1, 2, -1), b = A (1, 2, .., n): integers, so b is exact.
  for (int reset : {2, 100}) {
    const int n = 8;
    System S{n, Vec(n * n, 0.0), {}};
    for (int i = 0; i < n; ++i) {
      S.A[i * n + i] = 2.0;
      if (i > 0) S.A[i * n + i - 1] = -1.0;
      if (i + 1 < n) S.A[i * n + i + 1] = -1.0;
    }
    Vec want(n), b(n), x(n, 0.5);
    for (int i = 0; i < n; ++i) want[i] = i + 1.0;
    S.Multiply(want, &b);
    const CgState st = Solve(S, b, &x, MakeOptions(1, 100, reset, 1e-13, 0.0, false), 3);
    CHECK(st.termination_type == cse::kCgSuccess && st.iteration <= n + 2);
    for (int i = 0; i < n; ++i) CHECK(std::fabs(x[i] - want[i]) <= 1e-11);
  }
  // The quadratic test alone (r_tolerance -1): Ceres' LM setting stops early.
  // diag(1, 2), b = (1, 1) from zero: Q_1 = -4/3 (zeta 1), Q_2 = -3/2 at the
  // exact solution (1, 1/2), zeta = 2 (Q_2 - Q_1) / Q_2 = 2/9 < 1/4.
  {
    System S{2, {1, 0, 0, 2}, {}};
    Vec b{1, 1}, x{NAN, NAN};
    const CgState st = Solve(S, b, &x, MakeOptions(1, 50, 10, -1.0, 0.25, true));
    CHECK(st.termination_type == cse::kCgSuccess && st.reason == cse::kCgQTolerance);
    CHECK(st.iteration == 2 && std::fabs(st.zeta - 2.0 / 9.0) <= 1e-14);
    CHECK(std::fabs(st.Q1 + 1.5) <= 1e-15 && std::fabs(x[0] - 1.0) <= 1e-15 && std::fabs(x[1] - 0.5) <= 1e-15);
  }
  // A negative definite matrix: indefinite at iteration 1, x unchanged.
  {
    System S{2, {-1, 0, 0, -2}, {}};
    Vec b{1, 1}, x{0.25, -0.5};
    const CgState st = Solve(S, b, &x, MakeOptions(1, 10, 10, 1e-9, 0.0, false), 2);
    CHECK(st.termination_type == cse::kCgNoConvergence && st.reason == cse::kCgIndefinite);
    CHECK(st.iteration == 1 && x[0] == 0.25 && x[1] == -0.5);
  }
  // rhs = 0: SUCCESS, no iteration, x assigned zero.
  {
    System S{2, {1, 0, 0, 1}, {}};
    Vec b{0, 0}, x{NAN, NAN};
    const CgState st = Solve(S, b, &x, MakeOptions(1, 10, 10, 1e-9, 0.0, false), 2);
    CHECK(st.termination_type == cse::kCgSuccess && st.reason == cse::kCgZeroRhs && st.iteration == 0);
    CHECK(x[0] == 0.0 && x[1] == 0.0);
  }
}

// A state inside iteration `it` - 1's end: begun, not converged.
CgState Started(const CgParams& o, double norm_rhs = 2.0) {
  CgState s;
  std::memset(&s, 0xcd, sizeof(s));
  CHECK(cse::CgBegin(&s, norm_rhs));
  cse::CgInitialResidual(&s, o, norm_rhs, 0.0);
  CHECK(!s.done && s.rho == 1.0 && s.iteration == 0);
  return s;
}

void Expect(const CgState& s, int type, int reason, int iteration) {
  CHECK(s.done == 1);
  CHECK(s.termination_type == type);
  CHECK(s.reason == reason);
  CHECK(s.iteration == iteration);
}

void Branches() {
  const CgParams o{1, 10, -1.0, 0.0};
  // :116-118
  CHECK(cse::CgIsZeroOrInfinity(0.0) && cse::CgIsZeroOrInfinity(-0.0));
  CHECK(cse::CgIsZeroOrInfinity(kInf) && cse::CgIsZeroOrInfinity(-kInf));
  CHECK(!cse::CgIsZeroOrInfinity(1e-320) && !cse::CgIsZeroOrInfinity(NAN) && !cse::CgIsZeroOrInfinity(-3.0));
  // rho 0 and infinite (:168-172)
  for (double rho : {0.0, kInf, -kInf}) {
    CgState s = Started(o);
    CHECK(!cse::CgDirection(&s, rho));
    Expect(s, cse::kCgFailure, cse::kCgRho, 1);
  }
  // iteration 1 has no beta test: last_rho is the initial 1
  {
    CgState s = Started(o);
    CHECK(cse::CgDirection(&s, 1e300));
    CHECK(!s.done && s.iteration == 1 && s.last_rho == 1.0);
  }
  // beta 0 and infinite (:178-187), in iteration 2
  for (int which = 0; which < 2; ++which) {
    CgState s = Started(o);
    CHECK(cse::CgDirection(&s, which ? 1e-300 : 1e300));
    CHECK(cse::CgStep(&s, 1.0));
    cse::CgTests(&s, o, 1.0, 1.0);  // Q1 = -1, zeta = 1: goes on
    CHECK(!s.done && s.zeta == 1.0 && s.Q0 == -1.0);
    CHECK(!cse::CgDirection(&s, which ? 1e300 : 1e-300));
    CHECK(which ? s.beta == kInf : s.beta == 0.0);
    Expect(s, cse::kCgFailure, cse::kCgBeta, 2);
  }
  // pq <= 0 and infinite (:196-205)
  for (double pq : {0.0, -1.0, kInf, -kInf}) {
    CgState s = Started(o);
    CHECK(cse::CgDirection(&s, 2.0));
    CHECK(!cse::CgStep(&s, pq));
    Expect(s, cse::kCgNoConvergence, cse::kCgIndefinite, 1);
  }
  // alpha infinite (:208-216)
  {
    CgState s = Started(o);
    CHECK(cse::CgDirection(&s, 1e300));
    CHECK(!cse::CgStep(&s, 1e-300));
    CHECK(s.alpha == kInf);
    Expect(s, cse::kCgFailure, cse::kCgAlpha, 1);
  }
  // |b| = 0 (:131-136)
  {
    CgState s;
    std::memset(&s, 0xcd, sizeof(s));
    CHECK(!cse::CgBegin(&s, 0.0));
    Expect(s, cse::kCgSuccess, cse::kCgZeroRhs, 0);
  }
  // convergence before the first iteration needs min_num_iterations 0 (:147-152)
  for (int min_it : {0, 1}) {
    const CgParams p{min_it, 10, 1e-6, 0.0};
    CgState s;
    CHECK(cse::CgBegin(&s, 2.0));
    cse::CgInitialResidual(&s, p, 1e-6, 0.0);  // <= 1e-6 * 2
    if (min_it == 0) {
      Expect(s, cse::kCgSuccess, cse::kCgInitialResidual, 0);
    } else {
      CHECK(!s.done && s.rho == 1.0);
    }
  }
  // both tolerances held back by min_num_iterations (:273-297): the quadratic
  // test comes first once the iteration count allows it
  for (int which = 0; which < 2; ++which) {
    const CgParams p{3, 10, 0.5, which == 0 ? 0.1 : 0.0};
    CgState s = Started(p);
    for (int it = 1; it <= 3; ++it) {
      CHECK(cse::CgDirection(&s, 1.0));
      CHECK(cse::CgStep(&s, 1.0));
      // Q goes -1, -1.01, -1.0201: zeta = it * 0.01 / 1.01 < 0.1; |r| = 0.1 <= 0.5 * 2
      cse::CgTests(&s, p, std::pow(1.01, it - 1), 0.01);
      if (it < 3) CHECK(!s.done);
      if (it == 2) CHECK(s.zeta > 0.0 && s.zeta < 0.1 && s.norm_r <= 1.0);
    }
    Expect(s, cse::kCgSuccess, which == 0 ? cse::kCgQTolerance : cse::kCgRTolerance, 3);
  }
  // max_num_iterations reached (:299-301)
  {
    const CgParams p{1, 2, 1e-12, 0.0};
    CgState s = Started(p);
    for (int it = 1; it <= 2; ++it) {
      CHECK(!s.done);
      CHECK(cse::CgDirection(&s, 1.0));
      CHECK(cse::CgStep(&s, 1.0));
      cse::CgTests(&s, p, (double)it, 1.0);
    }
    Expect(s, cse::kCgNoConvergence, cse::kCgMaxIterations, 2);
    CHECK(s.norm_r == 1.0 && s.Q1 == -2.0);
  }
}

void Frozen() {
  const CgParams o{1, 10, 1e-3, 0.0};
  CgState s = Started(o);
  CHECK(cse::CgDirection(&s, 2.0));
  CHECK(cse::CgStep(&s, 4.0));
  cse::CgTests(&s, o, 1.0, 1e-12);
  Expect(s, cse::kCgSuccess, cse::kCgRTolerance, 1);
  CgState before;
  std::memcpy(&before, &s, sizeof(s));
  for (int k = 0; k < 3; ++k) {
    cse::CgInitialResidual(&s, o, 5.0, 6.0);
    CHECK(!cse::CgDirection(&s, 0.0));
    CHECK(!cse::CgDirection(&s, 7.0));
    CHECK(!cse::CgStep(&s, -1.0));
    CHECK(!cse::CgStep(&s, 3.0));
    cse::CgTests(&s, o, 9.0, 9.0);
    CHECK(std::memcmp(&before, &s, sizeof(s)) == 0);
  }
}

}  // namespace

int main() {
  static_assert(sizeof(CgState) == 96, "ten doubles and four int32");
  KnownAnswers();
  ClosedForms();
  Branches();
  Frozen();
  std::printf("cg_state_driver OK\n");
  return 0;
}
