// spse_state_driver.cpp -- the transitions of csrc/spse_state.hpp on the host,
// under AddressSanitizer + UBSan (tests/test_schur_spse.py, spse_state.mk).
//
// 1. A host loop drives the transitions in the order cse_schur_power_series'
//    kernels do (spse_kernels.hpp) -- every term enqueued, the state deciding
//    -- on small systems S = P - Q, beside a plain restatement of the
//    reference's loop (power_series_expansion_preconditioner.cc:51-72) that
//    breaks where the reference breaks.  Sum, term count and norms are equal
//    bit for bit.
// 2. The stop test's corners: tolerance 0 never stops early, a huge tolerance
//    stops after the first term, max_num_iterations 1 adds one term.
// 3. After `done`, further transitions change nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ceres-solver-cuda_amd/csrc/spse_state.hpp"

using cse::SpseState;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

namespace {

using Vec = std::vector<double>;

double Norm(const Vec& a) {
  double s = 0.0;
  for (double v : a) s += v * v;
  return std::sqrt(s);
}

// P = diag(p), Q dense n x n (row-major) with small entries: P^-1 Q contracts.
struct System {
  int n;
  Vec p, Q;
  void ApplyPinv(const Vec& x, Vec* y) const {
    for (int i = 0; i < n; ++i) (*y)[i] = x[i] / p[i];
  }
  void ApplyQ(const Vec& x, Vec* y) const {
    for (int i = 0; i < n; ++i) {
      double s = 0.0;
      for (int j = 0; j < n; ++j) s += Q[(size_t)i * n + j] * x[j];
      (*y)[i] = s;
    }
  }
};

System MakeSystem(int n, double coupling) {
  System s{n, Vec(n), Vec((size_t)n * n)};
  for (int i = 0; i < n; ++i) s.p[i] = 2.0 + 0.25 * i;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) s.Q[(size_t)i * n + j] = coupling / (1.0 + std::abs(i - j));
  return s;
}

struct Outcome {
  Vec y;
  int terms;
  double first, last;
};

// The reference's loop, breaking where it breaks.
Outcome Reference(const System& s, const Vec& x, int max_it, double tol) {
  Outcome o{Vec(s.n), 0, 0.0, 0.0};
  Vec prev(s.n), t(s.n), term(s.n);
  s.ApplyPinv(x, &o.y);
  prev = o.y;
  o.first = o.last = Norm(o.y);
  const double threshold = tol * o.first;
  for (int i = 1;; ++i) {
    s.ApplyQ(prev, &t);
    s.ApplyPinv(t, &term);
    for (int k = 0; k < s.n; ++k) o.y[k] += term[k];
    o.terms = i;
    o.last = Norm(term);
    if (i >= max_it || o.last < threshold) break;
    std::swap(prev, term);
  }
  return o;
}

// The device's order: every term is enqueued; the kernel of a term returns at
// once when the state is done, the product before it writes scratch only.
Outcome Device(const System& s, const Vec& x, int max_it, double tol, int extra, SpseState* keep) {
  Outcome o{Vec(s.n), 0, 0.0, 0.0};
  Vec prev(s.n), t(s.n);
  SpseState st;
  std::memset(&st, 0xff, sizeof(st));
  s.ApplyPinv(x, &o.y);
  prev = o.y;
  cse::SpseBegin(&st, Norm(o.y), tol);
  for (int i = 1; i <= max_it + extra; ++i) {
    s.ApplyQ(prev, &t);  // scratch
    if (st.done) continue;
    Vec term(s.n);
    s.ApplyPinv(t, &term);
    for (int k = 0; k < s.n; ++k) o.y[k] += term[k];
    prev = term;
    const bool on = cse::SpseTerm(&st, Norm(term), max_it);
    CHECK(on == !st.done);
  }
  CHECK(st.done == 1);
  o.terms = st.num_terms;
  o.first = st.norm_first;
  o.last = st.norm_last;
  if (keep) *keep = st;
  return o;
}

void Compare(const System& s, const Vec& x, int max_it, double tol, int want_terms) {
  const Outcome r = Reference(s, x, max_it, tol);
  const Outcome d = Device(s, x, max_it, tol, 3, nullptr);
  CHECK(r.terms == d.terms);
  CHECK(want_terms < 0 || r.terms == want_terms);
  CHECK(r.first == d.first && r.last == d.last);
  CHECK(std::memcmp(r.y.data(), d.y.data(), sizeof(double) * s.n) == 0);
  CHECK(d.terms >= 1 && d.terms <= max_it);
}

}  // namespace

int main() {
  for (int n : {1, 3, 9, 18}) {
    const System s = MakeSystem(n, 0.6 / n);
    Vec x(n);
    for (int i = 0; i < n; ++i) x[i] = std::sin(1.0 + i);
    Compare(s, x, 5, 0.0, 5);      // tolerance 0: every term
    Compare(s, x, 50, 0.0, 50);
    Compare(s, x, 1, 1e-14, 1);    // one term
    Compare(s, x, 50, 1e14, 1);    // the first term is below any such threshold
    Compare(s, x, 50, 1e-3, -1);
    Compare(s, x, 500, 1e-14, -1);
    // the long series is S^-1 x: (P - Q) y = x
    const Outcome d = Device(s, x, 500, 1e-14, 0, nullptr);
    CHECK(d.terms < 500);
    Vec qy(n);
    s.ApplyQ(d.y, &qy);
    double err = 0.0;
    for (int i = 0; i < n; ++i) err = std::fmax(err, std::fabs(s.p[i] * d.y[i] - qy[i] - x[i]));
    CHECK(err < 1e-12);
  }
  {
    // Frozen after termination.
    const System s = MakeSystem(4, 0.1);
    const Vec x{1.0, -2.0, 3.0, 0.5};
    SpseState st;
    Device(s, x, 7, 1e-2, 0, &st);
    const SpseState before = st;
    CHECK(!cse::SpseTerm(&st, 123.0, 7));
    CHECK(!cse::SpseTerm(&st, 0.0, 1000));
    CHECK(std::memcmp(&before, &st, sizeof(st)) == 0);
  }
  {
    // x = 0: every norm is 0, 0 < 0 is false, so the series runs to the limit
    // (as the reference's would).
    const System s = MakeSystem(3, 0.1);
    const Vec x(3, 0.0);
    Compare(s, x, 4, 0.1, 4);
  }
  std::printf("spse_state_driver: ok\n");
  return 0;
}
