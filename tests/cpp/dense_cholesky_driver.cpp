// The dense Cholesky plan (cse::PlanDenseCholesky, plan.hpp) and the blocked
// order of dense_cholesky_kernels.hpp replayed on the host, under ASan + UBSan
// (tests/test_dense_cholesky.py):
//   - the plan at n = 1, NB-1, NB, NB+1, 2 NB+1 and 16,002 in both precisions
//     against counts written out here;
//   - every lower-triangle tile of the rows below a panel is covered exactly
//     once by the trailing update's folded grid, for every step of those n;
//   - the blocked factorization and solve (diagonal block, stored inverse,
//     panel = product with the inverse's transpose, trailing update, blocked
//     substitutions) in double and float against the unblocked textbook loop
//     at n <= 200, and both against Higham's backward error bound
//     ||A - L L^T||_F <= 2 (n + 1) u trace(A) evaluated in long double.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ceres-solver-cuda_amd/csrc/plan.hpp"

namespace {

constexpr int NB = cse::kDenseCholeskyNB;
int failures = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

int64_t RoundUp(int64_t bytes) { return (bytes + 255) / 256 * 256; }

void CheckPlan(int64_t n) {
  const int64_t T = (n + NB - 1) / NB, padded = T * NB;
  for (int32_t precision : {CSE_DENSE_CHOLESKY_FP64, CSE_DENSE_CHOLESKY_FP32}) {
    cse::DenseCholeskyPlan P;
    CHECK(cse::PlanDenseCholesky(n, precision, &P) == CSE_OK);
    CHECK(P.n == n && P.precision == precision);
    CHECK(P.num_panels == T && P.padded == padded);
    const bool f32 = precision == CSE_DENSE_CHOLESKY_FP32;
    // one diagonal kernel per panel, a panel and a trailing kernel for all but the last
    CHECK(P.factor_launches == T + 2 * (T - 1) + (f32 ? 1 : 0));
    CHECK(P.substitution_launches == 2 * T);
    const int64_t e = f32 ? 4 : 8;
    int64_t bytes = RoundUp(T * NB * NB * e) + 2 * RoundUp(padded * e) + 256;
    if (f32) bytes += RoundUp(n * n * 4) + 2 * RoundUp(padded * 8);
    CHECK(P.workspace_bytes == bytes);
    CHECK(P.matrix_off == 0 && P.inverse_off == (f32 ? RoundUp(n * n * 4) : 0));
    CHECK(P.inverse_off < P.v_off && P.v_off < P.y_off && P.y_off <= P.x_off && P.x_off <= P.r_off);
    CHECK(P.r_off <= P.flag_off && P.flag_off + 256 == P.workspace_bytes);
    CHECK(P.SolveLaunches(0) == (f32 ? 2 * T + 4 : 2 * T + 2));
    if (f32) CHECK(P.SolveLaunches(3) == 1 + 4 * (2 * T + 2) + 3 + 1);
  }
  // every step's grids
  for (int64_t k = 0; k < T; ++k) {
    const int64_t R = cse::DenseCholeskyRowsBelow(T, k);
    CHECK(R == T - 1 - k);
    if (T > 300 && k % 37 != 0 && k + 3 < T) continue;  // 16,002: a sample of steps and the last ones
    const int64_t gx = cse::DenseCholeskyTrailingGridX(R), gy = cse::DenseCholeskyTrailingGridY(R);
    std::vector<int> seen((size_t)(R * R), 0);
    int64_t live = 0;
    for (int64_t y = 0; y < gy; ++y)
      for (int64_t x = 0; x < gx; ++x) {
        const cse::DenseCholeskyTile t = cse::DenseCholeskyTrailingTile(R, x, y);
        if (!t.live) continue;
        CHECK(t.j >= 0 && t.j <= t.i && t.i < R);
        if (t.j >= 0 && t.j <= t.i && t.i < R) ++seen[(size_t)(t.i * R + t.j)];
        ++live;
      }
    CHECK(live == R * (R + 1) / 2);
    bool once = true;
    for (int64_t i = 0; i < R; ++i)
      for (int64_t j = 0; j < R; ++j) once = once && seen[(size_t)(i * R + j)] == (j <= i ? 1 : 0);
    CHECK(once);
  }
}

void CheckRefusals() {
  cse::DenseCholeskyPlan P;
  CHECK(cse::PlanDenseCholesky(0, CSE_DENSE_CHOLESKY_FP64, &P) == CSE_ERR_INVALID);
  CHECK(cse::PlanDenseCholesky(-3, CSE_DENSE_CHOLESKY_FP32, &P) == CSE_ERR_INVALID);
  CHECK(cse::PlanDenseCholesky(5, 2, &P) == CSE_ERR_INVALID);
  CHECK(cse::PlanDenseCholesky(5, CSE_DENSE_CHOLESKY_FP64, nullptr) == CSE_ERR_INVALID);
}

// A symmetric matrix with eigenvalues in [n / 2, 3 n / 2]: n on the diagonal,
// entries of magnitude at most 1 / 2 off it (Gershgorin).
std::vector<double> Matrix(int n, uint32_t seed) {
  std::vector<double> A((size_t)n * n);
  uint32_t s = seed;
  auto next = [&s]() {
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / (double)(1u << 24) - 0.5;
  };
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) A[(size_t)i * n + j] = A[(size_t)j * n + i] = i == j ? (double)n + next() : next();
  return A;
}

// The textbook loop, right-looking, on the lower triangle.
template <typename T>
bool Unblocked(std::vector<T>& L, int n) {
  for (int j = 0; j < n; ++j) {
    const T d = L[(size_t)j * n + j];
    if (!(d > T(0))) return false;
    const T s = std::sqrt(d);
    L[(size_t)j * n + j] = s;
    for (int r = j + 1; r < n; ++r) L[(size_t)r * n + j] /= s;
    for (int c = j + 1; c < n; ++c)
      for (int r = c; r < n; ++r) L[(size_t)r * n + c] -= L[(size_t)r * n + j] * L[(size_t)c * n + j];
  }
  return true;
}

// The kernels' order: per panel the diagonal block, its inverse from L X = I
// eliminated row by row, the panel as a product with the inverse's
// transpose, the trailing tiles in the folded grid's order.
template <typename T>
bool Blocked(std::vector<T>& L, int n, std::vector<T>& inv) {
  const int panels = (n + NB - 1) / NB;
  inv.assign((size_t)panels * NB * NB, T(0));
  for (int k = 0; k < panels; ++k) {
    const int k0 = k * NB, nb = n - k0 < NB ? n - k0 : NB;
    std::vector<T> a((size_t)NB * NB, T(0));
    for (int r = 0; r < NB; ++r)
      for (int c = 0; c <= r; ++c) a[(size_t)r * NB + c] = r < nb ? L[(size_t)(k0 + r) * n + k0 + c] : (r == c ? T(1) : T(0));
    if (!Unblocked(a, NB)) return false;
    for (int r = 0; r < nb; ++r)
      for (int c = 0; c <= r; ++c) L[(size_t)(k0 + r) * n + k0 + c] = a[(size_t)r * NB + c];
    T* X = inv.data() + (size_t)k * NB * NB;
    // L X = I as the kernel carries it: row j over the pivot, then the rows below.
    for (int c = 0; c < NB; ++c) X[(size_t)c * NB + c] = T(1);
    for (int j = 0; j < NB; ++j) {
      for (int c = 0; c <= j; ++c) X[(size_t)j * NB + c] = X[(size_t)j * NB + c] / a[(size_t)j * NB + j];
      for (int r = j + 1; r < NB; ++r)
        for (int c = 0; c <= j; ++c) X[(size_t)r * NB + c] -= a[(size_t)r * NB + j] * X[(size_t)j * NB + c];
    }
    const int k1 = k0 + NB;
    if (k1 >= n) break;
    for (int r = k1; r < n; ++r) {
      T row[NB];
      for (int c = 0; c < NB; ++c) {
        T sum = T(0);
        for (int m = 0; m < NB; ++m) sum += L[(size_t)r * n + k0 + m] * X[(size_t)c * NB + m];
        row[c] = sum;
      }
      for (int c = 0; c < NB; ++c) L[(size_t)r * n + k0 + c] = row[c];
    }
    const int64_t R = cse::DenseCholeskyRowsBelow(panels, k);
    for (int64_t y = 0; y < cse::DenseCholeskyTrailingGridY(R); ++y)
      for (int64_t x = 0; x < cse::DenseCholeskyTrailingGridX(R); ++x) {
        const cse::DenseCholeskyTile t = cse::DenseCholeskyTrailingTile(R, x, y);
        if (!t.live) continue;
        const int i0 = (int)(k + 1 + t.i) * NB, j0 = (int)(k + 1 + t.j) * NB;
        for (int r = i0; r < i0 + NB && r < n; ++r)
          for (int c = j0; c < j0 + NB && c <= r; ++c) {
            T sum = T(0);
            for (int m = 0; m < NB; ++m) sum += L[(size_t)r * n + k0 + m] * L[(size_t)c * n + k0 + m];
            L[(size_t)r * n + c] -= sum;
          }
      }
  }
  return true;
}

// The blocked substitutions: every step's diagonal product with the stored
// inverse, then the block rows' updates.
template <typename T>
std::vector<T> BlockedSolve(const std::vector<T>& L, int n, const std::vector<T>& inv, const std::vector<double>& b) {
  const int panels = (n + NB - 1) / NB, padded = panels * NB;
  std::vector<T> v((size_t)padded, T(0)), y((size_t)padded, T(0));
  for (int i = 0; i < n; ++i) v[(size_t)i] = (T)b[(size_t)i];
  for (int k = 0; k < panels; ++k) {
    const T* X = inv.data() + (size_t)k * NB * NB;
    for (int r = 0; r < NB; ++r) {
      T sum = T(0);
      for (int c = 0; c < NB; ++c) sum += X[(size_t)r * NB + c] * v[(size_t)k * NB + c];
      y[(size_t)k * NB + r] = sum;
    }
    for (int r = (k + 1) * NB; r < n; ++r) {
      T sum = T(0);
      for (int c = 0; c < NB; ++c) sum += L[(size_t)r * n + k * NB + c] * y[(size_t)k * NB + c];
      v[(size_t)r] -= sum;
    }
  }
  for (int k = panels - 1; k >= 0; --k) {
    const T* X = inv.data() + (size_t)k * NB * NB;
    for (int c = 0; c < NB; ++c) {
      T sum = T(0);
      for (int r = 0; r < NB; ++r) sum += X[(size_t)r * NB + c] * y[(size_t)k * NB + r];
      v[(size_t)k * NB + c] = sum;
    }
    for (int c = 0; c < k * NB; ++c) {
      T sum = T(0);
      for (int r = k * NB; r < (k + 1) * NB && r < n; ++r) sum += L[(size_t)r * n + c] * v[(size_t)r];
      y[(size_t)c] -= sum;
    }
  }
  v.resize((size_t)n);
  return v;
}

template <typename T>
long double FactorError(const std::vector<double>& A, const std::vector<T>& L, int n) {
  long double sum = 0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      long double p = 0;
      for (int m = 0; m <= (i < j ? i : j); ++m) p += (long double)L[(size_t)i * n + m] * (long double)L[(size_t)j * n + m];
      const long double d = (long double)A[(size_t)i * n + j] - p;
      sum += d * d;
    }
  return std::sqrt(sum);
}

template <typename T>
void CheckReplay(int n, double u) {
  const std::vector<double> A = Matrix(n, 17u + (uint32_t)n);
  std::vector<T> textbook((size_t)n * n), blocked((size_t)n * n), inv;
  for (size_t i = 0; i < A.size(); ++i) textbook[i] = blocked[i] = (T)A[i];
  CHECK(Unblocked(textbook, n));
  CHECK(Blocked(blocked, n, inv));
  double trace = 0;
  for (int i = 0; i < n; ++i) trace += A[(size_t)i * n + i];
  // one more unit than Thm 10.3 for the cast of A to T
  const long double bound = 2.0L * (n + 2) * u * trace;
  CHECK(FactorError(A, textbook, n) <= bound);
  CHECK(FactorError(A, blocked, n) <= bound);
  // Each is the exact factor of A + dA, ||dA||_F <= bound.  To first order
  // ||dL||_F / ||L||_F <= kappa(A) / sqrt(2) ||dA||_F / ||A||_2 (Sun 1991), here
  // kappa <= 3 and ||A||_2 >= n / 2: the two differ by at most
  // 2 * 3 / sqrt(2) * bound / (n / 2) < 9 bound / n; 12 leaves room for the
  // second order.
  long double diff = 0, norm = 0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      const long double d = (long double)textbook[(size_t)i * n + j] - (long double)blocked[(size_t)i * n + j];
      diff += d * d;
      norm += (long double)textbook[(size_t)i * n + j] * (long double)textbook[(size_t)i * n + j];
    }
  CHECK(std::sqrt(diff) <= 12.0L * bound / n * std::sqrt(norm));
  // the solve: ||b - A x||_2 <= 2 (3 n + 3) u trace(A) ||x||_2
  std::vector<double> b((size_t)n);
  for (int i = 0; i < n; ++i) b[(size_t)i] = std::sin(1.0 + 0.37 * i);
  const std::vector<T> x = BlockedSolve(blocked, n, inv, b);
  long double res = 0, xn = 0;
  for (int i = 0; i < n; ++i) {
    long double s = b[(size_t)i];
    for (int j = 0; j < n; ++j) s -= (long double)A[(size_t)i * n + j] * (long double)x[(size_t)j];
    res += s * s;
    xn += (long double)x[(size_t)i] * (long double)x[(size_t)i];
  }
  CHECK(std::sqrt(res) <= 2.0L * (3 * n + 3) * u * trace * std::sqrt(xn));
}

}  // namespace

int main() {
  for (int64_t n : {(int64_t)1, (int64_t)NB - 1, (int64_t)NB, (int64_t)NB + 1, (int64_t)2 * NB + 1, (int64_t)16002})
    CheckPlan(n);
  CheckRefusals();
  for (int n : {1, 2, 17, NB - 1, NB, NB + 1, 2 * NB + 1, 200}) {
    CheckReplay<double>(n, std::ldexp(1.0, -53));
    CheckReplay<float>(n, std::ldexp(1.0, -24));
  }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("dense_cholesky_driver: ok\n");
  return 0;
}
