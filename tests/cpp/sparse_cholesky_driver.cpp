// sparse_cholesky_driver.cpp -- cse::PlanSparseCholesky on the host, under
// ASan + UBSan (tests/test_sparse_cholesky.py).  Reads one case from the file
// named on the command line,
//   N ordering
//   row_begin[N + 1]
//   block_col[row_begin[N]]
//   permutation[N]                 (ordering = CSE_SPARSE_ORDERING_GIVEN only)
//   has_values (0 or 1), then values[row_begin[N]][81] and rhs[9 N] as hexfloats
// prints the plan, and with values replays the numeric factorization and the
// solve on the host through the plan's own tables -- gather by `source`, the
// level table, the merge of two block rows, the column index -- in the order
// the device kernels take (products k ascending, L_jj^-1 applied as a product,
// seven partial sums a row in the solves), in plain double arithmetic.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "../../ceres-solver-cuda_amd/csrc/plan.hpp"

namespace cse {
std::string& LastError();  // layout.cpp
}  // namespace cse

namespace {

constexpr int B = 9, BB = 81, kSlots = 7;

template <typename T>
void PrintInts(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (T x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}
void PrintDoubles(const char* name, const std::vector<double>& v) {
  std::printf("%s", name);
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}

bool PivotOk(double d) { return d > 0.0 && d <= std::numeric_limits<double>::max(); }

// C -= X Y^T
void SubtractProduct(const double* X, const double* Y, double* C) {
  for (int m = 0; m < B; ++m)
    for (int n = 0; n < B; ++n) {
      double s = 0.0;
      for (int q = 0; q < B; ++q) s += X[m * B + q] * Y[n * B + q];
      C[m * B + n] -= s;
    }
}

struct Replay {
  const cse::SparseCholeskyPlan& P;
  std::vector<double> L, inverse;
  std::vector<int> status;
  int info = 0;
  explicit Replay(const cse::SparseCholeskyPlan& plan) : P(plan) {}

  void Factorize(const std::vector<double>& values) {
    const size_t N = (size_t)P.num_block_rows;
    L.assign((size_t)P.num_factor_blocks * BB, 0.0);
    inverse.assign(N * BB, 0.0);
    status.assign(N, 0);
    for (size_t t = 0; t < (size_t)P.num_factor_blocks; ++t) {
      const int32_t src = P.source[t];
      if (src == -1) continue;
      const size_t from = (size_t)(src < 0 ? -2 - src : src);
      for (int e = 0; e < BB; ++e)
        L[t * BB + (size_t)e] = values[from * BB + (size_t)(src < 0 ? (e % B) * B + e / B : e)];
    }
    for (int32_t l = 0; l < P.num_levels; ++l) {
      for (int64_t q = P.level_begin[(size_t)l]; q < P.level_begin[(size_t)l + 1]; ++q)
        Diagonal(P.level_columns[(size_t)q]);
      for (int64_t q = P.target_begin[(size_t)l]; q < P.target_begin[(size_t)l + 1]; ++q)
        Target(P.level_targets[(size_t)q]);
    }
    info = 0;
    for (size_t j = 0; j < N; ++j)
      if (status[j] && (info == 0 || (int)(B * j) + status[j] < info)) info = (int)(B * j) + status[j];
  }

  void Diagonal(int32_t j) {
    const int64_t first = P.row_begin[(size_t)j], diag = P.row_begin[(size_t)j + 1] - 1;
    double* a = &L[(size_t)diag * BB];
    for (int64_t b = first; b < diag; ++b) SubtractProduct(&L[(size_t)b * BB], &L[(size_t)b * BB], a);
    int fail = 0;
    for (int k = 0; k < B; ++k) {
      const double p = a[k * B + k];
      if (!PivotOk(p) && !fail) fail = k + 1;
      const double s = std::sqrt(p);
      a[k * B + k] = s;
      for (int r = k + 1; r < B; ++r) a[r * B + k] /= s;
      for (int c = k + 1; c < B; ++c)
        for (int r = c; r < B; ++r) a[r * B + c] -= a[r * B + k] * a[c * B + k];
    }
    double* x = &inverse[(size_t)j * BB];
    for (int c = 0; c < B; ++c)
      for (int r = c; r < B; ++r) {
        double s = 0.0;
        for (int q = c; q < r; ++q) s += a[r * B + q] * x[q * B + c];
        x[r * B + c] = (r == c ? 1.0 : -s) / a[r * B + r];
      }
    for (int r = 0; r < B; ++r)
      for (int c = r + 1; c < B; ++c) a[r * B + c] = 0.0;
    status[(size_t)j] = fail;
  }

  void Target(int32_t t) {
    const int32_t i = P.block_row[(size_t)t], j = P.block_col[(size_t)t];
    double* T = &L[(size_t)t * BB];
    int64_t pa = P.row_begin[(size_t)i], pb = P.row_begin[(size_t)j];
    const int64_t ea = P.row_begin[(size_t)i + 1] - 1, eb = P.row_begin[(size_t)j + 1] - 1;
    while (pa < ea && pb < eb) {
      const int32_t ca = P.block_col[(size_t)pa], cb = P.block_col[(size_t)pb];
      if (ca >= j) break;
      if (ca == cb) {
        SubtractProduct(&L[(size_t)pa * BB], &L[(size_t)pb * BB], T);
        ++pa, ++pb;
      } else if (ca < cb) {
        ++pa;
      } else {
        ++pb;
      }
    }
    const double* M = &inverse[(size_t)j * BB];
    double out[BB];
    for (int r = 0; r < B; ++r)
      for (int c = 0; c < B; ++c) {
        double s = 0.0;
        for (int q = 0; q < B; ++q) s += T[r * B + q] * M[c * B + q];
        out[r * B + c] = s;
      }
    for (int e = 0; e < BB; ++e) T[e] = out[e];
  }

  std::vector<double> Solve(const std::vector<double>& rhs) const {
    const size_t N = (size_t)P.num_block_rows;
    std::vector<double> y(N * B), x(N * B, 0.0);
    for (size_t k = 0; k < N; ++k)
      for (int r = 0; r < B; ++r) y[k * B + (size_t)r] = rhs[(size_t)P.permutation[k] * B + (size_t)r];
    for (int32_t l = 0; l < P.num_levels; ++l)
      for (int64_t q = P.level_begin[(size_t)l]; q < P.level_begin[(size_t)l + 1]; ++q) {
        const size_t i = (size_t)P.level_columns[(size_t)q];
        const int64_t first = P.row_begin[i], diag = P.row_begin[i + 1] - 1;
        double part[kSlots][B] = {}, t[B];
        for (int64_t b = first; b < diag; ++b)
          for (int r = 0; r < B; ++r)
            for (int c = 0; c < B; ++c)
              part[(b - first) % kSlots][r] +=
                  L[(size_t)b * BB + (size_t)(r * B + c)] * y[(size_t)P.block_col[(size_t)b] * B + (size_t)c];
        for (int r = 0; r < B; ++r) {
          double s = part[0][r];
          for (int k = 1; k < kSlots; ++k) s += part[k][r];
          t[r] = y[i * B + (size_t)r] - s;
        }
        for (int r = 0; r < B; ++r) {
          double s = 0.0;
          for (int c = 0; c <= r; ++c) s += inverse[i * BB + (size_t)(r * B + c)] * t[c];
          y[i * B + (size_t)r] = s;
        }
      }
    for (int32_t l = P.num_levels - 1; l >= 0; --l)
      for (int64_t q = P.level_begin[(size_t)l]; q < P.level_begin[(size_t)l + 1]; ++q) {
        const size_t j = (size_t)P.level_columns[(size_t)q];
        double part[kSlots][B] = {}, t[B];
        for (int64_t k = P.col_begin[j]; k < P.col_begin[j + 1]; ++k) {
          const size_t b = (size_t)P.col_block[(size_t)k];
          for (int c = 0; c < B; ++c)
            for (int r = 0; r < B; ++r)
              part[(k - P.col_begin[j]) % kSlots][c] +=
                  L[b * BB + (size_t)(r * B + c)] * y[(size_t)P.block_row[b] * B + (size_t)r];
        }
        for (int c = 0; c < B; ++c) {
          double s = part[0][c];
          for (int k = 1; k < kSlots; ++k) s += part[k][c];
          t[c] = y[j * B + (size_t)c] - s;
        }
        for (int c = 0; c < B; ++c) {
          double s = 0.0;
          for (int r = c; r < B; ++r) s += inverse[j * BB + (size_t)(r * B + c)] * t[r];
          y[j * B + (size_t)c] = s;
        }
      }
    if (info == 0)
      for (size_t k = 0; k < N; ++k)
        for (int r = 0; r < B; ++r) x[(size_t)P.permutation[k] * B + (size_t)r] = y[k * B + (size_t)r];
    return x;
  }
};

bool ReadDoubles(std::ifstream& in, std::vector<double>* v) {
  std::string tok;
  for (double& x : *v) {
    if (!(in >> tok)) return false;
    x = std::strtod(tok.c_str(), nullptr);
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: sparse_cholesky_driver CASE_FILE\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  long long N = 0;
  int ordering = 0;
  if (!(in >> N >> ordering) || N < 0 || N > 100000) return 2;
  std::vector<int64_t> row_begin((size_t)N + 1);
  for (int64_t& v : row_begin)
    if (!(in >> v)) return 2;
  const int64_t nin = row_begin.back();
  if (nin < 0 || nin > 10000000) return 2;
  std::vector<int32_t> block_col((size_t)nin), given;
  for (int32_t& v : block_col)
    if (!(in >> v)) return 2;
  if (ordering == CSE_SPARSE_ORDERING_GIVEN) {
    given.resize((size_t)N);
    for (int32_t& v : given)
      if (!(in >> v)) return 2;
  }
  int has_values = 0;
  if (!(in >> has_values)) return 2;
  std::vector<double> values, rhs;
  if (has_values) {
    values.resize((size_t)nin * BB);
    rhs.resize((size_t)N * B);
    if (!ReadDoubles(in, &values) || !ReadDoubles(in, &rhs)) return 2;
  }

  cse::SparseCholeskyPlan P;
  const int rc = cse::PlanSparseCholesky(N, row_begin.data(), block_col.data(), ordering,
                                         given.empty() ? nullptr : given.data(), &P);
  std::printf("rc %d\n", rc);
  if (rc) {
    std::printf("error %s\n", cse::LastError().c_str());
    return 0;
  }
  std::printf("summary %lld %lld %lld %lld %lld %d %d\n", (long long)P.num_block_rows, (long long)P.num_input_blocks,
              (long long)P.num_factor_blocks, (long long)P.num_block_products, (long long)P.device_bytes, P.num_levels,
              P.max_level_columns);
  PrintInts("permutation", P.permutation);
  PrintInts("row_begin", P.row_begin);
  PrintInts("block_col", P.block_col);
  PrintInts("block_row", P.block_row);
  PrintInts("col_begin", P.col_begin);
  PrintInts("col_block", P.col_block);
  PrintInts("parent", P.parent);
  PrintInts("level", P.level);
  PrintInts("scatter", P.scatter);
  PrintInts("source", P.source);
  PrintInts("level_begin", P.level_begin);
  PrintInts("level_columns", P.level_columns);
  PrintInts("target_begin", P.target_begin);
  PrintInts("level_targets", P.level_targets);
  if (has_values) {
    Replay R(P);
    R.Factorize(values);
    std::printf("info %d\n", R.info);
    PrintDoubles("L", R.L);
    PrintDoubles("x", R.Solve(rhs));
  }
  return 0;
}
