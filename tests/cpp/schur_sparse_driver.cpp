// schur_sparse_driver.cpp -- the host-only structure of the block-sparse Schur
// complement (cse::PlanSchurSparse, csrc/plan.cpp), built by g++ with
// AddressSanitizer + UBSan from plan.cpp, layout.cpp and this file
// (tests/test_schur_sparse.py runs it; no HIP, no GPU).
//
// Per problem -- BAL-shaped; points that see one camera several times; an
// unobserved camera in the middle and one at the end; one camera only; no
// residual block at all -- the structure over cse::PlanSchurPairs' plan is
// checked against brute force: rows ascending with the diagonal first, every
// plan block mapped exactly once, added diagonals mapped to -1, the transposed
// index of camera c exactly the blocks of column c above the diagonal in
// ascending row order, the finish list exactly the blocks that are not stored
// by one chunk, and the counts-only mode the same counts.  Then the product
// y = S x is replayed in the order of SchurExplicitRowKernel (a lane per
// entry, the row blocks cut over the waves by SchurExplicitPer, the per-wave
// sums added in wave order, each block's column contribution) and
// SchurExplicitColumnKernel (the contributions of a column's blocks added by
// slots) on random values and compared with the dense symmetric product per
// entry, to 1e-12 (|S| |x|)_i.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../ceres-solver-cuda_amd/csrc/plan.hpp"
#include "../../include/cse.h"

static int g_failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++g_failures;                                                     \
    }                                                                   \
  } while (0)

namespace {

uint64_t lcg = 0x9E3779B97F4A7C15ull;
double Uniform() {
  lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(lcg >> 11) * (1.0 / 9007199254740992.0);
}

typedef std::pair<int32_t, int32_t> Key;

// cams[p]: the cameras (0..C) of point p's observations; f block id = P + camera.
void Check(const char* what, int C, const std::vector<std::vector<int>>& cams) {
  const int P = (int)cams.size();
  std::vector<int32_t> ids;
  for (int p = 0; p < P; ++p)
    for (int c : cams[p]) {
      ids.push_back(P + c);
      ids.push_back(p);
    }
  const int64_t n = (int64_t)ids.size() / 2;
  cse::SchurPairPlan pairs, pair_counts;
  EXPECT(cse::PlanSchurPairs(ids.data(), n, false, &pairs) == CSE_OK);
  EXPECT(cse::PlanSchurPairs(ids.data(), n, true, &pair_counts) == CSE_OK);
  cse::SchurSparsePlan S, counts;
  EXPECT(cse::PlanSchurSparse(ids.data(), n, pairs, P, C, false, &S) == CSE_OK);
  EXPECT(cse::PlanSchurSparse(ids.data(), n, pair_counts, P, C, true, &counts) == CSE_OK);

  // Brute force: the co-visible pairs c <= c', and every diagonal.
  std::set<Key> want;
  std::vector<bool> observed((size_t)C, false);
  for (const auto& cs : cams)
    for (int a : cs) {
      observed[(size_t)a] = true;
      for (int b : cs)
        if (a <= b) want.insert(Key(a, b));
    }
  const int64_t covisible = (int64_t)want.size();
  for (int c = 0; c < C; ++c) want.insert(Key(c, c));
  const int64_t nb = (int64_t)want.size();
  EXPECT(pairs.num_blocks == covisible);
  EXPECT(S.num_block_rows == C && S.num_blocks == nb);
  // counts-only: the same counts, no table
  EXPECT(counts.num_block_rows == S.num_block_rows && counts.num_blocks == S.num_blocks &&
         counts.finish_capacity == S.finish_capacity && counts.device_bytes == S.device_bytes);
  EXPECT(counts.row_begin.empty() && counts.block_col.empty() && counts.plan_block.empty() &&
         counts.sparse_of_plan.empty() && counts.finish.empty() && counts.col_begin.empty() &&
         counts.col_block.empty() && counts.col_row.empty());
  EXPECT((int64_t)S.row_begin.size() == C + 1 && (int64_t)S.col_begin.size() == C + 1);
  EXPECT((int64_t)S.block_col.size() == nb && (int64_t)S.plan_block.size() == nb);
  EXPECT((int64_t)S.sparse_of_plan.size() == pairs.num_blocks);
  EXPECT((int64_t)S.col_block.size() == nb - C && (int64_t)S.col_row.size() == nb - C);
  EXPECT((int64_t)S.finish.size() <= S.finish_capacity);
  EXPECT(S.device_bytes ==
         16 * (C + 1) + 8 * nb + 4 * pairs.num_blocks + 4 * S.finish_capacity + 4 * (nb - C) + 72 * nb);
  if (g_failures) return;
  EXPECT(S.row_begin[0] == 0 && S.row_begin[(size_t)C] == nb);
  EXPECT(S.col_begin[0] == 0 && S.col_begin[(size_t)C] == nb - C);

  // Rows: ascending, the diagonal first; in all exactly the brute-force set
  // in lexicographic order.
  auto it = want.begin();
  std::vector<int> mapped((size_t)pairs.num_blocks, 0);
  std::set<int32_t> finish_want;
  for (int c = 0; c < C; ++c) {
    const int64_t b0 = S.row_begin[(size_t)c], b1 = S.row_begin[(size_t)c + 1];
    EXPECT(b1 > b0);
    if (b1 <= b0) return;
    EXPECT(S.block_col[(size_t)b0] == c);
    for (int64_t b = b0; b < b1; ++b, ++it) {
      if (b > b0) EXPECT(S.block_col[(size_t)b - 1] < S.block_col[(size_t)b]);
      EXPECT(it != want.end() && *it == Key(c, S.block_col[(size_t)b]));
      const int32_t k = S.plan_block[(size_t)b];
      if (b == b0 && !observed[(size_t)c]) {
        EXPECT(k == -1);  // an added diagonal
        EXPECT(b1 == b0 + 1);
        finish_want.insert((int32_t)b);
        continue;
      }
      EXPECT(k >= 0 && k < pairs.num_blocks);
      if (k < 0 || k >= pairs.num_blocks) return;
      ++mapped[(size_t)k];
      EXPECT(pairs.block_row[(size_t)k] == P + c && pairs.block_col[(size_t)k] == P + S.block_col[(size_t)b]);
      EXPECT(S.sparse_of_plan[(size_t)k] == b);
      if (pairs.chunk_off[(size_t)k + 1] - pairs.chunk_off[(size_t)k] != 1) finish_want.insert((int32_t)b);
    }
  }
  EXPECT(it == want.end());
  for (int v : mapped) EXPECT(v == 1);  // every plan block exactly once
  EXPECT(std::set<int32_t>(S.finish.begin(), S.finish.end()) == finish_want &&
         S.finish.size() == finish_want.size());

  // The transposed index of camera c: the blocks of column c above the
  // diagonal, in ascending row order.
  for (int c = 0; c < C; ++c) {
    std::vector<Key> col;  // (row, sparse block)
    for (int r = 0; r < c; ++r)
      for (int64_t b = S.row_begin[(size_t)r]; b < S.row_begin[(size_t)r + 1]; ++b)
        if (S.block_col[(size_t)b] == c) col.push_back(Key(r, (int32_t)b));
    const int64_t j0 = S.col_begin[(size_t)c], j1 = S.col_begin[(size_t)c + 1];
    EXPECT(j1 - j0 == (int64_t)col.size());
    if (j1 - j0 != (int64_t)col.size()) return;
    for (int64_t j = j0; j < j1; ++j)
      EXPECT(Key(S.col_row[(size_t)j], S.col_block[(size_t)j]) == col[(size_t)(j - j0)]);
  }

  // ---- The product replayed in the kernel's order against the dense one.
  const int64_t N = 9LL * C;
  std::vector<double> V(81 * (size_t)nb), x((size_t)N), dense((size_t)(N * N), 0.0);
  for (double& v : V) v = 2.0 * Uniform() - 1.0;
  for (double& v : x) v = 2.0 * Uniform() - 1.0;
  for (int c = 0; c < C; ++c)
    for (int64_t b = S.row_begin[(size_t)c]; b < S.row_begin[(size_t)c + 1]; ++b) {
      const int c2 = S.block_col[(size_t)b];
      for (int m = 0; m < 9; ++m)
        for (int k = 0; k < 9; ++k) {
          const double v = V[81 * (size_t)b + 9 * m + k];
          dense[(size_t)((9 * c + m) * N + 9 * c2 + k)] = v;
          if (c2 != c) dense[(size_t)((9 * c2 + k) * N + 9 * c + m)] = v;
        }
    }
  // SchurExplicitRowKernel: the row sums per lane and wave, and each block's
  // column contribution S(c, c')^T x_c, entries (0..9, n) added in that order.
  std::vector<double> contrib(9 * (size_t)nb, 0.0), yrow((size_t)N, 0.0);
  int longest = 0;
  for (int c = 0; c < C; ++c) {
    const int64_t r0 = S.row_begin[(size_t)c], nrow = S.row_begin[(size_t)c + 1] - r0;
    longest = std::max(longest, (int)nrow);
    const int64_t per = cse::SchurExplicitPer(nrow);
    double sums[cse::kSchurExplicitWaves][81];
    for (int w = 0; w < cse::kSchurExplicitWaves; ++w) {
      const int64_t lo = w * per, hi = std::min(lo + per, nrow);
      for (int e = 0; e < 81; ++e) {  // the lane that owns entry e
        double r = 0.0;
        for (int64_t i = lo; i < hi; ++i)
          r += V[81 * (size_t)(r0 + i) + e] * x[(size_t)(9 * S.block_col[(size_t)(r0 + i)] + e % 9)];
        sums[w][e] = r;
      }
    }
    for (int64_t b = r0; b < r0 + nrow; ++b)
      for (int k = 0; k < 9; ++k) {
        double s = 0.0;
        for (int m = 0; m < 9; ++m) s += V[81 * (size_t)b + 9 * m + k] * x[(size_t)(9 * c + m)];
        contrib[9 * (size_t)b + k] = s;
      }
    for (int i = 0; i < 9; ++i)
      for (int w = 0; w < cse::kSchurExplicitWaves; ++w) {
        double r = 0.0;
        for (int k = 0; k < 9; ++k) r += sums[w][9 * i + k];
        yrow[(size_t)(9 * c + i)] += r;
      }
  }
  // SchurExplicitColumnKernel: slot s sums the column list's entries s,
  // s + slots, .. in list order; the slots are added in slot order, onto y.
  const int kSlots = cse::kSchurExplicitSlots;
  double worst = 0.0;
  for (int c = 0; c < C; ++c) {
    double y[9];
    for (int i = 0; i < 9; ++i) {
      y[i] = yrow[(size_t)(9 * c + i)];
      const int64_t t0 = S.col_begin[(size_t)c], t1 = S.col_begin[(size_t)c + 1];
      if (t0 == t1) continue;
      double r = 0.0;
      for (int s = 0; s < kSlots; ++s) {
        double acc = 0.0;
        for (int64_t j = t0 + s; j < t1; j += kSlots) acc += contrib[9 * (size_t)S.col_block[(size_t)j] + i];
        r += acc;
      }
      y[i] += r;
    }
    for (int i = 0; i < 9; ++i) {
      double ref = 0.0, mag = 0.0;
      const int64_t row = 9LL * c + i;
      for (int64_t k = 0; k < N; ++k) {
        ref += dense[(size_t)(row * N + k)] * x[(size_t)k];
        mag += std::fabs(dense[(size_t)(row * N + k)]) * std::fabs(x[(size_t)k]);
      }
      EXPECT(std::fabs(y[i] - ref) <= 1e-12 * mag);
      if (mag > 0) worst = std::max(worst, std::fabs(y[i] - ref) / mag);
    }
  }
  std::printf("  %-26s %3d cameras %5lld blocks (%lld added, %lld finished), longest row %3d, replay worst %.2e\n",
              what, C, (long long)nb, (long long)(nb - covisible), (long long)S.finish.size(), longest, worst);
}

}  // namespace

int main() {
  std::printf("Block-sparse Schur complement structure driver\n");
  {
    std::vector<std::vector<int>> cams(60);
    for (int p = 0; p < 60; ++p)
      for (int k = 0; k < 1 + (p + 1) % 5; ++k) cams[p].push_back((p * 7 + k * 3) % 11);
    Check("BAL-shaped", 11, cams);
  }
  {  // blocks of several chunks: 3 cameras, 150 points that all see two or three of them
    std::vector<std::vector<int>> cams(150);
    for (int p = 0; p < 150; ++p) cams[p] = p % 3 ? std::vector<int>{0, 1, 2} : std::vector<int>{2, 0};
    Check("several chunks a block", 3, cams);
  }
  {  // a wider one: lists long enough to be cut over the waves, gaps inside rows
    std::vector<std::vector<int>> cams(400);
    for (int p = 0; p < 400; ++p)
      for (int k = 0; k < 2 + p % 4; ++k) cams[p].push_back((p * 13 + k * (1 + p % 7)) % 40);
    Check("40 cameras", 40, cams);
  }
  Check("duplicates", 5, {{0, 0, 1}, {2, 2, 2, 3}, {1, 4}, {3, 3, 0, 0, 0}, {4, 2}, {1, 0, 1}});
  Check("unobserved middle and end", 7, {{0, 1, 2}, {2, 4}, {4, 5, 0}, {1, 5}, {0, 2, 4, 5}});
  Check("one camera", 1, {{0}, {0, 0}, {0}});
  Check("no residual blocks", 4, {});
  {  // an f block outside the cameras
    const int32_t ids[] = {3, 0, 9, 0};
    cse::SchurPairPlan pairs;
    cse::SchurSparsePlan S;
    EXPECT(cse::PlanSchurPairs(ids, 2, true, &pairs) == CSE_OK);
    EXPECT(cse::PlanSchurSparse(ids, 2, pairs, 3, 4, true, &S) == CSE_ERR_INVALID);
    EXPECT(cse::PlanSchurSparse(ids, 2, pairs, 4, 8, true, &S) == CSE_ERR_INVALID);
  }
  if (g_failures) {
    std::printf("%d FAILED\n", g_failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
