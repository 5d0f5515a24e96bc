// schur_cluster_driver.cpp -- the host side of CLUSTER_JACOBI
// (cse_schur_set_clusters, cse_schur_cluster_jacobi): the cluster-filtered pair
// plan with its tile layout (cse::PlanSchurPairs' filter and
// cse::PlanSchurClusters, csrc/plan.cpp), built by g++ with AddressSanitizer +
// UBSan from plan.cpp, layout.cpp and this file (tests/test_schur_cluster.py
// runs it; no HIP, no GPU).
//
// Per problem and partition the filtered plan is checked against brute force
// over every (point, b, b'): exactly the blocks (c, c') with one label, each
// block's pair list in (point, b, b') order, and list and chunk cut equal to
// the UNFILTERED plan's for that block, entry by entry.  The tile layout: each
// cluster's cameras ascending, the tiles of its upper triangle from
// first_tile[g], every plan block on its tile, the finish list exactly the
// tiles of several chunks and the diagonals of unobserved cameras, the empty
// tiles exactly the others without a block.  Counts-only gives the same
// counts, and with one cluster of every camera the full plan's.
//
// Then a host replay of ClusterFactorKernel and ClusterApplyKernel
// (csrc/cluster_kernels.hpp) in the kernels' order -- the same tile layout, the
// diagonal tile column by column, the panel rows, the trailing tiles entry by
// entry, the block substitutions -- on random symmetric positive definite
// matrices of 1 to 16 cameras: for M z = r,
//     eta = |M z - r|_inf / (|M|_inf |z|_inf + |r|_inf) <= n gamma_{3n+1},
// gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability of
// Numerical Algorithms, Thm 10.4 in normwise form).  With a directory as
// argument, M, r and z of every size are written there for the caller to
// compare with its own solver.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
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
typedef std::vector<Key> PairList;

// cams[p]: the cameras (0..C) of point p's observations; f block id = P + camera.
void CheckPlan(const char* what, int C, const std::vector<std::vector<int>>& cams,
               const std::vector<int32_t>& label, int32_t G) {
  const int before = g_failures;
  const int P = (int)cams.size();
  std::vector<int32_t> ids;
  for (int p = 0; p < P; ++p)
    for (int c : cams[p]) {
      ids.push_back(P + c);
      ids.push_back(p);
    }
  const int64_t n = (int64_t)ids.size() / 2;
  cse::SchurPairPlan full;
  EXPECT(cse::PlanSchurPairs(ids.data(), n, false, &full) == CSE_OK);
  cse::SchurClusterPlan Z, counts;
  EXPECT(cse::PlanSchurClusters(ids.data(), n, P, C, label.data(), G, false, &Z) == CSE_OK);
  EXPECT(cse::PlanSchurClusters(ids.data(), n, P, C, label.data(), G, true, &counts) == CSE_OK);
  if (g_failures != before) return;
  const cse::SchurPairPlan& F = Z.pairs;

  // Brute force over every (point, b, b'): the rows of a point are one run.
  std::map<Key, PairList> want, all;
  std::vector<bool> observed((size_t)C, false);
  for (int64_t b = 0; b < n; ++b) observed[(size_t)(ids[2 * b] - P)] = true;
  for (int64_t r0 = 0; r0 < n;) {
    int64_t r1 = r0;
    while (r1 < n && ids[2 * r1 + 1] == ids[2 * r0 + 1]) ++r1;
    for (int64_t b = r0; b < r1; ++b)
      for (int64_t b2 = r0; b2 < r1; ++b2) {
        const int c = ids[2 * b] - P, c2 = ids[2 * b2] - P;
        if (c > c2) continue;
        all[Key(c, c2)].push_back(Key((int32_t)b, (int32_t)b2));
        if (label[(size_t)c] == label[(size_t)c2]) want[Key(c, c2)].push_back(Key((int32_t)b, (int32_t)b2));
      }
    r0 = r1;
  }
  // The unfiltered plan is the brute-force list of every block (its own test
  // checks that too): index its blocks.
  std::map<Key, int64_t> full_block;
  for (int64_t k = 0; k < full.num_blocks; ++k)
    full_block[Key(full.block_row[(size_t)k] - P, full.block_col[(size_t)k] - P)] = k;
  EXPECT(full_block.size() == all.size());

  EXPECT(F.num_blocks == (int64_t)want.size());
  EXPECT((int64_t)F.block_row.size() == F.num_blocks && (int64_t)F.pair_begin.size() == F.num_blocks + 1 &&
         (int64_t)F.chunk_off.size() == F.num_blocks + 1 && (int64_t)F.chunk_block.size() == F.num_chunks &&
         (int64_t)F.pairs.size() == 2 * F.num_pairs);
  if (g_failures != before) return;
  int64_t k = 0, npairs = 0, nchunks = 0, longest = 0;
  for (const auto& kv : want) {  // lexicographic, as the plan's blocks
    const PairList& list = kv.second;
    EXPECT(Key(F.block_row[(size_t)k] - P, F.block_col[(size_t)k] - P) == kv.first);
    const int64_t p0 = F.pair_begin[(size_t)k], p1 = F.pair_begin[(size_t)k + 1];
    EXPECT(p0 == npairs && p1 - p0 == (int64_t)list.size());
    if (p1 - p0 != (int64_t)list.size()) return;
    for (int64_t i = 0; i < p1 - p0; ++i)
      EXPECT(Key(F.pairs[(size_t)(2 * (p0 + i))], F.pairs[(size_t)(2 * (p0 + i) + 1)]) == list[(size_t)i]);
    // ... and the unfiltered plan's list and chunk cut of the same block
    const auto at = full_block.find(kv.first);
    EXPECT(at != full_block.end());
    if (at == full_block.end()) return;
    const int64_t kf = at->second, q0 = full.pair_begin[(size_t)kf];
    EXPECT(full.pair_begin[(size_t)kf + 1] - q0 == p1 - p0);
    for (int64_t i = 0; i < p1 - p0; ++i)
      EXPECT(F.pairs[(size_t)(2 * (p0 + i))] == full.pairs[(size_t)(2 * (q0 + i))] &&
             F.pairs[(size_t)(2 * (p0 + i) + 1)] == full.pairs[(size_t)(2 * (q0 + i) + 1)]);
    const int64_t chunks = F.chunk_off[(size_t)k + 1] - F.chunk_off[(size_t)k];
    EXPECT(F.chunk_off[(size_t)k] == nchunks);
    EXPECT(chunks == full.chunk_off[(size_t)kf + 1] - full.chunk_off[(size_t)kf]);
    EXPECT(chunks == (p1 - p0 + cse::kSchurPairChunk - 1) / cse::kSchurPairChunk);
    for (int64_t q = 0; q < chunks; ++q) EXPECT(F.chunk_block[(size_t)(nchunks + q)] == k);
    longest = std::max(longest, p1 - p0);
    npairs += p1 - p0;
    nchunks += chunks;
    ++k;
  }
  EXPECT(F.num_pairs == npairs && F.num_chunks == nchunks);

  // The tile layout.
  EXPECT(Z.num_clusters == G && Z.num_cameras == C);
  EXPECT((int64_t)Z.camera_begin.size() == G + 1 && (int64_t)Z.cameras.size() == C &&
         (int64_t)Z.first_tile.size() == G + 1 && (int64_t)Z.value_begin.size() == G + 1);
  if (g_failures != before) return;
  std::vector<int> local((size_t)C, -1);
  int64_t tiles = 0, values = 0, largest = 0;
  for (int32_t g = 0; g < G; ++g) {
    const int32_t c0 = Z.camera_begin[(size_t)g], c1 = Z.camera_begin[(size_t)g + 1];
    EXPECT(c1 > c0 && Z.first_tile[(size_t)g] == tiles && Z.value_begin[(size_t)g] == values);
    for (int32_t i = c0; i < c1; ++i) {
      const int32_t c = Z.cameras[(size_t)i];
      EXPECT(c >= 0 && c < C && label[(size_t)c] == g && local[(size_t)c] == -1);
      if (i > c0) EXPECT(Z.cameras[(size_t)i - 1] < c);
      local[(size_t)c] = i - c0;
    }
    const int64_t ng = c1 - c0;
    tiles += ng * (ng + 1) / 2;
    values += 81 * ng * ng;
    largest = std::max(largest, ng);
  }
  EXPECT(Z.camera_begin[(size_t)G] == C && Z.first_tile[(size_t)G] == tiles && Z.value_begin[(size_t)G] == values);
  EXPECT(Z.num_tiles == tiles && Z.num_values == values && Z.max_cameras == largest);
  EXPECT((int64_t)Z.tile_of_plan.size() == F.num_blocks && (int64_t)Z.plan_of_tile.size() == tiles &&
         (int64_t)Z.tile_camera.size() == tiles);
  if (g_failures != before) return;
  std::vector<int> written((size_t)tiles, 0);
  for (int64_t b = 0; b < F.num_blocks; ++b) {
    const int c = F.block_row[(size_t)b] - P, c2 = F.block_col[(size_t)b] - P;
    const int64_t t = Z.first_tile[(size_t)label[(size_t)c]] + cse::ClusterTile(local[(size_t)c], local[(size_t)c2]);
    EXPECT(local[(size_t)c] <= local[(size_t)c2]);
    EXPECT(Z.tile_of_plan[(size_t)b] == t && Z.plan_of_tile[(size_t)t] == b);
    ++written[(size_t)t];
  }
  std::set<int32_t> finish_want, empty_want;
  for (int32_t g = 0; g < G; ++g) {
    const int32_t c0 = Z.camera_begin[(size_t)g], ng = Z.camera_begin[(size_t)g + 1] - c0;
    for (int j = 0; j < ng; ++j)
      for (int i = 0; i <= j; ++i) {
        const int64_t t = Z.first_tile[(size_t)g] + cse::ClusterTile(i, j);
        const int32_t ci = Z.cameras[(size_t)(c0 + i)], cj = Z.cameras[(size_t)(c0 + j)];
        EXPECT(Z.tile_camera[(size_t)t] == ci);
        const bool has = want.count(Key(ci, cj)) != 0;
        EXPECT(written[(size_t)t] == (has ? 1 : 0));
        EXPECT((Z.plan_of_tile[(size_t)t] >= 0) == has);
        if (!has) {
          empty_want.insert((int32_t)t);
          // a diagonal without pairs: the camera has no residual block
          if (i == j) {
            EXPECT(!observed[(size_t)ci]);
            finish_want.insert((int32_t)t);
          }
        } else if (want[Key(ci, cj)].size() > (size_t)cse::kSchurPairChunk) {
          finish_want.insert((int32_t)t);
        }
      }
  }
  EXPECT(std::set<int32_t>(Z.finish.begin(), Z.finish.end()) == finish_want && Z.finish.size() == finish_want.size());
  EXPECT(std::set<int32_t>(Z.empty_tiles.begin(), Z.empty_tiles.end()) == empty_want &&
         Z.empty_tiles.size() == empty_want.size());
  EXPECT((int64_t)Z.finish.size() <= Z.finish_capacity);

  // Counts-only: the same counts and no table; one cluster of every camera
  // counts what the full plan counts.
  EXPECT(counts.num_clusters == Z.num_clusters && counts.num_cameras == Z.num_cameras &&
         counts.num_tiles == Z.num_tiles && counts.num_values == Z.num_values &&
         counts.max_cameras == Z.max_cameras && counts.finish_capacity == Z.finish_capacity);
  EXPECT(counts.pairs.num_blocks == F.num_blocks && counts.pairs.num_pairs == F.num_pairs &&
         counts.pairs.num_chunks == F.num_chunks && counts.pairs.plan_bytes == F.plan_bytes);
  EXPECT(counts.pairs.pairs.empty() && counts.pairs.block_row.empty() && counts.cameras.empty() &&
         counts.tile_of_plan.empty() && counts.plan_of_tile.empty() && counts.finish.empty());
  if (G == 1)
    EXPECT(counts.pairs.num_blocks == full.num_blocks && counts.pairs.num_pairs == full.num_pairs &&
           counts.pairs.num_chunks == full.num_chunks && counts.pairs.plan_bytes == full.plan_bytes);
  std::printf("  %-34s %3d cameras %3d clusters (largest %2lld): %4lld of %4lld blocks kept, %6lld pairs, "
              "%4lld chunks, longest list %4lld, %3lld tiles (%lld empty, %lld finished)\n",
              what, C, (int)G, (long long)largest, (long long)F.num_blocks, (long long)full.num_blocks,
              (long long)F.num_pairs, (long long)F.num_chunks, (long long)longest, (long long)tiles,
              (long long)Z.empty_tiles.size(), (long long)Z.finish.size());
}

std::vector<int32_t> Labels(int C, int32_t (*f)(int)) {
  std::vector<int32_t> l((size_t)C);
  for (int c = 0; c < C; ++c) l[(size_t)c] = f(c);
  return l;
}

// ---- The kernels' arithmetic on the host, in their order.  T holds the tiles
// of the lower triangle: entry (r, c) of block (I, J), J <= I, at
// El(I (I + 1) / 2 + J, r, c) = 81 t + 9 c + r (csrc/cluster_kernels.hpp).
int El(int t, int r, int c) { return 81 * t + 9 * c + r; }
int Tile(int I, int J) { return I * (I + 1) / 2 + J; }

bool PivotOk(double p) { return p > 0.0 && std::isfinite(p); }

// ClusterFactorKernel: returns false (T and inv zeroed) on a bad pivot.
bool Factor(int nc, std::vector<double>* tiles, std::vector<double>* inv_diag) {
  std::vector<double>& T = *tiles;
  std::vector<double>& inv = *inv_diag;
  inv.assign((size_t)(9 * nc), 0.0);
  bool ok = true;
  for (int k = 0; k < nc; ++k) {
    const int tkk = Tile(k, k);
    // 1. lane r holds row r of the diagonal tile
    double row[9][9];
    for (int r = 0; r < 9; ++r)
      for (int c = 0; c < 9; ++c) row[r][c] = T[(size_t)El(tkk, r, c)];
    for (int c = 0; c < 9; ++c) {
      const double piv = row[c][c];
      ok = ok && PivotOk(piv);
      const double l = std::sqrt(piv), iv = 1.0 / l;
      double lc[9];
      for (int r = 0; r < 9; ++r) lc[r] = r == c ? l : row[r][c] * iv;
      for (int r = 0; r < 9; ++r) row[r][c] = lc[r];
      inv[(size_t)(9 * k + c)] = iv;
      for (int j = c + 1; j < 9; ++j)
        for (int r = 0; r < 9; ++r) row[r][j] -= lc[r] * lc[j];
    }
    for (int r = 0; r < 9; ++r)
      for (int c = 0; c < 9; ++c) T[(size_t)El(tkk, r, c)] = c <= r ? row[r][c] : 0.0;
    // 2. the panel
    for (int I = k + 1; I < nc; ++I)
      for (int r = 0; r < 9; ++r) {
        const int t = Tile(I, k);
        double x[9];
        for (int c = 0; c < 9; ++c) {
          double v = T[(size_t)El(t, r, c)];
          for (int j = 0; j < c; ++j) v -= x[j] * T[(size_t)El(tkk, c, j)];
          x[c] = v * inv[(size_t)(9 * k + c)];
        }
        for (int c = 0; c < 9; ++c) T[(size_t)El(t, r, c)] = x[c];
      }
    // 3. the trailing tiles
    for (int I = k + 1; I < nc; ++I)
      for (int J = k + 1; J <= I; ++J)
        for (int c = 0; c < 9; ++c)
          for (int r = 0; r < 9; ++r) {
            double v = T[(size_t)El(Tile(I, J), r, c)];
            for (int t = 0; t < 9; ++t) v -= T[(size_t)El(Tile(I, k), r, t)] * T[(size_t)El(Tile(J, k), c, t)];
            T[(size_t)El(Tile(I, J), r, c)] = v;
          }
  }
  if (!ok) {
    std::fill(T.begin(), T.end(), 0.0);
    std::fill(inv.begin(), inv.end(), 0.0);
  }
  return ok;
}

// ClusterApplyKernel: v = L^-T L^-1 x.
void Apply(int nc, const std::vector<double>& T, const std::vector<double>& inv, std::vector<double>* vec) {
  std::vector<double>& v = *vec;
  const int n = 9 * nc;
  for (int k = 0; k < nc; ++k) {
    const int tkk = Tile(k, k);
    double x[9], w[9];
    for (int r = 0; r < 9; ++r) x[r] = v[(size_t)(9 * k + r)];
    for (int c = 0; c < 9; ++c) {
      w[c] = x[c] * inv[(size_t)(9 * k + c)];
      for (int r = c + 1; r < 9; ++r) x[r] -= T[(size_t)El(tkk, r, c)] * w[c];
    }
    for (int r = 0; r < 9; ++r) v[(size_t)(9 * k + r)] = w[r];
    for (int row = 9 * (k + 1); row < n; ++row) {
      const int I = row / 9, rr = row % 9;
      double s = v[(size_t)row];
      for (int c = 0; c < 9; ++c) s -= T[(size_t)El(Tile(I, k), rr, c)] * v[(size_t)(9 * k + c)];
      v[(size_t)row] = s;
    }
  }
  for (int k = nc - 1; k >= 0; --k) {
    const int tkk = Tile(k, k);
    double x[9], z[9];
    for (int r = 0; r < 9; ++r) x[r] = v[(size_t)(9 * k + r)];
    for (int c = 8; c >= 0; --c) {
      z[c] = x[c] * inv[(size_t)(9 * k + c)];
      for (int r = 0; r < c; ++r) x[r] -= T[(size_t)El(tkk, c, r)] * z[c];
    }
    for (int r = 0; r < 9; ++r) v[(size_t)(9 * k + r)] = z[r];
    for (int row = 0; row < 9 * k; ++row) {
      const int J = row / 9, rr = row % 9;
      double s = v[(size_t)row];
      for (int c = 0; c < 9; ++c) s -= T[(size_t)El(Tile(k, J), c, rr)] * v[(size_t)(9 * k + c)];
      v[(size_t)row] = s;
    }
  }
}

double Gamma(int k) {
  const double u = std::ldexp(1.0, -53);
  return k * u / (1.0 - k * u);
}

// A symmetric positive definite matrix: M = B B^T / n + 0.05 I, B uniform in
// [-1, 1] (entries of one scale, so that the normwise eta is not flattered
// by a few large rows).
void Replay(int nc, const char* dir) {
  const int n = 9 * nc;
  std::vector<double> B((size_t)(n * n)), M((size_t)(n * n)), r((size_t)n);
  for (double& v : B) v = 2.0 * Uniform() - 1.0;
  for (double& v : r) v = 2.0 * Uniform() - 1.0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0.0;
      for (int k = 0; k < n; ++k) s += B[(size_t)(i * n + k)] * B[(size_t)(j * n + k)];
      s = s / n + (i == j ? 0.05 : 0.0);
      M[(size_t)(i * n + j)] = M[(size_t)(j * n + i)] = s;
    }
  std::vector<double> T((size_t)(81 * nc * (nc + 1) / 2)), inv;
  for (int I = 0; I < nc; ++I)
    for (int J = 0; J <= I; ++J)
      for (int rr = 0; rr < 9; ++rr)
        for (int c = 0; c < 9; ++c) T[(size_t)El(Tile(I, J), rr, c)] = M[(size_t)((9 * I + rr) * n + 9 * J + c)];
  EXPECT(Factor(nc, &T, &inv));
  std::vector<double> z = r;
  Apply(nc, T, inv, &z);
  double res = 0.0, nm = 0.0, nz = 0.0, nr = 0.0;
  for (int i = 0; i < n; ++i) {
    long double s = 0.0L;
    double rowsum = 0.0;
    for (int j = 0; j < n; ++j) {
      s += (long double)M[(size_t)(i * n + j)] * z[(size_t)j];
      rowsum += std::fabs(M[(size_t)(i * n + j)]);
    }
    res = std::max(res, (double)fabsl(s - r[(size_t)i]));
    nm = std::max(nm, rowsum);
    nz = std::max(nz, std::fabs(z[(size_t)i]));
    nr = std::max(nr, std::fabs(r[(size_t)i]));
  }
  const double eta = res / (nm * nz + nr), bound = n * Gamma(3 * n + 1);
  std::printf("  replay %2d cameras (n = %3d): eta %.3e, bound %.3e\n", nc, n, eta, bound);
  EXPECT(eta <= bound);
  if (dir) {
    const std::string path = std::string(dir) + "/replay_" + std::to_string(nc) + ".bin";
    std::FILE* f = std::fopen(path.c_str(), "wb");
    EXPECT(f != nullptr);
    if (f) {
      EXPECT(std::fwrite(M.data(), sizeof(double), M.size(), f) == M.size());
      EXPECT(std::fwrite(r.data(), sizeof(double), r.size(), f) == r.size());
      EXPECT(std::fwrite(z.data(), sizeof(double), z.size(), f) == z.size());
      std::fclose(f);
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  std::printf("CLUSTER_JACOBI plan and replay driver\n");
  {
    // BAL-shaped, 10 cameras: singletons, one cluster, interleaved.
    std::vector<std::vector<int>> cams(80);
    for (int p = 0; p < 80; ++p)
      for (int k = 0; k < 2 + (p + 1) % 4; ++k) cams[p].push_back((p * 7 + k * 3) % 10);
    CheckPlan("singletons", 10, cams, Labels(10, [](int c) { return (int32_t)c; }), 10);
    CheckPlan("one cluster of all", 10, cams, Labels(10, [](int) { return (int32_t)0; }), 1);
    CheckPlan("interleaved (0,3,6,9 / 1,4,7 / ..)", 10, cams, Labels(10, [](int c) { return (int32_t)(c % 3); }), 3);
    CheckPlan("two halves", 10, cams, Labels(10, [](int c) { return (int32_t)(c / 5); }), 2);
  }
  {
    // camera 3 of 7 unobserved, cameras 5 and 6 share no point: {0,3,5,6} / {1,2,4}
    const std::vector<std::vector<int>> cams = {{0, 1, 2}, {2, 4, 5}, {4, 6, 0}, {1, 5}, {0, 2, 4, 6}, {0, 5}};
    const std::vector<int32_t> label = {0, 1, 1, 0, 1, 0, 0};
    CheckPlan("unobserved + non-covisible pair", 7, cams, label, 2);
    CheckPlan("unobserved, singletons", 7, cams, Labels(7, [](int c) { return (int32_t)c; }), 7);
    CheckPlan("unobserved, one cluster", 7, cams, Labels(7, [](int) { return (int32_t)0; }), 1);
  }
  {
    const std::vector<std::vector<int>> cams = {{0, 0, 1}, {2, 2, 2, 3}, {1, 4}, {3, 3, 0, 0, 0}, {4, 2}, {1, 0, 1}};
    CheckPlan("duplicates", 5, cams, {0, 0, 1, 1, 0}, 2);
    CheckPlan("duplicates, one cluster", 5, cams, {0, 0, 0, 0, 0}, 1);
  }
  {
    // lists above 64 and above 128 pairs: 3 cameras, 150 points
    std::vector<std::vector<int>> cams(150);
    for (int p = 0; p < 150; ++p) cams[p] = p % 3 ? std::vector<int>{0, 1, 2} : std::vector<int>{2, 0};
    CheckPlan("several chunks, {0,2} / {1}", 3, cams, {0, 1, 0}, 2);
    CheckPlan("several chunks, one cluster", 3, cams, {0, 0, 0}, 1);
  }
  {
    // clusters of exactly 16 of 40 cameras (and one of 8), membership scattered
    std::vector<std::vector<int>> cams(400);
    for (int p = 0; p < 400; ++p)
      for (int k = 0; k < 2 + p % 4; ++k) cams[p].push_back((p * 13 + k * (1 + p % 7)) % 40);
    CheckPlan("16 + 16 + 8 in runs", 40, cams, Labels(40, [](int c) { return (int32_t)(c / 16); }), 3);
    CheckPlan("16 + 16 + 8 scattered", 40, cams,
              Labels(40, [](int c) { return (int32_t)(c % 5 < 2 ? 0 : c % 5 < 4 ? 1 : 2); }), 3);
  }
  CheckPlan("no residual blocks", 4, {}, {1, 0, 1, 0}, 2);
  {
    // The refusals of the partition.
    const int32_t ids[] = {2, 0, 3, 0, 4, 1};
    cse::SchurClusterPlan Z;
    const std::vector<int32_t> ok = {0, 1, 0};
    EXPECT(cse::PlanSchurClusters(ids, 3, 2, 3, ok.data(), 2, true, &Z) == CSE_OK);
    EXPECT(cse::PlanSchurClusters(ids, 3, 2, 3, nullptr, 2, true, &Z) == CSE_ERR_INVALID);
    const std::vector<int32_t> out_of_range = {0, 2, 0}, negative = {0, -1, 0}, unused = {0, 2, 0};
    EXPECT(cse::PlanSchurClusters(ids, 3, 2, 3, out_of_range.data(), 2, true, &Z) == CSE_ERR_INVALID);
    EXPECT(cse::PlanSchurClusters(ids, 3, 2, 3, negative.data(), 2, true, &Z) == CSE_ERR_INVALID);
    EXPECT(cse::PlanSchurClusters(ids, 3, 2, 3, unused.data(), 3, true, &Z) == CSE_ERR_INVALID);
    EXPECT(cse::PlanSchurClusters(ids, 3, 3, 3, ok.data(), 2, true, &Z) == CSE_ERR_INVALID);  // an id outside
    const std::vector<int32_t> big(17, 0), fits(16, 0);
    EXPECT(cse::ValidateSchurClusters(big.data(), 17, 1) == CSE_ERR_UNSUPPORTED);
    EXPECT(cse::ValidateSchurClusters(fits.data(), 16, 1) == CSE_OK);
  }
  const char* dir = argc > 1 ? argv[1] : nullptr;
  for (int nc : {1, 2, 3, 4, 7, 11, 16}) Replay(nc, dir);
  {
    // A pivot that is not positive: zeros, and the apply gives zeros.
    std::vector<double> T((size_t)(81 * 3), 0.0), inv;
    for (int r = 0; r < 9; ++r) T[(size_t)El(Tile(0, 0), r, r)] = T[(size_t)El(Tile(1, 1), r, r)] = 1.0;
    T[(size_t)El(Tile(1, 1), 4, 4)] = -1.0;
    EXPECT(!Factor(2, &T, &inv));
    std::vector<double> v(18, 1.0);
    Apply(2, T, inv, &v);
    for (double e : v) EXPECT(e == 0.0);
  }
  if (g_failures) {
    std::printf("%d FAILED\n", g_failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
