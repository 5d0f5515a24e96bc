// schur_tridiagonal_driver.cpp -- the host side of CLUSTER_TRIDIAGONAL
// (cse_schur_set_cluster_forest, cse_schur_cluster_tridiagonal): the forest's
// validation and paths (cse::ValidateSchurForest), the pair plan filtered by
// label or forest edge and the tile layout (cse::PlanSchurTridiagonal,
// csrc/plan.cpp), built by g++ with AddressSanitizer + UBSan from plan.cpp,
// layout.cpp and this file (tests/test_schur_tridiagonal.py runs it; no HIP,
// no GPU).
//
// Per problem, partition and forest the plan is checked against brute force
// over every (point, b, b'): exactly the blocks (c, c') whose labels are equal
// or joined by an edge, each block's pair list in (point, b, b') order and list
// and chunk cut equal to the UNFILTERED plan's, entry by entry; the clusters'
// triangles as CLUSTER_JACOBI's; per edge the rectangle with tile (i, j) =
// S(min, max) of camera i of g and camera j of h -- both transposition cases
// are counted; the finish list and the empty tiles.  With no edge the plan is
// cse::PlanSchurClusters', table by table.  The paths against a separate walk.
//
// Then a host replay of TridiagonalFactorKernel (both passes) and
// TridiagonalApplyKernel (csrc/cluster_kernels.hpp) in the kernels' order, on
// the plan's own tiles filled from a dense symmetric matrix: per path, for
// M z = r with M assembled independently from the labels and edges,
//     eta = |M z - r|_inf / (|M|_inf |z|_inf + |r|_inf) <= n gamma_{3n+1},
// n the path's dimension (Higham, Thm 10.4 in normwise form).  The retry on an
// injected M = T (x) I_9, T = [[1, a, 0], [a, 1, a], [0, a, 1]]: a = 0.8 fails
// the first pass (1 - 0.8 sqrt 2 < 0) and passes the second (a = 0.4); a = 0.6
// needs none.  With a directory as argument, M, r and z of every replayed path
// are written there for the caller to compare with its own solver.
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

namespace cse {
std::string& LastError();  // csrc/layout.cpp: cse_last_error's text
}

namespace {

uint64_t lcg = 0x9E3779B97F4A7C15ull;
double Uniform() {
  lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(lcg >> 11) * (1.0 / 9007199254740992.0);
}

typedef std::pair<int32_t, int32_t> Key;
typedef std::vector<Key> PairList;
typedef std::vector<std::vector<int>> Cams;
typedef std::vector<Key> Edges;

std::vector<int32_t> Flat(const Edges& e) {
  std::vector<int32_t> f;
  for (const Key& k : e) {
    f.push_back(k.first);
    f.push_back(k.second);
  }
  return f;
}

bool Joined(const Edges& edges, int32_t a, int32_t b) {
  for (const Key& k : edges)
    if ((k.first == a && k.second == b) || (k.first == b && k.second == a)) return true;
  return false;
}

// The paths by a walk of their own: components by label propagation, each
// listed from its endpoint with the smaller label, sorted by first cluster.
std::vector<std::vector<int32_t>> PathsOf(int32_t G, const Edges& edges) {
  std::vector<int32_t> comp((size_t)G);
  for (int32_t g = 0; g < G; ++g) comp[(size_t)g] = g;
  for (int32_t pass = 0; pass < G; ++pass)
    for (const Key& k : edges) {
      const int32_t m = std::min(comp[(size_t)k.first], comp[(size_t)k.second]);
      comp[(size_t)k.first] = comp[(size_t)k.second] = m;
    }
  std::vector<std::vector<int32_t>> paths;
  for (int32_t root = 0; root < G; ++root) {
    std::vector<int32_t> members;
    for (int32_t g = 0; g < G; ++g)
      if (comp[(size_t)g] == root) members.push_back(g);
    if (members.empty()) continue;
    int32_t start = -1;
    for (int32_t g : members) {
      int degree = 0;
      for (int32_t h : members) degree += Joined(edges, g, h) ? 1 : 0;
      if (degree < 2 && start < 0) start = g;  // members ascend: the smaller endpoint
    }
    std::vector<int32_t> path = {start};
    while (path.size() < members.size())
      for (int32_t h : members)
        if (Joined(edges, path.back(), h) && std::find(path.begin(), path.end(), h) == path.end()) {
          path.push_back(h);
          break;
        }
    paths.push_back(path);
  }
  std::sort(paths.begin(), paths.end());
  return paths;
}

std::vector<int32_t> IdsOf(const Cams& cams) {
  const int P = (int)cams.size();
  std::vector<int32_t> ids;
  for (int p = 0; p < P; ++p)
    for (int c : cams[p]) {
      ids.push_back(P + c);
      ids.push_back(p);
    }
  return ids;
}

int g_direct = 0, g_transposed = 0;  // rectangle tiles met in either orientation

void CheckPlan(const char* what, int C, const Cams& cams, const std::vector<int32_t>& label, int32_t G,
               const Edges& edges) {
  const int before = g_failures;
  const int P = (int)cams.size();
  const std::vector<int32_t> ids = IdsOf(cams), flat = Flat(edges);
  const int64_t n = (int64_t)ids.size() / 2;
  const int32_t E = (int32_t)edges.size();
  cse::SchurPairPlan full;
  EXPECT(cse::PlanSchurPairs(ids.data(), n, false, &full) == CSE_OK);
  cse::SchurTridiagonalPlan Z, counts;
  EXPECT(cse::PlanSchurTridiagonal(ids.data(), n, P, C, label.data(), G, flat.data(), E, false, &Z) == CSE_OK);
  EXPECT(cse::PlanSchurTridiagonal(ids.data(), n, P, C, label.data(), G, flat.data(), E, true, &counts) == CSE_OK);
  if (g_failures != before) return;
  const cse::SchurPairPlan& F = Z.pairs;

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
        if (label[(size_t)c] == label[(size_t)c2] || Joined(edges, label[(size_t)c], label[(size_t)c2]))
          want[Key(c, c2)].push_back(Key((int32_t)b, (int32_t)b2));
      }
    r0 = r1;
  }
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
  for (const auto& kv : want) {
    const PairList& list = kv.second;
    EXPECT(Key(F.block_row[(size_t)k] - P, F.block_col[(size_t)k] - P) == kv.first);
    const int64_t p0 = F.pair_begin[(size_t)k], p1 = F.pair_begin[(size_t)k + 1];
    EXPECT(p0 == npairs && p1 - p0 == (int64_t)list.size());
    if (p1 - p0 != (int64_t)list.size()) return;
    for (int64_t i = 0; i < p1 - p0; ++i)
      EXPECT(Key(F.pairs[(size_t)(2 * (p0 + i))], F.pairs[(size_t)(2 * (p0 + i) + 1)]) == list[(size_t)i]);
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

  // The clusters' part of the layout is CLUSTER_JACOBI's.
  cse::SchurClusterPlan J;
  EXPECT(cse::PlanSchurClusters(ids.data(), n, P, C, label.data(), G, false, &J) == CSE_OK);
  EXPECT(Z.camera_begin == J.camera_begin && Z.cameras == J.cameras && Z.first_tile == J.first_tile &&
         Z.value_begin == J.value_begin);
  EXPECT(Z.num_clusters == G && Z.num_cameras == C && Z.num_edges == E && Z.num_cluster_tiles == J.num_tiles &&
         Z.max_cameras == J.max_cameras);
  if (E == 0) {
    EXPECT(F.block_row == J.pairs.block_row && F.block_col == J.pairs.block_col && F.pairs == J.pairs.pairs &&
           F.pair_begin == J.pairs.pair_begin && F.chunk_off == J.pairs.chunk_off &&
           F.chunk_block == J.pairs.chunk_block && F.plan_bytes == J.pairs.plan_bytes);
    EXPECT(Z.tile_of_plan == J.tile_of_plan && Z.plan_of_tile == J.plan_of_tile && Z.tile_camera == J.tile_camera &&
           Z.num_tiles == J.num_tiles && Z.num_values == J.num_values);
    EXPECT(std::set<int32_t>(Z.finish.begin(), Z.finish.end()) == std::set<int32_t>(J.finish.begin(), J.finish.end()));
    EXPECT(Z.empty_tiles == J.empty_tiles && Z.finish_capacity == J.finish_capacity);
  }
  // The rectangles.
  std::vector<int> local((size_t)C, -1), size((size_t)G, 0);
  for (int32_t g = 0; g < G; ++g) {
    size[(size_t)g] = Z.camera_begin[(size_t)g + 1] - Z.camera_begin[(size_t)g];
    for (int32_t i = Z.camera_begin[(size_t)g]; i < Z.camera_begin[(size_t)g + 1]; ++i)
      local[(size_t)Z.cameras[(size_t)i]] = i - Z.camera_begin[(size_t)g];
  }
  EXPECT((int64_t)Z.edge_tile.size() == E + 1 && (int64_t)Z.edge_value.size() == E + 1 && Z.edges == flat);
  if (g_failures != before) return;
  int64_t tiles = J.num_tiles, values = J.num_values, step = J.max_cameras;
  std::map<Key, int64_t> tile_want;  // (c <= c2) -> tile
  for (int32_t g = 0; g < G; ++g)
    for (int j = 0; j < size[(size_t)g]; ++j)
      for (int i = 0; i <= j; ++i)
        tile_want[Key(Z.cameras[(size_t)(Z.camera_begin[(size_t)g] + i)],
                      Z.cameras[(size_t)(Z.camera_begin[(size_t)g] + j)])] =
            Z.first_tile[(size_t)g] + cse::ClusterTile(i, j);
  for (int32_t e = 0; e < E; ++e) {
    const int32_t g = edges[(size_t)e].first, h = edges[(size_t)e].second;
    EXPECT(Z.edge_tile[(size_t)e] == tiles && Z.edge_value[(size_t)e] == values);
    for (int i = 0; i < size[(size_t)g]; ++i)
      for (int j = 0; j < size[(size_t)h]; ++j) {
        const int32_t a = Z.cameras[(size_t)(Z.camera_begin[(size_t)g] + i)];
        const int32_t b = Z.cameras[(size_t)(Z.camera_begin[(size_t)h] + j)];
        // The tile holds the plan's block S(min, max).
        tile_want[Key(std::min(a, b), std::max(a, b))] = tiles + (int64_t)i * size[(size_t)h] + j;
        ++(a < b ? g_direct : g_transposed);
      }
    tiles += (int64_t)size[(size_t)g] * size[(size_t)h];
    values += 81LL * size[(size_t)g] * size[(size_t)h];
    step = std::max<int64_t>(step, size[(size_t)g] + size[(size_t)h]);
  }
  EXPECT(Z.edge_tile[(size_t)E] == tiles && Z.edge_value[(size_t)E] == values);
  EXPECT(Z.num_tiles == tiles && Z.num_values == values && Z.max_step_cameras == step);
  EXPECT((int64_t)tile_want.size() == tiles);  // every tile is one camera pair's
  EXPECT((int64_t)Z.tile_of_plan.size() == F.num_blocks && (int64_t)Z.plan_of_tile.size() == tiles &&
         (int64_t)Z.tile_camera.size() == tiles);
  if (g_failures != before) return;
  std::vector<int> written((size_t)tiles, 0);
  for (int64_t b = 0; b < F.num_blocks; ++b) {
    const Key cc(F.block_row[(size_t)b] - P, F.block_col[(size_t)b] - P);
    const auto at = tile_want.find(cc);
    EXPECT(at != tile_want.end());
    if (at == tile_want.end()) continue;
    EXPECT(Z.tile_of_plan[(size_t)b] == at->second && Z.plan_of_tile[(size_t)at->second] == b);
    ++written[(size_t)at->second];
  }
  std::set<int32_t> finish_want, empty_want;
  for (const auto& kv : tile_want) {
    const bool has = want.count(kv.first) != 0;
    EXPECT(written[(size_t)kv.second] == (has ? 1 : 0));
    EXPECT((Z.plan_of_tile[(size_t)kv.second] >= 0) == has);
    if (!has) {
      empty_want.insert((int32_t)kv.second);
      if (kv.first.first == kv.first.second) {
        EXPECT(!observed[(size_t)kv.first.first]);
        EXPECT(Z.tile_camera[(size_t)kv.second] == kv.first.first);
        finish_want.insert((int32_t)kv.second);
      }
    } else if (want[kv.first].size() > (size_t)cse::kSchurPairChunk) {
      finish_want.insert((int32_t)kv.second);
    }
  }
  EXPECT(std::set<int32_t>(Z.finish.begin(), Z.finish.end()) == finish_want && Z.finish.size() == finish_want.size());
  EXPECT(std::set<int32_t>(Z.empty_tiles.begin(), Z.empty_tiles.end()) == empty_want &&
         Z.empty_tiles.size() == empty_want.size());
  EXPECT((int64_t)Z.finish.size() <= Z.finish_capacity);

  // The paths.
  const std::vector<std::vector<int32_t>> paths = PathsOf(G, edges);
  EXPECT(Z.num_paths == (int64_t)paths.size() && (int64_t)Z.paths.path_begin.size() == Z.num_paths + 1);
  EXPECT((int64_t)Z.paths.path_cluster.size() == G && (int64_t)Z.paths.path_edge.size() == G);
  if (g_failures != before) return;
  int64_t longest_path = 0;
  for (size_t p = 0; p < paths.size(); ++p) {
    const int32_t q0 = Z.paths.path_begin[p], q1 = Z.paths.path_begin[p + 1];
    EXPECT(q1 - q0 == (int32_t)paths[p].size());
    if (q1 - q0 != (int32_t)paths[p].size()) return;
    longest_path = std::max<int64_t>(longest_path, q1 - q0);
    for (int32_t q = q0; q < q1; ++q) {
      EXPECT(Z.paths.path_cluster[(size_t)q] == paths[p][(size_t)(q - q0)]);
      const int32_t pe = Z.paths.path_edge[(size_t)q];
      if (q == q1 - 1) {
        EXPECT(pe == -1);
        continue;
      }
      EXPECT(pe >= 0 && (pe >> 1) < E);
      if (pe < 0 || (pe >> 1) >= E) continue;
      const Key& ed = edges[(size_t)(pe >> 1)];
      const int32_t here = Z.paths.path_cluster[(size_t)q], next = paths[p][(size_t)(q + 1 - q0)];
      EXPECT((pe & 1) ? (ed.second == here && ed.first == next) : (ed.first == here && ed.second == next));
    }
  }
  EXPECT(Z.longest_path == longest_path);

  EXPECT(counts.num_tiles == Z.num_tiles && counts.num_values == Z.num_values && counts.num_paths == Z.num_paths &&
         counts.max_step_cameras == Z.max_step_cameras && counts.longest_path == Z.longest_path &&
         counts.finish_capacity == Z.finish_capacity && counts.num_edges == Z.num_edges);
  EXPECT(counts.pairs.num_blocks == F.num_blocks && counts.pairs.num_pairs == F.num_pairs &&
         counts.pairs.num_chunks == F.num_chunks && counts.pairs.plan_bytes == F.plan_bytes);
  EXPECT(counts.pairs.pairs.empty() && counts.cameras.empty() && counts.tile_of_plan.empty() &&
         counts.edge_tile.empty() && counts.finish.empty());
  std::printf("  %-40s %3d cameras %3d clusters %2d edges %2lld paths (longest %2lld): %4lld of %4lld blocks kept, "
              "%6lld pairs, %4lld chunks, longest list %4lld, %3lld tiles (%lld empty, %lld finished)\n",
              what, C, (int)G, (int)E, (long long)Z.num_paths, (long long)Z.longest_path, (long long)F.num_blocks,
              (long long)full.num_blocks, (long long)F.num_pairs, (long long)F.num_chunks, (long long)longest,
              (long long)tiles, (long long)Z.empty_tiles.size(), (long long)Z.finish.size());
}

std::vector<int32_t> Labels(int C, int32_t (*f)(int)) {
  std::vector<int32_t> l((size_t)C);
  for (int c = 0; c < C; ++c) l[(size_t)c] = f(c);
  return l;
}

// ---- The kernels' arithmetic on the host, in their order
// (csrc/cluster_kernels.hpp).
int El(int t, int r, int c) { return 81 * t + 9 * c + r; }
int Tile(int I, int J) { return I * (I + 1) / 2 + J; }
bool PivotOk(double p) { return p > 0.0 && std::isfinite(p); }

// ClusterFactorColumns: tile columns [0, ncols) of the nc x nc tile triangle.
void FactorColumns(std::vector<double>& T, std::vector<double>& inv, bool* bad, int nc, int ncols) {
  for (int k = 0; k < ncols; ++k) {
    const int tkk = Tile(k, k);
    double row[9][9];
    for (int r = 0; r < 9; ++r)
      for (int c = 0; c < 9; ++c) row[r][c] = T[(size_t)El(tkk, r, c)];
    for (int c = 0; c < 9; ++c) {
      const double piv = row[c][c];
      if (!PivotOk(piv)) *bad = true;
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
    for (int I = k + 1; I < nc; ++I)
      for (int J = k + 1; J <= I; ++J)
        for (int c = 0; c < 9; ++c)
          for (int r = 0; r < 9; ++r) {
            double v = T[(size_t)El(Tile(I, J), r, c)];
            for (int t = 0; t < 9; ++t) v -= T[(size_t)El(Tile(I, k), r, t)] * T[(size_t)El(Tile(J, k), c, t)];
            T[(size_t)El(Tile(I, J), r, c)] = v;
          }
  }
}

struct Device {
  cse::SchurTridiagonalPlan P;
  std::vector<double> tiles, factor, inv_diag, scratch;
  int failed = 0, status = 0;
  int Size(int g) const { return P.camera_begin[(size_t)g + 1] - P.camera_begin[(size_t)g]; }
};

// TridiagonalFactorKernel, path p.
void FactorPath(Device* D, int p, int scaled) {
  const cse::SchurTridiagonalPlan& P = D->P;
  if (scaled && D->failed == 0) return;
  const int q0 = P.paths.path_begin[(size_t)p], q1 = P.paths.path_begin[(size_t)p + 1];
  const int ms = (int)P.max_step_cameras;
  std::vector<double> T((size_t)(81 * ms * (ms + 1) / 2), 0.0), inv((size_t)(9 * ms), 0.0);
  bool bad = false;
  int g = P.paths.path_cluster[(size_t)q0], n1 = D->Size(g);
  for (int idx = 0; idx < 81 * n1 * (n1 + 1) / 2; ++idx) T[(size_t)idx] = D->tiles[(size_t)(P.first_tile[(size_t)g] * 81 + idx)];
  for (int q = q0; q < q1; ++q) {
    const int pe = P.paths.path_edge[(size_t)q], e = pe >> 1;
    int h = -1, n2 = 0;
    if (pe >= 0) {
      h = P.paths.path_cluster[(size_t)q + 1];
      n2 = D->Size(h);
      const int c1 = P.camera_begin[(size_t)g], c2 = P.camera_begin[(size_t)h];
      const bool flip = (pe & 1) != 0;
      const double scale = scaled ? 0.5 : 1.0;
      for (int idx = 0; idx < 81 * n1 * n2; ++idx) {
        const int t = idx / 81, el = idx % 81, j = t / n1, i = t % n1;
        const int src_tile = flip ? j * n1 + i : i * n2 + j;
        const bool direct = P.cameras[(size_t)(c1 + i)] < P.cameras[(size_t)(c2 + j)];
        const int src_el = direct ? el : (el % 9) * 9 + el / 9;
        T[(size_t)(81 * Tile(n1 + j, i) + el)] = scale * D->tiles[(size_t)((P.edge_tile[(size_t)e] + src_tile) * 81 + src_el)];
      }
      for (int J = 0; J < n2; ++J)
        for (int I = J; I < n2; ++I)
          for (int el = 0; el < 81; ++el)
            T[(size_t)(81 * Tile(n1 + I, n1 + J) + el)] = D->tiles[(size_t)((P.first_tile[(size_t)h] + Tile(I, J)) * 81 + el)];
    }
    FactorColumns(T, inv, &bad, n1 + n2, n1);
    for (int idx = 0; idx < 81 * n1 * (n1 + 1) / 2; ++idx) D->factor[(size_t)(P.first_tile[(size_t)g] * 81 + idx)] = T[(size_t)idx];
    for (int idx = 0; idx < 9 * n1; ++idx) D->inv_diag[(size_t)(9 * P.camera_begin[(size_t)g] + idx)] = inv[(size_t)idx];
    if (pe >= 0) {
      for (int idx = 0; idx < 81 * n1 * n2; ++idx) {
        const int t = idx / 81, el = idx % 81, j = t / n1, i = t % n1;
        D->factor[(size_t)(P.edge_tile[(size_t)e] * 81 + idx)] = T[(size_t)(81 * Tile(n1 + j, i) + el)];
      }
      // ascending: a destination is never above its source
      for (int t = 0; t < n2 * (n2 + 1) / 2; ++t) {
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= t) ++I;
        const int J = t - I * (I + 1) / 2;
        for (int el = 0; el < 81; ++el) T[(size_t)(81 * t + el)] = T[(size_t)(81 * Tile(n1 + I, n1 + J) + el)];
      }
      g = h;
      n1 = n2;
    }
  }
  if (!bad) return;
  if (!scaled) {
    D->failed = 1;
    return;
  }
  for (int q = q0; q < q1; ++q) {
    const int c = P.paths.path_cluster[(size_t)q], nc = D->Size(c);
    for (int idx = 0; idx < 81 * nc * (nc + 1) / 2; ++idx) D->factor[(size_t)(P.first_tile[(size_t)c] * 81 + idx)] = 0.0;
    for (int idx = 0; idx < 9 * nc; ++idx) D->inv_diag[(size_t)(9 * P.camera_begin[(size_t)c] + idx)] = 0.0;
    const int pe = P.paths.path_edge[(size_t)q];
    if (pe < 0) continue;
    for (int64_t idx = P.edge_tile[(size_t)(pe >> 1)] * 81; idx < P.edge_tile[(size_t)(pe >> 1) + 1] * 81; ++idx)
      D->factor[(size_t)idx] = 0.0;
  }
  D->status = 1;
}

// ClusterSubstituteForward / Backward on v with the tiles at T.
void SubstituteForward(const double* T, const double* inv, int nc, double* v) {
  const int n = 9 * nc;
  for (int k = 0; k < nc; ++k) {
    const int tkk = Tile(k, k);
    double x[9], w[9];
    for (int r = 0; r < 9; ++r) x[r] = v[9 * k + r];
    for (int c = 0; c < 9; ++c) {
      w[c] = x[c] * inv[9 * k + c];
      for (int r = c + 1; r < 9; ++r) x[r] -= T[El(tkk, r, c)] * w[c];
    }
    for (int r = 0; r < 9; ++r) v[9 * k + r] = w[r];
    for (int row = 9 * (k + 1); row < n; ++row) {
      const int I = row / 9, rr = row % 9;
      double s = v[row];
      for (int c = 0; c < 9; ++c) s -= T[El(Tile(I, k), rr, c)] * v[9 * k + c];
      v[row] = s;
    }
  }
}
void SubstituteBackward(const double* T, const double* inv, int nc, double* v) {
  for (int k = nc - 1; k >= 0; --k) {
    const int tkk = Tile(k, k);
    double x[9], z[9];
    for (int r = 0; r < 9; ++r) x[r] = v[9 * k + r];
    for (int c = 8; c >= 0; --c) {
      z[c] = x[c] * inv[9 * k + c];
      for (int r = 0; r < c; ++r) x[r] -= T[El(tkk, c, r)] * z[c];
    }
    for (int r = 0; r < 9; ++r) v[9 * k + r] = z[r];
    for (int row = 0; row < 9 * k; ++row) {
      const int J = row / 9, rr = row % 9;
      double s = v[row];
      for (int c = 0; c < 9; ++c) s -= T[El(Tile(k, J), c, rr)] * v[9 * k + c];
      v[row] = s;
    }
  }
}

// TridiagonalApplyKernel, path p; x and y may be one buffer.
void ApplyPath(Device* D, int p, const double* x, double* y, bool accumulate) {
  const cse::SchurTridiagonalPlan& P = D->P;
  const int q0 = P.paths.path_begin[(size_t)p], q1 = P.paths.path_begin[(size_t)p + 1];
  std::vector<double> v(144), other(144);
  int np = 0;
  for (int q = q0; q < q1; ++q) {
    const int g = P.paths.path_cluster[(size_t)q], cam0 = P.camera_begin[(size_t)g], nc = D->Size(g), n = 9 * nc;
    const double* T = &D->factor[(size_t)(P.first_tile[(size_t)g] * 81)];
    for (int idx = 0; idx < n; ++idx) v[(size_t)idx] = x[9 * P.cameras[(size_t)(cam0 + idx / 9)] + idx % 9];
    if (q > q0) {
      const double* panel = &D->factor[(size_t)(P.edge_tile[(size_t)(P.paths.path_edge[(size_t)q - 1] >> 1)] * 81)];
      for (int row = 0; row < n; ++row) {
        const int j = row / 9, rr = row % 9;
        double s = v[(size_t)row];
        for (int i = 0; i < np; ++i)
          for (int c = 0; c < 9; ++c) s -= panel[El(j * np + i, rr, c)] * other[(size_t)(9 * i + c)];
        v[(size_t)row] = s;
      }
    }
    SubstituteForward(T, &D->inv_diag[(size_t)(9 * cam0)], nc, v.data());
    for (int row = 0; row < n; ++row) {
      other[(size_t)row] = v[(size_t)row];
      D->scratch[(size_t)(9 * P.cameras[(size_t)(cam0 + row / 9)] + row % 9)] = v[(size_t)row];
    }
    np = nc;
  }
  for (int q = q1 - 1; q >= q0; --q) {
    const int g = P.paths.path_cluster[(size_t)q], cam0 = P.camera_begin[(size_t)g], nc = D->Size(g), n = 9 * nc;
    const double* T = &D->factor[(size_t)(P.first_tile[(size_t)g] * 81)];
    for (int idx = 0; idx < n; ++idx) v[(size_t)idx] = D->scratch[(size_t)(9 * P.cameras[(size_t)(cam0 + idx / 9)] + idx % 9)];
    if (q < q1 - 1) {
      const double* panel = &D->factor[(size_t)(P.edge_tile[(size_t)(P.paths.path_edge[(size_t)q] >> 1)] * 81)];
      for (int row = 0; row < n; ++row) {
        const int i = row / 9, c = row % 9;
        double s = v[(size_t)row];
        for (int j = 0; j < np; ++j)
          for (int rr = 0; rr < 9; ++rr) s -= panel[El(j * nc + i, rr, c)] * other[(size_t)(9 * j + rr)];
        v[(size_t)row] = s;
      }
    }
    SubstituteBackward(T, &D->inv_diag[(size_t)(9 * cam0)], nc, v.data());
    for (int row = 0; row < n; ++row) {
      other[(size_t)row] = v[(size_t)row];
      double* at = &y[9 * P.cameras[(size_t)(cam0 + row / 9)] + row % 9];
      *at = accumulate ? *at + v[(size_t)row] : v[(size_t)row];
    }
    np = nc;
  }
}

double Gamma(int k) {
  const double u = std::ldexp(1.0, -53);
  return k * u / (1.0 - k * u);
}

// The plan's tiles from a dense symmetric S of 9 C columns: every tile holds
// S(min, max) of its two cameras, row-major.
void FillTiles(Device* D, const std::vector<double>& S, int C, const std::vector<int32_t>& label, const Edges& edges) {
  const cse::SchurTridiagonalPlan& P = D->P;
  const int N = 9 * C;
  D->tiles.assign((size_t)(81 * P.num_tiles), 0.0);
  D->factor.assign((size_t)(81 * P.num_tiles), std::nan(""));
  D->inv_diag.assign((size_t)N, std::nan(""));
  D->scratch.assign((size_t)N, std::nan(""));
  auto put = [&](int64_t t, int a, int b) {  // a <= b
    for (int r = 0; r < 9; ++r)
      for (int c = 0; c < 9; ++c) D->tiles[(size_t)(81 * t + 9 * r + c)] = S[(size_t)((9 * a + r) * N + 9 * b + c)];
  };
  for (int32_t g = 0; g < (int32_t)P.num_clusters; ++g)
    for (int j = 0; j < D->Size(g); ++j)
      for (int i = 0; i <= j; ++i)
        put(P.first_tile[(size_t)g] + cse::ClusterTile(i, j), P.cameras[(size_t)(P.camera_begin[(size_t)g] + i)],
            P.cameras[(size_t)(P.camera_begin[(size_t)g] + j)]);
  for (size_t e = 0; e < edges.size(); ++e)
    for (int i = 0; i < D->Size(edges[e].first); ++i)
      for (int j = 0; j < D->Size(edges[e].second); ++j) {
        const int a = P.cameras[(size_t)(P.camera_begin[(size_t)edges[e].first] + i)];
        const int b = P.cameras[(size_t)(P.camera_begin[(size_t)edges[e].second] + j)];
        put(P.edge_tile[e] + (int64_t)i * D->Size(edges[e].second) + j, std::min(a, b), std::max(a, b));
      }
  (void)label;
}

// eta of path p's solve against M assembled from the labels and the edges,
// every edge block times edge_scale.
double PathEta(const Device& D, int p, const std::vector<double>& S, int C, const std::vector<int32_t>& label,
               const Edges& edges, double edge_scale, const std::vector<double>& r, const std::vector<double>& z,
               int* dim, const char* dir, const std::string& tag) {
  const cse::SchurTridiagonalPlan& P = D.P;
  std::vector<int> rows;
  for (int q = P.paths.path_begin[(size_t)p]; q < P.paths.path_begin[(size_t)p + 1]; ++q) {
    const int g = P.paths.path_cluster[(size_t)q];
    for (int i = P.camera_begin[(size_t)g]; i < P.camera_begin[(size_t)g + 1]; ++i)
      for (int k = 0; k < 9; ++k) rows.push_back(9 * P.cameras[(size_t)i] + k);
  }
  const int n = (int)rows.size(), N = 9 * C;
  std::vector<double> M((size_t)(n * n)), rp((size_t)n), zp((size_t)n);
  for (int i = 0; i < n; ++i) {
    rp[(size_t)i] = r[(size_t)rows[(size_t)i]];
    zp[(size_t)i] = z[(size_t)rows[(size_t)i]];
    for (int j = 0; j < n; ++j) {
      const int32_t la = label[(size_t)(rows[(size_t)i] / 9)], lb = label[(size_t)(rows[(size_t)j] / 9)];
      const double s = S[(size_t)(rows[(size_t)i] * N + rows[(size_t)j])];
      M[(size_t)(i * n + j)] = la == lb ? s : Joined(edges, la, lb) ? edge_scale * s : 0.0;
    }
  }
  double res = 0.0, nm = 0.0, nz = 0.0, nr = 0.0;
  for (int i = 0; i < n; ++i) {
    long double s = 0.0L;
    double rowsum = 0.0;
    for (int j = 0; j < n; ++j) {
      s += (long double)M[(size_t)(i * n + j)] * zp[(size_t)j];
      rowsum += std::fabs(M[(size_t)(i * n + j)]);
    }
    res = std::max(res, (double)fabsl(s - rp[(size_t)i]));
    nm = std::max(nm, rowsum);
    nz = std::max(nz, std::fabs(zp[(size_t)i]));
    nr = std::max(nr, std::fabs(rp[(size_t)i]));
  }
  *dim = n;
  if (dir) {
    const std::string path = std::string(dir) + "/replay_" + tag + "_" + std::to_string(p) + ".bin";
    std::FILE* f = std::fopen(path.c_str(), "wb");
    EXPECT(f != nullptr);
    if (f) {
      EXPECT(std::fwrite(M.data(), sizeof(double), M.size(), f) == M.size());
      EXPECT(std::fwrite(rp.data(), sizeof(double), rp.size(), f) == rp.size());
      EXPECT(std::fwrite(zp.data(), sizeof(double), zp.size(), f) == zp.size());
      std::fclose(f);
    }
  }
  return res / (nm * nz + nr);
}

// Builds the plan of `cams`, fills the tiles from S, runs both passes over
// every path in launch order and the apply; returns whether the second pass ran.
int Run(Device* D, int C, const Cams& cams, const std::vector<int32_t>& label, int32_t G, const Edges& edges,
        const std::vector<double>& S, const std::vector<double>& r, std::vector<double>* z, bool accumulate_in_place) {
  const std::vector<int32_t> ids = IdsOf(cams), flat = Flat(edges);
  EXPECT(cse::PlanSchurTridiagonal(ids.data(), (int64_t)ids.size() / 2, (int32_t)cams.size(), C, label.data(), G,
                                   flat.data(), (int32_t)edges.size(), false, &D->P) == CSE_OK);
  FillTiles(D, S, C, label, edges);
  D->failed = D->status = 0;
  for (int scaled = 0; scaled < 2; ++scaled)
    for (int p = 0; p < (int)D->P.num_paths; ++p) FactorPath(D, p, scaled);
  if (accumulate_in_place) {
    // x and y one buffer, y += M^-1 y: z = r + M^-1 r, then the r taken off again.
    *z = r;
    for (int p = 0; p < (int)D->P.num_paths; ++p) ApplyPath(D, p, z->data(), z->data(), true);
    for (size_t i = 0; i < z->size(); ++i) (*z)[i] -= r[i];
  } else {
    z->assign(r.size(), std::nan(""));
    for (int p = 0; p < (int)D->P.num_paths; ++p) ApplyPath(D, p, r.data(), z->data(), false);
  }
  return D->failed;
}

// S = B B^T / N + 2 I, B uniform in [-1, 1]: the part of S that M drops is
// small beside the 2 I, so M stays positive definite.
void Replay(const char* what, const std::string& tag, int C, const std::vector<int32_t>& label, int32_t G,
            const Edges& edges, const char* dir) {
  const int N = 9 * C;
  std::vector<double> B((size_t)(N * N)), S((size_t)(N * N)), r((size_t)N), z;
  for (double& v : B) v = 2.0 * Uniform() - 1.0;
  for (double& v : r) v = 2.0 * Uniform() - 1.0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0.0;
      for (int k = 0; k < N; ++k) s += B[(size_t)(i * N + k)] * B[(size_t)(j * N + k)];
      S[(size_t)(i * N + j)] = S[(size_t)(j * N + i)] = s / N + (i == j ? 2.0 : 0.0);
    }
  Cams cams(1);
  for (int c = 0; c < C; ++c) cams[0].push_back(c);  // one point seen by all: every block is in the plan
  Device D;
  EXPECT(Run(&D, C, cams, label, G, edges, S, r, &z, false) == 0 && D.status == 0);
  double worst = 0.0;
  for (int p = 0; p < (int)D.P.num_paths; ++p) {
    int n = 0;
    const double eta = PathEta(D, p, S, C, label, edges, 1.0, r, z, &n, dir, tag);
    const double bound = n * Gamma(3 * n + 1);
    worst = std::max(worst, eta / bound);
    EXPECT(eta <= bound);
  }
  std::printf("  replay %-34s %2lld paths, longest %2lld: worst eta / bound %.3e\n", what, (long long)D.P.num_paths,
              (long long)D.P.longest_path, worst);
}

// M = T (x) I_9 on three singleton clusters 0 - 1 - 2 (and a lone fourth
// cluster whose block is 2 I): returns whether the second pass ran.
void Retry(double a, bool expect_scaled, const char* dir) {
  const int C = 4, N = 36;
  std::vector<double> S((size_t)(N * N), 0.0), r((size_t)N), z;
  for (double& v : r) v = 2.0 * Uniform() - 1.0;
  for (int i = 0; i < N; ++i) S[(size_t)(i * N + i)] = i < 27 ? 1.0 : 2.0;
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < 9; ++i) S[(size_t)((9 * k + i) * N + 9 * (k + 1) + i)] = S[(size_t)((9 * (k + 1) + i) * N + 9 * k + i)] = a;
  const std::vector<int32_t> label = {0, 1, 2, 3};
  const Edges edges = {{1, 0}, {1, 2}};
  Cams cams(1);
  for (int c = 0; c < C; ++c) cams[0].push_back(c);
  for (int in_place = 0; in_place < 2; ++in_place) {
    Device D;
    const int scaled = Run(&D, C, cams, label, 4, edges, S, r, &z, in_place != 0);
    EXPECT(scaled == (expect_scaled ? 1 : 0) && D.status == 0);
    double worst = 0.0;
    for (int p = 0; p < (int)D.P.num_paths; ++p) {
      int n = 0;
      const double eta = PathEta(D, p, S, C, label, edges, scaled ? 0.5 : 1.0, r, z, &n, in_place ? nullptr : dir,
                                 "retry" + std::to_string((int)(10 * a)));
      EXPECT(eta <= n * Gamma(3 * n + 1));
      worst = std::max(worst, eta / (n * Gamma(3 * n + 1)));
    }
    std::printf("  retry a = %.1f%s: scaled %d, worst eta / bound %.3e\n", a, in_place ? " (x = y, accumulate)" : "",
                scaled, worst);
  }
}

void Refuse(const char* what, const Edges& edges, const std::vector<int32_t>& size, int want, const char* names) {
  const std::vector<int32_t> flat = Flat(edges);
  cse::SchurForestPaths paths;
  const int rc = cse::ValidateSchurForest(flat.data(), (int32_t)edges.size(), size.data(), (int32_t)size.size(), &paths);
  EXPECT(rc == want);
  const std::string msg = rc ? cse::LastError() : std::string();
  const bool named = !names || msg.find(names) != std::string::npos;
  EXPECT(named);
  std::printf("  refusal %-22s rc %d: %s\n", what, rc, rc ? msg.c_str() : "(accepted)");
}

}  // namespace

int main(int argc, char** argv) {
  std::printf("CLUSTER_TRIDIAGONAL forest, plan and replay driver\n");
  {
    const std::vector<int32_t> four = {4, 4, 4, 4}, big = {8, 9, 1, 15};
    Refuse("accepted path", {{0, 1}, {2, 1}, {2, 3}}, four, CSE_OK, nullptr);
    Refuse("no edges", {}, four, CSE_OK, nullptr);
    Refuse("label out of range", {{0, 4}}, four, CSE_ERR_INVALID, "edge 0 (0, 4)");
    Refuse("negative label", {{-1, 2}}, four, CSE_ERR_INVALID, "edge 0");
    Refuse("g = h", {{0, 1}, {2, 2}}, four, CSE_ERR_INVALID, "edge 1 (2, 2)");
    Refuse("duplicate", {{0, 1}, {2, 3}, {0, 1}}, four, CSE_ERR_INVALID, "twice");
    Refuse("duplicate, reversed", {{0, 1}, {1, 0}}, four, CSE_ERR_INVALID, "twice");
    Refuse("degree 3", {{0, 1}, {0, 2}, {0, 3}}, four, CSE_ERR_UNSUPPORTED, "cluster 0");
    Refuse("cycle", {{0, 1}, {1, 2}, {2, 0}}, four, CSE_ERR_UNSUPPORTED, "cycle");
    Refuse("17 cameras on an edge", {{0, 1}}, big, CSE_ERR_UNSUPPORTED, "edge 0 (0, 1)");
    Refuse("16 cameras on an edge", {{2, 3}}, big, CSE_OK, nullptr);
    cse::SchurForestPaths paths;
    const std::vector<int32_t> size = {1, 1};
    EXPECT(cse::ValidateSchurForest(nullptr, 1, size.data(), 2, &paths) == CSE_ERR_INVALID);
    EXPECT(cse::ValidateSchurForest(nullptr, 0, size.data(), 2, &paths) == CSE_OK && paths.path_begin.size() == 3);
    EXPECT(cse::ValidateSchurForest(nullptr, -1, size.data(), 2, &paths) == CSE_ERR_INVALID);
  }
  {
    // BAL-shaped, 16 cameras.
    Cams cams(120);
    for (int p = 0; p < 120; ++p)
      for (int k = 0; k < 2 + (p + 1) % 4; ++k) cams[p].push_back((p * 7 + k * 3) % 16);
    Edges chain;
    for (int g = 0; g + 1 < 16; ++g) chain.push_back(Key(g, g + 1));
    CheckPlan("singletons in one path", 16, cams, Labels(16, [](int c) { return (int32_t)c; }), 16, chain);
    CheckPlan("singletons, no edges", 16, cams, Labels(16, [](int c) { return (int32_t)c; }), 16, {});
    CheckPlan("two clusters of 8", 16, cams, Labels(16, [](int c) { return (int32_t)(c / 8); }), 2, {{0, 1}});
    CheckPlan("two clusters of 8, edge as (h, g)", 16, cams, Labels(16, [](int c) { return (int32_t)(c / 8); }), 2, {{1, 0}});
    CheckPlan("sizes (1, 15)", 16, cams, Labels(16, [](int c) { return (int32_t)(c ? 1 : 0); }), 2, {{0, 1}});
    CheckPlan("sizes (15, 1)", 16, cams, Labels(16, [](int c) { return (int32_t)(c == 15 ? 1 : 0); }), 2, {{0, 1}});
    CheckPlan("sizes (5, 3, 8)", 16, cams, Labels(16, [](int c) { return (int32_t)(c < 5 ? 0 : c < 8 ? 1 : 2); }), 3,
              {{0, 1}, {1, 2}});
    CheckPlan("path 2-0-1, edge given as (h, g)", 16, cams, Labels(16, [](int c) { return (int32_t)(c < 5 ? 0 : c < 8 ? 1 : 2); }),
              3, {{0, 2}, {1, 0}});
    CheckPlan("interleaved (even / odd)", 16, cams, Labels(16, [](int c) { return (int32_t)(c % 2); }), 2, {{0, 1}});
    CheckPlan("interleaved (even / odd), (h, g)", 16, cams, Labels(16, [](int c) { return (int32_t)(c % 2); }), 2, {{1, 0}});
    CheckPlan("several paths and lone clusters", 16, cams, Labels(16, [](int c) { return (int32_t)(c / 2); }), 8,
              {{6, 2}, {2, 4}, {0, 7}, {5, 6}});
  }
  EXPECT(g_direct > 0 && g_transposed > 0);
  std::printf("  rectangle tiles: %d hold S(g's, h's), %d its transpose\n", g_direct, g_transposed);
  {
    // camera 3 of 7 unobserved inside a cluster; clusters {5} and {6} share no point
    const Cams cams = {{0, 1, 2}, {2, 4, 5}, {4, 6, 0}, {1, 5}, {0, 2, 4, 6}, {0, 5}};
    CheckPlan("unobserved camera inside a cluster", 7, cams, {0, 1, 1, 0, 1, 2, 3}, 4, {{0, 1}, {1, 2}});
    CheckPlan("edge without a shared point", 7, cams, {0, 1, 1, 0, 1, 2, 3}, 4, {{2, 3}, {0, 1}});
  }
  {
    const Cams cams = {{0, 0, 1}, {2, 2, 2, 3}, {1, 4}, {3, 3, 0, 0, 0}, {4, 2}, {1, 0, 1}};
    CheckPlan("duplicates", 5, cams, {0, 0, 1, 1, 2}, 3, {{1, 0}, {2, 1}});
  }
  {
    Cams cams(150);
    for (int p = 0; p < 150; ++p) cams[p] = p % 3 ? std::vector<int>{0, 1, 2} : std::vector<int>{2, 0};
    CheckPlan("several chunks, {0,2} - {1}", 3, cams, {0, 1, 0}, 2, {{0, 1}});
    CheckPlan("several chunks, singletons 2-0-1", 3, cams, {0, 1, 2}, 3, {{0, 2}, {0, 1}});
  }
  CheckPlan("no residual blocks", 4, {}, {1, 0, 1, 0}, 2, {{0, 1}});

  const char* dir = argc > 1 ? argv[1] : nullptr;
  {
    Edges chain;
    for (int g = 0; g + 1 < 12; ++g) chain.push_back(Key(g, g + 1));
    Replay("12 singletons in one path", "chain", 12, Labels(12, [](int c) { return (int32_t)c; }), 12, chain, dir);
    Replay("two clusters of 8", "8x8", 16, Labels(16, [](int c) { return (int32_t)(c / 8); }), 2, {{0, 1}}, dir);
    Replay("(1, 15)", "1x15", 16, Labels(16, [](int c) { return (int32_t)(c ? 1 : 0); }), 2, {{0, 1}}, dir);
    Replay("(15, 1)", "15x1", 16, Labels(16, [](int c) { return (int32_t)(c == 15 ? 1 : 0); }), 2, {{0, 1}}, dir);
    Replay("(5, 3, 8) as 2-0-1, (h, g)", "538", 16, Labels(16, [](int c) { return (int32_t)(c < 5 ? 0 : c < 8 ? 1 : 2); }), 3,
           {{0, 2}, {1, 0}}, dir);
    Replay("interleaved (even / odd), (h, g)", "evenodd", 14, Labels(14, [](int c) { return (int32_t)(c % 2); }), 2, {{1, 0}}, dir);
    Replay("several paths and lone clusters", "several", 16, Labels(16, [](int c) { return (int32_t)(c / 2); }), 8,
           {{6, 2}, {2, 4}, {0, 7}, {5, 6}}, dir);
    Replay("a lone cluster of 16", "lone16", 16, Labels(16, [](int) { return (int32_t)0; }), 1, {}, dir);
  }
  Retry(0.8, true, dir);
  Retry(0.6, false, dir);
  {
    // A pivot that fails in both passes: the path's factor is zeroed, the
    // status is raised, the other path is intact.
    const int C = 3, N = 27;
    std::vector<double> S((size_t)(N * N), 0.0), r((size_t)N, 1.0), z;
    for (int i = 0; i < N; ++i) S[(size_t)(i * N + i)] = 1.0;
    S[(size_t)(13 * N + 13)] = -1.0;
    Cams cams(1);
    cams[0] = {0, 1, 2};
    Device D;
    EXPECT(Run(&D, C, cams, {0, 1, 2}, 3, {{0, 1}}, S, r, &z, false) == 1 && D.status == 1);
    for (int i = 0; i < 18; ++i) EXPECT(z[(size_t)i] == 0.0);
    for (int i = 18; i < 27; ++i) EXPECT(z[(size_t)i] == 1.0);
  }
  if (g_failures) {
    std::printf("%d FAILED\n", g_failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
