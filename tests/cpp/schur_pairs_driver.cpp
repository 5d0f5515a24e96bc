// schur_pairs_driver.cpp -- the host-only pair plan of the explicit Schur
// complement (cse::PlanSchurPairs, csrc/plan.cpp), built by g++ with
// AddressSanitizer + UBSan from plan.cpp, layout.cpp and this file
// (tests/test_schur_complement.py runs it; no HIP, no GPU).
//
// Small Schur-ordered problems -- BAL-shaped; a point seen once and points
// with 64, 65 and 130 observations; points that see one camera two and three
// times; a camera nobody observes -- go through Validate, ValidateGroups,
// PlanGroup and PlanProgram (the Schur structure must be eligible) and then
// PlanSchurPairs.  The plan is checked against brute force, and replayed on
// the host in the kernels' order (chunk partials, then the per-block finish)
// with random F, E and M_p against the dense formula
//     S(c,c') = delta (D_c^2 + sum F_b^T F_b) - sum_p G_pc M_p G_pc'^T,
//     G_pc = sum over the blocks b of p and c of F_b^T E_b.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../ceres-solver-cuda_amd/csrc/plan.hpp"
#include "../../include/cse.h"

namespace cse {
std::string& LastError();  // layout.cpp
}  // namespace cse

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

// A Schur-ordered problem: P points (program blocks 0..P), C cameras after
// them; cams[p] lists the cameras (0..C) of point p's observations.
struct Problem {
  int C = 0, P = 0;
  int64_t O = 0;
  std::vector<int32_t> ids;
  std::vector<double> data;
  std::vector<cse_parameter_block> pbs;
  std::vector<int64_t> begin, res_layout, jac_layout, jac_offsets;
  std::vector<int32_t> params, nres;
  int64_t num_values = 0;
  cse_residual_group g{};
  cse_problem_desc d{};
};

void Build(Problem* Q, int C, const std::vector<std::vector<int>>& cams) {
  Problem& q = *Q;
  q.C = C;
  const int P = q.P = (int)cams.size();
  for (int p = 0; p < P; ++p) q.pbs.push_back({3, 3, 0, 0, 3LL * p, 3LL * p, -1});
  for (int c = 0; c < C; ++c) q.pbs.push_back({9, 9, 0, 0, 3LL * P + 9LL * c, 3LL * P + 9LL * c, -1});
  q.begin.push_back(0);
  for (int p = 0; p < P; ++p) {
    for (int c : cams[p]) {
      q.ids.push_back(P + c);
      q.ids.push_back(p);
      q.params.push_back(P + c);
      q.params.push_back(p);
      q.begin.push_back((int64_t)q.params.size());
      q.nres.push_back(2);
      for (int k = 0; k < 2; ++k) q.data.push_back(200.0 * (Uniform() - 0.5));
    }
  }
  q.O = (int64_t)q.nres.size();
  const int64_t npb = (int64_t)q.pbs.size();
  const int64_t count = cse_layout_offsets_count(npb, q.pbs.data(), q.O, q.begin.data(), q.params.data(),
                                                 q.nres.data());
  q.res_layout.resize(q.O);
  q.jac_layout.resize(q.O);
  q.jac_offsets.resize(count > 0 ? count : 1);
  EXPECT(cse_block_sparse_layout(npb, q.pbs.data(), q.O, q.begin.data(), q.params.data(), q.nres.data(), P,
                                 q.res_layout.data(), q.jac_layout.data(), q.jac_offsets.data(),
                                 &q.num_values) == CSE_OK);
  q.g.functor_kind = CSE_FUNCTOR_SNAVELY_2_9_3;
  q.g.loss = cse_loss{CSE_LOSS_HUBER, 0, 1.0, 1.0, {}};
  q.g.num_blocks = q.O;
  q.g.parameter_block_ids = q.ids.data();
  q.g.functor_data = q.data.data();
  cse_problem_desc& d = q.d;
  d.abi_version = CSE_ABI_VERSION;
  d.num_groups = 1;
  d.groups = &q.g;
  d.num_parameter_blocks = npb;
  d.parameter_blocks = q.pbs.data();
  d.num_parameters = d.num_effective_parameters = 3LL * P + 9LL * C;
  d.num_residual_blocks = q.O;
  d.num_residuals = 2 * q.O;
  d.residual_layout = q.res_layout.data();
  d.jacobian_per_residual_layout = q.jac_layout.data();
  d.jacobian_per_residual_offsets = q.jac_offsets.data();
  d.num_jacobian_per_residual_offsets = count;
  d.num_jacobian_values = q.num_values;
}

typedef std::pair<int32_t, int32_t> Key;

// 3 x 3 symmetric inverse by cofactors (full storage).
void Invert3(const double* A, double* M) {
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8],
               c02 = A[3] * A[7] - A[4] * A[6];
  const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
  M[0] = c00 / det;
  M[1] = M[3] = c01 / det;
  M[2] = M[6] = c02 / det;
  M[4] = (A[0] * A[8] - A[2] * A[6]) / det;
  M[5] = M[7] = (A[2] * A[3] - A[0] * A[5]) / det;
  M[8] = (A[0] * A[4] - A[1] * A[3]) / det;
}

void Check(const char* what, int C, const std::vector<std::vector<int>>& cams, bool want_dup) {
  Problem q;
  Build(&q, C, cams);
  cse_options o{};
  o.device = -1;
  o.check_finite = 1;
  o.apply_loss_function = 1;
  cse::ProgramPlan PP;
  cse::GroupPlan G;
  cse::GroupTables T;
  EXPECT(cse::Validate(&q.d) == CSE_OK);
  EXPECT(cse::ValidateGroups(&q.d, nullptr, &PP, &o) == CSE_OK);
  cse::PlanGroup(&q.d, o, 0, &PP, &G, &T);
  cse::PlanProgram(&q.d, &G, &PP);
  EXPECT(PP.schur.eligible);
  EXPECT(PP.schur.duplicates == want_dup);
  EXPECT(PP.schur.f_cols == 9LL * C && PP.schur.e_cols == 3LL * q.P);

  const int64_t n = q.O;
  const int32_t* ids = q.ids.data();
  cse::SchurPairPlan S, counts;
  EXPECT(cse::PlanSchurPairs(ids, n, false, &S) == CSE_OK);
  EXPECT(cse::PlanSchurPairs(ids, n, true, &counts) == CSE_OK);
  EXPECT(counts.num_blocks == S.num_blocks && counts.num_pairs == S.num_pairs &&
         counts.num_chunks == S.num_chunks && counts.plan_bytes == S.plan_bytes);
  EXPECT(counts.pairs.empty() && counts.block_row.empty());

  // Brute force: every same-point pair (b, b') with cam(b) <= cam(b').
  std::map<Key, std::vector<Key>> want;
  for (int64_t b = 0; b < n; ++b)
    for (int64_t b2 = 0; b2 < n; ++b2)
      if (ids[2 * b + 1] == ids[2 * b2 + 1] && ids[2 * b] <= ids[2 * b2])
        want[Key(ids[2 * b], ids[2 * b2])].push_back(Key((int32_t)b, (int32_t)b2));
  int64_t want_pairs = 0, want_chunks = 0;
  for (auto& kv : want) {
    // blocks are sorted by point, so (point, b, b') order is (b, b') order
    std::sort(kv.second.begin(), kv.second.end());
    want_pairs += (int64_t)kv.second.size();
    want_chunks += ((int64_t)kv.second.size() + cse::kSchurPairChunk - 1) / cse::kSchurPairChunk;
  }
  // Closed forms: per point with k observations, m_c of them of camera c,
  // (k^2 + sum_c m_c^2) / 2 pairs.
  int64_t closed = 0;
  for (const auto& cs : cams) {
    std::map<int, int64_t> mult;
    for (int c : cs) ++mult[c];
    int64_t k = (int64_t)cs.size(), sq = 0;
    for (const auto& kv : mult) sq += kv.second * kv.second;
    closed += (k * k + sq) / 2;
  }
  EXPECT(S.num_pairs == want_pairs && S.num_pairs == closed);
  EXPECT(S.num_blocks == (int64_t)want.size());
  EXPECT(S.num_chunks == want_chunks);
  EXPECT((int64_t)S.block_row.size() == S.num_blocks && (int64_t)S.block_col.size() == S.num_blocks);
  EXPECT((int64_t)S.pair_begin.size() == S.num_blocks + 1 && (int64_t)S.chunk_off.size() == S.num_blocks + 1);
  EXPECT((int64_t)S.chunk_block.size() == S.num_chunks && (int64_t)S.pairs.size() == 2 * S.num_pairs);
  EXPECT(S.pair_begin[0] == 0 && S.pair_begin.back() == S.num_pairs);
  EXPECT(S.chunk_off[0] == 0 && S.chunk_off.back() == S.num_chunks);
  EXPECT(S.plan_bytes == 8 * S.num_blocks + 16 * (S.num_blocks + 1) + 4 * S.num_chunks + 8 * S.num_pairs +
                             648 * S.num_chunks);
  // Blocks sorted and unique, each block's pairs exactly the brute-force
  // list in its order (so every pair appears once, under the right block).
  auto it = want.begin();
  for (int64_t k = 0; k < S.num_blocks && it != want.end(); ++k, ++it) {
    EXPECT(S.block_row[k] <= S.block_col[k]);
    EXPECT(Key(S.block_row[k], S.block_col[k]) == it->first);  // std::map order = lexicographic
    if (k > 0) EXPECT(Key(S.block_row[k - 1], S.block_col[k - 1]) < Key(S.block_row[k], S.block_col[k]));
    const int64_t p0 = S.pair_begin[k], p1 = S.pair_begin[k + 1];
    EXPECT(p1 - p0 == (int64_t)it->second.size());
    if (p1 - p0 != (int64_t)it->second.size()) continue;
    bool same = true;
    for (int64_t p = p0; p < p1; ++p)
      same = same && Key(S.pairs[2 * p], S.pairs[2 * p + 1]) == it->second[(size_t)(p - p0)];
    EXPECT(same);
    // The chunks tile the block's pairs.
    const int64_t nch = S.chunk_off[k + 1] - S.chunk_off[k];
    EXPECT(nch == (p1 - p0 + cse::kSchurPairChunk - 1) / cse::kSchurPairChunk);
    for (int64_t c = S.chunk_off[k]; c < S.chunk_off[k + 1]; ++c) EXPECT(S.chunk_block[c] == k);
  }

  // ---- Replay on the host against the dense formula.
  std::vector<double> F(18 * n), E(6 * n), M(9 * (size_t)q.P), D(9 * (size_t)C);
  for (double& v : F) v = 2.0 * Uniform() - 1.0;
  for (double& v : E) v = 2.0 * Uniform() - 1.0;
  for (double& v : D) v = 0.1 + 1.9 * Uniform();
  for (int p = 0; p < q.P; ++p) {  // M_p = (sum E_b^T E_b + d^2 I)^-1: SPD
    double A[9] = {0};
    for (int64_t b = 0; b < n; ++b)
      if (ids[2 * b + 1] == p)
        for (int r = 0; r < 2; ++r)
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) A[3 * i + j] += E[6 * b + 3 * r + i] * E[6 * b + 3 * r + j];
    const double d = 0.5 + Uniform();
    for (int i = 0; i < 3; ++i) A[4 * i] += d * d;
    Invert3(A, &M[9 * (size_t)p]);
  }
  const int64_t N = 9LL * C;
  auto cam = [&](int64_t b) { return (int64_t)ids[2 * b] - q.P; };
  // the plan's way
  std::vector<double> part(81 * (size_t)S.num_chunks, 0.0), got((size_t)(N * N), 0.0);
  for (int64_t c = 0; c < S.num_chunks; ++c) {
    const int64_t k = S.chunk_block[c];
    const int64_t p0 = S.pair_begin[k] + (c - S.chunk_off[k]) * cse::kSchurPairChunk;
    const int64_t p1 = std::min(p0 + cse::kSchurPairChunk, S.pair_begin[k + 1]);
    EXPECT(p0 < p1);
    for (int64_t p = p0; p < p1; ++p) {
      const int64_t b = S.pairs[2 * p], b2 = S.pairs[2 * p + 1];
      const double* Mp = &M[9 * (size_t)ids[2 * b + 1]];
      double Qm[2][2];
      for (int r = 0; r < 2; ++r)
        for (int s = 0; s < 2; ++s) {
          double v = b == b2 && r == s ? 1.0 : 0.0;
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) v -= E[6 * b + 3 * r + i] * Mp[3 * i + j] * E[6 * b2 + 3 * s + j];
          Qm[r][s] = v;
        }
      for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j)
          for (int r = 0; r < 2; ++r)
            part[81 * (size_t)c + 9 * i + j] +=
                F[18 * b + 9 * r + i] * (Qm[r][0] * F[18 * b2 + j] + Qm[r][1] * F[18 * b2 + 9 + j]);
    }
  }
  for (int64_t k = 0; k < C * 9; ++k) got[(size_t)(k * N + k)] = D[(size_t)k] * D[(size_t)k];
  for (int64_t k = 0; k < S.num_blocks; ++k) {
    const int64_t c = S.block_row[k] - q.P, c2 = S.block_col[k] - q.P;
    for (int i = 0; i < 9; ++i)
      for (int j = 0; j < 9; ++j) {
        if (c == c2 && i > j) continue;
        double v = 0.0;
        for (int64_t ch = S.chunk_off[k]; ch < S.chunk_off[k + 1]; ++ch) v += part[81 * (size_t)ch + 9 * i + j];
        if (c == c2 && i == j) v += D[(size_t)(9 * c + i)] * D[(size_t)(9 * c + i)];
        got[(size_t)((9 * c + i) * N + 9 * c2 + j)] = v;
        got[(size_t)((9 * c2 + j) * N + 9 * c + i)] = v;
      }
  }
  // the dense formula
  std::vector<double> ref((size_t)(N * N), 0.0);
  for (int64_t k = 0; k < N; ++k) ref[(size_t)(k * N + k)] = D[(size_t)k] * D[(size_t)k];
  for (int64_t b = 0; b < n; ++b)
    for (int i = 0; i < 9; ++i)
      for (int j = 0; j < 9; ++j)
        ref[(size_t)((9 * cam(b) + i) * N + 9 * cam(b) + j)] +=
            F[18 * b + i] * F[18 * b + j] + F[18 * b + 9 + i] * F[18 * b + 9 + j];
  for (int p = 0; p < q.P; ++p) {
    std::map<int64_t, std::vector<double>> Gp;  // camera -> 9 x 3
    for (int64_t b = 0; b < n; ++b) {
      if (ids[2 * b + 1] != p) continue;
      std::vector<double>& g = Gp[cam(b)];
      g.resize(27, 0.0);
      for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 3; ++j)
          g[3 * i + j] += F[18 * b + i] * E[6 * b + j] + F[18 * b + 9 + i] * E[6 * b + 3 + j];
    }
    const double* Mp = &M[9 * (size_t)p];
    for (const auto& a : Gp)
      for (const auto& bb : Gp)
        for (int i = 0; i < 9; ++i)
          for (int j = 0; j < 9; ++j) {
            double v = 0.0;
            for (int s = 0; s < 3; ++s)
              for (int t = 0; t < 3; ++t) v += a.second[3 * i + s] * Mp[3 * s + t] * bb.second[3 * j + t];
            ref[(size_t)((9 * a.first + i) * N + 9 * bb.first + j)] -= v;
          }
  }
  double worst = 0.0;
  bool symmetric = true;
  for (int64_t c = 0; c < C; ++c)
    for (int64_t c2 = 0; c2 < C; ++c2) {
      double dn = 0.0, rn = 0.0;
      for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) {
          const size_t at = (size_t)((9 * c + i) * N + 9 * c2 + j);
          dn += (got[at] - ref[at]) * (got[at] - ref[at]);
          rn += ref[at] * ref[at];
          symmetric = symmetric && got[at] == got[(size_t)((9 * c2 + j) * N + 9 * c + i)];
        }
      if (rn == 0.0) {
        EXPECT(dn == 0.0);  // no shared point: exactly zero both ways
        continue;
      }
      worst = std::max(worst, std::sqrt(dn / rn));
    }
  EXPECT(symmetric);
  EXPECT(worst <= 1e-13);
  std::printf("  %-22s %4lld blocks (%d cameras) %6lld pairs %5lld chunks, replay worst block %.2e\n", what,
              (long long)S.num_blocks, C, (long long)S.num_pairs, (long long)S.num_chunks, worst);
}

}  // namespace

int main() {
  std::printf("Schur complement pair plan driver\n");
  {
    std::vector<std::vector<int>> cams(60);
    for (int p = 0; p < 60; ++p)
      for (int k = 0; k < 1 + (p + 1) % 5; ++k) cams[p].push_back((p * 7 + k * 3) % 11);
    Check("BAL-shaped", 11, cams, false);
  }
  {
    const int C = 140;
    std::vector<std::vector<int>> cams;
    int p = 0;
    for (int k : {1, 64, 65, 130, 3, 2, 5}) {
      cams.emplace_back();
      for (int j = 0; j < k; ++j) cams.back().push_back((p * 11 + j) % C);
      ++p;
    }
    Check("runs 1, 64, 65, 130", C, cams, false);
  }
  {  // blocks of several chunks: 3 cameras, 150 points that all see two or three of them
    std::vector<std::vector<int>> cams(150);
    for (int p = 0; p < 150; ++p) cams[p] = p % 3 ? std::vector<int>{0, 1, 2} : std::vector<int>{2, 0};
    Check("several chunks a block", 3, cams, false);
  }
  Check("duplicates", 5, {{0, 0, 1}, {2, 2, 2, 3}, {1, 4}, {3, 3, 0, 0, 0}, {4, 2}, {1, 0, 1}}, true);
  Check("unobserved camera", 6, {{0, 1, 2}, {2, 4}, {4, 5, 0}, {1, 5}, {0, 2, 4, 5}}, false);
  {  // an empty group and the 2^31 refusal
    cse::SchurPairPlan S;
    EXPECT(cse::PlanSchurPairs(nullptr, 0, false, &S) == CSE_OK);
    EXPECT(S.num_blocks == 0 && S.num_pairs == 0 && S.pair_begin.size() == 1);
    EXPECT(cse::PlanSchurPairs(nullptr, (int64_t)1 << 31, true, &S) == CSE_ERR_UNSUPPORTED);
  }
  if (g_failures) {
    std::printf("%d FAILED\n", g_failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
