// schur_held_driver.cpp -- the implicit Schur complement's plan on problems with
// held (constant) cameras (cse::PlanProgram's SchurPlan and its held tables,
// csrc/plan.cpp), built by g++ with AddressSanitizer + UBSan from plan.cpp,
// layout.cpp and this file (tests/test_schur_held.py runs it; no HIP, no GPU).
//
// Per problem -- BAL-shaped; runs shorter and longer than a wave with held rows
// at chunk and stride boundaries; points seen by held cameras alone; one active
// camera only -- the plan is checked against brute force: eligibility, e_cols
// and f_cols, every wave chunk's first F-cell rank and active-lane mask, every
// big run's rank, the F cell of every entry of the slot-0 gradient plan's perm,
// every camera's active rank, and `duplicates` over the active cameras alone.
// The plan of a program without held cameras is compared field by field with
// the rule it has always followed (written out again here), and its held
// tables are empty.  Then the refusals: a held point, active cameras whose
// columns do not tile the f columns in id order, every camera held, and a
// caller that does not pass the group's tables.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
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

constexpr int kWave = 64;

// A Schur-ordered problem: P points (parameter blocks 0..P), C cameras after
// them, observations point-major.  Held cameras live in the constant state and
// the active ones' columns follow the points, 9 each, in id order.
struct Problem {
  int C = 0, P = 0;
  int64_t O = 0;
  std::set<int> held;
  std::vector<int32_t> ids, params, nres;
  std::vector<double> data, cstate;
  std::vector<cse_parameter_block> pbs;
  std::vector<int64_t> begin, res_layout, jac_layout, jac_offsets;
  int64_t num_values = 0;
  cse_residual_group g{};
  cse_problem_desc d{};
};

enum Twist { kNone, kHeldPoint, kSwappedColumns };

void Build(Problem* Q, int C, const std::vector<std::vector<int>>& cams, const std::set<int>& held,
           Twist twist = kNone) {
  Problem& q = *Q;
  q.C = C;
  q.P = (int)cams.size();
  q.held = held;
  const int P = q.P;
  int64_t nconst = 0;
  for (int p = 0; p < P; ++p) {
    if (twist == kHeldPoint && p == 1) {
      q.pbs.push_back({3, 3, 1, 0, nconst, 0, -1});
      nconst += 3;
    } else {
      const int64_t at = 3LL * (p - (twist == kHeldPoint && p > 1 ? 1 : 0));
      q.pbs.push_back({3, 3, 0, 0, at, at, -1});
    }
  }
  const int64_t e_cols = 3LL * (P - (twist == kHeldPoint ? 1 : 0));
  int64_t rank = 0;
  for (int c = 0; c < C; ++c) {
    if (held.count(c)) {
      q.pbs.push_back({9, 9, 1, 0, nconst, 0, -1});
      nconst += 9;
    } else {
      const int64_t at = e_cols + 9 * rank++;
      q.pbs.push_back({9, 9, 0, 0, at, at, -1});
    }
  }
  if (twist == kSwappedColumns) {
    // The first two active cameras trade their columns: a valid program whose
    // cameras no longer tile the f columns in id order.
    int a = -1, b = -1;
    for (int c = 0; c < C && b < 0; ++c)
      if (!held.count(c)) (a < 0 ? a : b) = c;
    std::swap(q.pbs[(size_t)(P + a)].delta_offset, q.pbs[(size_t)(P + b)].delta_offset);
    std::swap(q.pbs[(size_t)(P + a)].state_offset, q.pbs[(size_t)(P + b)].state_offset);
  }
  q.cstate.assign((size_t)nconst, 0.25);
  q.begin.push_back(0);
  for (int p = 0; p < P; ++p)
    for (int c : cams[(size_t)p]) {
      q.ids.push_back(P + c);
      q.ids.push_back(p);
      q.params.push_back(P + c);
      q.params.push_back(p);
      q.begin.push_back((int64_t)q.params.size());
      q.nres.push_back(2);
      q.data.push_back(1.0);
      q.data.push_back(-2.0);
    }
  q.O = (int64_t)q.nres.size();
  const int64_t npb = (int64_t)q.pbs.size();
  const int64_t count = cse_layout_offsets_count(npb, q.pbs.data(), q.O, q.begin.data(), q.params.data(),
                                                 q.nres.data());
  q.res_layout.resize((size_t)q.O);
  q.jac_layout.resize((size_t)q.O);
  q.jac_offsets.resize((size_t)(count > 0 ? count : 1));
  EXPECT(cse_block_sparse_layout(npb, q.pbs.data(), q.O, q.begin.data(), q.params.data(), q.nres.data(), P,
                                 q.res_layout.data(), q.jac_layout.data(), q.jac_offsets.data(),
                                 &q.num_values) == CSE_OK);
  q.g.functor_kind = CSE_FUNCTOR_SNAVELY_2_9_3;
  q.g.loss = cse_loss{CSE_LOSS_HUBER, 1, 1.0, 2.0, {}};
  q.g.num_blocks = q.O;
  q.g.parameter_block_ids = q.ids.data();
  q.g.functor_data = q.data.data();
  cse_problem_desc& d = q.d;
  d.abi_version = CSE_ABI_VERSION;
  d.num_groups = 1;
  d.groups = &q.g;
  d.num_parameter_blocks = npb;
  d.parameter_blocks = q.pbs.data();
  for (const cse_parameter_block& pb : q.pbs) {
    (pb.is_constant ? d.num_constant_parameters : d.num_parameters) += pb.size;
    if (!pb.is_constant) d.num_effective_parameters += pb.tangent_size;
  }
  d.constant_state = q.cstate.empty() ? nullptr : q.cstate.data();
  d.num_residual_blocks = q.O;
  d.num_residuals = 2 * q.O;
  d.residual_layout = q.res_layout.data();
  d.jacobian_per_residual_layout = q.jac_layout.data();
  d.jacobian_per_residual_offsets = q.jac_offsets.data();
  d.num_jacobian_per_residual_offsets = count;
  d.num_jacobian_values = q.num_values;
}

struct Planned {
  cse::ProgramPlan P;
  cse::GroupPlan G;
  cse::GroupTables T;
};

int Plan(const cse_problem_desc& d, Planned* out, bool pass_tables = true) {
  cse_options o{};
  o.device = -1;
  o.check_finite = 1;
  o.apply_loss_function = 1;
  int rc = cse::Validate(&d);
  if (rc) return rc;
  if ((rc = cse::ValidateGroups(&d, nullptr, &out->P, &o))) return rc;
  cse::PlanGroup(&d, o, 0, &out->P, &out->G, &out->T);
  cse::PlanProgram(&d, &out->G, &out->P, pass_tables ? &out->T : nullptr);
  return CSE_OK;
}

// The chunk rule, written out again: runs of equal point are packed into
// chunks of at most a wave of whole runs; a longer run is big, and no chunk
// straddles it.
void ChunkRule(const Problem& q, std::vector<int64_t>* ranges, std::vector<int64_t>* big) {
  const int64_t n = q.O;
  int64_t lo = 0, i = 0;
  while (i < n) {
    int64_t j = i;
    while (j < n && q.ids[(size_t)(2 * j + 1)] == q.ids[(size_t)(2 * i + 1)]) ++j;
    if (j - i > kWave) {
      if (i > lo) {
        ranges->push_back(lo);
        ranges->push_back(i);
      }
      big->push_back(i);
      big->push_back(j);
      lo = j;
    } else if (j - lo > kWave) {
      ranges->push_back(lo);
      ranges->push_back(i);
      lo = i;
    }
    i = j;
  }
  if (n > lo) {
    ranges->push_back(lo);
    ranges->push_back(n);
  }
}

struct Facts {
  int held_chunks = 0, lane0_held = 0, last_held = 0, straddle = 0;
};

void Check(const char* what, int C, const std::vector<std::vector<int>>& cams, const std::set<int>& held,
           Facts* facts = nullptr) {
  Problem q;
  Build(&q, C, cams, held);
  Planned pl;
  EXPECT(Plan(q.d, &pl) == CSE_OK);
  const cse::SchurPlan& S = pl.P.schur;
  const int P = q.P;
  const int64_t n = q.O;
  auto active = [&](int64_t i) { return !held.count(q.ids[(size_t)(2 * i)] - P); };
  EXPECT(pl.G.policy == cse::kAffinePacked && pl.G.fuse_ok);
  EXPECT(pl.G.const0 == !held.empty());
  EXPECT(S.eligible);
  if (!S.eligible) return;
  const int64_t nactive = C - (int64_t)held.size();
  EXPECT(S.e_cols == 3LL * P && S.f_cols == 9 * nactive);
  EXPECT(S.e_cols + S.f_cols == q.d.num_effective_parameters);
  std::vector<int64_t> ranges, big;
  ChunkRule(q, &ranges, &big);
  EXPECT(pl.P.schur_chunk_begin == ranges && pl.P.schur_big == big);
  EXPECT(S.nchunks == (int64_t)ranges.size() / 2 && S.nbig == (int64_t)big.size() / 2);
  // duplicates: some point sees one ACTIVE camera twice
  bool dup = false;
  for (const auto& cs : cams) {
    std::multiset<int> seen;
    for (int c : cs)
      if (!held.count(c)) seen.insert(c);
    for (int c : seen) dup = dup || seen.count(c) > 1;
  }
  EXPECT(S.duplicates == dup);
  if (held.empty()) {
    // Field by field what the plan has always been.
    EXPECT(!S.held && S.num_active == 0);
    EXPECT(S.f_col_base == -9LL * P);
    EXPECT(pl.P.schur_chunk_held.empty() && pl.P.schur_big_rank.empty() && pl.P.schur_fcell.empty() &&
           pl.P.schur_cam_rank.empty());
    // and it does not depend on the tables being passed
    Planned bare;
    EXPECT(Plan(q.d, &bare, false) == CSE_OK);
    const cse::SchurPlan& B = bare.P.schur;
    EXPECT(B.eligible == S.eligible && B.duplicates == S.duplicates && B.e_cols == S.e_cols &&
           B.f_cols == S.f_cols && B.f_col_base == S.f_col_base && B.nchunks == S.nchunks &&
           B.nbig == S.nbig && B.held == S.held && B.num_active == S.num_active);
    EXPECT(bare.P.schur_chunk_begin == pl.P.schur_chunk_begin && bare.P.schur_big == pl.P.schur_big);
    std::printf("  %-28s %3d cameras, none held: %lld chunks %lld big\n", what, C, (long long)S.nchunks,
                (long long)S.nbig);
    return;
  }
  EXPECT(S.held && S.num_active == nactive);
  // Brute force: the F cell of block i = the blocks with an active camera before it.
  std::vector<int64_t> cell((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) cell[(size_t)i + 1] = cell[(size_t)i] + (active(i) ? 1 : 0);
  EXPECT((int64_t)pl.P.schur_chunk_held.size() == 2 * S.nchunks);
  EXPECT((int64_t)pl.P.schur_big_rank.size() == S.nbig);
  if (g_failures) return;
  Facts f;
  for (int64_t c = 0; c < S.nchunks; ++c) {
    const int64_t i0 = ranges[(size_t)(2 * c)], i1 = ranges[(size_t)(2 * c + 1)];
    EXPECT(i1 - i0 >= 1 && i1 - i0 <= kWave);
    uint64_t mask = 0;
    for (int64_t i = i0; i < i1; ++i)
      if (active(i)) mask |= (uint64_t)1 << (i - i0);
    EXPECT(pl.P.schur_chunk_held[(size_t)(2 * c)] == cell[(size_t)i0]);
    EXPECT((uint64_t)pl.P.schur_chunk_held[(size_t)(2 * c + 1)] == mask);
    // the chunk's F segment is contiguous: its active blocks' cells are rank0, rank0 + 1, ..
    EXPECT(cell[(size_t)i1] - cell[(size_t)i0] == (int64_t)__builtin_popcountll(mask));
    if (mask == 0) ++f.held_chunks;
    if (mask != 0 && !(mask & 1)) ++f.lane0_held;
    if (mask != 0 && !((mask >> (i1 - i0 - 1)) & 1)) ++f.last_held;
  }
  for (int64_t r = 0; r < S.nbig; ++r) {
    const int64_t i0 = big[(size_t)(2 * r)], i1 = big[(size_t)(2 * r + 1)];
    EXPECT(i1 - i0 > kWave);
    EXPECT(pl.P.schur_big_rank[(size_t)r] == cell[(size_t)i0]);
    for (int64_t i = i0 + kWave; i < i1; i += kWave)
      if (!active(i - 1) && !active(i)) ++f.straddle;
  }
  // The camera pass: perm lists exactly the blocks with an active camera,
  // and fcell their cells.
  const cse::GradPlanInfo& I = pl.T.grad_info[0];
  EXPECT(I.ready && !I.sorted && I.lo == P && I.count == C && I.nperm == cell[(size_t)n]);
  EXPECT((int64_t)pl.P.schur_fcell.size() == std::max<int64_t>(I.nperm, 1));
  std::vector<int> seen((size_t)n, 0);
  for (int64_t k = 0; k < I.nperm; ++k) {
    const int32_t i = pl.T.grad[0].perm[(size_t)k];
    EXPECT(i >= 0 && i < n && active(i));
    if (i < 0 || i >= n) return;
    ++seen[(size_t)i];
    EXPECT(pl.P.schur_fcell[(size_t)k] == cell[(size_t)i]);
  }
  for (int64_t i = 0; i < n; ++i) EXPECT(seen[(size_t)i] == (active(i) ? 1 : 0));
  // Camera ranks, and the columns they stand for.
  EXPECT((int64_t)pl.P.schur_cam_rank.size() == C);
  int32_t rank = 0;
  for (int c = 0; c < C && (int64_t)pl.P.schur_cam_rank.size() == C; ++c) {
    const int32_t got = pl.P.schur_cam_rank[(size_t)c];
    if (held.count(c)) {
      EXPECT(got == -1);
    } else {
      EXPECT(got == rank);
      EXPECT(q.pbs[(size_t)(P + c)].delta_offset == S.e_cols + 9LL * rank);
      EXPECT(pl.T.dlt[(size_t)c] == S.e_cols + 9LL * rank);  // the multiply's f rows (delta0)
      ++rank;
    }
  }
  std::printf("  %-28s %3d cameras %2d held: %lld of %lld blocks held, %lld chunks (%d all held, %d lane 0, "
              "%d last lane) %lld big (%d held strides)\n",
              what, C, (int)held.size(), (long long)(n - cell[(size_t)n]), (long long)n,
              (long long)S.nchunks, f.held_chunks, f.lane0_held, f.last_held, (long long)S.nbig, f.straddle);
  if (facts) *facts = f;
}

void ExpectRefused(const char* what, const Problem& q, bool pass_tables = true) {
  Planned pl;
  EXPECT(Plan(q.d, &pl, pass_tables) == CSE_OK);
  EXPECT(!pl.P.schur.eligible && !pl.P.schur.held);
  EXPECT(pl.P.schur_chunk_held.empty() && pl.P.schur_fcell.empty() && pl.P.schur_cam_rank.empty());
  std::printf("  %-28s refused (policy %d, const0 %d)\n", what, pl.G.policy, (int)pl.G.const0);
}

std::vector<std::vector<int>> BalShaped(int P, int C) {
  std::vector<std::vector<int>> cams((size_t)P);
  for (int p = 0; p < P; ++p)
    for (int k = 0; k < 1 + (p + 1) % 5; ++k) cams[(size_t)p].push_back((p * 7 + k * 3) % C);
  return cams;
}

}  // namespace

int main() {
  std::printf("Implicit Schur complement plan with held cameras\n");
  const auto bal = BalShaped(60, 11);
  Check("BAL-shaped", 11, bal, {});
  Check("BAL-shaped", 11, bal, {0});
  Check("BAL-shaped", 11, bal, {10});
  Check("BAL-shaped", 11, bal, {0, 3, 7, 10});
  Check("one active camera", 11, bal, {0, 1, 2, 3, 4, 5, 6, 7, 8, 10});
  {
    // Runs around a wave: each point sees cameras p 7 + 3 k (mod 140), distinct.
    const int counts[] = {1, 2, 70, 3, 130, 64, 65, 5, 4, 6, 63, 1, 66, 2, 7, 8, 3, 1, 200, 5, 2, 9};
    std::vector<std::vector<int>> cams;
    for (int n : counts) {
      const int p = (int)cams.size();
      cams.emplace_back();
      for (int k = 0; k < n; ++k) cams.back().push_back((p * 7 + k * 3) % 140);
    }
    Check("runs", 140, cams, {});
    // Held: point 0's only camera; both of point 1's; the first and last row of
    // the 70-run; rows 63 and 64 of the 130-run (both sides of its stride).
    std::set<int> held = {cams[0][0], cams[1][0], cams[1][1], cams[2][0], cams[2][69], cams[4][63], cams[4][64]};
    Facts f;
    Check("runs, boundaries held", 140, cams, held, &f);
    EXPECT(f.held_chunks >= 1 && f.straddle >= 1);
    std::set<int> most;
    for (int c = 0; c < 140; ++c)
      if (c % 9 != 4) most.insert(c);
    Check("runs, 8 of 9 held", 140, cams, most);
  }
  // duplicates count over active cameras only
  Check("duplicate of a held camera", 5, {{0, 0, 1}, {2, 3}, {1, 4}, {0, 0, 0, 3}, {4, 2}}, {0});
  Check("duplicate of an active one", 5, {{0, 0, 1}, {2, 3}, {1, 4}, {0, 3, 3}, {4, 2}}, {0});

  {
    // A constant camera that no residual block uses is not a held slot-0
    // block of the group: refused, as before.
    Problem q;
    Build(&q, 6, {{0, 1}, {1, 2}, {2, 4}, {4, 5, 0}}, {3});
    ExpectRefused("held camera never observed", q);
  }
  {
    Problem q;
    Build(&q, 11, bal, {2}, kHeldPoint);
    ExpectRefused("a held point", q);
  }
  {
    Problem q;
    Build(&q, 11, bal, {}, kHeldPoint);
    ExpectRefused("a held point, no camera", q);
  }
  {
    Problem q;
    Build(&q, 11, bal, {2}, kSwappedColumns);
    ExpectRefused("columns not in id order", q);
  }
  {
    Problem q;
    std::set<int> all;
    for (int c = 0; c < 11; ++c) all.insert(c);
    Build(&q, 11, bal, all);
    ExpectRefused("every camera held", q);
  }
  {
    Problem q;
    Build(&q, 11, bal, {2});
    ExpectRefused("tables not passed", q, false);
  }
  if (g_failures) {
    std::printf("%d FAILED\n", g_failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
