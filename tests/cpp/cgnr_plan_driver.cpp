// cgnr_plan_driver.cpp -- cse_cgnr_init's block table (cse::PlanCgnrBlocks,
// csrc/plan.cpp) against brute force, built by g++ with AddressSanitizer +
// UBSan from plan.cpp, layout.cpp and this file (tests/test_cgnr_solve.py runs
// it; no HIP, no GPU).
//
// The planner reads the descriptor's parameter blocks and
// num_effective_parameters alone, so the descriptors here carry nothing else:
// mixed block sizes, constant blocks in the middle, blocks out of delta order,
// a gap, an overlap, an oversize block, a zero-size block and an empty program.
// Per descriptor: the entries are the non-constant blocks with columns, sorted
// by delta_offset; value_offset is the running sum of tangent_size^2; num_values,
// max_size, `tiles` (a brute-force cover count of every column) and `fits`;
// FindCgnrBlock finds every entry and nothing else.  The planner keeps the table
// as runs of equal blocks (cse::CgnrRun); the runs must partition it and
// ExpandCgnrBlocks must give it back.
#include <algorithm>
#include <cstdint>
#include <cstdio>
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

struct Block {
  int tangent;
  bool constant;
  int64_t delta;
};

void Check(const char* name, const std::vector<Block>& blocks, int64_t num_effective, bool want_tiles,
           bool want_fits) {
  std::vector<cse_parameter_block> pbs;
  int64_t state = 0, cstate = 0;
  for (const Block& b : blocks) {
    cse_parameter_block pb{};
    pb.size = pb.tangent_size = b.tangent;
    pb.is_constant = b.constant ? 1 : 0;
    pb.state_offset = b.constant ? cstate : state;
    (b.constant ? cstate : state) += b.tangent;
    pb.delta_offset = b.constant ? 0 : b.delta;
    pb.plus_jacobian_offset = -1;
    pbs.push_back(pb);
  }
  cse_problem_desc d{};
  d.abi_version = CSE_ABI_VERSION;
  d.num_parameter_blocks = (int64_t)pbs.size();
  d.parameter_blocks = pbs.data();
  d.num_effective_parameters = num_effective;
  cse::CgnrBlockPlan plan;
  plan.max_size = 77;  // overwritten
  cse::PlanCgnrBlocks(&d, &plan);
  // The table is kept as runs and expanded on demand.
  std::vector<cse::CgnrBlock> table;
  table.push_back({1, 2, 3, 0});  // overwritten
  cse::ExpandCgnrBlocks(plan, &table);
  EXPECT((int64_t)table.size() == plan.num_blocks);
  int64_t in_runs = 0;
  for (const cse::CgnrRun& r : plan.runs) {
    EXPECT(r.first_block == in_runs && r.count > 0);
    in_runs += r.count;
  }
  EXPECT(in_runs == plan.num_blocks);

  // Brute force: the active blocks with columns, by delta offset (stable).
  std::vector<Block> act;
  for (const Block& b : blocks)
    if (!b.constant && b.tangent > 0) act.push_back(b);
  std::stable_sort(act.begin(), act.end(), [](const Block& x, const Block& y) { return x.delta < y.delta; });
  EXPECT(table.size() == act.size());
  int64_t values = 0;
  int max_size = 0;
  for (size_t i = 0; i < act.size() && i < table.size(); ++i) {
    EXPECT(table[i].delta_offset == act[i].delta);
    EXPECT(table[i].tangent_size == act[i].tangent);
    EXPECT(table[i].value_offset == values);
    values += (int64_t)act[i].tangent * act[i].tangent;
    max_size = std::max(max_size, act[i].tangent);
  }
  EXPECT(plan.num_values == values);
  EXPECT(plan.max_size == max_size);
  // Every column of [0, num_effective) covered exactly once, and none outside.
  std::vector<int> cover((size_t)std::max<int64_t>(num_effective, 0), 0);
  bool tiles = true;
  for (const Block& b : act)
    for (int c = 0; c < b.tangent; ++c) {
      const int64_t col = b.delta + c;
      if (col < 0 || col >= num_effective)
        tiles = false;
      else
        ++cover[(size_t)col];
    }
  for (int v : cover) tiles = tiles && v == 1;
  EXPECT(tiles == want_tiles);
  EXPECT(plan.tiles == tiles);
  EXPECT(plan.fits == (max_size <= cse::kCgnrMaxBlockColumns));
  EXPECT(plan.fits == want_fits);
  // Lookup (of a table that tiles: JACOBI takes no other): every entry by its
  // offset, nothing in between.
  for (size_t i = 0; tiles && i < table.size(); ++i) {
    const cse::CgnrRun* run = nullptr;
    const int64_t at = cse::FindCgnrBlock(plan, table[i].delta_offset, &run);
    EXPECT(at >= 0 && table[(size_t)at].delta_offset == table[i].delta_offset);
    EXPECT(run && run->first_block <= at && at < run->first_block + run->count);
    if (tiles) EXPECT(at == (int64_t)i && run->tangent_size == table[i].tangent_size);
    if (table[i].tangent_size > 1 && tiles)
      EXPECT(cse::FindCgnrBlock(plan, table[i].delta_offset + 1) == -1);
  }
  EXPECT(cse::FindCgnrBlock(plan, -1) == -1);
  EXPECT(cse::FindCgnrBlock(plan, num_effective) == -1);
  std::printf("%-28s %3zu blocks in %zu runs, %4lld values, max %2d: %s%s\n", name, table.size(),
              plan.runs.size(), (long long)plan.num_values, plan.max_size, plan.tiles ? "tiles" : "refused (does not tile)",
              plan.fits ? "" : ", refused (oversize)");
}

}  // namespace

int main() {
  // points of 3, cameras of 9, in order
  Check("bal-shaped", {{3, false, 0}, {3, false, 3}, {3, false, 6}, {9, false, 9}, {9, false, 18}}, 27, true, true);
  // sizes 1 to 16 mixed
  Check("mixed sizes", {{1, false, 0}, {16, false, 1}, {2, false, 17}, {10, false, 19}, {7, false, 29}, {11, false, 36}},
        47, true, true);
  // constant blocks at the start, in the middle and at the end
  Check("constant blocks in the middle",
        {{9, true, 0}, {3, false, 0}, {9, true, 0}, {4, false, 3}, {3, true, 0}, {9, false, 7}, {2, true, 0}}, 16, true,
        true);
  // the program lists the cameras first, their columns come last
  Check("blocks out of delta order", {{9, false, 6}, {9, false, 15}, {3, false, 0}, {3, false, 3}}, 24, true, true);
  // columns [6, 8) belong to no block
  Check("a gap", {{3, false, 0}, {3, false, 3}, {9, false, 8}}, 17, false, true);
  // the last block stops short of num_effective_parameters
  Check("a gap at the end", {{3, false, 0}, {3, false, 3}}, 7, false, true);
  // two blocks share column 3
  Check("an overlap", {{4, false, 0}, {3, false, 3}}, 6, false, true);
  // 17 tangent columns
  Check("an oversize block", {{3, false, 0}, {17, false, 3}}, 20, true, false);
  // a block without columns is no entry
  Check("a zero-size block", {{3, false, 0}, {0, false, 3}, {2, false, 3}}, 5, true, true);
  Check("every block constant", {{3, true, 0}, {9, true, 0}}, 0, true, true);
  Check("an empty program", {}, 0, true, true);
  if (g_failures) {
    std::printf("%d failures\n", g_failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
