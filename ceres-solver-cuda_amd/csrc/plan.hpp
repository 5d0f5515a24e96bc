// plan.hpp -- the host-only planner behind cse_create.
//
// Everything the evaluator decides about a cse_problem_desc before it touches
// the GPU: descriptor validation, the layout policy of each residual group,
// its gradient plans and store runs, and the program-level tables (Plus runs,
// the Schur structure, the PbDev table).  Plain C++17 over include/cse.h and
// host_shared.hpp, so a CPU program (tests/cpp/asan_driver.cpp, built by g++)
// can drive it under ASan/UBSan.  The library's own plan.o is built by ROCm's
// clang++, not g++: cse_create's loops over every residual block ran about
// 15 % slower as g++ -O3 compiled them (the Makefile has the figures).
//
// cse_create (cse_evaluator.hip) is the one caller that uploads:
//   Validate, ValidateGroups                    refuse or accept the descriptor
//   for each group: PlanGroup, upload, release  one group's tables at a time
//   PlanProgram, upload
// The scalars of a plan are plain structs that the evaluator's Group and
// Group::GradPlan derive from; the tables are std::vectors the caller may
// drop as soon as they are uploaded (a slot-0 perm is 116 MB at
// problem-13682).
#ifndef CSE_PLAN_HPP_
#define CSE_PLAN_HPP_

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/cse.h"
#include "host_shared.hpp"

// Records msg as the thread's last error (cse_last_error) and returns code.
int CseFail(int code, const std::string& msg);

namespace cse {

// Layout policy of a group: 0 = table, 1 = affine packed cells (BSM),
// 2 = affine interleaved rows (CRS).
enum Policy { kTable = 0, kAffinePacked = 1, kAffineCrs = 2 };

// Internal kernel kinds (never in a descriptor): a group whose slot-0
// blocks carry a manifold the affine kernels build in registers.
constexpr int kKindQuaternionTangent = -100;  // SNAVELY_QUATERNION_2_10_3, slot 0 on
                                              // CSE_MANIFOLD_QUATERNION_EUCLIDEAN

struct KindShape {
  int nr = 0, nb = 0, data = 0;
  int sz[kMaxSlots] = {};
  int s0 = 0, s1 = 0;  // sz[0], sz[1] (0 if absent): the two-slot affine path
  int x0 = 0;          // slot-0 values gathered (ambient; s0 is the Jacobian's columns)
};

// The shapes of the library's functor kinds; cse_evaluator.hip ties every row
// to the kind's KindTraits by static_assert.
struct KindRow {
  int kind, nr, nb, data, x0;
  int sz[kMaxSlots];
};
constexpr KindRow kKindRows[] = {
    {kKindQuaternionTangent, 2, 2, 2, 10, {9, 3}},
    {CSE_FUNCTOR_SNAVELY_2_9_3, 2, 2, 2, 9, {9, 3}},
    {CSE_FUNCTOR_SNAVELY_NO_DISTORTION_2_7_3, 2, 2, 2, 7, {7, 3}},
    {CSE_FUNCTOR_SNAVELY_QUATERNION_2_10_3, 2, 2, 2, 10, {10, 3}},
    {CSE_FUNCTOR_POINT_DISPLACEMENT_3_3, 3, 1, 3, 3, {3}},
    {CSE_FUNCTOR_TEST_LINEAR_3_2_3_4, 3, 3, 2, 2, {2, 3, 4}},
    {CSE_FUNCTOR_TEST_LINEAR_3_4_3_2, 3, 3, 2, 4, {4, 3, 2}},
    {CSE_FUNCTOR_TEST_LINEAR_2_2_3, 2, 2, 2, 2, {2, 3}},
    {CSE_FUNCTOR_TEST_LINEAR_3_2_4, 3, 2, 2, 2, {2, 4}},
    {CSE_FUNCTOR_TEST_LINEAR_4_3_4, 4, 2, 2, 3, {3, 4}},
    {CSE_FUNCTOR_TEST_BILINEAR_1_2_2, 1, 2, 1, 2, {2, 2}},
    {CSE_FUNCTOR_TEST_TEN_PARAMETER_1_x10, 1, 10, 1, 1, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1}},
    {CSE_FUNCTOR_TEST_PARTIAL_OUTPUT_2_1, 2, 1, 1, 1, {1}},
};
constexpr const KindRow* KindRowOf(int kind) {
  for (const KindRow& r : kKindRows)
    if (r.kind == kind) return &r;
  return nullptr;
}

// The shape of a library kind, or of a registered user kind (user = its
// launch table); false for a kind that is neither.
bool ShapeOf(int kind, const cse_functor_ops* user, KindShape* k);

// Known-answer-test kinds: general path and trivial loss only.
inline bool IsTestKind(int kind) { return kind >= 100 && kind < CSE_FUNCTOR_USER_FIRST; }

// Kinds with the fused gradient: the Snavely camera and the quaternion
// camera on its manifold (the same 2 x (9 + 3) Jacobian shape).
inline bool FusedKind(int kind) {
  return kind == CSE_FUNCTOR_SNAVELY_2_9_3 || kind == kKindQuaternionTangent;
}

// The Jacobian operators built for the Snavely shape (CgnrMultiplyKernel,
// the Schur kernels) read only the Jacobian's values, so they serve every
// fused-gradient group of that shape -- 2 residuals, blocks of 9 (tangent)
// and 3 -- the library's kinds and user kinds alike.
inline bool SnavelyShaped(const KindShape& k) {
  return k.nb == 2 && k.nr == 2 && k.s0 == 9 && k.s1 == 3;
}

// Every affine kernel of a user kind present (the header builds all eight
// or none).
bool UserAffine(const cse_functor_ops* u);

// User kinds that registered the fused gradient's launches (cse_functor_ops
// ABI 5: two slots, slot 1 of 3 parameters): gradient_mode 0's form only
// (points kernel, CameraGradientKernel, the tail); the other modes, the Jet
// form and the operators stay with the library's kinds.
bool UserFused(const cse_functor_ops* user, const KindShape& k);

// A registered user kind and its name; null for any other kind.  The
// registry lives in cse_evaluator.hip; a caller without user kinds passes a
// null lookup.
using UserLookup = const cse_functor_ops* (*)(int kind, std::string* name);

// ---- Gradient post-pass plan of one slot (affine groups with a Jacobian
// layout): the scalars, and the tables BuildGradPlan fills.
struct GradPlanInfo {
  bool ready = false;
  bool sorted = true;  // blocks already in parameter-block order: no perm, no chunks
  bool wave = false;   // one wave (not one lane) per parameter block
  int32_t lo = 0;
  int64_t count = 0;
  int passes = 1;
  int64_t nchunks = 0;
  int64_t nperm = 0;  // blocks in the plan (all but those with a constant block)
  bool all_present = false;  // every id in [lo, lo + count) has a block
};
struct GradTables {
  std::vector<int32_t> perm;  // empty = identity
  std::vector<int64_t> off;
  // !sorted: chunks of at most kGradChunk blocks
  std::vector<int64_t> chunk_begin, chunk_off;
  std::vector<int32_t> chunk_pb;     // parameter block (id) of each chunk
  std::vector<int32_t> chunk_order;  // passes > 1: the chunks pass-major
};

int CamGradPasses(const cse_residual_group& g, const KindShape& k);
void BuildGradPlan(const cse_residual_group& g, const KindShape& k, int j, GradPlanInfo* plan,
                   GradTables* tables, const cse_parameter_block* cpb = nullptr, int passes = 1);

// ---- One residual group: every decision PlanGroup makes, as scalars.
struct GroupPlan {
  int kind = 0;
  const cse_functor_ops* user = nullptr;  // a registered user functor kind
  KindShape shape{};
  cse_loss loss{};
  // Doubles of loss parameters at the end of each functor_data row (0 or 2,
  // cse_residual_group.loss_data_size); no planning decision depends on it.
  int loss_data_size = 0;
  int64_t n = 0;
  bool affine = false;
  int policy = 0;
  int64_t partial_offset = 0;
  int64_t num_wg = 0;
  int64_t first = 0;
  // affine parameters
  int64_t state_base[2] = {0, 0};
  int64_t delta_base[2] = {0, 0};
  int64_t res_base = 0;
  int64_t jac_base[2][3] = {{0, 0, 0}, {0, 0, 0}};
  int64_t jac_stride[2] = {0, 0};
  // Repacked slot-0 table (affine path and plain table groups, small id
  // ranges): repack0 says the evaluator keeps one, slot0_count rows of
  // packed_stride doubles.
  bool repack0 = false;
  int32_t slot0_lo = 0;
  int64_t slot0_count = 0;
  int slot0_stride = 0;
  int packed_stride = 0;  // row stride of the repacked slot-0 table (doubles)
  // The manifold DetectAffine chose for slot 0, taken from the first block
  // with an active slot 0 (held blocks carry no Jacobian columns, so their
  // own manifold does not matter).
  int slot0_manifold = CSE_MANIFOLD_MATRIX;
  // Gradient mode 0 writes every gradient row exactly once (grad_exact): one
  // group, no constant blocks, every camera and point id of its ranges
  // present and their rows tiling the effective parameters.  Then the tail
  // kernels assign instead of adding and the gradient is not zeroed first.
  bool grad_exact = false;
  // Constant slot-0 blocks on the affine path: GroupTables' bits, src, dlt,
  // fbase and prev_seg; fbase0 = fbase[0] (HeldWindowsAligned).
  bool const0 = false;
  int64_t fbase0 = 0;
  // Fused gradient (cse::FusedGrad) eligibility.
  bool fuse_ok = false;
  // cse_options.jacobian_form = CSE_JACOBIAN_JET on a Snavely group: its
  // Jacobian kernels are the Jet<double, 12> instantiations (jet_kernels.h).
  bool jet = false;
  // Table policy: slot 0 plain in every block (DetectPlain0).
  bool plain0 = false;
  int64_t plain0_state_base = 0, plain0_delta_base = 0;
};

struct GroupTables {
  // const0: the active-bit table over the slot-0 id range, each id's repack
  // source (state offset, or -1 - constant-state offset) and delta offset,
  // per 64-block chunk the offset of its first F cell (BSM) or row block
  // (CRS) and then the end, and the previous chunk with a non-empty segment.
  std::vector<uint32_t> bits;
  std::vector<int64_t> src, dlt, fbase;
  std::vector<int32_t> prev_seg;
  // Table policy: each 64-block chunk's store runs, [chunks][2 + nb].
  std::vector<int64_t> runs;
  GradPlanInfo grad_info[2];
  GradTables grad[2];
};

// ---- The program: what validation counts, what the groups add up to, and
// the program-level tables.
struct SchurPlan {
  bool eligible = false;
  bool duplicates = false;  // an e block sees one f block twice
  int64_t e_cols = 0, f_cols = 0;
  int64_t f_col_base = 0;  // f index of camera id = f_col_base + 9 id (0 and unused when held)
  int64_t nchunks = 0, nbig = 0;
  // Held cameras (a const0 group): f_cols = 9 num_active, an active camera's f
  // index is 9 times its rank among the active ones (ProgramPlan::
  // schur_cam_rank) and the F cell of a block is found by its rank among the
  // blocks with an active camera (schur_chunk_held, schur_big_rank, schur_fcell).
  bool held = false;
  int64_t num_active = 0;
};

struct ProgramPlan {
  // ValidateGroups
  bool has_layout = false;
  std::vector<KindShape> shapes;               // per group
  std::vector<const cse_functor_ops*> users;   // per group, null for a library kind
  std::vector<std::string> user_names;
  std::vector<int32_t> owner;  // which (group, slot) uses each parameter block:
                               // 2 group + slot, -1 none, -2 several
  bool res_covered = true, jac_covered = true;  // every value is written by some block
  int64_t bytes_jac = 0, bytes_res = 0;
  // PlanGroup, summed over the groups
  int64_t total_wg = 0;
  bool any_general = false;
  // PlanProgram
  bool plus_supported = true;
  std::vector<PlusRun> plus_runs;
  std::vector<QuatPlusBlock> plus_quat;
  SchurPlan schur;
  std::vector<int64_t> schur_chunk_begin, schur_big;  // [begin, end) pairs
  // schur.held only (empty otherwise).  Per wave chunk (rank0, mask): the
  // F-cell rank of its first block -- the blocks with an active camera before
  // it -- and bit l set when block begin + l has one; per big run its rank0;
  // per entry q of the slot-0 gradient plan's perm the F-cell rank of block
  // perm[q]; per camera id lo + p of that plan's range its rank among the
  // active cameras, -1 if held.
  std::vector<int64_t> schur_chunk_held, schur_big_rank;
  std::vector<int32_t> schur_fcell, schur_cam_rank;
  std::vector<PbDev> pbs;                             // only when any_general
};

// The descriptor's own fields and parameter blocks.
int Validate(const cse_problem_desc* d);
// Every group and every residual block of it; fills the ValidateGroups part
// of the plan.  Nothing below may be called on a descriptor these two refuse.
// Per-block loss parameters (cse_residual_group.loss_data_size): the library's
// losses on the library's kinds, closed-form Jacobian.  Their values are not
// checked, as the uniform loss.a and loss.scale are not.  Needs Validate(d)
// only, so cse_create refuses these before it touches a device;
// ValidateGroups applies it too.  opts may be null (no options to check).
int ValidateLossData(const cse_problem_desc* d, const cse_options* opts);
int ValidateGroups(const cse_problem_desc* d, UserLookup lookup, ProgramPlan* P,
                   const cse_options* opts = nullptr);

// Plans group gi: G and T are overwritten, P's sums advance.
void PlanGroup(const cse_problem_desc* d, const cse_options& opts, int gi, ProgramPlan* P,
               GroupPlan* G, GroupTables* T);
// After every group: the Plus runs, the PbDev table and the Schur structure
// (only = the plan of the program's one group, null when it has several;
// only_tables = that group's tables, needed for the Schur structure of a group
// with held cameras alone: without them such a group is not eligible).
void PlanProgram(const cse_problem_desc* d, const GroupPlan* only, ProgramPlan* P,
                 const GroupTables* only_tables = nullptr);

// ---- cse_cgnr_init's block-Jacobi preconditioner: one entry per non-constant
// parameter block with columns, sorted by delta_offset; value_offset is the
// running sum of tangent_size^2 (packed row-major blocks,
// BlockCRSJacobiPreconditioner's storage, block_jacobi_preconditioner.cc:135-170).
// Needs only the descriptor's parameter blocks and num_effective_parameters.
// cse_create keeps the table as runs -- consecutive entries of one size whose
// columns follow each other (two runs for a BAL problem: the points, the
// cameras) -- so that a program that never asks for JACOBI pays a pass over its
// parameter blocks and a few bytes; the first JACOBI init expands them
// (ExpandCgnrBlocks: 24 bytes per block, 107 MB at problem-13682), uploads the
// table and drops it.
struct CgnrRun {
  int64_t delta_offset;  // of the run's first block
  int64_t value_offset;
  int64_t first_block;   // its index in the table
  int64_t count;
  int32_t tangent_size;
  int32_t pad;
};
struct CgnrBlockPlan {
  std::vector<CgnrRun> runs;
  int64_t num_blocks = 0;
  int64_t num_values = 0;  // sum of tangent_size^2
  int max_size = 0;        // largest tangent_size
  // JACOBI needs both: the blocks tile [0, num_effective_parameters) exactly
  // (no gap, no overlap), and none has more than kCgnrMaxBlockColumns columns.
  bool tiles = false;
  bool fits = false;
};
void PlanCgnrBlocks(const cse_problem_desc* d, CgnrBlockPlan* plan);
// The table itself, num_blocks entries.
void ExpandCgnrBlocks(const CgnrBlockPlan& plan, std::vector<CgnrBlock>* blocks);
// The index of the entry whose delta_offset is `delta`, or -1; *run (may be
// null) receives its run.  For a plan that tiles (runs that overlap may hide
// an entry; JACOBI refuses such a plan before any lookup).
int64_t FindCgnrBlock(const CgnrBlockPlan& plan, int64_t delta, const CgnrRun** run = nullptr);

// ---- The explicit Schur complement's pair plan (cse_schur_complement): which
// residual-block pairs add into which 9 x 9 block of S.  Host only; built on
// the first cse_schur_complement or cse_schur_complement_plan call, never by
// cse_create (it is sum_p k_p^2 in size).
constexpr int kSchurPairChunk = 64;  // pairs per work chunk (one wave each)
constexpr int kSchurBlockDoubles = 81;

struct SchurPairCounts {
  int64_t num_blocks = 0;  // non-zero blocks of S's upper triangle, diagonal included
  int64_t num_pairs = 0;   // pair records
  int64_t num_chunks = 0;  // work chunks: sum over blocks of ceil(pairs / kSchurPairChunk)
  int64_t plan_bytes = 0;  // device bytes of the tables below and the chunk partials
};
struct SchurPairPlan : SchurPairCounts {
  // Block k = S(block_row[k], block_col[k]), parameter-block ids with row <=
  // col, in lexicographic order; its pairs are [pair_begin[k], pair_begin[k+1])
  // and its chunks [chunk_off[k], chunk_off[k+1]): chunk q of block k takes
  // kSchurPairChunk pairs from pair_begin[k] + (q - chunk_off[k]) kSchurPairChunk,
  // so no chunk straddles a block.
  std::vector<int32_t> block_row, block_col;
  std::vector<int64_t> pair_begin, chunk_off;  // [num_blocks + 1]
  std::vector<int32_t> chunk_block;            // [num_chunks]
  // [num_pairs][2]: residual blocks (b, b') of one e block with f block of b =
  // block_row, of b' = block_col, ordered by (e block, b, b') inside a block.
  // A diagonal block holds every ordered pair, b = b' included (that pair
  // also carries F_b^T F_b).
  std::vector<int32_t> pairs;
};
// ids: the group's [n][2] (f block, e block), sorted by e block (each e
// block's rows one contiguous run).  counts_only fills the SchurPairCounts
// part alone.  Needs a host table of 8 C^2 bytes for C = the f-block id range
// (1/81 of the dense S the plan is for).  CSE_ERR_UNSUPPORTED when n >= 2^31
// (pair entries are int32), CSE_ERR_OOM when host memory runs out.
// cluster (may be null: every block): cluster[id - first_id] is the label of f
// block id; only the blocks whose two f blocks carry one label are kept.  A
// kept block's pairs, their order and its chunk cut are the unfiltered
// plan's (the same walk with the other blocks' counts left at zero).
// neighbor (may be null; needs cluster): [labels][2], the labels a cluster is
// joined to by an edge of the cluster forest (-1: none); a block whose two
// labels are joined is kept too (CLUSTER_TRIDIAGONAL).
int PlanSchurPairs(const int32_t* ids, int64_t n, bool counts_only, SchurPairPlan* plan,
                   const int32_t* cluster = nullptr, int32_t first_id = 0, const int32_t* neighbor = nullptr);

// ---- CLUSTER_JACOBI (cse_schur_set_clusters, cse_schur_cluster_jacobi): the
// cluster-filtered pair plan and where its blocks go.  Cluster g of n_g
// cameras c_0 < c_1 < .. (camera index = f block id - first_id, in f-column
// order) owns the n_g (n_g + 1) / 2 tiles of its upper triangle from
// first_tile[g]: tile first_tile[g] + j (j + 1) / 2 + i, i <= j, is S(c_i, c_j),
// 81 doubles row-major as the block-sparse store writes a block.
constexpr int kSchurMaxClusterCameras = 16;
constexpr int64_t ClusterTile(int64_t i, int64_t j) { return j * (j + 1) / 2 + i; }  // i <= j

struct SchurClusterCounts {
  int64_t num_clusters = 0, num_cameras = 0;
  int64_t num_tiles = 0;        // sum of n_g (n_g + 1) / 2
  int64_t num_values = 0;       // sum of (9 n_g)^2: the unfactored matrices
  int64_t max_cameras = 0;      // largest n_g
  int64_t finish_capacity = 0;  // bound on the finish list known from the counts
};
struct SchurClusterPlan : SchurClusterCounts {
  SchurPairPlan pairs;                  // the filtered plan
  std::vector<int32_t> camera_begin;    // [num_clusters + 1] into cameras
  std::vector<int32_t> cameras;         // [num_cameras]: ascending inside a cluster
  std::vector<int64_t> first_tile;      // [num_clusters + 1]
  std::vector<int64_t> value_begin;     // [num_clusters + 1]: offset of M_g in the matrices
  std::vector<int32_t> tile_of_plan;    // [pairs.num_blocks]: a plan block's tile
  std::vector<int32_t> plan_of_tile;    // [num_tiles]: the inverse, -1 = no plan block writes it
  std::vector<int32_t> tile_camera;     // [num_tiles]: camera index of the tile's row block
  // The tiles the finish kernel writes: several chunks, or the diagonal of a
  // camera without residual blocks (D^2 or zeros).  The off-diagonal tiles no
  // plan block writes are not listed: they are zero, and the caller zeroes them.
  std::vector<int32_t> finish;
  std::vector<int32_t> empty_tiles;     // every tile with plan_of_tile = -1, diagonal or not
};
// cluster[c], c in [0, C): labels in [0, num_clusters), every label used, no
// cluster above kSchurMaxClusterCameras (CSE_ERR_INVALID / CSE_ERR_UNSUPPORTED
// otherwise).  counts_only fills the SchurClusterCounts part and the counts
// of `pairs` alone.
int ValidateSchurClusters(const int32_t* cluster, int64_t C, int32_t num_clusters);
int PlanSchurClusters(const int32_t* ids, int64_t n, int32_t first_id, int64_t C, const int32_t* cluster,
                      int32_t num_clusters, bool counts_only, SchurClusterPlan* plan);

// ---- CLUSTER_TRIDIAGONAL (cse_schur_set_cluster_forest,
// cse_schur_cluster_tridiagonal): the partition above and a forest over its
// clusters in which every cluster has at most two edges, so that each tree is
// a path.  M keeps S's blocks inside a cluster and between the two clusters of
// an edge; in path order it is block tridiagonal.
//
// The tiles: the clusters' triangles exactly as SchurClusterPlan lays them
// out (tiles [0, first_tile[num_clusters])), then per edge e = (g, h), as it
// was given, a rectangle of n_g n_h tiles from edge_tile[e]: tile
// edge_tile[e] + i n_h + j belongs to the cameras a = (camera i of g) and
// b = (camera j of h) and HOLDS S(min(a, b), max(a, b)), the plan's block,
// row-major as the block store writes it.  So it is S(a, b) when a < b and its
// transpose otherwise; the kernels compare the two camera indices.  An edge's
// two clusters hold at most kSchurMaxClusterCameras cameras together: one
// elimination step works on their combined triangle in one workgroup's LDS.
struct SchurForestPaths {
  // Path p is path_cluster[path_begin[p] .. path_begin[p + 1]), listed from its
  // end with the smaller label; the paths are ordered by their first cluster; a
  // cluster without an edge is a path of one.  path_edge[q] joins
  // path_cluster[q] and path_cluster[q + 1]: 2 e + flip, flip = 1 when
  // path_cluster[q] is the edge's h; -1 at a path's last cluster.
  std::vector<int32_t> path_begin, path_cluster, path_edge;
  std::vector<int32_t> neighbor;  // [num_clusters][2], -1 = none
};
// edges: [num_edges][2] labels.  size[g] = cameras of cluster g.
// CSE_ERR_INVALID: null edges with num_edges > 0, a label out of range, g = h,
// a duplicate (in either orientation).  CSE_ERR_UNSUPPORTED, naming the
// cluster or edge: a cluster with three edges, a cycle, an edge whose clusters
// hold more than kSchurMaxClusterCameras cameras together.
int ValidateSchurForest(const int32_t* edges, int32_t num_edges, const int32_t* size, int32_t num_clusters,
                        SchurForestPaths* paths);

struct SchurTridiagonalCounts : SchurClusterCounts {
  // num_tiles, num_values: the clusters' and the edges' together.
  int64_t num_edges = 0, num_paths = 0;
  int64_t num_cluster_tiles = 0;  // the clusters' triangles: the edges' rectangles follow
  int64_t max_step_cameras = 0;   // the most cameras one elimination step holds: an edge's two clusters, or a lone cluster
  int64_t longest_path = 0;       // clusters
};
struct SchurTridiagonalPlan : SchurTridiagonalCounts {
  SchurPairPlan pairs;                // the filtered plan: one label, or the two labels of an edge
  std::vector<int32_t> camera_begin, cameras;
  std::vector<int64_t> first_tile, value_begin;   // per cluster, as SchurClusterPlan's
  std::vector<int32_t> edges;                     // [num_edges][2] as given
  std::vector<int64_t> edge_tile, edge_value;     // [num_edges + 1]: first tile; offset of S[g, h] in the matrices
  SchurForestPaths paths;
  std::vector<int32_t> tile_of_plan, plan_of_tile, tile_camera, finish, empty_tiles;  // as SchurClusterPlan's
};
int PlanSchurTridiagonal(const int32_t* ids, int64_t n, int32_t first_id, int64_t C, const int32_t* cluster,
                         int32_t num_clusters, const int32_t* edges, int32_t num_edges, bool counts_only,
                         SchurTridiagonalPlan* plan);

// ---- The block-sparse Schur complement (cse_schur_complement_sparse,
// cse_schur_explicit_multiply): S's upper triangle as block-compressed rows,
// BlockRandomAccessSparseMatrix's cells (SPARSE_SCHUR, and ITERATIVE_SCHUR's
// use_explicit_schur_complement).  Cameras are indexed 0 .. C-1 in f-column
// order; every camera has its diagonal block, observed or not.
constexpr int kSchurExplicitWaves = 4;  // waves that share one row of the product

// The product's fixed cut of a camera's `len` row blocks over the waves of its
// workgroup: wave w takes [w per, (w + 1) per) clipped to len.
constexpr int kSchurExplicitSlots = 28;  // partial sums of a camera's column contributions (28 x 9 threads)
constexpr int64_t SchurExplicitPer(int64_t len) {
  return (len + kSchurExplicitWaves - 1) / kSchurExplicitWaves;
}

struct SchurSparseCounts {
  int64_t num_block_rows = 0;   // C
  int64_t num_blocks = 0;       // the pair plan's blocks + the added diagonals
  int64_t finish_capacity = 0;  // bound on num_finish known from the counts alone
  int64_t device_bytes = 0;     // device bytes of the tables below (col_row stays on the host)
                                // and of the product's 72-byte column contribution per block
};
struct SchurSparsePlan : SchurSparseCounts {
  // Block k of row c, k in [row_begin[c], row_begin[c+1]), is S(c, block_col[k]);
  // block_col ascends inside a row and starts at c.
  std::vector<int64_t> row_begin;       // [C + 1]
  std::vector<int32_t> block_col;       // [num_blocks]
  std::vector<int32_t> plan_block;      // [num_blocks]: the pair plan's block, -1 = added diagonal
  std::vector<int32_t> sparse_of_plan;  // [pair plan's num_blocks]: the inverse
  // The blocks the finish kernel writes (several chunks, or an added
  // diagonal); the others are stored by their one chunk.
  std::vector<int32_t> finish;          // [num_finish <= finish_capacity]
  // The transposed index: the blocks of column c above the diagonal are
  // col_block[j], j in [col_begin[c], col_begin[c+1]), of rows col_row[j],
  // in ascending row order (the product sums contributions in this order).
  std::vector<int64_t> col_begin;            // [C + 1]
  std::vector<int32_t> col_block, col_row;   // [num_blocks - C]
};
// From the pair plan of the same ids (a counts-only plan when counts_only):
// camera index = f block id - first_id, in [0, C).  counts_only fills the
// SchurSparseCounts part alone (it marks the observed cameras in C bits and
// builds no table).  CSE_ERR_INVALID when an id falls outside the C cameras,
// CSE_ERR_UNSUPPORTED at 2^31 or more blocks, CSE_ERR_OOM.
int PlanSchurSparse(const int32_t* ids, int64_t n, const SchurPairPlan& plan, int32_t first_id, int64_t C,
                    bool counts_only, SchurSparsePlan* sparse);

// ---- The dense Cholesky factorization (cse_dense_cholesky_*): a blocked
// right-looking factorization, one panel of kDenseCholeskyNB columns per step.
// Step k launches the diagonal kernel (one workgroup), then -- unless it is
// the last -- the panel kernel over the block rows below it and the trailing
// update over the lower-triangle tiles of the remaining block rows; a solve
// launches one kernel per block row forward and one backward.
constexpr int kDenseCholeskyNB = 64;
constexpr int64_t kDenseCholeskyAlign = 256;  // every workspace segment's size is a multiple

struct DenseCholeskyPlan {
  int64_t n = 0;
  int32_t precision = 0;
  int64_t num_panels = 0;  // ceil(n / NB)
  int64_t padded = 0;      // num_panels * NB: the length of the workspace vectors
  // Kernel launches of a factorization (the FP32 cast included), of one
  // forward + backward substitution, and of a whole solve with `refinements`
  // refinement iterations: SolveLaunches(refinements).
  int64_t factor_launches = 0, substitution_launches = 0;
  // The workspace, in bytes from its start.  FP64: the inverses of the
  // diagonal blocks [num_panels][NB][NB], the vectors v and y [padded], the
  // failure flag.  FP32: the float copy of the matrix [n][n] first, those in
  // float, and the FP64 vectors x and r [padded] of the refinement.
  int64_t matrix_off = 0, inverse_off = 0, v_off = 0, y_off = 0, x_off = 0, r_off = 0, flag_off = 0;
  int64_t workspace_bytes = 0;
  int64_t SolveLaunches(int64_t refinements) const {
    // FP64: load, substitutions, store.  FP32: init, per iteration cast +
    // substitutions + accumulate, a residual between iterations, store.
    if (precision == 0) return substitution_launches + 2;
    return 1 + (refinements + 1) * (substitution_launches + 2) + refinements + 1;
  }
};

// The launch grids of step k (workgroups): the panel kernel takes the block
// rows k+1 .. num_panels-1, the trailing update the lower-triangle tiles (i, j),
// k < j <= i, of those R rows, folded into (R + 1) x ceil(R / 2) workgroups:
// grid row y holds block row y's y + 1 tiles and then block row R-1-y's R - y.
constexpr int64_t DenseCholeskyRowsBelow(int64_t num_panels, int64_t k) { return num_panels - k - 1; }
constexpr int64_t DenseCholeskyTrailingGridX(int64_t R) { return R + 1; }
constexpr int64_t DenseCholeskyTrailingGridY(int64_t R) { return (R + 1) / 2; }
struct DenseCholeskyTile {
  int64_t i, j;  // block row and column among the R remaining, j <= i
  bool live;     // false: the odd middle row's second half, no tile
};
constexpr DenseCholeskyTile DenseCholeskyTrailingTile(int64_t R, int64_t x, int64_t y) {
  if (x <= y) return DenseCholeskyTile{y, x, true};
  return DenseCholeskyTile{R - 1 - y, x - y - 1, R - 1 - y != y};
}

// CSE_ERR_INVALID: n < 1 or an unknown precision.
int PlanDenseCholesky(int64_t n, int32_t precision, DenseCholeskyPlan* plan);

// ---- The block-sparse Cholesky factorization (cse_sparse_cholesky_*): the
// SparseCholesky behind SPARSE_SCHUR (sparse_cholesky.h:72-113), a supernode =
// one 9 x 9 block column.  The input is the upper triangle A(r, c), r <= c, as
// block-compressed rows (PlanSchurSparse's format).  With B = P A P^T and
// permutation[k] = the original block row at position k, L's block (i, j),
// i >= j, starts from B(i, j): the input block (permutation[j], permutation[i])
// transposed, or (permutation[i], permutation[j]) as it is.
//
// The factorization is left-looking by levels of the elimination tree: every
// block of column j reads columns on lower levels only, so one level's columns
// are independent.  A level launches the diagonal kernel over its columns and
// the target kernel over its off-diagonal blocks; a solve launches one kernel
// a level forward and one backward.
struct SparseCholeskyCounts {
  int64_t num_block_rows = 0, num_input_blocks = 0, num_factor_blocks = 0;
  // sum over columns k of m_k (m_k + 1) / 2, m_k = the blocks of column k below
  // its diagonal: the 9 x 9 x 9 products of one factorization.
  int64_t num_block_products = 0;
  int64_t device_bytes = 0;
  int32_t num_levels = 0, max_level_columns = 0;
};
struct SparseCholeskyPlan : SparseCholeskyCounts {
  std::vector<int32_t> permutation, position;  // position = the inverse
  // L by block rows in the permuted order: row i is [row_begin[i],
  // row_begin[i + 1]), columns ascending, the diagonal last.
  std::vector<int64_t> row_begin;  // [N + 1]
  std::vector<int32_t> block_col, block_row;  // [num_factor_blocks]
  // The column index: the blocks of column j below the diagonal, rows ascending.
  std::vector<int64_t> col_begin;  // [N + 1]
  std::vector<int32_t> col_block;  // [num_factor_blocks - N]
  std::vector<int32_t> parent, level;  // [N]; parent -1 at a root
  // Scatter: input block b lands in L's block scatter[b] as it is, or, when
  // scatter[b] is negative, in block ~scatter[b] transposed.  source is the
  // inverse by L's blocks: input block source[t] >= 0 as it is, -1 = fill,
  // source[t] <= -2 = input block -2 - source[t] transposed.  Both hold every
  // index below 2^31 - 1.
  std::vector<int32_t> scatter;  // [num_input_blocks]
  std::vector<int32_t> source;   // [num_factor_blocks]
  // The level table: level l's columns are level_columns[level_begin[l] ..
  // level_begin[l + 1]) ascending, its off-diagonal target blocks
  // level_targets[target_begin[l] .. target_begin[l + 1]) ascending.
  std::vector<int64_t> level_begin, target_begin;  // [num_levels + 1]
  std::vector<int32_t> level_columns;              // [N]
  std::vector<int32_t> level_targets;              // [num_factor_blocks - N]
  // The input's own arrays and its transposed index (the refinement's
  // residual reads the lower half through it): the blocks of column c above
  // the diagonal are in_col_block[in_col_begin[c] ..), of rows in_col_row, ascending.
  std::vector<int64_t> in_row_begin, in_col_begin;  // [N + 1]
  std::vector<int32_t> in_block_col;                // [num_input_blocks]
  std::vector<int32_t> in_col_block, in_col_row;    // [num_input_blocks - N]
};
// The greedy minimum-degree order: repeatedly the block row with the fewest
// uneliminated neighbours in the elimination graph (fill edges included), the
// lowest index on ties; once the remaining graph is a clique the rest follows
// in index order.  Bit rows: N^2 / 8 bytes of host memory.
int SparseCholeskyMinimumDegree(int64_t N, const int64_t* row_begin, const int32_t* block_col,
                                std::vector<int32_t>* permutation);
// ordering: CSE_SPARSE_ORDERING_*; permutation is read with GIVEN only.
// CSE_ERR_INVALID: null pointers, N < 1, a row without its leading diagonal,
// columns not ascending or out of range, a GIVEN array that is no permutation,
// an unknown ordering.  CSE_ERR_UNSUPPORTED: 2^31 or more factor blocks (or
// 9 N + 1 beyond int32).  CSE_ERR_OOM.
int PlanSparseCholesky(int64_t N, const int64_t* row_begin, const int32_t* block_col, int32_t ordering,
                       const int32_t* permutation, SparseCholeskyPlan* plan);

}  // namespace cse

#endif  // CSE_PLAN_HPP_
