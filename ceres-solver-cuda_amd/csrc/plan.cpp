// plan.cpp -- the host-only planner behind cse_create (plan.hpp).
//
// Pure host logic over a cse_problem_desc: no HIP, no device memory.  The
// caller validates first (Validate, ValidateGroups); the planning functions
// index the descriptor's arrays without further checks.
#include "plan.hpp"

#include <algorithm>
#include <cmath>
#include <new>
#include <utility>

namespace cse {
std::string& LastError();  // layout.cpp: one per thread, shared by every entry point
}  // namespace cse

int CseFail(int code, const std::string& msg) {
  cse::LastError() = msg;
  return code;
}

namespace cse {

namespace {

int Fail(int code, const std::string& msg) { return CseFail(code, msg); }

// Gradient post-pass kernels of the built-in shapes; a user kind brings its
// own (cse_functor_ops.gradient).
bool GradSupported(int nr, int size, const cse_functor_ops* user, int slot) {
  if (user) return user->gradient[slot] != nullptr;
  return (nr == 2 && (size == 9 || size == 3 || size == 7 || size == 10)) || (nr == 3 && size == 3);
}

int64_t BlockIndex(const cse_residual_group& g, int64_t i) {
  return g.residual_block_index ? g.residual_block_index[i] : g.first_residual_block + i;
}

}  // namespace

bool ShapeOf(int kind, const cse_functor_ops* user, KindShape* k) {
  *k = KindShape{};
  if (user) {
    k->nr = user->num_residuals;
    k->nb = user->num_parameter_blocks;
    k->data = user->data_size;
    for (int j = 0; j < k->nb; ++j) k->sz[j] = user->parameter_block_sizes[j];
    k->x0 = k->sz[0];
  } else {
    const KindRow* r = KindRowOf(kind);
    if (!r) return false;
    k->nr = r->nr;
    k->nb = r->nb;
    k->data = r->data;
    for (int j = 0; j < r->nb; ++j) k->sz[j] = r->sz[j];
    k->x0 = r->x0;
  }
  k->s0 = k->sz[0];
  k->s1 = k->nb > 1 ? k->sz[1] : 0;
  return true;
}

bool UserAffine(const cse_functor_ops* u) {
  bool all = true;
  for (int c = 0; c < 2; ++c)
    for (int j = 0; j < 2; ++j)
      for (int d = 0; d < 2; ++d) all = all && u->affine[c][j][d] != nullptr;
  return all;
}

bool UserFused(const cse_functor_ops* user, const KindShape& k) {
  return user && user->fused_points[0] && user->fused_points[1] && user->camera_gradient &&
         k.nb == 2 && k.s1 == 3 && k.s0 >= 1 && k.s0 <= 16;
}

int Validate(const cse_problem_desc* d) {
  if (!d) return Fail(CSE_ERR_INVALID, "null descriptor");
  if (d->abi_version != CSE_ABI_VERSION)
    return Fail(CSE_ERR_INVALID, "abi_version mismatch: descriptor " +
                                     std::to_string(d->abi_version) + ", library " +
                                     std::to_string(CSE_ABI_VERSION));
  if (d->num_groups < 0 || (d->num_groups > 0 && !d->groups))
    return Fail(CSE_ERR_INVALID, "bad groups");
  if (d->num_parameter_blocks < 0 || (d->num_parameter_blocks > 0 && !d->parameter_blocks))
    return Fail(CSE_ERR_INVALID, "bad parameter blocks");
  for (int64_t b = 0; b < d->num_parameter_blocks; ++b) {
    const cse_parameter_block& pb = d->parameter_blocks[b];
    if (pb.size <= 0 || pb.tangent_size < 0 || pb.tangent_size > pb.size)
      return Fail(CSE_ERR_INVALID, "parameter block " + std::to_string(b) + " has bad size");
    const int64_t lim = pb.is_constant ? d->num_constant_parameters : d->num_parameters;
    if (pb.state_offset < 0 || pb.state_offset + pb.size > lim)
      return Fail(CSE_ERR_INVALID, "parameter block " + std::to_string(b) + " state out of range");
    if (!pb.is_constant && (pb.delta_offset < 0 ||
                            pb.delta_offset + pb.tangent_size > d->num_effective_parameters))
      return Fail(CSE_ERR_INVALID, "parameter block " + std::to_string(b) + " delta out of range");
    if (pb.plus_jacobian_offset >= 0 &&
        pb.plus_jacobian_offset + (int64_t)pb.size * pb.tangent_size > d->num_plus_jacobian_values)
      return Fail(CSE_ERR_INVALID, "parameter block " + std::to_string(b) +
                                       " plus jacobian out of range");
    if (pb.manifold != CSE_MANIFOLD_MATRIX && pb.manifold != CSE_MANIFOLD_QUATERNION_EUCLIDEAN)
      return Fail(CSE_ERR_INVALID, "parameter block " + std::to_string(b) + ": unknown manifold " +
                                       std::to_string(pb.manifold));
    if (pb.manifold == CSE_MANIFOLD_QUATERNION_EUCLIDEAN &&
        (pb.size < 4 || pb.tangent_size != pb.size - 1 || pb.plus_jacobian_offset >= 0))
      return Fail(CSE_ERR_INVALID, "parameter block " + std::to_string(b) +
                                       ": the quaternion manifold needs size >= 4, tangent_size "
                                       "size - 1 and plus_jacobian_offset -1");
  }
  if (d->num_constant_parameters > 0 && !d->constant_state)
    return Fail(CSE_ERR_INVALID, "constant_state missing");
  if (d->num_plus_jacobian_values > 0 && !d->plus_jacobians)
    return Fail(CSE_ERR_INVALID, "plus_jacobians missing");
  if (d->num_residual_blocks < 0 || !d->residual_layout)
    return Fail(CSE_ERR_INVALID, "residual_layout missing");
  return CSE_OK;
}

int ValidateLossData(const cse_problem_desc* d, const cse_options* opts) {
  for (int gi = 0; gi < d->num_groups; ++gi) {
    const cse_residual_group& g = d->groups[gi];
    if (g.loss_data_size == 0) continue;
    const std::string what = "group " + std::to_string(gi) + ": loss_data_size " +
                             std::to_string(g.loss_data_size);
    if (g.loss_data_size != 2) return Fail(CSE_ERR_INVALID, what + " is neither 0 nor 2");
    if (g.loss.kind == CSE_LOSS_USER)
      return Fail(CSE_ERR_UNSUPPORTED, what + " with the user loss kind (3): a user loss object has no per-block form");
    if (g.functor_kind >= CSE_FUNCTOR_USER_FIRST)
      return Fail(CSE_ERR_UNSUPPORTED, what + " with a user functor kind: its launch table has no "
                                              "per-block loss kernels");
    if (IsTestKind(g.functor_kind))
      return Fail(CSE_ERR_UNSUPPORTED, what + " with a test functor kind");
    if (g.loss.kind == CSE_LOSS_TRIVIAL && !g.loss.scaled)
      return Fail(CSE_ERR_INVALID, what + " with the unscaled trivial loss: nothing varies per block");
    if (opts && opts->jacobian_form == CSE_JACOBIAN_JET)
      return Fail(CSE_ERR_UNSUPPORTED, what + " with the Jet jacobian_form: the Jet kernels have no "
                                              "per-block loss form");
  }
  return CSE_OK;
}

int ValidateGroups(const cse_problem_desc* d, UserLookup lookup, ProgramPlan* P,
                   const cse_options* opts) {
  *P = ProgramPlan{};
  if (const int rc = ValidateLossData(d, opts)) return rc;
  P->has_layout = d->jacobian_per_residual_layout && d->jacobian_per_residual_offsets;
  P->shapes.resize((size_t)d->num_groups);
  P->users.assign((size_t)d->num_groups, nullptr);
  P->user_names.resize((size_t)d->num_groups);
  P->owner.assign((size_t)d->num_parameter_blocks, -1);
  int64_t covered_res = 0, covered_jac = 0;
  std::vector<char> seen((size_t)d->num_parameter_blocks, 0);
  for (int gi = 0; gi < d->num_groups; ++gi) {
    const cse_residual_group& g = d->groups[gi];
    KindShape& k = P->shapes[gi];
    const cse_functor_ops* user =
        lookup && g.functor_kind >= 0 ? lookup(g.functor_kind, &P->user_names[gi]) : nullptr;
    if (g.functor_kind < 0 || !ShapeOf(g.functor_kind, user, &k))
      return Fail(CSE_ERR_UNSUPPORTED, "unknown functor kind " + std::to_string(g.functor_kind));
    if (g.loss.kind < CSE_LOSS_TRIVIAL || g.loss.kind > CSE_LOSS_USER)
      return Fail(CSE_ERR_UNSUPPORTED, "unknown loss kind " + std::to_string(g.loss.kind));
    if (IsTestKind(g.functor_kind) && (g.loss.kind != CSE_LOSS_TRIVIAL || g.loss.scaled))
      return Fail(CSE_ERR_UNSUPPORTED, "test functor kinds take the trivial loss only");
    P->users[gi] = user;
    if (user) {
      // The kernels of a user kind apply the loss they were built with
      // (AutoDiffResidualBlockCUDAEvaluator<F, LossFunctionCUDA, ...>).
      if (g.loss.kind != user->loss_kind)
        return Fail(CSE_ERR_INVALID, "group " + std::to_string(gi) + ": user functor kind " +
                                         P->user_names[gi] + " was registered with loss kind " +
                                         std::to_string(user->loss_kind) + ", the group has " +
                                         std::to_string(g.loss.kind));
    } else if (g.loss.kind == CSE_LOSS_USER) {
      return Fail(CSE_ERR_INVALID, "the user loss kind (3) needs a user functor kind registered with it");
    }
    if (g.num_blocks < 0 || (g.num_blocks > 0 && (!g.parameter_block_ids || !g.functor_data)))
      return Fail(CSE_ERR_INVALID, "group " + std::to_string(gi) + " arrays missing");
    for (int64_t i = 0; i < g.num_blocks; ++i) {
      const int64_t gidx = BlockIndex(g, i);
      if (gidx < 0 || gidx >= d->num_residual_blocks)
        return Fail(CSE_ERR_INVALID, "residual block index out of range in group " + std::to_string(gi));
      if (d->residual_layout[gidx] < 0 || d->residual_layout[gidx] + k.nr > d->num_residuals)
        return Fail(CSE_ERR_INVALID, "residual_layout out of range");
      covered_res += k.nr;
      for (int j = 0; j < k.nb; ++j) {
        const int32_t id = g.parameter_block_ids[i * k.nb + j];
        if (id < 0 || id >= d->num_parameter_blocks)
          return Fail(CSE_ERR_INVALID, "parameter block id out of range in group " + std::to_string(gi));
        const int want = k.sz[j];
        const cse_parameter_block& pb = d->parameter_blocks[id];
        if (pb.size != want)
          return Fail(CSE_ERR_INVALID, "parameter block size does not match the functor");
        if (!pb.is_constant) covered_jac += (int64_t)k.nr * pb.tangent_size;
        const int32_t tag = 2 * gi + j;
        if (P->owner[id] == -1) P->owner[id] = tag;
        else if (P->owner[id] != tag) P->owner[id] = -2;
        if (!seen[id]) {
          seen[id] = 1;
          P->bytes_jac += 8LL * pb.size;
          P->bytes_res += 8LL * pb.size;
        }
      }
      if (P->has_layout) {
        const int64_t base = d->jacobian_per_residual_layout[gidx];
        int na = 0;
        for (int j = 0; j < k.nb; ++j)
          if (!d->parameter_blocks[g.parameter_block_ids[i * k.nb + j]].is_constant) ++na;
        if (base < 0 || base + (int64_t)na * k.nr > d->num_jacobian_per_residual_offsets)
          return Fail(CSE_ERR_INVALID, "jacobian_per_residual_layout out of range");
        int a = 0;
        for (int j = 0; j < k.nb; ++j) {
          const cse_parameter_block& pb = d->parameter_blocks[g.parameter_block_ids[i * k.nb + j]];
          if (pb.is_constant) continue;
          for (int r = 0; r < k.nr; ++r) {
            const int64_t off = d->jacobian_per_residual_offsets[base + a * k.nr + r];
            if (off < 0 || off + pb.tangent_size > d->num_jacobian_values)
              return Fail(CSE_ERR_INVALID, "jacobian offset out of range");
          }
          ++a;
        }
      }
    }
    const int64_t per_block = 8LL * (k.data + g.loss_data_size) + 4LL * k.nb + 8LL * k.nr;
    P->bytes_res += per_block * g.num_blocks;
    P->bytes_jac += per_block * g.num_blocks;
  }
  P->bytes_jac += 8LL * covered_jac;
  P->res_covered = covered_res == d->num_residuals;
  P->jac_covered = covered_jac == d->num_jacobian_values;
  return CSE_OK;
}

// CameraGradientKernel's passes: its point gathers (slot 1, a table of
// 8 s1 bytes per point) hit the Infinity Cache only while the table plus
// every byte streamed between two uses of a line fits in ~256 MiB
// (MI355X_MICROARCH.md, Infinity Cache).  In camera order a point's blocks
// are spread over the whole launch, between which the sorted functor data
// and slot-1 ids (8 data + 4 bytes a block) stream by: 107 + 580 MB at
// problem-13682.  Cut into passes of consecutive point ranges, taken one
// after the other, each pass touches 1/passes of both: passes = the total
// over kCamGradPassBytes, at most 64.  (Passes 8 times finer dealt to the
// XCDs measured no faster.)  The camera sums over written contributions
// (gradient_mode 3, the Schur and CGNR operators' F^T u) take the same
// plan's chunks pass-major too (GradientContribKernel's order).
constexpr double kCamGradPassBytes = 96e6;
int CamGradPasses(const cse_residual_group& g, const KindShape& k) {
  int32_t lo = INT32_MAX, hi = INT32_MIN;
  for (int64_t i = 0; i < g.num_blocks; ++i) {
    lo = std::min(lo, g.parameter_block_ids[i * k.nb + 1]);
    hi = std::max(hi, g.parameter_block_ids[i * k.nb + 1]);
  }
  if (g.num_blocks == 0) return 1;
  const double bytes = 8.0 * k.s1 * ((double)hi - lo + 1) + (8.0 * k.data + 4.0) * g.num_blocks;
  const int p = (int)std::ceil(bytes / kCamGradPassBytes);
  return std::max(1, std::min(64, p));
}

// Blocks of slot j listed per parameter block (stable counting sort): the
// gradient post-pass sums each parameter block's blocks in this order.
// cpb (may be null): the descriptor's parameter blocks; blocks whose slot-j
// parameter block is constant are left out (a held camera has no gradient
// row), which makes the plan a permutation of the other blocks only.
// passes > 1 (slot 0 of a two-slot kind): each parameter block's list is
// further ordered by pass, pass(i) = i * passes / n (block order: in a
// Schur-ordered problem, consecutive point ranges), and no chunk straddles
// two passes; chunk_order lists the chunks pass-major, the order in which
// CameraGradientKernel takes them (CamGradPasses).
void BuildGradPlan(const cse_residual_group& g, const KindShape& k, int j, GradPlanInfo* plan,
                   GradTables* tables, const cse_parameter_block* cpb, int passes) {
  const int64_t n = g.num_blocks;
  *plan = GradPlanInfo{};
  *tables = GradTables{};
  if (passes < 1 || n < passes) passes = 1;
  auto skip = [&](int64_t i) {
    return cpb && cpb[g.parameter_block_ids[i * k.nb + j]].is_constant;
  };
  auto pass_of = [&](int64_t i) { return (int)((__int128)i * passes / n); };
  int32_t lo = g.parameter_block_ids[j], hi = lo;
  for (int64_t i = 0; i < n; ++i) {
    lo = std::min(lo, g.parameter_block_ids[i * k.nb + j]);
    hi = std::max(hi, g.parameter_block_ids[i * k.nb + j]);
  }
  const int64_t count = (int64_t)hi - lo + 1;
  // Counting sort on (parameter block, pass): poff[p * passes + t].
  std::vector<int64_t> poff(count * passes + 1, 0);
  bool sorted = true;
  int64_t kept = 0, prev = INT64_MIN;
  for (int64_t i = 0; i < n; ++i) {
    if (skip(i)) {
      sorted = false;  // a permutation of the kept blocks, never the identity
      continue;
    }
    const int32_t id = g.parameter_block_ids[i * k.nb + j];
    ++poff[(id - lo) * passes + pass_of(i) + 1];
    if (id < prev) sorted = false;
    prev = id;
    ++kept;
  }
  plan->nperm = kept;
  for (int64_t p = 0; p < count * passes; ++p) poff[p + 1] += poff[p];
  std::vector<int64_t>& off = tables->off;
  off.resize(count + 1);
  for (int64_t p = 0; p <= count; ++p) off[p] = poff[p * passes];
  plan->all_present = true;
  for (int64_t p = 0; p < count && plan->all_present; ++p) plan->all_present = off[p + 1] > off[p];
  plan->sorted = sorted;
  plan->lo = lo;
  plan->count = count;
  plan->wave = !sorted && n >= 32 * count;  // on average 32+ blocks per parameter block
  if (!sorted) {
    std::vector<int32_t>& perm = tables->perm;
    perm.resize(std::max<int64_t>(kept, 1));
    std::vector<int64_t> next(poff.begin(), poff.end() - 1);
    for (int64_t i = 0; i < n; ++i)
      if (!skip(i))
        perm[next[(g.parameter_block_ids[i * k.nb + j] - lo) * passes + pass_of(i)]++] = (int32_t)i;
    // Chunks: the wave-mode post-pass and the fused gradient's slot-0 pass.
    std::vector<int64_t>& begin = tables->chunk_begin;
    std::vector<int64_t>& coff = tables->chunk_off;
    std::vector<int32_t>& chunk_pb = tables->chunk_pb;
    std::vector<int32_t> cpass;
    coff.assign(count + 1, 0);
    for (int64_t p = 0; p < count; ++p) {
      coff[p] = (int64_t)begin.size();
      for (int t = 0; t < passes; ++t)
        for (int64_t q = poff[p * passes + t]; q < poff[p * passes + t + 1]; q += kGradChunk) {
          begin.push_back(q);
          chunk_pb.push_back((int32_t)(lo + p));
          cpass.push_back(t);
        }
    }
    coff[count] = (int64_t)begin.size();
    plan->nchunks = (int64_t)begin.size();
    plan->passes = passes;
    if (passes > 1) {  // pass-major launch order, camera order within a pass
      std::vector<int32_t>& order = tables->chunk_order;
      order.reserve(begin.size());
      for (int t = 0; t < passes; ++t)
        for (int64_t c = 0; c < plan->nchunks; ++c)
          if (cpass[c] == t) order.push_back((int32_t)c);
    }
    // Chunk c covers [begin[c], begin[c + 1]): a parameter block's last
    // chunk ends at off[p + 1], where the next non-empty one starts.
    begin.push_back(kept);
  }
  plan->ready = true;
}

namespace {

// Is the group table-free?  Returns the Policy (see evaluate_kernel.hpp
// for the two affine shapes) and fills G's affine parameters; with constant
// slot-0 blocks also T->fbase.
int DetectAffine(const cse_problem_desc* d, const cse_residual_group& g, const KindShape& k,
                 GroupPlan* G, GroupTables* T) {
  const int64_t n = g.num_blocks;
  if (n == 0) return kTable;
  // The affine kernels take one or two slots, at most three residuals; a
  // user kind has them only for the shapes its header instantiates.
  if (k.nb > 2 || k.nr > 3 || IsTestKind(g.functor_kind)) return kTable;
  if (G->user && !UserAffine(G->user)) return kTable;
  auto gidx = [&](int64_t i) { return BlockIndex(g, i); };
  // Ambient sizes (state offsets) and tangent sizes (delta offsets, the
  // Jacobian's columns).  Slot 0 of the quaternion camera may be on
  // CSE_MANIFOLD_QUATERNION_EUCLIDEAN (then in every block): the kernel kind
  // becomes kKindQuaternionTangent, which builds the plus-Jacobian itself.
  const int ambient[2] = {k.s0, k.s1};
  int sizes[2] = {k.s0, k.s1};
  int manifold[2] = {CSE_MANIFOLD_MATRIX, CSE_MANIFOLD_MATRIX};
  // The first block whose slot j is active (bases and the manifold come from it).
  int64_t first[2] = {-1, -1};
  for (int64_t i = 0; i < n && (first[0] < 0 || (k.nb > 1 && first[1] < 0)); ++i)
    for (int j = 0; j < k.nb; ++j)
      if (first[j] < 0 && !d->parameter_blocks[g.parameter_block_ids[i * k.nb + j]].is_constant)
        first[j] = i;
  for (int j = 0; j < k.nb; ++j)
    if (first[j] < 0) return kTable;
  if (g.functor_kind == CSE_FUNCTOR_SNAVELY_QUATERNION_2_10_3 &&
      d->parameter_blocks[g.parameter_block_ids[first[0] * k.nb]].manifold ==
          CSE_MANIFOLD_QUATERNION_EUCLIDEAN) {
    manifold[0] = CSE_MANIFOLD_QUATERNION_EUCLIDEAN;
    sizes[0] = k.s0 - 1;
  }
  G->slot0_manifold = manifold[0];
  // Constant slot-0 blocks (a held camera) are allowed for the kinds with the
  // constant-aware kernels (the 9-column cameras, cse::ShippedTuneC0).
  const bool const0_ok = k.nb == 2 && (g.functor_kind == CSE_FUNCTOR_SNAVELY_2_9_3 ||
                                       manifold[0] == CSE_MANIFOLD_QUATERNION_EUCLIDEAN);
  // Parameters: active (slot 0 may be constant, above), no explicit
  // plus-Jacobian, state/delta offsets affine in the id.
  for (int j = 0; j < k.nb; ++j) {
    const int32_t id0 = g.parameter_block_ids[first[j] * k.nb + j];
    const cse_parameter_block& pb0 = d->parameter_blocks[id0];
    G->state_base[j] = pb0.state_offset - (int64_t)ambient[j] * id0;
    G->delta_base[j] = pb0.delta_offset - (int64_t)sizes[j] * id0;
  }
  // With constant slot-0 blocks the active ones need not be affine either
  // (a held camera in the middle shifts the later ones' offsets): their values
  // come through the repacked table, their gradient rows through a table.
  G->const0 = false;
  for (int64_t i = 0; i < n && !G->const0; ++i)
    G->const0 = d->parameter_blocks[g.parameter_block_ids[i * k.nb]].is_constant != 0;
  if (G->const0 && !const0_ok) return kTable;
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < k.nb; ++j) {
      const int32_t id = g.parameter_block_ids[i * k.nb + j];
      const cse_parameter_block& pb = d->parameter_blocks[id];
      if (pb.is_constant) {
        if (j != 0 || pb.size != ambient[0]) return kTable;
        continue;
      }
      if (pb.plus_jacobian_offset >= 0 || pb.manifold != manifold[j] ||
          pb.tangent_size != sizes[j] || pb.size != ambient[j])
        return kTable;
      if (j == 0 && G->const0) continue;
      if (pb.state_offset != G->state_base[j] + (int64_t)ambient[j] * id) return kTable;
      if (pb.delta_offset != G->delta_base[j] + (int64_t)sizes[j] * id) return kTable;
    }
  // Slot-0 id range (the repacked table of the cooperative gather).
  int32_t lo = g.parameter_block_ids[0], hi = lo;
  for (int64_t i = 0; i < n; ++i) {
    lo = std::min(lo, g.parameter_block_ids[i * k.nb]);
    hi = std::max(hi, g.parameter_block_ids[i * k.nb]);
  }
  G->slot0_lo = lo;
  G->slot0_count = (int64_t)hi - lo + 1;
  G->slot0_stride = (sizes[0] + 1) & ~1;  // per-block slot-0 gradient contributions
  G->packed_stride = PackedRowDoubles(ambient[0]);
  // Residuals.
  G->res_base = d->residual_layout[gidx(0)];
  for (int64_t i = 0; i < n; ++i)
    if (d->residual_layout[gidx(i)] != G->res_base + (int64_t)k.nr * i) return kTable;
  // Jacobian rows.
  if (!d->jacobian_per_residual_layout || !d->jacobian_per_residual_offsets) return kAffinePacked;
  const int64_t* L = d->jacobian_per_residual_layout;
  const int64_t* O = d->jacobian_per_residual_offsets;
  if (G->const0) {
    const int NR = k.nr, S0 = sizes[0], S1 = sizes[1];
    auto act = [&](int64_t i) {
      return !d->parameter_blocks[g.parameter_block_ids[i * k.nb]].is_constant;
    };
    const int64_t nchunks = (n + kWave - 1) / kWave;
    // BlockSparseMatrix: the E (slot 1) cells affine, kR x S1 packed at
    // e0 + kR*S1*i; the F cells of the blocks with an active camera packed in
    // block order from f0 (a constant camera has none; its block's first
    // active entries are the E rows).  Per chunk of 64 blocks: its first F
    // cell, then the end of the F cells.
    auto try_bsm = [&]() -> bool {
      const int64_t f0 = O[L[gidx(first[0])]];
      const int64_t e0 = O[L[gidx(0)] + (act(0) ? NR : 0)];
      std::vector<int64_t> fb;
      fb.reserve((size_t)nchunks + 1);
      int64_t rank = 0;
      for (int64_t i = 0; i < n; ++i) {
        if (i % kWave == 0) fb.push_back(f0 + (int64_t)NR * S0 * rank);
        const int64_t base = L[gidx(i)];
        int a = 0;
        if (act(i)) {
          for (int r = 0; r < NR; ++r)
            if (O[base + r] != f0 + (int64_t)NR * S0 * rank + (int64_t)r * S0) return false;
          ++rank;
          a = 1;
        }
        for (int r = 0; r < NR; ++r)
          if (O[base + a * NR + r] != e0 + (int64_t)NR * S1 * i + (int64_t)r * S1) return false;
      }
      for (int r = 0; r < NR; ++r) {
        G->jac_base[0][r] = f0 + (int64_t)r * S0;
        G->jac_base[1][r] = e0 + (int64_t)r * S1;
      }
      G->jac_stride[0] = (int64_t)NR * S0;
      G->jac_stride[1] = (int64_t)NR * S1;
      fb.push_back(f0 + (int64_t)NR * S0 * rank);
      T->fbase = std::move(fb);
      return true;
    };
    // CompressedRowSparseMatrix (compressed_row_jacobian_writer.cc:145-185):
    // every block's rows packed in block order, NR x (S0 + S1) with an active
    // camera (camera and point at fixed columns of the row) and NR x S1 with
    // a held one (the point alone).  Per chunk: the offset of its first row,
    // then the end.
    auto try_crs = [&]() -> bool {
      const int N = S0 + S1;
      const int64_t b0 = L[gidx(first[0])];
      const int64_t cam0 = O[b0], pt0 = O[b0 + NR];
      const int64_t rb0 = std::min(cam0, pt0);
      const int camcol = (int)(cam0 - rb0), ptcol = (int)(pt0 - rb0);
      if (!((camcol == 0 && ptcol == S0) || (ptcol == 0 && camcol == S1))) return false;
      const int64_t r0 = rb0 - (int64_t)NR * S1 * first[0];
      std::vector<int64_t> cb;
      cb.reserve((size_t)nchunks + 1);
      int64_t pos = r0;
      for (int64_t i = 0; i < n; ++i) {
        if (i % kWave == 0) cb.push_back(pos);
        const int64_t base = L[gidx(i)];
        if (act(i)) {
          for (int r = 0; r < NR; ++r)
            if (O[base + r] != pos + (int64_t)r * N + camcol ||
                O[base + NR + r] != pos + (int64_t)r * N + ptcol)
              return false;
          pos += (int64_t)NR * N;
        } else {
          for (int r = 0; r < NR; ++r)
            if (O[base + r] != pos + (int64_t)r * S1) return false;
          pos += (int64_t)NR * S1;
        }
      }
      cb.push_back(pos);
      for (int r = 0; r < NR; ++r) {
        G->jac_base[0][r] = r0 + (int64_t)r * N + camcol;
        G->jac_base[1][r] = r0 + (int64_t)r * N + ptcol;
      }
      G->jac_stride[0] = G->jac_stride[1] = (int64_t)NR * N;
      T->fbase = std::move(cb);
      return true;
    };
    if (try_bsm()) return kAffinePacked;
    if (try_crs()) return kAffineCrs;
    return kTable;
  }
  for (int j = 0; j < k.nb; ++j)
    for (int r = 0; r < k.nr; ++r) G->jac_base[j][r] = O[L[gidx(0)] + j * k.nr + r];
  for (int j = 0; j < k.nb; ++j)
    G->jac_stride[j] = n > 1 ? O[L[gidx(1)] + j * k.nr] - G->jac_base[j][0] : (int64_t)k.nr * sizes[j];
  for (int64_t i = 0; i < n; ++i)
    for (int j = 0; j < k.nb; ++j)
      for (int r = 0; r < k.nr; ++r)
        if (O[L[gidx(i)] + j * k.nr + r] != G->jac_base[j][r] + G->jac_stride[j] * i) return kTable;
  const int N = sizes[0] + sizes[1];
  // Shape 1: packed cells (BlockSparseMatrix).
  bool packed = true;
  for (int j = 0; j < k.nb; ++j) {
    if (G->jac_stride[j] != (int64_t)k.nr * sizes[j]) packed = false;
    for (int r = 0; r < k.nr; ++r)
      if (G->jac_base[j][r] != G->jac_base[j][0] + (int64_t)r * sizes[j]) packed = false;
  }
  if (packed && !(G->jac_stride[0] == (int64_t)k.nr * N && k.nb > 1)) return kAffinePacked;
  // Shape 2: interleaved rows (CompressedRowSparseMatrix): every slot has
  // stride kR*N, row r of the block starts at row0 + r*N and each slot sits
  // at a fixed column position inside the row, the slots tiling [0, N).
  int64_t row0 = G->jac_base[0][0];
  for (int j = 0; j < k.nb; ++j) row0 = std::min(row0, G->jac_base[j][0]);
  bool cover[32] = {false};
  for (int j = 0; j < k.nb; ++j) {
    if (G->jac_stride[j] != (int64_t)k.nr * N) return kTable;
    const int64_t col = G->jac_base[j][0] - row0;
    if (col < 0 || col + sizes[j] > N) return kTable;
    for (int c = 0; c < sizes[j]; ++c) {
      if (cover[col + c]) return kTable;
      cover[col + c] = true;
    }
    for (int r = 0; r < k.nr; ++r)
      if (G->jac_base[j][r] != row0 + (int64_t)r * N + col) return kTable;
  }
  return kAffineCrs;
}

// The tables of a group with constant slot-0 blocks: per id of the slot-0
// range its active bit, repack source and delta offset, and per chunk the
// previous chunk with F cells (BSM) or row blocks (CRS).
void BuildConst0Tables(const cse_problem_desc* d, const GroupPlan& G, GroupTables* T) {
  const KindShape& k = G.shape;
  T->bits.assign((size_t)((G.slot0_count + 31) / 32), 0u);
  T->src.assign((size_t)G.slot0_count, 0);
  T->dlt.assign((size_t)G.slot0_count, -1);
  // Ids in the range that are not camera-sized rows in bounds (blocks no
  // block of the group uses) repack the first active camera (never read).
  const int64_t fallback = G.state_base[0] + (int64_t)k.x0 * G.slot0_lo;  // overwritten below
  int64_t first_active = -1;
  for (int64_t q = 0; q < G.slot0_count && first_active < 0; ++q) {
    const cse_parameter_block& pb = d->parameter_blocks[G.slot0_lo + q];
    if (!pb.is_constant && pb.size == k.x0) first_active = pb.state_offset;
  }
  for (int64_t q = 0; q < G.slot0_count; ++q) {
    const cse_parameter_block& pb = d->parameter_blocks[G.slot0_lo + q];
    const bool fits = pb.size == k.x0 && pb.state_offset >= 0 &&
                      pb.state_offset + k.x0 <= (pb.is_constant ? d->num_constant_parameters
                                                                : d->num_parameters);
    if (!fits) {
      T->src[q] = first_active >= 0 ? first_active : fallback;
    } else if (pb.is_constant) {
      T->src[q] = -1 - pb.state_offset;
    } else {
      T->bits[q >> 5] |= 1u << (q & 31);
      T->src[q] = pb.state_offset;
      T->dlt[q] = pb.delta_offset;
    }
  }
  if (!T->fbase.empty()) {
    const int64_t nchunks = (int64_t)T->fbase.size() - 1;
    T->prev_seg.assign((size_t)nchunks, -1);
    int32_t last = -1;
    for (int64_t c = 0; c < nchunks; ++c) {
      T->prev_seg[c] = last;
      if (T->fbase[c + 1] > T->fbase[c]) last = (int32_t)c;
    }
  }
}

// A table group whose slot-0 blocks are all plain: active, no manifold
// (plus_jacobian_offset -1), tangent size = size = the kind's, state and
// delta offsets affine in the id.  EvaluateTableKernel then forms their PbDev
// records instead of loading them: one cache line less per lane for a
// camera-like slot 0, whose lines the point stream evicts from L2 between
// uses.
void DetectPlain0(const cse_problem_desc* d, const cse_residual_group& g, GroupPlan* G) {
  const KindShape& k = G->shape;
  G->plain0 = false;
  if (G->affine || G->n == 0) return;
  const int S = k.sz[0];
  const int32_t id0 = g.parameter_block_ids[0];
  const int64_t sb = d->parameter_blocks[id0].state_offset - (int64_t)S * id0;
  const int64_t db = d->parameter_blocks[id0].delta_offset - (int64_t)S * id0;
  for (int64_t i = 0; i < G->n; ++i) {
    const int32_t id = g.parameter_block_ids[i * k.nb];
    const cse_parameter_block& p = d->parameter_blocks[id];
    if (p.is_constant || p.manifold != CSE_MANIFOLD_MATRIX || p.plus_jacobian_offset != -1 ||
        p.size != S || p.tangent_size != S || p.state_offset != sb + (int64_t)S * id ||
        p.delta_offset != db + (int64_t)S * id)
      return;
  }
  G->plain0 = true;
  G->plain0_state_base = sb;
  G->plain0_delta_base = db;
  // A plain slot 0 of a small id range (the cameras) is read from a
  // repacked copy, as the affine kernels read it (RepackSlot0Kernel, every
  // evaluation): one 128-byte row a lane instead of its values at an
  // 8-byte alignment.
  int32_t lo = INT32_MAX, hi = INT32_MIN;
  for (int64_t i = 0; i < g.num_blocks; ++i) {
    lo = std::min(lo, g.parameter_block_ids[i * k.nb]);
    hi = std::max(hi, g.parameter_block_ids[i * k.nb]);
  }
  const int64_t count = (int64_t)hi - lo + 1;
  if (k.sz[0] <= 16 && count <= (1 << 20)) {
    G->repack0 = true;
    G->slot0_lo = lo;
    G->slot0_count = count;
    G->packed_stride = PackedRowDoubles(k.sz[0]);
    G->state_base[0] = G->plain0_state_base;
  }
}

// The general kernel's store runs, found once per 64-block chunk (the
// wave's blocks) by the tests TableStores makes on the device: flags
// kTableRunFlagResiduals when the chunk's residuals are one run (NR apart),
// kTableRunFlagBsm / Crs when every slot is active in all or none of its
// blocks with one tangent size and its Jacobian rows form BlockSparseMatrix
// cell runs / CompressedRow row blocks; then the residual run's start and
// each active slot's first row.  [chunks][2 + nb]; shapes the kernel stages
// (kTableStaged: NR x N <= 32) only.
void BuildTableRuns(const cse_problem_desc* d, const cse_residual_group& g, const GroupPlan& G,
                    bool has_layout, std::vector<int64_t>* out) {
  const KindShape& k = G.shape;
  int N = 0;
  for (int j = 0; j < k.nb; ++j) N += k.sz[j];
  if (G.affine || G.n == 0 || k.nr * N > 32) return;
  const int NB = k.nb, NR = k.nr, W = 2 + NB;
  const int64_t n = G.n, nch = (n + kWave - 1) / kWave;
  std::vector<int64_t>& runs = *out;
  runs.assign((size_t)(nch * W), 0);
  auto gidx = [&](int64_t i) { return BlockIndex(g, i); };
  auto pb = [&](int64_t i, int j) -> const cse_parameter_block& {
    return d->parameter_blocks[g.parameter_block_ids[i * NB + j]];
  };
  for (int64_t c = 0; c < nch; ++c) {
    const int64_t i0 = c * kWave;
    const int nb = (int)std::min<int64_t>(kWave, n - i0);
    int64_t* R = &runs[(size_t)(c * W)];
    const int64_t off0 = d->residual_layout[gidx(i0)];
    bool rr = true;
    for (int l = 1; rr && l < nb; ++l) rr = d->residual_layout[gidx(i0 + l)] == off0 + (int64_t)NR * l;
    if (rr) {
      R[0] |= kTableRunFlagResiduals;
      R[1] = off0;
    }
    if (!has_layout) continue;
    bool cst[CSE_MAX_PARAMETER_BLOCKS];
    int t[CSE_MAX_PARAMETER_BLOCKS];
    bool uniform = true;
    for (int j = 0; j < NB; ++j) {
      cst[j] = pb(i0, j).is_constant != 0;
      t[j] = pb(i0, j).tangent_size;
      for (int l = 1; uniform && l < nb; ++l) {
        const cse_parameter_block& p = pb(i0 + l, j);
        uniform = (p.is_constant != 0) == cst[j] && (cst[j] || p.tangent_size == t[j]);
      }
    }
    if (!uniform) continue;
    // Row (j, kk) of lane l: offsets[layout[gidx] + a NR + kk], a = slot j's
    // position among the active slots.
    auto row = [&](int l, int a, int kk) {
      return d->jacobian_per_residual_offsets[d->jacobian_per_residual_layout[gidx(i0 + l)] + (int64_t)a * NR + kk];
    };
    int64_t base[CSE_MAX_PARAMETER_BLOCKS] = {0};
    int64_t r0 = INT64_MAX;
    int w = 0, a = 0;
    for (int j = 0; j < NB; ++j) {
      if (cst[j]) continue;
      base[j] = row(0, a++, 0);
      r0 = std::min(r0, base[j]);
      w += t[j];
    }
    bool bsm = true, crs = true;
    a = 0;
    for (int j = 0; j < NB; ++j) {
      if (cst[j]) continue;
      for (int l = 0; l < nb && (bsm || crs); ++l)
        for (int kk = 0; kk < NR; ++kk) {
          const int64_t v = row(l, a, kk);
          bsm = bsm && v == base[j] + (int64_t)l * NR * t[j] + (int64_t)kk * t[j];
          crs = crs && v == base[j] + (int64_t)l * NR * w + (int64_t)kk * w;
        }
      ++a;
      const int64_t cj = base[j] - r0;
      crs = crs && cj >= 0 && cj + t[j] <= w;
      for (int j2 = 0; j2 < j; ++j2) {
        if (cst[j2]) continue;
        const int64_t c2 = base[j2] - r0;
        crs = crs && (cj + t[j] <= c2 || c2 + t[j2] <= cj);
      }
    }
    R[0] |= (bsm ? kTableRunFlagBsm : 0) | (crs ? kTableRunFlagCrs : 0);
    for (int j = 0; j < NB; ++j) R[2 + j] = base[j];
  }
}

// The implicit Schur complement's structure (cse_schur_*): one Snavely
// group on the fused-gradient path with the BlockSparseMatrix layout, its
// e blocks (slot 1, points) the leading columns [0, e_cols) and its f blocks
// (slot 0, cameras) the rest, as ITERATIVE_SCHUR's elimination ordering puts
// them (iterative_schur_complement_solver.cc:66-80).  The e-block runs are cut
// into wave chunks of whole runs; longer runs are listed as big.
//
// Held cameras (a const0 group; every other constant parameter is refused): a
// block whose camera is held has an E cell and no F cell, the F cells of the
// other blocks are packed in block order, and the active cameras of the id
// range must tile [e_cols, num_effective) in id order, 9 columns each -- the
// f vector then has 9 entries per active camera, by rank.  The plan adds the
// tables that turn a block into its F cell and a camera id into its rank
// (ProgramPlan::schur_chunk_held and the others); T = the group's tables, for
// the slot-0 gradient plan's perm.
void BuildSchurPlan(const cse_problem_desc* d, const GroupPlan* only, const GroupTables* T,
                    ProgramPlan* P) {
  SchurPlan& S = P->schur;
  S = SchurPlan{};
  if (!only || d->num_groups != 1) return;
  const GroupPlan& G = *only;
  if (!G.fuse_ok || G.policy != kAffinePacked || !SnavelyShaped(G.shape) || !P->has_layout) return;
  const bool held = G.const0;
  if (held ? T == nullptr : d->num_constant_parameters > 0) return;
  const cse_residual_group& g = d->groups[0];
  const int32_t* ids = g.parameter_block_ids;
  const int64_t n = g.num_blocks;
  int32_t pmin = ids[1], pmax = ids[1], cmin = ids[0], cmax = ids[0];
  for (int64_t i = 0; i < n; ++i) {
    pmin = std::min(pmin, ids[2 * i + 1]);
    pmax = std::max(pmax, ids[2 * i + 1]);
    cmin = std::min(cmin, ids[2 * i]);
    cmax = std::max(cmax, ids[2 * i]);
  }
  const int64_t e_lo = G.delta_base[1] + 3LL * pmin, e_hi = G.delta_base[1] + 3LL * pmax + 3;
  std::vector<int32_t> cam_rank;
  if (held) {
    if (e_lo != 0) return;
    // The chunk kernel moves F and E cells in 16-byte pieces.
    if (G.jac_base[0][0] % 2 != 0 || G.jac_base[1][0] % 2 != 0) return;
    // A constant block of the program outside the cameras' id range (a held
    // point, a block no residual uses) is not this structure.
    int64_t constant = 0;
    for (int64_t b = 0; b < d->num_parameter_blocks; ++b)
      if (d->parameter_blocks[b].is_constant && (b < cmin || b > cmax)) ++constant;
    if (constant > 0) return;
    const GradPlanInfo& I = T->grad_info[0];
    if (!I.ready || I.lo != cmin || I.count != (int64_t)cmax - cmin + 1) return;
    cam_rank.assign((size_t)I.count, -1);
    int64_t rank = 0;
    for (int64_t q = 0; q < I.count; ++q) {
      const cse_parameter_block& pb = d->parameter_blocks[cmin + q];
      if (pb.is_constant) continue;
      if (pb.tangent_size != 9 || pb.delta_offset != e_hi + 9 * rank) return;
      cam_rank[(size_t)q] = (int32_t)rank++;
    }
    if (rank == 0 || e_hi + 9 * rank != d->num_effective_parameters) return;
    S.held = true;
    S.num_active = rank;
    S.e_cols = e_hi;
    S.f_cols = 9 * rank;
    S.f_col_base = 0;
  } else {
    const int64_t f_lo = G.delta_base[0] + 9LL * cmin, f_hi = G.delta_base[0] + 9LL * cmax + 9;
    if (e_lo < 0 || f_lo != e_hi || f_hi != d->num_effective_parameters || e_lo != 0) return;
    S.e_cols = e_hi;
    S.f_cols = f_hi - f_lo;
    S.f_col_base = G.delta_base[0] - S.e_cols;
  }
  auto active = [&](int64_t i) { return !held || cam_rank[(size_t)(ids[2 * i] - cmin)] >= 0; };
  // One pass over the runs of equal e block: small runs are packed into
  // chunks of at most a wave ([begin, end) pairs; chunks never straddle a
  // big run), big runs listed on their own.
  std::vector<int64_t>& ranges = P->schur_chunk_begin;
  std::vector<int64_t>& big = P->schur_big;
  std::vector<int32_t> cams;
  bool dup = false;
  int64_t run_start = 0, chunk_lo = 0;
  for (int64_t i = 1; i <= n; ++i) {
    if (i < n && ids[2 * i + 1] == ids[2 * (i - 1) + 1]) continue;
    const int64_t len = i - run_start;  // the run [run_start, i)
    if (held) {  // a held camera has no f block to see twice
      cams.clear();
      for (int64_t q = run_start; q < i; ++q)
        if (active(q)) cams.push_back(ids[2 * q]);
    } else {
      cams.assign(len, 0);
      for (int64_t q = 0; q < len; ++q) cams[q] = ids[2 * (run_start + q)];
    }
    std::sort(cams.begin(), cams.end());
    dup = dup || std::adjacent_find(cams.begin(), cams.end()) != cams.end();
    if (len > kWave) {
      if (run_start > chunk_lo) ranges.insert(ranges.end(), {chunk_lo, run_start});
      big.insert(big.end(), {run_start, i});
      chunk_lo = i;
    } else if (i - chunk_lo > kWave) {
      ranges.insert(ranges.end(), {chunk_lo, run_start});
      chunk_lo = run_start;
    }
    run_start = i;
  }
  if (n > chunk_lo) ranges.insert(ranges.end(), {chunk_lo, n});
  S.duplicates = dup;
  S.nchunks = (int64_t)ranges.size() / 2;
  S.nbig = (int64_t)big.size() / 2;
  if (held) {
    // before[i]: the blocks with an active camera in [0, i) = block i's F cell.
    std::vector<int32_t> before((size_t)n + 1);
    int32_t cells = 0;
    for (int64_t i = 0; i < n; ++i) {
      before[(size_t)i] = cells;
      if (active(i)) ++cells;
    }
    before[(size_t)n] = cells;
    P->schur_chunk_held.resize(ranges.size());
    for (int64_t c = 0; c < S.nchunks; ++c) {
      const int64_t i0 = ranges[2 * c], i1 = ranges[2 * c + 1];
      uint64_t mask = 0;
      for (int64_t i = i0; i < i1; ++i)
        if (active(i)) mask |= (uint64_t)1 << (i - i0);
      P->schur_chunk_held[2 * c] = before[(size_t)i0];
      P->schur_chunk_held[2 * c + 1] = (int64_t)mask;
    }
    P->schur_big_rank.resize((size_t)S.nbig);
    for (int64_t q = 0; q < S.nbig; ++q) P->schur_big_rank[(size_t)q] = before[(size_t)big[2 * q]];
    const std::vector<int32_t>& perm = T->grad[0].perm;
    const int64_t nperm = T->grad_info[0].nperm;
    if (nperm != cells || (int64_t)perm.size() < nperm) {  // not the plan of these blocks
      S = SchurPlan{};
      ranges.clear();
      big.clear();
      P->schur_chunk_held.clear();
      P->schur_big_rank.clear();
      return;
    }
    P->schur_fcell.resize((size_t)std::max<int64_t>(nperm, 1), 0);
    for (int64_t q = 0; q < nperm; ++q) P->schur_fcell[(size_t)q] = before[(size_t)perm[(size_t)q]];
    P->schur_cam_rank = std::move(cam_rank);
  }
  S.eligible = true;
}

}  // namespace

void PlanGroup(const cse_problem_desc* d, const cse_options& opts, int gi, ProgramPlan* P,
               GroupPlan* Gp, GroupTables* T) {
  const cse_residual_group& g = d->groups[gi];
  *Gp = GroupPlan{};
  *T = GroupTables{};
  GroupPlan& G = *Gp;
  G.kind = g.functor_kind;
  G.user = P->users[gi];
  G.shape = P->shapes[gi];
  G.loss = g.loss;
  G.loss_data_size = g.loss_data_size;
  G.n = g.num_blocks;
  G.first = g.first_residual_block;
  const KindShape& k = G.shape;  // follows G.shape when the kind changes below

  // ---- The policy, decided here and nowhere else.
  G.policy = opts.force_general_layout ? kTable : DetectAffine(d, g, k, &G, T);
  // Constant slot-0 blocks need the repacked table (their values come from
  // the constant state through it).
  if (G.policy != kTable && G.const0 && G.slot0_count > (1 << 20)) G.policy = kTable;
  // The Jet form of the Snavely functor (cse_options.jacobian_form) is
  // instantiated for the affine kernels with the LDS-DMA gather and without
  // held cameras, and for the table kernel: other Snavely groups take the
  // table path.
  G.jet = opts.jacobian_form == CSE_JACOBIAN_JET && g.functor_kind == CSE_FUNCTOR_SNAVELY_2_9_3;
  if (G.jet && G.policy != kTable &&
      (G.const0 || G.slot0_count <= 0 || G.slot0_count > (1 << 20)))
    G.policy = kTable;
  G.affine = G.policy != kTable;
  if (!G.affine) {
    G.const0 = false;  // DetectAffine may have set it before giving up
    T->fbase.clear();
  }
  if (G.affine && g.functor_kind == CSE_FUNCTOR_SNAVELY_QUATERNION_2_10_3 &&
      G.slot0_manifold == CSE_MANIFOLD_QUATERNION_EUCLIDEAN) {
    // Slot 0 on the quaternion manifold (DetectAffine checked every active
    // block; a held camera's own manifold is irrelevant): the kernel kind
    // with the tangent Jacobian (k follows G.shape).
    G.kind = kKindQuaternionTangent;
    ShapeOf(G.kind, nullptr, &G.shape);
  }
  // Table-path tables: also for const0 groups (their J products use the
  // table kernels).
  if (G.const0 || !G.affine) P->any_general = true;

  // ---- Workgroups; every kernel writes one cost partial per wave.
  if (G.affine) {
    const int64_t chunks = (g.num_blocks + kWave - 1) / kWave;
    G.num_wg = std::max<int64_t>(1, (chunks + kWavesPerBlock - 1) / kWavesPerBlock);
  } else {
    G.num_wg = (g.num_blocks + kBlockThreads - 1) / kBlockThreads;
  }
  G.partial_offset = P->total_wg;
  P->total_wg += G.num_wg * kWavesPerBlock;

  // The LDS-DMA gather reads slot 0 from a repacked copy refreshed every
  // evaluation; worth it while the slot-0 id range is small (BAL: the
  // cameras), otherwise gather 8-byte pieces from the state directly.
  G.repack0 = G.affine && G.slot0_count > 0 && G.slot0_count <= (1 << 20);
  if (G.const0) {
    BuildConst0Tables(d, G, T);
    if (!T->fbase.empty()) G.fbase0 = T->fbase[0];
  }
  const bool fused_kind = FusedKind(G.kind) || UserFused(G.user, k);
  if (G.affine && P->has_layout) {
    const int sizes[2] = {k.s0, k.s1};
    for (int j = 0; j < k.nb; ++j)
      if (GradSupported(k.nr, sizes[j], G.user, j))
        BuildGradPlan(g, k, j, &T->grad_info[j], &T->grad[j],
                      j == 0 && G.const0 ? d->parameter_blocks : nullptr,
                      j == 0 && k.nb == 2 && fused_kind ? CamGradPasses(g, k) : 1);
  }
  BuildTableRuns(d, g, G, P->has_layout, &T->runs);
  DetectPlain0(d, g, &G);

  // Fused gradient eligibility: a Snavely group on the affine LDS-DMA path
  // whose slot-1 blocks are sorted (identity plan) and used by no other
  // group or slot (the fused kernel stores their rows, it does not add),
  // and whose slot-0 blocks have a chunked plan.
  const GradPlanInfo* I = T->grad_info;
  bool ok = fused_kind && G.affine && G.n > 0 && G.repack0 && I[0].ready && !I[0].sorted &&
            I[0].nchunks > 0 && I[1].ready && I[1].sorted;
  for (int64_t i = 0; ok && i < g.num_blocks; ++i)
    ok = P->owner[g.parameter_block_ids[2 * i + 1]] == 2 * gi + 1;
  G.fuse_ok = ok;
  G.grad_exact = ok && d->num_groups == 1 && !G.const0 && d->num_constant_parameters == 0 &&
                 k.s1 == 3 && I[0].all_present && I[1].all_present &&
                 k.s0 * I[0].count + 3 * I[1].count == d->num_effective_parameters;
}

void PlanProgram(const cse_problem_desc* d, const GroupPlan* only, ProgramPlan* P,
                 const GroupTables* only_tables) {
  // Plus runs: active blocks sorted by state offset, merged while
  // contiguous with a constant delta shift.
  std::vector<std::pair<int64_t, int64_t>> blocks;  // (state_offset, index)
  for (int64_t b = 0; b < d->num_parameter_blocks; ++b) {
    const cse_parameter_block& pb = d->parameter_blocks[b];
    if (pb.is_constant) continue;
    if (pb.manifold == CSE_MANIFOLD_QUATERNION_EUCLIDEAN) {
      P->plus_quat.push_back({pb.state_offset, pb.delta_offset, pb.size, 0});
      continue;
    }
    if (pb.plus_jacobian_offset >= 0 || pb.tangent_size != pb.size) P->plus_supported = false;
    blocks.emplace_back(pb.state_offset, b);
  }
  std::sort(blocks.begin(), blocks.end());
  for (const auto& e : blocks) {
    const cse_parameter_block& pb = d->parameter_blocks[e.second];
    const int64_t shift = pb.state_offset - pb.delta_offset;
    auto& R = P->plus_runs;
    if (!R.empty() && R.back().state_begin + R.back().length == pb.state_offset &&
        R.back().delta_shift == shift)
      R.back().length += pb.size;
    else
      R.push_back({pb.state_offset, pb.size, shift});
  }
  BuildSchurPlan(d, only, only_tables, P);
  if (P->any_general) {
    P->pbs.resize((size_t)d->num_parameter_blocks);
    for (int64_t b = 0; b < d->num_parameter_blocks; ++b) {
      const cse_parameter_block& pb = d->parameter_blocks[b];
      const int64_t pj = pb.manifold == CSE_MANIFOLD_QUATERNION_EUCLIDEAN ? kPlusJacobianQuaternion
                                                                          : pb.plus_jacobian_offset;
      P->pbs[b] = {pb.state_offset, pb.delta_offset, pj, pb.tangent_size, pb.is_constant};
    }
  }
}

void PlanCgnrBlocks(const cse_problem_desc* d, CgnrBlockPlan* plan) {
  *plan = CgnrBlockPlan{};
  int64_t next = 0;
  bool tiles = true;
  auto add = [&](int64_t delta, int32_t size) {
    tiles = tiles && delta == next;
    auto& R = plan->runs;
    if (!R.empty() && R.back().tangent_size == size &&
        R.back().delta_offset + R.back().count * size == delta && delta == next)
      ++R.back().count;
    else
      R.push_back({delta, plan->num_values, plan->num_blocks, 1, size, 0});
    next = delta + size;
    ++plan->num_blocks;
    plan->num_values += (int64_t)size * size;
    plan->max_size = std::max(plan->max_size, (int)size);
  };
  // A program's blocks come in delta order as a rule (4.4 million at
  // problem-13682): one pass, nothing stored but the runs.
  bool sorted = true;
  int64_t last = -1;
  for (int64_t b = 0; b < d->num_parameter_blocks && sorted; ++b) {
    const cse_parameter_block& pb = d->parameter_blocks[b];
    if (pb.is_constant || pb.tangent_size <= 0) continue;
    sorted = pb.delta_offset >= last;
    last = pb.delta_offset;
    if (sorted) add(pb.delta_offset, pb.tangent_size);
  }
  if (!sorted) {
    // Out of order: the blocks are listed, sorted and run through again.
    *plan = CgnrBlockPlan{};
    next = 0;
    tiles = true;
    std::vector<std::pair<int64_t, int32_t>> all;
    for (int64_t b = 0; b < d->num_parameter_blocks; ++b) {
      const cse_parameter_block& pb = d->parameter_blocks[b];
      if (!pb.is_constant && pb.tangent_size > 0) all.emplace_back(pb.delta_offset, pb.tangent_size);
    }
    std::stable_sort(all.begin(), all.end(),
                     [](const std::pair<int64_t, int32_t>& x, const std::pair<int64_t, int32_t>& y) {
                       return x.first < y.first;
                     });
    for (const auto& e : all) add(e.first, e.second);
  }
  plan->tiles = tiles && next == d->num_effective_parameters;
  plan->fits = plan->max_size <= kCgnrMaxBlockColumns;
}

void ExpandCgnrBlocks(const CgnrBlockPlan& plan, std::vector<CgnrBlock>* blocks) {
  blocks->clear();
  blocks->reserve((size_t)plan.num_blocks);
  for (const CgnrRun& r : plan.runs) {
    const int64_t s = r.tangent_size;
    for (int64_t k = 0; k < r.count; ++k)
      blocks->push_back({r.delta_offset + k * s, r.value_offset + k * s * s, r.tangent_size, 0});
  }
}

int64_t FindCgnrBlock(const CgnrBlockPlan& plan, int64_t delta, const CgnrRun** run) {
  const auto& R = plan.runs;
  // The last run that starts at or before delta.
  auto it = std::upper_bound(R.begin(), R.end(), delta,
                             [](int64_t v, const CgnrRun& x) { return v < x.delta_offset; });
  if (it == R.begin()) return -1;
  --it;
  // Runs of equal start (overlapping blocks, no tiling): the first of them.
  while (it != R.begin() && (it - 1)->delta_offset == it->delta_offset) --it;
  const int64_t k = delta - it->delta_offset;
  if (k % it->tangent_size != 0 || k / it->tangent_size >= it->count) return -1;
  if (run) *run = &*it;
  return it->first_block + k / it->tangent_size;
}

int PlanSchurPairs(const int32_t* ids, int64_t n, bool counts_only, SchurPairPlan* plan,
                   const int32_t* cluster, int32_t first_id, const int32_t* neighbor) {
  *plan = SchurPairPlan{};
  if (n >= ((int64_t)1 << 31))
    return CseFail(CSE_ERR_UNSUPPORTED, "Schur complement plan: 2^31 or more residual blocks");
  try {
    if (!counts_only) {
      plan->pair_begin.assign(1, 0);
      plan->chunk_off.assign(1, 0);
    }
    if (n <= 0) return CSE_OK;
    int32_t cmin = ids[0], cmax = ids[0];
    for (int64_t i = 1; i < n; ++i) {
      cmin = std::min(cmin, ids[2 * i]);
      cmax = std::max(cmax, ids[2 * i]);
    }
    const int64_t C = (int64_t)cmax - cmin + 1;
    // Pass 1: pairs per block, in a dense C x C table (upper triangle used).
    std::vector<int64_t> at((size_t)(C * C), 0);
    // The filter: a block is kept when its two cameras carry one label, or
    // two labels that an edge of the forest joins.
    const int32_t* label = cluster ? cluster + ((int64_t)cmin - first_id) : nullptr;
    auto kept = [&](int64_t c, int64_t c2) {
      if (!label || label[c] == label[c2]) return true;
      return neighbor && (neighbor[2 * label[c]] == label[c2] || neighbor[2 * label[c] + 1] == label[c2]);
    };
    auto each_pair = [&](auto&& f) {
      int64_t r0 = 0;
      for (int64_t i = 1; i <= n; ++i) {
        if (i < n && ids[2 * i + 1] == ids[2 * r0 + 1]) continue;
        for (int64_t b = r0; b < i; ++b) {
          const int64_t c = ids[2 * b] - cmin;
          for (int64_t b2 = r0; b2 < i; ++b2) {
            const int64_t c2 = ids[2 * b2] - cmin;
            if (c <= c2 && kept(c, c2)) f(c * C + c2, b, b2);
          }
        }
        r0 = i;
      }
    };
    each_pair([&](int64_t cell, int64_t, int64_t) { ++at[(size_t)cell]; });
    // The blocks in lexicographic order; each cell becomes its block's cursor.
    for (int64_t c = 0; c < C; ++c) {
      for (int64_t c2 = c; c2 < C; ++c2) {
        int64_t& cell = at[(size_t)(c * C + c2)];
        if (cell == 0) continue;
        const int64_t count = cell, chunks = (count + kSchurPairChunk - 1) / kSchurPairChunk;
        cell = plan->num_pairs;
        if (!counts_only) {
          plan->block_row.push_back((int32_t)(cmin + c));
          plan->block_col.push_back((int32_t)(cmin + c2));
          plan->pair_begin.push_back(plan->num_pairs + count);
          plan->chunk_off.push_back(plan->num_chunks + chunks);
          plan->chunk_block.insert(plan->chunk_block.end(), (size_t)chunks, (int32_t)plan->num_blocks);
        }
        plan->num_blocks += 1;
        plan->num_pairs += count;
        plan->num_chunks += chunks;
      }
    }
    plan->plan_bytes = 2 * 4 * plan->num_blocks + 2 * 8 * (plan->num_blocks + 1) + 4 * plan->num_chunks +
                       2 * 4 * plan->num_pairs + 8LL * kSchurBlockDoubles * plan->num_chunks;
    if (counts_only) return CSE_OK;
    // Pass 2: the runs again in the same order, so a block's pairs come out
    // ordered by (e block, b, b').
    plan->pairs.resize((size_t)(2 * plan->num_pairs));
    each_pair([&](int64_t cell, int64_t b, int64_t b2) {
      const int64_t k = at[(size_t)cell]++;
      plan->pairs[(size_t)(2 * k)] = (int32_t)b;
      plan->pairs[(size_t)(2 * k + 1)] = (int32_t)b2;
    });
  } catch (const std::bad_alloc&) {
    *plan = SchurPairPlan{};
    return CseFail(CSE_ERR_OOM, "Schur complement plan: host allocation failed");
  }
  return CSE_OK;
}

int PlanSchurSparse(const int32_t* ids, int64_t n, const SchurPairPlan& plan, int32_t first_id, int64_t C,
                    bool counts_only, SchurSparsePlan* sparse) {
  *sparse = SchurSparsePlan{};
  if (C < 0) return CseFail(CSE_ERR_INVALID, "block-sparse Schur complement: negative camera count");
  try {
    std::vector<bool> seen((size_t)C, false);
    int64_t observed = 0;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t c = (int64_t)ids[2 * i] - first_id;
      if (c < 0 || c >= C)
        return CseFail(CSE_ERR_INVALID, "block-sparse Schur complement: an f block outside the cameras");
      if (!seen[(size_t)c]) ++observed;
      seen[(size_t)c] = true;
    }
    const int64_t added = C - observed;
    sparse->num_block_rows = C;
    sparse->num_blocks = plan.num_blocks + added;
    if (sparse->num_blocks >= ((int64_t)1 << 31))
      return CseFail(CSE_ERR_UNSUPPORTED, "block-sparse Schur complement: 2^31 or more blocks");
    // A block of q chunks has q - 1 beyond its first: at most num_chunks -
    // num_blocks blocks have several.
    sparse->finish_capacity = plan.num_chunks - plan.num_blocks + added;
    sparse->device_bytes = 2 * 8 * (C + 1) + 2 * 4 * sparse->num_blocks + 4 * plan.num_blocks +
                           4 * sparse->finish_capacity + 4 * (sparse->num_blocks - C) +
                           8 * 9 * sparse->num_blocks;
    if (counts_only) return CSE_OK;
    SchurSparsePlan& S = *sparse;
    S.row_begin.reserve((size_t)C + 1);
    S.block_col.reserve((size_t)S.num_blocks);
    S.plan_block.reserve((size_t)S.num_blocks);
    S.sparse_of_plan.assign((size_t)plan.num_blocks, -1);
    S.col_begin.assign((size_t)C + 1, 0);
    int64_t k = 0;  // the pair plan's blocks come in (row, col) order
    for (int64_t c = 0; c < C; ++c) {
      S.row_begin.push_back((int64_t)S.block_col.size());
      if (!(k < plan.num_blocks && plan.block_row[(size_t)k] - first_id == c &&
            plan.block_col[(size_t)k] - first_id == c)) {
        S.finish.push_back((int32_t)S.block_col.size());
        S.block_col.push_back((int32_t)c);
        S.plan_block.push_back(-1);
      }
      for (; k < plan.num_blocks && plan.block_row[(size_t)k] - first_id == c; ++k) {
        const int64_t c2 = (int64_t)plan.block_col[(size_t)k] - first_id;
        const int32_t at = (int32_t)S.block_col.size();
        if (plan.chunk_off[(size_t)k + 1] - plan.chunk_off[(size_t)k] != 1) S.finish.push_back(at);
        if (c2 > c) ++S.col_begin[(size_t)c2 + 1];
        S.sparse_of_plan[(size_t)k] = at;
        S.block_col.push_back((int32_t)c2);
        S.plan_block.push_back((int32_t)k);
      }
    }
    S.row_begin.push_back((int64_t)S.block_col.size());
    if (k != plan.num_blocks || (int64_t)S.block_col.size() != S.num_blocks ||
        (int64_t)S.finish.size() > S.finish_capacity)
      return CseFail(CSE_ERR_INVALID, "block-sparse Schur complement: the pair plan is not of these ids");
    for (int64_t c = 0; c < C; ++c) S.col_begin[(size_t)c + 1] += S.col_begin[(size_t)c];
    // Blocks in storage order are in ascending row order: so is each column's list.
    std::vector<int64_t> cursor(S.col_begin.begin(), S.col_begin.end() - 1);
    S.col_block.resize((size_t)(S.num_blocks - C));
    S.col_row.resize((size_t)(S.num_blocks - C));
    for (int64_t c = 0; c < C; ++c)
      for (int64_t b = S.row_begin[(size_t)c] + 1; b < S.row_begin[(size_t)c + 1]; ++b) {
        const int64_t j = cursor[(size_t)S.block_col[(size_t)b]]++;
        S.col_block[(size_t)j] = (int32_t)b;
        S.col_row[(size_t)j] = (int32_t)c;
      }
  } catch (const std::bad_alloc&) {
    *sparse = SchurSparsePlan{};
    return CseFail(CSE_ERR_OOM, "block-sparse Schur complement: host allocation failed");
  }
  return CSE_OK;
}

int ValidateSchurClusters(const int32_t* cluster, int64_t C, int32_t num_clusters) {
  if (!cluster) return CseFail(CSE_ERR_INVALID, "cluster partition: null cluster_of_camera");
  if (C < 0 || num_clusters < 0 || (C > 0 && num_clusters < 1) || num_clusters > C)
    return CseFail(CSE_ERR_INVALID, "cluster partition: num_clusters is not in [1, num_cameras]");
  try {
    std::vector<int32_t> size((size_t)num_clusters, 0);
    for (int64_t c = 0; c < C; ++c) {
      if (cluster[c] < 0 || cluster[c] >= num_clusters)
        return CseFail(CSE_ERR_INVALID, "cluster partition: camera " + std::to_string(c) + " has label " +
                                            std::to_string(cluster[c]) + ", outside [0, " +
                                            std::to_string(num_clusters) + ")");
      ++size[(size_t)cluster[c]];
    }
    for (int32_t g = 0; g < num_clusters; ++g) {
      if (size[(size_t)g] == 0)
        return CseFail(CSE_ERR_INVALID, "cluster partition: label " + std::to_string(g) + " is not used");
      if (size[(size_t)g] > kSchurMaxClusterCameras)
        return CseFail(CSE_ERR_UNSUPPORTED, "cluster partition: cluster " + std::to_string(g) + " has " +
                                                std::to_string(size[(size_t)g]) + " cameras, more than " +
                                                std::to_string(kSchurMaxClusterCameras) +
                                                " (one cluster is factored in the LDS of one workgroup)");
    }
  } catch (const std::bad_alloc&) {
    return CseFail(CSE_ERR_OOM, "cluster partition: host allocation failed");
  }
  return CSE_OK;
}

int PlanSchurClusters(const int32_t* ids, int64_t n, int32_t first_id, int64_t C, const int32_t* cluster,
                      int32_t num_clusters, bool counts_only, SchurClusterPlan* plan) {
  *plan = SchurClusterPlan{};
  int rc = ValidateSchurClusters(cluster, C, num_clusters);
  if (rc) return rc;
  try {
    std::vector<bool> seen((size_t)C, false);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t c = (int64_t)ids[2 * i] - first_id;
      if (c < 0 || c >= C) return CseFail(CSE_ERR_INVALID, "cluster plan: an f block outside the cameras");
      seen[(size_t)c] = true;
    }
    if ((rc = PlanSchurPairs(ids, n, counts_only, &plan->pairs, cluster, first_id))) return rc;
    SchurClusterPlan& Z = *plan;
    Z.num_clusters = num_clusters;
    Z.num_cameras = C;
    std::vector<int32_t> size((size_t)num_clusters, 0);
    int64_t unobserved = 0;
    for (int64_t c = 0; c < C; ++c) {
      ++size[(size_t)cluster[c]];
      if (!seen[(size_t)c]) ++unobserved;
    }
    for (int32_t g = 0; g < num_clusters; ++g) {
      const int64_t ng = size[(size_t)g];
      Z.num_tiles += ng * (ng + 1) / 2;
      Z.num_values += 81 * ng * ng;
      Z.max_cameras = std::max(Z.max_cameras, ng);
    }
    if (Z.num_tiles >= ((int64_t)1 << 31))
      return CseFail(CSE_ERR_UNSUPPORTED, "cluster plan: 2^31 or more tiles");
    // As PlanSchurSparse: the blocks of several chunks, and the added diagonals.
    Z.finish_capacity = Z.pairs.num_chunks - Z.pairs.num_blocks + unobserved;
    if (counts_only) return CSE_OK;
    Z.camera_begin.assign((size_t)num_clusters + 1, 0);
    Z.first_tile.assign((size_t)num_clusters + 1, 0);
    Z.value_begin.assign((size_t)num_clusters + 1, 0);
    for (int32_t g = 0; g < num_clusters; ++g) {
      const int64_t ng = size[(size_t)g];
      Z.camera_begin[(size_t)g + 1] = Z.camera_begin[(size_t)g] + (int32_t)ng;
      Z.first_tile[(size_t)g + 1] = Z.first_tile[(size_t)g] + ng * (ng + 1) / 2;
      Z.value_begin[(size_t)g + 1] = Z.value_begin[(size_t)g] + 81 * ng * ng;
    }
    // Cameras in ascending order fill their cluster's list; local[c] is the
    // rank of camera c inside its cluster.
    Z.cameras.resize((size_t)C);
    std::vector<int32_t> local((size_t)C), cursor(Z.camera_begin.begin(), Z.camera_begin.end() - 1);
    for (int64_t c = 0; c < C; ++c) {
      const int32_t g = cluster[c];
      local[(size_t)c] = cursor[(size_t)g] - Z.camera_begin[(size_t)g];
      Z.cameras[(size_t)cursor[(size_t)g]++] = (int32_t)c;
    }
    Z.plan_of_tile.assign((size_t)Z.num_tiles, -1);
    Z.tile_camera.resize((size_t)Z.num_tiles);
    for (int32_t g = 0; g < num_clusters; ++g)
      for (int32_t j = 0; j < size[(size_t)g]; ++j)
        for (int32_t i = 0; i <= j; ++i)
          Z.tile_camera[(size_t)(Z.first_tile[(size_t)g] + ClusterTile(i, j))] =
              Z.cameras[(size_t)(Z.camera_begin[(size_t)g] + i)];
    Z.tile_of_plan.resize((size_t)Z.pairs.num_blocks);
    for (int64_t k = 0; k < Z.pairs.num_blocks; ++k) {
      const int64_t c = (int64_t)Z.pairs.block_row[(size_t)k] - first_id;
      const int64_t c2 = (int64_t)Z.pairs.block_col[(size_t)k] - first_id;
      const int64_t t = Z.first_tile[(size_t)cluster[c]] + ClusterTile(local[(size_t)c], local[(size_t)c2]);
      Z.tile_of_plan[(size_t)k] = (int32_t)t;
      Z.plan_of_tile[(size_t)t] = (int32_t)k;
    }
    for (int32_t g = 0; g < num_clusters; ++g)
      for (int32_t j = 0; j < size[(size_t)g]; ++j)
        for (int32_t i = 0; i <= j; ++i) {
          const int64_t t = Z.first_tile[(size_t)g] + ClusterTile(i, j);
          const int64_t k = Z.plan_of_tile[(size_t)t];
          if (k < 0) {
            Z.empty_tiles.push_back((int32_t)t);
            // A diagonal tile no block writes: the camera has no residual block.
            if (i == j) Z.finish.push_back((int32_t)t);
          } else if (Z.pairs.chunk_off[(size_t)k + 1] - Z.pairs.chunk_off[(size_t)k] != 1) {
            Z.finish.push_back((int32_t)t);
          }
        }
    if ((int64_t)Z.finish.size() > Z.finish_capacity)
      return CseFail(CSE_ERR_INVALID, "cluster plan: the finish list exceeds its bound");
  } catch (const std::bad_alloc&) {
    *plan = SchurClusterPlan{};
    return CseFail(CSE_ERR_OOM, "cluster plan: host allocation failed");
  }
  return CSE_OK;
}

int ValidateSchurForest(const int32_t* edges, int32_t num_edges, const int32_t* size, int32_t num_clusters,
                        SchurForestPaths* paths) {
  *paths = SchurForestPaths{};
  if (num_edges < 0) return CseFail(CSE_ERR_INVALID, "cluster forest: negative num_edges");
  if (num_edges > 0 && !edges) return CseFail(CSE_ERR_INVALID, "cluster forest: null edges");
  auto name = [&](int32_t e) {
    return "edge " + std::to_string(e) + " (" + std::to_string(edges[2 * e]) + ", " +
           std::to_string(edges[2 * e + 1]) + ")";
  };
  try {
    std::vector<int32_t>& nb = paths->neighbor;
    nb.assign((size_t)(2 * (int64_t)num_clusters), -1);
    std::vector<int32_t> nb_edge(nb.size(), -1);
    for (int32_t e = 0; e < num_edges; ++e) {
      const int32_t g = edges[2 * e], h = edges[2 * e + 1];
      if (g < 0 || g >= num_clusters || h < 0 || h >= num_clusters)
        return CseFail(CSE_ERR_INVALID, "cluster forest: " + name(e) + " has a label outside [0, " +
                                            std::to_string(num_clusters) + ")");
      if (g == h) return CseFail(CSE_ERR_INVALID, "cluster forest: " + name(e) + " joins a cluster to itself");
    }
    // Duplicates, in either orientation, before degrees: an edge given twice
    // is invalid whatever else the list holds.
    {
      std::vector<std::pair<std::pair<int32_t, int32_t>, int32_t>> sorted;
      sorted.reserve((size_t)num_edges);
      for (int32_t e = 0; e < num_edges; ++e)
        sorted.push_back({{std::min(edges[2 * e], edges[2 * e + 1]), std::max(edges[2 * e], edges[2 * e + 1])}, e});
      std::sort(sorted.begin(), sorted.end());
      for (size_t i = 1; i < sorted.size(); ++i)
        if (sorted[i].first == sorted[i - 1].first)
          return CseFail(CSE_ERR_INVALID, "cluster forest: " + name(sorted[i].second) + " is given twice (as edge " +
                                              std::to_string(sorted[i - 1].second) + ")");
    }
    for (int32_t e = 0; e < num_edges; ++e) {
      const int32_t g = edges[2 * e], h = edges[2 * e + 1];
      for (int32_t v : {g, h}) {
        const int32_t w = v == g ? h : g;
        int32_t* slot = &nb[2 * (size_t)v];
        const int at = slot[0] < 0 ? 0 : slot[1] < 0 ? 1 : 2;
        if (at == 2) {
          return CseFail(CSE_ERR_UNSUPPORTED, "cluster forest: cluster " + std::to_string(v) +
                                                  " has three edges (" + name(e) +
                                                  " is the third); every tree must be a path");
        }
        slot[at] = w;
        nb_edge[2 * (size_t)v + at] = e;
      }
    }
    for (int32_t e = 0; e < num_edges; ++e) {
      const int64_t sum = (int64_t)size[edges[2 * e]] + size[edges[2 * e + 1]];
      if (sum > kSchurMaxClusterCameras)
        return CseFail(CSE_ERR_UNSUPPORTED,
                       "cluster forest: the clusters of " + name(e) + " hold " + std::to_string(sum) +
                           " cameras together, more than " + std::to_string(kSchurMaxClusterCameras) +
                           " (one elimination step works in the LDS of one workgroup)");
    }
    // The paths: from every cluster of degree < 2 not yet visited, in label
    // order, so a path starts at its end with the smaller label and the paths
    // come ordered by their first cluster.
    std::vector<bool> visited((size_t)num_clusters, false);
    paths->path_begin.assign(1, 0);
    for (int32_t g = 0; g < num_clusters; ++g) {
      if (visited[(size_t)g] || nb[2 * (size_t)g + 1] >= 0) continue;
      int32_t prev = -1, at = g;
      while (at >= 0) {
        visited[(size_t)at] = true;
        const int which = nb[2 * (size_t)at] >= 0 && nb[2 * (size_t)at] != prev ? 0
                          : nb[2 * (size_t)at + 1] >= 0 && nb[2 * (size_t)at + 1] != prev ? 1 : -1;
        paths->path_cluster.push_back(at);
        if (which < 0) {
          paths->path_edge.push_back(-1);
          break;
        }
        const int32_t e = nb_edge[2 * (size_t)at + which];
        paths->path_edge.push_back(2 * e + (edges[2 * e + 1] == at ? 1 : 0));
        prev = at;
        at = nb[2 * (size_t)at + which];
      }
      paths->path_begin.push_back((int32_t)paths->path_cluster.size());
    }
    // What is left has degree 2 throughout: a cycle.
    for (int32_t g = 0; g < num_clusters; ++g)
      if (!visited[(size_t)g])
        return CseFail(CSE_ERR_UNSUPPORTED, "cluster forest: cluster " + std::to_string(g) +
                                                " lies on a cycle; every tree must be a path");
  } catch (const std::bad_alloc&) {
    *paths = SchurForestPaths{};
    return CseFail(CSE_ERR_OOM, "cluster forest: host allocation failed");
  }
  return CSE_OK;
}

int PlanSchurTridiagonal(const int32_t* ids, int64_t n, int32_t first_id, int64_t C, const int32_t* cluster,
                         int32_t num_clusters, const int32_t* edges, int32_t num_edges, bool counts_only,
                         SchurTridiagonalPlan* plan) {
  *plan = SchurTridiagonalPlan{};
  int rc = ValidateSchurClusters(cluster, C, num_clusters);
  if (rc) return rc;
  try {
    std::vector<int32_t> size((size_t)num_clusters, 0);
    for (int64_t c = 0; c < C; ++c) ++size[(size_t)cluster[c]];
    SchurTridiagonalPlan& Z = *plan;
    if ((rc = ValidateSchurForest(edges, num_edges, size.data(), num_clusters, &Z.paths))) return rc;
    std::vector<bool> seen((size_t)C, false);
    int64_t unobserved = 0;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t c = (int64_t)ids[2 * i] - first_id;
      if (c < 0 || c >= C) return CseFail(CSE_ERR_INVALID, "tridiagonal plan: an f block outside the cameras");
      seen[(size_t)c] = true;
    }
    for (int64_t c = 0; c < C; ++c)
      if (!seen[(size_t)c]) ++unobserved;
    if ((rc = PlanSchurPairs(ids, n, counts_only, &Z.pairs, cluster, first_id, Z.paths.neighbor.data()))) return rc;
    Z.num_clusters = num_clusters;
    Z.num_cameras = C;
    Z.num_edges = num_edges;
    Z.num_paths = (int64_t)Z.paths.path_begin.size() - 1;
    for (int32_t g = 0; g < num_clusters; ++g) {
      const int64_t ng = size[(size_t)g];
      Z.num_cluster_tiles += ng * (ng + 1) / 2;
      Z.num_values += 81 * ng * ng;
      Z.max_cameras = std::max(Z.max_cameras, ng);
    }
    Z.num_tiles = Z.num_cluster_tiles;
    Z.max_step_cameras = Z.max_cameras;
    for (int32_t e = 0; e < num_edges; ++e) {
      const int64_t ng = size[(size_t)edges[2 * e]], nh = size[(size_t)edges[2 * e + 1]];
      Z.num_tiles += ng * nh;
      Z.num_values += 81 * ng * nh;
      Z.max_step_cameras = std::max(Z.max_step_cameras, ng + nh);
    }
    for (int64_t p = 0; p < Z.num_paths; ++p)
      Z.longest_path = std::max<int64_t>(Z.longest_path, Z.paths.path_begin[(size_t)p + 1] - Z.paths.path_begin[(size_t)p]);
    if (Z.num_tiles >= ((int64_t)1 << 31))
      return CseFail(CSE_ERR_UNSUPPORTED, "tridiagonal plan: 2^31 or more tiles");
    Z.finish_capacity = Z.pairs.num_chunks - Z.pairs.num_blocks + unobserved;
    if (counts_only) return CSE_OK;
    Z.camera_begin.assign((size_t)num_clusters + 1, 0);
    Z.first_tile.assign((size_t)num_clusters + 1, 0);
    Z.value_begin.assign((size_t)num_clusters + 1, 0);
    for (int32_t g = 0; g < num_clusters; ++g) {
      const int64_t ng = size[(size_t)g];
      Z.camera_begin[(size_t)g + 1] = Z.camera_begin[(size_t)g] + (int32_t)ng;
      Z.first_tile[(size_t)g + 1] = Z.first_tile[(size_t)g] + ng * (ng + 1) / 2;
      Z.value_begin[(size_t)g + 1] = Z.value_begin[(size_t)g] + 81 * ng * ng;
    }
    Z.edges.assign(edges, edges + 2 * (size_t)num_edges);
    Z.edge_tile.assign((size_t)num_edges + 1, Z.num_cluster_tiles);
    Z.edge_value.assign((size_t)num_edges + 1, Z.value_begin[(size_t)num_clusters]);
    for (int32_t e = 0; e < num_edges; ++e) {
      const int64_t cells = (int64_t)size[(size_t)edges[2 * e]] * size[(size_t)edges[2 * e + 1]];
      Z.edge_tile[(size_t)e + 1] = Z.edge_tile[(size_t)e] + cells;
      Z.edge_value[(size_t)e + 1] = Z.edge_value[(size_t)e] + 81 * cells;
    }
    Z.cameras.resize((size_t)C);
    std::vector<int32_t> local((size_t)C), cursor(Z.camera_begin.begin(), Z.camera_begin.end() - 1);
    for (int64_t c = 0; c < C; ++c) {
      const int32_t g = cluster[c];
      local[(size_t)c] = cursor[(size_t)g] - Z.camera_begin[(size_t)g];
      Z.cameras[(size_t)cursor[(size_t)g]++] = (int32_t)c;
    }
    Z.plan_of_tile.assign((size_t)Z.num_tiles, -1);
    Z.tile_camera.resize((size_t)Z.num_tiles);
    for (int32_t g = 0; g < num_clusters; ++g)
      for (int32_t j = 0; j < size[(size_t)g]; ++j)
        for (int32_t i = 0; i <= j; ++i)
          Z.tile_camera[(size_t)(Z.first_tile[(size_t)g] + ClusterTile(i, j))] =
              Z.cameras[(size_t)(Z.camera_begin[(size_t)g] + i)];
    for (int32_t e = 0; e < num_edges; ++e) {
      const int32_t g = edges[2 * e], nh = size[(size_t)edges[2 * e + 1]];
      for (int32_t i = 0; i < size[(size_t)g]; ++i)
        for (int32_t j = 0; j < nh; ++j)  // not read: only an empty diagonal tile's camera is
          Z.tile_camera[(size_t)(Z.edge_tile[(size_t)e] + (int64_t)i * nh + j)] =
              Z.cameras[(size_t)(Z.camera_begin[(size_t)g] + i)];
    }
    // The edge of two joined labels, by the smaller label's neighbour slot.
    auto edge_of = [&](int32_t a, int32_t b) {
      for (int32_t e = 0; e < num_edges; ++e)
        if ((edges[2 * e] == a && edges[2 * e + 1] == b) || (edges[2 * e] == b && edges[2 * e + 1] == a)) return e;
      return (int32_t)-1;
    };
    std::vector<int32_t> slot_edge((size_t)(2 * (int64_t)num_clusters), -1);
    for (int32_t g = 0; g < num_clusters; ++g)
      for (int s = 0; s < 2; ++s)
        if (Z.paths.neighbor[2 * (size_t)g + s] >= 0 && Z.paths.neighbor[2 * (size_t)g + s] > g)
          slot_edge[2 * (size_t)g + s] = edge_of(g, Z.paths.neighbor[2 * (size_t)g + s]);
    Z.tile_of_plan.resize((size_t)Z.pairs.num_blocks);
    for (int64_t k = 0; k < Z.pairs.num_blocks; ++k) {
      const int64_t c = (int64_t)Z.pairs.block_row[(size_t)k] - first_id;
      const int64_t c2 = (int64_t)Z.pairs.block_col[(size_t)k] - first_id;
      const int32_t l = cluster[c], l2 = cluster[c2];
      int64_t t;
      if (l == l2) {
        t = Z.first_tile[(size_t)l] + ClusterTile(local[(size_t)c], local[(size_t)c2]);
      } else {
        const int32_t lo = std::min(l, l2), hi = std::max(l, l2);
        const int s = Z.paths.neighbor[2 * (size_t)lo] == hi ? 0 : 1;
        const int32_t e = slot_edge[2 * (size_t)lo + s];
        if (e < 0) return CseFail(CSE_ERR_INVALID, "tridiagonal plan: a kept block without an edge");
        // The camera of the edge's g gives the rectangle's row.
        const int64_t cg = edges[2 * e] == l ? c : c2, ch = edges[2 * e] == l ? c2 : c;
        t = Z.edge_tile[(size_t)e] + (int64_t)local[(size_t)cg] * size[(size_t)edges[2 * e + 1]] + local[(size_t)ch];
      }
      Z.tile_of_plan[(size_t)k] = (int32_t)t;
      Z.plan_of_tile[(size_t)t] = (int32_t)k;
    }
    for (int64_t t = 0; t < Z.num_tiles; ++t) {
      const int64_t k = Z.plan_of_tile[(size_t)t];
      if (k < 0) {
        Z.empty_tiles.push_back((int32_t)t);
        continue;
      }
      if (Z.pairs.chunk_off[(size_t)k + 1] - Z.pairs.chunk_off[(size_t)k] != 1) Z.finish.push_back((int32_t)t);
    }
    // A diagonal tile no block writes: the camera has no residual block.
    for (int32_t g = 0; g < num_clusters; ++g)
      for (int32_t j = 0; j < size[(size_t)g]; ++j) {
        const int64_t t = Z.first_tile[(size_t)g] + ClusterTile(j, j);
        if (Z.plan_of_tile[(size_t)t] < 0) Z.finish.push_back((int32_t)t);
      }
    if ((int64_t)Z.finish.size() > Z.finish_capacity)
      return CseFail(CSE_ERR_INVALID, "tridiagonal plan: the finish list exceeds its bound");
  } catch (const std::bad_alloc&) {
    *plan = SchurTridiagonalPlan{};
    return CseFail(CSE_ERR_OOM, "tridiagonal plan: host allocation failed");
  }
  return CSE_OK;
}

int PlanDenseCholesky(int64_t n, int32_t precision, DenseCholeskyPlan* plan) {
  if (!plan) return CseFail(CSE_ERR_INVALID, "dense Cholesky plan: null plan");
  if (n < 1) return CseFail(CSE_ERR_INVALID, "dense Cholesky: n must be at least 1");
  if (precision != CSE_DENSE_CHOLESKY_FP64 && precision != CSE_DENSE_CHOLESKY_FP32)
    return CseFail(CSE_ERR_INVALID, "dense Cholesky: unknown precision " + std::to_string(precision));
  DenseCholeskyPlan P;
  P.n = n;
  P.precision = precision;
  P.num_panels = (n + kDenseCholeskyNB - 1) / kDenseCholeskyNB;
  P.padded = P.num_panels * kDenseCholeskyNB;
  const bool f32 = precision == CSE_DENSE_CHOLESKY_FP32;
  // Diagonal, panel and trailing update per step; the last step has no rows below.
  P.factor_launches = 3 * P.num_panels - 2 + (f32 ? 1 : 0);
  P.substitution_launches = 2 * P.num_panels;
  const int64_t elem = f32 ? 4 : 8;
  auto segment = [](int64_t bytes) { return (bytes + kDenseCholeskyAlign - 1) / kDenseCholeskyAlign * kDenseCholeskyAlign; };
  int64_t off = 0;
  P.matrix_off = off;
  if (f32) off += segment(n * n * elem);
  P.inverse_off = off;
  off += segment(P.num_panels * kDenseCholeskyNB * kDenseCholeskyNB * elem);
  P.v_off = off;
  off += segment(P.padded * elem);
  P.y_off = off;
  off += segment(P.padded * elem);
  P.x_off = off;
  if (f32) off += segment(P.padded * 8);
  P.r_off = off;
  if (f32) off += segment(P.padded * 8);
  P.flag_off = off;
  off += kDenseCholeskyAlign;
  P.workspace_bytes = off;
  *plan = P;
  return CSE_OK;
}

namespace {

// The input's format (PlanSchurSparse's): diagonal first, columns ascending and in range.
int ValidateSparseRows(int64_t N, const int64_t* row_begin, const int32_t* block_col) {
  if (N < 1) return CseFail(CSE_ERR_INVALID, "sparse Cholesky: num_block_rows must be at least 1");
  if (N > (INT32_MAX - 1) / 9)
    return CseFail(CSE_ERR_UNSUPPORTED, "sparse Cholesky: 9 num_block_rows + 1 does not fit int32");
  if (!row_begin || !block_col) return CseFail(CSE_ERR_INVALID, "sparse Cholesky: null pointer");
  if (row_begin[0] != 0) return CseFail(CSE_ERR_INVALID, "sparse Cholesky: row_begin[0] is not 0");
  for (int64_t r = 0; r < N; ++r) {
    const int64_t b = row_begin[r], e = row_begin[r + 1];
    if (e <= b || block_col[b] != r)
      return CseFail(CSE_ERR_INVALID,
                     "sparse Cholesky: block row " + std::to_string(r) + " does not start with its diagonal block");
    for (int64_t k = b + 1; k < e; ++k)
      if (block_col[k] <= block_col[k - 1] || block_col[k] >= N)
        return CseFail(CSE_ERR_INVALID, "sparse Cholesky: block row " + std::to_string(r) +
                                            " has columns that do not ascend or are out of range");
    if (e >= INT32_MAX) return CseFail(CSE_ERR_UNSUPPORTED, "sparse Cholesky: 2^31 or more input blocks");
  }
  return CSE_OK;
}

inline int Popcount(const uint64_t* w, int64_t words) {
  int n = 0;
  for (int64_t k = 0; k < words; ++k) n += __builtin_popcountll(w[k]);
  return n;
}

}  // namespace

int SparseCholeskyMinimumDegree(int64_t N, const int64_t* row_begin, const int32_t* block_col,
                                std::vector<int32_t>* permutation) {
  try {
    const int64_t W = (N + 63) / 64;
    std::vector<uint64_t> adj((size_t)(N * W), 0);
    auto set = [&](int64_t a, int64_t b) { adj[(size_t)(a * W + b / 64)] |= uint64_t(1) << (b % 64); };
    for (int64_t r = 0; r < N; ++r)
      for (int64_t k = row_begin[r] + 1; k < row_begin[r + 1]; ++k) set(r, block_col[k]), set(block_col[k], r);
    std::vector<int32_t> degree((size_t)N);
    std::vector<char> alive((size_t)N, 1);
    for (int64_t v = 0; v < N; ++v) degree[(size_t)v] = Popcount(&adj[(size_t)(v * W)], W);
    permutation->clear();
    permutation->reserve((size_t)N);
    for (int64_t remaining = N; remaining > 0; --remaining) {
      int64_t v = -1;
      for (int64_t u = 0; u < N; ++u)
        if (alive[(size_t)u] && (v < 0 || degree[(size_t)u] < degree[(size_t)v])) v = u;
      if (degree[(size_t)v] == remaining - 1) {  // a clique: index order from here
        for (int64_t u = 0; u < N; ++u)
          if (alive[(size_t)u]) permutation->push_back((int32_t)u);
        break;
      }
      permutation->push_back((int32_t)v);
      alive[(size_t)v] = 0;
      const uint64_t* rv = &adj[(size_t)(v * W)];
      for (int64_t w = 0; w < W; ++w)
        for (uint64_t bits = rv[w]; bits; bits &= bits - 1) {
          const int64_t u = 64 * w + __builtin_ctzll(bits);
          uint64_t* ru = &adj[(size_t)(u * W)];
          for (int64_t k = 0; k < W; ++k) ru[k] |= rv[k];
          ru[u / 64] &= ~(uint64_t(1) << (u % 64));
          ru[v / 64] &= ~(uint64_t(1) << (v % 64));
          degree[(size_t)u] = Popcount(ru, W);
        }
    }
  } catch (const std::bad_alloc&) {
    return CseFail(CSE_ERR_OOM, "sparse Cholesky: host allocation of the minimum-degree bit rows failed");
  }
  return CSE_OK;
}

int PlanSparseCholesky(int64_t N, const int64_t* row_begin, const int32_t* block_col, int32_t ordering,
                       const int32_t* permutation, SparseCholeskyPlan* plan) {
  if (!plan) return CseFail(CSE_ERR_INVALID, "sparse Cholesky plan: null plan");
  int rc = ValidateSparseRows(N, row_begin, block_col);
  if (rc) return rc;
  if (ordering != CSE_SPARSE_ORDERING_NATURAL && ordering != CSE_SPARSE_ORDERING_MINIMUM_DEGREE &&
      ordering != CSE_SPARSE_ORDERING_GIVEN)
    return CseFail(CSE_ERR_INVALID, "sparse Cholesky: unknown ordering " + std::to_string(ordering));
  if (ordering == CSE_SPARSE_ORDERING_GIVEN && !permutation)
    return CseFail(CSE_ERR_INVALID, "sparse Cholesky: the given ordering without a permutation");
  try {
    SparseCholeskyPlan P;
    const size_t n = (size_t)N;
    P.num_block_rows = N;
    P.num_input_blocks = row_begin[N];
    P.in_row_begin.assign(row_begin, row_begin + N + 1);
    P.in_block_col.assign(block_col, block_col + P.num_input_blocks);
    // The order.
    P.position.assign(n, -1);
    if (ordering == CSE_SPARSE_ORDERING_MINIMUM_DEGREE) {
      if ((rc = SparseCholeskyMinimumDegree(N, row_begin, block_col, &P.permutation))) return rc;
    } else {
      P.permutation.resize(n);
      for (size_t k = 0; k < n; ++k)
        P.permutation[k] = ordering == CSE_SPARSE_ORDERING_GIVEN ? permutation[k] : (int32_t)k;
    }
    for (size_t k = 0; k < n; ++k) {
      const int32_t r = P.permutation[k];
      if (r < 0 || r >= N || P.position[(size_t)r] >= 0)
        return CseFail(CSE_ERR_INVALID, "sparse Cholesky: the given order is not a permutation of the block rows");
      P.position[(size_t)r] = (int32_t)k;
    }
    // The input's transposed index, and B's strict lower triangle by columns.
    P.in_col_begin.assign(n + 1, 0);
    std::vector<int64_t> a_begin(n + 1, 0);
    for (int64_t r = 0; r < N; ++r)
      for (int64_t k = row_begin[r] + 1; k < row_begin[r + 1]; ++k) {
        ++P.in_col_begin[(size_t)block_col[k] + 1];
        ++a_begin[(size_t)std::min(P.position[(size_t)r], P.position[(size_t)block_col[k]]) + 1];
      }
    for (size_t c = 0; c < n; ++c) P.in_col_begin[c + 1] += P.in_col_begin[c], a_begin[c + 1] += a_begin[c];
    P.in_col_block.resize((size_t)(P.num_input_blocks - N));
    P.in_col_row.resize(P.in_col_block.size());
    std::vector<int32_t> a_rows(P.in_col_block.size());
    {
      std::vector<int64_t> fill(P.in_col_begin.begin(), P.in_col_begin.end() - 1);
      std::vector<int64_t> afill(a_begin.begin(), a_begin.end() - 1);
      for (int64_t r = 0; r < N; ++r)
        for (int64_t k = row_begin[r] + 1; k < row_begin[r + 1]; ++k) {
          const int32_t c = block_col[k];
          const int64_t at = fill[(size_t)c]++;
          P.in_col_block[(size_t)at] = (int32_t)k, P.in_col_row[(size_t)at] = (int32_t)r;
          const int32_t p = P.position[(size_t)r], q = P.position[(size_t)c];
          a_rows[(size_t)afill[(size_t)std::min(p, q)]++] = std::max(p, q);
        }
    }
    // Column structures with fill, the elimination tree and its levels:
    // struct(j) = B's column j below the diagonal, and struct(c) \ {j} of every
    // child c; parent(j) = min struct(j).
    P.parent.assign(n, -1);
    P.level.assign(n, 0);
    P.col_begin.assign(n + 1, 0);
    std::vector<int32_t> col_rows, child_head(n, -1), child_next(n, -1), mark(n, -1);
    for (int64_t j = 0; j < N; ++j) {
      const size_t begin = col_rows.size();
      for (int64_t k = a_begin[(size_t)j]; k < a_begin[(size_t)j + 1]; ++k) {
        const int32_t i = a_rows[(size_t)k];
        if (mark[(size_t)i] != j) mark[(size_t)i] = (int32_t)j, col_rows.push_back(i);
      }
      for (int32_t c = child_head[(size_t)j]; c >= 0; c = child_next[(size_t)c])
        for (int64_t k = P.col_begin[(size_t)c]; k < P.col_begin[(size_t)c + 1]; ++k) {
          const int32_t i = col_rows[(size_t)k];
          if (i != j && mark[(size_t)i] != j) mark[(size_t)i] = (int32_t)j, col_rows.push_back(i);
        }
      std::sort(col_rows.begin() + (std::ptrdiff_t)begin, col_rows.end());
      P.col_begin[(size_t)j + 1] = (int64_t)col_rows.size();
      if ((int64_t)col_rows.size() + N >= INT32_MAX)
        return CseFail(CSE_ERR_UNSUPPORTED, "sparse Cholesky: 2^31 or more factor blocks");
      if (col_rows.size() > begin) {
        const int32_t p = col_rows[begin];
        P.parent[(size_t)j] = p;
        child_next[(size_t)j] = child_head[(size_t)p], child_head[(size_t)p] = (int32_t)j;
        P.level[(size_t)p] = std::max(P.level[(size_t)p], P.level[(size_t)j] + 1);
      }
      const int64_t m = (int64_t)(col_rows.size() - begin);
      P.num_block_products += m * (m + 1) / 2;
    }
    P.num_factor_blocks = (int64_t)col_rows.size() + N;
    // L by rows: a row's columns ascend because the columns are walked in order.
    P.row_begin.assign(n + 1, 0);
    for (int32_t i : col_rows) ++P.row_begin[(size_t)i + 1];
    for (size_t i = 0; i < n; ++i) P.row_begin[i + 1] += P.row_begin[i] + 1;
    P.block_col.resize((size_t)P.num_factor_blocks);
    P.block_row.resize((size_t)P.num_factor_blocks);
    P.col_block.resize(col_rows.size());
    {
      std::vector<int64_t> fill(P.row_begin.begin(), P.row_begin.end() - 1);
      for (int64_t j = 0; j < N; ++j)
        for (int64_t k = P.col_begin[(size_t)j]; k < P.col_begin[(size_t)j + 1]; ++k) {
          const int32_t i = col_rows[(size_t)k];
          const int64_t id = fill[(size_t)i]++;
          P.block_col[(size_t)id] = (int32_t)j, P.block_row[(size_t)id] = i;
          P.col_block[(size_t)k] = (int32_t)id;
        }
      for (int64_t i = 0; i < N; ++i) {
        const int64_t id = P.row_begin[(size_t)i + 1] - 1;
        P.block_col[(size_t)id] = P.block_row[(size_t)id] = (int32_t)i;
      }
    }
    // Scatter and its inverse.
    P.scatter.resize((size_t)P.num_input_blocks);
    P.source.assign((size_t)P.num_factor_blocks, -1);
    for (int64_t r = 0; r < N; ++r)
      for (int64_t k = row_begin[r]; k < row_begin[r + 1]; ++k) {
        const int32_t p = P.position[(size_t)r], q = P.position[(size_t)block_col[k]];
        const int32_t i = std::max(p, q), j = std::min(p, q);
        const int32_t* first = &P.block_col[(size_t)P.row_begin[(size_t)i]];
        const int32_t* last = &P.block_col[(size_t)P.row_begin[(size_t)i + 1] - 1] + 1;
        const int64_t id = P.row_begin[(size_t)i] + (std::lower_bound(first, last, j) - first);
        const bool transposed = p < q;
        P.scatter[(size_t)k] = transposed ? ~(int32_t)id : (int32_t)id;
        P.source[(size_t)id] = transposed ? -2 - (int32_t)k : (int32_t)k;
      }
    // The level table.
    for (size_t j = 0; j < n; ++j) P.num_levels = std::max(P.num_levels, P.level[j] + 1);
    P.level_begin.assign((size_t)P.num_levels + 1, 0);
    P.target_begin.assign((size_t)P.num_levels + 1, 0);
    for (size_t j = 0; j < n; ++j) {
      ++P.level_begin[(size_t)P.level[j] + 1];
      P.target_begin[(size_t)P.level[j] + 1] += P.col_begin[j + 1] - P.col_begin[j];
    }
    for (int32_t l = 0; l < P.num_levels; ++l) {
      P.max_level_columns = std::max<int64_t>(P.max_level_columns, P.level_begin[(size_t)l + 1]);
      P.level_begin[(size_t)l + 1] += P.level_begin[(size_t)l];
      P.target_begin[(size_t)l + 1] += P.target_begin[(size_t)l];
    }
    P.level_columns.resize(n);
    P.level_targets.resize(col_rows.size());
    {
      std::vector<int64_t> fill(P.level_begin.begin(), P.level_begin.end() - 1);
      std::vector<int64_t> tfill(P.target_begin.begin(), P.target_begin.end() - 1);
      for (int64_t j = 0; j < N; ++j) {
        const size_t l = (size_t)P.level[(size_t)j];
        P.level_columns[(size_t)fill[l]++] = (int32_t)j;
        for (int64_t k = P.col_begin[(size_t)j]; k < P.col_begin[(size_t)j + 1]; ++k)
          P.level_targets[(size_t)tfill[l]++] = P.col_block[(size_t)k];
      }
    }
    // Device bytes: the tables, L and the inverses of its diagonal blocks,
    // the two solve vectors, the per-column status words and info.
    const int64_t nf = P.num_factor_blocks, ni = P.num_input_blocks;
    P.device_bytes = 4 * (2 * N)                     // permutation, position
                     + 8 * 2 * (N + 1) + 4 * (2 * nf + (nf - N) + nf)  // row/col begin, block col/row, col_block, source
                     + 4 * (N + (nf - N))            // level columns, level targets
                     + 8 * 2 * (N + 1) + 4 * (ni + 2 * (ni - N))       // the input's arrays
                     + 8 * 81 * (nf + N) + 8 * 2 * 9 * N + 4 * (N + 1);
    *plan = std::move(P);
  } catch (const std::bad_alloc&) {
    return CseFail(CSE_ERR_OOM, "sparse Cholesky plan: host allocation failed");
  }
  return CSE_OK;
}

}  // namespace cse
