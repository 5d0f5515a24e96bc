// per_block_loss_driver.cpp -- the host-only planner (csrc/plan.cpp) on groups
// with per-block loss parameters (cse_residual_group.loss_data_size == 2),
// built by g++ with AddressSanitizer + UBSan from plan.cpp, layout.cpp and this
// file (tests/test_per_block_loss.py compiles and runs it; no HIP, no GPU).
//
// For a Snavely group in the BlockSparseMatrix and CompressedRowSparseMatrix
// layouts, with and without a held camera, and for a one-slot
// POINT_DISPLACEMENT group: Validate, ValidateGroups and PlanGroup accept the
// widened rows and every plan scalar and table equals the uniform twin's (the
// same blocks, loss_data_size 0); only the byte counts grow, by 16 per block.
// Then every descriptor cse_create must refuse, with its code and a message
// that names loss_data_size.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ceres-solver-cuda_amd/csrc/plan.hpp"
#include "../../include/cse.h"

namespace cse {
std::string& LastError();  // layout.cpp (cse_last_error reads it in the HIP half)
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
// them, observations point-major; every camera and every point is used.
struct Problem {
  int C = 0, P = 0;
  int64_t O = 0;
  int cam_size = 9;
  bool one_slot = false;  // POINT_DISPLACEMENT_3_3: one block per point, no cameras
  std::vector<int32_t> ids;
  std::vector<double> data;       // [O][D]
  std::vector<double> wide;       // [O][D + 2]: data, then (a, scale)
  std::vector<cse_parameter_block> pbs;
  std::vector<int64_t> begin, res_layout, jac_layout, jac_offsets;
  std::vector<int32_t> params, nres;
  std::vector<double> cstate;
  int64_t num_values = 0;
  cse_residual_group g{};
  cse_problem_desc d{};
};

void Build(Problem* Q, int C, int P, int per_point, bool crs, int held, bool one_slot) {
  Problem& q = *Q;
  q.C = one_slot ? 0 : C;
  q.P = P;
  q.one_slot = one_slot;
  const int D = one_slot ? 3 : 2, nr = one_slot ? 3 : 2;
  for (int p = 0; p < P; ++p) q.pbs.push_back({3, 3, 0, 0, 3LL * p, 3LL * p, -1});
  for (int c = 0; c < q.C; ++c) {
    const int64_t at = 3LL * P + 9LL * (c - (held >= 0 && c > held ? 1 : 0));
    if (c == held) q.pbs.push_back({9, 9, 1, 0, 0, 0, -1});
    else q.pbs.push_back({9, 9, 0, 0, at, at, -1});
  }
  if (held >= 0) q.cstate.assign(9, 0.25);
  q.begin.push_back(0);
  for (int p = 0; p < P; ++p) {
    const int n = one_slot ? 1 : 1 + (p + 1) % per_point;
    for (int k = 0; k < n; ++k) {
      if (!one_slot) {
        q.ids.push_back(P + (p * 7 + k * 3) % C);
        q.params.push_back(q.ids.back());
      }
      q.ids.push_back(p);
      q.params.push_back(p);
      q.begin.push_back((int64_t)q.params.size());
      q.nres.push_back(nr);
      for (int c = 0; c < D; ++c) q.data.push_back(200.0 * (Uniform() - 0.5));
    }
  }
  q.O = (int64_t)q.nres.size();
  for (int64_t i = 0; i < q.O; ++i) {
    for (int c = 0; c < D; ++c) q.wide.push_back(q.data[i * D + c]);
    q.wide.push_back(0.5 + (double)(i % 3));   // a
    q.wide.push_back(0.25 * (double)(1 << (2 * (i % 3))));  // scale: 0.25, 1, 4
  }
  const int64_t npb = (int64_t)q.pbs.size();
  const int64_t count = cse_layout_offsets_count(npb, q.pbs.data(), q.O, q.begin.data(), q.params.data(),
                                                 q.nres.data());
  q.res_layout.resize(q.O);
  q.jac_layout.resize(q.O);
  q.jac_offsets.resize(count > 0 ? count : 1);
  if (!crs) {
    EXPECT(cse_block_sparse_layout(npb, q.pbs.data(), q.O, q.begin.data(), q.params.data(), q.nres.data(),
                                   one_slot ? 0 : P, q.res_layout.data(), q.jac_layout.data(),
                                   q.jac_offsets.data(), &q.num_values) == CSE_OK);
  } else {
    std::vector<int64_t> rows(nr * q.O + 1);
    EXPECT(cse_compressed_row_layout(npb, q.pbs.data(), q.O, q.begin.data(), q.params.data(),
                                     q.nres.data(), q.res_layout.data(), q.jac_layout.data(),
                                     q.jac_offsets.data(), &q.num_values, rows.data(), nullptr) == CSE_OK);
  }
  q.g.functor_kind = one_slot ? CSE_FUNCTOR_POINT_DISPLACEMENT_3_3 : CSE_FUNCTOR_SNAVELY_2_9_3;
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
  d.num_residuals = nr * q.O;
  d.residual_layout = q.res_layout.data();
  d.jacobian_per_residual_layout = q.jac_layout.data();
  d.jacobian_per_residual_offsets = q.jac_offsets.data();
  d.num_jacobian_per_residual_offsets = count;
  d.num_jacobian_values = q.num_values;
}

void SetPerBlock(Problem* q, bool on) {
  q->g.loss_data_size = on ? 2 : 0;
  q->g.functor_data = on ? q->wide.data() : q->data.data();
}

cse_options DefaultOptions() {
  cse_options o{};
  o.device = -1;
  o.check_finite = 1;
  o.apply_loss_function = 1;
  return o;
}

struct Planned {
  cse::ProgramPlan P;
  cse::GroupPlan G;
  cse::GroupTables T;
};

int Plan(const cse_problem_desc& d, const cse_options& o, Planned* out) {
  int rc = cse::Validate(&d);
  if (rc) return rc;
  if ((rc = cse::ValidateGroups(&d, nullptr, &out->P, &o))) return rc;
  cse::PlanGroup(&d, o, 0, &out->P, &out->G, &out->T);
  cse::PlanProgram(&d, &out->G, &out->P);
  return CSE_OK;
}

bool SameInfo(const cse::GradPlanInfo& a, const cse::GradPlanInfo& b) {
  return a.ready == b.ready && a.sorted == b.sorted && a.wave == b.wave && a.lo == b.lo &&
         a.count == b.count && a.passes == b.passes && a.nchunks == b.nchunks && a.nperm == b.nperm &&
         a.all_present == b.all_present;
}

// Every decision of the per-block plan equals the uniform twin's.
void ExpectSamePlan(const Planned& u, const Planned& p, int64_t n, const char* what) {
  std::printf("  %s: policy %d affine %d const0 %d fuse_ok %d grad_exact %d repack0 %d plain0 %d wg %lld\n",
              what, p.G.policy, (int)p.G.affine, (int)p.G.const0, (int)p.G.fuse_ok, (int)p.G.grad_exact,
              (int)p.G.repack0, (int)p.G.plain0, (long long)p.G.num_wg);
  const cse::GroupPlan &a = u.G, &b = p.G;
  EXPECT(a.loss_data_size == 0 && b.loss_data_size == 2);
  EXPECT(a.kind == b.kind && a.n == b.n && a.affine == b.affine && a.policy == b.policy);
  EXPECT(a.partial_offset == b.partial_offset && a.num_wg == b.num_wg && a.first == b.first);
  EXPECT(!std::memcmp(a.state_base, b.state_base, sizeof(a.state_base)));
  EXPECT(!std::memcmp(a.delta_base, b.delta_base, sizeof(a.delta_base)));
  EXPECT(!std::memcmp(a.jac_base, b.jac_base, sizeof(a.jac_base)));
  EXPECT(!std::memcmp(a.jac_stride, b.jac_stride, sizeof(a.jac_stride)));
  EXPECT(a.res_base == b.res_base && a.repack0 == b.repack0 && a.slot0_lo == b.slot0_lo);
  EXPECT(a.slot0_count == b.slot0_count && a.slot0_stride == b.slot0_stride);
  EXPECT(a.packed_stride == b.packed_stride && a.slot0_manifold == b.slot0_manifold);
  EXPECT(a.grad_exact == b.grad_exact && a.const0 == b.const0 && a.fbase0 == b.fbase0);
  EXPECT(a.fuse_ok == b.fuse_ok && a.jet == b.jet && a.plain0 == b.plain0);
  EXPECT(a.plain0_state_base == b.plain0_state_base && a.plain0_delta_base == b.plain0_delta_base);
  for (int j = 0; j < 2; ++j) {
    EXPECT(SameInfo(u.T.grad_info[j], p.T.grad_info[j]));
    EXPECT(u.T.grad[j].perm == p.T.grad[j].perm && u.T.grad[j].off == p.T.grad[j].off);
    EXPECT(u.T.grad[j].chunk_begin == p.T.grad[j].chunk_begin);
    EXPECT(u.T.grad[j].chunk_off == p.T.grad[j].chunk_off && u.T.grad[j].chunk_pb == p.T.grad[j].chunk_pb);
    EXPECT(u.T.grad[j].chunk_order == p.T.grad[j].chunk_order);
  }
  EXPECT(u.T.bits == p.T.bits && u.T.src == p.T.src && u.T.dlt == p.T.dlt && u.T.fbase == p.T.fbase);
  EXPECT(u.T.prev_seg == p.T.prev_seg && u.T.runs == p.T.runs);
  EXPECT(u.P.total_wg == p.P.total_wg && u.P.any_general == p.P.any_general);
  EXPECT(u.P.res_covered == p.P.res_covered && u.P.jac_covered == p.P.jac_covered);
  EXPECT(u.P.schur.eligible == p.P.schur.eligible && u.P.schur.nchunks == p.P.schur.nchunks);
  EXPECT(u.P.schur.nbig == p.P.schur.nbig && u.P.schur_chunk_begin == p.P.schur_chunk_begin);
  // 16 bytes more per block in both traffic figures, nothing else.
  EXPECT(p.P.bytes_jac == u.P.bytes_jac + 16 * n);
  EXPECT(p.P.bytes_res == u.P.bytes_res + 16 * n);
}

void Twin(const char* what, int C, int P, int per_point, bool crs, int held, bool one_slot,
          bool general = false) {
  Problem q;
  Build(&q, C, P, per_point, crs, held, one_slot);
  cse_options o = DefaultOptions();
  o.force_general_layout = general;
  Planned u, p;
  SetPerBlock(&q, false);
  EXPECT(Plan(q.d, o, &u) == CSE_OK);
  SetPerBlock(&q, true);
  const int rc = Plan(q.d, o, &p);
  EXPECT(rc == CSE_OK);
  if (rc != CSE_OK) {
    std::printf("  %s: refused (%d): %s\n", what, rc, cse::LastError().c_str());
    return;
  }
  ExpectSamePlan(u, p, q.O, what);
}

// The refusals (cse.h, cse_residual_group): code and a message that names
// the field.
void Refuse(Problem* q, const cse_options& o, int want, const char* what) {
  cse::ProgramPlan P;
  EXPECT(cse::Validate(&q->d) == CSE_OK);
  // the check cse_create runs before it picks a device, and ValidateGroups
  const int rc0 = cse::ValidateLossData(&q->d, &o);
  const std::string msg0 = cse::LastError();
  const int rc1 = cse::ValidateGroups(&q->d, nullptr, &P, &o);
  const std::string msg1 = cse::LastError();
  std::printf("  refusal %-28s -> %d: %s\n", what, rc0, msg0.c_str());
  EXPECT(rc0 == want && rc1 == want);
  EXPECT(msg0.find("loss_data_size") != std::string::npos);
  EXPECT(msg1.find("loss_data_size") != std::string::npos);
}

void Refusals() {
  Problem q;
  Build(&q, 6, 40, 3, false, -1, false);
  SetPerBlock(&q, true);
  const cse_options o = DefaultOptions();
  const cse_residual_group good = q.g;
  {
    Planned p;
    EXPECT(Plan(q.d, o, &p) == CSE_OK);
  }
  for (int size : {1, 3, -2}) {
    q.g = good;
    q.g.loss_data_size = size;
    Refuse(&q, o, CSE_ERR_INVALID, "size other than 0 or 2");
  }
  q.g = good;
  q.g.loss.kind = CSE_LOSS_USER;
  Refuse(&q, o, CSE_ERR_UNSUPPORTED, "CSE_LOSS_USER");
  q.g = good;
  q.g.functor_kind = CSE_FUNCTOR_USER_FIRST + 2;
  Refuse(&q, o, CSE_ERR_UNSUPPORTED, "user functor kind");
  q.g = good;
  q.g.functor_kind = CSE_FUNCTOR_TEST_LINEAR_2_2_3;
  q.g.loss = cse_loss{CSE_LOSS_TRIVIAL, 0, 1.0, 1.0, {}};
  Refuse(&q, o, CSE_ERR_UNSUPPORTED, "TEST_* kind");
  q.g = good;
  q.g.loss = cse_loss{CSE_LOSS_TRIVIAL, 0, 1.0, 1.0, {}};
  Refuse(&q, o, CSE_ERR_INVALID, "unscaled trivial loss");
  q.g = good;
  cse_options jet = o;
  jet.jacobian_form = CSE_JACOBIAN_JET;
  Refuse(&q, jet, CSE_ERR_UNSUPPORTED, "CSE_JACOBIAN_JET");
  // ... and what stays accepted: the scaled trivial loss, Cauchy, unscaled Huber.
  for (const cse_loss& l : {cse_loss{CSE_LOSS_TRIVIAL, 1, 1.0, 3.0, {}}, cse_loss{CSE_LOSS_CAUCHY, 0, 2.0, 1.0, {}},
                            cse_loss{CSE_LOSS_HUBER, 0, 1.0, 1.0, {}}}) {
    q.g = good;
    q.g.loss = l;
    Planned p;
    EXPECT(Plan(q.d, o, &p) == CSE_OK);
  }
  // A uniform group under the Jet form is still fine.
  q.g = good;
  SetPerBlock(&q, false);
  Planned p;
  EXPECT(Plan(q.d, jet, &p) == CSE_OK);
}

}  // namespace

int main() {
  std::printf("per-block loss planner driver\n");
  Twin("Snavely BSM", 12, 300, 4, false, -1, false);
  Twin("Snavely CRS", 12, 300, 4, true, -1, false);
  Twin("Snavely BSM, held camera", 12, 300, 4, false, 3, false);
  Twin("Snavely CRS, held camera", 12, 300, 4, true, 3, false);
  Twin("Snavely BSM, general layout", 12, 300, 4, false, -1, false, true);
  Twin("Snavely BSM, 1 block", 6, 1, 1, false, -1, false);
  Twin("PointDisplacement BSM", 0, 200, 1, false, -1, true);
  Twin("PointDisplacement CRS", 0, 200, 1, true, -1, true);
  Refusals();
  if (g_failures) {
    std::printf("%d FAILED\n", g_failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
