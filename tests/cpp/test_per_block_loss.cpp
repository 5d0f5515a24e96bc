// Per-block loss objects through the C++ facade (ceres_amd/problem_cuda.h,
// EvaluatorCUDA::Options::merge_loss_parameters) against the CPU oracle: 300
// Snavely residual blocks, each added with its own
// ScaledLossCUDA<HuberLossCUDA>(HuberLossCUDA(a_i), w_i) -- the ordinary way
// to carry per-observation weights -- with 12 distinct (a_i, w_i) values.
//   merge_loss_parameters = true:  one group, per-block (a, scale) rows;
//   merge_loss_parameters = false: one group per distinct value (12).
// Both against the oracle, which takes the loss per block.  Tolerances: those
// of tests/parity_util.py (isApprox 1e-13 per vector, the per-element bound
// 1e-10 |y_i| + 1e-13 max|y|, cost 1e-12 relative).
//
// Needs a GPU (run by tests/test_per_block_loss_facade_gpu.py under -m gpu).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <vector>

#include "ceres_amd/problem_cuda.h"
#include "oracle.h"

using namespace ceres_amd;

static int failures = 0;
#define EXPECT(cond)                                                 \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static bool Parity(const std::vector<double>& x, const std::vector<double>& y, const char* what) {
  if (x.size() != y.size()) return false;
  double d = 0, nx = 0, ny = 0, ymax = 0;
  for (size_t i = 0; i < x.size(); ++i) {
    d += (x[i] - y[i]) * (x[i] - y[i]);
    nx += x[i] * x[i];
    ny += y[i] * y[i];
    ymax = std::max(ymax, std::fabs(y[i]));
  }
  bool ok = std::sqrt(d) <= 1e-13 * std::sqrt(std::min(nx, ny));
  double worst = 0;
  for (size_t i = 0; i < x.size(); ++i)
    worst = std::max(worst, std::fabs(x[i] - y[i]) / (1e-10 * std::fabs(y[i]) + 1e-13 * ymax));
  ok = ok && worst <= 1.0;
  std::printf("  %-10s |x - y| / |y| = %.3e, per-element bound ratio %.3f\n", what,
              std::sqrt(d) / std::sqrt(ny), worst);
  return ok;
}

static uint64_t lcg = 0x2545F4914F6CDD1Dull;
static double Uniform() {
  lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(lcg >> 11) * (1.0 / 9007199254740992.0);
}

constexpr int kCameras = 8, kPoints = 60, kBlocks = 300;
static double cameras[kCameras][9];
static double points[kPoints][3];

// The 25th, 50th and 75th percentile of the blocks' unrobustified residual
// norms (oracle, apply_loss_function 0): widths that put both Huber branches
// in every run by construction.
static void Percentiles(oracle_program op, const std::vector<double>& state, double out[3]) {
  op.apply_loss_function = 0;
  double cost = 0, none = 0;
  std::vector<double> r(2 * kBlocks), norms(kBlocks);
  EXPECT(oracle_evaluate(&op, state.data(), &none, 1, &cost, r.data(), nullptr, nullptr) == 1);
  for (int i = 0; i < kBlocks; ++i) norms[i] = std::sqrt(r[2 * i] * r[2 * i] + r[2 * i + 1] * r[2 * i + 1]);
  std::sort(norms.begin(), norms.end());
  for (int k = 0; k < 3; ++k) out[k] = norms[(k + 1) * kBlocks / 4];
}

static void Run(bool merge, JacobianFormat format, int want_groups) {
  const bool crs = format == JacobianFormat::kCompressedRow;
  const double weights[4] = {0.25, 1.0, 2.0, 4.0};
  // The reduced program for the oracle; program order: the points (the
  // elimination group), then the cameras.
  std::vector<int32_t> params, lk(kBlocks, ORACLE_LOSS_HUBER), lsd(kBlocks, 1), kind(kBlocks, ORACLE_SNAVELY_2_9_3);
  std::vector<double> la(kBlocks, 1.0), ls(kBlocks, 1.0), data;
  std::vector<int64_t> pbeg = {0}, dbeg = {0};
  lcg = 0x2545F4914F6CDD1Dull;
  for (int i = 0; i < kBlocks; ++i) {
    const int p = i / 5, c = (i * 3 + p) % kCameras;  // point-major: Schur order
    params.push_back(kPoints + c);
    params.push_back(p);
    pbeg.push_back((int64_t)params.size());
    data.push_back(200.0 * (Uniform() - 0.5));
    data.push_back(200.0 * (Uniform() - 0.5));
    dbeg.push_back((int64_t)data.size());
  }
  std::vector<int32_t> pb_size, pb_const(kPoints + kCameras, 0);
  for (int p = 0; p < kPoints; ++p) pb_size.push_back(3);
  for (int c = 0; c < kCameras; ++c) pb_size.push_back(9);
  std::vector<int64_t> pb_pj(kPoints + kCameras, -1);
  double no_pj = 0;
  oracle_program op{kPoints + kCameras, pb_size.data(), pb_size.data(), pb_const.data(), pb_pj.data(), &no_pj,
                    kBlocks, kind.data(), lk.data(), la.data(), ls.data(), lsd.data(), pbeg.data(),
                    params.data(), dbeg.data(), data.data(),
                    crs ? ORACLE_COMPRESSED_ROW : ORACLE_BLOCK_SPARSE, kPoints, 1, nullptr};
  std::vector<double> ostate;
  for (int p = 0; p < kPoints; ++p) ostate.insert(ostate.end(), points[p], points[p] + 3);
  for (int c = 0; c < kCameras; ++c) ostate.insert(ostate.end(), cameras[c], cameras[c] + 9);
  double widths[3];
  Percentiles(op, ostate, widths);
  std::printf("  Huber widths %.3f %.3f %.3f\n", widths[0], widths[1], widths[2]);

  ProblemCUDA problem;
  std::vector<double*> elim;
  for (int p = 0; p < kPoints; ++p) {
    problem.AddParameterBlock(points[p], 3);
    elim.push_back(points[p]);
  }
  for (int c = 0; c < kCameras; ++c) problem.AddParameterBlock(cameras[c], 9);
  problem.SetEliminationGroup(elim);
  for (int i = 0; i < kBlocks; ++i) {
    la[i] = widths[i % 3];
    ls[i] = weights[i % 4];
    const ScaledLossCUDA<HuberLossCUDA> loss(HuberLossCUDA(la[i]), ls[i]);
    problem.AddResidualBlock<SnavelyReprojectionError, 2, 9, 3>(
        SnavelyReprojectionError(data[2 * i], data[2 * i + 1]), &loss, cameras[params[2 * i] - kPoints],
        points[params[2 * i + 1]]);
  }
  EvaluatorCUDA::Options options;
  options.format = format;
  options.merge_loss_parameters = merge;
  EvaluatorCUDA evaluator(problem, options);
  std::printf("%s merge_loss_parameters=%d: %d group(s)\n", crs ? "CRS" : "BSM", (int)merge,
              evaluator.NumGroups());
  EXPECT(evaluator.NumGroups() == want_groups);
  EXPECT(evaluator.NumResidualBlocks() == kBlocks && evaluator.NumResiduals() == 2 * kBlocks);
  std::vector<double> state(evaluator.NumParameters());
  evaluator.ParameterBlocksToStateVector(state.data());
  double cost = -1;
  std::vector<double> r(2 * kBlocks), g(evaluator.NumEffectiveParameters());
  std::vector<double> J(evaluator.NumJacobianValues(), -1.0);
  EXPECT(evaluator.Evaluate(state.data(), &cost, r.data(), g.data(), J.data()));

  oracle_sizes sz;
  EXPECT(oracle_sizes_of(&op, &sz) == 0);
  EXPECT(sz.num_jacobian_values == evaluator.NumJacobianValues());
  EXPECT(sz.num_parameters == evaluator.NumParameters());
  EXPECT(ostate == state);
  double ocost = -1, none = 0;
  std::vector<double> orr(2 * kBlocks), og(sz.num_effective_parameters), oJ(sz.num_jacobian_values);
  EXPECT(oracle_evaluate(&op, ostate.data(), &none, 1, &ocost, orr.data(), og.data(), oJ.data()) == 1);
  std::printf("  cost %.15e (oracle %.15e)\n", cost, ocost);
  EXPECT(std::fabs(cost - ocost) <= 1e-12 * std::fabs(ocost));
  EXPECT(Parity(r, orr, "residuals"));
  EXPECT(Parity(g, og, "gradient"));
  EXPECT(Parity(J, oJ, "jacobian"));
  // Both Huber branches occur: the unrobustified block norms against a_i.
  oracle_program raw = op;
  raw.apply_loss_function = 0;
  std::vector<double> rr(2 * kBlocks);
  EXPECT(oracle_evaluate(&raw, ostate.data(), &none, 1, &ocost, rr.data(), nullptr, nullptr) == 1);
  int outliers = 0;
  for (int i = 0; i < kBlocks; ++i)
    outliers += rr[2 * i] * rr[2 * i] + rr[2 * i + 1] * rr[2 * i + 1] > la[i] * la[i];
  std::printf("  %d of %d blocks past their Huber width\n", outliers, kBlocks);
  EXPECT(outliers >= kBlocks / 10 && outliers <= kBlocks - kBlocks / 10);
}

int main() {
  for (auto& cam : cameras) {
    const double v[9] = {0.1 * (Uniform() - 0.5), 0.1 * (Uniform() - 0.5), 0.1 * (Uniform() - 0.5),
                         Uniform() - 0.5,         Uniform() - 0.5,         -10.0 + Uniform(),
                         400.0 + 800.0 * Uniform(), 0.01 * (Uniform() - 0.5), 0.001 * Uniform()};
    std::copy(v, v + 9, cam);
  }
  for (auto& pt : points)
    for (double& x : pt) x = 6.0 * Uniform() - 3.0;
  Run(true, JacobianFormat::kBlockSparse, 1);
  Run(true, JacobianFormat::kCompressedRow, 1);
  Run(false, JacobianFormat::kBlockSparse, 12);  // 3 widths x 4 weights, as before
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
