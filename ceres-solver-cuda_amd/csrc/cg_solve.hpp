// cg_solve.hpp -- the host loop that cse_schur_solve (schur_operators.hip) and
// cse_cgnr_solve (linear_operators.hip) share: the reference's conjugate
// gradients on the device (cg_state.hpp; the vector kernels through
// cg_kernels.h).  Host only: it defines no kernel.
#ifndef CSE_CG_SOLVE_HPP_
#define CSE_CG_SOLVE_HPP_

#include <string>

#include "cg_kernels.h"
#include "evaluator.hpp"

namespace cse {

// The loop of conjugate_gradients_solver.h:108-305 over any operator and either
// set of vector kernels: `op(x, y)` enqueues y = A x on the stream `s` and
// returns a cse status; `L` launches the vector kernels over its arguments
// L.a through four members,
//     void Init(bool zero_guess, hipStream_t) const;
//     void InitialResidual(hipStream_t) const;
//     void Direction(hipStream_t) const;
//     void Update(CgUpdateMode, hipStream_t) const;
// (SchurCgLaunch: cg_kernels.hpp's one-workgroup kernels; CgnrCgLaunch:
// cg_sliced_kernels.hpp's).  The host enqueues check_period iterations, copies
// the state to pinned memory, waits once and stops or goes on; it computes no
// scalar of the iteration.  Nothing is allocated here.
template <class Launch, class Op>
int CgSolve(const char* what, const Launch& L, const cse_cg_options& o, CgState* state_host, hipStream_t s,
            Op&& op, cse_cg_summary* summary) {
  const auto& a = L.a;
  int rc;
  int32_t syncs = 0, enqueued = 0;
  auto look = [&]() -> int {
    CSE_HIP(hipMemcpyAsync(state_host, a.state, sizeof(CgState), hipMemcpyDeviceToHost, s));
    CSE_HIP(hipStreamSynchronize(s));
    ++syncs;
    return CSE_OK;
  };
  const bool zero_guess = (o.flags & CSE_CG_ZERO_INITIAL_GUESS) != 0;
  L.Init(zero_guess, s);
  if (!zero_guess) {
    if ((rc = op((const double*)a.x, a.tmp))) return rc;
    L.InitialResidual(s);
  }
  CSE_HIP(hipGetLastError());
  // |b| = 0 and convergence before the first iteration end here.
  if ((rc = look())) return rc;
  for (int32_t it = 1; !state_host->done && it <= o.max_num_iterations; ++it) {
    L.Direction(s);
    if ((rc = op((const double*)a.p, a.z))) return rc;
    if (it % o.residual_reset_period == 0) {
      L.Update(kCgUpdateX, s);
      if ((rc = op((const double*)a.x, a.tmp))) return rc;
      L.Update(kCgUpdateReset, s);
    } else {
      L.Update(kCgUpdateFull, s);
    }
    CSE_HIP(hipGetLastError());
    ++enqueued;
    if (enqueued % o.check_period == 0 || it == o.max_num_iterations)
      if ((rc = look())) return rc;
  }
  const CgState& st = *state_host;
  if (!st.done) return Fail(CSE_ERR_HIP, std::string(what) + ": the device state did not terminate");
  summary->termination_type = st.termination_type;
  summary->reason = st.reason;
  summary->num_iterations = st.iteration;
  summary->num_iterations_enqueued = enqueued;
  summary->num_synchronizations = syncs;
  summary->reserved = 0;
  summary->norm_rhs = st.norm_rhs;
  summary->norm_r = st.norm_r;
  summary->q = st.Q1;
  summary->zeta = st.zeta;
  summary->rho = st.rho;
  summary->pq = st.pq;
  return CSE_OK;
}

// The argument checks cse_schur_solve and cse_cgnr_solve share.
inline int CgArgumentCheck(const char* what, const cse_cg_options* options, const double* d_rhs,
                           const double* d_x, const cse_cg_summary* summary) {
  const std::string w = std::string(what) + ": ";
  if (!options || !summary || !d_rhs || !d_x)
    return Fail(CSE_ERR_INVALID, w + "null options, summary, d_rhs or d_x");
  const cse_cg_options& o = *options;
  if (o.check_period < 1) return Fail(CSE_ERR_INVALID, w + "check_period is below 1");
  if (o.residual_reset_period < 1) return Fail(CSE_ERR_INVALID, w + "residual_reset_period is below 1");
  if (o.max_num_iterations < 1) return Fail(CSE_ERR_INVALID, w + "max_num_iterations is below 1");
  if (o.min_num_iterations < 0) return Fail(CSE_ERR_INVALID, w + "min_num_iterations is negative");
  if (o.reserved != 0) return Fail(CSE_ERR_INVALID, w + "options.reserved is not 0");
  if (o.flags & ~CSE_CG_ZERO_INITIAL_GUESS) return Fail(CSE_ERR_INVALID, w + "unknown flags");
  return CSE_OK;
}

}  // namespace cse

#endif  // CSE_CG_SOLVE_HPP_
