// spse_state.hpp -- the scalar logic of PowerSeriesExpansionPreconditioner::
// RightMultiplyAndAccumulate (internal/ceres/power_series_expansion_
// preconditioner.cc:51-72) as transitions of one small struct, in plain C++
// for the host and the device alike (as cg_state.hpp is for the PCG).
//
// cse_schur_power_series keeps this struct in device memory: lane 0 of the
// series' vector kernels (spse_kernels.hpp) calls a transition after each
// norm, and every later kernel of the series reads `done` from it.
// tests/cpp/spse_state_driver.cpp drives the same functions with host loops.
//
// Once `done` is set SpseTerm returns without touching the state: the terms
// the host enqueued past the end change nothing (the frozen rule).
#ifndef CSE_SPSE_STATE_HPP_
#define CSE_SPSE_STATE_HPP_

#include <cstdint>

#include "cg_state.hpp"

namespace cse {

struct SpseState {
  double threshold;   // spse_tolerance * |P^-1 x| (:59)
  double norm_first;  // |P^-1 x|
  double norm_last;   // |the last term added|
  int32_t num_terms;  // terms added after the zeroth
  int32_t done;
};

// :55-59, after y = prev = P^-1 x: norm = |y|.
CSE_CG_HD void SpseBegin(SpseState* s, double norm, double tolerance) {
  s->threshold = tolerance * norm;
  s->norm_first = norm;
  s->norm_last = norm;
  s->num_terms = 0;
  s->done = 0;
}

// :61-70, after y += term: norm = |term|, the term being number
// num_terms + 1.  Returns true when the series goes on.
CSE_CG_HD bool SpseTerm(SpseState* s, double norm, int32_t max_num_iterations) {
  if (s->done) return false;
  s->num_terms += 1;
  s->norm_last = norm;
  if (s->num_terms >= max_num_iterations || norm < s->threshold) {
    s->done = 1;
    return false;
  }
  return true;
}

}  // namespace cse

#endif  // CSE_SPSE_STATE_HPP_
