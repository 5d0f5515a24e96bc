"""CPU: cse_schur_power_series' entry points, the numpy restatement of the
reference's power series expansion it is compared with, the scalar transitions
behind it, and the inputs of its GPU parity test.

cse_schur_power_series (include/cse.h) is PowerSeriesExpansionPreconditioner::
RightMultiplyAndAccumulate (internal/ceres/power_series_expansion_
preconditioner.cc:51-72) over the device's Schur passes.  Here, without a GPU:
the symbols and the constant are exported, wrapped and declared and the ABI
version did not move; the transitions of csrc/spse_state.hpp pass their
stand-alone driver under AddressSanitizer + UBSan (tests/cpp/
spse_state_driver.cpp); bundle_adjuster's parse refuses what the reference
refuses; and every case of the GPU test is a fair input: on the oracle's
Jacobian the float64 and np.longdouble runs of tests/spse_reference.py add the
same number of terms, no term norm lies near its threshold, the long series is
S^-1, the dense preconditioner M_m is symmetric, and cg_reference under M_m
(and from the series' start) ends alike in both precisions.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse

import cg_reference as R
import schur_solve_util as SU
import spse_reference as P

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
LD = np.longdouble

# (max_num_iterations, tolerance) -> the range of terms observed over the six problems
SERIES = {(5, 0.0): (5, 5), (5, 0.1): (1, 2), (50, 1e-3): (7, 11), (500, 1e-14): (51, 77)}
# The PCG option sets under M_m on which cg_reference ends alike in float64 and
# np.longdouble ("resets" is IDENTITY's; "min6" at m = 5 runs six iterations,
# past float64's precision, and on "bal" the two precisions end differently).
PCG_SETS = {1: ("lm", "max4", "min6", "guess", "zero"), 5: ("lm", "max4", "guess", "zero")}
SPSE_START = (5, 0.1)  # bundle_adjuster's defaults for --use_spse_initialization


@functools.lru_cache(maxsize=None)
def inputs(which):
    """(S, rhs, Pinv, Q): SU.oracle_inputs' dense S and reduced rhs, and the
    series' operators in np.longdouble."""
    prog, J, e_cols, D, S, rhs = SU.oracle_inputs(which)
    Pinv, Q = P.operators(S, J, e_cols, D, LD)
    return S, rhs, Pinv, Q


@functools.lru_cache(maxsize=None)
def dense_preconditioner(which, m):
    """M_m in float64, as SU.dense_preconditioner's matrices are: cg_reference
    runs in both precisions on the same float64 inputs."""
    S, rhs, Pinv, Q = inputs(which)
    return P.dense_preconditioner(Pinv, Q, m, np.float64)


def solve_longdouble(S, rhs):
    """S^-1 rhs in np.longdouble: float64's solve, refined."""
    A = S.astype(LD)
    x = np.linalg.solve(S, rhs).astype(LD)
    for _ in range(3):
        x = x + np.linalg.solve(S, (rhs.astype(LD) - A @ x).astype(np.float64)).astype(LD)
    return x


def rel(a, b):
    return float(np.linalg.norm((a - b).astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


# --------------------------------------------------------------------------
# The library surface (fails without the feature).
# --------------------------------------------------------------------------
def test_entry_points_are_exported_wrapped_and_declared():
    lib = C.CDLL(_cse.LIB_PATH)
    for name in ("cse_schur_power_series", "cse_schur_set_spse_iterations"):
        assert hasattr(lib, name), name
        assert name in _cse.SIGNATURES
    assert _cse.SCHUR_POWER_SERIES_EXPANSION == 3
    assert _cse.SIGNATURES["cse_schur_power_series"][1] == [
        C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(_cse.cse_spse_summary)]
    assert _cse.SIGNATURES["cse_schur_set_spse_iterations"][1] == [C.c_void_p, C.c_int32]
    assert C.sizeof(_cse.cse_spse_summary) == 24
    assert [f[0] for f in _cse.cse_spse_summary._fields_] == ["num_terms", "reserved", "norm_first", "norm_last"]
    assert callable(ca.Evaluator.schur_power_series_device)
    assert callable(ca.Evaluator.schur_set_spse_iterations)
    with open(os.path.join(HERE, "..", "include", "cse.h")) as f:
        header = f.read()
    assert "CSE_SCHUR_POWER_SERIES_EXPANSION = 3" in header
    assert "int cse_schur_power_series(cse_evaluator* ev, int32_t max_num_iterations, double tolerance," in header
    assert "int cse_schur_set_spse_iterations(cse_evaluator* ev, int32_t max_num_iterations);" in header
    assert "typedef struct cse_spse_summary {" in header
    assert _cse.lib().cse_abi_version() == 6  # new symbols and one enum value: no struct changed


def test_null_evaluator_is_refused_without_a_gpu():
    L = _cse.lib()
    assert L.cse_schur_power_series(None, 5, 0.0, None, None, None) == _cse.CSE_ERR_INVALID
    assert "null evaluator" in _cse.last_error()
    assert L.cse_schur_set_spse_iterations(None, 5) == _cse.CSE_ERR_INVALID
    assert "null evaluator" in _cse.last_error()


def test_state_transitions_under_sanitizers():
    """csrc/spse_state.hpp driven on the host against a plain restatement of the
    reference's loop (tests/cpp/spse_state_driver.cpp), under ASan + UBSan."""
    exe = os.path.join(CPP, "build", "spse_state_driver")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", CPP, "-f", "spse_state.mk", "driver"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "spse_state_driver: ok" in out.stdout


def test_parse_refusals():
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", "problem-16-22106"]
    series = ["--preconditioner", "schur_power_series_expansion"]
    args = bundle_adjuster.parse(base + series + ["--max_num_spse_iterations", "3", "--device_pcg"])
    assert args.preconditioner == "schur_power_series_expansion" and args.max_num_spse_iterations == 3
    args = bundle_adjuster.parse(base + ["--use_spse_initialization", "--held_cameras", "2"])
    assert args.use_spse_initialization and args.spse_tolerance == 0.1 and args.max_num_spse_iterations == 5
    args = bundle_adjuster.parse(base)
    assert not args.use_spse_initialization and args.preconditioner == "jacobi"
    for bad in (series + ["--use_explicit_schur_complement"],
                ["--use_spse_initialization", "--use_explicit_schur_complement"],
                series + ["--linear_solver", "cgnr"],
                series + ["--linear_solver", "dense_schur"],
                ["--use_spse_initialization", "--linear_solver", "cgnr"],
                ["--use_spse_initialization", "--linear_solver", "dense_schur"],
                series + ["--max_num_spse_iterations", "0"],
                ["--use_spse_initialization", "--spse_tolerance", "-1"],
                ["--use_spse_initialization", "--spse_tolerance", "inf"],
                ["--use_spse_initialization", "--spse_tolerance", "nan"]):
        with pytest.raises(SystemExit):
            bundle_adjuster.parse(base + bad)


# --------------------------------------------------------------------------
# The GPU test's inputs are fair.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("which", SU.PROBLEMS)
def test_term_counts_agree_and_no_norm_is_near_its_threshold(which):
    S, rhs, Pinv, Q = inputs(which)
    for (mx, tol), (lo, hi) in SERIES.items():
        f64 = P.series(Pinv, Q, rhs, mx, tol, np.float64)
        ld = P.series(Pinv, Q, rhs, mx, tol, LD)
        threshold = LD(tol) * ld.norms[0]
        gap = min((abs(float((n - threshold) / threshold)) for n in ld.norms[1:]), default=np.inf) if tol else np.inf
        print(f"{which} ({mx}, {tol:g}): {f64.num_terms} / {ld.num_terms} terms, closest norm to the "
              f"threshold {gap:.2e} relative")
        assert f64.num_terms == ld.num_terms
        assert lo <= ld.num_terms <= hi
        assert gap > 1e-6  # the GPU's count may not hang on rounding
        assert rel(f64.y.astype(LD), ld.y) < 1e-13


@pytest.mark.parametrize("which", SU.PROBLEMS)
def test_long_series_is_the_inverse_and_short_ones_are_not(which):
    """power_series_expansion_preconditioner_test.cc's known answer: the series
    run to a tolerance of 1e-14 is S^-1; its two bad cases, one term and a
    tolerance of 1 / 1e-14, are far from it."""
    S, rhs, Pinv, Q = inputs(which)
    want = solve_longdouble(S, rhs)
    good = rel(P.series(Pinv, Q, rhs, 500, 1e-14, LD).y, want)
    G = Pinv.astype(np.float64) @ Q.astype(np.float64)
    rho = float(np.max(np.abs(np.linalg.eigvals(G))))
    bad = [rel(P.series(Pinv, Q, rhs, 1, 1e-14, LD).y, want), rel(P.series(Pinv, Q, rhs, 50, 1e14, LD).y, want)]
    print(f"{which}: spectral radius of P^-1 Q {rho:.3f}; (500, 1e-14) is {good:.2e} from S^-1 rhs, "
          f"(1, 1e-14) {bad[0]:.2e}, (50, 1e14) {bad[1]:.2e}")
    assert good <= 2e-14
    assert min(bad) > 1e-3


@pytest.mark.parametrize("which", SU.PROBLEMS)
def test_dense_preconditioner_is_symmetric(which):
    S, rhs, Pinv, Q = inputs(which)
    for m in (1, 5):
        M = dense_preconditioner(which, m)
        asym = float(np.linalg.norm(M - M.T) / np.linalg.norm(M))
        print(f"{which} m {m}: |M - M'| / |M| {asym:.2e}")
        assert asym <= 1e-15
        # ... and it is the series with m terms and tolerance 0
        assert rel((M @ rhs).astype(LD), P.series(Pinv, Q, rhs, m, 0.0, LD).y) < 1e-13


@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("which", SU.PROBLEMS)
def test_cg_reference_agrees_with_itself_under_the_series(which, m):
    S, rhs, Pinv, Q = inputs(which)
    Minv = dense_preconditioner(which, m)
    for option_set in PCG_SETS[m]:
        ref = SU.reference(S, Minv, rhs, option_set)
        print(f"{which} m {m} {option_set}: {ref.f64[1:4]} / {ref.ld[1:4]} d_ref {ref.d_ref:.2e}")
        assert SU.same_outcome(ref.f64, ref.ld), option_set
        if option_set == "zero":  # r_tolerance 1e-6: JACOBI takes 9-10
            assert ref.ld.num_iterations in ((3, 4) if m == 5 else (6, 7))


@pytest.mark.parametrize("which", SU.PROBLEMS)
def test_jacobi_from_the_series_start_agrees_with_itself(which):
    prog, J, e_cols, D, S, rhs = SU.oracle_inputs(which)
    _, _, Pinv, Q = inputs(which)
    x0 = P.series(Pinv, Q, rhs, *SPSE_START, LD).y
    Minv = SU.dense_preconditioner(_cse.SCHUR_JACOBI, S, J, e_cols, D)
    o = SU.OPTION_SETS["guess"].options
    f64 = R.solve(S, rhs, x0, o, Minv, np.float64)
    ld = R.solve(S, rhs, x0, o, Minv, LD)
    print(f"{which}: {f64[1:4]} / {ld[1:4]}")
    assert SU.same_outcome(f64, ld)
    assert ld.num_iterations in (6, 7)
