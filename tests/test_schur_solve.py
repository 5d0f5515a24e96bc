"""CPU: cse_schur_solve's entry points, the numpy restatement of the
reference's conjugate gradients it is compared with, the scalar transitions
behind it, and the inputs of its GPU parity test.

cse_schur_solve (include/cse.h) is ConjugateGradientsSolver
(internal/ceres/conjugate_gradients_solver.h:108-305) over the device's Schur
operators, with every vector, scalar and stopping test on the device.  Here,
without a GPU: the symbols are exported, wrapped and declared and the ABI
version did not move; tests/cg_reference.py reproduces the reference's own two
known answers (tests/golden/cg_kat.json); the transitions of csrc/cg_state.hpp
pass their stand-alone driver under AddressSanitizer + UBSan
(tests/cpp/cg_state_driver.cpp); bundle_adjuster takes --device_pcg with
iterative_schur alone; and every case of the GPU parity test is a fair input:
on the oracle's Jacobian the float64 and the np.longdouble runs of
cg_reference end with the same termination type, reason and iteration count.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse

import cg_reference as R
import schur_solve_util as SU

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")


def ulps_apart(a, b):
    """The distance gtest's ASSERT_DOUBLE_EQ bounds by 4 (sign-magnitude to
    biased integers)."""
    def biased(x):
        u = int(np.float64(x).view(np.uint64))
        return (1 << 64) - u if u >> 63 else u | (1 << 63)
    return abs(biased(a) - biased(b))


def kat_cases():
    with open(os.path.join(HERE, "golden", "cg_kat.json")) as f:
        return json.load(f)["cases"]


def test_entry_points_are_exported_wrapped_and_declared():
    lib = C.CDLL(_cse.LIB_PATH)
    for name in ("cse_schur_solve", "cse_cg_default_options"):
        assert hasattr(lib, name), name
        assert name in _cse.SIGNATURES
    assert _cse.SIGNATURES["cse_schur_solve"][1] == [
        C.c_void_p, C.POINTER(_cse.cse_cg_options), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
        C.POINTER(_cse.cse_cg_summary)]
    assert callable(ca.Evaluator.schur_solve_device)
    with open(os.path.join(HERE, "..", "include", "cse.h")) as f:
        header = f.read()
    assert "int cse_schur_solve(cse_evaluator* ev, const cse_cg_options* options," in header
    assert "void cse_cg_default_options(cse_cg_options* options);" in header
    # in the ITERATIVE_SCHUR section, after cse_schur_explicit_multiply
    assert header.index("int cse_schur_explicit_multiply(") < header.index(
        "int cse_schur_solve(") < header.index("int cse_create_multi(")
    for name, value in (("CSE_CG_SUCCESS", _cse.CG_SUCCESS), ("CSE_CG_NO_CONVERGENCE", _cse.CG_NO_CONVERGENCE),
                        ("CSE_CG_FAILURE", _cse.CG_FAILURE),
                        ("CSE_CG_REASON_INDEFINITE", _cse.CG_REASON_INDEFINITE),
                        ("CSE_CG_REASON_R_TOLERANCE", _cse.CG_REASON_R_TOLERANCE)):
        assert f"{name} = {value}" in header
    assert "#define CSE_CG_ZERO_INITIAL_GUESS 1u" in header and _cse.CG_ZERO_INITIAL_GUESS == 1
    # the reference module numbers its outcomes as the header does
    assert (R.SUCCESS, R.NO_CONVERGENCE, R.FAILURE) == (_cse.CG_SUCCESS, _cse.CG_NO_CONVERGENCE,
                                                        _cse.CG_FAILURE)
    assert R.REASON_Q_TOLERANCE == _cse.CG_REASON_Q_TOLERANCE and R.REASON_RHO == _cse.CG_REASON_RHO


def test_struct_layouts_and_defaults():
    assert C.sizeof(_cse.cse_cg_options) == 40
    assert C.sizeof(_cse.cse_cg_summary) == 72
    assert _cse.cse_cg_summary.norm_rhs.offset == 24
    o = _cse.cg_options()
    assert (o.min_num_iterations, o.max_num_iterations, o.residual_reset_period, o.check_period) == (
        1, 500, 10, 1)
    assert (o.r_tolerance, o.q_tolerance, o.flags, o.reserved) == (-1.0, 0.0, 0, 0)
    assert _cse.cg_options(check_period=8).check_period == 8
    with pytest.raises(TypeError):
        _cse.cg_options(no_such_field=1)


def test_abi_version_is_still_6():
    assert _cse.lib().cse_abi_version() == 6 and _cse.CSE_ABI_VERSION == 6


def test_solve_refuses_bad_arguments_without_a_gpu():
    """The argument checks come before any HIP call."""
    L = _cse.lib()
    o, s = _cse.cg_options(), _cse.cse_cg_summary()
    assert L.cse_schur_solve(None, C.byref(o), None, 8, 16, None, C.byref(s)) == _cse.CSE_ERR_INVALID
    assert "null evaluator" in _cse.last_error()


def test_driver_takes_the_flags_with_iterative_schur_only():
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", "problem-16-22106"]
    args = bundle_adjuster.parse(base)
    assert not args.device_pcg and args.pcg_termination == "residual" and args.pcg_check_period == 1
    args = bundle_adjuster.parse(base + ["--device_pcg", "--pcg_check_period", "4"])
    assert args.device_pcg and args.pcg_check_period == 4
    args = bundle_adjuster.parse(base + ["--device_pcg", "--use_explicit_schur_complement",
                                         "--pcg_termination", "quadratic"])
    assert args.device_pcg and args.use_explicit_schur_complement and args.pcg_termination == "quadratic"
    for solver in ("dense_schur", "cgnr"):
        with pytest.raises(SystemExit, match="device_pcg"):
            bundle_adjuster.parse(base + ["--device_pcg", "--linear_solver", solver])
    with pytest.raises(SystemExit, match="needs --device_pcg"):
        bundle_adjuster.parse(base + ["--pcg_termination", "quadratic"])
    with pytest.raises(SystemExit, match="pcg_check_period"):
        bundle_adjuster.parse(base + ["--device_pcg", "--pcg_check_period", "0"])


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("case", kat_cases(), ids=lambda c: c["name"])
def test_cg_reference_reproduces_the_known_answers(case, dtype):
    """conjugate_gradients_solver_test.cc:47-152: termination SUCCESS and x to
    ASSERT_DOUBLE_EQ's 4 ulp (x rounded to double for np.longdouble)."""
    got = R.solve(case["A"], case["b"], case["x0"], R.Options(**case["options"]), None, dtype)
    assert got.termination_type == case["termination_type"] == R.SUCCESS
    assert got.reason == R.REASON_R_TOLERANCE
    if case["num_iterations"] is not None:
        assert got.num_iterations == case["num_iterations"]
    assert got.x.dtype == dtype
    for have, want in zip(got.x, case["x"]):
        assert ulps_apart(float(have), want) <= 4, (have, want)


def test_cg_reference_branches():
    """The outcomes the reference's text gives for the degenerate inputs."""
    eye = np.eye(3)
    got = R.solve(eye, np.zeros(3), np.full(3, np.nan))
    assert (got.termination_type, got.reason, got.num_iterations) == (R.SUCCESS, R.REASON_ZERO_RHS, 0)
    assert np.array_equal(got.x, np.zeros(3))
    x0 = np.array([1.0, -2.0, 0.5])
    got = R.solve(-eye, np.ones(3), x0, R.Options(1, 10, 10, 1e-9, 0.0))
    assert (got.termination_type, got.reason, got.num_iterations) == (R.NO_CONVERGENCE, R.REASON_INDEFINITE, 1)
    assert np.array_equal(got.x, x0)
    got = R.solve(eye, np.ones(3), np.ones(3), R.Options(0, 10, 10, 1e-9, 0.0))
    assert (got.termination_type, got.reason, got.num_iterations) == (R.SUCCESS, R.REASON_INITIAL_RESIDUAL, 0)
    got = R.solve(np.diag([1.0, 10.0, 100.0]), np.ones(3), None, R.Options(1, 2, 10, 1e-14, 0.0))
    assert (got.termination_type, got.reason, got.num_iterations) == (R.NO_CONVERGENCE, R.REASON_MAX_ITERATIONS, 2)
    got = R.solve(eye, np.ones(3), None, R.Options(4, 10, 10, 1e-3, 0.0))  # exact after 1, held to 4...
    # ... but r = 0 after the first iteration, so the second ends on rho = 0
    assert (got.termination_type, got.reason, got.num_iterations) == (R.FAILURE, R.REASON_RHO, 2)


def test_cg_state_driver_under_asan_ubsan():
    """The stand-alone driver, g++ -fsanitize=address,undefined with static
    runtimes: csrc/cg_state.hpp's transitions under host loops on small SPD
    systems, through every branch with crafted scalars, and frozen after
    `done`."""
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "cg_state.mk", "driver"])
    out = subprocess.run([os.path.join(CPP, "build", "cg_state_driver")], capture_output=True, text=True)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0
    assert out.stdout.rstrip().endswith("OK")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


@pytest.mark.parametrize("which,precond,option_set", SU.CASES)
def test_parity_cases_do_not_sit_on_a_threshold(which, precond, option_set):
    """Every case of tests/test_schur_solve_gpu.py's parity test: float64 and
    np.longdouble end alike.  d_ref, the gap between their solutions, is what
    the order of a sum may change; the GPU test allows ten times it."""
    prog, J, e_cols, D, S, rhs = SU.oracle_inputs(which)
    Minv = SU.dense_preconditioner(precond, S, J, e_cols, D)
    ref = SU.reference(S, Minv, rhs, option_set)
    print(f"{which} precond {precond} {option_set}: type {ref.ld.termination_type} reason {ref.ld.reason} "
          f"iterations {ref.ld.num_iterations} d_ref {ref.d_ref:.3e}")
    assert SU.same_outcome(ref.f64, ref.ld), (ref.f64[1:4], ref.ld[1:4])
    o = SU.OPTION_SETS[option_set].options
    if option_set == "max4":
        assert (ref.ld.termination_type, ref.ld.num_iterations) == (R.NO_CONVERGENCE, 4)
    if option_set == "min6":
        assert ref.ld.num_iterations >= o.min_num_iterations
