"""CPU: CGNR on the device -- cse_cgnr_init, cse_cgnr_precondition and
cse_cgnr_solve (include/cse.h), CudaCgnrSolver (internal/ceres/cgnr_solver.cc:
218-387) over the evaluator's Jacobian values.

Here, without a GPU: the symbols are exported, wrapped and declared, and their
argument checks come before any HIP call; the ABI version did not move;
bundle_adjuster takes --device_cgnr with cgnr alone; the preconditioner's
block table (cse::PlanCgnrBlocks) passes its stand-alone driver under
AddressSanitizer + UBSan (tests/cpp/cgnr_plan_driver.cpp); and every case of
the GPU parity test is a fair input: on the oracle's Jacobian the float64 and
the np.longdouble runs of tests/cg_reference.py end with the same termination
type, reason and iteration count.
"""
import ctypes as C
import os
import subprocess

import pytest

import ceres_amd as ca
from ceres_amd import _cse

import cg_reference as R
import cgnr_solve_util as CU

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")


def test_entry_points_are_exported_wrapped_and_declared():
    lib = C.CDLL(_cse.LIB_PATH)
    for name in ("cse_cgnr_init", "cse_cgnr_precondition", "cse_cgnr_solve"):
        assert hasattr(lib, name), name
        assert name in _cse.SIGNATURES
    assert _cse.SIGNATURES["cse_cgnr_init"][1] == [C.c_void_p] * 5 + [C.c_int]
    assert _cse.SIGNATURES["cse_cgnr_precondition"][1] == [C.c_void_p] * 3
    assert _cse.SIGNATURES["cse_cgnr_solve"][1] == [
        C.c_void_p, C.POINTER(_cse.cse_cg_options), C.c_void_p, C.c_void_p, C.POINTER(_cse.cse_cg_summary)]
    for method in ("cgnr_init_device", "cgnr_precondition_device", "cgnr_solve_device"):
        assert callable(getattr(ca.Evaluator, method)), method
    with open(os.path.join(HERE, "..", "include", "cse.h")) as f:
        header = f.read()
    assert "int cse_cgnr_init(cse_evaluator* ev, const double* d_jacobian_values, const double* d_D," in header
    assert "int cse_cgnr_precondition(cse_evaluator* ev, const double* d_x, double* d_y);" in header
    assert "int cse_cgnr_solve(cse_evaluator* ev, const cse_cg_options* options, const double* d_rhs," in header
    assert "enum cse_cgnr_preconditioner { CSE_CGNR_IDENTITY = 0, CSE_CGNR_JACOBI = 1 };" in header
    assert (_cse.CGNR_IDENTITY, _cse.CGNR_JACOBI) == (0, 1)
    # after cse_schur_solve, whose options and summary it shares
    assert header.index("int cse_schur_solve(") < header.index("int cse_cgnr_init(") < header.index(
        "int cse_cgnr_solve(") < header.index("int cse_create_multi(")
    # the comments cite the reference
    assert "cgnr_solver.cc:218-387" in header and "block_jacobi_preconditioner.cc" in header


def test_abi_version_is_still_6():
    assert _cse.lib().cse_abi_version() == 6 and _cse.CSE_ABI_VERSION == 6


def test_calls_refuse_bad_arguments_without_a_gpu():
    """The argument checks come before any HIP call."""
    L = _cse.lib()
    o, s = _cse.cg_options(), _cse.cse_cg_summary()
    assert L.cse_cgnr_init(None, 8, None, None, None, _cse.CGNR_JACOBI) == _cse.CSE_ERR_INVALID
    assert "null evaluator" in _cse.last_error()
    assert L.cse_cgnr_precondition(None, 8, 16) == _cse.CSE_ERR_INVALID
    assert "null evaluator" in _cse.last_error()
    assert L.cse_cgnr_solve(None, C.byref(o), 8, 16, C.byref(s)) == _cse.CSE_ERR_INVALID
    assert "null evaluator" in _cse.last_error()


def test_driver_takes_the_flags_with_cgnr_only():
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", "problem-16-22106"]
    args = bundle_adjuster.parse(base + ["--linear_solver", "cgnr"])
    assert not args.device_cgnr and args.cgnr_preconditioner == "jacobi" and args.cgnr_check_period == 1
    args = bundle_adjuster.parse(base + ["--linear_solver", "cgnr", "--device_cgnr", "--cgnr_check_period", "4",
                                         "--cgnr_preconditioner", "identity"])
    assert args.device_cgnr and args.cgnr_check_period == 4 and args.cgnr_preconditioner == "identity"
    # with held cameras and Jacobi scaling too
    args = bundle_adjuster.parse(base + ["--linear_solver", "cgnr", "--device_cgnr", "--held_cameras", "2",
                                         "--jacobi_scaling"])
    assert args.device_cgnr and args.held_cameras == 2
    for solver in (["--linear_solver", "iterative_schur"], ["--linear_solver", "dense_schur"], []):
        with pytest.raises(SystemExit, match="device_cgnr"):
            bundle_adjuster.parse(base + ["--device_cgnr"] + solver)
    with pytest.raises(SystemExit, match="cgnr_check_period"):
        bundle_adjuster.parse(base + ["--linear_solver", "cgnr", "--device_cgnr", "--cgnr_check_period", "0"])
    with pytest.raises(SystemExit):
        bundle_adjuster.parse(base + ["--linear_solver", "cgnr", "--cgnr_preconditioner", "schur_jacobi"])
    # --device_pcg stays the Schur solver's
    with pytest.raises(SystemExit, match="device_pcg"):
        bundle_adjuster.parse(base + ["--device_pcg", "--linear_solver", "cgnr"])


def test_cgnr_plan_driver_under_asan_ubsan():
    """The stand-alone driver, g++ -fsanitize=address,undefined with static
    runtimes: the block table against brute force on mixed block sizes,
    constant blocks in the middle, blocks out of delta order, a gap, an
    overlap, an oversize block and an empty program."""
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "cgnr_plan.mk", "driver"])
    out = subprocess.run([os.path.join(CPP, "build", "cgnr_plan_driver")], capture_output=True, text=True)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0
    assert out.stdout.rstrip().endswith("OK")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    for case in ("mixed sizes", "constant blocks in the middle", "a gap", "an oversize block", "an empty program"):
        assert case in out.stdout
    assert "refused (does not tile)" in out.stdout and "refused (oversize)" in out.stdout


@pytest.mark.parametrize("which,precond,option_set", CU.CASES)
def test_parity_cases_do_not_sit_on_a_threshold(which, precond, option_set):
    """Every case of tests/test_cgnr_solve_gpu.py's parity test: float64 and
    np.longdouble end alike.  d_ref, the gap between their solutions, is what
    the order of a sum may change; the GPU test allows ten times it."""
    c = CU.oracle_inputs(which, precond)
    ref = CU.reference(c.A, c.Minv, c.rhs, option_set)
    print(f"{which} precond {precond} {option_set}: type {ref.ld.termination_type} reason {ref.ld.reason} "
          f"iterations {ref.ld.num_iterations} d_ref {ref.d_ref:.3e}")
    assert CU.same_outcome(ref.f64, ref.ld), (ref.f64[1:4], ref.ld[1:4])
    o = CU.OPTION_SETS[option_set].options
    if option_set == "max4":
        assert (ref.ld.termination_type, ref.ld.num_iterations) == (R.NO_CONVERGENCE, 4)
    if option_set == "min6":
        assert ref.ld.num_iterations >= o.min_num_iterations
