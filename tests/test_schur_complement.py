"""CPU: the explicit Schur complement's entry points, its host-only pair plan
and the tolerance of its GPU test.

cse_schur_complement / cse_schur_complement_plan (include/cse.h) form the
dense reduced camera matrix S of DENSE_SCHUR (SchurEliminator::Eliminate,
schur_eliminator_impl.h).  Here, without a GPU: the symbols are exported and
wrapped; the ABI version did not move; the planner behind them
(cse::PlanSchurPairs) passes its stand-alone driver under AddressSanitizer +
UBSan (tests/cpp/schur_pairs_driver.cpp); and the bounds
tests/test_schur_complement_gpu.py holds the device to are bounds the numpy
float64 reference itself meets with a factor of ten to spare, measured against
the same formula in np.longdouble on the oracle's Jacobian.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse

import schur_complement_util as U

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


def test_entry_points_are_exported_and_wrapped():
    lib = C.CDLL(_cse.LIB_PATH)
    for name in ("cse_schur_complement", "cse_schur_complement_plan"):
        assert hasattr(lib, name), name
        assert name in _cse.SIGNATURES
    assert _cse.SIGNATURES["cse_schur_complement"][1] == [C.c_void_p, C.c_void_p, C.c_int64]
    assert callable(ca.Evaluator.schur_complement_device)
    assert callable(ca.Evaluator.schur_complement_plan)
    with open(os.path.join(os.path.dirname(CPP), "..", "include", "cse.h")) as f:
        header = f.read()
    assert "int cse_schur_complement(cse_evaluator* ev, double* d_S, int64_t ld);" in header
    assert "int cse_schur_complement_plan(cse_evaluator* ev, int64_t* num_blocks," in header


def test_abi_version_is_still_6():
    assert _cse.lib().cse_abi_version() == 6 and _cse.CSE_ABI_VERSION == 6


def test_driver_offers_dense_schur():
    from ceres_amd import bundle_adjuster
    args = bundle_adjuster.parse(["--synthetic", "problem-16-22106", "--linear_solver", "dense_schur"])
    assert args.linear_solver == "dense_schur" and args.max_schur_gb == 16.0


def test_pair_plan_driver_under_asan_ubsan():
    """The stand-alone pair-plan driver, g++ -fsanitize=address,undefined with
    static runtimes: the plan against brute force and a host replay of it
    against the dense formula."""
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "schur_pairs.mk", "driver"])
    out = subprocess.run([os.path.join(CPP, "build", "schur_pairs_driver")], capture_output=True,
                         text=True)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0
    assert out.stdout.rstrip().endswith("OK")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


@pytest.mark.parametrize("which,with_D", [c for c in U.CASES if c[0] != "user"])
def test_float64_reference_meets_a_tenth_of_the_bounds(which, with_D):
    """The GPU test compares the device's S with numpy's float64 S to
    1e-12 ||S||_F and, per block, 1e-12 times the magnitude of the summed
    terms.  The float64 reference sits within a tenth of both, measured
    against np.longdouble.  (The user-kind problem is the "bal" problem with
    the Snavely functor compiled as a user kind: the same Jacobian.)"""
    import oracle_py as O
    from test_spmv_gpu import dense_jacobian
    prog = U.make_program(which)
    op = O.OracleProgram.from_program(
        prog.with_explicit_manifolds(prog.state) if which == "quaternion" else prog)
    ok, _, _, _, jv = op.evaluate(prog.state)
    assert ok
    J = dense_jacobian(prog, jv)
    ccol, _, _ = U.structure(prog)
    e_cols = int(ccol.min())
    D = U.damping(prog, with_D)
    S, Minv = U.schur_float64(J, e_cols, D)
    SL = U.schur_longdouble(prog, J, e_cols, D)
    diff = (S - SL).astype(np.float64)
    norm_ratio = np.linalg.norm(diff) / np.linalg.norm(S)
    bound = U.block_bound(J, e_cols, D, Minv)
    err = U.block_norms(diff)
    live = bound > 0
    block_ratio = (err[live] / bound[live]).max()
    print(f"{which} D={with_D}: |dS|/|S| {norm_ratio:.3e}, worst block error / magnitude {block_ratio:.3e}")
    assert norm_ratio <= 0.1 * U.RTOL
    assert block_ratio <= 0.1 * U.RTOL
    assert (err[~live] == 0).all()  # cameras that share no point: zero in both
