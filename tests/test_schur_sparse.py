"""CPU: the block-sparse Schur complement's entry points, its host-only
structure planner and the driver flag.

cse_schur_complement_sparse_structure / cse_schur_complement_sparse /
cse_schur_explicit_multiply (include/cse.h) give S as the 9 x 9 blocks of its
upper triangle, BlockRandomAccessSparseMatrix's cells (SPARSE_SCHUR, and
ITERATIVE_SCHUR's use_explicit_schur_complement), and multiply by them.  Here,
without a GPU: the symbols are exported, wrapped and declared; the ABI version
did not move; the planner behind them (cse::PlanSchurSparse) and a host replay
of the product's summation order pass their stand-alone driver under
AddressSanitizer + UBSan (tests/cpp/schur_sparse_driver.cpp); and
bundle_adjuster takes --use_explicit_schur_complement with iterative_schur
alone.
"""
import ctypes as C
import os
import subprocess

import pytest

import ceres_amd as ca
from ceres_amd import _cse

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")

NAMES = ("cse_schur_complement_sparse_structure", "cse_schur_complement_sparse",
         "cse_schur_explicit_multiply")


def test_entry_points_are_exported_wrapped_and_declared():
    lib = C.CDLL(_cse.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _cse.SIGNATURES
    assert _cse.SIGNATURES["cse_schur_complement_sparse_structure"][1] == [
        C.c_void_p, _cse.P_i64, _cse.P_i64, _cse.P_i64, _cse.P_i64, _cse.P_i32]
    assert _cse.SIGNATURES["cse_schur_complement_sparse"][1] == [C.c_void_p, C.c_void_p]
    assert _cse.SIGNATURES["cse_schur_explicit_multiply"][1] == [C.c_void_p] * 4
    assert callable(ca.Evaluator.schur_complement_sparse_structure)
    assert callable(ca.Evaluator.schur_complement_sparse_device)
    assert callable(ca.Evaluator.schur_explicit_multiply_device)
    with open(os.path.join(os.path.dirname(CPP), "..", "include", "cse.h")) as f:
        header = f.read()
    assert "int cse_schur_complement_sparse_structure(cse_evaluator* ev, int64_t* num_block_rows," in header
    assert "int cse_schur_complement_sparse(cse_evaluator* ev, double* d_values);" in header
    assert "int cse_schur_explicit_multiply(cse_evaluator* ev, const double* d_values," in header
    # in the ITERATIVE_SCHUR section, after cse_schur_complement_plan
    assert header.index("int cse_schur_complement_plan(") < header.index(
        "int cse_schur_complement_sparse_structure(") < header.index("int cse_create_multi(")


def test_abi_version_is_still_6():
    assert _cse.lib().cse_abi_version() == 6 and _cse.CSE_ABI_VERSION == 6


def test_driver_takes_the_flag_with_iterative_schur_only():
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", "problem-16-22106"]
    args = bundle_adjuster.parse(base + ["--use_explicit_schur_complement"])
    assert args.use_explicit_schur_complement and args.linear_solver == "iterative_schur"
    assert not bundle_adjuster.parse(base).use_explicit_schur_complement
    for solver in ("dense_schur", "cgnr"):
        with pytest.raises(SystemExit, match="use_explicit_schur_complement"):
            bundle_adjuster.parse(base + ["--use_explicit_schur_complement", "--linear_solver", solver])


def test_sparse_structure_driver_under_asan_ubsan():
    """The stand-alone driver, g++ -fsanitize=address,undefined with static
    runtimes: the structure against brute force and the product replayed in
    the kernel's order against the dense symmetric product."""
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "schur_sparse.mk", "driver"])
    out = subprocess.run([os.path.join(CPP, "build", "schur_sparse_driver")], capture_output=True,
                         text=True)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0
    assert out.stdout.rstrip().endswith("OK")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
