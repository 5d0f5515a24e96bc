"""CPU: the dense Cholesky factorization's boundary (cse_dense_cholesky_*), its
host plan, the driver's flags and the bounds the GPU tests hold the device to.

The GPU tests (tests/test_dense_cholesky_gpu.py) check the device's factor and
solve against Higham's backward error bounds (dense_cholesky_util.py).  Here
numpy's LAPACK in float64 and float32 is shown to meet a tenth of those bounds
on exactly the same inputs (n = 1: the bound itself), measured against
longdouble, which pins the bounds independently of the device.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import dense_cholesky_util as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "cse.h")
CPP = os.path.join(REPO, "tests", "cpp")

SYMBOLS = ("cse_dense_cholesky_factorize", "cse_dense_cholesky_solve", "cse_dense_cholesky_info",
           "cse_dense_cholesky_workspace")


def test_symbols_exported_and_wrapped():
    from ceres_amd import _cse
    C = ctypes
    lib = C.CDLL(_cse.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    S = _cse.SIGNATURES
    assert S["cse_dense_cholesky_factorize"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                           C.c_int32])
    assert S["cse_dense_cholesky_solve"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32])
    assert S["cse_dense_cholesky_info"] == (C.c_int, [C.c_void_p, _cse.P_i32])
    assert S["cse_dense_cholesky_workspace"] == (C.c_int, [C.c_int64, C.c_int32, _cse.P_i64])
    assert (_cse.DENSE_CHOLESKY_FP64, _cse.DENSE_CHOLESKY_FP32) == (0, 1)


def test_evaluator_methods():
    import ceres_amd as ca
    from ceres_amd import _cse
    sig = inspect.signature(ca.Evaluator.dense_cholesky_factorize_device)
    assert list(sig.parameters) == ["self", "d_A", "n", "ld", "precision"]
    assert sig.parameters["ld"].default is None
    assert sig.parameters["precision"].default == _cse.DENSE_CHOLESKY_FP64
    sig = inspect.signature(ca.Evaluator.dense_cholesky_solve_device)
    assert list(sig.parameters) == ["self", "d_rhs", "d_x", "max_num_refinement_iterations"]
    assert sig.parameters["max_num_refinement_iterations"].default == 0
    assert list(inspect.signature(ca.Evaluator.dense_cholesky_info).parameters) == ["self"]
    assert isinstance(inspect.getattr_static(ca.Evaluator, "dense_cholesky_workspace"), staticmethod)


def test_header_lines():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert "enum { CSE_DENSE_CHOLESKY_FP64 = 0, CSE_DENSE_CHOLESKY_FP32 = 1 };" in flat
    assert ("int cse_dense_cholesky_factorize(cse_evaluator* ev, int64_t n, double* d_A, int64_t ld, "
            "int32_t precision);") in flat
    assert ("int cse_dense_cholesky_solve(cse_evaluator* ev, const double* d_rhs, double* d_x, "
            "int32_t max_num_refinement_iterations);") in flat
    assert "int cse_dense_cholesky_info(cse_evaluator* ev, int32_t* info);" in flat
    assert ("int cse_dense_cholesky_workspace(int64_t n, int32_t precision, int64_t* device_bytes);") in flat
    # each symbol names the reference lines it replaces
    for ref in ("dense_cholesky.h:195-302", "dense_cholesky.cc:364-407", "dense_cholesky.cc:409-450", ":594-637",
                "dense_cholesky.cc:397-403"):
        assert ref in text, ref


def test_abi_version_is_still_6():
    from ceres_amd import _cse
    assert re.search(r"#define CSE_ABI_VERSION 6\b", open(HEADER).read())
    assert _cse.CSE_ABI_VERSION == 6
    assert _cse.lib().cse_abi_version() == 6


def test_workspace_by_hand_needs_no_evaluator():
    """n = 441 is 7 panels of 64, vectors padded to 448; every segment is
    rounded up to 256 bytes and the failure flag takes one such unit."""
    import ceres_amd as ca
    from ceres_amd import _cse
    # FP64: the inverses of the diagonal blocks, v and y, the flag
    fp64 = 7 * 64 * 64 * 8 + 2 * 448 * 8 + 256
    assert fp64 == 236800
    assert ca.Evaluator.dense_cholesky_workspace(441, _cse.DENSE_CHOLESKY_FP64) == fp64
    # FP32: the float copy (441 * 441 * 4 = 777924 -> 777984), those in float, x and r in double
    fp32 = 777984 + 7 * 64 * 64 * 4 + 2 * 448 * 4 + 2 * 448 * 8 + 256
    assert fp32 == 903680
    assert ca.Evaluator.dense_cholesky_workspace(441, _cse.DENSE_CHOLESKY_FP32) == fp32
    out = ctypes.c_int64(-1)
    L = _cse.lib()
    assert L.cse_dense_cholesky_workspace(0, 0, ctypes.byref(out)) == _cse.CSE_ERR_INVALID
    assert "n must be at least 1" in _cse.last_error()
    assert L.cse_dense_cholesky_workspace(5, 2, ctypes.byref(out)) == _cse.CSE_ERR_INVALID
    assert "unknown precision" in _cse.last_error()
    assert L.cse_dense_cholesky_workspace(5, 0, None) == _cse.CSE_ERR_INVALID
    assert out.value == -1
    # no evaluator either for the calls' own null check
    assert L.cse_dense_cholesky_factorize(None, 5, None, 5, 0) == _cse.CSE_ERR_INVALID
    assert L.cse_dense_cholesky_solve(None, None, None, 0) == _cse.CSE_ERR_INVALID
    assert L.cse_dense_cholesky_info(None, None) == _cse.CSE_ERR_INVALID


def test_driver_flags():
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", "problem-16-22106", "--linear_solver", "dense_schur"]
    args = bundle_adjuster.parse(base)
    assert args.dense_linear_algebra_library == "torch"
    assert args.mixed_precision_solves is False
    assert args.max_num_refinement_iterations == 0
    args = bundle_adjuster.parse(base + ["--dense_linear_algebra_library", "cse", "--mixed_precision_solves",
                                         "--max_num_refinement_iterations", "3"])
    assert args.dense_linear_algebra_library == "cse"
    assert args.mixed_precision_solves is True
    assert args.max_num_refinement_iterations == 3
    with pytest.raises(SystemExit, match="--mixed_precision_solves needs --dense_linear_algebra_library cse"):
        bundle_adjuster.parse(base + ["--mixed_precision_solves"])
    with pytest.raises(SystemExit, match="--max_num_refinement_iterations needs --mixed_precision_solves"):
        bundle_adjuster.parse(base + ["--max_num_refinement_iterations", "2"])
    with pytest.raises(SystemExit, match="--max_num_refinement_iterations needs --mixed_precision_solves"):
        bundle_adjuster.parse(base + ["--dense_linear_algebra_library", "cse",
                                      "--max_num_refinement_iterations", "2"])
    with pytest.raises(SystemExit, match="must not be negative"):
        bundle_adjuster.parse(base + ["--dense_linear_algebra_library", "cse", "--mixed_precision_solves",
                                      "--max_num_refinement_iterations", "-1"])
    with pytest.raises(SystemExit, match="needs --linear_solver dense_schur"):
        bundle_adjuster.parse(["--synthetic", "problem-16-22106", "--dense_linear_algebra_library", "cse"])


def test_driver_under_asan_ubsan():
    subprocess.run(["make", "-C", CPP, "-f", "dense_cholesky.mk", "driver"], check=True, capture_output=True)
    run = subprocess.run([os.path.join(CPP, "build", "dense_cholesky_driver")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "dense_cholesky_driver: ok" in run.stdout


def test_shipped_panel_width_is_the_utils():
    text = open(os.path.join(REPO, "ceres-solver-cuda_amd", "csrc", "plan.hpp")).read()
    assert re.search(r"constexpr int kDenseCholeskyNB = (\d+);", text).group(1) == str(U.NB)
    for n in (U.NB - 1, U.NB, U.NB + 1, 2 * U.NB + 1):
        assert n in U.SIZES


@pytest.mark.parametrize("n,kappa", U.CASES)
def test_numpy_references_meet_a_tenth_of_the_bounds(n, kappa):
    A = U.spd(n, kappa)
    b = U.rhs(n, 0)
    share = 1.0 if n == 1 else 0.1
    # float64
    L = np.linalg.cholesky(A)
    x = U.cholesky_solve(L, b)
    f = U.factor_error(n, kappa, L) / U.factor_bound(A, U.U64)
    s = U.solve_residual(n, kappa, b, x) / U.solve_bound(A, x, U.U64)
    print(f"n {n} kappa {kappa:g} float64: factor {f:.4f} solve {s:.4f} of the bound")
    assert f <= share and s <= share
    # float32 factor and unrefined solve
    L32 = np.linalg.cholesky(A.astype(np.float32))
    assert L32.dtype == np.float32
    x32 = U.cholesky_solve(L32, b)
    assert x32.dtype == np.float32
    f = U.factor_error(n, kappa, L32) / U.factor_bound(A, U.U32)
    s = U.solve_residual(n, kappa, b, x32) / U.solve_bound(A, x32, U.U32, units=3)
    print(f"n {n} kappa {kappa:g} float32: factor {f:.4f} solve {s:.4f} of the bound")
    assert f <= share and s <= share
