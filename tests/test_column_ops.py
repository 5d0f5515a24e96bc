"""cse_jacobian_squared_column_norm and cse_jacobian_scale_columns
(SparseMatrix::SquaredColumnNorm / ScaleColumns on the device): the boundary,
without a GPU.  The kernels are checked in tests/test_column_ops_gpu.py."""
import ctypes
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "cse.h")
NAMES = ("cse_jacobian_squared_column_norm", "cse_jacobian_scale_columns")


def test_declared_exported_and_bound():
    from ceres_amd import _cse
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    exported = subprocess.run(["nm", "-D", "--defined-only", _cse.LIB_PATH], capture_output=True,
                              text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert re.search(r"\bT %s$" % name, exported, flags=re.M), name
        restype, argtypes = _cse.SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p] * 3
        assert getattr(_cse.lib(), name).argtypes == argtypes


def test_header_cites_the_reference_interface():
    text = open(HEADER).read()
    assert "SparseMatrix::SquaredColumnNorm" in text and "SparseMatrix::ScaleColumns" in text


def test_evaluator_methods_exist():
    import ceres_amd as ca
    assert callable(ca.Evaluator.squared_column_norm_device)
    assert callable(ca.Evaluator.scale_columns_device)


def test_null_arguments_are_invalid_without_a_gpu():
    from ceres_amd import _cse
    L = _cse.lib()
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name in NAMES:
        fn = getattr(L, name)
        assert fn(None, None, None) == _cse.CSE_ERR_INVALID
        assert "null" in _cse.last_error()
        assert fn(None, p, p) == _cse.CSE_ERR_INVALID
        assert "null evaluator" in _cse.last_error()
