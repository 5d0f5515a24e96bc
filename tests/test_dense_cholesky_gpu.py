"""GPU: the dense Cholesky factorization (cse_dense_cholesky_factorize, _solve,
_info), DenseCholesky's device forms (internal/ceres/dense_cholesky.h:195-302):
the FP64 factor and solve, and the FP32 factor with FP64 iterative refinement.

Inputs and bounds: dense_cholesky_util.py (generated matrices; Higham's Thm
10.3 and 10.4, evaluated in longdouble).  tests/test_dense_cholesky.py shows
that numpy's LAPACK meets a tenth of the same bounds on the same inputs.
Failures (info) are exact.  Measured on an MI355X, as shares of the bounds,
largest over all cases (each test prints its figures before it asserts): FP64
factor 0.0093, FP64 solve 0.0021; FP32 unrefined solve 0.013 of the 2^-24
bound and at least 630 times the FP64 bound for n >= 15; FP32 with 3
refinements 0.0012 and with 20 refinements 0.0016 of the FP64 bound; the Schur
chain 1.2e-12 against its 1e-8.
"""
import functools
import types

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse, bal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dense_cholesky_util as U  # noqa: E402
import schur_complement_util as SU  # noqa: E402
from test_spmv_gpu import dense_jacobian  # noqa: E402

SENTINEL = -7.5
PAD = 5
NB = U.NB
FP64, FP32 = _cse.DENSE_CHOLESKY_FP64, _cse.DENSE_CHOLESKY_FP32


def device():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def evaluator():
    """The factorization needs an evaluator for its device, stream and
    workspace only; any program does."""
    prog = bal.synthetic_program((4, 30, 100), seed=3)
    return ca.Evaluator(prog, stream=torch.cuda.current_stream(device()).cuda_stream)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device())


def lower_with(A, upper, ld=None, pad=SENTINEL):
    """A's lower triangle, `upper` in the strict upper triangle, `pad` in the
    columns [n, ld)."""
    n = A.shape[0]
    M = np.full((n, n if ld is None else ld), pad)
    M[:, :n] = np.where(np.tri(n, dtype=bool), A, upper)
    return M


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@functools.lru_cache(maxsize=None)
def run_fp64(n, kappa):
    """Everything the device computes in FP64 for one input, once."""
    ev = evaluator()
    A = U.spd(n, kappa)
    b1, b2 = U.rhs(n, 1), U.rhs(n, 2)
    c = types.SimpleNamespace(n=n, kappa=kappa, A=A, b1=b1, b2=b2)
    nan = lambda k: torch.full((k,), float("nan"), dtype=torch.float64, device=device())
    ld = n + PAD
    dA = to_dev(lower_with(A, np.nan, ld))
    ev.dense_cholesky_factorize_device(dA.data_ptr(), n, ld, FP64)
    db1, db2, x1, x2 = to_dev(b1), to_dev(b2), nan(n), nan(n)
    ev.dense_cholesky_solve_device(db1.data_ptr(), x1.data_ptr())
    alias = to_dev(b1)
    ev.dense_cholesky_solve_device(alias.data_ptr(), alias.data_ptr(), 0)
    ev.dense_cholesky_solve_device(db2.data_ptr(), x2.data_ptr())
    c.info = ev.dense_cholesky_info()
    c.status = ev.wait()
    c.M = dA.cpu().numpy()
    c.x1, c.x2, c.alias = x1.cpu().numpy(), x2.cpu().numpy(), alias.cpu().numpy()
    assert np.array_equal(db1.cpu().numpy(), b1)  # the right-hand side is read only
    # once more: ld = n by default, the precision by default
    dA2 = to_dev(lower_with(A, np.nan))
    ev.dense_cholesky_factorize_device(dA2.data_ptr(), n)
    y1 = nan(n)
    ev.dense_cholesky_solve_device(db1.data_ptr(), y1.data_ptr())
    c.info2 = ev.dense_cholesky_info()
    c.M2, c.y1 = dA2.cpu().numpy(), y1.cpu().numpy()
    return c


@functools.lru_cache(maxsize=None)
def run_fp32(n, kappa):
    ev = evaluator()
    A = U.spd(n, kappa)
    b = U.rhs(n, 1)
    c = types.SimpleNamespace(n=n, kappa=kappa, A=A, b=b, x={})
    M = lower_with(A, np.nan)
    dA = to_dev(M)
    ev.dense_cholesky_factorize_device(dA.data_ptr(), n, None, FP32)
    c.info = ev.dense_cholesky_info()
    c.unchanged_after_factorize = np.array_equal(bits(dA.cpu().numpy()), bits(M))
    db = to_dev(b)
    for refinements in (0, 3, 20):
        x = torch.full((n,), float("nan"), dtype=torch.float64, device=device())
        ev.dense_cholesky_solve_device(db.data_ptr(), x.data_ptr(), refinements)
        c.x[refinements] = x.cpu().numpy()
    alias = to_dev(b)
    ev.dense_cholesky_solve_device(alias.data_ptr(), alias.data_ptr(), 3)
    again = torch.empty(n, dtype=torch.float64, device=device())
    ev.dense_cholesky_solve_device(db.data_ptr(), again.data_ptr(), 3)
    c.status = ev.wait()
    c.alias, c.again = alias.cpu().numpy(), again.cpu().numpy()
    c.unchanged_after_solves = np.array_equal(bits(dA.cpu().numpy()), bits(M))
    return c


# ---- FP64

@pytest.mark.parametrize("n,kappa", U.CASES)
def test_fp64_factor_and_solve_bounds(gpu, n, kappa):
    c = run_fp64(n, kappa)
    assert c.info == 0 and c.info2 == 0 and c.status == _cse.CSE_OK
    L = c.M[:, :n]
    assert np.all(np.isfinite(L[np.tri(n, dtype=bool)]))
    f = U.factor_error(n, kappa, L) / U.factor_bound(c.A, U.U64)
    s1 = U.solve_residual(n, kappa, c.b1, c.x1) / U.solve_bound(c.A, c.x1, U.U64)
    s2 = U.solve_residual(n, kappa, c.b2, c.x2) / U.solve_bound(c.A, c.x2, U.U64)
    print(f"n {n} kappa {kappa:g} FP64: factor {f:.4f}, solves {s1:.4f} {s2:.4f} of the bound")
    assert f <= 1.0
    assert np.all(np.isfinite(c.x1)) and np.all(np.isfinite(c.x2))
    assert s1 <= 1.0 and s2 <= 1.0  # a second solve on the same factor, another right-hand side


@pytest.mark.parametrize("n,kappa", U.CASES)
def test_fp64_touches_the_lower_triangle_only(gpu, n, kappa):
    c = run_fp64(n, kappa)
    upper = ~np.tri(n, dtype=bool)
    assert np.all(np.isnan(c.M[:, :n][upper]))  # neither read (L is finite) nor written
    assert np.all(np.isnan(c.M2[upper]))
    assert np.all(c.M[:, n:] == SENTINEL)


@pytest.mark.parametrize("n,kappa", U.CASES)
def test_fp64_aliasing_and_repeatability(gpu, n, kappa):
    c = run_fp64(n, kappa)
    assert np.array_equal(bits(c.alias), bits(c.x1))  # d_rhs == d_x
    # another buffer, another leading dimension: bit for bit the same factor and solution
    lower = np.tri(n, dtype=bool)
    assert np.array_equal(bits(c.M[:, :n][lower]), bits(c.M2[lower]))
    assert np.array_equal(bits(c.y1), bits(c.x1))


# ---- FP32 factor, FP64 refinement

@pytest.mark.parametrize("n,kappa", U.CASES)
def test_fp32_leaves_the_matrix_alone(gpu, n, kappa):
    c = run_fp32(n, kappa)
    assert c.info == 0 and c.status == _cse.CSE_OK
    assert c.unchanged_after_factorize and c.unchanged_after_solves


@pytest.mark.parametrize("n,kappa", U.CASES)
def test_fp32_unrefined_solve_is_single_precision(gpu, n, kappa):
    c = run_fp32(n, kappa)
    x = c.x[0]
    res = U.solve_residual(n, kappa, c.b, x)
    s32 = res / U.solve_bound(c.A, x, U.U32, units=3)
    s64 = res / U.solve_bound(c.A, x, U.U64)
    print(f"n {n} kappa {kappa:g} FP32, 0 refinements: {s32:.4f} of the 2^-24 bound, {s64:.1f} of the 2^-53 bound")
    assert np.all(np.isfinite(x))
    assert s32 <= 1.0
    if n >= 15:
        assert s64 > 10.0  # the factor really is single precision


@pytest.mark.parametrize("n,kappa", U.CASES)
def test_fp32_refined_solve_meets_the_fp64_bound(gpu, n, kappa):
    c = run_fp32(n, kappa)
    for refinements in (3, 20):
        x = c.x[refinements]
        s = U.solve_residual(n, kappa, c.b, x) / U.solve_bound(c.A, x, U.U64)
        print(f"n {n} kappa {kappa:g} FP32, {refinements} refinements: {s:.4f} of the 2^-53 bound")
        assert np.all(np.isfinite(x))
        assert s <= 1.0
    assert np.array_equal(bits(c.alias), bits(c.x[3]))  # d_rhs == d_x
    assert np.array_equal(bits(c.again), bits(c.x[3]))  # run to run


def test_factorizations_of_changing_size_on_one_evaluator(gpu):
    """A larger n, a smaller one and the larger again on one evaluator, in both
    precisions: each factorization and solve is correct.  Whether the
    allocation was kept or made anew is not visible through the C ABI, so this
    shows only that a change of size or precision between calls is harmless."""
    prog = bal.synthetic_program((4, 30, 100), seed=4)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(device()).cuda_stream)
    for n, precision, refinements in ((65, FP32, 3), (441, FP32, 3), (17, FP32, 3), (441, FP64, 0), (65, FP64, 0),
                                      (441, FP32, 3)):
        kappa = 1e2
        A, b = U.spd(n, kappa), U.rhs(n, 1)
        dA, db = to_dev(lower_with(A, np.nan)), to_dev(b)
        x = torch.empty(n, dtype=torch.float64, device=device())
        ev.dense_cholesky_factorize_device(dA.data_ptr(), n, None, precision)
        ev.dense_cholesky_solve_device(db.data_ptr(), x.data_ptr(), refinements)
        assert ev.dense_cholesky_info() == 0
        x = x.cpu().numpy()
        assert U.solve_residual(n, kappa, b, x) <= U.solve_bound(A, x, U.U64)
    ev.close()


# ---- Failures: exact

def failure_cases():
    n = 3 * NB + 8  # three whole tiles and a ragged last one
    cases = []
    for k in (3, NB - 1, NB, n - 5):
        A = U.spd(n, 1e2).copy()
        A[k, k] = -1.0
        cases.append((f"negative pivot {k}", A, k + 1))
    m = NB + 6
    A = np.eye(m + 2 + 30)
    A[m:m + 2, m:m + 2] = [[4.0, 2.0], [2.0, 1.0]]  # SingularMatrix: the second pivot is exactly 0
    cases.append(("singular", A, m + 2))
    A = U.spd(n, 1e2).copy()
    A[150, 20] = np.nan
    cases.append(("nan", A, None))
    return cases


@pytest.mark.parametrize("precision", [FP64, FP32])
def test_failures_are_reported_exactly(gpu, precision):
    ev = evaluator()
    good_n, kappa = 65, 1e2
    good, b = U.spd(good_n, kappa), U.rhs(good_n, 1)
    for name, A, expect in failure_cases():
        n = A.shape[0]
        dA = to_dev(lower_with(A, np.nan))
        ev.dense_cholesky_factorize_device(dA.data_ptr(), n, None, precision)
        info = ev.dense_cholesky_info()
        if expect is None:
            assert info != 0, name
        else:
            assert info == expect, (name, info)
        x = torch.full((n,), float("nan"), dtype=torch.float64, device=device())
        rhs = to_dev(U.rhs(n, 1))
        ev.dense_cholesky_solve_device(rhs.data_ptr(), x.data_ptr(), 2 if precision == FP32 else 0)
        assert ev.wait() == _cse.CSE_OK, name  # the evaluator's status word is not touched
        assert np.array_equal(bits(x.cpu().numpy()), bits(np.zeros(n))), name
        # the next factorization starts from a clean flag
        dG, db = to_dev(lower_with(good, np.nan)), to_dev(b)
        y = torch.empty(good_n, dtype=torch.float64, device=device())
        ev.dense_cholesky_factorize_device(dG.data_ptr(), good_n, None, precision)
        ev.dense_cholesky_solve_device(db.data_ptr(), y.data_ptr(), 3 if precision == FP32 else 0)
        assert ev.dense_cholesky_info() == 0, name
        y = y.cpu().numpy()
        assert U.solve_residual(good_n, kappa, b, y) <= U.solve_bound(good, y, U.U64), name


def test_nan_in_the_strict_upper_triangle_changes_nothing(gpu):
    ev = evaluator()
    n, kappa = 129, 1e4
    A, b = U.spd(n, kappa), U.rhs(n, 1)
    out = []
    for precision, refinements in ((FP64, 0), (FP32, 3)):
        for upper in (np.nan, A):
            dA, db = to_dev(lower_with(A, upper)), to_dev(b)
            x = torch.empty(n, dtype=torch.float64, device=device())
            ev.dense_cholesky_factorize_device(dA.data_ptr(), n, None, precision)
            ev.dense_cholesky_solve_device(db.data_ptr(), x.data_ptr(), refinements)
            assert ev.dense_cholesky_info() == 0
            out.append(x.cpu().numpy())
    assert np.array_equal(bits(out[0]), bits(out[1]))
    assert np.array_equal(bits(out[2]), bits(out[3]))


# ---- Refusals

def test_refusals(gpu):
    dev = device()
    refuse = lambda code, msg: pytest.raises(RuntimeError, match=rf"cse_dense_cholesky_\w+ failed \({code}\).*{msg}")
    INVALID, UNSUPPORTED, OOM = _cse.CSE_ERR_INVALID, _cse.CSE_ERR_UNSUPPORTED, _cse.CSE_ERR_OOM
    prog = bal.synthetic_program((4, 30, 100), seed=5)
    n = 20
    A = to_dev(lower_with(U.spd(n, 1e2), 0.0))
    buf = torch.zeros(3 * n, dtype=torch.float64, device=dev)
    p = buf.data_ptr()
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    # before any factorize
    with refuse(INVALID, "no cse_dense_cholesky_factorize before it"):
        ev.dense_cholesky_solve_device(p, p + 8 * n)
    with refuse(INVALID, "no cse_dense_cholesky_factorize before it"):
        ev.dense_cholesky_info()
    with refuse(INVALID, "null pointer"):
        ev.dense_cholesky_factorize_device(None, n)
    with refuse(INVALID, "n must be at least 1"):
        ev.dense_cholesky_factorize_device(A.data_ptr(), 0)
    with refuse(INVALID, "ld is smaller than n"):
        ev.dense_cholesky_factorize_device(A.data_ptr(), n, n - 1)
    with refuse(INVALID, "unknown precision"):
        ev.dense_cholesky_factorize_device(A.data_ptr(), n, n, 2)
    # none of those counts as a factorize
    with refuse(INVALID, "no cse_dense_cholesky_factorize before it"):
        ev.dense_cholesky_info()
    # the workspace does not fit: 4 n^2 bytes of float copy
    with refuse(OOM, "hipMalloc"):
        ev.dense_cholesky_factorize_device(A.data_ptr(), 4_000_000, None, FP32)
    with refuse(INVALID, "no cse_dense_cholesky_factorize before it"):
        ev.dense_cholesky_solve_device(p, p + 8 * n)
    ev.dense_cholesky_factorize_device(A.data_ptr(), n)
    with refuse(INVALID, "null pointer"):
        ev.dense_cholesky_solve_device(None, p)
    with refuse(INVALID, "null pointer"):
        ev.dense_cholesky_solve_device(p, None)
    with refuse(INVALID, "negative"):
        ev.dense_cholesky_solve_device(p, p + 8 * n, -1)
    with refuse(INVALID, "overlaps d_rhs partially"):
        ev.dense_cholesky_solve_device(p, p + 8 * (n - 1))
    with refuse(INVALID, "overlaps d_rhs partially"):
        ev.dense_cholesky_solve_device(p + 8, p)
    with refuse(UNSUPPORTED, "refinement needs an FP32 factorization"):
        ev.dense_cholesky_solve_device(p, p + 8 * n, 1)
    ev.dense_cholesky_solve_device(p, p + 8 * n)
    assert ev.dense_cholesky_info() == 0
    with pytest.raises(RuntimeError, match=r"cse_dense_cholesky_info failed \(-1\).*null pointer"):
        _cse.check(_cse.lib().cse_dense_cholesky_info(ev.handle, None), "cse_dense_cholesky_info")
    ev.close()
    # a multi-device handle
    ev = ca.Evaluator(bal.synthetic_program((10, 300, 1500), seed=9), devices=[0, 0])
    with refuse(UNSUPPORTED, "multi-device"):
        ev.dense_cholesky_factorize_device(A.data_ptr(), n)
    with refuse(UNSUPPORTED, "multi-device"):
        ev.dense_cholesky_solve_device(p, p + 8 * n)
    with refuse(UNSUPPORTED, "multi-device"):
        ev.dense_cholesky_info()
    ev.close()


# ---- Through the Schur path

@pytest.mark.parametrize("precision,refinements", [(FP64, 0), (FP32, 3)])
def test_dense_schur_chain_on_the_device(gpu, precision, refinements):
    """cse_schur_complement -> factorize -> solve -> cse_schur_back_substitute
    against the dense normal equations solved in numpy, at the tolerance of
    test_schur_complement_gpu.py's host-Cholesky test of the same chain."""
    prog = SU.make_program("bal")
    dev = device()
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, r, _, jv = ev.evaluate()
    assert ok
    J = dense_jacobian(prog, jv)
    n = prog.num_effective_parameters
    e_cols, f_cols = ev.schur_structure()
    D = SU.damping(prog, True)
    b = -r
    dj, dD, db = to_dev(jv), to_dev(D), to_dev(b)
    rhs = torch.empty(f_cols, dtype=torch.float64, device=dev)
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), _cse.SCHUR_IDENTITY)
    S = torch.empty((f_cols, f_cols), dtype=torch.float64, device=dev)
    ev.schur_complement_device(S.data_ptr())  # both triangles: a valid input as it stands
    ev.dense_cholesky_factorize_device(S.data_ptr(), f_cols, None, precision)
    xf = torch.empty(f_cols, dtype=torch.float64, device=dev)
    ev.dense_cholesky_solve_device(rhs.data_ptr(), xf.data_ptr(), refinements)
    dx = torch.empty(n, dtype=torch.float64, device=dev)
    ev.schur_back_substitute_device(xf.data_ptr(), dx.data_ptr())
    assert ev.dense_cholesky_info() == 0
    assert ev.wait() == _cse.CSE_OK
    ref = np.linalg.solve(J.T @ J + np.diag(D * D), J.T @ b)
    got = dx.cpu().numpy()
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"precision {precision}, {refinements} refinements: relative error {err:.3e}")
    assert err <= 1e-8
    ev.close()


# ---- The driver

DRIVER = ["--synthetic", "problem-49-7776", "--linear_solver", "dense_schur"]


@pytest.fixture
def problem_49(monkeypatch):
    """BAL's problem-49-7776 (31,843 observations) as a named synthetic shape,
    as tools/dense_cholesky_probe.py names it, for these tests alone."""
    monkeypatch.setitem(bal.CONFIGS, "problem-49-7776", (49, 7776, 31843))


@functools.lru_cache(maxsize=None)
def torch_path_cost():
    from ceres_amd import bundle_adjuster
    return bundle_adjuster.main(DRIVER)[1]


@pytest.mark.parametrize("extra", [[], ["--mixed_precision_solves", "--max_num_refinement_iterations", "3"]],
                         ids=["fp64", "mixed"])
def test_bundle_adjuster_with_the_library_cholesky(gpu, capsys, problem_49, extra):
    from ceres_amd import bundle_adjuster
    ref = torch_path_cost()
    c0, c1, rows = bundle_adjuster.main(DRIVER + ["--dense_linear_algebra_library", "cse"] + extra)
    table = capsys.readouterr().out
    print(table)
    print(f"final cost {c1!r} against the torch path's {ref!r}: relative {abs(c1 - ref) / abs(ref):.3e}")
    assert c1 < c0
    assert abs(c1 - ref) <= 1e-9 * abs(ref)
    assert "Dense Cholesky factor & solve" in table
