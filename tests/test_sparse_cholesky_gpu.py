"""GPU: the block-sparse Cholesky factorization (cse_sparse_cholesky_analyze,
_structure, _factorize, _factor_values, _solve, _info), the SparseCholesky
behind SPARSE_SCHUR (internal/ceres/sparse_cholesky.h:72-113,
schur_complement_solver.cc:290-333).

Inputs, restatements and bounds: sparse_cholesky_util.py (generated block
matrices; Higham's Thm 10.3 and 10.4 with n = 9 C and u = 2^-53, evaluated in
longdouble).  tests/test_sparse_cholesky.py shows that the plan equals the
Python restatement the structure is compared with here, and that numpy's
LAPACK meets a tenth of the same bounds on the same inputs.  Failures (info)
are exact.  Each test prints its figures before it asserts; measured on an
MI355X, as shares of the bounds, largest over all cases: factor 0.0151 and
solve 0.0048 (both on the one-block shape; 0.0001 to 0.002 from 12 blocks on),
solve with 1 refinement 0.0014, with 3 refinements 0.0030; the Schur chain
1.7e-12 against its 1e-8; the driver's final costs equal dense_schur's to the
last digit (relative difference 0).
"""
import functools
import types

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse, bal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import schur_complement_util as SU  # noqa: E402
import sparse_cholesky_util as U  # noqa: E402
from test_spmv_gpu import dense_jacobian  # noqa: E402

B = U.B


def device():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def evaluator():
    """The factorization needs an evaluator for its device, stream and storage
    only; any program does."""
    prog = bal.synthetic_program((4, 30, 100), seed=3)
    return ca.Evaluator(prog, stream=torch.cuda.current_stream(device()).cuda_stream)


def to_dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(device())  # a copy: the inputs are read-only arrays


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def analyze(ev, name, ordering):
    row_begin, block_col, _, _ = U.matrix(name)
    return ev.sparse_cholesky_analyze(row_begin, block_col, ordering,
                                      U.given_order(name) if ordering == U.GIVEN else None)


def factor_and_solve(ev, d_values, d_rhs, refinements=0, alias=False):
    """(info, L values, x) of one factorize + solve on the device."""
    s = ev._sparse_cholesky_summary
    ev.sparse_cholesky_factorize_device(d_values.data_ptr())
    L = torch.full((s.num_factor_blocks, B, B), np.nan, dtype=torch.float64, device=device())
    ev.sparse_cholesky_factor_values_device(L.data_ptr())
    if alias:
        x = d_rhs.clone()
        ev.sparse_cholesky_solve_device(x.data_ptr(), x.data_ptr(), refinements)
    else:
        x = torch.full_like(d_rhs, np.nan)
        ev.sparse_cholesky_solve_device(d_rhs.data_ptr(), x.data_ptr(), refinements)
    info = ev.sparse_cholesky_info()
    return info, L.cpu().numpy(), x.cpu().numpy()


@functools.lru_cache(maxsize=None)
def run(name, ordering):
    """Everything the device computes for one case, once."""
    ev = evaluator()
    _, _, values, A = U.matrix(name)
    b = U.rhs(name)
    out = types.SimpleNamespace(A=A, b=b)
    out.summary = analyze(ev, name, ordering)
    out.structure = ev.sparse_cholesky_structure()
    d_values, d_rhs = to_dev(values), to_dev(b)
    out.info, out.L, out.x = factor_and_solve(ev, d_values, d_rhs)
    out.again = factor_and_solve(ev, d_values, d_rhs)
    out.aliased = factor_and_solve(ev, d_values, d_rhs, alias=True)
    out.refined = {}
    for count in (0, 1, 3):
        x = torch.full_like(d_rhs, np.nan)
        ev.sparse_cholesky_solve_device(d_rhs.data_ptr(), x.data_ptr(), count)
        out.refined[count] = x.cpu().numpy()
    x = d_rhs.clone()
    ev.sparse_cholesky_solve_device(x.data_ptr(), x.data_ptr(), 3)
    out.refined_aliased = x.cpu().numpy()
    out.values_after, out.rhs_after = d_values.cpu().numpy(), d_rhs.cpu().numpy()
    assert ev.wait() == _cse.CSE_OK
    return out


cases = pytest.mark.parametrize("case", U.CASES, ids=U.case_id)


@cases
def test_structure_equals_the_plan(gpu, case):
    name, ordering = case
    C, pairs = U.SHAPES[name]
    out = run(name, ordering)
    perm, row_begin, block_col, parent, level = out.structure
    # Against the Python restatement, not the CPU driver's output: tests/test_sparse_cholesky.py
    # holds the CPU plan to the same restatement, case by case, so the two are equal, and no
    # GPU test starts a further process.
    order = U.expected_order(name, ordering)
    np.testing.assert_array_equal(perm, order)
    want_begin, want_col, want_parent = U.fill(C, pairs, order)
    np.testing.assert_array_equal(row_begin, want_begin)
    np.testing.assert_array_equal(block_col, want_col)
    np.testing.assert_array_equal(parent, want_parent)
    np.testing.assert_array_equal(level, U.levels(want_parent))
    s = out.summary
    assert (s.num_block_rows, s.num_input_blocks, s.num_factor_blocks) == (C, C + len(pairs), len(want_col))
    assert s.num_block_products == U.block_products(want_begin, want_col)
    assert s.num_levels == level.max() + 1 and s.max_level_columns == np.bincount(level).max()
    assert s.device_bytes >= 8 * 81 * (len(want_col) + C)


@cases
def test_factor_and_solve_bounds(gpu, case):
    name, ordering = case
    out = run(name, ordering)
    perm, row_begin, block_col, _, _ = out.structure
    assert out.info == 0
    # a diagonal block's strict upper triangle is zero
    diagonal = out.L[row_begin[1:] - 1]
    assert not diagonal[:, np.triu_indices(B, 1)[0], np.triu_indices(B, 1)[1]].any()
    L = U.dense_factor(row_begin, block_col, out.L)
    f = U.factor_error(out.A, perm, L) / U.factor_bound(out.A, U.U64)
    s = U.solve_residual(out.A, out.b, out.x) / U.solve_bound(out.A, out.x, U.U64)
    print(f"{U.case_id(case)}: factor {f:.4f} solve {s:.4f} of the bound")
    assert f <= 1.0
    assert s <= 1.0


@cases
def test_inputs_aliasing_and_repeatability(gpu, case):
    name, ordering = case
    out = run(name, ordering)
    _, _, values, _ = U.matrix(name)
    assert np.array_equal(bits(out.values_after), bits(values))
    assert np.array_equal(bits(out.rhs_after), bits(out.b))
    for info, L, x in (out.again, out.aliased):
        assert info == 0
        assert np.array_equal(bits(L), bits(out.L))
        assert np.array_equal(bits(x), bits(out.x))
    assert np.array_equal(bits(out.refined_aliased), bits(out.refined[3]))


@cases
def test_refinement(gpu, case):
    name, ordering = case
    out = run(name, ordering)
    assert np.array_equal(bits(out.refined[0]), bits(out.x))
    for count in (1, 3):
        x = out.refined[count]
        s = U.solve_residual(out.A, out.b, x) / U.solve_bound(out.A, x, U.U64)
        print(f"{U.case_id(case)}: {count} refinements, solve {s:.4f} of the bound")
        assert s <= 1.0


@pytest.mark.parametrize("name", sorted(U.SHAPES))
def test_given_identity_is_natural(gpu, name):
    ev = evaluator()
    row_begin, block_col, values, _ = U.matrix(name)
    d_values, d_rhs = to_dev(values), to_dev(U.rhs(name))
    ev.sparse_cholesky_analyze(row_begin, block_col, U.GIVEN, np.arange(len(row_begin) - 1, dtype=np.int32))
    info, L, x = factor_and_solve(ev, d_values, d_rhs)
    natural = run(name, U.NATURAL)
    assert info == 0
    assert np.array_equal(bits(L), bits(natural.L))
    assert np.array_equal(bits(x), bits(natural.x))


def test_one_analysis_two_factorizations_then_another_shape(gpu):
    """sparse_cholesky.h:55-56: the analysis once, Factorize again with other
    values of the same structure; a second analyze replaces the first."""
    ev = ca.Evaluator(bal.synthetic_program((4, 30, 100), seed=3),
                      stream=torch.cuda.current_stream(device()).cuda_stream)
    for name, seeds in (("random", (0, 1)), ("arrow-80", (0,)), ("two", (0, 2)), ("band", (1,))):
        analyze(ev, name, U.MINIMUM_DEGREE)
        perm, row_begin, block_col, _, _ = ev.sparse_cholesky_structure()
        for seed in seeds:
            _, _, values, A = U.matrix(name, seed)
            b = U.rhs(name, seed)
            info, Lv, x = factor_and_solve(ev, to_dev(values), to_dev(b))
            assert info == 0
            f = U.factor_error(A, perm, U.dense_factor(row_begin, block_col, Lv)) / U.factor_bound(A, U.U64)
            s = U.solve_residual(A, b, x) / U.solve_bound(A, x, U.U64)
            print(f"{name} seed {seed}: factor {f:.4f} solve {s:.4f} of the bound")
            assert f <= 1.0 and s <= 1.0
            if name == "random" and seed == 0:
                assert np.array_equal(bits(x), bits(run(name, U.MINIMUM_DEGREE).x))
    ev.close()


# ---- Failures, exact

def failing(name, cameras, value):
    row_begin, _, values, _ = U.matrix(name)
    bad = values.copy()
    for c in cameras:
        if value == "minus identity":
            bad[row_begin[c]] = -np.eye(B)
        else:
            bad[row_begin[c], 4, 4] = np.nan
    return bad


FAILURES = [("band", (17,), "minus identity"), ("random", (30,), "minus identity"), ("full", (0,), "minus identity"),
            ("arrow-first", (0,), "minus identity"), ("forest", U.FOREST_BAD, "minus identity"),
            ("forest", U.FOREST_BAD[::-1], "minus identity"), ("pairs-300", (299, 4), "minus identity"),
            ("one", (0,), "minus identity"), ("band", (22,), "nan"), ("random", (58,), "nan")]


@pytest.mark.parametrize("ordering", U.ORDERINGS, ids=["natural", "minimum_degree", "given"])
def test_failures_are_reported_exactly(gpu, ordering):
    """Diagonal block c = -I: every earlier pivot comes from an SPD principal
    submatrix, so info = 9 pos(c) + 1 whatever the rounding; with two bad
    blocks in different trees the smaller position is reported.  A NaN at
    (4, 4) of a diagonal block reaches no earlier pivot and fails that block's
    column 4: info = 9 pos(c) + 5."""
    ev = evaluator()
    for name, cameras, value in FAILURES:
        analyze(ev, name, ordering)
        pos = np.argsort(ev.sparse_cholesky_structure()[0])
        first = min(int(pos[c]) for c in cameras)
        _, _, good, _ = U.matrix(name)
        d_rhs = to_dev(U.rhs(name))
        info, _, x = factor_and_solve(ev, to_dev(failing(name, cameras, value)), d_rhs)
        print(f"{name} {cameras} {value}: info {info}")
        assert info == 9 * first + (5 if value == "nan" else 1)
        assert not x.any() and np.isfinite(x).all()  # assigned zeros
        # a refining solve too
        xr = torch.full_like(d_rhs, np.nan)
        ev.sparse_cholesky_solve_device(d_rhs.data_ptr(), xr.data_ptr(), 2)
        assert not xr.cpu().numpy().any()
        # the evaluator's status word is not touched
        assert ev.wait() == _cse.CSE_OK
        # and the next good factorize reports 0
        info, _, x = factor_and_solve(ev, to_dev(good), d_rhs)
        assert info == 0
        assert np.array_equal(bits(x), bits(run(name, ordering).x))


# ---- Refusals

def test_refusals(gpu):
    dev = device()
    refuse = lambda code, msg: pytest.raises(RuntimeError, match=rf"cse_sparse_cholesky_\w+ failed \({code}\).*{msg}")
    INVALID, UNSUPPORTED = _cse.CSE_ERR_INVALID, _cse.CSE_ERR_UNSUPPORTED
    ev = ca.Evaluator(bal.synthetic_program((4, 30, 100), seed=5), stream=torch.cuda.current_stream(dev).cuda_stream)
    row_begin, block_col, values, _ = U.matrix("band")
    n = B * (len(row_begin) - 1)
    d_values = to_dev(values)
    buf = torch.zeros(3 * n, dtype=torch.float64, device=dev)
    p = buf.data_ptr()
    # before any analyze
    with refuse(INVALID, "no cse_sparse_cholesky_analyze before it"):
        ev.sparse_cholesky_factorize_device(d_values.data_ptr())
    with refuse(INVALID, "no cse_sparse_cholesky_analyze before it"):
        ev.sparse_cholesky_structure()
    # the structures tests/test_sparse_cholesky.py shows the plan refuses
    with refuse(INVALID, "does not start with its diagonal block"):
        ev.sparse_cholesky_analyze([0, 2, 3], [1, 1, 1], U.NATURAL)
    with refuse(INVALID, "do not ascend or are out of range"):
        ev.sparse_cholesky_analyze([0, 3, 4, 5], [0, 2, 1, 1, 2], U.NATURAL)
    with refuse(INVALID, "do not ascend or are out of range"):
        ev.sparse_cholesky_analyze([0, 2, 3], [0, 2, 1], U.NATURAL)
    with refuse(INVALID, "unknown ordering"):
        ev.sparse_cholesky_analyze(row_begin, block_col, 3)
    with refuse(INVALID, "without a permutation"):
        ev.sparse_cholesky_analyze(row_begin, block_col, U.GIVEN)
    with refuse(INVALID, "not a permutation"):
        ev.sparse_cholesky_analyze(row_begin, block_col, U.GIVEN, np.zeros(len(row_begin) - 1, np.int32))
    with pytest.raises(RuntimeError, match=r"cse_sparse_cholesky_analyze failed \(-1\).*null pointer"):
        _cse.check(_cse.lib().cse_sparse_cholesky_analyze(ev.handle, 3, None, None, 0, None, None),
                   "cse_sparse_cholesky_analyze")
    # none of those counts as an analyze
    with refuse(INVALID, "no cse_sparse_cholesky_analyze before it"):
        ev.sparse_cholesky_factorize_device(d_values.data_ptr())
    ev.sparse_cholesky_analyze(row_begin, block_col, U.NATURAL)
    # before any factorize
    with refuse(INVALID, "no cse_sparse_cholesky_factorize before it"):
        ev.sparse_cholesky_solve_device(p, p + 8 * n)
    with refuse(INVALID, "no cse_sparse_cholesky_factorize before it"):
        ev.sparse_cholesky_info()
    with refuse(INVALID, "no cse_sparse_cholesky_factorize before it"):
        ev.sparse_cholesky_factor_values_device(p)
    with refuse(INVALID, "null pointer"):
        ev.sparse_cholesky_factorize_device(None)
    ev.sparse_cholesky_factorize_device(d_values.data_ptr())
    with refuse(INVALID, "null pointer"):
        ev.sparse_cholesky_solve_device(None, p)
    with refuse(INVALID, "null pointer"):
        ev.sparse_cholesky_solve_device(p, None)
    with refuse(INVALID, "null pointer"):
        ev.sparse_cholesky_factor_values_device(None)
    with refuse(INVALID, "negative"):
        ev.sparse_cholesky_solve_device(p, p + 8 * n, -1)
    with refuse(INVALID, "overlaps d_rhs partially"):
        ev.sparse_cholesky_solve_device(p, p + 8 * (n - 1))
    with refuse(INVALID, "overlaps d_rhs partially"):
        ev.sparse_cholesky_solve_device(p + 8, p)
    ev.sparse_cholesky_solve_device(p, p + 8 * n, 1)
    assert ev.sparse_cholesky_info() == 0
    with pytest.raises(RuntimeError, match=r"cse_sparse_cholesky_info failed \(-1\).*null pointer"):
        _cse.check(_cse.lib().cse_sparse_cholesky_info(ev.handle, None), "cse_sparse_cholesky_info")
    # a refused analyze leaves the last analysis and its factor in place
    with refuse(INVALID, "unknown ordering"):
        ev.sparse_cholesky_analyze(row_begin, block_col, -1)
    assert ev.sparse_cholesky_info() == 0
    # a new analyze drops the factor
    ev.sparse_cholesky_analyze(row_begin, block_col, U.NATURAL)
    with refuse(INVALID, "no cse_sparse_cholesky_factorize before it"):
        ev.sparse_cholesky_info()
    ev.close()
    # a multi-device handle
    ev = ca.Evaluator(bal.synthetic_program((10, 300, 1500), seed=9), devices=[0, 0])
    with refuse(UNSUPPORTED, "multi-device"):
        ev.sparse_cholesky_analyze(row_begin, block_col, U.NATURAL)
    with refuse(UNSUPPORTED, "multi-device"):
        ev.sparse_cholesky_factorize_device(d_values.data_ptr())
    with refuse(UNSUPPORTED, "multi-device"):
        ev.sparse_cholesky_solve_device(p, p + 8 * n)
    with refuse(UNSUPPORTED, "multi-device"):
        ev.sparse_cholesky_info()
    ev.close()


# ---- Through the Schur path

@pytest.mark.parametrize("ordering", [U.NATURAL, U.MINIMUM_DEGREE], ids=["natural", "minimum_degree"])
@pytest.mark.parametrize("which", ["bal", "duplicates", "unobserved"])
def test_sparse_schur_chain_on_the_device(gpu, which, ordering):
    """cse_schur_complement_sparse_structure -> analyze -> cse_schur_complement_
    sparse -> factorize -> solve -> cse_schur_back_substitute against the dense
    normal equations solved in numpy, to the dense chain's criterion."""
    prog = SU.make_program(which)
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
    row_begin, block_col, _ = ev.schur_complement_sparse_structure()  # a valid input as it stands
    summary = ev.sparse_cholesky_analyze(row_begin, block_col, ordering)
    assert B * summary.num_block_rows == f_cols
    values = torch.empty(81 * len(block_col), dtype=torch.float64, device=dev)
    ev.schur_complement_sparse_device(values.data_ptr())
    ev.sparse_cholesky_factorize_device(values.data_ptr())
    xf = torch.empty(f_cols, dtype=torch.float64, device=dev)
    ev.sparse_cholesky_solve_device(rhs.data_ptr(), xf.data_ptr(), 1)
    dx = torch.empty(n, dtype=torch.float64, device=dev)
    ev.schur_back_substitute_device(xf.data_ptr(), dx.data_ptr())
    assert ev.sparse_cholesky_info() == 0
    assert ev.wait() == _cse.CSE_OK
    ref = np.linalg.solve(J.T @ J + np.diag(D * D), J.T @ b)
    got = dx.cpu().numpy()
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print(f"{which}, ordering {ordering}: relative error {err:.3e}")
    assert err <= 1e-8
    ev.close()


# ---- The driver

@pytest.fixture
def problem_49(monkeypatch):
    """BAL's problem-49-7776 (31,843 observations) as a named synthetic shape,
    as test_dense_cholesky_gpu.py names it, for these tests alone."""
    monkeypatch.setitem(bal.CONFIGS, "problem-49-7776", (49, 7776, 31843))


SHAPES = ["problem-49-7776", "banded-60-3000-w6"]


@functools.lru_cache(maxsize=None)
def dense_schur_cost(shape):
    from ceres_amd import bundle_adjuster
    return bundle_adjuster.main(["--synthetic", shape, "--linear_solver", "dense_schur"])[1]


@pytest.mark.parametrize("ordering", ["minimum_degree", "natural"])
@pytest.mark.parametrize("shape", SHAPES)
def test_bundle_adjuster_with_sparse_schur(gpu, capsys, problem_49, shape, ordering):
    from ceres_amd import bundle_adjuster
    ref = dense_schur_cost(shape)
    c0, c1, rows = bundle_adjuster.main(["--synthetic", shape, "--linear_solver", "sparse_schur",
                                         "--sparse_ordering", ordering])
    table = capsys.readouterr().out
    print(table)
    print(f"final cost {c1!r} against dense_schur's {ref!r}: relative {abs(c1 - ref) / abs(ref):.3e}")
    assert c1 < c0
    assert abs(c1 - ref) <= 1e-9 * abs(ref)
    assert "Sparse Cholesky factor & solve" in table
    assert all(row[6] == 1 for row in rows)  # ls_iter, schur_complement_solver.cc:329


def test_bundle_adjuster_rejects_the_step_of_a_failed_factorization(gpu, capsys, monkeypatch):
    """LinearSolverTerminationType::FAILURE (schur_complement_solver.cc:316-321):
    the driver takes no step, the trust-region loop rejects it and halves the
    radius, and the run goes on.  The first solve's info is replaced by a
    failure's; the factorization itself is not disturbed."""
    from ceres_amd import bundle_adjuster
    calls = []
    real = ca.Evaluator.sparse_cholesky_info

    def info(self):
        calls.append(real(self))
        return 10 if len(calls) == 1 else calls[-1]

    monkeypatch.setattr(ca.Evaluator, "sparse_cholesky_info", info)
    c0, c1, rows = bundle_adjuster.main(["--synthetic", SHAPES[1], "--linear_solver", "sparse_schur"])
    table = capsys.readouterr().out
    print(table)
    assert calls == [0] * 5
    assert "sparse_schur: S is not positive definite (permuted scalar column 9); the step is rejected" in table
    # (iteration, cost, new cost, |gradient|, |step|, radius, ls_iter, accepted)
    assert rows[0][7] is False and rows[0][4] == 0.0 and rows[0][6] == 1
    assert rows[1][5] == rows[0][5] / 2.0
    assert all(row[7] for row in rows[1:])
    assert c1 < c0
