"""GPU: the block-sparse Schur complement (cse_schur_complement_sparse_structure,
cse_schur_complement_sparse) and the product with it (cse_schur_explicit_multiply).

The structure is BlockRandomAccessSparseMatrix's: the 9 x 9 blocks of S's upper
triangle for every co-visible camera pair plus every diagonal block, as
block-compressed rows.  The values are held to the dense S that
cse_schur_complement forms on the same init, bit for bit (the same sums in the
same order, by two store paths: a block of one 64-pair chunk is stored by its
chunk, a longer one by the finish), and through it to numpy
(test_schur_complement_gpu.check_bounds).  The product is held to the device
values scattered into a dense symmetric matrix, per entry, and to the implicit
operator cse_schur_multiply; then a PCG on it to the dense normal equations, and
bundle_adjuster --use_explicit_schur_complement to the two existing solvers.
"""
import functools
import types

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse, bal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import schur_complement_util as U  # noqa: E402
from test_schur_complement_gpu import check_bounds  # noqa: E402
from test_schur_gpu import runs_problem  # noqa: E402
from test_spmv_gpu import dense_jacobian  # noqa: E402

WIDE = "wide"
CASES = U.CASES + [(WIDE, True)]


def make_program(which):
    if which == WIDE:
        # 7,533 of 11,325 upper blocks, up to 115 blocks in a row, 10 blocks above 64 pairs
        return bal.synthetic_program((150, 2000, 8000), loss=ca.Loss.huber(1.0), seed=3)
    return U.make_program(which)


def pair_counts(prog, e_cols):
    """(C, C) brute force: the residual-block pairs summed into block (c, c'),
    sum over the points of m_c m_c' (m_c = the point's blocks of camera c)."""
    ccol, pcol, _ = U.structure(prog)
    C = (prog.num_effective_parameters - e_cols) // 9
    M = np.zeros((e_cols // 3, C), np.int64)
    np.add.at(M, (pcol // 3, (ccol - e_cols) // 9), 1)
    return M.T @ M


def scatter(values, row_begin, block_col):
    """The blocks into a dense symmetric matrix (off-diagonal blocks mirrored)."""
    C = len(row_begin) - 1
    S = np.zeros((C, 9, C, 9))
    rows = np.repeat(np.arange(C), np.diff(row_begin))
    S[rows, :, block_col, :] = values
    off = rows != block_col
    S[block_col[off], :, rows[off], :] = values[off].transpose(0, 2, 1)
    return S.reshape(9 * C, 9 * C)


@functools.lru_cache(maxsize=None)
def run_case(which, with_D):
    """Everything the device computes for one problem, once; the tests below
    read it."""
    prog = make_program(which)
    dev = torch.device("cuda", 0)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, r, _, jv = ev.evaluate()
    assert ok
    n, m = prog.num_effective_parameters, prog.num_residuals
    e_cols, f_cols = ev.schur_structure()
    rng = np.random.default_rng(1)
    D = U.damping(prog, with_D)
    b = rng.normal(size=m)
    x = rng.normal(size=f_cols)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dj, db, dx = t(jv), t(b), t(x)
    dD = t(D) if with_D else None
    rhs = torch.empty(f_cols, dtype=torch.float64, device=dev)
    c = types.SimpleNamespace(which=which, with_D=with_D, prog=prog, jv=jv, D=D, e_cols=e_cols,
                              f_cols=f_cols, x=x)
    # before any init, and before anything is uploaded: the counts alone
    c.counts_before = ev.schur_complement_sparse_counts()
    c.plan = ev.schur_complement_plan()
    c.row_begin, c.block_col, c.device_bytes = ev.schur_complement_sparse_structure()
    c.counts_after = ev.schur_complement_sparse_counts()
    nb = len(c.block_col)
    precond = _cse.SCHUR_JACOBI if with_D else _cse.SCHUR_IDENTITY
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr() if with_D else None, db.data_ptr(),
                         rhs.data_ptr(), precond)
    assert ev.wait() == _cse.CSE_OK
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    V1, V2, S = nan(nb, 9, 9), nan(nb, 9, 9), nan(f_cols, f_cols)
    ev.schur_complement_sparse_device(V1.data_ptr())
    ev.schur_complement_sparse_device(V2.data_ptr())
    ev.schur_complement_device(S.data_ptr())
    y1, y2, yi = nan(f_cols), nan(f_cols), nan(f_cols)
    ev.schur_explicit_multiply_device(V1.data_ptr(), dx.data_ptr(), y1.data_ptr())
    ev.schur_explicit_multiply_device(V1.data_ptr(), dx.data_ptr(), y2.data_ptr())
    ev.schur_multiply_device(dx.data_ptr(), yi.data_ptr())
    assert ev.wait() == _cse.CSE_OK
    c.V1, c.V2, c.S = V1.cpu().numpy(), V2.cpu().numpy(), S.cpu().numpy()
    c.y1, c.y2, c.yi, c.x_after = y1.cpu().numpy(), y2.cpu().numpy(), yi.cpu().numpy(), dx.cpu().numpy()
    # another binding on the same evaluator: the cached structure carries no values
    c.D2 = np.random.default_rng(7).uniform(0.1, 2.0, n)
    dD2, db2 = t(c.D2), t(rng.normal(size=m))
    ev.schur_init_device(dj.data_ptr(), dD2.data_ptr(), db2.data_ptr(), rhs.data_ptr(),
                         _cse.SCHUR_IDENTITY)
    V3, S3 = nan(nb, 9, 9), nan(f_cols, f_cols)
    ev.schur_complement_sparse_device(V3.data_ptr())
    ev.schur_complement_device(S3.data_ptr())
    assert ev.wait() == _cse.CSE_OK
    c.V3, c.S3 = V3.cpu().numpy(), S3.cpu().numpy()
    ev.close()
    return c


def dense_blocks(S, row_begin, block_col):
    C = len(row_begin) - 1
    rows = np.repeat(np.arange(C), np.diff(row_begin))
    return S.reshape(C, 9, C, 9)[rows, :, block_col, :]


@pytest.mark.parametrize("which,with_D", CASES)
def test_sparse_structure(gpu, which, with_D):
    c = run_case(which, with_D)
    C = c.f_cols // 9
    want = U.covisible_blocks(c.prog, c.e_cols)
    observed = {a for a, _ in want}
    unobserved = C - len(observed)
    assert unobserved == (1 if which == "unobserved" else 0)
    want |= {(a, a) for a in range(C)}
    assert c.row_begin.dtype == np.int64 and c.block_col.dtype == np.int32
    assert c.row_begin.shape == (C + 1,) and c.row_begin[0] == 0 and c.row_begin[-1] == len(c.block_col)
    rows = np.repeat(np.arange(C), np.diff(c.row_begin))
    got = list(zip(rows.tolist(), c.block_col.tolist()))
    assert got == sorted(want)  # lexicographic: rows ascending, the diagonal first
    assert len(c.block_col) == c.plan[0] + unobserved
    assert c.counts_before == (C, len(c.block_col), c.device_bytes)
    assert c.counts_after == c.counts_before  # the uploaded structure is the counted one
    assert c.device_bytes >= 16 * (C + 1) + 4 * len(c.block_col)


@pytest.mark.parametrize("which,with_D", CASES)
def test_sparse_values_are_the_dense_blocks(gpu, which, with_D):
    c = run_case(which, with_D)
    assert not np.isnan(c.V1).any()  # every value assigned
    want = dense_blocks(c.S, c.row_begin, c.block_col)
    assert np.array_equal(c.V1, want)  # the same sums in the same order
    diag = c.V1[c.row_begin[:-1]]
    assert np.array_equal(diag, diag.transpose(0, 2, 1))
    assert np.array_equal(c.V1, c.V2)  # fixed-order sums: bit-identical
    # the dense matrix holds nothing else
    assert np.array_equal(scatter(c.V1, c.row_begin, c.block_col), c.S)
    if which == "unobserved":
        k = c.row_begin[3]
        assert c.row_begin[4] == k + 1
        d = c.D[c.e_cols + 27:c.e_cols + 36] ** 2 if with_D else np.zeros(9)
        assert np.array_equal(c.V1[k], np.diag(d))


@pytest.mark.parametrize("which,with_D", CASES)
def test_sparse_values_take_both_store_paths(gpu, which, with_D):
    """A block of at most 64 pairs (one chunk) is stored by the chunk kernel,
    a longer one by the finish: the problems have both kinds."""
    c = run_case(which, with_D)
    pairs = pair_counts(c.prog, c.e_cols)
    rows = np.repeat(np.arange(len(c.row_begin) - 1), np.diff(c.row_begin))
    per_block = pairs[rows, c.block_col]
    assert int(np.triu(pairs).sum()) == c.plan[1]
    print(f"{which}: {(per_block <= 64).sum()} blocks of <= 64 pairs, {(per_block > 64).sum()} of > 64")
    if which in ("bal", WIDE):
        assert (per_block > 64).any() and ((per_block > 0) & (per_block <= 64)).any()
    if which == "bal":
        assert (per_block <= 64).sum() == 15 and (per_block > 64).sum() == 40
    if which == WIDE:
        C = len(c.row_begin) - 1
        assert len(c.block_col) == 7533 and (per_block > 64).sum() == 10
        assert np.diff(c.row_begin).max() == 115          # rows cut over the waves
        assert len(c.block_col) < C * (C + 1) // 2 and C > 1  # empty blocks inside rows, many workgroups
        gaps = [np.any(np.diff(c.block_col[a:b]) > 1) for a, b in zip(c.row_begin[:-1], c.row_begin[1:])]
        assert any(gaps)


def check_bounds_by_points(got, prog, J, e_cols, D, what):
    """check_bounds' criteria -- 1e-12 in norm and, per block, 1e-12 of the
    magnitude of the summed terms; blocks of cameras that share no point
    exactly zero -- for the 150-camera problem, where check_bounds' dense
    formulas (E^T E is 6000 x 6000, J 16000 x 7350) take tens of seconds.  The
    reference is U.schur_longdouble, point by point; the magnitude
    |F|^T |F| + D_f^2 + |F^T E| |M| |E^T F| is accumulated point by point too,
    which is the same matrix: every row of J belongs to one point, so F^T E and
    M are block-diagonal by point."""
    ref = U.schur_longdouble(prog, J, e_cols, D).astype(np.float64)
    f_cols = J.shape[1] - e_cols
    B = np.diag(D[e_cols:] ** 2)
    ccol, pcol, row0 = U.structure(prog)
    for p in np.unique(pcol):
        blocks = np.nonzero(pcol == p)[0]
        rows = np.stack([row0[blocks], row0[blocks] + 1], 1).ravel()
        Ep = J[rows, p:p + 3]
        M = np.linalg.inv(Ep.T @ Ep + np.diag(D[p:p + 3] ** 2))
        cols = (np.unique(ccol[blocks])[:, None] + np.arange(9)[None, :]).ravel()
        Fp = J[np.ix_(rows, cols)]
        FtE = np.abs(Fp.T @ Ep)
        B[np.ix_(cols - e_cols, cols - e_cols)] += np.abs(Fp).T @ np.abs(Fp) + FtE @ np.abs(M) @ FtE.T
    bound = U.block_norms(B)
    norm_ratio = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    err = U.block_norms(got - ref)
    live = bound > 0
    block_ratio = (err[live] / bound[live]).max()
    print(f"{what}: |dS|/|S| {norm_ratio:.3e}, worst block error / magnitude {block_ratio:.3e}")
    assert got.shape == (f_cols, f_cols) and np.isfinite(got).all()
    assert norm_ratio <= U.RTOL
    assert block_ratio <= U.RTOL
    assert (err[~live] == 0).all() and (~live).any()  # this problem has cameras that share no point


def against_numpy(c, values, D, what):
    J = dense_jacobian(c.prog, c.jv)
    check = check_bounds_by_points if c.which == WIDE else check_bounds
    check(scatter(values, c.row_begin, c.block_col), *((c.prog,) if c.which == WIDE else ()), J, c.e_cols, D,
          what)


@pytest.mark.parametrize("which,with_D", CASES)
def test_sparse_values_match_numpy(gpu, which, with_D):
    c = run_case(which, with_D)
    against_numpy(c, c.V1, c.D, f"{which} D={with_D}")


@pytest.mark.parametrize("which,with_D", CASES)
def test_sparse_values_follow_a_new_init(gpu, which, with_D):
    c = run_case(which, with_D)
    assert not np.isnan(c.V3).any()
    assert np.array_equal(c.V3, dense_blocks(c.S3, c.row_begin, c.block_col))
    assert not np.array_equal(c.V3, c.V1)
    against_numpy(c, c.V3, c.D2, f"{which} after re-init")


@pytest.mark.parametrize("which,with_D", CASES)
def test_explicit_multiply(gpu, which, with_D):
    c = run_case(which, with_D)
    assert not np.isnan(c.y1).any()  # every entry assigned
    Sd = scatter(c.V1, c.row_begin, c.block_col)
    # a-priori: 2 n 2^-53 with n <= 9 * 150 terms, about 3e-13, numpy's own error included
    err, bound = np.abs(c.y1 - Sd @ c.x), 1e-12 * (np.abs(Sd) @ np.abs(c.x))
    live = bound > 0
    print(f"{which} D={with_D}: worst |y - S x|_i / (|S| |x|)_i = {(err[live] / bound[live]).max() * 1e-12:.3e}")
    assert (err <= bound).all()
    assert np.linalg.norm(c.y1 - c.yi) <= U.RTOL * np.linalg.norm(c.yi)  # the implicit operator
    assert np.array_equal(c.y1, c.y2)
    assert np.array_equal(c.x_after, c.x)


def test_sparse_refusals(gpu):
    dev = torch.device("cuda", 0)
    refuse = lambda code: pytest.raises(RuntimeError, match=rf"cse_schur_\w+ failed \({code}\)")
    buf = torch.zeros(81 * 55, dtype=torch.float64, device=dev)
    xy = torch.zeros(2, 90, dtype=torch.float64, device=dev)
    every = lambda ev: (lambda: ev.schur_complement_sparse_counts(),
                        lambda: ev.schur_complement_sparse_structure(),
                        lambda: ev.schur_complement_sparse_device(buf.data_ptr()),
                        lambda: ev.schur_explicit_multiply_device(buf.data_ptr(), xy[0].data_ptr(),
                                                                  xy[1].data_ptr()))
    # not Schur-eligible
    prog = bal.synthetic_program((10, 300, 1500), format=ca.COMPRESSED_ROW, seed=9)
    ev = ca.Evaluator(prog)
    for call in every(ev):
        with refuse(_cse.CSE_ERR_UNSUPPORTED):
            call()
    ev.close()
    # a multi-device handle
    prog = bal.synthetic_program((10, 300, 1500), seed=9)
    ev = ca.Evaluator(prog, devices=[0, 0])
    for call in every(ev):
        with refuse(_cse.CSE_ERR_UNSUPPORTED):
            call()
    ev.close()
    # before cse_schur_init: the structure, not the values or the product
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, r, _, jv = ev.evaluate()
    e_cols, f_cols = ev.schur_structure()
    assert f_cols == 90
    assert ev.schur_complement_sparse_counts()[:2] == (10, 55)
    row_begin, block_col, _ = ev.schur_complement_sparse_structure()
    assert len(block_col) == 55 and row_begin[-1] == 55
    calls = every(ev)
    for call in calls[2:]:
        with refuse(_cse.CSE_ERR_INVALID):
            call()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dj, db = t(jv), t(-r)
    rhs = torch.empty(f_cols, dtype=torch.float64, device=dev)
    ev.schur_init_device(dj.data_ptr(), None, db.data_ptr(), rhs.data_ptr(), _cse.SCHUR_IDENTITY)
    # null pointers
    with refuse(_cse.CSE_ERR_INVALID):
        ev.schur_complement_sparse_device(None)
    for args in ((None, xy[0].data_ptr(), xy[1].data_ptr()), (buf.data_ptr(), None, xy[1].data_ptr()),
                 (buf.data_ptr(), xy[0].data_ptr(), None)):
        with refuse(_cse.CSE_ERR_INVALID):
            ev.schur_explicit_multiply_device(*args)
    # x and y that overlap
    both = torch.zeros(135, dtype=torch.float64, device=dev)
    for x, y in ((both, both), (both, both[45:]), (both[45:], both), (both[89:], both)):
        with refuse(_cse.CSE_ERR_INVALID):
            ev.schur_explicit_multiply_device(buf.data_ptr(), x.data_ptr(), y.data_ptr())
    for call in calls[2:]:
        call()
    assert ev.wait() == _cse.CSE_OK
    ev.close()


@pytest.mark.parametrize("which", ["bal", "unobserved"])
def test_sparse_after_the_dense_complement(gpu, which):
    """The dense cse_schur_complement first: the pair plan is on the device
    already when the block-sparse structure is built, which then takes the
    plan's block tables from there.  Same structure, same values."""
    c = run_case(which, True)
    dev = torch.device("cuda", 0)
    ev = ca.Evaluator(c.prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dj, dD, db = t(c.jv), t(c.D), t(np.zeros(c.prog.num_residuals))
    rhs = torch.empty(c.f_cols, dtype=torch.float64, device=dev)
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), _cse.SCHUR_JACOBI)
    S = torch.full((c.f_cols, c.f_cols), float("nan"), dtype=torch.float64, device=dev)
    ev.schur_complement_device(S.data_ptr())
    V = torch.full((len(c.block_col), 9, 9), float("nan"), dtype=torch.float64, device=dev)
    ev.schur_complement_sparse_device(V.data_ptr())
    row_begin, block_col, device_bytes = ev.schur_complement_sparse_structure()
    assert ev.wait() == _cse.CSE_OK
    assert np.array_equal(row_begin, c.row_begin) and np.array_equal(block_col, c.block_col)
    assert device_bytes == c.device_bytes
    assert np.array_equal(S.cpu().numpy(), c.S)
    assert np.array_equal(V.cpu().numpy(), c.V1)
    ev.close()


@pytest.mark.parametrize("which", ["runs", "duplicates"])
def test_explicit_pcg_solve_matches_dense_normal_equations(gpu, which):
    """SolveReducedLinearSystemUsingConjugateGradients end to end: the blocks of
    S from the device, a float64 PCG in numpy on cse_schur_explicit_multiply
    (block Jacobi from the diagonal blocks) to a relative residual of 1e-12,
    back substitution on the device."""
    prog = runs_problem(seed=8) if which == "runs" else U.duplicates_problem()
    dev = torch.device("cuda", 0)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, r, _, jv = ev.evaluate()
    J = dense_jacobian(prog, jv)
    n = prog.num_effective_parameters
    e_cols, f_cols = ev.schur_structure()
    D = np.sqrt(1e-2 * np.maximum(np.sum(J * J, axis=0), 1e-6))
    b = -r
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dj, dD, db = t(jv), t(D), t(b)
    rhs = torch.empty(f_cols, dtype=torch.float64, device=dev)
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(),
                         _cse.SCHUR_IDENTITY)
    row_begin, block_col, _ = ev.schur_complement_sparse_structure()
    V = torch.empty(len(block_col), 9, 9, dtype=torch.float64, device=dev)
    ev.schur_complement_sparse_device(V.data_ptr())
    assert ev.wait() == _cse.CSE_OK
    Minv = np.linalg.inv(V.cpu().numpy()[row_begin[:-1]])
    dp = torch.empty(f_cols, dtype=torch.float64, device=dev)
    dAp = torch.empty_like(dp)

    def multiply(p):
        dp.copy_(torch.from_numpy(p))
        ev.schur_explicit_multiply_device(V.data_ptr(), dp.data_ptr(), dAp.data_ptr())
        assert ev.wait() == _cse.CSE_OK
        return dAp.cpu().numpy()

    precondition = lambda v: np.einsum("cij,cj->ci", Minv, v.reshape(-1, 9)).ravel()
    rhs_h = rhs.cpu().numpy()
    xf, res = np.zeros(f_cols), rhs_h.copy()
    z = precondition(res)
    p, rz = z.copy(), res @ z
    for it in range(5000):
        Ap = multiply(p)
        alpha = rz / (p @ Ap)
        xf += alpha * p
        res -= alpha * Ap
        if np.linalg.norm(res) <= 1e-12 * np.linalg.norm(rhs_h):
            break
        z = precondition(res)
        rz_new = res @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    assert np.linalg.norm(res) <= 1e-12 * np.linalg.norm(rhs_h), it
    dxf = t(xf)
    dx = torch.empty(n, dtype=torch.float64, device=dev)
    ev.schur_back_substitute_device(dxf.data_ptr(), dx.data_ptr())
    torch.cuda.synchronize(dev)
    ref = np.linalg.solve(J.T @ J + np.diag(D * D), J.T @ b)
    assert np.linalg.norm(dx.cpu().numpy() - ref) <= 1e-8 * np.linalg.norm(ref)
    ev.close()


def test_bundle_adjuster_explicit_schur_complement(gpu, capsys):
    """The explicit PCG against the two existing solvers: its final cost is as
    close to dense_schur's (the exact solve) as another PCG stopped at the
    same eta -- the explicit and the implicit PCG apply the same operator to
    rounding but may stop one iteration apart, hence the factor 10."""
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", "problem-16-22106", "--robustify", "--point_sigma", "0.05",
            "--num_iterations", "4"]
    c0, c_explicit, rows = bundle_adjuster.main(base + ["--use_explicit_schur_complement"])
    table = capsys.readouterr().out
    _, c_iterative, _ = bundle_adjuster.main(base)
    _, c_dense, _ = bundle_adjuster.main(base + ["--linear_solver", "dense_schur"])
    capsys.readouterr()
    print(table)
    print(f"final cost: explicit {c_explicit:.9e} iterative {c_iterative:.9e} dense {c_dense:.9e}")
    costs = [r[1] for r in rows] + [c_explicit]
    assert c_explicit < 0.9 * c0
    assert all(b <= a for a, b in zip(costs, costs[1:]))  # monotone
    assert all(r[-1] for r in rows)                       # every step successful
    assert all(r[6] > 0 for r in rows)                    # ls_iter
    assert abs(c_explicit - c_dense) <= 10 * abs(c_iterative - c_dense) + 1e-12 * c_dense


def test_bundle_adjuster_explicit_refuses_above_max_schur_gb(gpu):
    from ceres_amd import bundle_adjuster
    with pytest.raises(SystemExit, match="max_schur_gb"):
        bundle_adjuster.main(["--synthetic", "problem-16-22106", "--num_iterations", "1",
                              "--use_explicit_schur_complement", "--max_schur_gb", "0.0001"])
