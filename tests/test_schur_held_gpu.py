"""GPU: ITERATIVE_SCHUR's operators and the device PCG with held (constant) cameras.

A block whose camera is held (Problem::SetParameterBlockConstant) has an E cell
and no F cell: in every formula of tests/test_schur_gpu.py F_b = 0 for it.  The
held camera has no column, so S, rhs and the preconditioner have 9 x (active
cameras) rows; M_p, E^T z and the gradient's e rows still sum over all blocks
of a point.  The kHeld kernels (csrc/schur_kernels.hpp) find a block's F cell
by its rank among the blocks with an active camera and a camera's x by its
rank among the active cameras; checked here against the dense numpy formulas
of tests/test_schur_gpu.py on the Jacobian the evaluator returned (dense_
jacobian leaves a held camera out, so E and F are the right ones as they
stand), at that file's tolerances: 1e-12 norm-wise for rhs, S x and the e part
of the back substitution, 1e-11 for the preconditioner.
"""
import functools
import types

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse, bal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import schur_solve_util as SU  # noqa: E402
from test_constant_gpu import held  # noqa: E402
from test_schur_gpu import block_inverse, close, dense_schur  # noqa: E402
from test_spmv_gpu import dense_jacobian  # noqa: E402

PRECONDITIONERS = [_cse.SCHUR_IDENTITY, _cse.SCHUR_JACOBI, _cse.SCHUR_SCHUR_JACOBI]
WAVE = 64


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def empty(n):
    return torch.full((n,), float("nan"), dtype=torch.float64, device=torch.device("cuda", 0))


def schur_chunks(pi):
    """The planner's chunk rule on the point index of every block: runs of one
    point packed into wave chunks of whole runs, a run longer than a wave big
    and no chunk across it.  ([begin, end) chunks, [begin, end) big runs)."""
    n = len(pi)
    starts = [0] + [i for i in range(1, n) if pi[i] != pi[i - 1]] + [n]
    chunks, big, lo = [], [], 0
    for i, j in zip(starts[:-1], starts[1:]):
        if j - i > WAVE:
            if i > lo:
                chunks.append((lo, i))
            big.append((i, j))
            lo = j
        elif j - lo > WAVE:
            chunks.append((lo, i))
            lo = i
    if n > lo:
        chunks.append((lo, n))
    return chunks, big


@functools.lru_cache(maxsize=None)
def boundary_problem():
    """test_schur_gpu.runs_problem(seed=3)'s recipe (runs of 1 .. 130 blocks, 140
    cameras, distinct cameras per point) with the cameras of these blocks held:
    block 0 (point 0's only block), both blocks of point 1, the first and last
    row of the 70-run, rows 63 and 64 of the 130-run, the last block.  That
    puts held lanes where the kernels' addressing can go wrong, asserted below
    so that a change of recipe cannot lose them: 8 held cameras and 72 held
    blocks of 1,022; points 0, 1 and 133 seen by held cameras alone; one wave
    chunk entirely held, two with lane 0 held, three with their last lane held;
    held rows on both sides of a big run's 64-row stride."""
    seed = 3
    rng = np.random.default_rng(seed)
    counts = [1, 2, 70, 3, 130, 64, 65, 5, 4, 6, 63, 1, 66, 2] + list(rng.integers(1, 9, 120))
    C = 140
    P = len(counts)
    cams, pts, _, _, _ = bal.synthetic(C, P, P, seed=seed)
    ci = np.concatenate([rng.permutation(C)[:k] for k in counts]).astype(np.int32)
    pi = np.repeat(np.arange(P, dtype=np.int32), counts)
    obs = bal.project(cams, pts, ci, pi) + rng.normal(0, 1.0, (len(ci), 2))
    n = len(ci)
    first = np.concatenate([[0], np.cumsum(counts)])
    rows = [0, 1, 2, first[2], first[2] + 69, first[4] + 63, first[4] + 64, n - 1]
    held_cams = sorted({int(ci[b]) for b in rows})
    is_held = np.isin(ci, held_cams)
    # the facts the cases below rely on
    assert (len(held_cams), int(is_held.sum()), n) == (8, 72, 1022)
    alone = [p for p in range(P) if is_held[first[p]:first[p + 1]].all()]
    assert alone == [0, 1, 133]
    chunks, big = schur_chunks(pi)
    masks = [is_held[a:b] for a, b in chunks]
    assert sum(m.all() for m in masks) == 1
    assert sum(m[0] for m in masks) == 2  # the chunk that is all held among them
    assert sum(m[-1] for m in masks) == 3
    assert any(is_held[a + WAVE - 1] and is_held[a + WAVE] for a, b in big)
    prog = bal.program(cams, pts, ci, pi, obs, loss=ca.Loss.huber(1.0), constant_cameras=held_cams)
    return prog, held_cams


def evaluated(prog):
    """(ev, r, g, jv, J, e_cols, f_cols) of a program on the current stream."""
    dev = torch.device("cuda", 0)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, cost, r, g, jv = ev.evaluate()
    assert ok
    e_cols, f_cols = ev.schur_structure()
    return ev, r, g, jv, dense_jacobian(prog, jv), e_cols, f_cols


def check_operators(prog, precond, num_active, gradient=False):
    ev, r, g, jv, J, e_cols, f_cols = evaluated(prog)
    n, m = prog.num_effective_parameters, prog.num_residuals
    assert f_cols == 9 * num_active and e_cols + f_cols == n and e_cols % 3 == 0
    rng = np.random.default_rng(1)
    D = rng.uniform(0.1, 2.0, n)
    b = -r if gradient else rng.normal(size=m)
    x = rng.normal(size=f_cols)
    y0 = rng.normal(size=f_cols)
    E, F, Minv, S, rhs = dense_schur(J, e_cols, D, b)
    dj, dD, db, dx = to_device(jv), to_device(D), to_device(b), to_device(x)
    drhs, dy, dy2, dback = empty(f_cols), empty(f_cols), empty(f_cols), empty(n)
    dp = to_device(y0)
    if gradient:
        dg = empty(n)
        ev.schur_init_gradient_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), drhs.data_ptr(),
                                      dg.data_ptr(), precond)
    else:
        ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), drhs.data_ptr(), precond)
    ev.schur_multiply_device(dx.data_ptr(), dy.data_ptr())
    ev.schur_multiply_device(dx.data_ptr(), dy2.data_ptr())
    ev.schur_precondition_device(dx.data_ptr(), dp.data_ptr())
    ev.schur_back_substitute_device(dx.data_ptr(), dback.data_ptr())
    assert ev.wait() == _cse.CSE_OK
    assert close(drhs.cpu().numpy(), rhs)
    assert close(dy.cpu().numpy(), S @ x)
    assert torch.equal(dy, dy2)  # fixed-order sums: bit-identical
    back = dback.cpu().numpy()
    assert close(back[:e_cols], Minv @ (E.T @ (b - F @ x)))
    assert np.array_equal(back[e_cols:], x)
    if precond == _cse.SCHUR_IDENTITY:
        P = np.eye(f_cols)
    elif precond == _cse.SCHUR_JACOBI:
        P = block_inverse(F.T @ F + np.diag(D[e_cols:] ** 2), 9)
    else:
        P = block_inverse(S, 9)
    assert close(dp.cpu().numpy(), y0 + P @ x, 1e-11)
    if gradient:
        # g = J^T r over the effective parameters: a held camera has no row in it
        got = dg.cpu().numpy()
        assert got.shape == (n,) and np.isfinite(got).all()
        assert close(got, J.T @ r, 1e-12)
        assert close(got, g, 1e-12)
    ev.close()


@pytest.mark.parametrize("const", [(0,), (7,), (15,), (0, 3, 9, 15)])
@pytest.mark.parametrize("precond", PRECONDITIONERS)
def test_operators_match_dense(gpu, const, precond):
    check_operators(held(counts=(16, 700, 2900), const=const), precond, 16 - len(const))


def test_operators_match_dense_on_the_quaternion_manifold(gpu):
    prog = held(counts=(16, 700, 2900), const=(0, 3, 9, 15), quaternion_manifold=True)
    check_operators(prog, _cse.SCHUR_SCHUR_JACOBI, 12)


@pytest.mark.parametrize("gradient", [False, True], ids=["init", "init_gradient"])
@pytest.mark.parametrize("precond", PRECONDITIONERS)
def test_boundary_problem(gpu, precond, gradient):
    prog, held_cams = boundary_problem()
    check_operators(prog, precond, 140 - len(held_cams), gradient)


def test_almost_every_camera_held(gpu):
    """One active camera: most chunks have no F cell at all."""
    check_operators(held(counts=(10, 2000, 9000), const=range(1, 10)), _cse.SCHUR_JACOBI, 1)


def test_pcg_solve_matches_dense_normal_equations(gpu):
    """test_schur_gpu's host-loop PCG (JACOBI) and back substitution on the
    boundary problem against a dense solve of (J^T J + D^2) dx = J^T b, at its
    1e-8; then cse_schur_solve and its back substitution on the same system."""
    prog, _ = boundary_problem()
    dev = torch.device("cuda", 0)
    ev, r, g, jv, J, e_cols, f_cols = evaluated(prog)
    n = prog.num_effective_parameters
    D = np.sqrt(1e-2 * np.maximum(np.sum(J * J, axis=0), 1e-6))
    b = -r
    dj, dD, db = to_device(jv), to_device(D), to_device(b)
    rhs = empty(f_cols)
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), _cse.SCHUR_JACOBI)
    xf = torch.zeros(f_cols, dtype=torch.float64, device=dev)
    res = rhs.clone()
    z = torch.zeros_like(res)
    ev.schur_precondition_device(res.data_ptr(), z.data_ptr())
    p = z.clone()
    rz = torch.dot(res, z)
    Ap = torch.empty_like(p)
    for _ in range(2000):
        ev.schur_multiply_device(p.data_ptr(), Ap.data_ptr())
        alpha = rz / torch.dot(p, Ap)
        xf += alpha * p
        res -= alpha * Ap
        if float(res.norm()) <= 1e-12 * float(rhs.norm()):
            break
        z.zero_()
        ev.schur_precondition_device(res.data_ptr(), z.data_ptr())
        rz_new = torch.dot(res, z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    dx = empty(n)
    ev.schur_back_substitute_device(xf.data_ptr(), dx.data_ptr())
    assert ev.wait() == _cse.CSE_OK
    ref = np.linalg.solve(J.T @ J + np.diag(D * D), J.T @ b)
    got = dx.cpu().numpy()
    err_host = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    # the whole solve on the device
    xd, step = empty(f_cols), empty(n)
    o = _cse.cg_options(r_tolerance=1e-12, q_tolerance=-1.0, max_num_iterations=2000,
                        flags=_cse.CG_ZERO_INITIAL_GUESS)
    s = ev.schur_solve_device(rhs.data_ptr(), xd.data_ptr(), o, None, step.data_ptr())
    err_dev = np.linalg.norm(step.cpu().numpy() - ref) / np.linalg.norm(ref)
    print(f"host loop error {err_host:.3e}; cse_schur_solve {s.num_iterations} iterations, error {err_dev:.3e}")
    assert err_host <= 1e-8
    assert s.termination_type == _cse.CG_SUCCESS
    assert err_dev <= 1e-8
    ev.close()


@functools.lru_cache(maxsize=None)
def solve_problem():
    """The boundary problem bound as tests/test_schur_solve_gpu.py binds its
    problems: SU.damping's D (its docstring says why a parity test with
    cg_reference needs that much camera damping) and SU.right_hand_side."""
    prog, _ = boundary_problem()
    ev, r, g, jv, J, e_cols, f_cols = evaluated(prog)
    D = SU.damping(J, e_cols)
    c = types.SimpleNamespace(ev=ev, J=J, D=D, e_cols=e_cols, f_cols=f_cols, bound=None)
    c.S = dense_schur(J, e_cols, D, np.zeros(prog.num_residuals))[3]
    c.dj, c.dD, c.db = to_device(jv), to_device(D), to_device(SU.right_hand_side(prog))
    c.rhs = empty(f_cols)
    return c


@pytest.mark.parametrize("precond,option_set",
                         [(p, s) for p in PRECONDITIONERS for s, o in SU.OPTION_SETS.items()
                          if not (o.identity_only and p != _cse.SCHUR_IDENTITY)])
def test_device_pcg_parity_with_cg_reference(gpu, precond, option_set):
    """tests/test_schur_solve_gpu.py's criterion on the boundary problem:
    termination type, reason and iteration count are cg_reference's, and x is
    within max(10 d_ref, 1e-14) of the np.longdouble x."""
    c = solve_problem()
    if c.bound != precond:
        c.ev.schur_init_device(c.dj.data_ptr(), c.dD.data_ptr(), c.db.data_ptr(), c.rhs.data_ptr(), precond)
        assert c.ev.wait() == _cse.CSE_OK
        c.bound = precond
        c.rhs_host = c.rhs.cpu().numpy()
    ref = SU.reference(c.S, SU.dense_preconditioner(precond, c.S, c.J, c.e_cols, c.D), c.rhs_host, option_set)
    assert SU.same_outcome(ref.f64, ref.ld)
    o = SU.OPTION_SETS[option_set]
    if o.start == "random":
        x, flags = to_device(SU.initial_guess(c.S, c.rhs_host)), 0
    else:
        x, flags = empty(c.f_cols), _cse.CG_ZERO_INITIAL_GUESS
    q = o.options
    options = _cse.cg_options(min_num_iterations=q.min_num_iterations, max_num_iterations=q.max_num_iterations,
                              residual_reset_period=q.residual_reset_period, r_tolerance=q.r_tolerance,
                              q_tolerance=q.q_tolerance, flags=flags)
    s = c.ev.schur_solve_device(c.rhs.data_ptr(), x.data_ptr(), options, None)
    got = x.cpu().numpy()
    x_ld = ref.ld.x
    err = float(np.linalg.norm((got - x_ld).astype(np.float64)) / np.linalg.norm(x_ld.astype(np.float64)))
    print(f"precond {precond} {option_set}: {(s.termination_type, s.reason, s.num_iterations)} reference "
          f"{ref.ld[1:4]} error {err:.3e} d_ref {ref.d_ref:.3e}")
    assert (s.termination_type, s.reason, s.num_iterations) == (ref.ld.termination_type, ref.ld.reason,
                                                                ref.ld.num_iterations)
    assert np.isfinite(got).all()
    assert err <= max(10 * ref.d_ref, 1e-14)


def test_init_reports_singular_point_blocks_without_D(gpu):
    """As the unheld test: with d_D = NULL the points seen once have a singular
    E^T E and cse_wait says so; with a positive D everything factors, and no
    held camera raises the status (it has no block to factor)."""
    prog, _ = boundary_problem()
    ev, r, g, jv, J, e_cols, f_cols = evaluated(prog)
    dj, db = to_device(jv), to_device(-r)
    rhs = empty(f_cols)
    ev.schur_init_device(dj.data_ptr(), None, db.data_ptr(), rhs.data_ptr(), _cse.SCHUR_JACOBI)
    assert ev.wait() == _cse.CSE_EVALUATION_FAILED
    assert torch.isfinite(rhs).all()
    dD = to_device(np.full(prog.num_effective_parameters, 0.5))
    for precond in PRECONDITIONERS:
        ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), precond)
        assert ev.wait() == _cse.CSE_OK
    ev.close()


def test_explicit_complements_are_refused(gpu):
    prog = held(counts=(16, 700, 2900), const=(0, 3), loss=ca.Loss.huber(1.0))
    ev, r, g, jv, J, e_cols, f_cols = evaluated(prog)
    dj, db = to_device(jv), to_device(-r)
    dD = to_device(np.full(prog.num_effective_parameters, 0.5))
    rhs, x = empty(f_cols), empty(f_cols)
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), _cse.SCHUR_JACOBI)
    buf = torch.zeros(max(f_cols * f_cols, 81 * 200), dtype=torch.float64, device=torch.device("cuda", 0))
    refused = r"failed \(-4\).*held cameras"
    with pytest.raises(RuntimeError, match=refused):
        ev.schur_complement_plan()
    with pytest.raises(RuntimeError, match=refused):
        ev.schur_complement_device(buf.data_ptr())
    with pytest.raises(RuntimeError, match=refused):
        ev.schur_complement_sparse_counts()
    with pytest.raises(RuntimeError, match=refused):
        ev.schur_complement_sparse_device(buf.data_ptr())
    with pytest.raises(RuntimeError, match=refused):
        ev.schur_explicit_multiply_device(buf.data_ptr(), rhs.data_ptr(), x.data_ptr())
    with pytest.raises(RuntimeError, match=refused):
        ev.schur_solve_device(rhs.data_ptr(), x.data_ptr(), _cse.cg_options(), buf.data_ptr())
    # the implicit operator is served
    s = ev.schur_solve_device(rhs.data_ptr(), x.data_ptr(),
                              _cse.cg_options(r_tolerance=1e-6, flags=_cse.CG_ZERO_INITIAL_GUESS), None)
    assert s.termination_type == _cse.CG_SUCCESS
    ev.close()


DRIVER = ["--synthetic", "problem-16-22106", "--robustify", "--point_sigma", "0.05", "--num_iterations", "3",
          "--eta", "1e-10"]


@functools.lru_cache(maxsize=None)
def driver_run(solver, held_cameras):
    from ceres_amd import bundle_adjuster
    extra = {"iterative_schur": [], "device_pcg": ["--device_pcg"], "cgnr": ["--linear_solver", "cgnr"]}[solver]
    return bundle_adjuster.main(DRIVER + extra + ["--held_cameras", str(held_cameras)])


def test_bundle_adjuster_with_held_cameras(gpu, capsys):
    """--held_cameras 2: every step accepted and the cost falling, for
    iterative_schur (host loop and --device_pcg) and cgnr.  The two solvers
    solve the same system to the same eta; what differs is where each PCG
    stops, so their final-cost gap is held to the gap the same pair leaves
    with --held_cameras 0, times 10, plus 1e-12 of the cost."""
    final = {}
    for solver in ("iterative_schur", "device_pcg", "cgnr"):
        c0, c1, rows = driver_run(solver, 2)
        costs = [c0] + [row[2] for row in rows]
        assert all(row[7] for row in rows), (solver, rows)
        assert all(b < a for a, b in zip(costs[:-1], costs[1:])), (solver, costs)
        assert c1 == costs[-1]
        final[solver] = c1
    gap_held = abs(final["iterative_schur"] - final["cgnr"])
    gap_free = abs(driver_run("iterative_schur", 0)[1] - driver_run("cgnr", 0)[1])
    out = capsys.readouterr().out
    print(out)
    print(f"final-cost gap iterative_schur vs cgnr: held {gap_held:.3e}, unheld {gap_free:.3e}; "
          f"host loop vs device PCG, held: {abs(final['iterative_schur'] - final['device_pcg']):.3e}")
    assert gap_held <= 10 * gap_free + 1e-12 * final["cgnr"]
