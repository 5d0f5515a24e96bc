"""GPU: CGNR on the device -- the block-Jacobi preconditioner of cse_cgnr_init
against dense numpy block inverses, and cse_cgnr_solve, the reference's
conjugate gradients with every vector, scalar and stopping test on the device,
against tests/cg_reference.py.

The dense J^T J + D^2 and M^-1 of a case come from the Jacobian the evaluator
returned (tests/cgnr_solve_util.py).  The device sums in another order than
numpy: what the order of a sum may change is measured by d_ref, the gap between
cg_reference in float64 and in np.longdouble on the same inputs, and the
device's x is held to max(10 d_ref, 1e-14) of the np.longdouble x, with the
termination type, reason and iteration count equal (DESIGN 3.6c's criterion).
tests/test_cgnr_solve.py checks on the CPU that every case is a fair input.

The vector kernels are sliced, 2,048 entries per workgroup: "bal" (990
columns) is one ragged slice, "runs" (1,662) one, "slices" (4,560) two full
slices and a ragged third, the smallest shape on which the last workgroup
combines more than two partials.
"""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse, bal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cg_reference as R  # noqa: E402
import cgnr_solve_util as CU  # noqa: E402
import schur_solve_util as SU  # noqa: E402
from test_schur_gpu import RTOL, close  # noqa: E402
from test_spmv_gpu import dense_jacobian  # noqa: E402

NAN = float("nan")
FORMATS = {"bsm": ca.BLOCK_SPARSE, "crs": ca.COMPRESSED_ROW}
worst_ratio = {"value": 0.0, "case": None}  # device error / d_ref over the parity cases


def device():
    return torch.device("cuda", 0)


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device())


def filled(n, value):
    return torch.full((n,), value, dtype=torch.float64, device=device())


def options_of(o, **more):
    return _cse.cg_options(min_num_iterations=o.min_num_iterations, max_num_iterations=o.max_num_iterations,
                           residual_reset_period=o.residual_reset_period, r_tolerance=o.r_tolerance,
                           q_tolerance=o.q_tolerance, **more)


def outcome(s):
    return s.termination_type, s.reason, s.num_iterations


def evaluator_of(prog, **opts):
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(device()).cuda_stream, **opts)
    ok, _, r, _, jv = ev.evaluate()
    assert ok
    return ev, r, jv


# --------------------------------------------------------------------------
# 1. The preconditioner and the right-hand side.
# --------------------------------------------------------------------------
def two_groups():
    """Huber and Cauchy halves of one BAL problem: two groups that share
    cameras (and the points on the split)."""
    prog = bal.synthetic_program((12, 400, 1600), seed=5)
    g = prog.groups[0]
    half = g.n // 2
    idx = np.arange(g.n, dtype=np.int64)
    prog.groups = [ca.ResidualGroup(g.kind, ca.Loss.huber(1.0), g.ids[:half], g.data[:half], idx[:half]),
                   ca.ResidualGroup(g.kind, ca.Loss.cauchy(2.0), g.ids[half:], g.data[half:], idx[half:])]
    prog.compile(ca.BLOCK_SPARSE, num_eliminate_blocks=400)
    return prog


def held_cameras():
    return bal.synthetic_program((10, 300, 1500), loss=ca.Loss.huber(1.0), seed=9, constant_cameras=(0, 6))


# name -> (builder, deterministic: every group through its gradient plans)
PROGRAMS = {
    "bal_bsm": (lambda: CU.make_program("bal"), True),
    "bal_crs": (lambda: CU.make_program("bal", ca.COMPRESSED_ROW), True),
    "runs": (lambda: CU.make_program("runs"), True),
    "unobserved": (lambda: CU.make_program("unobserved"), True),
    "duplicates": (lambda: CU.make_program("duplicates"), True),
    "quaternion": (lambda: CU.make_program("quaternion"), True),
    "held_cameras": (held_cameras, False),  # the table path
    "two_groups": (two_groups, True),
    "no_distortion": (lambda: bal.synthetic_program((10, 300, 1500), loss=ca.Loss.huber(1.0), seed=9,
                                                    kind=_cse.SNAVELY_NO_DISTORTION_2_7_3), True),  # 7 x 7 blocks
}


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_preconditioner_and_rhs_match_dense(gpu, name):
    """y += M^-1 x against the dense inverse of every diagonal block of
    J^T J + D^2 to 1e-11 with D = U(0.1, 2), as test_schur_operators_match_dense
    holds the same 9 x 9 blocks; rhs = J^T b to test_schur_gpu's RTOL; repeats
    bit-identical where every group goes through its gradient plans."""
    build, deterministic = PROGRAMS[name]
    prog = build()
    ev, _, jv = evaluator_of(prog)
    try:
        if deterministic:
            assert ev.info().num_affine_groups == len(prog.groups)
        J = dense_jacobian(prog, jv)
        n, m = prog.num_effective_parameters, prog.num_residuals
        rng = np.random.default_rng(1)
        D = rng.uniform(0.1, 2.0, n)
        b = rng.normal(size=m)
        x = rng.normal(size=n)
        y0 = rng.normal(size=n)
        blocks = CU.blocks_of(prog)
        assert sum(s for _, s in blocks) == n
        M = CU.dense_block_inverse(CU.dense_operator(J, D), blocks)
        dj, dD, db, dx = to_device(jv), to_device(D), to_device(b), to_device(x)
        runs = []
        for _ in range(2):
            drhs, dy = filled(n, NAN), to_device(y0)
            ev.cgnr_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), drhs.data_ptr(), _cse.CGNR_JACOBI)
            ev.cgnr_precondition_device(dx.data_ptr(), dy.data_ptr())
            assert ev.wait() == _cse.CSE_OK
            runs.append((drhs.cpu().numpy(), dy.cpu().numpy()))
        for rhs, y in runs:
            err_rhs = np.linalg.norm(rhs - J.T @ b) / np.linalg.norm(J.T @ b)
            err_y = np.linalg.norm(y - (y0 + M @ x)) / np.linalg.norm(y0 + M @ x)
            print(f"{name}: rhs error {err_rhs:.3e}, preconditioner error {err_y:.3e}")
            assert close(rhs, J.T @ b, RTOL)
            assert close(y, y0 + M @ x, 1e-11)
        if deterministic:
            assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
        # IDENTITY: y += x, and no right-hand side asked for
        dy = to_device(y0)
        ev.cgnr_init_device(dj.data_ptr(), dD.data_ptr(), None, None, _cse.CGNR_IDENTITY)
        ev.cgnr_precondition_device(dx.data_ptr(), dy.data_ptr())
        assert ev.wait() == _cse.CSE_OK
        assert np.array_equal(dy.cpu().numpy(), y0 + x)
    finally:
        ev.close()


def test_unobserved_block_without_damping_raises_the_status(gpu):
    """D = NULL on "unobserved": the camera no block sees has G = 0, its first
    pivot is not positive: the block is left zero, cse_wait reports
    CSE_EVALUATION_FAILED, and every other block is the dense inverse."""
    prog = CU.make_program("unobserved")
    ev, _, jv = evaluator_of(prog)
    try:
        J = dense_jacobian(prog, jv)
        n = prog.num_effective_parameters
        blocks = CU.blocks_of(prog)
        A = CU.dense_operator(J, None)
        empty = [(off, s) for off, s in blocks if not np.any(J[:, off:off + s])]
        assert len(empty) == 1 and empty[0][1] == 9
        M = CU.dense_block_inverse(A, [blk for blk in blocks if blk != empty[0]])
        x = np.random.default_rng(2).normal(size=n)
        dj, dx, dy = to_device(jv), to_device(x), filled(n, 0.0)
        ev.cgnr_init_device(dj.data_ptr(), None, None, None, _cse.CGNR_JACOBI)
        ev.cgnr_precondition_device(dx.data_ptr(), dy.data_ptr())
        assert ev.wait() == _cse.CSE_EVALUATION_FAILED
        y = dy.cpu().numpy()
        off = empty[0][0]
        assert np.array_equal(y[off:off + 9], np.zeros(9))
        # Every other block was factored.  Without D the blocks are ill-conditioned, so each is
        # held to the forward error of an inverse by Cholesky, a small multiple of eps cond:
        # 1e-13 cond(block), about 1000 eps cond.
        assert np.isfinite(y).all()
        for o, s in blocks:
            if (o, s) != empty[0]:
                want = M[o:o + s, o:o + s] @ x[o:o + s]
                cond = np.linalg.cond(A[o:o + s, o:o + s])
                assert np.linalg.norm(y[o:o + s] - want) <= 1e-13 * cond * np.linalg.norm(want), (o, s, cond)
        # with D the same evaluator is fine again
        dD = filled(n, 1.0)
        ev.cgnr_init_device(dj.data_ptr(), dD.data_ptr(), None, None, _cse.CGNR_JACOBI)
        assert ev.wait() == _cse.CSE_OK
    finally:
        ev.close()


# --------------------------------------------------------------------------
# 2. Parity with cg_reference.
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_problem(which, fmt="bsm"):
    """One evaluator per problem and layout, kept for the module."""
    prog = CU.make_program(which, FORMATS[fmt])
    ev, _, jv = evaluator_of(prog)
    c = types.SimpleNamespace(which=which, prog=prog, ev=ev, J=dense_jacobian(prog, jv),
                              n=prog.num_effective_parameters, e_cols=CU.camera_columns(prog))
    c.dj, c.db, c.b = to_device(jv), to_device(SU.right_hand_side(prog)), SU.right_hand_side(prog)
    c.rhs = filled(c.n, NAN)
    c.bound = None
    c.inputs = {}
    return c


def bind(which, precond, fmt="bsm"):
    """cse_cgnr_init with `precond` and its D on the problem's evaluator,
    unless that is what it is bound to."""
    c = device_problem(which, fmt)
    if precond not in c.inputs:
        i = CU.inputs_from(c.prog, c.J, c.e_cols, c.b, precond)
        c.inputs[precond] = (i, to_device(i.D))
    c.i, c.dD = c.inputs[precond]
    if c.bound != precond:
        c.ev.cgnr_init_device(c.dj.data_ptr(), c.dD.data_ptr(), c.db.data_ptr(), c.rhs.data_ptr(), precond)
        assert c.ev.wait() == _cse.CSE_OK
        c.bound = precond
        c.rhs_host = c.rhs.cpu().numpy()
    return c


@functools.lru_cache(maxsize=None)
def reference(which, precond, option_set, fmt="bsm"):
    c = bind(which, precond, fmt)
    return CU.reference(c.i.A, c.i.Minv, c.rhs_host, option_set)


def solve(c, option_set, **more):
    """(summary, x) of one cse_cgnr_solve from the option set's start."""
    o = CU.OPTION_SETS[option_set]
    if o.start == "random":
        x = to_device(CU.initial_guess(c.i.A, c.rhs_host))
        flags = 0
    else:
        x = filled(c.n, NAN)
        flags = _cse.CG_ZERO_INITIAL_GUESS
    summary = c.ev.cgnr_solve_device(c.rhs.data_ptr(), x.data_ptr(), options_of(o.options, flags=flags, **more))
    return summary, x.cpu().numpy()


PARITY = [(w, p, s, "bsm") for w, p, s in CU.CASES] + [("bal", p, s, "crs") for w, p, s in CU.CASES if w == "bal"]


@pytest.mark.parametrize("which,precond,option_set,fmt", PARITY)
def test_parity_with_cg_reference(gpu, which, precond, option_set, fmt):
    """Termination type, reason and num_iterations are the reference's; x is
    within max(10 d_ref, 1e-14) of the np.longdouble x."""
    c = bind(which, precond, fmt)
    ref = reference(which, precond, option_set, fmt)
    assert CU.same_outcome(ref.f64, ref.ld)
    summary, x = solve(c, option_set)
    x_ld = ref.ld.x
    err = float(np.linalg.norm((x - x_ld).astype(np.float64)) / np.linalg.norm(x_ld.astype(np.float64)))
    ratio = err / ref.d_ref if ref.d_ref > 0 else 0.0
    if ratio > worst_ratio["value"]:
        worst_ratio.update(value=ratio, case=(which, precond, option_set, fmt))
    print(f"{which} {fmt} precond {precond} {option_set}: {outcome(summary)} reference {ref.ld[1:4]} "
          f"error {err:.3e} d_ref {ref.d_ref:.3e} ratio {ratio:.2f} "
          f"(worst so far {worst_ratio['value']:.2f} at {worst_ratio['case']})")
    assert outcome(summary) == (ref.ld.termination_type, ref.ld.reason, ref.ld.num_iterations)
    assert np.isfinite(x).all()
    assert err <= max(10 * ref.d_ref, 1e-14)
    if option_set == "max4":
        assert outcome(summary) == (_cse.CG_NO_CONVERGENCE, _cse.CG_REASON_MAX_ITERATIONS, 4)
    assert summary.norm_rhs == pytest.approx(float(ref.ld.norm_rhs), rel=1e-13)
    # |r| to 1 %, or to ten times what the two references disagree by: after a residual reset at
    # |r| / |b| near 1e-10 the recomputed r = b - A x is rounding of A x ("unobserved", IDENTITY).
    r_ld = float(ref.ld.norm_r)
    r_gap = abs(float(ref.f64.norm_r) - r_ld) / r_ld if r_ld > 0 else 0.0
    print(f"  |r| device {summary.norm_r:.6e} float64 {float(ref.f64.norm_r):.6e} longdouble {r_ld:.6e}")
    assert summary.norm_r == pytest.approx(r_ld, rel=max(1e-2, 10 * r_gap))
    assert summary.num_iterations_enqueued == summary.num_iterations  # check_period 1


# --------------------------------------------------------------------------
# 3. Frozen after termination: the result does not depend on check_period.
# --------------------------------------------------------------------------
def check_periods(c, option_set, periods=(1, 3, 64)):
    o = CU.OPTION_SETS[option_set].options
    runs = [solve(c, option_set, check_period=p) for p in periods]
    s0, x0 = runs[0]
    for p, (s, x) in zip(periods, runs):
        assert np.array_equal(x, x0), p
        assert outcome(s) == outcome(s0)
        assert (s.norm_r, s.zeta, s.rho, s.pq, s.q) == (s0.norm_r, s0.zeta, s0.rho, s0.pq, s0.q)
        assert s.num_iterations <= s.num_iterations_enqueued <= min(
            o.max_num_iterations, p * math.ceil(s.num_iterations / p))
        assert s.num_synchronizations <= math.ceil(s.num_iterations_enqueued / p) + 1
    return runs[0]


@pytest.mark.parametrize("which", ["bal", CU.SLICES])
def test_bit_identical_under_check_periods_and_repeats(gpu, which):
    c = bind(which, _cse.CGNR_IDENTITY)
    s, x = check_periods(c, "resets")
    assert s.termination_type == _cse.CG_SUCCESS and s.num_iterations > 3  # past a reset
    s2, x2 = solve(c, "resets")
    assert np.array_equal(x, x2) and outcome(s) == outcome(s2) and (s.norm_r, s.zeta) == (s2.norm_r, s2.zeta)
    # another cse_cgnr_init on the same evaluator, JACOBI, the periods again
    c = bind(which, _cse.CGNR_JACOBI)
    s3, x3 = check_periods(c, "zero")
    ref = reference(which, _cse.CGNR_JACOBI, "zero")
    assert outcome(s3) == (ref.ld.termination_type, ref.ld.reason, ref.ld.num_iterations)
    # ... and back: the first result, bit for bit
    c = bind(which, _cse.CGNR_IDENTITY)
    s4, x4 = solve(c, "resets", check_period=3)
    assert np.array_equal(x, x4) and outcome(s) == outcome(s4) and (s.norm_r, s.zeta) == (s4.norm_r, s4.zeta)


# --------------------------------------------------------------------------
# 4. Degenerate outcomes.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _cse.CG_ZERO_INITIAL_GUESS])
@pytest.mark.parametrize("which", ["bal", CU.SLICES])
def test_zero_rhs(gpu, which, flags):
    c = bind(which, _cse.CGNR_JACOBI)
    drhs, x = filled(c.n, 0.0), filled(c.n, NAN)
    s = c.ev.cgnr_solve_device(drhs.data_ptr(), x.data_ptr(),
                               options_of(R.Options(1, 10, 10, 1e-9, 0.0), flags=flags))
    assert outcome(s) == (_cse.CG_SUCCESS, _cse.CG_REASON_ZERO_RHS, 0)
    assert s.num_iterations_enqueued == 0 and s.num_synchronizations == 1
    assert np.array_equal(x.cpu().numpy(), np.zeros(c.n)) and s.norm_rhs == 0.0


@pytest.mark.parametrize("which", ["bal", CU.SLICES])
def test_convergence_before_the_first_iteration(gpu, which):
    """min_num_iterations 0 and a start that solves the system (:147-152)."""
    c = bind(which, _cse.CGNR_JACOBI)
    want = np.linalg.solve(c.i.A, c.rhs_host)
    x = to_device(want)
    s = c.ev.cgnr_solve_device(c.rhs.data_ptr(), x.data_ptr(), options_of(R.Options(0, 10, 10, 1e-9, 0.0)))
    assert outcome(s) == (_cse.CG_SUCCESS, _cse.CG_REASON_INITIAL_RESIDUAL, 0)
    assert s.num_iterations_enqueued == 0 and np.array_equal(x.cpu().numpy(), want)


@pytest.mark.parametrize("which", ["bal", CU.SLICES])
def test_infinite_rho_is_a_failure(gpu, which):
    """rho = r'z overflows to infinity in the first iteration (:168-172); x
    stays at the zero start."""
    c = bind(which, _cse.CGNR_IDENTITY)
    drhs, x = filled(c.n, 1e200), filled(c.n, NAN)
    s = c.ev.cgnr_solve_device(drhs.data_ptr(), x.data_ptr(),
                               options_of(R.Options(1, 10, 10, 1e-9, 0.0), flags=_cse.CG_ZERO_INITIAL_GUESS,
                                          check_period=4))
    assert outcome(s) == (_cse.CG_FAILURE, _cse.CG_REASON_RHO, 1)
    assert math.isinf(s.rho)
    assert np.array_equal(x.cpu().numpy(), np.zeros(c.n))


def test_max_iterations_is_no_convergence(gpu):
    c = bind(CU.SLICES, _cse.CGNR_IDENTITY)
    x = filled(c.n, NAN)
    s = c.ev.cgnr_solve_device(c.rhs.data_ptr(), x.data_ptr(),
                               options_of(R.Options(1, 4, 10, 1e-12, -1.0), flags=_cse.CG_ZERO_INITIAL_GUESS,
                                          check_period=3))
    assert outcome(s) == (_cse.CG_NO_CONVERGENCE, _cse.CG_REASON_MAX_ITERATIONS, 4)
    assert s.num_iterations_enqueued == 4 and np.isfinite(x.cpu().numpy()).all()


# --------------------------------------------------------------------------
# 5. The table path end to end.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["held_cameras", "two_groups"])
def test_solve_matches_dense_normal_equations(gpu, name):
    """JACOBI, r_tolerance 1e-10: x against np.linalg.solve of the dense
    normal equations to 1e-8, the bound of
    test_solve_and_back_substitution_match_dense_normal_equations.
    q_tolerance -1: the quadratic test is off, as there."""
    precond = _cse.CGNR_JACOBI
    prog = PROGRAMS[name][0]()
    ev, r, jv = evaluator_of(prog)
    try:
        J = dense_jacobian(prog, jv)
        n = prog.num_effective_parameters
        D = np.sqrt(1e-2 * np.maximum(np.sum(J * J, axis=0), 1e-6))
        b = -r
        dj, dD, db = to_device(jv), to_device(D), to_device(b)
        rhs, x = filled(n, NAN), filled(n, NAN)
        ev.cgnr_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), precond)
        o = _cse.cg_options(max_num_iterations=5000, r_tolerance=1e-10, q_tolerance=-1.0,
                            flags=_cse.CG_ZERO_INITIAL_GUESS, check_period=16)
        s = ev.cgnr_solve_device(rhs.data_ptr(), x.data_ptr(), o)
        assert ev.wait() == _cse.CSE_OK
        print(name, precond, outcome(s), s.norm_r / s.norm_rhs)
        assert (s.termination_type, s.reason) == (_cse.CG_SUCCESS, _cse.CG_REASON_R_TOLERANCE)
        ref = np.linalg.solve(J.T @ J + np.diag(D * D), J.T @ b)
        got = x.cpu().numpy()
        assert np.linalg.norm(got - ref) <= 1e-8 * np.linalg.norm(ref)
    finally:
        ev.close()


# --------------------------------------------------------------------------
# 6. Refusals.
# --------------------------------------------------------------------------
def test_refusals(gpu):
    dev = device()
    L = _cse.lib()
    prog = bal.synthetic_program((10, 300, 1500), seed=9)
    n = prog.num_effective_parameters
    buf = torch.zeros(4, n, dtype=torch.float64, device=dev)
    rhs, x = buf[0].data_ptr(), buf[1].data_ptr()
    summary = _cse.cse_cg_summary()

    def call(ev, options=_cse.cg_options(), d_rhs=rhs, d_x=x, s=summary):
        rc = L.cse_cgnr_solve(ev.handle, None if options is None else C.byref(options), d_rhs, d_x,
                              None if s is None else C.byref(s))
        if rc < 0:
            assert _cse.last_error(), "a refusal without a message"
        return rc

    # a multi-device handle
    ev = ca.Evaluator(prog, devices=[0, 0])
    assert call(ev) == _cse.CSE_ERR_UNSUPPORTED and "cse_create_multi" in _cse.last_error()
    assert L.cse_cgnr_init(ev.handle, rhs, None, None, None, 0) == _cse.CSE_ERR_UNSUPPORTED
    assert "cse_create_multi" in _cse.last_error()
    assert L.cse_cgnr_precondition(ev.handle, rhs, x) == _cse.CSE_ERR_UNSUPPORTED
    ev.close()
    ev, r, jv = evaluator_of(prog)
    # before cse_cgnr_init
    assert call(ev) == _cse.CSE_ERR_INVALID and "cse_cgnr_init has not run" in _cse.last_error()
    assert L.cse_cgnr_precondition(ev.handle, rhs, x) == _cse.CSE_ERR_INVALID
    assert "cse_cgnr_init has not run" in _cse.last_error()
    dj, db = to_device(jv), to_device(-r)
    # cse_cgnr_init's own arguments
    assert L.cse_cgnr_init(ev.handle, None, None, None, None, 0) == _cse.CSE_ERR_INVALID
    assert "d_jacobian_values" in _cse.last_error()
    for d_b, d_rhs in ((db.data_ptr(), None), (None, rhs)):
        assert L.cse_cgnr_init(ev.handle, dj.data_ptr(), None, d_b, d_rhs, 0) == _cse.CSE_ERR_INVALID
        assert "d_b and d_rhs" in _cse.last_error()
    assert L.cse_cgnr_init(ev.handle, dj.data_ptr(), None, None, None, 2) == _cse.CSE_ERR_INVALID
    assert "unknown preconditioner" in _cse.last_error()
    assert call(ev) == _cse.CSE_ERR_INVALID  # none of those bound anything
    ev.cgnr_init_device(dj.data_ptr(), None, db.data_ptr(), buf[2].data_ptr(), _cse.CGNR_IDENTITY)
    # null pointers
    for kw in (dict(options=None), dict(s=None), dict(d_rhs=None), dict(d_x=None)):
        assert call(ev, **kw) == _cse.CSE_ERR_INVALID, kw
        assert "null" in _cse.last_error()
    for a, b in ((None, x), (rhs, None)):
        assert L.cse_cgnr_precondition(ev.handle, a, b) == _cse.CSE_ERR_INVALID and "null" in _cse.last_error()
    assert L.cse_cgnr_precondition(ev.handle, rhs, rhs) == _cse.CSE_ERR_INVALID and "overlap" in _cse.last_error()
    # the options' ranges
    for field, value in (("check_period", 0), ("residual_reset_period", 0), ("max_num_iterations", 0),
                         ("min_num_iterations", -1), ("reserved", 1), ("flags", 2)):
        assert call(ev, options=_cse.cg_options(**{field: value})) == _cse.CSE_ERR_INVALID, field
        assert field.split("_")[0] in _cse.last_error() and "cse_cgnr_solve" in _cse.last_error()
    # d_x overlapping d_rhs
    both = torch.zeros(n + n // 2, dtype=torch.float64, device=dev)
    for a, b in ((both, both), (both, both[n // 2:]), (both[n // 2:], both), (both[n - 1:], both)):
        assert call(ev, d_rhs=a.data_ptr(), d_x=b.data_ptr()) == _cse.CSE_ERR_INVALID
        assert "overlaps" in _cse.last_error()
    # and a solve goes through, every termination type CSE_OK
    lm = _cse.cg_options(q_tolerance=0.1, max_num_iterations=50)
    assert call(ev, options=lm, d_rhs=buf[2].data_ptr()) == _cse.CSE_OK
    assert summary.num_iterations >= 1 and summary.num_synchronizations >= 2
    assert call(ev, options=_cse.cg_options(max_num_iterations=1, r_tolerance=1e-30),
                d_rhs=buf[2].data_ptr()) == _cse.CSE_OK
    assert summary.termination_type == _cse.CG_NO_CONVERGENCE
    ev.close()
    # blocks that do not tile the columns: the last two cameras share theirs.
    # JACOBI is refused, IDENTITY is not.
    prog = bal.synthetic_program((10, 300, 1500), seed=9)
    prog.delta_offset = np.array(prog.delta_offset).copy()
    prog.delta_offset[-1] = prog.delta_offset[-2]
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    assert L.cse_cgnr_init(ev.handle, dj.data_ptr(), None, None, None, _cse.CGNR_JACOBI) == _cse.CSE_ERR_UNSUPPORTED
    assert "tile" in _cse.last_error()
    assert L.cse_cgnr_init(ev.handle, dj.data_ptr(), None, None, None, _cse.CGNR_IDENTITY) == _cse.CSE_OK
    ev.close()
    # a block of 17 tangent columns (no residual block uses it: the library's kinds stop at 10):
    # JACOBI is refused, IDENTITY is not
    prog = bal.synthetic_program((10, 300, 1500), seed=9, compile=False)
    prog.pb_size = np.append(prog.pb_size, 17).astype(np.int32)
    prog.pb_tangent = np.append(prog.pb_tangent, 17).astype(np.int32)
    prog.pb_constant = np.append(prog.pb_constant, 0).astype(np.int32)
    prog.pb_plus_jacobian = np.append(prog.pb_plus_jacobian, -1).astype(np.int64)
    prog.state = np.concatenate([prog.state, np.zeros(17)])
    prog.compile(ca.BLOCK_SPARSE, num_eliminate_blocks=300)
    assert prog.num_effective_parameters == n + 17
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    big = torch.zeros(prog.num_jacobian_values, dtype=torch.float64, device=dev)
    assert L.cse_cgnr_init(ev.handle, big.data_ptr(), None, None, None, _cse.CGNR_JACOBI) == _cse.CSE_ERR_UNSUPPORTED
    assert "at most 16 tangent columns" in _cse.last_error() and "17" in _cse.last_error()
    assert L.cse_cgnr_init(ev.handle, big.data_ptr(), None, None, None, _cse.CGNR_IDENTITY) == _cse.CSE_OK
    ev.close()
    # a descriptor without a Jacobian layout: all three calls refuse
    prog = bal.synthetic_program((10, 300, 1500), seed=9)
    prog.jacobian_per_residual_layout = None
    prog.jacobian_per_residual_offsets = None
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    assert L.cse_cgnr_init(ev.handle, dj.data_ptr(), None, None, None, _cse.CGNR_IDENTITY) == _cse.CSE_ERR_INVALID
    assert "no Jacobian layout" in _cse.last_error()
    assert L.cse_cgnr_precondition(ev.handle, rhs, x) == _cse.CSE_ERR_INVALID
    assert "no Jacobian layout" in _cse.last_error()
    assert call(ev) == _cse.CSE_ERR_INVALID and "no Jacobian layout" in _cse.last_error()
    ev.close()


# --------------------------------------------------------------------------
# 7. The driver.
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driver_run(solver):
    from ceres_amd import bundle_adjuster
    from test_schur_held_gpu import DRIVER
    extra = {"iterative_schur": [], "cgnr": ["--linear_solver", "cgnr"],
             "device_cgnr": ["--linear_solver", "cgnr", "--device_cgnr"]}[solver]
    return bundle_adjuster.main(DRIVER + extra)


def test_bundle_adjuster_device_cgnr(gpu, capsys):
    """--device_cgnr on test_schur_held_gpu's DRIVER arguments: every step
    accepted and the cost falling.  The host loop and the device solver solve
    the same system to the same eta with different preconditioners; what
    differs is where each PCG stops, so their final-cost gap is held to the
    gap iterative_schur leaves to the host cgnr, times 10, plus 1e-12 of the
    cost: that file's own rule."""
    final = {}
    for solver in ("iterative_schur", "cgnr", "device_cgnr"):
        c0, c1, rows = driver_run(solver)
        costs = [c0] + [row[2] for row in rows]
        assert all(row[7] for row in rows), (solver, rows)
        assert all(b < a for a, b in zip(costs[:-1], costs[1:])), (solver, costs)
        assert all(row[6] > 0 for row in rows)
        assert c1 == costs[-1]
        final[solver] = c1
    gap = abs(final["device_cgnr"] - final["cgnr"])
    yardstick = abs(final["iterative_schur"] - final["cgnr"])
    print(capsys.readouterr().out)
    print(f"final-cost gap device_cgnr vs host cgnr {gap:.3e}; iterative_schur vs host cgnr {yardstick:.3e}")
    assert gap <= 10 * yardstick + 1e-12 * final["cgnr"]
