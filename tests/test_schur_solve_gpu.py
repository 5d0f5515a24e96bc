"""GPU: cse_schur_solve, the reference's conjugate gradients with every vector,
scalar and stopping test on the device, against tests/cg_reference.py.

The dense S and M^-1 of a case come from the Jacobian the evaluator returned
(tests/schur_solve_util.py: schur_float64, block_inverse); the right-hand side
is the one cse_schur_init wrote.  The device sums in another order than numpy:
what the order of a sum may change is measured by d_ref, the gap between
cg_reference in float64 and in np.longdouble on the same inputs, and the
device's x is held to max(10 d_ref, 1e-14) of the np.longdouble x, with the
termination type, reason and iteration count equal.  tests/test_schur_solve.py
checks on the CPU that every case is a fair input (float64 and np.longdouble
end alike).

The vector kernels are one workgroup for every vector length (csrc/
cg_kernels.hpp), so there is no size at which their launch shape changes and
no pair of problems around one; test_long_vectors runs 65,700 entries, 64
strided passes of the 1,024 lanes.
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
import schur_complement_util as U  # noqa: E402
import schur_solve_util as SU  # noqa: E402
from test_schur_gpu import runs_problem  # noqa: E402
from test_spmv_gpu import dense_jacobian  # noqa: E402

NAN = float("nan")
worst_ratio = {"value": 0.0, "case": None}  # device error / d_ref over the parity cases


def to_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def filled(n, value):
    return torch.full((n,), value, dtype=torch.float64, device=torch.device("cuda", 0))


def options_of(o, **more):
    return _cse.cg_options(min_num_iterations=o.min_num_iterations, max_num_iterations=o.max_num_iterations,
                           residual_reset_period=o.residual_reset_period, r_tolerance=o.r_tolerance,
                           q_tolerance=o.q_tolerance, **more)


def outcome(s):
    return s.termination_type, s.reason, s.num_iterations


@functools.lru_cache(maxsize=None)
def device_problem(which):
    """One evaluator per problem, kept for the module: its Jacobian, D, the
    dense S, and the block-sparse structure uploaded."""
    dev = torch.device("cuda", 0)
    prog = SU.make_program(which)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, _, _, jv = ev.evaluate()
    assert ok
    J = dense_jacobian(prog, jv)
    e_cols, f_cols = ev.schur_structure()
    D = SU.damping(J, e_cols)
    c = types.SimpleNamespace(which=which, prog=prog, ev=ev, J=J, D=D, e_cols=e_cols, f_cols=f_cols)
    c.S = SU.dense_operator(prog, J, e_cols, D)
    c.dj, c.dD, c.db = to_device(jv), to_device(D), to_device(SU.right_hand_side(prog))
    c.rhs = filled(f_cols, NAN)
    _, block_col, _ = ev.schur_complement_sparse_structure()
    c.values = filled(81 * len(block_col), NAN)
    c.bound = None
    return c


def bind(which, precond):
    """cse_schur_init with `precond` (and S's values after it) on the problem's
    evaluator, unless that is what it is bound to."""
    c = device_problem(which)
    if c.bound != precond:
        c.ev.schur_init_device(c.dj.data_ptr(), c.dD.data_ptr(), c.db.data_ptr(), c.rhs.data_ptr(), precond)
        c.ev.schur_complement_sparse_device(c.values.data_ptr())
        assert c.ev.wait() == _cse.CSE_OK
        c.bound = precond
        c.rhs_host = c.rhs.cpu().numpy()
    return c


@functools.lru_cache(maxsize=None)
def reference(which, precond, option_set):
    c = bind(which, precond)
    Minv = SU.dense_preconditioner(precond, c.S, c.J, c.e_cols, c.D)
    return SU.reference(c.S, Minv, c.rhs_host, option_set)


def solve(c, option_set, explicit, **more):
    """(summary, x) of one cse_schur_solve from the option set's start."""
    o = SU.OPTION_SETS[option_set]
    if o.start == "random":
        x = to_device(SU.initial_guess(c.S, c.rhs_host))
        flags = 0
    else:
        x = filled(c.f_cols, NAN)
        flags = _cse.CG_ZERO_INITIAL_GUESS
    summary = c.ev.schur_solve_device(c.rhs.data_ptr(), x.data_ptr(), options_of(o.options, flags=flags, **more),
                                      c.values.data_ptr() if explicit else None)
    return summary, x.cpu().numpy()


@pytest.mark.parametrize("explicit", [False, True], ids=["implicit", "explicit"])
@pytest.mark.parametrize("which,precond,option_set", SU.CASES)
def test_parity_with_cg_reference(gpu, which, precond, option_set, explicit):
    """Termination type, reason and num_iterations are the reference's; x is
    within max(10 d_ref, 1e-14) of the np.longdouble x.  Worst device error /
    d_ref over the cases measured: see DESIGN 3.6c."""
    c = bind(which, precond)
    ref = reference(which, precond, option_set)
    assert SU.same_outcome(ref.f64, ref.ld)
    summary, x = solve(c, option_set, explicit)
    x_ld = ref.ld.x
    err = float(np.linalg.norm((x - x_ld).astype(np.float64)) / np.linalg.norm(x_ld.astype(np.float64)))
    ratio = err / ref.d_ref if ref.d_ref > 0 else 0.0
    if ratio > worst_ratio["value"]:
        worst_ratio.update(value=ratio, case=(which, precond, option_set, explicit))
    print(f"{which} precond {precond} {option_set} {'explicit' if explicit else 'implicit'}: "
          f"{outcome(summary)} reference {ref.ld[1:4]} error {err:.3e} d_ref {ref.d_ref:.3e} "
          f"ratio {ratio:.2f} (worst so far {worst_ratio['value']:.2f} at {worst_ratio['case']})")
    assert outcome(summary) == (ref.ld.termination_type, ref.ld.reason, ref.ld.num_iterations)
    assert np.isfinite(x).all()
    assert err <= max(10 * ref.d_ref, 1e-14)
    if option_set == "max4":
        assert outcome(summary) == (_cse.CG_NO_CONVERGENCE, _cse.CG_REASON_MAX_ITERATIONS, 4)
    assert summary.norm_rhs == pytest.approx(float(ref.ld.norm_rhs), rel=1e-13)
    assert summary.norm_r == pytest.approx(float(ref.ld.norm_r), rel=1e-2)
    assert summary.num_iterations_enqueued == summary.num_iterations  # check_period 1


# --------------------------------------------------------------------------
# Two cameras: 18 columns, under one wave; the test writes S's blocks itself.
# (The operators need two cameras: a single camera's slot-0 ids are sorted,
# which the fused-gradient path the Schur operators sit on does not take, so
# cse_schur_structure refuses a one-camera problem.)
# --------------------------------------------------------------------------
N2 = 18


@functools.lru_cache(maxsize=None)
def two_cameras():
    dev = torch.device("cuda", 0)
    prog = U._program(2, [[0, 1], [1], [0], [1, 0]] * 5, 12)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, r, _, jv = ev.evaluate()
    assert ok
    e_cols, f_cols = ev.schur_structure()
    assert f_cols == N2
    c = types.SimpleNamespace(ev=ev, n=prog.num_effective_parameters)
    c.keep = (to_device(jv), filled(c.n, 1.0), to_device(-r), filled(N2, NAN))
    ev.schur_init_device(c.keep[0].data_ptr(), c.keep[1].data_ptr(), c.keep[2].data_ptr(),
                         c.keep[3].data_ptr(), _cse.SCHUR_IDENTITY)
    c.row_begin, c.block_col, _ = ev.schur_complement_sparse_structure()
    assert list(c.row_begin) == [0, 2, 3] and list(c.block_col) == [0, 1, 1]
    assert ev.wait() == _cse.CSE_OK
    return c


def solve_block(block, rhs, x0, options, step=None):
    """S = diag(block, I9): `block` is camera 0's diagonal block, the
    off-diagonal block is zero; rhs and x0 are padded with zeros."""
    c = two_cameras()
    blocks = np.stack([np.asarray(block, np.float64), np.zeros((9, 9)), np.eye(9)])
    pad = lambda v: np.concatenate([np.asarray(v, np.float64), np.zeros(N2 - len(v))])
    values, drhs, x = to_device(blocks.reshape(-1)), to_device(pad(rhs)), to_device(pad(x0))
    summary = c.ev.schur_solve_device(drhs.data_ptr(), x.data_ptr(), options, values.data_ptr(),
                                      None if step is None else step.data_ptr())
    got = x.cpu().numpy()
    assert np.array_equal(got[9:], np.zeros(9))  # camera 1: rhs 0, start 0
    return summary, got[:9]


def embedded(case):
    A = np.eye(9)
    A[:3, :3] = case["A"]
    pad = lambda v: np.concatenate([np.asarray(v, np.float64), np.zeros(6)])
    return A, pad(case["b"]), pad(case["x0"]), pad(case["x"])


def test_known_answers_in_one_block(gpu):
    """conjugate_gradients_solver_test.cc:47-152 embedded in a 9 x 9 diagonal
    block (identity elsewhere, rhs and start 0 there): x to ASSERT_DOUBLE_EQ's
    4 ulp."""
    from test_schur_solve import kat_cases, ulps_apart
    for case in kat_cases():
        A, b, x0, want = embedded(case)
        summary, x = solve_block(A, b, x0, options_of(R.Options(**case["options"])))
        print(case["name"], outcome(summary), x)
        assert summary.termination_type == _cse.CG_SUCCESS and summary.reason == _cse.CG_REASON_R_TOLERANCE
        if case["num_iterations"] is not None:
            assert summary.num_iterations == case["num_iterations"]
        host = R.solve(A, b, x0, R.Options(**case["options"]))
        assert summary.num_iterations == host.num_iterations
        for have, expect in zip(x, want):
            assert ulps_apart(float(have), expect) <= 4, (have, expect)


def test_negative_definite_block_is_indefinite(gpu):
    x0 = np.linspace(-1.0, 1.0, 9)
    summary, x = solve_block(-np.diag(np.arange(1.0, 10.0)), np.ones(9), x0,
                             options_of(R.Options(1, 10, 10, 1e-9, 0.0), check_period=4))
    assert outcome(summary) == (_cse.CG_NO_CONVERGENCE, _cse.CG_REASON_INDEFINITE, 1)
    assert summary.pq < 0
    assert np.array_equal(x, x0)


@pytest.mark.parametrize("flags", [0, _cse.CG_ZERO_INITIAL_GUESS])
def test_zero_rhs(gpu, flags):
    c = two_cameras()
    drhs, x = filled(N2, 0.0), filled(N2, NAN)
    values = to_device(np.stack([np.eye(9), np.zeros((9, 9)), np.eye(9)]).reshape(-1))
    summary = c.ev.schur_solve_device(drhs.data_ptr(), x.data_ptr(),
                                      options_of(R.Options(1, 10, 10, 1e-9, 0.0), flags=flags),
                                      values.data_ptr())
    assert outcome(summary) == (_cse.CG_SUCCESS, _cse.CG_REASON_ZERO_RHS, 0)
    assert summary.num_iterations_enqueued == 0 and summary.num_synchronizations == 1
    assert np.array_equal(x.cpu().numpy(), np.zeros(N2)) and summary.norm_rhs == 0.0


def test_convergence_before_the_first_iteration(gpu):
    """min_num_iterations 0 and a start that solves the system (:147-152)."""
    want = np.arange(1.0, 10.0)
    A = np.diag(np.arange(2.0, 11.0))
    summary, x = solve_block(A, A @ want, want, options_of(R.Options(0, 10, 10, 1e-9, 0.0)))
    assert outcome(summary) == (_cse.CG_SUCCESS, _cse.CG_REASON_INITIAL_RESIDUAL, 0)
    assert summary.num_iterations_enqueued == 0 and np.array_equal(x, want)


def test_failure_leaves_the_step_untouched(gpu):
    """rho = r'z overflows to infinity in the first iteration: FAILURE, and no
    back substitution (iterative_schur_complement_solver.cc:63-170)."""
    c = two_cameras()
    step = filled(c.n, NAN)
    summary, x = solve_block(np.eye(9), np.full(9, 1e200), np.zeros(9),
                             options_of(R.Options(1, 10, 10, 1e-9, 0.0), flags=_cse.CG_ZERO_INITIAL_GUESS),
                             step)
    assert outcome(summary) == (_cse.CG_FAILURE, _cse.CG_REASON_RHO, 1)
    assert math.isinf(summary.rho)
    assert torch.isnan(step).all()
    # ... and with a finite right-hand side the step is written
    summary, x = solve_block(np.eye(9), np.ones(9), np.zeros(9),
                             options_of(R.Options(1, 10, 10, 1e-9, -1.0)), step)
    assert summary.termination_type == _cse.CG_SUCCESS
    got = step.cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got[-N2:-9], x)


# --------------------------------------------------------------------------
# Frozen after termination: the result does not depend on check_period.
# --------------------------------------------------------------------------
def check_periods(c, option_set, explicit, periods=(1, 3, 64)):
    o = SU.OPTION_SETS[option_set].options
    runs = [solve(c, option_set, explicit, check_period=p) for p in periods]
    s0, x0 = runs[0]
    for p, (s, x) in zip(periods, runs):
        assert np.array_equal(x, x0), p
        assert (s.num_iterations, s.reason, s.termination_type) == (s0.num_iterations, s0.reason,
                                                                    s0.termination_type)
        assert (s.norm_r, s.zeta, s.rho, s.pq, s.q) == (s0.norm_r, s0.zeta, s0.rho, s0.pq, s0.q)
        assert s.num_iterations <= s.num_iterations_enqueued <= min(
            o.max_num_iterations, p * math.ceil(s.num_iterations / p))
        assert s.num_synchronizations <= math.ceil(s.num_iterations_enqueued / p) + 1
    return runs[0]


@pytest.mark.parametrize("explicit", [False, True], ids=["implicit", "explicit"])
@pytest.mark.parametrize("which", ["runs", SU.WIDE])
def test_frozen_after_termination(gpu, which, explicit):
    c = bind(which, _cse.SCHUR_IDENTITY)
    s, x = check_periods(c, "resets", explicit)
    assert s.termination_type == _cse.CG_SUCCESS and s.num_iterations > 3  # past a reset
    # two identical calls are bit-identical
    s2, x2 = solve(c, "resets", explicit)
    assert np.array_equal(x, x2) and outcome(s) == outcome(s2) and s.norm_r == s2.norm_r
    # another cse_schur_init on the same evaluator, then a solve
    c = bind(which, _cse.SCHUR_JACOBI)
    ref = reference(which, _cse.SCHUR_JACOBI, "zero")
    s3, x3 = solve(c, "zero", explicit, check_period=5)
    assert outcome(s3) == (ref.ld.termination_type, ref.ld.reason, ref.ld.num_iterations)
    err = np.linalg.norm((x3 - ref.ld.x).astype(np.float64)) / np.linalg.norm(ref.ld.x.astype(np.float64))
    assert err <= max(10 * ref.d_ref, 1e-14)


# --------------------------------------------------------------------------
# Long vectors: 7,300 cameras, f_cols = 65,700.
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_problem():
    """8,000 points seen by 2 or 3 of 7,300 cameras each (with D): a short
    evaluation, a small S, long vectors."""
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(21)
    cams = 7300
    lists = [[int(v) for v in rng.choice(cams, size=int(rng.integers(2, 4)), replace=False)]
             for _ in range(8000)]
    prog = U._program(cams, lists, 21)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, r, _, jv = ev.evaluate()
    assert ok
    n, m = prog.num_effective_parameters, prog.num_residuals
    e_cols, f_cols = ev.schur_structure()
    assert f_cols == 9 * cams >= 65700
    c = types.SimpleNamespace(ev=ev, f_cols=f_cols)
    c.dj, c.db = to_device(jv), to_device(-r)
    # diag(J^T J) by one left multiply of the squared values, as the driver
    diag = torch.zeros(n, dtype=torch.float64, device=dev)
    ones = torch.ones(m, dtype=torch.float64, device=dev)
    ev.left_multiply_device((c.dj * c.dj).data_ptr(), ones.data_ptr(), diag.data_ptr())
    D = torch.ones(n, dtype=torch.float64, device=dev)
    D[e_cols:] = torch.sqrt(1e-3 * diag[e_cols:].max())
    c.dD = D
    c.rhs = filled(f_cols, NAN)
    ev.schur_init_device(c.dj.data_ptr(), c.dD.data_ptr(), c.db.data_ptr(), c.rhs.data_ptr(), _cse.SCHUR_JACOBI)
    _, block_col, _ = ev.schur_complement_sparse_structure()
    c.values = filled(81 * len(block_col), NAN)
    ev.schur_complement_sparse_device(c.values.data_ptr())
    assert ev.wait() == _cse.CSE_OK
    return c


def test_long_vectors(gpu):
    """JACOBI, r_tolerance 1e-8, zero start, both operators: SUCCESS; the true
    residual from one cse_schur_multiply is within 2 r_tolerance |rhs| (the
    recurrence's drift is O(eps cond) and far below 1e-8: the 2 is slack);
    implicit and explicit x agree to 1e-6; the result does not depend on
    check_period.  q_tolerance -1: the quadratic test is off, as in
    schur_solve_util's "resets"."""
    c = long_problem()
    r_tol = 1e-8
    xs = []
    for explicit in (False, True):
        results = []
        for period in (1, 3, 64):
            x = filled(c.f_cols, NAN)
            o = _cse.cg_options(max_num_iterations=300, r_tolerance=r_tol, q_tolerance=-1.0,
                                flags=_cse.CG_ZERO_INITIAL_GUESS, check_period=period)
            s = c.ev.schur_solve_device(c.rhs.data_ptr(), x.data_ptr(), o,
                                        c.values.data_ptr() if explicit else None)
            results.append((s, x))
            assert s.num_iterations_enqueued <= min(300, period * math.ceil(s.num_iterations / period))
            assert s.num_synchronizations <= math.ceil(s.num_iterations_enqueued / period) + 1
        s0, x0 = results[0]
        print(f"explicit {explicit}: {outcome(s0)} |r|/|b| {s0.norm_r / s0.norm_rhs:.3e}")
        assert (s0.termination_type, s0.reason) == (_cse.CG_SUCCESS, _cse.CG_REASON_R_TOLERANCE)
        assert s0.num_iterations > 1
        for s, x in results[1:]:
            assert torch.equal(x, x0) and outcome(s) == outcome(s0) and s.norm_r == s0.norm_r
        y = filled(c.f_cols, NAN)
        c.ev.schur_multiply_device(x0.data_ptr(), y.data_ptr())
        assert c.ev.wait() == _cse.CSE_OK
        true_residual = float((c.rhs - y).norm())
        assert true_residual <= 2 * r_tol * float(c.rhs.norm())
        assert s0.norm_rhs == pytest.approx(float(c.rhs.norm()), rel=1e-12)
        xs.append(x0)
    assert float((xs[0] - xs[1]).norm()) <= 1e-6 * float(xs[0].norm())


# --------------------------------------------------------------------------
# End to end, refusals, the driver.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("explicit", [False, True], ids=["implicit", "explicit"])
def test_solve_and_back_substitution_match_dense_normal_equations(gpu, explicit):
    """test_schur_gpu.py's test_schur_pcg_solve_matches_dense_normal_equations
    as one call: JACOBI, r_tolerance 1e-12, at most 2000 iterations, d_step
    given.  q_tolerance -1: at |r| / |b| near 1e-8 the quadratic model's
    decrease is below its rounding and a q_tolerance of 0 would stop there."""
    prog = runs_problem(seed=8)
    dev = torch.device("cuda", 0)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, cost, r, g, jv = ev.evaluate()
    J = dense_jacobian(prog, jv)
    n = prog.num_effective_parameters
    e_cols, f_cols = ev.schur_structure()
    D = np.sqrt(1e-2 * np.maximum(np.sum(J * J, axis=0), 1e-6))
    b = -r
    dj, dD, db = to_device(jv), to_device(D), to_device(b)
    rhs = filled(f_cols, NAN)
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), _cse.SCHUR_JACOBI)
    values = None
    if explicit:
        _, block_col, _ = ev.schur_complement_sparse_structure()
        values = filled(81 * len(block_col), NAN)
        ev.schur_complement_sparse_device(values.data_ptr())
    xf, step = filled(f_cols, NAN), filled(n, NAN)
    o = _cse.cg_options(max_num_iterations=2000, r_tolerance=1e-12, q_tolerance=-1.0,
                        flags=_cse.CG_ZERO_INITIAL_GUESS, check_period=8)
    s = ev.schur_solve_device(rhs.data_ptr(), xf.data_ptr(), o, None if values is None else values.data_ptr(),
                              step.data_ptr())
    assert ev.wait() == _cse.CSE_OK
    print(outcome(s), s.norm_r / s.norm_rhs)
    assert (s.termination_type, s.reason) == (_cse.CG_SUCCESS, _cse.CG_REASON_R_TOLERANCE)
    ref = np.linalg.solve(J.T @ J + np.diag(D * D), J.T @ b)
    got = step.cpu().numpy()
    assert np.array_equal(got[e_cols:], xf.cpu().numpy())
    assert np.linalg.norm(got - ref) <= 1e-8 * np.linalg.norm(ref)
    ev.close()


def test_refusals(gpu):
    dev = torch.device("cuda", 0)
    L = _cse.lib()
    prog = bal.synthetic_program((10, 300, 1500), seed=9)
    buf = torch.zeros(4, 90, dtype=torch.float64, device=dev)
    rhs, x = buf[0].data_ptr(), buf[1].data_ptr()
    summary = _cse.cse_cg_summary()

    def call(ev, options=_cse.cg_options(), values=None, d_rhs=rhs, d_x=x, s=summary):
        rc = L.cse_schur_solve(ev.handle, None if options is None else C.byref(options), values, d_rhs, d_x,
                               None, None if s is None else C.byref(s))
        if rc < 0:
            assert _cse.last_error(), "a refusal without a message"
        return rc

    # a multi-device handle
    ev = ca.Evaluator(prog, devices=[0, 0])
    assert call(ev) == _cse.CSE_ERR_UNSUPPORTED and "cse_create_multi" in _cse.last_error()
    ev.close()
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, r, _, jv = ev.evaluate()
    assert ev.schur_structure()[1] == 90
    # before cse_schur_init
    assert call(ev) == _cse.CSE_ERR_INVALID and "cse_schur_init has not run" in _cse.last_error()
    dj, db = to_device(jv), to_device(-r)
    ev.schur_init_device(dj.data_ptr(), None, db.data_ptr(), buf[2].data_ptr(), _cse.SCHUR_IDENTITY)
    # null pointers
    for kw in (dict(options=None), dict(s=None), dict(d_rhs=None), dict(d_x=None)):
        assert call(ev, **kw) == _cse.CSE_ERR_INVALID, kw
        assert "null" in _cse.last_error()
    # the options' ranges
    for field, value in (("check_period", 0), ("residual_reset_period", 0), ("max_num_iterations", 0),
                         ("min_num_iterations", -1), ("reserved", 1), ("flags", 2)):
        assert call(ev, options=_cse.cg_options(**{field: value})) == _cse.CSE_ERR_INVALID, field
        assert field.split("_")[0] in _cse.last_error()
    # d_x overlapping d_rhs
    both = torch.zeros(135, dtype=torch.float64, device=dev)
    for a, b in ((both, both), (both, both[45:]), (both[45:], both), (both[89:], both)):
        assert call(ev, d_rhs=a.data_ptr(), d_x=b.data_ptr()) == _cse.CSE_ERR_INVALID
        assert "overlaps" in _cse.last_error()
    # the explicit operator before the sparse structure is uploaded
    values = torch.zeros(81 * 55, dtype=torch.float64, device=dev)
    assert call(ev, values=values.data_ptr()) == _cse.CSE_ERR_INVALID
    assert "structure" in _cse.last_error()
    ev.schur_complement_sparse_upload()
    ev.schur_complement_sparse_device(values.data_ptr())
    ev.schur_init_device(dj.data_ptr(), None, db.data_ptr(), rhs, _cse.SCHUR_IDENTITY)
    lm = _cse.cg_options(q_tolerance=0.1, max_num_iterations=50)
    assert call(ev, options=lm, values=values.data_ptr()) == _cse.CSE_OK
    assert call(ev, options=lm) == _cse.CSE_OK
    assert summary.num_iterations >= 1 and summary.num_synchronizations >= 2
    ev.close()
    # not Schur-eligible
    ev = ca.Evaluator(bal.synthetic_program((10, 300, 1500), format=ca.COMPRESSED_ROW, seed=9))
    assert call(ev) == _cse.CSE_ERR_UNSUPPORTED
    ev.close()


def run_driver(extra):
    from ceres_amd import bundle_adjuster
    bal.CONFIGS.setdefault("problem-49-7776", (49, 7776, 31843))  # tools/schur_complement_probe.py's shape
    return bundle_adjuster.main(["--synthetic", "problem-49-7776", "--num_iterations", "4"] + extra)


@functools.lru_cache(maxsize=None)
def host_loop_run(explicit):
    return run_driver(["--use_explicit_schur_complement"] if explicit else [])


@pytest.mark.parametrize("explicit", [False, True], ids=["implicit", "explicit"])
@pytest.mark.parametrize("period", [1, 4])
def test_bundle_adjuster_device_pcg(gpu, capsys, explicit, period):
    """--device_pcg with the residual test is the host loop's solve: the same
    ls_iter list, the final cost within 1e-9 relative."""
    flag = ["--use_explicit_schur_complement"] if explicit else []
    _, c_host, rows_host = host_loop_run(explicit)
    _, c_dev, rows_dev = run_driver(flag + ["--device_pcg", "--pcg_check_period", str(period)])
    out = capsys.readouterr().out
    print(out)
    print([r[6] for r in rows_host], [r[6] for r in rows_dev], c_host, c_dev)
    assert [r[6] for r in rows_dev] == [r[6] for r in rows_host]
    assert all(r[6] > 0 for r in rows_dev)
    assert abs(c_dev - c_host) <= 1e-9 * abs(c_host)


def test_bundle_adjuster_quadratic_termination(gpu, capsys):
    c0, c1, rows = run_driver(["--device_pcg", "--pcg_termination", "quadratic"])
    print(capsys.readouterr().out)
    assert c1 < c0 and all(r[6] > 0 for r in rows)
    assert any(r[7] for r in rows)  # a step was accepted
