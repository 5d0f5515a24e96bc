"""GPU: cse_schur_power_series -- the reference's power series expansion of
S^-1 (power_series_expansion_preconditioner.cc:51-72) on the device -- as a
call, as cse_schur_init's fourth preconditioner, inside cse_schur_solve and as
the PCG's start, against tests/spse_reference.py and tests/cg_reference.py.

The dense S, P^-1 and Q of a case come from the Jacobian the evaluator returned;
the series' input is the right-hand side cse_schur_init wrote.  The series is
held to test_schur_gpu's bound for one S product, close(y, y_longdouble, 1e-12):
the series contracts (the spectral radius of P^-1 Q is 0.58-0.68 on these
problems, tests/test_schur_spse.py), so chained terms do not grow a term's
error.  The PCG under the series is held as tests/test_schur_solve_gpu.py holds
it: termination type, reason and iteration count equal, x within
max(10 d_ref, 1e-14) of the np.longdouble x.  tests/test_schur_spse.py checks
on the CPU that every case is a fair input.

The series' vector kernels are one workgroup for every vector length (csrc/
spse_kernels.hpp, as the PCG's), so there is no length at which their launch
shape changes and no pair of problems around one; the lengths here run from 18
entries (under one wave) to 1,350 (past the workgroup's 1,024 lanes).

Worst figures measured: see DESIGN 3.6e.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse, bal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cg_reference as R  # noqa: E402
import schur_complement_util as U  # noqa: E402
import schur_solve_util as SU  # noqa: E402
import spse_reference as P  # noqa: E402
import test_schur_solve_gpu as G  # noqa: E402
import test_schur_spse as CPU  # noqa: E402
from test_constant_gpu import held  # noqa: E402
from test_schur_gpu import block_inverse, close, dense_schur  # noqa: E402
from test_schur_held_gpu import boundary_problem, evaluated  # noqa: E402
from test_spmv_gpu import dense_jacobian  # noqa: E402

LD = np.longdouble
NAN = float("nan")
SERIES = [(1, 0.0), (2, 0.0), (5, 0.0), (5, 0.1), (50, 1e-3), (500, 1e-14)]
SERIES_BOUND = 1e-12  # test_schur_gpu.RTOL, one S product's
SPSE = _cse.SCHUR_POWER_SERIES_EXPANSION
worst = {"series": (0.0, None), "pcg": (0.0, None)}

to_device, filled, outcome = G.to_device, G.filled, G.outcome


def note(kind, value, case):
    if value > worst[kind][0]:
        worst[kind] = (value, case)
    return worst[kind]


def rel_ld(got, want):
    return float(np.linalg.norm((got.astype(LD) - want).astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def operators(which):
    """(Pinv, Q) in np.longdouble from the device problem's dense S."""
    c = G.device_problem(which)
    return P.operators(c.S, c.J, c.e_cols, c.D, LD)


def run_series(ev, d_x, n, mx, tol, want_summary=True):
    y = filled(n, NAN)  # assignment: nothing of the pre-fill may survive
    s = ev.schur_power_series_device(d_x.data_ptr(), y.data_ptr(), mx, tol, want_summary=want_summary)
    return s, y


def check_series(ev, d_x, x_host, Pinv, Q, cases, label):
    for mx, tol in cases:
        ref = P.series(Pinv, Q, x_host, mx, tol, LD)
        if tol:  # a fair input: the count does not hang on rounding
            threshold = LD(tol) * ref.norms[0]
            assert min(abs(float((v - threshold) / threshold)) for v in ref.norms[1:]) > 1e-6
        s, y = run_series(ev, d_x, len(x_host), mx, tol)
        got = y.cpu().numpy()
        err = rel_ld(got, ref.y)
        w = note("series", err / SERIES_BOUND, (label, mx, tol))
        print(f"{label} ({mx}, {tol:g}): {s.num_terms} terms (reference {ref.num_terms}), error {err:.3e} = "
              f"{err / SERIES_BOUND:.4f} of the bound; worst so far {w[0]:.4f} at {w[1]}")
        assert s.num_terms == ref.num_terms and s.reserved == 0
        assert np.isfinite(got).all()
        assert close(got, ref.y.astype(np.float64), SERIES_BOUND) and err <= SERIES_BOUND
        assert s.norm_first == pytest.approx(float(ref.norms[0]), rel=1e-12)
        assert s.norm_last == pytest.approx(float(ref.norms[-1]), rel=1e-12)
        # the same bits when the host does not look, and run to run
        _, y2 = run_series(ev, d_x, len(x_host), mx, tol, want_summary=False)
        assert torch.equal(y, y2)


# --------------------------------------------------------------------------
# 1, 2. The series against the reference, on every shape.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("which", SU.PROBLEMS)
def test_series_parity(gpu, which):
    """All six problems: "runs" has runs of 63, 64, 65, 66, 70 and 130 rows (the
    wave boundary, SchurBigKernel's 64-row stride), "unobserved" a camera
    without blocks (a zero term row, P = D^2), "duplicates" a point that sees a
    camera twice, "wide" 1,350 columns (past the 1,024-lane workgroup)."""
    c = G.bind(which, _cse.SCHUR_JACOBI)
    Pinv, Q = operators(which)
    check_series(c.ev, c.rhs, c.rhs_host, Pinv, Q, SERIES, which)
    assert c.ev.wait() == _cse.CSE_OK


def test_two_cameras(gpu):
    """test_schur_solve_gpu.two_cameras' program: 18 columns, under one wave and
    under one finish workgroup; bound with IDENTITY, so the blocks are built on
    demand.  With SU.damping's D, as every problem here: under two_cameras' own
    D = 1 the unscaled cameras' blocks of F^T F + D^2 have condition numbers
    near 1e10 and the spectral radius of P^-1 Q is 0.98, so the series does not
    contract to speak of and the bound's premise is gone (measured there: one
    term 1.7e-13, five 4.3e-13, fifty 2.2e-12 from the np.longdouble series)."""
    dev = torch.device("cuda", 0)
    prog = U._program(2, [[0, 1], [1], [0], [1, 0]] * 5, 12)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, _, _, jv = ev.evaluate()
    assert ok
    e_cols, f_cols = ev.schur_structure()
    assert f_cols == G.N2
    J = dense_jacobian(prog, jv)
    D, b = SU.damping(J, e_cols), SU.right_hand_side(prog)
    _, _, _, S, rhs_dense = dense_schur(J, e_cols, D, b)
    dj, dD, db, drhs = to_device(jv), to_device(D), to_device(b), filled(f_cols, NAN)
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), drhs.data_ptr(), _cse.SCHUR_IDENTITY)
    rhs = drhs.cpu().numpy()
    assert close(rhs, rhs_dense)
    Pinv, Q = P.operators(S, J, e_cols, D, LD)
    check_series(ev, drhs, rhs, Pinv, Q, SERIES, "two cameras")
    assert ev.wait() == _cse.CSE_OK
    ev.close()


# --------------------------------------------------------------------------
# 3. Held cameras.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["held", "boundary"])
@pytest.mark.parametrize("precond", [_cse.SCHUR_JACOBI, _cse.SCHUR_IDENTITY], ids=["jacobi", "on-demand"])
def test_series_with_held_cameras(gpu, which, precond):
    """The kHeld chunk and big kernels in series mode: a block whose camera is
    held has F_b = 0 and enters only the point sum.  Against the series built
    from the dense S and P of the active columns."""
    prog = held(counts=(16, 700, 2900), const=(0, 3, 9, 15)) if which == "held" else boundary_problem()[0]
    ev, r, g, jv, J, e_cols, f_cols = evaluated(prog)
    D = SU.damping(J, e_cols)
    b = SU.right_hand_side(prog)
    _, _, _, S, rhs_dense = dense_schur(J, e_cols, D, b)
    dj, dD, db, drhs = to_device(jv), to_device(D), to_device(b), filled(f_cols, NAN)
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), drhs.data_ptr(), precond)
    rhs = drhs.cpu().numpy()
    assert close(rhs, rhs_dense)
    Pinv, Q = P.operators(S, J, e_cols, D, LD)
    check_series(ev, drhs, rhs, Pinv, Q, [(5, 0.0), (50, 1e-3)], f"{which} cameras held")
    assert ev.wait() == _cse.CSE_OK
    ev.close()


# --------------------------------------------------------------------------
# 4. Blocks on demand.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["bal", "runs"])
def test_blocks_on_demand(gpu, which):
    """After an IDENTITY or a SCHUR_JACOBI init the first series builds the
    (F^T F + D_f^2)^-1 blocks by the pass a JACOBI init runs, on the same
    inputs: y is the JACOBI init's BIT FOR BIT (also when the init wrote the
    gradient, whose u_b records have another stride).  cse_schur_precondition
    keeps applying the init's own preconditioner."""
    rng = np.random.default_rng(5)
    c = G.bind(which, _cse.SCHUR_JACOBI)
    _, want = run_series(c.ev, c.rhs, c.f_cols, 5, 0.0)
    x, y0 = rng.normal(size=c.f_cols), rng.normal(size=c.f_cols)
    dx = to_device(x)
    for precond in (_cse.SCHUR_IDENTITY, _cse.SCHUR_SCHUR_JACOBI):
        c = G.bind(which, precond)
        _, got = run_series(c.ev, c.rhs, c.f_cols, 5, 0.0)
        assert torch.equal(got, want), precond
        _, again = run_series(c.ev, c.rhs, c.f_cols, 5, 0.0)  # the blocks are kept
        assert torch.equal(again, want), precond
        dy = to_device(y0)
        c.ev.schur_precondition_device(dx.data_ptr(), dy.data_ptr())
        assert c.ev.wait() == _cse.CSE_OK
        if precond == _cse.SCHUR_IDENTITY:
            assert np.array_equal(dy.cpu().numpy(), y0 + x)
        else:
            assert close(dy.cpu().numpy(), y0 + block_inverse(c.S, 9) @ x, 1e-11)
    # ... and after an init that also wrote the gradient
    c = G.device_problem(which)
    grad = filled(c.prog.num_effective_parameters, NAN)
    c.ev.schur_init_gradient_device(c.dj.data_ptr(), c.dD.data_ptr(), c.db.data_ptr(), c.rhs.data_ptr(),
                                    grad.data_ptr(), _cse.SCHUR_IDENTITY)
    c.bound = None
    _, got = run_series(c.ev, c.rhs, c.f_cols, 5, 0.0)
    assert torch.equal(got, want)
    assert c.ev.wait() == _cse.CSE_OK


# --------------------------------------------------------------------------
# 5. The preconditioner.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["bal", "unobserved", SU.WIDE])
def test_preconditioner_accumulates_the_series(gpu, which):
    """Under a POWER_SERIES init cse_schur_precondition gives y0 + M_5 x to the
    existing preconditioner bound, close(., 1e-11); after
    cse_schur_set_spse_iterations(1), y0 + M_1 x; two calls give equal bits."""
    c = G.bind(which, SPSE)
    Pinv, Q = operators(which)
    rng = np.random.default_rng(6)
    x, y0 = rng.normal(size=c.f_cols), rng.normal(size=c.f_cols)
    dx = to_device(x)
    try:
        for m in (5, 1):
            if m != 5:
                c.ev.schur_set_spse_iterations(m)
            want = (y0.astype(LD) + P.series(Pinv, Q, x, m, 0.0, LD).y).astype(np.float64)
            dy, dy2 = to_device(y0), to_device(y0)
            c.ev.schur_precondition_device(dx.data_ptr(), dy.data_ptr())
            c.ev.schur_precondition_device(dx.data_ptr(), dy2.data_ptr())
            assert c.ev.wait() == _cse.CSE_OK
            got = dy.cpu().numpy()
            print(f"{which} m {m}: |y - (y0 + M x)| / |.| {np.linalg.norm(got - want) / np.linalg.norm(want):.3e}")
            assert close(got, want, 1e-11)
            assert torch.equal(dy, dy2)
    finally:
        c.ev.schur_set_spse_iterations(5)


# --------------------------------------------------------------------------
# 6. cse_schur_solve under the series.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5])
@pytest.mark.parametrize("which", ["bal", "runs", "unobserved", SU.WIDE])
def test_pcg_parity_under_the_series(gpu, which, m):
    c = G.bind(which, SPSE)
    Pinv, Q = operators(which)
    Minv = P.dense_preconditioner(Pinv, Q, m, np.float64)
    c.ev.schur_set_spse_iterations(m)
    try:
        for option_set in CPU.PCG_SETS[m]:
            ref = SU.reference(c.S, Minv, c.rhs_host, option_set)
            assert SU.same_outcome(ref.f64, ref.ld)
            summary, x = G.solve(c, option_set, False)
            err = rel_ld(x, ref.ld.x)
            ratio = err / ref.d_ref if ref.d_ref > 0 else 0.0
            w = note("pcg", ratio, (which, m, option_set))
            print(f"{which} m {m} {option_set}: {outcome(summary)} reference {ref.ld[1:4]} error {err:.3e} "
                  f"d_ref {ref.d_ref:.3e} ratio {ratio:.2f}; worst so far {w[0]:.2f} at {w[1]}")
            assert outcome(summary) == (ref.ld.termination_type, ref.ld.reason, ref.ld.num_iterations)
            assert np.isfinite(x).all()
            assert err <= max(10 * ref.d_ref, 1e-14)
            # check_period 4 and a repeat: equal bits
            for period in (4, 1):
                s2, x2 = G.solve(c, option_set, False, check_period=period)
                assert np.array_equal(x2, x) and outcome(s2) == outcome(summary), period
                assert (s2.norm_r, s2.rho, s2.pq) == (summary.norm_r, summary.rho, summary.pq)
        # d_step is written: the back substitution of x
        o = SU.OPTION_SETS["zero"]
        dx, step = filled(c.f_cols, NAN), filled(c.prog.num_effective_parameters, NAN)
        s = c.ev.schur_solve_device(c.rhs.data_ptr(), dx.data_ptr(),
                                    G.options_of(o.options, flags=_cse.CG_ZERO_INITIAL_GUESS), None,
                                    step.data_ptr())
        assert s.termination_type == _cse.CG_SUCCESS
        got = step.cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got[c.e_cols:], dx.cpu().numpy())
        assert c.ev.wait() == _cse.CSE_OK
    finally:
        c.ev.schur_set_spse_iterations(5)


# --------------------------------------------------------------------------
# 7. The SPSE start.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["bal", "runs", "unobserved", SU.WIDE])
def test_jacobi_from_the_series_start(gpu, which):
    """use_spse_initialization: x0 = series(5, 0.1, rhs), then cse_schur_solve
    with JACOBI and no zero-guess flag, against cg_reference from the
    np.longdouble x0."""
    c = G.bind(which, _cse.SCHUR_JACOBI)
    Pinv, Q = operators(which)
    mx, tol = CPU.SPSE_START
    x0 = P.series(Pinv, Q, c.rhs_host, mx, tol, LD).y
    Minv = SU.dense_preconditioner(_cse.SCHUR_JACOBI, c.S, c.J, c.e_cols, c.D)
    o = SU.OPTION_SETS["guess"].options
    f64 = R.solve(c.S, c.rhs_host, x0, o, Minv, np.float64)
    ld = R.solve(c.S, c.rhs_host, x0, o, Minv, LD)
    assert SU.same_outcome(f64, ld)
    d_ref = rel_ld(f64.x.astype(np.float64), ld.x)
    dx = filled(c.f_cols, NAN)
    c.ev.schur_power_series_device(c.rhs.data_ptr(), dx.data_ptr(), mx, tol)
    s = c.ev.schur_solve_device(c.rhs.data_ptr(), dx.data_ptr(), G.options_of(o, flags=0))
    x = dx.cpu().numpy()
    err = rel_ld(x, ld.x)
    ratio = err / d_ref if d_ref > 0 else 0.0
    w = note("pcg", ratio, (which, "spse start"))
    print(f"{which}: {outcome(s)} reference {ld[1:4]} error {err:.3e} d_ref {d_ref:.3e} ratio {ratio:.2f}; "
          f"worst so far {w[0]:.2f} at {w[1]}")
    assert outcome(s) == (ld.termination_type, ld.reason, ld.num_iterations)
    assert err <= max(10 * d_ref, 1e-14)
    # fewer iterations than from zero (9-10 under JACOBI)
    assert s.num_iterations < SU.reference(c.S, Minv, c.rhs_host, "zero").ld.num_iterations


# --------------------------------------------------------------------------
# 8. Refusals.
# --------------------------------------------------------------------------
def test_refusals(gpu):
    dev = torch.device("cuda", 0)
    L = _cse.lib()
    prog = bal.synthetic_program((10, 300, 1500), seed=9)
    buf = torch.zeros(4, 90, dtype=torch.float64, device=dev)
    x, y = buf[0].data_ptr(), buf[1].data_ptr()

    def call(ev, mx=5, tol=0.0, d_x=x, d_y=y):
        rc = L.cse_schur_power_series(ev.handle, mx, tol, d_x, d_y, None)
        if rc < 0:
            assert _cse.last_error(), "a refusal without a message"
        return rc

    # a multi-device handle
    ev = ca.Evaluator(prog, devices=[0, 0])
    assert call(ev) == _cse.CSE_ERR_UNSUPPORTED and "cse_create_multi" in _cse.last_error()
    assert L.cse_schur_set_spse_iterations(ev.handle, 3) == _cse.CSE_ERR_UNSUPPORTED
    ev.close()
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, r, _, jv = ev.evaluate()
    assert ev.schur_structure()[1] == 90
    # before cse_schur_init
    assert call(ev) == _cse.CSE_ERR_INVALID and "cse_schur_init has not run" in _cse.last_error()
    dj, db = to_device(jv), to_device(-r)
    dD = filled(prog.num_effective_parameters, 1.0)
    rhs = buf[2]
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), _cse.SCHUR_IDENTITY)
    for kw in (dict(d_x=None), dict(d_y=None)):
        assert call(ev, **kw) == _cse.CSE_ERR_INVALID and "null" in _cse.last_error(), kw
    for mx in (0, -1):
        assert call(ev, mx=mx) == _cse.CSE_ERR_INVALID and "max_num_iterations" in _cse.last_error()
    for tol in (-1e-300, -1.0, float("inf"), float("-inf"), NAN):
        assert call(ev, tol=tol) == _cse.CSE_ERR_INVALID and "tolerance" in _cse.last_error(), tol
    both = torch.zeros(135, dtype=torch.float64, device=dev)
    for a, b in ((both, both), (both, both[45:]), (both[45:], both), (both[89:], both)):
        assert call(ev, d_x=a.data_ptr(), d_y=b.data_ptr()) == _cse.CSE_ERR_INVALID
        assert "overlaps" in _cse.last_error()
    assert L.cse_schur_set_spse_iterations(ev.handle, 0) == _cse.CSE_ERR_INVALID
    assert "max_num_iterations" in _cse.last_error()
    # an unknown preconditioner is still refused
    assert L.cse_schur_init(ev.handle, dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), 4) \
        == _cse.CSE_ERR_INVALID
    # the explicit complement with a POWER_SERIES init
    ev.schur_complement_sparse_upload()
    values = torch.zeros(81 * ev.schur_complement_sparse_counts()[1], dtype=torch.float64, device=dev)
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), SPSE)
    ev.schur_complement_sparse_device(values.data_ptr())
    summary = _cse.cse_cg_summary()
    lm = _cse.cg_options(q_tolerance=0.1, max_num_iterations=50)
    assert L.cse_schur_solve(ev.handle, C.byref(lm), values.data_ptr(), rhs.data_ptr(), x, None,
                             C.byref(summary)) == _cse.CSE_ERR_UNSUPPORTED
    assert "POWER_SERIES" in _cse.last_error()
    # the preconditioner's x and y may not overlap
    assert L.cse_schur_precondition(ev.handle, x, x) == _cse.CSE_ERR_INVALID and "overlap" in _cse.last_error()
    # legal calls afterwards still work
    assert L.cse_schur_solve(ev.handle, C.byref(lm), None, rhs.data_ptr(), x, None, C.byref(summary)) == _cse.CSE_OK
    assert summary.termination_type == _cse.CG_SUCCESS and summary.num_iterations >= 1
    assert call(ev, d_x=rhs.data_ptr()) == _cse.CSE_OK
    assert call(ev, d_x=rhs.data_ptr(), tol=-0.0) == _cse.CSE_OK
    assert ev.wait() == _cse.CSE_OK
    assert torch.isfinite(buf[1]).all() and float(buf[1].norm()) > 0
    ev.close()
    # not Schur-eligible
    ev = ca.Evaluator(bal.synthetic_program((10, 300, 1500), format=ca.COMPRESSED_ROW, seed=9))
    assert call(ev) == _cse.CSE_ERR_UNSUPPORTED
    ev.close()


# --------------------------------------------------------------------------
# 9. Release.
# --------------------------------------------------------------------------
def test_create_series_solve_destroy_does_not_leak(gpu):
    """The series' scratch -- two vectors, the state, the on-demand blocks with
    their pass's scratch -- is released by cse_destroy
    (test_hygiene_gpu.test_create_evaluate_destroy_does_not_leak's method)."""
    prog = bal.synthetic_program((30, 4000, 16000), loss=ca.Loss.huber(1.0), seed=4)
    dev = torch.device("cuda", 0)
    n, m = prog.num_effective_parameters, prog.num_residuals
    jac = torch.empty(prog.num_jacobian_values, dtype=torch.float64, device=dev)
    st = torch.from_numpy(prog.state).to(dev)
    cost = torch.zeros(1, dtype=torch.float64, device=dev)
    res = torch.empty(m, dtype=torch.float64, device=dev)
    D = torch.ones(n, dtype=torch.float64, device=dev)
    rhs, x, y = (torch.empty(270, dtype=torch.float64, device=dev) for _ in range(3))
    o = _cse.cg_options(max_num_iterations=20, r_tolerance=1e-6, flags=_cse.CG_ZERO_INITIAL_GUESS)

    def cycle(precond):
        ev = ca.Evaluator(prog, device=0)
        ev.evaluate_device(st.data_ptr(), cost.data_ptr(), res.data_ptr(), None, jac.data_ptr())
        ev.schur_init_device(jac.data_ptr(), D.data_ptr(), res.data_ptr(), rhs.data_ptr(), precond)
        ev.schur_power_series_device(rhs.data_ptr(), y.data_ptr(), 5, 0.1)
        ev.schur_solve_device(rhs.data_ptr(), x.data_ptr(), o)
        assert ev.wait() == 0
        ev.close()

    cycle(SPSE)
    cycle(_cse.SCHUR_IDENTITY)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(dev)
    for k in range(10):
        cycle(SPSE if k % 2 else _cse.SCHUR_IDENTITY)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(dev)
    assert free0 - free1 < 2 << 20, (free0, free1)


# --------------------------------------------------------------------------
# 10. The driver.
# --------------------------------------------------------------------------
DRIVER = ["--synthetic", "problem-16-22106", "--robustify", "--point_sigma", "0.05", "--num_iterations", "3"]


@functools.lru_cache(maxsize=None)
def driver_run(*extra):
    from ceres_amd import bundle_adjuster
    return bundle_adjuster.main(DRIVER + list(extra))


@pytest.mark.parametrize("extra,base", [
    (("--preconditioner", "schur_power_series_expansion"), ()),
    (("--preconditioner", "schur_power_series_expansion", "--device_pcg"), ()),
    (("--use_spse_initialization",), ()),
    (("--use_spse_initialization", "--device_pcg"), ()),
    (("--preconditioner", "schur_power_series_expansion", "--held_cameras", "2"), ("--held_cameras", "2")),
], ids=["host-loop", "device-pcg", "spse-start", "spse-start-device-pcg", "held"])
def test_bundle_adjuster(gpu, capsys, extra, base):
    """Each run reaches the jacobi run's final cost to 1e-6 relative: the same
    linear systems solved to the same eta."""
    _, want, rows_jacobi = driver_run(*base)
    c0, c1, rows = driver_run(*extra)
    print(capsys.readouterr().out)
    print(f"{extra}: final cost {c1:.12e}, jacobi's {want:.12e}, relative gap {abs(c1 - want) / want:.3e}; "
          f"ls_iter {[r[6] for r in rows]} against {[r[6] for r in rows_jacobi]}")
    assert c1 < c0 and all(r[6] > 0 for r in rows)
    assert abs(c1 - want) <= 1e-6 * want
