"""GPU: CLUSTER_TRIDIAGONAL on the device -- cse_schur_set_cluster_forest and
cse_schur_cluster_tridiagonal: the cluster blocks of S and the blocks of the
forest's edges, the block tridiagonal factor along every path, the retry with
halved edges, and the factor applied by cse_schur_precondition and inside
cse_schur_solve.

1. Every 9 x 9 cell of d_matrices -- cluster matrices and edge rectangles -- is
   np.array_equal to the same cell of cse_schur_complement's dense S.
2. The apply against numpy on the assembled M, per path: for M z = r,
   eta = |M z - r|_inf / (|M|_inf |z|_inf + |r|_inf) <= n gamma_{3n+1}, n the
   path's dimension (Higham, Thm 10.4; tests/test_schur_tridiagonal.py holds the
   host replay and numpy itself to it).
3. Two clusters that cover every camera, joined: M = S.
4. cse_schur_solve against tests/cg_reference.py given the dense M^-1, as
   tests/test_schur_cluster_gpu.py holds CLUSTER_JACOBI.
5. The retry: an input whose unscaled M numpy cannot factor and whose halved M
   it can.  6. A pivot that fails in both passes.  7. Refusals.  8. Release.
9. bundle_adjuster.

The evaluators here are this module's own.  Worst figures measured: see DESIGN
3.6g.
"""
import functools
import types

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse, bal, clustering

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import schur_complement_util as U  # noqa: E402
import schur_solve_util as SU  # noqa: E402
from test_constant_gpu import held  # noqa: E402
from test_schur_cluster import eta, solve_bound  # noqa: E402
from test_schur_cluster_gpu import (check_cells, cluster_jacobi, columns, dense_S, init,  # noqa: E402
                                    precondition, solve)
from test_schur_solve_gpu import filled, outcome, to_device  # noqa: E402
from test_spmv_gpu import dense_jacobian  # noqa: E402

LD = np.longdouble
NAN = float("nan")
worst = {"eta": (0.0, None), "pcg": (0.0, None)}


def note(kind, value, case):
    if value > worst[kind][0]:
        worst[kind] = (value, case)
    return worst[kind]


def make_program(which):
    if which == "sixteen":  # 16 cameras, about 18 pairs on an off-diagonal block and 80 on a diagonal one
        return bal.synthetic_program((16, 300, 1300), loss=ca.Loss.huber(1.0), seed=21)
    if which == "forty":  # local visibility: a point's four cameras from a window of five
        return bal.synthetic_program("banded-40-400-w5", loss=ca.Loss.huber(1.0), seed=22)
    return SU.make_program(which)  # "bal": 10 cameras, lists of 60 to 150 pairs; "unobserved"; "duplicates"


def bind(prog, jv):
    """An evaluator of this module's own with jv, D and b on the device."""
    dev = torch.device("cuda", 0)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    e_cols, f_cols = ev.schur_structure()
    c = types.SimpleNamespace(prog=prog, ev=ev, jv=jv, e_cols=e_cols, f_cols=f_cols, num_cameras=f_cols // 9)
    c.J = dense_jacobian(prog, jv)
    c.rhs = filled(f_cols, NAN)
    c.values = None
    return c


@functools.lru_cache(maxsize=None)
def device_problem(which):
    prog = make_program(which)
    dev = torch.device("cuda", 0)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, _, _, jv = ev.evaluate()
    assert ok
    ev.close()
    c = bind(prog, jv)
    c.which = which
    c.D = SU.damping(c.J, c.e_cols)
    c.dj, c.dD, c.db = to_device(jv), to_device(c.D), to_device(SU.right_hand_side(prog))
    return c


def sized(*sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)


def forest_case(name, num):
    """name -> (labels, edges as given to the device)."""
    chain = [(g, g + 1) for g in range(num - 1)]
    cases = {
        "chain": (np.arange(num), chain),                         # singletons in one path
        "chain, no edges": (np.arange(num), []),
        "halves": (np.arange(num) // ((num + 1) // 2), [(0, 1)]),
        "8+8": (sized(8, 8), [(0, 1)]),
        "1+15": (sized(1, 15), [(0, 1)]),
        "15+1": (sized(15, 1), [(0, 1)]),
        "5+3+8": (sized(5, 3, 8), [(0, 1), (1, 2)]),
        "2-0-1": (sized(5, 3, 8), [(0, 2), (1, 0)]),              # label order is not path order; an edge as (h, g)
        "evenodd": (np.arange(num) % 2, [(1, 0)]),                # both transposition cases in one rectangle
        "several": (np.arange(num) // 2, [(6, 2), (2, 4), (0, 7), (5, 6)]),  # paths 0-7, 1, 3, 4-2-6-5
        "pairs chain": (np.arange(num) // 2, [(g + 1, g) for g in range((num + 1) // 2 - 1)]),
        # "unobserved" (8 cameras): camera 3 has no observation
        "unobserved inside": (np.array([0, 1, 1, 0, 1, 2, 3, 3]), [(0, 1), (1, 2)]),
        "edge without a point": (np.array([0, 0, 1, 2, 1, 1, 3, 3]), [(2, 3), (0, 1)]),  # {3} - {6, 7}: all zero
    }
    labels, edges = cases[name]
    return labels.astype(np.int32), np.array(edges, np.int32).reshape(-1, 2)


def tridiagonal(c, labels, edges, want_matrices=True):
    """Installs partition and forest and builds.  Returns ([(cameras, M_g)],
    [((g, h), S[g, h])], raw buffer, scaled)."""
    labels = np.asarray(labels, np.int32)
    c.ev.schur_set_clusters(labels)
    c.ev.schur_set_cluster_forest(edges)
    groups = [np.nonzero(labels == g)[0] for g in range(int(labels.max()) + 1)]
    scaled = torch.full((1,), -7, dtype=torch.int32, device=c.rhs.device)
    if not want_matrices:
        c.ev.schur_cluster_tridiagonal_device(None, scaled.data_ptr())
        return groups, None, None, scaled
    total = sum((9 * len(g)) ** 2 for g in groups) + sum(81 * len(groups[g]) * len(groups[h]) for g, h in edges)
    buf = filled(total, NAN)
    c.ev.schur_cluster_tridiagonal_device(buf.data_ptr(), scaled.data_ptr())
    host = buf.cpu().numpy()
    clusters, rects, at = [], [], 0
    for g in groups:
        n = 9 * len(g)
        clusters.append((g, host[at:at + n * n].reshape(n, n)))
        at += n * n
    for g, h in edges:
        rows, cols = 9 * len(groups[g]), 9 * len(groups[h])
        rects.append(((int(g), int(h)), host[at:at + rows * cols].reshape(rows, cols)))
        at += rows * cols
    assert at == total
    return clusters, rects, buf, scaled


def check_rectangles(rects, labels, S):
    for (g, h), R in rects:
        cg, ch = np.nonzero(labels == g)[0], np.nonzero(labels == h)[0]
        assert not np.isnan(R).any()
        assert np.array_equal(R, S[np.ix_(columns(cg), columns(ch))]), (g, h)


def assemble(S, labels, edges, scale=1.0):
    """The numpy model of M: S's blocks inside a cluster, scale times S's
    blocks between the two clusters of an edge, zero elsewhere."""
    lab = np.repeat(np.asarray(labels), 9)
    weight = (lab[:, None] == lab[None, :]).astype(np.float64)
    for g, h in np.asarray(edges).reshape(-1, 2):
        weight[np.ix_(lab == g, lab == h)] = scale
        weight[np.ix_(lab == h, lab == g)] = scale
    return S * weight


def path_columns(labels, edges):
    paths = clustering.forest_paths(int(np.max(labels)) + 1, edges)
    return [columns(np.concatenate([np.nonzero(labels == g)[0] for g in path])) for path in paths]


# --------------------------------------------------------------------------
# 1. The cells.
# --------------------------------------------------------------------------
CELL_CASES = [("sixteen", n) for n in ("chain", "8+8", "1+15", "15+1", "5+3+8", "2-0-1", "evenodd", "several")] + \
             [("bal", "chain"), ("bal", "halves"), ("bal", "evenodd"),
              ("unobserved", "unobserved inside"), ("unobserved", "edge without a point"),
              ("duplicates", "pairs chain")]


@pytest.mark.parametrize("which,name", CELL_CASES)
def test_matrices_are_the_dense_cells(gpu, which, name):
    """Cluster matrices and edge rectangles, NaN pre-filled, have the bits of
    the dense S's cells; a second call repeats them; cse_schur_cluster_jacobi
    on the same evaluator gives the bits it gave before the forest was set."""
    c = device_problem(which)
    init(c)
    S = dense_S(c)
    labels, edges = forest_case(name, c.num_cameras)
    _, jacobi_before = cluster_jacobi(c, labels)
    clusters, rects, buf, scaled = tridiagonal(c, labels, edges)
    assert c.ev.wait() == _cse.CSE_OK
    check_cells(clusters, S)
    check_rectangles(rects, labels, S)
    assert int(scaled.item()) in (0, 1)
    if name == "edge without a point":
        assert not rects[0][1].any()  # exactly zero
        assert np.array_equal(clusters[2][1], np.diag(c.D[c.e_cols + 27:c.e_cols + 36] ** 2))
    _, _, again, _ = tridiagonal(c, labels, edges)
    assert torch.equal(buf, again)
    _, jacobi_after = cluster_jacobi(c, labels)
    assert torch.equal(jacobi_before, jacobi_after)
    assert torch.equal(buf[:jacobi_after.numel()], jacobi_after)  # the cluster part is CLUSTER_JACOBI's layout
    assert c.ev.wait() == _cse.CSE_OK


def test_changed_forest_changed_partition_and_second_init(gpu):
    c = device_problem("sixteen")
    init(c)
    S = dense_S(c)
    for name in ("5+3+8", "2-0-1", "chain", "chain, no edges", "8+8", "5+3+8"):
        labels, edges = forest_case(name, 16)
        clusters, rects, _, _ = tridiagonal(c, labels, edges)
        check_cells(clusters, S)
        check_rectangles(rects, labels, S)
    twice = to_device(2.0 * c.D)  # bound by the init: alive until the next one
    init(c, _cse.SCHUR_JACOBI, twice)
    S2 = dense_S(c)
    assert not np.array_equal(S, S2)
    clusters, rects, _, _ = tridiagonal(c, labels, edges)
    check_cells(clusters, S2)
    check_rectangles(rects, labels, S2)
    assert c.ev.wait() == _cse.CSE_OK


# --------------------------------------------------------------------------
# 2. The apply.
# --------------------------------------------------------------------------
APPLY_CASES = [("sixteen", n) for n in ("chain", "8+8", "1+15", "15+1", "2-0-1", "evenodd", "several")] + \
              [("forty", "chain"), ("bal", "halves"), ("unobserved", "edge without a point"),
               ("duplicates", "pairs chain")]


@pytest.mark.parametrize("which,name", APPLY_CASES)
def test_apply_solves_every_path(gpu, which, name):
    """("forty", "chain"): one path of 40 singleton clusters, for depth."""
    c = device_problem(which)
    init(c)
    S = dense_S(c)
    labels, edges = forest_case(name, c.num_cameras)
    _, _, _, scaled = tridiagonal(c, labels, edges)
    M = assemble(S, labels, edges, 0.5 if int(scaled.item()) else 1.0)
    rng = np.random.default_rng(7)
    x = rng.normal(size=c.f_cols)
    z = precondition(c, x, np.zeros(c.f_cols)).cpu().numpy()
    assert c.ev.wait() == _cse.CSE_OK
    assert np.isfinite(z).all()
    paths = path_columns(labels, edges)
    assert sorted(np.concatenate(paths).tolist()) == list(range(c.f_cols))
    for cols in paths:
        Mp = M[np.ix_(cols, cols)]
        rest = np.delete(M[cols], cols, axis=1)
        assert not rest.any()  # M is block diagonal over the paths
        e, bound = eta(Mp, z[cols], x[cols]), solve_bound(len(cols))
        w = note("eta", e / bound, (which, name, len(cols)))
        print(f"{which} {name} n {len(cols):3d}: eta {e:.3e}, bound {bound:.3e}, scaled {int(scaled.item())}; "
              f"worst eta / bound so far {w[0]:.3e} at {w[1]}")
        assert e <= bound
    # accumulation into a non-zero y: the same z added, bit for bit; twice the same bits
    y0 = rng.normal(size=c.f_cols)
    y = precondition(c, x, y0)
    assert np.array_equal(y.cpu().numpy(), y0 + z)
    assert torch.equal(y, precondition(c, x, y0))
    # x and y as one buffer
    d = to_device(x)
    c.ev.schur_precondition_device(d.data_ptr(), d.data_ptr())
    assert np.array_equal(d.cpu().numpy(), x + z)
    assert c.ev.wait() == _cse.CSE_OK


@pytest.mark.parametrize("which,name", [("sixteen", "5+3+8"), ("sixteen", "chain"), ("bal", "evenodd")])
def test_no_edges_agrees_with_cluster_jacobi(gpu, which, name):
    c = device_problem(which)
    init(c)
    labels, _ = forest_case(name, c.num_cameras)
    x, y0 = np.random.default_rng(8).normal(size=c.f_cols), np.zeros(c.f_cols)
    cluster_jacobi(c, labels, want_matrices=False)
    want = precondition(c, x, y0).cpu().numpy()
    _, _, _, scaled = tridiagonal(c, labels, np.zeros((0, 2), np.int32), want_matrices=False)
    got = precondition(c, x, y0).cpu().numpy()
    assert c.ev.wait() == _cse.CSE_OK and int(scaled.item()) == 0
    gap = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"{which} {name}: |tridiagonal without edges - cluster_jacobi| / |.| {gap:.3e}")
    assert gap <= 1e-12
    # the latest build is the active one
    cluster_jacobi(c, labels, want_matrices=False)
    assert np.array_equal(precondition(c, x, y0).cpu().numpy(), want)


# --------------------------------------------------------------------------
# 3. M = S.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("explicit", [False, True], ids=["implicit", "explicit"])
def test_two_joined_clusters_of_all_cameras_solve_S(gpu, explicit):
    c = device_problem("sixteen")
    if c.values is None:
        _, block_col, _ = c.ev.schur_complement_sparse_structure()
        c.values = filled(81 * len(block_col), NAN)
    init(c)
    c.ev.schur_complement_sparse_device(c.values.data_ptr())
    c.S = dense_S(c)
    c.rhs_host = c.rhs.cpu().numpy()
    s_own, _ = solve(c, "zero", explicit)
    for name in ("8+8", "evenodd", "1+15"):
        labels, edges = forest_case(name, 16)
        _, _, _, scaled = tridiagonal(c, labels, edges, want_matrices=False)
        r = np.random.default_rng(9).normal(size=c.f_cols)
        z = precondition(c, r, np.zeros(c.f_cols)).cpu().numpy()
        assert int(scaled.item()) == 0  # M = S is positive definite
        e = eta(c.S, z, r)
        print(f"{name}: eta against the dense S {e:.3e}, bound {solve_bound(144):.3e}")
        assert e <= solve_bound(144)
        s, x = solve(c, "zero", explicit)
        print(f"{name}: iterations {s.num_iterations} (IDENTITY's {s_own.num_iterations})")
        assert s.termination_type == _cse.CG_SUCCESS and s.num_iterations == 1 < s_own.num_iterations
    assert c.ev.wait() == _cse.CSE_OK


# --------------------------------------------------------------------------
# 4. The PCG.
# --------------------------------------------------------------------------
@pytest.mark.parametrize("explicit", [False, True], ids=["implicit", "explicit"])
@pytest.mark.parametrize("which,name", [("sixteen", "2-0-1"), ("sixteen", "several"), ("bal", "halves"),
                                        ("unobserved", "unobserved inside"), ("duplicates", "pairs chain")])
def test_pcg_parity_with_cg_reference(gpu, which, name, explicit):
    c = device_problem(which)
    if c.values is None:
        _, block_col, _ = c.ev.schur_complement_sparse_structure()
        c.values = filled(81 * len(block_col), NAN)
    init(c)
    c.ev.schur_complement_sparse_device(c.values.data_ptr())
    c.S = dense_S(c)
    c.rhs_host = c.rhs.cpu().numpy()
    labels, edges = forest_case(name, c.num_cameras)
    _, _, _, scaled = tridiagonal(c, labels, edges)
    Minv = np.linalg.inv(assemble(c.S, labels, edges, 0.5 if int(scaled.item()) else 1.0))
    for option_set in ("lm", "max4", "min6", "guess", "zero"):
        ref = SU.reference(c.S, Minv, c.rhs_host, option_set)
        assert SU.same_outcome(ref.f64, ref.ld)  # a fair input
        summary, x = solve(c, option_set, explicit)
        err = float(np.linalg.norm((x.astype(LD) - ref.ld.x).astype(np.float64)) /
                    np.linalg.norm(ref.ld.x.astype(np.float64)))
        ratio = err / ref.d_ref if ref.d_ref > 0 else 0.0
        w = note("pcg", ratio, (which, name, option_set, explicit))
        print(f"{which} {name} {option_set}: {outcome(summary)} reference {ref.ld[1:4]} error {err:.3e} "
              f"d_ref {ref.d_ref:.3e} ratio {ratio:.2f}; worst so far {w[0]:.2f} at {w[1]}")
        assert outcome(summary) == (ref.ld.termination_type, ref.ld.reason, ref.ld.num_iterations)
        assert np.isfinite(x).all()
        assert err <= max(10 * ref.d_ref, 1e-14)
        for period in (4, 1):
            s2, x2 = solve(c, option_set, explicit, check_period=period)
            assert np.array_equal(x2, x) and outcome(s2) == outcome(summary), period
            assert (s2.norm_r, s2.rho, s2.pq) == (summary.norm_r, summary.rho, summary.pq)
    assert c.ev.wait() == _cse.CSE_OK
    # the next init brings its own preconditioner back
    rng = np.random.default_rng(10)
    xx, y0 = rng.normal(size=c.f_cols), rng.normal(size=c.f_cols)
    init(c, _cse.SCHUR_IDENTITY)
    assert np.array_equal(precondition(c, xx, y0).cpu().numpy(), y0 + xx)


# --------------------------------------------------------------------------
# 5. The retry.
# --------------------------------------------------------------------------
RETRY_LABELS = np.arange(7, dtype=np.int32)
RETRY_EDGES = np.array([(1, 0), (1, 2), (3, 4), (4, 5)], np.int32)  # paths 0-1-2, 3-4-5, 6


@functools.lru_cache(maxsize=None)
def retry_problem(d_f):
    """The construction: seven cameras in singleton clusters; 8 points seen by
    cameras 0, 1, 2, 12 by cameras 3, 4, 5 and 6 by cameras 5, 6; the Jacobian
    VALUES are not an evaluated Jacobian but standard normal draws (seed 2);
    D_e = 1e-3.  With generic E and F cells the coupling S[0, 2] that the path
    0 - 1 - 2 drops is as strong as the ones it keeps, and with D_f = 0.1 the
    unscaled block of that path has the eigenvalue -0.376 (the halved one
    0.31); the path 3 - 4 - 5 has three times the points per camera and is
    positive definite as it is (0.90).  With D_f = 5 nothing fails."""
    lists = [[0, 1, 2]] * 8 + [[3, 4, 5]] * 12 + [[5, 6]] * 6
    prog = U._program(7, lists, 1)
    jv = np.random.default_rng(2).normal(size=prog.num_jacobian_values)
    c = bind(prog, jv)
    c.D = np.r_[np.full(c.e_cols, 1e-3), np.full(c.f_cols, d_f)]
    c.dj, c.dD, c.db = to_device(jv), to_device(c.D), to_device(SU.right_hand_side(prog))
    c.S_model = U.schur_float64(c.J, c.e_cols, c.D)[0]
    return c


def is_positive_definite(M):
    try:
        np.linalg.cholesky(M)
        return True
    except np.linalg.LinAlgError:
        return False


def test_retry_with_halved_edges(gpu):
    c = retry_problem(0.1)
    labels, edges = RETRY_LABELS, RETRY_EDGES
    paths = path_columns(labels, edges)
    assert [len(p) for p in paths] == [27, 27, 9]
    # The preconditions, on the numpy model, before the device is looked at.
    M1, Mh = assemble(c.S_model, labels, edges), assemble(c.S_model, labels, edges, 0.5)
    a, b = paths[0], paths[1]
    assert not is_positive_definite(M1) and not is_positive_definite(M1[np.ix_(a, a)])
    assert is_positive_definite(Mh)
    assert is_positive_definite(M1[np.ix_(b, b)])  # the healthy path, unscaled
    # with a margin: far from where rounding could decide either way
    assert np.linalg.eigvalsh(M1[np.ix_(a, a)])[0] < -0.1 and np.linalg.eigvalsh(Mh[np.ix_(a, a)])[0] > 0.05
    init(c)
    S = dense_S(c)
    assert np.allclose(S, c.S_model, rtol=1e-9, atol=1e-9)
    clusters, rects, _, scaled = tridiagonal(c, labels, edges)
    x = np.random.default_rng(13).normal(size=c.f_cols)
    z = precondition(c, x, np.zeros(c.f_cols)).cpu().numpy()
    assert int(scaled.item()) == 1
    assert c.ev.wait() == _cse.CSE_OK
    # d_matrices is still unscaled
    check_cells(clusters, S)
    check_rectangles(rects, labels, S)
    # ALL paths' edges are halved, the healthy path's too
    Mdev = assemble(S, labels, edges, 0.5)
    for cols in paths:
        e, bound = eta(Mdev[np.ix_(cols, cols)], z[cols], x[cols]), solve_bound(len(cols))
        print(f"retry, n {len(cols)}: eta {e:.3e}, bound {bound:.3e}")
        assert e <= bound
    unhalved = eta(M1[np.ix_(b, b)], z[b], x[b])
    print(f"the healthy path against its UNSCALED block: eta {unhalved:.3e}")
    assert unhalved > 1e3 * solve_bound(27)
    # a second build repeats the bits, the flag included
    _, _, _, scaled2 = tridiagonal(c, labels, edges, want_matrices=False)
    assert np.array_equal(precondition(c, x, np.zeros(c.f_cols)).cpu().numpy(), z) and int(scaled2.item()) == 1
    # and cse_schur_solve runs with the scaled factor
    xf = filled(c.f_cols, NAN)
    s = c.ev.schur_solve_device(c.rhs.data_ptr(), xf.data_ptr(),
                                _cse.cg_options(max_num_iterations=300, r_tolerance=1e-12, q_tolerance=-1.0,
                                                flags=_cse.CG_ZERO_INITIAL_GUESS))
    assert s.termination_type == _cse.CG_SUCCESS and c.ev.wait() == _cse.CSE_OK
    got = xf.cpu().numpy()
    want = np.linalg.solve(S, c.rhs.cpu().numpy())
    assert np.linalg.norm(got - want) <= 1e-6 * np.linalg.norm(want)


def test_no_retry_when_nothing_fails(gpu):
    c = retry_problem(5.0)
    labels, edges = RETRY_LABELS, RETRY_EDGES
    assert is_positive_definite(assemble(c.S_model, labels, edges))
    init(c)
    S = dense_S(c)
    _, _, _, scaled = tridiagonal(c, labels, edges)
    x = np.random.default_rng(13).normal(size=c.f_cols)
    z = precondition(c, x, np.zeros(c.f_cols)).cpu().numpy()
    assert int(scaled.item()) == 0 and c.ev.wait() == _cse.CSE_OK
    M = assemble(S, labels, edges)
    for cols in path_columns(labels, edges):
        assert eta(M[np.ix_(cols, cols)], z[cols], x[cols]) <= solve_bound(len(cols))


# --------------------------------------------------------------------------
# 6. A pivot that fails in both passes.
# --------------------------------------------------------------------------
def test_a_pivot_that_fails_twice_raises_the_status_word(gpu):
    """d_D = NULL: the unobserved camera 3 has a zero diagonal block, whatever
    its edges are scaled by.  Its path adds zeros, cse_wait reports it, the
    other paths are right; with D > 0 the same call is clean."""
    c = device_problem("unobserved")
    labels = np.array([0, 1, 1, 0, 2, 2, 3, 4], np.int32)  # camera 3 with camera 0
    edges = np.array([(0, 1), (2, 3)], np.int32)            # paths 0-1 (cameras 0 3 1 2), 2-3 (4 5 6), 4 (7)
    init(c, _cse.SCHUR_IDENTITY, None)
    assert c.ev.wait() == _cse.CSE_OK
    S = dense_S(c)
    clusters, rects, _, scaled = tridiagonal(c, labels, edges)
    rng = np.random.default_rng(11)
    x, y0 = rng.normal(size=c.f_cols), rng.normal(size=c.f_cols)
    y = precondition(c, x, y0).cpu().numpy()
    z = precondition(c, x, np.zeros(c.f_cols)).cpu().numpy()
    assert int(scaled.item()) == 1
    assert c.ev.wait() == _cse.CSE_EVALUATION_FAILED
    check_cells(clusters, S)
    check_rectangles(rects, labels, S)
    M = assemble(S, labels, edges, 0.5)
    paths = path_columns(labels, edges)
    assert len(paths) == 3
    for cols in paths:
        if 27 in cols:  # camera 3's path
            assert np.array_equal(y[cols], y0[cols]) and not z[cols].any()
        else:
            assert np.array_equal(y[cols], y0[cols] + z[cols])
            assert eta(M[np.ix_(cols, cols)], z[cols], x[cols]) <= solve_bound(len(cols))
    init(c)
    _, _, _, scaled = tridiagonal(c, labels, edges, want_matrices=False)
    y = precondition(c, x, y0).cpu().numpy()
    assert c.ev.wait() == _cse.CSE_OK
    assert (y != y0).all()


# --------------------------------------------------------------------------
# 7. Refusals.
# --------------------------------------------------------------------------
def test_refusals(gpu):
    dev = torch.device("cuda", 0)
    L = _cse.lib()
    prog = bal.synthetic_program((20, 300, 1500), seed=9)

    def set_forest(ev, edges, num=None):
        edges = None if edges is None else np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
        rc = L.cse_schur_set_cluster_forest(
            ev.handle, None if edges is None or not edges.size else edges.ctypes.data_as(_cse.P_i32),
            (0 if edges is None else len(edges)) if num is None else num)
        if rc < 0:
            assert _cse.last_error(), "a refusal without a message"
        return rc

    def build(ev):
        rc = L.cse_schur_cluster_tridiagonal(ev.handle, None, None)
        if rc < 0:
            assert _cse.last_error(), "a refusal without a message"
        return rc

    # a multi-device handle
    ev = ca.Evaluator(prog, devices=[0, 0])
    assert set_forest(ev, [(0, 1)]) == _cse.CSE_ERR_UNSUPPORTED and "cse_create_multi" in _cse.last_error()
    assert build(ev) == _cse.CSE_ERR_UNSUPPORTED and "cse_create_multi" in _cse.last_error()
    ev.close()
    # not Schur-eligible
    ev = ca.Evaluator(bal.synthetic_program((20, 300, 1500), format=ca.COMPRESSED_ROW, seed=9))
    assert set_forest(ev, [(0, 1)]) == _cse.CSE_ERR_UNSUPPORTED
    assert build(ev) == _cse.CSE_ERR_UNSUPPORTED
    ev.close()
    # held cameras
    ev = ca.Evaluator(held(counts=(16, 700, 2900), const=(0, 3)))
    assert set_forest(ev, [(0, 1)]) == _cse.CSE_ERR_UNSUPPORTED and "held" in _cse.last_error()
    assert build(ev) == _cse.CSE_ERR_UNSUPPORTED and "held" in _cse.last_error()
    ev.close()

    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    ok, _, r, _, jv = ev.evaluate()
    assert ev.schur_structure()[1] == 180
    # no partition
    assert set_forest(ev, [(0, 1)]) == _cse.CSE_ERR_INVALID and "cse_schur_set_clusters has not run" in _cse.last_error()
    labels = sized(5, 5, 4, 3, 3)
    ev.schur_set_clusters(labels)
    # the forest may be set before the init; the build may not run
    assert set_forest(ev, [(0, 1)]) == _cse.CSE_OK
    assert build(ev) == _cse.CSE_ERR_INVALID and "cse_schur_init has not run" in _cse.last_error()
    dj, db = to_device(jv), to_device(-r)
    dD = filled(prog.num_effective_parameters, 1.0)
    rhs, x, y = filled(180, NAN), filled(180, 1.0), filled(180, 0.0)
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), _cse.SCHUR_JACOBI)
    assert build(ev) == _cse.CSE_OK
    # a changed partition drops the forest
    ev.schur_set_clusters(sized(5, 5, 4, 3, 2, 1))
    assert build(ev) == _cse.CSE_ERR_INVALID and "cse_schur_set_cluster_forest has not run" in _cse.last_error()
    assert L.cse_schur_cluster_jacobi(ev.handle, None) == _cse.CSE_OK  # the partition alone serves CLUSTER_JACOBI
    # num_edges = 0 counts as set
    assert set_forest(ev, []) == _cse.CSE_OK and build(ev) == _cse.CSE_OK
    # the forest's own refusals; each leaves the forest in place as it was
    assert set_forest(ev, None, num=2) == _cse.CSE_ERR_INVALID and "null" in _cse.last_error()
    assert set_forest(ev, [(0, 1)], num=-1) == _cse.CSE_ERR_INVALID
    assert set_forest(ev, [(0, 6)]) == _cse.CSE_ERR_INVALID and "edge 0 (0, 6)" in _cse.last_error()
    assert set_forest(ev, [(0, 1), (-1, 2)]) == _cse.CSE_ERR_INVALID and "edge 1" in _cse.last_error()
    assert set_forest(ev, [(2, 2)]) == _cse.CSE_ERR_INVALID and "itself" in _cse.last_error()
    assert set_forest(ev, [(0, 1), (1, 0)]) == _cse.CSE_ERR_INVALID and "twice" in _cse.last_error()
    assert set_forest(ev, [(0, 1), (2, 3), (0, 1)]) == _cse.CSE_ERR_INVALID and "twice" in _cse.last_error()
    assert set_forest(ev, [(2, 3), (2, 4), (2, 5)]) == _cse.CSE_ERR_UNSUPPORTED and "cluster 2" in _cse.last_error()
    assert set_forest(ev, [(2, 3), (3, 4), (4, 2)]) == _cse.CSE_ERR_UNSUPPORTED and "cycle" in _cse.last_error()
    assert build(ev) == _cse.CSE_OK
    ev.schur_set_clusters(sized(9, 8, 3))
    assert set_forest(ev, [(1, 2), (0, 1)]) == _cse.CSE_ERR_UNSUPPORTED
    assert "edge 1 (0, 1) hold 17 cameras" in _cse.last_error()
    assert build(ev) == _cse.CSE_ERR_INVALID  # and there is still no forest for this partition
    ev.schur_set_clusters(sized(16, 4))  # a cluster of 16 without an edge is legal; with one it is not
    assert set_forest(ev, [(0, 1)]) == _cse.CSE_ERR_UNSUPPORTED and "20 cameras" in _cse.last_error()
    assert set_forest(ev, []) == _cse.CSE_OK and build(ev) == _cse.CSE_OK
    # an unknown preconditioner is still refused by the init
    assert L.cse_schur_init(ev.handle, dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), 4) \
        == _cse.CSE_ERR_INVALID
    # legal calls afterwards still work
    ev.schur_set_clusters(sized(5, 5, 4, 3, 3))
    assert set_forest(ev, [(4, 3), (0, 1), (1, 2)]) == _cse.CSE_OK and build(ev) == _cse.CSE_OK
    ev.schur_precondition_device(x.data_ptr(), y.data_ptr())
    summary = ev.schur_solve_device(rhs.data_ptr(), x.data_ptr(),
                                    _cse.cg_options(r_tolerance=1e-8, flags=_cse.CG_ZERO_INITIAL_GUESS))
    assert ev.wait() == _cse.CSE_OK
    assert summary.termination_type == _cse.CG_SUCCESS and summary.num_iterations >= 1
    assert torch.isfinite(y).all() and float(y.norm()) > 0
    # a changed forest deactivates the factor: the init's own preconditioner is back
    xx, y0 = filled(180, 1.0), filled(180, 0.0)
    with_factor = y0.clone()
    ev.schur_precondition_device(xx.data_ptr(), with_factor.data_ptr())
    assert set_forest(ev, [(0, 1)]) == _cse.CSE_OK
    own = y0.clone()
    ev.schur_precondition_device(xx.data_ptr(), own.data_ptr())
    assert not torch.equal(own, with_factor)
    ev.schur_init_device(dj.data_ptr(), dD.data_ptr(), db.data_ptr(), rhs.data_ptr(), _cse.SCHUR_JACOBI)
    again = y0.clone()
    ev.schur_precondition_device(xx.data_ptr(), again.data_ptr())
    assert torch.equal(own, again)
    ev.close()


# --------------------------------------------------------------------------
# 8. Release.
# --------------------------------------------------------------------------
def test_create_tridiagonal_solve_destroy_does_not_leak(gpu):
    prog = bal.synthetic_program("banded-30-4000-w6", loss=ca.Loss.huber(1.0), seed=4)
    dev = torch.device("cuda", 0)
    n, m = prog.num_effective_parameters, prog.num_residuals
    jac = torch.empty(prog.num_jacobian_values, dtype=torch.float64, device=dev)
    st = torch.from_numpy(prog.state).to(dev)
    cost = torch.zeros(1, dtype=torch.float64, device=dev)
    res = torch.empty(m, dtype=torch.float64, device=dev)
    D = torch.ones(n, dtype=torch.float64, device=dev)
    rhs, x, y = (torch.zeros(270, dtype=torch.float64, device=dev) for _ in range(3))
    o = _cse.cg_options(max_num_iterations=20, r_tolerance=1e-6, flags=_cse.CG_ZERO_INITIAL_GUESS)

    def cycle(size):
        ev = ca.Evaluator(prog, device=0)
        ev.evaluate_device(st.data_ptr(), cost.data_ptr(), res.data_ptr(), None, jac.data_ptr())
        ev.schur_init_device(jac.data_ptr(), D.data_ptr(), res.data_ptr(), rhs.data_ptr(), _cse.SCHUR_IDENTITY)
        for s in (size, size // 2):  # a second structure on the same handle
            labels = clustering.blocks(30, s)
            k = int(labels.max()) + 1
            ev.schur_set_clusters(labels)
            ev.schur_set_cluster_forest([(g, g + 1) for g in range(k - 1)])
            ev.schur_cluster_tridiagonal_device()
            ev.schur_precondition_device(rhs.data_ptr(), y.data_ptr())
            ev.schur_solve_device(rhs.data_ptr(), x.data_ptr(), o)
        assert ev.wait() == 0
        ev.close()

    cycle(8)
    cycle(4)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(dev)
    for k in range(10):
        cycle(8 if k % 2 else 4)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(dev)
    assert free0 - free1 < 2 << 20, (free0, free1)


# --------------------------------------------------------------------------
# 9. The driver.
# --------------------------------------------------------------------------
DRIVER = ["--synthetic", "banded-24-3000-w6", "--robustify", "--point_sigma", "0.05", "--num_iterations", "3"]


@functools.lru_cache(maxsize=None)
def driver_run(*extra):
    from ceres_amd import bundle_adjuster
    stats = {}
    return bundle_adjuster.main(DRIVER + list(extra), stats) + (stats,)


@pytest.mark.parametrize("extra", [(), ("--device_pcg",)], ids=["host-loop", "device-pcg"])
def test_bundle_adjuster(gpu, capsys, extra):
    """A small banded problem: every step accepted and the cost falling.  The
    preconditioners solve the same system to the same eta; what differs is
    where each PCG stops, so the final-cost gap to schur_jacobi's run is held
    to the gap jacobi's run leaves to schur_jacobi's, times 10, plus 1e-12 of
    the cost (tests/test_schur_held_gpu.py's bound for two solvers)."""
    _, want, rows_sj, _ = driver_run("--preconditioner", "schur_jacobi", *extra)
    _, jacobi, _, _ = driver_run(*extra)
    c0, c1, rows, stats = driver_run("--preconditioner", "cluster_tridiagonal", "--visibility_clustering", "blocks",
                                     "--max_cluster_cameras", "4", *extra)
    out = capsys.readouterr().out
    print(out)
    gap, allowed = abs(c1 - want), 10 * abs(jacobi - want) + 1e-12 * want
    print(f"{extra}: final cost {c1:.12e}, schur_jacobi's {want:.12e}, gap {gap:.3e}, allowed {allowed:.3e}; "
          f"ls_iter {[r[6] for r in rows]} against schur_jacobi's {[r[6] for r in rows_sj]}")
    costs = [c0] + [row[2] for row in rows]
    assert len(rows) == 3 and all(r[7] for r in rows) and all(r[6] > 0 for r in rows)
    assert all(b < a for a, b in zip(costs[:-1], costs[1:])) and c1 == costs[-1]
    assert gap <= allowed
    assert "cluster_tridiagonal: 5 forest edges, 1 paths, the longest of 6 clusters" in out
    assert len(stats["scaled_solves"]) == 3 and "of 3 linear solves were scaled" in out
    assert list(stats["path_lengths"]) == [6] and len(stats["forest_edges"]) == 5
