"""CPU: CLUSTER_TRIDIAGONAL's entry points, its host-only forest and plan, a
host replay of its kernels, the forest in ceres_amd/clustering.py, the banded
synthetic problem and the driver's flags.

cse_schur_set_cluster_forest / cse_schur_cluster_tridiagonal (include/cse.h)
install the reference's CLUSTER_TRIDIAGONAL preconditioner.  Here, without a
GPU: the symbols are exported, wrapped and declared and the ABI version did not
move; the forest's validation and paths, the pair plan filtered by label or
forest edge with both tile layouts against brute force, and a host replay of
TridiagonalFactorKernel (both passes, the retry on an injected matrix) and
TridiagonalApplyKernel against the Cholesky-solve backward-error bound, pass
their stand-alone driver under AddressSanitizer + UBSan
(tests/cpp/schur_tridiagonal_driver.cpp); numpy's own solve of the same
matrices is held to the same bound.
"""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse, bal, clustering

from test_schur_cluster import eta, hand_built, solve_bound

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


def test_entry_points_are_exported_wrapped_and_declared():
    lib = C.CDLL(_cse.LIB_PATH)
    for name in ("cse_schur_set_cluster_forest", "cse_schur_cluster_tridiagonal"):
        assert hasattr(lib, name), name
        assert name in _cse.SIGNATURES
    assert _cse.SIGNATURES["cse_schur_set_cluster_forest"][1] == [C.c_void_p, _cse.P_i32, C.c_int32]
    assert _cse.SIGNATURES["cse_schur_cluster_tridiagonal"][1] == [C.c_void_p, C.c_void_p, C.c_void_p]
    assert callable(ca.Evaluator.schur_set_cluster_forest)
    assert callable(ca.Evaluator.schur_cluster_tridiagonal_device)
    with open(os.path.join(os.path.dirname(CPP), "..", "include", "cse.h")) as f:
        header = f.read()
    assert "int cse_schur_set_cluster_forest(cse_evaluator* ev, const int32_t* edges" in header
    assert "int cse_schur_cluster_tridiagonal(cse_evaluator* ev, double* d_matrices" in header
    # cse_schur_init's enum got no new value, the ABI did not move
    assert "CSE_SCHUR_CLUSTER" not in header.replace("CSE_SCHUR_MAX_CLUSTER_CAMERAS", "")
    assert _cse.lib().cse_abi_version() == 6 and _cse.CSE_ABI_VERSION == 6


def test_refusals_that_need_no_device():
    L = _cse.lib()
    assert L.cse_schur_set_cluster_forest(None, None, 0) == _cse.CSE_ERR_INVALID and _cse.last_error()
    assert L.cse_schur_cluster_tridiagonal(None, None, None) == _cse.CSE_ERR_INVALID and _cse.last_error()


def test_forest_plan_and_replay_driver_under_asan_ubsan(tmp_path):
    """The stand-alone driver, g++ -fsanitize=address,undefined with static
    runtimes (no LD_PRELOAD): every refusal of the forest, the paths, the
    filtered plan and both tile layouts against brute force on every
    partition of the issue, both kernels replayed in their order within
    n gamma_{3n+1} per path, and the retry on T (x) I_9.  numpy's Cholesky
    solve of each replayed path is held to the same bound."""
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "schur_tridiagonal.mk", "driver"])
    out = subprocess.run([os.path.join(CPP, "build", "schur_tridiagonal_driver"), str(tmp_path)],
                         capture_output=True, text=True)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0
    assert out.stdout.rstrip().endswith("OK")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    for what in ("label out of range", "g = h", "duplicate, reversed", "degree 3", "cycle", "17 cameras on an edge",
                 "singletons in one path", "two clusters of 8", "sizes (1, 15)", "sizes (15, 1)", "sizes (5, 3, 8)",
                 "path 2-0-1, edge given as (h, g)", "interleaved (even / odd)", "unobserved camera inside a cluster",
                 "edge without a shared point", "duplicates", "several paths and lone clusters", "several chunks",
                 "retry a = 0.8: scaled 1", "retry a = 0.6: scaled 0"):
        assert what in out.stdout, what
    files = sorted(tmp_path.glob("replay_*.bin"))
    assert len(files) >= 12
    worst = 0.0
    for path in files:
        data = np.fromfile(path)
        n = int(round(np.sqrt(data.size + 1) - 1))
        assert data.size == n * n + 2 * n
        M, r, z = data[:n * n].reshape(n, n), data[n * n:n * n + n], data[n * n + n:]
        assert np.array_equal(M, M.T)
        L = np.linalg.cholesky(M)
        z_numpy = np.linalg.solve(L.T, np.linalg.solve(L, r))
        e_replay, e_numpy = eta(M, z, r), eta(M, z_numpy, r)
        print(f"{path.name}: n = {n:3d}: eta of the replay {e_replay:.3e}, of numpy {e_numpy:.3e}, "
              f"bound {solve_bound(n):.3e}")
        assert e_replay <= solve_bound(n) and e_numpy <= solve_bound(n)
        worst = max(worst, e_replay / solve_bound(n))
    print(f"worst eta / bound of the replay: {worst:.3e}")
    # the retry's matrix is the HALVED one: T_{0.4} (x) I
    M = np.fromfile(tmp_path / "replay_retry8_0.bin")[:27 * 27].reshape(27, 27)
    T = np.array([[1, 0.4, 0], [0.4, 1, 0.4], [0, 0.4, 1]])
    assert np.array_equal(M, np.kron(T, np.eye(9)))
    assert np.linalg.eigvalsh(np.kron(2 * T - np.eye(3), np.eye(9))).min() < 0  # a = 0.8 is indefinite


# --------------------------------------------------------------------------
# ceres_amd/clustering.py: the cluster graph and the forest
# --------------------------------------------------------------------------
def forest_restated(num, g, h, w, sizes=None, cap=16):
    """Degree2MaximumSpanningForest, plainly: sort (w, (g, h)) descending;
    components as sets."""
    edges = sorted(((float(x), (int(a), int(b))) for a, b, x in zip(g, h, w)), reverse=True)
    comp = [{v} for v in range(num)]
    degree = [0] * num
    kept = []
    for _, (a, b) in edges:
        if degree[a] == 2 or degree[b] == 2:
            continue
        if sizes is not None and sizes[a] + sizes[b] > cap:
            continue
        ca_, cb_ = next(s for s in comp if a in s), next(s for s in comp if b in s)
        if ca_ is cb_:
            continue
        comp.remove(cb_)
        ca_ |= cb_
        degree[a] += 1
        degree[b] += 1
        kept.append((a, b))
    return kept


def is_degree2_forest(num, edges):
    degree = np.bincount(np.asarray(edges, np.int64).ravel(), minlength=num) if len(edges) else np.zeros(num, int)
    if degree.max(initial=0) > 2:
        return False
    try:
        paths = clustering.forest_paths(num, edges)
    except ValueError:
        return False
    return sum(len(p) for p in paths) == num and sum(len(p) - 1 for p in paths) == len(edges)


def test_cluster_graph_against_set_intersections():
    ci, pi, sees = hand_built()
    labels = np.array([0, 1, 1, 2, 0, 3, 4, 0, 3, 3])
    # a duplicate observation counts once
    g, h, w = clustering.cluster_graph(np.r_[ci, 6], np.r_[pi, 3], labels)
    points = {}
    for c, p in sees.items():
        points.setdefault(int(labels[c]), set()).update(p)
    want = {}
    for a in range(5):
        for b in range(a + 1, 5):
            if points[a] & points[b]:
                want[(a, b)] = len(points[a] & points[b])
    assert {(int(a), int(b)): int(x) for a, b, x in zip(g, h, w)} == want
    assert want == {(0, 4): 8}  # only the chain camera 6 shares points with group one
    rng = np.random.default_rng(5)
    for _ in range(5):
        ncam, npt = 12, 30
        ci, pi = rng.integers(0, ncam, 90), rng.integers(0, npt, 90)
        labels = clustering.relabel(rng.integers(0, 5, ncam))
        g, h, w = clustering.cluster_graph(ci, pi, labels)
        k = int(labels.max()) + 1
        sets = [set(pi[labels[ci] == a].tolist()) for a in range(k)]
        want = {(a, b): len(sets[a] & sets[b]) for a in range(k) for b in range(a + 1, k) if sets[a] & sets[b]}
        assert {(int(a), int(b)): int(x) for a, b, x in zip(g, h, w)} == want


def test_forest_hand_cases():
    f = clustering.degree2_maximum_spanning_forest
    # tie-breaking: equal weights go to the lexicographically LARGER pair first,
    # so (1, 2) and (0, 2) are taken and (0, 1) closes a cycle
    assert f(3, [0, 0, 1], [1, 2, 2], [5, 5, 5]).tolist() == [[1, 2], [0, 2]]
    # the degree-2 skip: vertex 0 takes its two heaviest edges; (0, 3) is
    # refused although it joins two components
    assert f(4, [0, 0, 0], [1, 2, 3], [9, 8, 7]).tolist() == [[0, 1], [0, 2]]
    # the cycle skip: (0, 2) would close 0 - 1 - 2; the lighter (2, 3) is taken
    assert f(4, [0, 1, 0, 2], [1, 2, 2, 3], [9, 8, 7, 1]).tolist() == [[0, 1], [1, 2], [2, 3]]
    # the camera-sum skip (ours): 9 + 8 cameras do not fit one step
    sizes = [9, 8, 7]
    assert f(3, [0, 1], [1, 2], [9, 1], sizes=sizes).tolist() == [[1, 2]]
    assert f(3, [0, 1], [1, 2], [9, 1]).tolist() == [[0, 1], [1, 2]]
    assert f(3, [0, 1], [1, 2], [9, 1], sizes=sizes, max_edge_cameras=17).tolist() == [[0, 1], [1, 2]]
    # edges given as (h, g) are the same edges
    assert f(3, [1, 2, 2], [0, 0, 1], [5, 5, 5]).tolist() == [[1, 2], [0, 2]]
    assert f(3, [], [], []).shape == (0, 2)
    assert clustering.forest_paths(5, [[3, 1], [1, 4]]) == [[0], [2], [3, 1, 4]]
    with pytest.raises(ValueError):
        clustering.forest_paths(3, [[0, 1], [1, 2], [2, 0]])


def test_forest_against_a_plain_restatement():
    rng = np.random.default_rng(17)
    for num in (1, 2, 5, 17, 40):
        a, b = np.triu_indices(num, 1)
        pick = rng.random(len(a)) < 4.0 / max(num, 2)
        a, b = a[pick], b[pick]
        w = rng.integers(1, 4, len(a))  # many ties
        sizes = rng.integers(1, 13, num)
        for s in (None, sizes):
            got = clustering.degree2_maximum_spanning_forest(num, a, b, w, sizes=s)
            assert [tuple(e) for e in got.tolist()] == forest_restated(num, a, b, w, s)
            assert is_degree2_forest(num, got)
            if s is not None and len(got):
                assert (sizes[got[:, 0]] + sizes[got[:, 1]]).max() <= 16


# --------------------------------------------------------------------------
# bal.synthetic_banded
# --------------------------------------------------------------------------
def test_banded_cameras_are_distinct_and_local():
    for (Cn, P, O, W, seed) in ((49, 300, 1250, 8, 1), (20, 100, 450, 5, 2), (16, 64, 64, 1, 3), (12, 50, 600, 12, 4)):
        cams, pts, ci, pi, obs = bal.synthetic_banded(Cn, P, O, W, seed=seed)
        assert cams.shape == (Cn, 9) and pts.shape == (P, 3) and obs.shape == (O, 2) and len(ci) == O
        assert np.array_equal(pi, np.sort(pi)) and ci.min() >= 0 and ci.max() < Cn
        spans = set()
        for p in range(P):
            c = ci[pi == p]
            assert len(c) in (O // P, O // P + 1) and len(set(c.tolist())) == len(c)
            assert c.max() - c.min() < W
            spans.add(int(c.min()))
        assert len(spans) > 1 or W == Cn  # not one window for all
        # the geometry is synthetic()'s: the same cameras and points for the seed
        ref = bal._synthetic(Cn, P, O, seed, 0.05)
        assert np.array_equal(cams, ref[0]) and np.array_equal(pts, ref[1])
    with pytest.raises(ValueError):
        bal.synthetic_banded(10, 10, 50, 4)  # five cameras a point from a window of four
    with pytest.raises(ValueError):
        bal.synthetic_banded(10, 10, 20, 11)


def test_banded_names():
    assert bal.parse_banded("banded-49-7776-w8") == (49, 7776, 4 * 7776, 8)
    assert bal.parse_banded("banded-49-7776-31843-w16") == (49, 7776, 31843, 16)
    for bad in ("problem-16-22106", "banded-49-7776", "banded-49-x-w8", "banded-49-7776-w0", "banded-1-2-3-4-w5"):
        assert bal.parse_banded(bad) is None
    assert bal.synthetic_name("problem-16-22106") == "problem-16-22106"
    with pytest.raises(ValueError):
        bal.synthetic_name("problem-17")
    a = bal.synthetic_named("banded-12-40-w6", seed=3)
    b = bal.synthetic_banded(12, 40, 160, 6, seed=3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    prog = bal.synthetic_program("banded-12-40-w6", seed=3, compile=False)
    assert prog.num_residual_blocks == 160


# sha256 over cameras, points, cam_idx, pt_idx, obs of bal._synthetic, recorded
# from the parent of the commit that added synthetic_banded.
RECORDED = {
    ((7, 50, 170), 0xCE2E5, 0.05): "b25f8d7438c449992db91a705ad3c01de6e81d358a8a0677483e662c88537b16",
    ((16, 300, 1100), 5, 0.05): "a255b2c8e9d9c52c52c3ff8d6ce1fec0c4c728ae0f2f25640853996b7ff54bbf",
    ((49, 400, 1500), 11, 0.2): "e4079542c1815e9321d19ae4684574b93ead67f5d42c616ac34b230fd2e8b46f",
    ((5, 20, 90), 3, 0.05): "9370c7821f5780a38c1856a421d69a85f384cbb7f2881cee18d0932fafd109d9",  # the dense-rows branch
}


def test_synthetic_is_byte_identical_to_the_recorded_parent():
    for (counts, seed, outliers), want in RECORDED.items():
        h = hashlib.sha256()
        for a in bal.synthetic(*counts, seed=seed, outlier_fraction=outliers):
            h.update(np.ascontiguousarray(a).tobytes())
        assert h.hexdigest() == want, counts


def test_driver_flags():
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", "banded-49-7776-w8", "--preconditioner", "cluster_tridiagonal"]
    args = bundle_adjuster.parse(base)
    assert (args.visibility_clustering, args.cluster_min_similarity, args.max_cluster_cameras) == \
        ("single_linkage", 0.9, 8)
    assert bundle_adjuster.parse(base + ["--max_cluster_cameras", "5", "--device_pcg"]).max_cluster_cameras == 5
    # the other preconditioners keep their default
    assert bundle_adjuster.parse(["--synthetic", "problem-16-22106", "--preconditioner", "cluster_jacobi"]) \
        .max_cluster_cameras == 16
    assert bundle_adjuster.parse(["--synthetic", "problem-16-22106"]).max_cluster_cameras == 16
    with pytest.raises(SystemExit, match="held_cameras"):
        bundle_adjuster.parse(base + ["--held_cameras", "2"])
    for solver in ("cgnr", "dense_schur"):
        with pytest.raises(SystemExit, match="cluster_tridiagonal"):
            bundle_adjuster.parse(base + ["--linear_solver", solver])
    for bad in ("0", "17"):
        with pytest.raises(SystemExit, match="max_cluster_cameras"):
            bundle_adjuster.parse(base + ["--max_cluster_cameras", bad])
    with pytest.raises(SystemExit):
        bundle_adjuster.parse(["--synthetic", "banded-49-w8", "--preconditioner", "cluster_tridiagonal"])
