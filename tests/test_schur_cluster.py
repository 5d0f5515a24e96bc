"""CPU: CLUSTER_JACOBI's entry points, its host-only plan, a host replay of its
kernels, the clustering module and the driver's flags.

cse_schur_set_clusters / cse_schur_cluster_jacobi (include/cse.h) install the
reference's CLUSTER_JACOBI preconditioner: the blocks of S over the camera
clusters, factored.  Here, without a GPU: the symbols are exported, wrapped and
declared and the ABI version did not move; the cluster-filtered pair plan with
its tile layout (cse::PlanSchurClusters) against brute force, and a host replay
of ClusterFactorKernel and ClusterApplyKernel in the kernels' order against
the Cholesky-solve backward-error bound, pass their stand-alone driver under
AddressSanitizer + UBSan (tests/cpp/schur_cluster_driver.cpp); numpy's own
solve of the same matrices is held to the same bound and both figures are
printed; ceres_amd/clustering.py against brute-force connected components;
bundle_adjuster's flags.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse, clustering

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
U53 = 2.0 ** -53


def gamma(k):
    return k * U53 / (1.0 - k * U53)


def solve_bound(n):
    """n gamma_{3n+1}: the normwise backward error of a Cholesky solve
    (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.4)."""
    return n * gamma(3 * n + 1)


def eta(M, z, r):
    """|M z - r|_inf / (|M|_inf |z|_inf + |r|_inf), the residual in np.longdouble."""
    res = np.abs(M.astype(np.longdouble) @ z.astype(np.longdouble) - r).max()
    return float(res / (np.abs(M).sum(axis=1).max() * np.abs(z).max() + np.abs(r).max()))


def test_entry_points_are_exported_wrapped_and_declared():
    lib = C.CDLL(_cse.LIB_PATH)
    for name in ("cse_schur_set_clusters", "cse_schur_cluster_jacobi"):
        assert hasattr(lib, name), name
        assert name in _cse.SIGNATURES
    assert _cse.SIGNATURES["cse_schur_set_clusters"][1] == [C.c_void_p, _cse.P_i32, C.c_int64, C.c_int32]
    assert _cse.SIGNATURES["cse_schur_cluster_jacobi"][1] == [C.c_void_p, C.c_void_p]
    assert callable(ca.Evaluator.schur_set_clusters) and callable(ca.Evaluator.schur_cluster_jacobi_device)
    with open(os.path.join(os.path.dirname(CPP), "..", "include", "cse.h")) as f:
        header = f.read()
    assert "#define CSE_SCHUR_MAX_CLUSTER_CAMERAS 16" in header
    assert _cse.SCHUR_MAX_CLUSTER_CAMERAS == 16
    assert "int cse_schur_set_clusters(cse_evaluator* ev, const int32_t* cluster_of_camera," in header
    assert "int cse_schur_cluster_jacobi(cse_evaluator* ev, double* d_matrices" in header
    # cse_schur_init's enum got no new value
    assert "CSE_SCHUR_CLUSTER" not in header.replace("CSE_SCHUR_MAX_CLUSTER_CAMERAS", "")


def test_abi_version_is_still_6():
    assert _cse.lib().cse_abi_version() == 6 and _cse.CSE_ABI_VERSION == 6


def test_refusals_that_need_no_device():
    L = _cse.lib()
    assert L.cse_schur_set_clusters(None, None, 0, 0) == _cse.CSE_ERR_INVALID
    assert L.cse_schur_cluster_jacobi(None, None) == _cse.CSE_ERR_INVALID and _cse.last_error()


def test_plan_and_replay_driver_under_asan_ubsan(tmp_path):
    """The stand-alone driver, g++ -fsanitize=address,undefined with static
    runtimes: the filtered plan and the tile layout against brute force on
    every partition of the issue, the factor and the apply replayed in the
    kernels' order within n gamma_{3n+1}.  numpy's Cholesky solve of the same
    M and r is held to the same bound; both figures are printed."""
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "schur_cluster.mk", "driver"])
    out = subprocess.run([os.path.join(CPP, "build", "schur_cluster_driver"), str(tmp_path)],
                         capture_output=True, text=True)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0
    assert out.stdout.rstrip().endswith("OK")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    for what in ("singletons", "one cluster of all", "interleaved", "unobserved + non-covisible pair",
                 "duplicates", "several chunks", "16 + 16 + 8"):
        assert what in out.stdout, what
    for nc in (1, 2, 3, 4, 7, 11, 16):
        n = 9 * nc
        data = np.fromfile(tmp_path / f"replay_{nc}.bin")
        assert data.size == n * n + 2 * n
        M, r, z = data[:n * n].reshape(n, n), data[n * n:n * n + n], data[n * n + n:]
        L = np.linalg.cholesky(M)
        z_numpy = np.linalg.solve(L.T, np.linalg.solve(L, r))
        e_replay, e_numpy = eta(M, z, r), eta(M, z_numpy, r)
        print(f"n = {n:3d}: eta of the replay {e_replay:.3e}, of numpy {e_numpy:.3e}, bound {solve_bound(n):.3e}, "
              f"condition {np.linalg.cond(M):.1e}")
        assert e_replay <= solve_bound(n) and e_numpy <= solve_bound(n)
    assert solve_bound(144) == pytest.approx(6.9e-12, rel=0.01)


# --------------------------------------------------------------------------
# ceres_amd/clustering.py
# --------------------------------------------------------------------------
def components(num, i, j, keep):
    """Brute-force connected components, labelled by smallest member."""
    adj = np.eye(num, dtype=bool)
    adj[i[keep], j[keep]] = adj[j[keep], i[keep]] = True
    reach = adj.copy()
    for _ in range(num):
        reach = (reach.astype(np.int64) @ adj.astype(np.int64)) > 0
    labels, nxt = -np.ones(num, np.int64), 0
    for c in range(num):
        if labels[c] < 0:
            labels[reach[c]] = nxt
            nxt += 1
    return labels


def hand_built():
    """Ten cameras: three groups that see the same points each (0, 4, 7 /
    1, 2 / 5, 8, 9), a loner (3), and a chain 6 - 0: camera 6 sees eight of
    group one's ten points and two of its own."""
    sees = {0: range(0, 10), 4: range(0, 10), 7: range(0, 10),
            1: range(10, 16), 2: range(10, 16),
            5: range(16, 20), 8: range(16, 20), 9: range(16, 20),
            3: range(20, 23),
            6: list(range(0, 8)) + [23, 24]}
    ci = np.concatenate([[c] * len(list(p)) for c, p in sees.items()])
    pi = np.concatenate([list(p) for p in sees.values()])
    return ci, pi, sees


def test_visibility_weights():
    ci, pi, sees = hand_built()
    # a duplicate observation counts once
    i, j, w, seen = clustering.visibility_edges(np.r_[ci, 0], np.r_[pi, 0], 10)
    assert list(seen) == [len(set(sees[c])) for c in range(10)]
    got = {(int(a), int(b)): float(x) for a, b, x in zip(i, j, w)}
    want = {}
    for a in range(10):
        for b in range(a + 1, 10):
            shared = len(set(sees[a]) & set(sees[b]))
            if shared:
                want[(a, b)] = shared / np.sqrt(len(set(sees[a])) * len(set(sees[b])))
    assert got.keys() == want.keys()
    assert all(got[k] == pytest.approx(want[k], rel=1e-15) for k in want)
    assert got[(0, 4)] == 1.0 and got[(0, 6)] == pytest.approx(0.8)


def test_single_linkage_against_connected_components():
    ci, pi, _ = hand_built()
    i, j, w, _ = clustering.visibility_edges(ci, pi, 10)
    labels = clustering.single_linkage(10, i, j, w)  # 0.9: the chain's 0.8 stays out
    assert list(labels) == [0, 1, 1, 2, 0, 3, 4, 0, 3, 3]
    assert np.array_equal(labels, components(10, i, j, w >= 0.9))
    joined = clustering.single_linkage(10, i, j, w, 0.8)  # camera 6 joins group one
    assert list(joined) == [0, 1, 1, 2, 0, 3, 0, 0, 3, 3]
    assert np.array_equal(joined, components(10, i, j, w >= 0.8))
    # random graphs
    rng = np.random.default_rng(3)
    for num in (1, 2, 17, 40):
        a, b = np.triu_indices(num, 1)
        pick = rng.random(len(a)) < 1.5 / max(num, 2)
        a, b, wt = a[pick], b[pick], rng.random(int(pick.sum()))
        for t in (0.0, 0.3, 0.9):
            assert np.array_equal(clustering.single_linkage(num, a, b, wt, t), components(num, a, b, wt >= t))


def test_single_linkage_is_single():
    """A chain a - b - c in which only a-b and b-c reach the threshold: one
    cluster, although a and c are not similar."""
    i, j, w = np.array([0, 1, 0]), np.array([1, 2, 2]), np.array([0.95, 0.92, 0.1])
    assert list(clustering.single_linkage(4, i, j, w)) == [0, 0, 0, 1]
    assert list(clustering.single_linkage(4, i, j, w, 0.93)) == [0, 0, 1, 2]


def test_cap_rule():
    labels = np.array([1, 0, 1, 1, 0, 1, 1, 2, 1])  # cluster 1: cameras 0 2 3 5 6 8
    assert list(clustering.cap_clusters(labels, 16)) == [0, 1, 0, 0, 1, 0, 0, 2, 0]
    # runs of 4 in camera order: 0 2 3 5 | 6 8
    assert list(clustering.cap_clusters(labels, 4)) == [0, 1, 0, 0, 1, 0, 2, 3, 2]
    assert list(clustering.cap_clusters(labels, 1)) == list(range(9))
    one = clustering.cap_clusters(np.zeros(40, int))
    assert list(np.bincount(one)) == [16, 16, 8] and list(one[:17]) == [0] * 16 + [1]
    assert list(clustering.blocks(10, 4)) == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2]
    with pytest.raises(ValueError):
        clustering.cap_clusters(labels, 0)
    with pytest.raises(ValueError):
        clustering.cluster_cameras([0], [0], 1, max_cluster_cameras=17)
    ci, pi, _ = hand_built()
    assert list(clustering.cluster_cameras(ci, pi, 10, max_cluster_cameras=2)) == [0, 1, 1, 2, 0, 3, 4, 5, 3, 6]
    assert list(clustering.cluster_cameras(ci, pi, 10, "blocks", max_cluster_cameras=5)) == [0] * 5 + [1] * 5


def test_driver_flags():
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", "problem-16-22106", "--preconditioner", "cluster_jacobi"]
    args = bundle_adjuster.parse(base)
    assert (args.visibility_clustering, args.cluster_min_similarity, args.max_cluster_cameras) == \
        ("single_linkage", 0.9, 16)
    args = bundle_adjuster.parse(base + ["--visibility_clustering", "blocks", "--max_cluster_cameras", "4",
                                         "--device_pcg"])
    assert args.visibility_clustering == "blocks" and args.max_cluster_cameras == 4
    with pytest.raises(SystemExit, match="held_cameras"):
        bundle_adjuster.parse(base + ["--held_cameras", "2"])
    for solver in ("cgnr", "dense_schur"):
        with pytest.raises(SystemExit, match="cluster_jacobi"):
            bundle_adjuster.parse(base + ["--linear_solver", solver])
    for bad in ("0", "17"):
        with pytest.raises(SystemExit, match="max_cluster_cameras"):
            bundle_adjuster.parse(base + ["--max_cluster_cameras", bad])
    with pytest.raises(SystemExit, match="cluster_min_similarity"):
        bundle_adjuster.parse(base + ["--cluster_min_similarity", "1.5"])
    with pytest.raises(SystemExit):
        bundle_adjuster.parse(base + ["--visibility_clustering", "canonical_views"])
