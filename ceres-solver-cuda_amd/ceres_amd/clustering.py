"""Camera partitions for CLUSTER_JACOBI (Evaluator.schur_set_clusters) and the
cluster forest of CLUSTER_TRIDIAGONAL (Evaluator.schur_set_cluster_forest), on
the host in numpy.

The reference's visibility-based preconditioners cluster the cameras by what
they see.  Camera i sees the point set V_i; the visibility graph joins two
cameras that share a point with the weight

    w_ij = |V_i n V_j| / sqrt(|V_i| |V_j|)

(1 when they see exactly the same points).  Single-linkage clustering at a
threshold `min_similarity` (the reference's default: 0.9) is the connected
components of the edges with w_ij >= min_similarity.  Clusters are labelled
0 .. k-1 in the order of their smallest member.

The device factors one cluster in the LDS of one workgroup, so a cluster has
at most _cse.SCHUR_MAX_CLUSTER_CAMERAS cameras: cap_clusters cuts a larger one
into runs of at most that many cameras in camera order.

CLUSTER_TRIDIAGONAL keeps the couplings along a degree-2 maximum spanning
forest of the cluster graph (cluster_graph, degree2_maximum_spanning_forest):
the weight of (g, h) is the number of points seen from both clusters.  The
device eliminates the two clusters of an edge in one workgroup's LDS, so they
hold at most _cse.SCHUR_MAX_CLUSTER_CAMERAS cameras together; a cluster cap of
DEFAULT_TRIDIAGONAL_CLUSTER_CAMERAS (8) makes every edge fit.

Canonical-views clustering, the reference's other choice, is not implemented.
"""
import numpy as np

from . import _cse

DEFAULT_MIN_SIMILARITY = 0.9  # the reference's single-linkage threshold


def shared_points(camera_index, point_index, num_cameras):
    """(i, j, shared, seen): the pairs i < j that see a common point, in
    lexicographic order, with shared = |V_i n V_j|, and seen[c] = |V_c|.  A
    point observed by one camera several times counts once.  Work and memory
    are the sum over the points of k_p^2 for k_p cameras a point."""
    cam = np.asarray(camera_index, np.int64)
    pt = np.asarray(point_index, np.int64)
    C = int(num_cameras)
    if cam.size and (cam.min() < 0 or cam.max() >= C):
        raise ValueError("a camera index outside [0, num_cameras)")
    # the distinct (point, camera) incidences, sorted by point then camera
    code = np.unique(pt * C + cam)
    pt, cam = code // C, code % C
    seen = np.bincount(cam, minlength=C)
    points, first, degree = np.unique(pt, return_index=True, return_counts=True)
    pair_codes = []
    for k in np.unique(degree):
        if k < 2:
            continue
        rows = first[degree == k][:, None] + np.arange(k)[None, :]
        cams_k = cam[rows]  # (points of degree k, k), ascending in a row
        a, b = np.triu_indices(k, 1)
        pair_codes.append((cams_k[:, a] * C + cams_k[:, b]).ravel())
    if not pair_codes:
        empty = np.empty(0, np.int64)
        return empty, empty, empty, seen
    pairs, shared = np.unique(np.concatenate(pair_codes), return_counts=True)
    return pairs // C, pairs % C, shared, seen


def visibility_edges(camera_index, point_index, num_cameras):
    """(i, j, w, seen): the visibility graph's edges i < j with their weights
    w_ij, and seen[c] = |V_c| (shared_points' pairs and counts)."""
    i, j, shared, seen = shared_points(camera_index, point_index, num_cameras)
    if not len(i):
        return i, j, np.empty(0, np.float64), seen
    w = shared / np.sqrt(seen[i].astype(np.float64) * seen[j])
    return i, j, w, seen


def relabel(labels):
    """The same partition with labels 0 .. k-1 in the order of each cluster's
    smallest member."""
    labels = np.asarray(labels)
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int32)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first), dtype=np.int32)
    return rank[inverse.ravel()]


def single_linkage(num_cameras, i, j, w, min_similarity=DEFAULT_MIN_SIMILARITY):
    """labels[c]: the connected components of the edges with w >= min_similarity
    (union-find with path halving)."""
    parent = np.arange(int(num_cameras), dtype=np.int64)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    keep = np.asarray(w) >= min_similarity
    for a, b in zip(np.asarray(i)[keep].tolist(), np.asarray(j)[keep].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return relabel(np.array([find(c) for c in range(int(num_cameras))], np.int64))


def cap_clusters(labels, max_cluster_cameras=_cse.SCHUR_MAX_CLUSTER_CAMERAS):
    """Cuts every cluster above the cap into runs of at most
    `max_cluster_cameras` cameras in camera order."""
    cap = int(max_cluster_cameras)
    if cap < 1:
        raise ValueError("max_cluster_cameras must be at least 1")
    labels = relabel(labels)
    # rank of a camera inside its cluster, in camera order
    order = np.argsort(labels, kind="stable")
    start = np.r_[0, np.cumsum(np.bincount(labels))[:-1]]
    rank = np.empty(len(labels), np.int64)
    rank[order] = np.arange(len(labels)) - start[labels[order]]
    return relabel(labels.astype(np.int64) * (len(labels) + 1) + rank // cap)


def blocks(num_cameras, max_cluster_cameras=_cse.SCHUR_MAX_CLUSTER_CAMERAS):
    """Consecutive runs of `max_cluster_cameras` cameras (not a reference
    clustering: for problems whose visibility carries no structure)."""
    cap = int(max_cluster_cameras)
    if cap < 1:
        raise ValueError("max_cluster_cameras must be at least 1")
    return (np.arange(int(num_cameras)) // cap).astype(np.int32)


DEFAULT_TRIDIAGONAL_CLUSTER_CAMERAS = _cse.SCHUR_MAX_CLUSTER_CAMERAS // 2  # two clusters of an edge fit the cap


def cluster_graph(camera_index, point_index, labels):
    """(g, h, w): the cluster graph of CLUSTER_TRIDIAGONAL, edges g < h in
    lexicographic order with w = the number of points seen from both clusters
    (the reference's ComputeClusterVisibility and CreateClusterGraph); only
    positive weights are edges."""
    labels = np.asarray(labels, np.int64)
    cam = np.asarray(camera_index, np.int64)
    if cam.size and (cam.min() < 0 or cam.max() >= labels.size):
        raise ValueError("a camera index outside the labels")
    # a cluster sees a point once, however many of its cameras do
    k = int(labels.max()) + 1 if labels.size else 0
    g, h, shared, _ = shared_points(labels[cam], point_index, k)
    return g, h, shared


def degree2_maximum_spanning_forest(num_clusters, g, h, w, sizes=None,
                                    max_edge_cameras=_cse.SCHUR_MAX_CLUSTER_CAMERAS):
    """The reference's Degree2MaximumSpanningForest (graph_algorithms.h): the
    edges (g, h), g < h, are taken greedily in descending (weight, (g, h))
    order -- its reverse sort of pair<weight, pair>, so equal weights go to the
    lexicographically larger pair first -- skipping an edge at a vertex that has
    two edges already and an edge inside one component.  Every tree of the
    result is a path.

    One rule is ours, not the reference's: with `sizes` (cameras per cluster)
    an edge whose two clusters hold more than `max_edge_cameras` cameras
    together is skipped too, since the device eliminates the two clusters of an
    edge in one workgroup's LDS.  Returns the kept edges, [k][2] int32, in the
    order they were taken."""
    n = int(num_clusters)
    g, h, w = np.asarray(g, np.int64), np.asarray(h, np.int64), np.asarray(w)
    lo, hi = np.minimum(g, h), np.maximum(g, h)
    order = np.lexsort((hi, lo, w))[::-1]
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    degree = [0] * n
    kept = []
    for k in order.tolist():
        a, b = int(lo[k]), int(hi[k])
        if a == b or degree[a] == 2 or degree[b] == 2:
            continue
        if sizes is not None and int(sizes[a]) + int(sizes[b]) > int(max_edge_cameras):
            continue
        ra, rb = find(a), find(b)
        if ra == rb:
            continue
        parent[max(ra, rb)] = min(ra, rb)
        degree[a] += 1
        degree[b] += 1
        kept.append((a, b))
    return np.array(kept, np.int32).reshape(-1, 2)


def forest_paths(num_clusters, edges):
    """The paths of a degree-2 forest as lists of labels: each from its end with
    the smaller label, ordered by first cluster (the order the device walks)."""
    nb = [[] for _ in range(int(num_clusters))]
    for a, b in np.asarray(edges, np.int64).reshape(-1, 2).tolist():
        nb[a].append(b)
        nb[b].append(a)
    seen, paths = set(), []
    for s in range(int(num_clusters)):
        if s in seen or len(nb[s]) == 2:
            continue
        path, prev, at = [], -1, s
        while at >= 0:
            path.append(at)
            seen.add(at)
            nxt = [x for x in nb[at] if x != prev]
            prev, at = at, (nxt[0] if nxt else -1)
        paths.append(path)
    if len(seen) != int(num_clusters):
        raise ValueError("the forest has a cycle")
    return paths


def cluster_cameras(camera_index, point_index, num_cameras, method="single_linkage",
                    min_similarity=DEFAULT_MIN_SIMILARITY,
                    max_cluster_cameras=_cse.SCHUR_MAX_CLUSTER_CAMERAS):
    """labels for Evaluator.schur_set_clusters: `single_linkage` (capped) or
    `blocks`."""
    if not 1 <= int(max_cluster_cameras) <= _cse.SCHUR_MAX_CLUSTER_CAMERAS:
        raise ValueError(f"max_cluster_cameras must be in [1, {_cse.SCHUR_MAX_CLUSTER_CAMERAS}]")
    if method == "blocks":
        return blocks(num_cameras, max_cluster_cameras)
    if method != "single_linkage":
        raise ValueError(f"unknown clustering method {method!r}")
    i, j, w, _ = visibility_edges(camera_index, point_index, num_cameras)
    return cap_clusters(single_linkage(num_cameras, i, j, w, min_similarity), max_cluster_cameras)
