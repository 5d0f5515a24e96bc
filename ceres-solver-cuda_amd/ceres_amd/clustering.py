"""Camera partitions for CLUSTER_JACOBI (Evaluator.schur_set_clusters), on the
host in numpy.

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

Canonical-views clustering, the reference's other choice, is not implemented.
"""
import numpy as np

from . import _cse

DEFAULT_MIN_SIMILARITY = 0.9  # the reference's single-linkage threshold


def visibility_edges(camera_index, point_index, num_cameras):
    """(i, j, w, seen): the visibility graph's edges i < j with their weights
    w_ij, and seen[c] = |V_c|.  A point observed by one camera several times
    counts once.  Work and memory are the sum over the points of k_p^2 for
    k_p cameras a point."""
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
        return empty, empty, np.empty(0, np.float64), seen
    pairs, shared = np.unique(np.concatenate(pair_codes), return_counts=True)
    i, j = pairs // C, pairs % C
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
