"""Shared by tests/test_schur_complement.py (CPU) and
tests/test_schur_complement_gpu.py: the problems the explicit Schur
complement (cse_schur_complement) is checked on, its numpy references and the
per-block error bound.

Per 9 x 9 block (c, c') the bound is
    1e-12 * || (|F|^T |F| + D_f^2 + |F^T E| |M| |E^T F|)_cc' ||_F ,
the magnitude of the terms that are summed into the block: a misplaced small
block cannot hide behind the norm of the whole matrix.
"""
import numpy as np

import ceres_amd as ca
from ceres_amd import bal

RTOL = 1e-12  # tests/test_schur_gpu.py's RTOL for S x

# which -> may run with d_D = NULL (no point seen by a single residual block)
CASES = [(w, d) for w in ("bal", "runs", "quaternion", "user", "duplicates", "unobserved")
         for d in (True, False) if d or w != "runs"]


def _program(C, cam_lists, seed):
    rng = np.random.default_rng(seed)
    P = len(cam_lists)
    cams, pts, _, _, _ = bal.synthetic(C, P, P, seed=seed)
    ci = np.concatenate([np.asarray(c) for c in cam_lists]).astype(np.int32)
    pi = np.repeat(np.arange(P, dtype=np.int32), [len(c) for c in cam_lists])
    obs = bal.project(cams, pts, ci, pi) + rng.normal(0, 1.0, (len(ci), 2))
    return bal.program(cams, pts, ci, pi, obs, loss=ca.Loss.huber(1.0))


def duplicates_problem(seed=5):
    """Points that see one camera in two and in three residual blocks (and at
    least two other cameras, so that E^T E is regular without D)."""
    rng = np.random.default_rng(seed)
    C, lists = 7, []
    for p in range(40):
        cams = list(rng.permutation(C)[:int(rng.integers(3, 6))])
        if p % 3 == 0:
            cams += [cams[0]]
        if p % 3 == 1:
            cams += [cams[1], cams[1]]
        lists.append([int(c) for c in rng.permutation(cams)])
    return _program(C, lists, seed)


def unobserved_problem(seed=6):
    """Camera 3 of 8 has no observation; every other camera has some."""
    rng = np.random.default_rng(seed)
    seen = np.array([0, 1, 2, 4, 5, 6, 7])
    lists = [[int(c) for c in rng.permutation(seen)[:int(rng.integers(2, 5))]] for _ in range(50)]
    lists[0], lists[1] = [0, 7, 1], [7, 0, 6]
    return _program(8, lists, seed)


def make_program(which):
    from test_schur_gpu import runs_problem, user_kind_program
    if which == "runs":
        return runs_problem()
    if which == "user":
        return user_kind_program()
    if which == "duplicates":
        return duplicates_problem()
    if which == "unobserved":
        return unobserved_problem()
    return bal.synthetic_program((10, 300, 1500), loss=ca.Loss.huber(1.0), seed=9,
                                 quaternion_manifold=which == "quaternion")


def damping(prog, with_D, seed=1):
    return np.random.default_rng(seed).uniform(0.1, 2.0, prog.num_effective_parameters) if with_D else None


def structure(prog):
    """(camera columns [n], point columns [n], first residual row [n]) per
    residual block, columns as delta offsets."""
    begin, ids = prog.block_params_csr()
    b = np.arange(prog.num_residual_blocks)
    cam, pt = ids[begin[b]], ids[begin[b] + 1]
    return (np.asarray(prog.delta_offset)[cam].astype(np.int64),
            np.asarray(prog.delta_offset)[pt].astype(np.int64),
            np.asarray(prog.residual_layout).astype(np.int64))


def covisible_blocks(prog, e_cols):
    """The brute-force set of (c, c') with c <= c' (camera indices in S) that
    share a point."""
    ccol, pcol, _ = structure(prog)
    cams = (ccol - e_cols) // 9
    out = set()
    for p in np.unique(pcol):
        cs = np.unique(cams[pcol == p])
        out.update((int(a), int(b)) for a in cs for b in cs if a <= b)
    return out


def schur_float64(J, e_cols, D):
    """tests/test_schur_gpu.py's dense_schur (D = None: no damping)."""
    E, F = J[:, :e_cols], J[:, e_cols:]
    D = np.zeros(J.shape[1]) if D is None else D
    Minv = np.linalg.inv(E.T @ E + np.diag(D[:e_cols] ** 2))
    return F.T @ F + np.diag(D[e_cols:] ** 2) - F.T @ E @ Minv @ E.T @ F, Minv


def _inverse3(A):
    c00 = A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]
    c01 = A[1, 2] * A[2, 0] - A[1, 0] * A[2, 2]
    c02 = A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]
    det = A[0, 0] * c00 + A[0, 1] * c01 + A[0, 2] * c02
    M = np.empty((3, 3), A.dtype)
    M[0, 0], M[0, 1], M[0, 2] = c00, c01, c02
    M[1, 1] = A[0, 0] * A[2, 2] - A[0, 2] * A[2, 0]
    M[1, 2] = A[0, 2] * A[1, 0] - A[0, 0] * A[1, 2]
    M[2, 2] = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
    M[1, 0], M[2, 0], M[2, 1] = M[0, 1], M[0, 2], M[1, 2]
    return M / det


def schur_longdouble(prog, J, e_cols, D):
    """The same S in np.longdouble, point by point:
    S = D_f^2 + sum_p F_p^T (I - E_p M_p E_p^T) F_p over the rows of p."""
    L = np.longdouble
    f_cols = J.shape[1] - e_cols
    S = np.zeros((f_cols, f_cols), L)
    if D is not None:
        S[np.diag_indices(f_cols)] = D[e_cols:].astype(L) ** 2
    ccol, pcol, row0 = structure(prog)
    for p in np.unique(pcol):
        blocks = np.nonzero(pcol == p)[0]
        rows = np.stack([row0[blocks], row0[blocks] + 1], 1).ravel()
        Ep = J[rows, p:p + 3].astype(L)
        A = Ep.T @ Ep
        if D is not None:
            A = A + np.diag(D[p:p + 3].astype(L) ** 2)
        W = np.eye(len(rows), dtype=L) - Ep @ _inverse3(A) @ Ep.T
        cols = (np.unique(ccol[blocks])[:, None] + np.arange(9)[None, :]).ravel()
        Fp = J[np.ix_(rows, cols)].astype(L)
        S[np.ix_(cols - e_cols, cols - e_cols)] += Fp.T @ W @ Fp
    return S


def block_norms(A):
    """Frobenius norm of every 9 x 9 block: (C, C)."""
    C = A.shape[0] // 9
    return np.sqrt((np.asarray(A, np.float64).reshape(C, 9, C, 9) ** 2).sum(axis=(1, 3)))


def block_bound(J, e_cols, D, Minv):
    """|| (|F|^T |F| + D_f^2 + |F^T E| |M| |E^T F|)_cc' ||_F per block."""
    E, F = J[:, :e_cols], J[:, e_cols:]
    FtE = np.abs(F.T @ E)
    B = np.abs(F).T @ np.abs(F) + FtE @ np.abs(Minv) @ FtE.T
    if D is not None:
        B = B + np.diag(D[e_cols:] ** 2)
    return block_norms(B)
