"""PowerSeriesExpansionPreconditioner::RightMultiplyAndAccumulate
(internal/ceres/power_series_expansion_preconditioner.cc:51-72) restated in
numpy, statement for statement, for any float dtype (float64 and
np.longdouble): the reference of tests/test_schur_spse.py and
tests/test_schur_spse_gpu.py.

Dense inputs: Pinv, the block-diagonal (F^T F + D_f^2)^-1, and Q = P - S =
F^T E (E^T E + D_e^2)^-1 E^T F (F^T F is block diagonal here: every row of the
Jacobian has one camera).
"""
import collections

import numpy as np

Result = collections.namedtuple("Result", "y num_terms norms")  # norms[0] = |P^-1 x|, then each term's


def _norm(v):
    return np.sqrt(np.dot(v, v))


def block_diagonal(A, size=9):
    """The size x size diagonal blocks of A, everything else zero."""
    out = np.zeros_like(A)
    for k in range(0, A.shape[0], size):
        out[k:k + size, k:k + size] = A[k:k + size, k:k + size]
    return out


def operators(S, J, e_cols, D, dtype=np.longdouble):
    """(Pinv, Q) in `dtype` from the dense S: P = the diagonal blocks of
    F^T F + D_f^2 (F's columns alone: S's own diagonal blocks are
    SCHUR_JACOBI's), Q = P - S."""
    T = dtype
    F = np.asarray(J[:, e_cols:]).astype(T)
    f_cols = F.shape[1]
    P = np.zeros((f_cols, f_cols), T)
    Pinv = np.zeros((f_cols, f_cols), T)
    Df = np.asarray(D[e_cols:]).astype(T)
    for k in range(0, f_cols, 9):
        Fc = F[:, k:k + 9]
        P[k:k + 9, k:k + 9] = Fc.T @ Fc + np.diag(Df[k:k + 9] ** 2)
        # np.linalg.inv has no long double: float64's inverse, then one Newton
        # step X (2 I - P X) in T, which squares its relative error.
        X = np.linalg.inv(P[k:k + 9, k:k + 9].astype(np.float64)).astype(T)
        for _ in range(2):
            X = X @ (2 * np.eye(9, dtype=T) - P[k:k + 9, k:k + 9] @ X)
        Pinv[k:k + 9, k:k + 9] = X
    return Pinv, P - np.asarray(S).astype(T)


def series(Pinv, Q, x, max_num_iterations, tolerance, dtype=np.float64):
    T = dtype
    Pinv = np.asarray(Pinv).astype(T)
    Q = np.asarray(Q).astype(T)
    x = np.asarray(x).astype(T)
    y = Pinv @ x
    prev = y.copy()
    norms = [_norm(y)]
    threshold = T(tolerance) * norms[0]
    i = 1
    while True:
        term = Pinv @ (Q @ prev)
        y = y + term
        norms.append(_norm(term))
        if i >= max_num_iterations or norms[-1] < threshold:
            break
        prev = term
        i += 1
    return Result(y, i, norms)


def dense_preconditioner(Pinv, Q, m, dtype=np.float64):
    """M_m = sum_{i <= m} (P^-1 Q)^i P^-1: the series with m terms and
    tolerance 0 as a matrix."""
    T = dtype
    Pinv = np.asarray(Pinv).astype(T)
    G = Pinv @ np.asarray(Q).astype(T)
    term = Pinv.copy()
    M = Pinv.copy()
    for _ in range(m):
        term = G @ term
        M = M + term
    return M
