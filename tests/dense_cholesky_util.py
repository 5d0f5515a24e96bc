"""Inputs, references and bounds of the dense Cholesky tests
(tests/test_dense_cholesky.py, tests/test_dense_cholesky_gpu.py).

The matrices are generated: spd(n, kappa, seed) = Q diag(logspace(0, log10
kappa, n)) Q^T, symmetrised, Q from the QR of a seeded normal matrix; the
right-hand sides are seeded normal vectors.

The bounds are Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3
and 10.4, which hold for any order of summation (so for the blocked order and
the matrix cores' order):
    |A - L L^T|  <= gamma_{n+1}  |L| |L^T|
    |b - A x|    <= gamma_{3n+1} |L| |L^T| |x|
with || |L| |L^T| || <= ||L||_F^2 ~ trace(A) and a factor 2 for the ~:
    factor:  ||A - L L^T||_F <= 2 (n + 1) u trace(A)
    solve:   ||b - A x||_2   <= 2 (3 n + 1) u trace(A) ||x||_2
u = 2^-53 in FP64.  For the FP32 factor and the unrefined FP32 solve u = 2^-24
and (3 n + 3) in place of (3 n + 1): the two extra units cover the casts of A
and of the right-hand side.  Residuals are evaluated in np.longdouble against
the lower triangle mirrored.
"""
import functools

import numpy as np

NB = 64  # kDenseCholeskyNB, the shipped panel width
SIZES = sorted({1, 15, 16, 17, 63, 64, 65, 129, 200, 441, 777, NB - 1, NB, NB + 1, 2 * NB + 1})
KAPPAS = (1e2, 1e4)
CASES = [(n, kappa) for n in SIZES for kappa in KAPPAS]
U64 = 2.0 ** -53
U32 = 2.0 ** -24


def case_seed(n, kappa):
    return 1000 * int(round(np.log10(kappa))) + n


@functools.lru_cache(maxsize=None)
def spd(n, kappa, seed=None):
    rng = np.random.default_rng(case_seed(n, kappa) if seed is None else seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0.0, np.log10(kappa), n)) @ Q.T
    A = 0.5 * (A + A.T)
    A.setflags(write=False)
    return A


def rhs(n, seed):
    return np.random.default_rng(50000 + 7 * n + seed).standard_normal(n)


def mirror_lower(A):
    """The symmetric matrix a lower triangle stands for."""
    L = np.tril(A)
    return L + np.tril(A, -1).T


def factor_bound(A, u):
    n = A.shape[0]
    return 2.0 * (n + 1) * u * float(np.trace(A))


def solve_bound(A, x, u, units=1):
    n = A.shape[0]
    return 2.0 * (3 * n + units) * u * float(np.trace(A)) * float(np.linalg.norm(x))


@functools.lru_cache(maxsize=None)
def _long(n, kappa):
    return mirror_lower(spd(n, kappa)).astype(np.longdouble)


def factor_error(n, kappa, L):
    """||A - L L^T||_F in longdouble; L's strict upper triangle is ignored."""
    Ll = np.tril(L).astype(np.longdouble)
    return float(np.linalg.norm(_long(n, kappa) - Ll @ Ll.T))


def solve_residual(n, kappa, b, x):
    """||b - A x||_2 in longdouble."""
    return float(np.linalg.norm(b.astype(np.longdouble) - _long(n, kappa) @ x.astype(np.longdouble)))


def cholesky_solve(L, b):
    """x = L^-T L^-1 b in L's precision by numpy's LAPACK."""
    b = b.astype(L.dtype)
    return np.linalg.solve(L.T, np.linalg.solve(L, b))
