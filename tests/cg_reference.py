"""ConjugateGradientsSolver (internal/ceres/conjugate_gradients_solver.h:
108-305) restated in numpy, statement for statement, for any float dtype
(float64 and np.longdouble): the reference of tests/test_schur_solve.py and
tests/test_schur_solve_gpu.py.  Dense operator, dense preconditioner (M^-1 as
a matrix; None: IDENTITY).
"""
import collections

import numpy as np

SUCCESS, NO_CONVERGENCE, FAILURE = 0, 1, 2
(REASON_MAX_ITERATIONS, REASON_ZERO_RHS, REASON_INITIAL_RESIDUAL, REASON_RHO, REASON_BETA,
 REASON_INDEFINITE, REASON_ALPHA, REASON_Q_TOLERANCE, REASON_R_TOLERANCE) = range(9)

Result = collections.namedtuple(
    "Result", "x termination_type reason num_iterations norm_rhs norm_r q zeta rho pq")

Options = collections.namedtuple(
    "Options", "min_num_iterations max_num_iterations residual_reset_period r_tolerance q_tolerance",
    defaults=(1, 500, 10, -1.0, 0.0))


def _norm(v):
    return np.sqrt(np.dot(v, v))


def _zero_or_inf(v):
    return v == 0 or np.isinf(v)


def solve(A, b, x0, options=Options(), Minv=None, dtype=np.float64):
    """x0 None: the zero start (SetZero(solution) first, as
    IterativeSchurComplementSolver).  Returns a Result; x has `dtype`."""
    T = dtype
    o = options
    A = np.asarray(A).astype(T)
    b = np.asarray(b).astype(T)
    Minv = None if Minv is None else np.asarray(Minv).astype(T)
    x = np.zeros(b.shape, T) if x0 is None else np.asarray(x0).astype(T).copy()
    it, norm_r, Q1, zeta, rho, pq = 0, T(0), T(0), T(0), T(0), T(0)

    def result(ttype, reason):
        return Result(x, ttype, reason, it, norm_rhs, norm_r, Q1, zeta, rho, pq)

    norm_rhs = _norm(b)
    if norm_rhs == 0:
        x[:] = 0
        return result(SUCCESS, REASON_ZERO_RHS)
    tol_r = T(o.r_tolerance) * norm_rhs
    tmp = A @ x
    r = b - tmp
    norm_r = _norm(r)
    if o.min_num_iterations == 0 and norm_r <= tol_r:
        return result(SUCCESS, REASON_INITIAL_RESIDUAL)
    rho = T(1)
    Q0 = -np.dot(x, b + r)
    p = None
    with np.errstate(all="ignore"):
        it = 1
        while True:
            z = r.copy() if Minv is None else Minv @ r
            last_rho = rho
            rho = np.dot(r, z)
            if _zero_or_inf(rho):
                return result(FAILURE, REASON_RHO)
            if it == 1:
                p = z.copy()
            else:
                beta = rho / last_rho
                if _zero_or_inf(beta):
                    return result(FAILURE, REASON_BETA)
                p = z + beta * p
            q = A @ p
            pq = np.dot(p, q)
            if pq <= 0 or np.isinf(pq):
                return result(NO_CONVERGENCE, REASON_INDEFINITE)
            alpha = rho / pq
            if np.isinf(alpha):
                return result(FAILURE, REASON_ALPHA)
            x = x + alpha * p
            if it % o.residual_reset_period == 0:
                tmp = A @ x
                r = b - tmp
            else:
                r = r - alpha * q
            Q1 = -np.dot(x, b + r)
            zeta = T(it) * (Q1 - Q0) / Q1
            if zeta < T(o.q_tolerance) and it >= o.min_num_iterations:
                norm_r = _norm(r)
                return result(SUCCESS, REASON_Q_TOLERANCE)
            Q0 = Q1
            norm_r = _norm(r)
            if norm_r <= tol_r and it >= o.min_num_iterations:
                return result(SUCCESS, REASON_R_TOLERANCE)
            if it >= o.max_num_iterations:
                return result(NO_CONVERGENCE, REASON_MAX_ITERATIONS)
            it += 1
