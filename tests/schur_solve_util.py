"""Shared by tests/test_schur_solve.py (CPU) and tests/test_schur_solve_gpu.py:
the problems, preconditioners and option sets cse_schur_solve is compared with
tests/cg_reference.py on, and the dense operator and preconditioner of a case.

A case is (problem, preconditioner, option set); the GPU test runs each with
the implicit and the explicit operator.  Every problem has D (the "runs" and
"unobserved" problems need it: a point seen once, a camera never seen); see
damping() for its size.
"""
import collections
import functools

import numpy as np

import ceres_amd as ca
from ceres_amd import _cse, bal

import cg_reference as R
import schur_complement_util as U

WIDE = "wide"  # the 150-camera problem of tests/test_schur_sparse_gpu.py: 1,350 columns
PROBLEMS = ("bal", "runs", "unobserved", "duplicates", "quaternion", WIDE)
PRECONDITIONERS = (_cse.SCHUR_IDENTITY, _cse.SCHUR_JACOBI, _cse.SCHUR_SCHUR_JACOBI)

# name -> (cg_reference.Options, start): start "zero" = CSE_CG_ZERO_INITIAL_GUESS
# over a NaN pre-fill, "random" = a random initial guess without the flag.
OptionSet = collections.namedtuple("OptionSet", "options start identity_only")
OPTION_SETS = {
    # LevenbergMarquardtStrategy's setting (levenberg_marquardt_strategy.cc:98-103)
    "lm": OptionSet(R.Options(1, 50, 10, -1.0, 0.1), "zero", False),
    # the residual test with a reset every third iteration.  q_tolerance -1
    # switches the quadratic test off: once |r| / |b| is below 1e-8 the decrease
    # Q_i - Q_{i-1} is below Q's rounding, zeta's sign is noise, and a
    # q_tolerance of 0 ends the solve on it in either precision at random.
    "resets": OptionSet(R.Options(1, 200, 3, 1e-10, -1.0), "zero", True),
    # NO_CONVERGENCE after four iterations
    "max4": OptionSet(R.Options(1, 4, 10, 1e-10, -1.0), "zero", False),
    # a tolerance met in the first iterations, held back by min_num_iterations
    "min6": OptionSet(R.Options(6, 50, 10, 0.5, 0.0), "zero", False),
    # the initial product: r = rhs - S x0
    "guess": OptionSet(R.Options(1, 100, 10, 1e-6, 0.0), "random", False),
    # the same options from the zero start, x pre-filled with NaN
    "zero": OptionSet(R.Options(1, 100, 10, 1e-6, 0.0), "zero", False),
}

CASES = [(w, p, s) for w in PROBLEMS for p in PRECONDITIONERS for s, o in OPTION_SETS.items()
         if not (o.identity_only and p != _cse.SCHUR_IDENTITY)
         and not (w == "duplicates" and p == _cse.SCHUR_SCHUR_JACOBI)]


def make_program(which):
    if which == WIDE:
        return bal.synthetic_program((150, 2000, 8000), loss=ca.Loss.huber(1.0), seed=3)
    return U.make_program(which)


CAMERA_DAMPING = 0.1


CAMERA_DAMPING = 0.3


def damping(J, e_cols, seed=1):
    """D of cse_schur_init.  The points get U.damping's uniform(0.1, 2); the
    cameras get sqrt(0.3 max diag(F^T F)) uniform(0.8, 1.2), which holds the
    condition number of S near 5 whatever the cameras' column scales are.

    Why so much: conjugate gradients amplify a rounding error from iteration
    to iteration, the faster the better separated S's large eigenvalues are.
    Without camera damping S is the unscaled reduced camera matrix (condition
    1e7 to 1e8 here, where Ceres would have scaled the columns), and the
    float64 and np.longdouble references agree on neither the iteration count
    nor two digits of x.  At a factor of 0.1 (condition 8 to 17, 20 to 40
    IDENTITY iterations to 1e-10) their residuals still differ by a quarter at
    the 1e-10 threshold on "runs" and "unobserved", for every seed tried; at
    0.3 (17 to 25 iterations) they agree to five digits on every problem.  A
    parity test needs inputs on which the reference agrees with itself."""
    rng = np.random.default_rng(seed)
    D = rng.uniform(0.1, 2.0, J.shape[1])
    F = J[:, e_cols:]
    scale = np.sqrt(CAMERA_DAMPING * np.einsum("ij,ij->j", F, F).max())
    D[e_cols:] = scale * rng.uniform(0.8, 1.2, J.shape[1] - e_cols)
    return D


def right_hand_side(prog, seed=1):
    """b of cse_schur_init (num_residuals)."""
    return np.random.default_rng(seed).normal(size=prog.num_residuals)


def initial_guess(S, rhs):
    """A start with Q(x0) = x0' S x0 - 2 rhs' x0 < 0, as Q is at every iterate
    from zero: half the steepest-descent step along rhs, its entries perturbed
    by a tenth.  (From a start with Q > 0 zeta is negative at once and a
    q_tolerance of 0 ends the solve after one iteration.)"""
    t = 0.5 * (rhs @ rhs) / (rhs @ (S @ rhs))
    x0 = t * rhs * (1.0 + 0.1 * np.random.default_rng(4).normal(size=len(rhs)))
    assert x0 @ (S @ x0) - 2.0 * (rhs @ x0) < 0
    return x0


def reduced_rhs(prog, J, e_cols, D, b):
    """F^T (b - E (E^T E + D_e^2)^-1 E^T b), point by point (every row of J
    belongs to one point)."""
    rhs = np.zeros(J.shape[1] - e_cols)
    ccol, pcol, row0 = U.structure(prog)
    for p in np.unique(pcol):
        blocks = np.nonzero(pcol == p)[0]
        rows = np.stack([row0[blocks], row0[blocks] + 1], 1).ravel()
        Ep = J[rows, p:p + 3]
        M = np.linalg.inv(Ep.T @ Ep + np.diag(D[p:p + 3] ** 2))
        u = b[rows] - Ep @ (M @ (Ep.T @ b[rows]))
        for k, c in enumerate(ccol[blocks]):
            rhs[c - e_cols:c - e_cols + 9] += J[rows[2 * k:2 * k + 2], c:c + 9].T @ u[2 * k:2 * k + 2]
    return rhs


def dense_operator(prog, J, e_cols, D):
    """S in float64: U.schur_float64, or for the 150-camera problem (E^T E is
    6000 x 6000) U.schur_longdouble's point-by-point sum rounded to float64."""
    if J.shape[1] - e_cols > 1000:
        return U.schur_longdouble(prog, J, e_cols, D).astype(np.float64)
    return U.schur_float64(J, e_cols, D)[0]


def dense_preconditioner(precond, S, J, e_cols, D):
    """M^-1 as a dense matrix (None: IDENTITY), with test_schur_gpu's
    block_inverse."""
    from test_schur_gpu import block_inverse
    if precond == _cse.SCHUR_IDENTITY:
        return None
    if precond == _cse.SCHUR_SCHUR_JACOBI:
        return block_inverse(S, 9)
    f_cols = J.shape[1] - e_cols
    A = np.diag(D[e_cols:] ** 2)
    for k in range(0, f_cols, 9):  # the diagonal blocks of F^T F alone
        Fc = J[:, e_cols + k:e_cols + k + 9]
        A[k:k + 9, k:k + 9] += Fc.T @ Fc
    return block_inverse(A, 9)


Reference = collections.namedtuple("Reference", "f64 ld d_ref")


def reference(S, Minv, rhs, option_set):
    """cg_reference in float64 and in np.longdouble on the same float64 inputs;
    d_ref = |x_f64 - x_ld| / |x_ld|, what the arithmetic alone changes."""
    o = OPTION_SETS[option_set]
    x0 = initial_guess(S, rhs) if o.start == "random" else None
    f64 = R.solve(S, rhs, x0, o.options, Minv, np.float64)
    ld = R.solve(S, rhs, x0, o.options, Minv, np.longdouble)
    nx = np.linalg.norm(ld.x.astype(np.float64))
    d_ref = float(np.linalg.norm((f64.x - ld.x).astype(np.float64)) / nx) if nx > 0 else 0.0
    return Reference(f64, ld, d_ref)


def same_outcome(a, b):
    return (a.termination_type, a.reason, a.num_iterations) == (b.termination_type, b.reason,
                                                                 b.num_iterations)


@functools.lru_cache(maxsize=None)
def oracle_inputs(which):
    """(prog, J, e_cols, D, S, rhs) from the oracle's Jacobian, as
    tests/test_schur_complement.py gets it."""
    import oracle_py as O
    from test_spmv_gpu import dense_jacobian
    prog = make_program(which)
    op = O.OracleProgram.from_program(
        prog.with_explicit_manifolds(prog.state) if which == "quaternion" else prog)
    ok, _, _, _, jv = op.evaluate(prog.state)
    assert ok
    J = dense_jacobian(prog, jv)
    ccol, _, _ = U.structure(prog)
    e_cols = int(ccol.min())
    seed = 1
    D = damping(J, e_cols, seed)
    S = dense_operator(prog, J, e_cols, D)
    rhs = reduced_rhs(prog, J, e_cols, D, right_hand_side(prog, seed))
    return prog, J, e_cols, D, S, rhs
