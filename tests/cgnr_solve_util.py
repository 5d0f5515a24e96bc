"""Shared by tests/test_cgnr_solve.py (CPU) and tests/test_cgnr_solve_gpu.py:
the problems, preconditioners and option sets cse_cgnr_solve is compared with
tests/cg_reference.py on, and the dense normal operator and block-Jacobi
preconditioner of a case.

A case is (problem, preconditioner, option set).  The problems are those of
tests/schur_solve_util.py plus "slices": about 4,560 columns, two full slices
of the vector kernels (2,048 entries each) and a ragged third.

D depends on the preconditioner (damping()): a parity test needs inputs on
which the reference agrees with itself, and what makes the normal equations
well conditioned differs with the preconditioner.
"""
import collections
import functools

import numpy as np

import ceres_amd as ca
from ceres_amd import _cse, bal

import schur_complement_util as U
import schur_solve_util as SU

SLICES = "slices"
PROBLEMS = ("bal", "runs", "unobserved", "duplicates", "quaternion", SLICES)
PRECONDITIONERS = (_cse.CGNR_IDENTITY, _cse.CGNR_JACOBI)
OPTION_SETS = SU.OPTION_SETS
SLICE_OPTION_SETS = ("lm", "resets", "zero")

# Every problem x both preconditioners x the option sets ("resets" with
# IDENTITY only); "slices" with lm / resets / zero.
CASES = [(w, p, s) for w in PROBLEMS for p in PRECONDITIONERS for s, o in OPTION_SETS.items()
         if not (o.identity_only and p != _cse.CGNR_IDENTITY)
         and not (w == SLICES and s not in SLICE_OPTION_SETS)]

DAMPING = 0.3


def make_program(which, format=ca.BLOCK_SPARSE):
    if which == SLICES:
        prog = bal.synthetic_program((40, 1400, 6000), loss=ca.Loss.huber(1.0), seed=17, format=format)
        n = prog.num_effective_parameters
        assert 2 * 2048 < n < 3 * 2048 and n % 2048 != 0, n  # two full slices and a ragged third
        return prog
    if which == "bal" and format != ca.BLOCK_SPARSE:
        return bal.synthetic_program((10, 300, 1500), loss=ca.Loss.huber(1.0), seed=9, format=format)
    assert format == ca.BLOCK_SPARSE
    return SU.make_program(which)


def blocks_of(prog):
    """[(delta_offset, tangent_size)] of the non-constant parameter blocks."""
    return sorted((int(prog.delta_offset[b]), int(prog.pb_tangent[b])) for b in range(prog.num_parameter_blocks)
                  if not prog.pb_constant[b] and prog.pb_tangent[b] > 0)


def camera_columns(prog):
    """The first camera column of a BAL-shaped program (points first)."""
    ccol, _, _ = U.structure(prog)
    return int(ccol.min())


def damping(J, e_cols, precond, seed=1):
    """D of cse_cgnr_init, from diag = the squared column norms of J:
    sqrt(0.3 max(diag)) uniform(0.8, 1.2), the maximum over all columns for
    IDENTITY and per class (points, cameras) for JACOBI.

    IDENTITY iterates on J^T J + D^2 itself, whose columns span many orders of
    magnitude (focal length against rotation): only damping by the largest
    column holds the condition number near 8.  JACOBI iterates on the
    block-scaled operator, so each class is damped by its own largest column
    (condition 4 to 5, 10 to 14 iterations); with that D and IDENTITY the
    condition number is 165 to 3,551 and the float64 and np.longdouble
    references stop on different iterations in half the cases, so that
    combination is no test input."""
    rng = np.random.default_rng(seed)
    diag = np.einsum("ij,ij->j", J, J)
    u = rng.uniform(0.8, 1.2, J.shape[1])
    if precond == _cse.CGNR_IDENTITY:
        return np.sqrt(DAMPING * diag.max()) * u
    D = np.empty(J.shape[1])
    D[:e_cols] = np.sqrt(DAMPING * diag[:e_cols].max()) * u[:e_cols]
    D[e_cols:] = np.sqrt(DAMPING * diag[e_cols:].max()) * u[e_cols:]
    return D


def dense_operator(J, D):
    A = J.T @ J
    if D is not None:
        A[np.diag_indices_from(A)] += D * D
    return A


def dense_block_inverse(A, blocks):
    """BlockCRSJacobiPreconditioner as a dense matrix: the inverse of every
    diagonal block of A."""
    M = np.zeros_like(A)
    for off, size in blocks:
        M[off:off + size, off:off + size] = np.linalg.inv(A[off:off + size, off:off + size])
    return M


def dense_preconditioner(precond, A, blocks):
    return None if precond == _cse.CGNR_IDENTITY else dense_block_inverse(A, blocks)


def initial_guess(A, rhs):
    return SU.initial_guess(A, rhs)


Reference = SU.Reference


def reference(A, Minv, rhs, option_set):
    return SU.reference(A, Minv, rhs, option_set)


same_outcome = SU.same_outcome


@functools.lru_cache(maxsize=None)
def oracle_jacobian(which):
    """(prog, J, e_cols, b) from the oracle's Jacobian."""
    import oracle_py as O
    from test_spmv_gpu import dense_jacobian
    prog = make_program(which)
    op = O.OracleProgram.from_program(
        prog.with_explicit_manifolds(prog.state) if which == "quaternion" else prog)
    ok, _, _, _, jv = op.evaluate(prog.state)
    assert ok
    J = dense_jacobian(prog, jv)
    return prog, J, camera_columns(prog), SU.right_hand_side(prog)


Inputs = collections.namedtuple("Inputs", "prog J e_cols D A Minv rhs")


def inputs_from(prog, J, e_cols, b, precond):
    D = damping(J, e_cols, precond)
    A = dense_operator(J, D)
    return Inputs(prog, J, e_cols, D, A, dense_preconditioner(precond, A, blocks_of(prog)), J.T @ b)


@functools.lru_cache(maxsize=None)
def oracle_inputs(which, precond):
    return inputs_from(*oracle_jacobian(which), precond)
