"""Inputs, restatements and bounds of the block-sparse Cholesky tests
(tests/test_sparse_cholesky.py, tests/test_sparse_cholesky_gpu.py).

matrix(C, pairs, seed): off-diagonal blocks are standard_normal((9, 9)) taken
in sorted pair order; then diagonal block c = G G^T / 9 + (1 + sum of ||B||_F
over the blocks of its block row and column) I, G standard_normal((9, 9)) in
camera order.  SPD by block diagonal dominance.

The bounds are dense_cholesky_util's (Higham, Thm 10.3 and 10.4) with n = 9 C
and u = 2^-53; they hold for any elimination and summation order, so for every
permutation and for the level order.  Residuals are evaluated in longdouble.

minimum_degree and fill restate the plan's rules with Python sets, sharing no
code with csrc/plan.cpp.
"""
import functools
import os
import subprocess
import tempfile

import numpy as np

from dense_cholesky_util import U64, factor_bound, solve_bound  # noqa: F401

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
B = 9
NATURAL, MINIMUM_DEGREE, GIVEN = 0, 1, 2
ORDERINGS = (NATURAL, MINIMUM_DEGREE, GIVEN)


def _band(C, w):
    return [(i, j) for i in range(C) for j in range(i + 1, min(C, i + w + 1))]


def _forest():
    """Three disjoint bands (half-width 2) of 7, 8 and 9 cameras, their indices
    interleaved round-robin."""
    sizes = (7, 8, 9)
    index = {}
    for m in range(max(sizes)):
        for b, size in enumerate(sizes):
            if m < size:
                index[(b, m)] = len(index)
    pairs = []
    for b, size in enumerate(sizes):
        for i, j in _band(size, 2):
            u, v = index[(b, i)], index[(b, j)]
            pairs.append((min(u, v), max(u, v)))
    return sorted(pairs)


def _random():
    rng = np.random.default_rng(1)
    return [(i, j) for i in range(57) for j in range(i + 1, 57) if rng.random() < 0.08]


# name -> (C, pairs)
SHAPES = {
    "one": (1, []),
    "two": (2, [(0, 1)]),
    "isolated": (5, []),
    "arrow-first": (12, [(0, k) for k in range(1, 12)]),
    "arrow-last": (12, [(k, 11) for k in range(11)]),
    "arrow-80": (80, [(0, k) for k in range(1, 80)]),
    "band": (40, _band(40, 3)),
    "forest": (24, _forest()),
    "pairs-300": (300, [(2 * i, 2 * i + 1) for i in range(150)]),
    "random": (60, _random()),
    "full": (20, _band(20, 20)),
}
FOREST_BAD = (3, 4)  # forest's camera 3 belongs to the band of 7, camera 4 to the band of 8: two trees
CASES = [(name, ordering) for name in SHAPES for ordering in ORDERINGS]


def case_id(case):
    return f"{case[0]}-{('natural', 'minimum_degree', 'given')[case[1]]}"


def structure(C, pairs):
    """Block-compressed rows of the upper triangle, the diagonal first."""
    rows = [[c] for c in range(C)]
    for i, j in sorted(pairs):
        assert 0 <= i < j < C
        rows[i].append(j)
    row_begin = np.zeros(C + 1, dtype=np.int64)
    row_begin[1:] = np.cumsum([len(r) for r in rows])
    block_col = np.array([c for r in rows for c in r], dtype=np.int32)
    return row_begin, block_col


@functools.lru_cache(maxsize=None)
def matrix(name, seed=0):
    """(row_begin, block_col, values [blocks][9][9], dense A), read-only."""
    C, pairs = SHAPES[name]
    pairs = sorted(pairs)
    rng = np.random.default_rng(seed)
    off = {p: rng.standard_normal((B, B)) for p in pairs}
    weight = np.ones(C)
    for (i, j), blk in off.items():
        f = np.linalg.norm(blk)
        weight[i] += f
        weight[j] += f
    row_begin, block_col = structure(C, pairs)
    values = np.zeros((len(block_col), B, B))
    A = np.zeros((B * C, B * C))
    for c in range(C):
        G = rng.standard_normal((B, B))
        values[row_begin[c]] = G @ G.T / 9.0 + weight[c] * np.eye(B)
        values[row_begin[c]] = 0.5 * (values[row_begin[c]] + values[row_begin[c]].T)
    for r in range(C):
        for k in range(row_begin[r], row_begin[r + 1]):
            c = block_col[k]
            if c != r:
                values[k] = off[(r, c)]
            A[B * r:B * r + B, B * c:B * c + B] = values[k]
            A[B * c:B * c + B, B * r:B * r + B] = values[k].T
    for a in (row_begin, block_col, values, A):
        a.setflags(write=False)
    return row_begin, block_col, values, A


def rhs(name, seed=0):
    C = SHAPES[name][0]
    return np.random.default_rng(70000 + 13 * C + seed).standard_normal(B * C)


def given_order(name):
    """GIVEN's order in every test: the reversed one."""
    C = SHAPES[name][0]
    return np.arange(C - 1, -1, -1, dtype=np.int32)


def minimum_degree(C, pairs):
    """The greedy rule: the camera with the fewest uneliminated neighbours in
    the elimination graph, fill included, lowest index on ties; once what
    remains is a clique the rest follows in index order."""
    adj = [set() for _ in range(C)]
    for i, j in pairs:
        adj[i].add(j)
        adj[j].add(i)
    alive = set(range(C))
    order = []
    while alive:
        v = min(alive, key=lambda u: (len(adj[u]), u))
        if len(adj[v]) == len(alive) - 1:
            order += sorted(alive)
            break
        order.append(v)
        alive.remove(v)
        for u in adj[v]:
            adj[u] |= adj[v]
            adj[u] -= {u, v}
    return np.array(order, dtype=np.int32)


def expected_order(name, ordering):
    C, pairs = SHAPES[name]
    if ordering == NATURAL:
        return np.arange(C, dtype=np.int32)
    if ordering == MINIMUM_DEGREE:
        return minimum_degree(C, pairs)
    return given_order(name)


def fill(C, pairs, order):
    """The elimination game on the permuted graph: (factor_row_begin,
    factor_block_col, parent) of L, a row's columns ascending, the diagonal last."""
    pos = np.empty(C, dtype=np.int64)
    pos[np.asarray(order)] = np.arange(C)
    adj = [set() for _ in range(C)]
    for i, j in pairs:
        adj[pos[i]].add(int(pos[j]))
        adj[pos[j]].add(int(pos[i]))
    rows = [[] for _ in range(C)]
    parent = np.full(C, -1, dtype=np.int32)
    for j in range(C):
        higher = sorted(i for i in adj[j] if i > j)
        for i in higher:
            rows[i].append(j)
            adj[i] |= set(higher) - {i}
        if higher:
            parent[j] = higher[0]
    for i in range(C):
        rows[i].append(i)
    row_begin = np.zeros(C + 1, dtype=np.int64)
    row_begin[1:] = np.cumsum([len(r) for r in rows])
    return row_begin, np.array([c for r in rows for c in r], dtype=np.int32), parent


def levels(parent):
    level = np.zeros(len(parent), dtype=np.int32)
    for j, p in enumerate(parent):  # children come before their parent
        if p >= 0:
            level[p] = max(level[p], level[j] + 1)
    return level


def block_products(row_begin, block_col):
    C = len(row_begin) - 1
    m = np.bincount(block_col, minlength=C) - 1  # blocks of each column below its diagonal
    return int(np.sum(m * (m + 1) // 2))


def dense_factor(row_begin, block_col, L_values):
    """The dense lower-triangular matrix L's blocks stand for."""
    C = len(row_begin) - 1
    L = np.zeros((B * C, B * C))
    for i in range(C):
        for k in range(row_begin[i], row_begin[i + 1]):
            j = block_col[k]
            L[B * i:B * i + B, B * j:B * j + B] = L_values[k]
    return L


def permuted(A, order):
    idx = (B * np.asarray(order, dtype=np.int64)[:, None] + np.arange(B)[None, :]).ravel()
    return A[np.ix_(idx, idx)]


def factor_error(A, order, L):
    """||P A P^T - L L^T||_F in longdouble, L dense.  numpy has no fast
    longdouble product, so L L^T is taken column by column over L's non-zero
    blocks alone (every product of two blocks of one block column)."""
    C = L.shape[0] // B
    blocks = L.reshape(C, B, C, B).transpose(0, 2, 1, 3)
    nonzero = np.abs(blocks).max(axis=(2, 3)) > 0
    R = permuted(A, order).astype(np.longdouble)
    for j in range(C):
        rows = np.flatnonzero(nonzero[:, j])
        if len(rows) == 0:
            continue
        Lc = blocks[rows, j].astype(np.longdouble)
        idx = (B * rows[:, None] + np.arange(B)[None, :]).ravel()
        R[np.ix_(idx, idx)] -= np.einsum("aik,bjk->aibj", Lc, Lc).reshape(len(idx), len(idx))
    return float(np.linalg.norm(R))


def solve_residual(A, b, x):
    """||b - A x||_2 in longdouble."""
    return float(np.linalg.norm(b.astype(np.longdouble) - A.astype(np.longdouble) @ x.astype(np.longdouble)))


def build_driver():
    subprocess.run(["make", "-C", CPP, "-f", "sparse_cholesky.mk", "driver"], check=True, capture_output=True)
    return os.path.join(CPP, "build", "sparse_cholesky_driver")


def run_driver(row_begin, block_col, ordering, given=None, values=None, b=None):
    """The CPU driver on one case: a dict of its output lines (ints as int64
    arrays, L and x as float64 arrays), 'rc' and 'error' always."""
    exe = build_driver()
    C = len(row_begin) - 1
    with tempfile.NamedTemporaryFile("w", suffix=".case", delete=False) as f:
        f.write(f"{C} {ordering}\n")
        f.write(" ".join(str(int(v)) for v in row_begin) + "\n")
        f.write(" ".join(str(int(v)) for v in block_col) + "\n")
        if ordering == GIVEN:
            f.write(" ".join(str(int(v)) for v in given) + "\n")
        if values is None:
            f.write("0\n")
        else:
            f.write("1\n")
            f.write(" ".join(float(v).hex() for v in np.asarray(values).ravel()) + "\n")
            f.write(" ".join(float(v).hex() for v in np.asarray(b).ravel()) + "\n")
        path = f.name
    try:
        run = subprocess.run([exe, path], capture_output=True, text=True)
    finally:
        os.unlink(path)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    out = {"error": ""}
    for line in run.stdout.splitlines():
        key, _, rest = line.partition(" ")
        if key == "error":
            out[key] = rest
        elif key in ("L", "x"):
            out[key] = np.array([float.fromhex(t) for t in rest.split()])
        elif key in ("rc", "info"):
            out[key] = int(rest)
        else:
            out[key] = np.array([int(t) for t in rest.split()], dtype=np.int64)
    return out


@functools.lru_cache(maxsize=None)
def driver_case(name, ordering):
    row_begin, block_col, values, _ = matrix(name)
    given = given_order(name) if ordering == GIVEN else None
    return run_driver(row_begin, block_col, ordering, given, values, rhs(name))
