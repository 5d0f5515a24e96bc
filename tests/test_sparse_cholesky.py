"""CPU: the block-sparse Cholesky factorization's boundary
(cse_sparse_cholesky_*), its host plan, the driver's flags and the bounds the
GPU tests hold the device to.

The plan (cse::PlanSparseCholesky) runs in tests/cpp/sparse_cholesky_driver.cpp
under ASan + UBSan; its permutation, L's structure, the elimination tree, the
levels and the product count are compared with restatements in Python sets
(sparse_cholesky_util.minimum_degree, fill) that share no code with it.  The
driver also replays the numeric factorization and the solve on the host through
the plan's tables; the replay meets Higham's bounds, and numpy's Cholesky of
P A P^T meets a tenth of them on the same inputs, every shape and ordering
(largest shares: factor 0.0145, solve 0.0020, on the one-block shape), which
pins the bounds independently of the device.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import sparse_cholesky_util as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "cse.h")

SYMBOLS = ("cse_sparse_cholesky_analyze", "cse_sparse_cholesky_structure", "cse_sparse_cholesky_factorize",
           "cse_sparse_cholesky_factor_values", "cse_sparse_cholesky_solve", "cse_sparse_cholesky_info")
CSE_ERR_INVALID = -1


def test_symbols_exported_and_wrapped():
    from ceres_amd import _cse
    C = ctypes
    lib = C.CDLL(_cse.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    S = _cse.SIGNATURES
    assert S["cse_sparse_cholesky_analyze"] == (C.c_int, [C.c_void_p, C.c_int64, _cse.P_i64, _cse.P_i32, C.c_int32,
                                                          _cse.P_i32, C.POINTER(_cse.cse_sparse_cholesky_summary)])
    assert S["cse_sparse_cholesky_structure"] == (C.c_int, [C.c_void_p, _cse.P_i32, _cse.P_i64, _cse.P_i32,
                                                            _cse.P_i32, _cse.P_i32])
    assert S["cse_sparse_cholesky_factorize"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert S["cse_sparse_cholesky_factor_values"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert S["cse_sparse_cholesky_solve"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32])
    assert S["cse_sparse_cholesky_info"] == (C.c_int, [C.c_void_p, _cse.P_i32])
    assert (_cse.SPARSE_ORDERING_NATURAL, _cse.SPARSE_ORDERING_MINIMUM_DEGREE, _cse.SPARSE_ORDERING_GIVEN) == (0, 1, 2)
    assert _cse.CSE_ERR_INVALID == CSE_ERR_INVALID
    fields = [(n, t) for n, t in _cse.cse_sparse_cholesky_summary._fields_]
    assert fields == [("num_block_rows", C.c_int64), ("num_input_blocks", C.c_int64),
                      ("num_factor_blocks", C.c_int64), ("num_block_products", C.c_int64),
                      ("device_bytes", C.c_int64), ("num_levels", C.c_int32), ("max_level_columns", C.c_int32)]
    # no evaluator: the calls' own null check
    L = _cse.lib()
    assert L.cse_sparse_cholesky_analyze(None, 1, None, None, 0, None, None) == CSE_ERR_INVALID
    assert L.cse_sparse_cholesky_structure(None, None, None, None, None, None) == CSE_ERR_INVALID
    assert L.cse_sparse_cholesky_factorize(None, None) == CSE_ERR_INVALID
    assert L.cse_sparse_cholesky_factor_values(None, None) == CSE_ERR_INVALID
    assert L.cse_sparse_cholesky_solve(None, None, None, 0) == CSE_ERR_INVALID
    assert L.cse_sparse_cholesky_info(None, None) == CSE_ERR_INVALID


def test_evaluator_methods():
    import ceres_amd as ca
    from ceres_amd import _cse
    sig = inspect.signature(ca.Evaluator.sparse_cholesky_analyze)
    assert list(sig.parameters) == ["self", "row_begin", "block_col", "ordering", "permutation"]
    assert sig.parameters["ordering"].default == _cse.SPARSE_ORDERING_MINIMUM_DEGREE
    assert sig.parameters["permutation"].default is None
    assert list(inspect.signature(ca.Evaluator.sparse_cholesky_structure).parameters) == ["self"]
    assert list(inspect.signature(ca.Evaluator.sparse_cholesky_factorize_device).parameters) == ["self", "d_values"]
    assert list(inspect.signature(ca.Evaluator.sparse_cholesky_factor_values_device).parameters) == ["self", "d_L"]
    sig = inspect.signature(ca.Evaluator.sparse_cholesky_solve_device)
    assert list(sig.parameters) == ["self", "d_rhs", "d_x", "max_num_refinement_iterations"]
    assert sig.parameters["max_num_refinement_iterations"].default == 0
    assert list(inspect.signature(ca.Evaluator.sparse_cholesky_info).parameters) == ["self"]


def test_header_lines():
    text = open(HEADER).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("enum { CSE_SPARSE_ORDERING_NATURAL = 0, CSE_SPARSE_ORDERING_MINIMUM_DEGREE = 1, "
            "CSE_SPARSE_ORDERING_GIVEN = 2 };") in flat
    assert ("typedef struct cse_sparse_cholesky_summary { int64_t num_block_rows, num_input_blocks, "
            "num_factor_blocks, num_block_products; int64_t device_bytes;") in flat
    assert "int32_t num_levels, max_level_columns; } cse_sparse_cholesky_summary;" in flat
    assert ("int cse_sparse_cholesky_analyze(cse_evaluator* ev, int64_t num_block_rows, const int64_t* row_begin, "
            "const int32_t* block_col, int32_t ordering, const int32_t* permutation, "
            "cse_sparse_cholesky_summary* summary);") in flat
    assert ("int cse_sparse_cholesky_structure(cse_evaluator* ev, int32_t* permutation, int64_t* factor_row_begin, "
            "int32_t* factor_block_col, int32_t* parent, int32_t* level);") in flat
    assert "int cse_sparse_cholesky_factorize(cse_evaluator* ev, const double* d_values);" in flat
    assert "int cse_sparse_cholesky_factor_values(cse_evaluator* ev, double* d_L);" in flat
    assert ("int cse_sparse_cholesky_solve(cse_evaluator* ev, const double* d_rhs, double* d_x, "
            "int32_t max_num_refinement_iterations);") in flat
    assert "int cse_sparse_cholesky_info(cse_evaluator* ev, int32_t* info);" in flat
    # the reference lines the section replaces
    for ref in ("schur_complement_solver.cc:290-333", "sparse_cholesky.h:72-113", "sparse_cholesky.h:55-56",
                "sparse_cholesky.h:119"):
        assert ref in text, ref


def test_abi_version_is_still_6():
    from ceres_amd import _cse
    assert re.search(r"#define CSE_ABI_VERSION 6\b", open(HEADER).read())
    assert _cse.CSE_ABI_VERSION == 6
    assert _cse.lib().cse_abi_version() == 6


def test_nonfinite_flags_for_the_translation_unit():
    text = open(os.path.join(REPO, "ceres-solver-cuda_amd", "Makefile")).read()
    assert "sparse_cholesky" in re.search(r"^NONFINITE_TUS := (.*)$", text, re.M).group(1).split()


def test_exact_factor_block_counts():
    """The issue's table: the arrow fills completely when its hub goes first
    and not at all when it goes last; a band and the full matrix do not fill."""
    def count(name, order):
        C, pairs = U.SHAPES[name]
        return len(U.fill(C, pairs, order)[1])
    assert count("arrow-first", np.arange(12)) == 78 == 12 * 13 // 2
    assert count("arrow-last", np.arange(12)) == 23 == 2 * 12 - 1
    assert count("band", np.arange(40)) == 154
    assert count("full", np.arange(20)) == 210
    for name, want in (("arrow-first", 78), ("arrow-last", 23), ("band", 154), ("full", 210)):
        out = U.driver_case(name, U.NATURAL)
        assert out["summary"][2] == want == len(out["block_col"])


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_plan_equals_the_restatement(case):
    name, ordering = case
    C, pairs = U.SHAPES[name]
    out = U.driver_case(name, ordering)
    assert out["rc"] == 0, out["error"]
    order = U.expected_order(name, ordering)
    np.testing.assert_array_equal(out["permutation"], order)
    row_begin, block_col, parent = U.fill(C, pairs, order)
    np.testing.assert_array_equal(out["row_begin"], row_begin)
    np.testing.assert_array_equal(out["block_col"], block_col)
    np.testing.assert_array_equal(out["parent"], parent)
    level = U.levels(parent)
    np.testing.assert_array_equal(out["level"], level)
    # every column a column reads lies on a lower level
    for i in range(C):
        for k in range(row_begin[i], row_begin[i + 1] - 1):
            assert level[block_col[k]] < level[i]
    n_in = len(pairs) + C
    summary = out["summary"]
    assert list(summary[:4]) == [C, n_in, len(block_col), U.block_products(row_begin, block_col)]
    assert summary[5] == level.max() + 1
    assert summary[6] == np.bincount(level).max()
    # the tables: rows of the blocks, the column index, scatter and its inverse, the level lists
    np.testing.assert_array_equal(out["block_row"], np.repeat(np.arange(C), np.diff(row_begin)))
    col_block = out["col_block"]
    assert sorted(col_block) == [k for k in range(len(block_col)) if out["block_row"][k] != block_col[k]]
    for j in range(C):
        mine = col_block[out["col_begin"][j]:out["col_begin"][j + 1]]
        assert all(block_col[k] == j for k in mine)
        assert list(out["block_row"][mine]) == sorted(out["block_row"][mine])
    pos = np.argsort(order)
    in_row_begin, in_block_col = U.structure(C, pairs)
    for r in range(C):
        for k in range(in_row_begin[r], in_row_begin[r + 1]):
            p, q = pos[r], pos[in_block_col[k]]
            s = int(out["scatter"][k])  # block t as it is, or ~t: transposed
            t, transposed = (~s, True) if s < 0 else (s, False)
            assert (out["block_row"][t], block_col[t]) == (max(p, q), min(p, q))
            assert transposed == (p < q)
            assert out["source"][t] == (-2 - k if transposed else k)
    assert np.count_nonzero(out["source"] == -1) == len(block_col) - n_in
    for l in range(int(summary[5])):
        cols = out["level_columns"][out["level_begin"][l]:out["level_begin"][l + 1]]
        assert list(cols) == [j for j in range(C) if level[j] == l]
        targets = out["level_targets"][out["target_begin"][l]:out["target_begin"][l + 1]]
        assert sorted(targets) == sorted(k for k in col_block if level[block_col[k]] == l)


def test_minimum_degree_moves_the_hub_behind_the_leaves_and_keeps_a_clique_in_order():
    # leaves 1 .. 10 go first; the hub and the last leaf are then a clique of two: index order
    assert list(U.driver_case("arrow-first", U.MINIMUM_DEGREE)["permutation"]) == list(range(1, 11)) + [0, 11]
    assert list(U.driver_case("full", U.MINIMUM_DEGREE)["permutation"]) == list(range(20))
    assert U.driver_case("arrow-first", U.MINIMUM_DEGREE)["summary"][2] == 23


@pytest.mark.parametrize("case", U.CASES, ids=U.case_id)
def test_replay_and_numpy_reference_against_the_bounds(case):
    name, ordering = case
    _, _, _, A = U.matrix(name)
    b = U.rhs(name)
    out = U.driver_case(name, ordering)
    order = out["permutation"]
    assert out["info"] == 0
    L = U.dense_factor(out["row_begin"], out["block_col"], out["L"].reshape(-1, U.B, U.B))
    assert np.array_equal(L, np.tril(L))
    x = out["x"]
    fb, sb = U.factor_bound(A, U.U64), U.solve_bound(A, x, U.U64)
    f = U.factor_error(A, order, L) / fb
    s = U.solve_residual(A, b, x) / sb
    print(f"{U.case_id(case)} replay: factor {f:.4f} solve {s:.4f} of the bound")
    assert f <= 1.0 and s <= 1.0
    # numpy's LAPACK on P A P^T: a tenth of the same bounds
    PA = U.permuted(A, order)
    Ln = np.linalg.cholesky(PA)
    idx = (U.B * np.asarray(order)[:, None] + np.arange(U.B)[None, :]).ravel()
    xn = np.empty_like(b)
    xn[idx] = np.linalg.solve(Ln.T, np.linalg.solve(Ln, b[idx]))
    f = U.factor_error(A, order, Ln) / fb
    s = U.solve_residual(A, b, xn) / U.solve_bound(A, xn, U.U64)
    print(f"{U.case_id(case)} numpy: factor {f:.4f} solve {s:.4f} of the bound")
    assert f <= 0.1 and s <= 0.1


def test_replay_reports_the_first_failed_column():
    """Diagonal block c = -I: 9 pos(c) + 1, whatever the order."""
    name = "forest"
    row_begin, block_col, values, _ = U.matrix(name)
    bad = values.copy()
    bad[row_begin[U.FOREST_BAD[0]]] = -np.eye(U.B)
    bad[row_begin[U.FOREST_BAD[1]]] = -np.eye(U.B)
    for ordering in U.ORDERINGS:
        given = U.given_order(name) if ordering == U.GIVEN else None
        out = U.run_driver(row_begin, block_col, ordering, given, bad, U.rhs(name))
        pos = np.argsort(out["permutation"])
        assert out["info"] == 9 * min(pos[U.FOREST_BAD[0]], pos[U.FOREST_BAD[1]]) + 1
        assert not out["x"].any()


INVALID = {
    "row_begin does not start at 0": ([1, 2, 3], [0, 1, 1], U.NATURAL, None),
    "missing diagonal": ([0, 2, 3], [1, 1, 1], U.NATURAL, None),
    "empty row": ([0, 2, 2], [0, 1], U.NATURAL, None),
    "diagonal not first": ([0, 2, 3, 4], [1, 0, 1, 2], U.NATURAL, None),
    "columns descend": ([0, 3, 4, 5], [0, 2, 1, 1, 2], U.NATURAL, None),
    "column repeats": ([0, 3, 4, 5], [0, 1, 1, 1, 2], U.NATURAL, None),
    "column out of range": ([0, 2, 3], [0, 2, 1], U.NATURAL, None),
    "unknown ordering": ([0, 1, 2], [0, 1], 3, None),
    "negative ordering": ([0, 1, 2], [0, 1], -1, None),
    "given repeats": ([0, 1, 2], [0, 1], U.GIVEN, [0, 0]),
    "given out of range": ([0, 1, 2], [0, 1], U.GIVEN, [0, 2]),
    "given negative": ([0, 1, 2], [0, 1], U.GIVEN, [-1, 0]),
}


@pytest.mark.parametrize("what", sorted(INVALID))
def test_invalid_structures_are_refused(what):
    row_begin, block_col, ordering, given = INVALID[what]
    out = U.run_driver(np.array(row_begin), np.array(block_col), ordering, given)
    assert out["rc"] == CSE_ERR_INVALID, what
    assert "sparse Cholesky" in out["error"]


def test_driver_flags():
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", "problem-16-22106", "--linear_solver", "sparse_schur"]
    args = bundle_adjuster.parse(base)
    assert args.linear_solver == "sparse_schur"
    assert args.sparse_ordering == "minimum_degree"
    assert args.max_num_refinement_iterations == 0
    args = bundle_adjuster.parse(base + ["--sparse_ordering", "natural", "--max_num_refinement_iterations", "2"])
    assert args.sparse_ordering == "natural"
    assert args.max_num_refinement_iterations == 2
    # the defaults of the other solvers are unchanged
    args = bundle_adjuster.parse(["--synthetic", "problem-16-22106"])
    assert (args.linear_solver, args.dense_linear_algebra_library, args.preconditioner) == \
        ("iterative_schur", "torch", "jacobi")
    refusals = [
        (["--held_cameras", "2"], "--held_cameras needs --linear_solver iterative_schur or cgnr, not sparse_schur"),
        (["--dense_linear_algebra_library", "cse"], "needs --linear_solver dense_schur, not sparse_schur"),
        (["--mixed_precision_solves"], "--mixed_precision_solves needs"),
        (["--use_explicit_schur_complement"], "--use_explicit_schur_complement needs --linear_solver iterative_schur"),
        (["--preconditioner", "schur_jacobi"], "--preconditioner schur_jacobi needs --linear_solver iterative_schur"),
        (["--preconditioner", "cluster_tridiagonal"], "needs --linear_solver iterative_schur"),
        (["--use_spse_initialization"], "--use_spse_initialization needs --linear_solver iterative_schur"),
        (["--device_pcg"], "--device_pcg needs --linear_solver iterative_schur"),
        (["--device_cgnr"], "--device_cgnr needs --linear_solver cgnr"),
        (["--max_num_refinement_iterations", "-1"], "must not be negative"),
    ]
    for extra, message in refusals:
        with pytest.raises(SystemExit, match=re.escape(message)):
            bundle_adjuster.parse(base + extra)
    with pytest.raises(SystemExit):
        bundle_adjuster.parse(base + ["--sparse_ordering", "amd"])
