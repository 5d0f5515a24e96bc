"""GPU: cse_jacobian_squared_column_norm and cse_jacobian_scale_columns
(SparseMatrix::SquaredColumnNorm / ScaleColumns, sparse_matrix.h:81-87) on the
values the evaluator wrote, and the driver's --jacobi_scaling.

The reference of every check is the dense reconstruction of J from the layout
tables (tests/test_spmv_gpu.py::dense_jacobian), in numpy on the host.

Norm: per column math.fsum of the squared entries; the bound
    |got - ref| <= 1.01 (terms + 2) 2^-53 ref,   terms = stored entries of the column,
is the forward error of a sum of non-negative terms in any order (terms - 1
additions and one rounding per square, against a reference that rounds each
square and its exact sum once), so nothing in it is tuned.  The output is
prefilled with NaN: an entry that is not assigned fails.  On the affine path
two calls are bit-identical.

Scale: a random vector in [0.5, 2]; every stored value must be exactly
value * scale[column] (np.array_equal on the dense J and on the whole buffer,
whose values outside every cell and whose 64-double tail must not change), at
a 16-byte aligned base and at one shifted by 8 bytes.  The norm of the scaled
values equals scale^2 norm within the bound above plus 3 ulp (one rounding in
each scaled value, squared, and two in scale^2 ref).
"""
import dataclasses
import math

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import bal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U53 = 2.0 ** -53
SENTINEL = -7.25e77


def _bal(counts, fmt, **kw):
    return bal.synthetic_program(counts, loss=ca.Loss.huber(1.0), format=fmt, seed=counts[2], **kw)


def _mini_ba(fmt):
    from test_parity_gpu import mini_ba
    return mini_ba(fmt)


def _held(fmt):
    from test_constant_gpu import held
    return held(const=(0, 6), loss=ca.Loss.huber(1.0), fmt=fmt, seed=12)


def _quaternion(fmt):
    from test_manifold_gpu import quat_program
    return quat_program(counts=(16, 300, 1300), loss=ca.Loss.huber(1.0), fmt=fmt)


def _bundler(fmt):
    import user_functors as U
    prog = _bal((12, 400, 1600), fmt)
    prog.groups = [dataclasses.replace(g, kind=U.kind("BundlerResidual/Huber")) for g in prog.groups]
    return prog


def _pose(fmt):
    from test_user_functor_gpu import _pose_point_problem
    pb, n_elim = _pose_point_problem("PoseReprojectionError/Huber", C=13, P=211, per_point=5)
    prog = pb.program()
    prog.compile(fmt, num_eliminate_blocks=n_elim if fmt == ca.BLOCK_SPARSE else 0)
    return prog


def _three_cameras(fmt):
    # 3 cameras, 300 points, 1800 observations: 600 blocks per camera, more
    # than kGradChunk = 512, so every camera has two chunks.  The generator
    # gives a point at most one observation per camera, so each of its 900
    # observations is taken twice (a second, shifted measurement), point-major.
    cams, pts, ci, pi, obs = bal.synthetic(3, 300, 900, seed=1800)
    ci, pi = np.repeat(ci, 2), np.repeat(pi, 2)
    obs = np.repeat(obs, 2, axis=0)
    obs[1::2] += 0.5
    prog = bal.program(cams, pts, ci, pi, obs, loss=ca.Loss.huber(1.0), format=fmt)
    assert prog.num_residual_blocks == 1800 and np.all(np.bincount(ci) > 512)
    return prog


def _unobserved(fmt):
    # Five observed cameras and a sixth that no block sees.
    cams, pts, ci, pi, obs = bal.synthetic(5, 150, 700, seed=31)
    cams = np.concatenate([cams, cams[:1]])
    return bal.program(cams, pts, ci, pi, obs, loss=ca.Loss.huber(1.0), format=fmt)


# name -> (builder, Evaluator options, every group on the affine path without held cameras)
CASES = {
    "one_chunk_plus_one": (lambda f: _bal((5, 21, 65), f), {}, True),
    "12_400_1600": (lambda f: _bal((12, 400, 1600), f), {}, True),
    "long_point_runs": (lambda f: _bal((210, 20, 4097), f), {}, True),
    "ordered_chunk_reduce": (_three_cameras, {}, True),
    "general_layout": (lambda f: _bal((12, 400, 1600), f), {"force_general_layout": True}, False),
    "mini_ba": (_mini_ba, {}, False),
    "held_cameras": (_held, {}, False),
    "quaternion_manifold": (_quaternion, {}, True),
    "user_bundler_huber": (_bundler, {}, True),
    "user_pose_reprojection": (_pose, {}, True),
    "unobserved_camera": (_unobserved, {}, True),
}
FORMATS = {"bsm": ca.BLOCK_SPARSE, "crs": ca.COMPRESSED_ROW}


def value_columns(prog):
    """The delta column of every stored Jacobian value (-1: in no cell), by
    the addressing of test_spmv_gpu.dense_jacobian."""
    col = np.full(prog.num_jacobian_values, -1, np.int64)
    begin, ids = prog.block_params_csr()
    nres = prog.residuals_per_block()
    for b in range(prog.num_residual_blocks):
        q = int(prog.jacobian_per_residual_layout[b])
        for pid in ids[begin[b]:begin[b + 1]]:
            if prog.pb_constant[pid]:
                continue
            d0, t = int(prog.delta_offset[pid]), int(prog.pb_tangent[pid])
            for _ in range(int(nres[b])):
                off = int(prog.jacobian_per_residual_offsets[q])
                q += 1
                assert np.all(col[off:off + t] == -1)  # no value in two cells
                col[off:off + t] = np.arange(d0, d0 + t)
    return col


def norm_reference(vals, col, n):
    """(fsum of the squared entries, stored entries) per column."""
    order = np.argsort(col, kind="stable")
    order = order[col[order] >= 0]
    sq = vals[order] * vals[order]
    terms = np.bincount(col[order], minlength=n)
    ends = np.cumsum(terms)
    ref = np.array([math.fsum(sq[e - t:e]) for t, e in zip(terms, ends)])
    return ref, terms


def check_norm(got, ref, terms, extra=0.0, what=""):
    assert not np.isnan(got).any(), (what, "an entry was not assigned")
    err = np.abs(got - ref)
    bound = (1.01 * (terms + 2) * U53 + extra) * ref
    worst = int(np.argmax(err - bound))
    print(f"{what}: worst column {worst}: err {err[worst]:.3e} bound {bound[worst]:.3e} "
          f"terms {terms[worst]}")
    assert np.all(err <= bound), (what, worst, err[worst], bound[worst])


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("case", list(CASES))
def test_column_ops_match_the_dense_jacobian(gpu, case, fmt):
    from test_spmv_gpu import dense_jacobian
    build, opts, affine = CASES[case]
    prog = build(FORMATS[fmt])
    dev = torch.device("cuda", 0)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream, **opts)
    try:
        ok, cost, r, g, jvals = ev.evaluate()
        assert ok
        info = ev.info()
        if affine:
            assert info.num_affine_groups == len(prog.groups)
        n, nv = prog.num_effective_parameters, prog.num_jacobian_values
        col = value_columns(prog)
        ref, terms = norm_reference(jvals, col, n)
        J = dense_jacobian(prog, jvals)
        assert np.array_equal(terms, np.count_nonzero(dense_jacobian(prog, np.ones(nv)), axis=0))

        # ---- the norm: assigned over a NaN prefill, within the bound, repeatable
        dj = torch.from_numpy(jvals).to(dev)
        outs = []
        for _ in range(2):
            dn = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
            ev.squared_column_norm_device(dj.data_ptr(), dn.data_ptr())
            torch.cuda.synchronize(dev)
            outs.append(dn.cpu().numpy())
        check_norm(outs[0], ref, terms, what=f"{case}/{fmt} norm")
        check_norm(outs[1], ref, terms, what=f"{case}/{fmt} norm (repeat)")
        assert np.all(outs[0][terms == 0] == 0.0)
        if affine:
            assert np.array_equal(outs[0], outs[1])
        assert np.array_equal(dj.cpu().numpy(), jvals)  # J is only read

        # ---- scaling: exact, every cell once, nothing else; both base alignments
        rng = np.random.default_rng(7)
        scale = rng.uniform(0.5, 2.0, n)
        ds = torch.from_numpy(scale).to(dev)
        want = np.where(col >= 0, jvals * scale[np.maximum(col, 0)], jvals)
        for shift in (0, 1):
            host = np.full(shift + nv + 64, SENTINEL)
            host[shift:shift + nv] = jvals
            buf = torch.from_numpy(host).to(dev)
            assert buf.data_ptr() % 16 == 0
            ev.scale_columns_device(buf.data_ptr() + 8 * shift, ds.data_ptr())
            torch.cuda.synchronize(dev)
            back = buf.cpu().numpy()
            scaled = back[shift:shift + nv]
            assert np.array_equal(dense_jacobian(prog, scaled), J * scale[None, :]), shift
            assert np.array_equal(scaled, want), shift
            assert np.all(back[:shift] == SENTINEL) and np.all(back[shift + nv:] == SENTINEL), shift

        # ---- the norm of the scaled values: scale^2 norm
        dsc = torch.from_numpy(np.ascontiguousarray(scaled)).to(dev)
        dn = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        ev.squared_column_norm_device(dsc.data_ptr(), dn.data_ptr())
        torch.cuda.synchronize(dev)
        check_norm(dn.cpu().numpy(), scale * scale * ref, terms, extra=3 * 2.0 ** -52,
                   what=f"{case}/{fmt} norm after scale")
    finally:
        ev.close()


def test_unobserved_camera_reads_exactly_zero(gpu):
    prog = _unobserved(ca.BLOCK_SPARSE)
    dev = torch.device("cuda", 0)
    ev = ca.Evaluator(prog, stream=torch.cuda.current_stream(dev).cuda_stream)
    try:
        ok, cost, r, g, jvals = ev.evaluate()
        assert ok
        n = prog.num_effective_parameters
        dj = torch.from_numpy(jvals).to(dev)
        dn = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        ev.squared_column_norm_device(dj.data_ptr(), dn.data_ptr())
        torch.cuda.synchronize(dev)
        got = dn.cpu().numpy()
    finally:
        ev.close()
    # The sixth camera's nine columns are the last delta columns.
    cam = prog.num_parameter_blocks - 1
    d0 = int(prog.delta_offset[cam])
    assert int(prog.pb_tangent[cam]) == 9
    assert np.array_equal(got[d0:d0 + 9], np.zeros(9))
    assert np.all(got[:d0] > 0)


def test_multi_device_evaluator_refuses_both(gpu):
    prog = bal.synthetic_program((8, 300, 1200), seed=2)
    ev = ca.Evaluator(prog, devices=[0, 0])
    try:
        with pytest.raises(RuntimeError, match="multi-device"):
            ev.squared_column_norm_device(1, 1)
        with pytest.raises(RuntimeError, match="multi-device"):
            ev.scale_columns_device(1, 1)
    finally:
        ev.close()


# ---- the driver ------------------------------------------------------------
BASE = ["--synthetic", "problem-16-22106", "--robustify", "--point_sigma", "0.05",
        "--num_iterations", "4"]


@pytest.mark.parametrize("solver", ["iterative_schur", "dense_schur", "cgnr"])
def test_driver_jacobi_scaling_reduces_cost(gpu, solver):
    from ceres_amd import bundle_adjuster
    c0, c1, rows = bundle_adjuster.main(BASE + ["--jacobi_scaling", "--linear_solver", solver])
    costs = [r[1] for r in rows] + [c1]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    assert all(r[-1] for r in rows)
    assert c1 < 0.9 * c0


def test_driver_jacobi_scaling_solves_the_same_systems(gpu):
    """dense_schur with and without --jacobi_scaling: with D_s = S^2 D the
    scaled system S (J^T J + D / radius) S y = -S g has y = S^-1 dx, so while
    neither clamp is active the two runs take the same steps in exact
    arithmetic and their costs differ by rounding alone, amplified by the
    conditioning of the two Cholesky factorizations.
    Measured on an MI355X (scaling in [4.9e-5, 0.87], LM diagonals in
    [0.016, 5.2e8] unscaled and [0.0095, 2.6] scaled, both clear of the
    clamps): the steps of the two runs differ by 1e-15 relative, the gradient
    norms by 1e-13, and all nine costs (four old, four new, the final one) are
    bit-identical -- an observed difference of 0, below the resolution of the
    measurement, which is one ulp of the cost (2^-52 relative).  The assertion
    is two orders of magnitude above that resolution, 100 x 2^-52 = 2.2e-14.
    Whatever was measured, a relative difference above 1e-6 is a wrong
    un-scaling, not rounding."""
    from ceres_amd import bundle_adjuster
    runs = {}
    for flag in (False, True):
        stats = {}
        argv = BASE + ["--linear_solver", "dense_schur"] + (["--jacobi_scaling"] if flag else [])
        c0, c1, rows = bundle_adjuster.main(argv, stats=stats)
        lo = min(d[0] for d in stats["lm_diagonal"])
        hi = max(d[1] for d in stats["lm_diagonal"])
        assert lo > 1e-6 and hi < 1e32, ("a clamp is active", flag, lo, hi)
        assert all(r[-1] for r in rows)
        runs[flag] = np.array([r[1] for r in rows] + [r[2] for r in rows] + [c1])
    rel = np.abs(runs[True] - runs[False]) / np.abs(runs[False])
    print("jacobi_scaling vs not, relative cost differences:", rel)
    assert rel.max() <= REL_BOUND
    assert rel.max() <= 1e-6


# 100 x the resolution of the measured (zero) difference: see the test above.
REL_BOUND = 100 * 2.0 ** -52
