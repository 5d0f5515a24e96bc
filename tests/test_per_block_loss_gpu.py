"""Per-block loss parameters on the GPU (cse_residual_group.loss_data_size 2;
csrc/per_block_loss_kernels.hip): one group per (functor kind, loss type)
whose blocks each bring their own (a, scale).

Problems: bal.synthetic_program over the chunk (64) and workgroup (256)
boundaries; n % 4 == 0 takes the group-store kernel, the others the one-wave
kernel (tests/test_group_store_gpu.py).  Per-block values: the Huber/Cauchy
width a_i is the 25th, 50th or 75th percentile of the unrobustified block
residual norms (oracle, apply_loss_function=False), round-robin, so both
Huber branches occur by construction -- asserted below (at least 10 % of the
blocks on each side of s > a_i^2 for n >= 64; a single block, n = 1, has one
side only); the scales are 0.25, 1, 4, round-robin in step with the widths, so
a problem has three distinct (a, scale) values.

Checker: the oracle takes the loss per block (rb_loss_a, rb_loss_scale); its
arrays op.a["la"], op.a["ls"] are filled in place with the per-block values.
Tolerances: tests/parity_util.py (assert_parity, COST_RTOL), no other number.
Bit-equality (np.array_equal) wherever kernels and arithmetic are the same:
against the split program (one group per distinct value) in residuals and
Jacobian, against a uniform group when every row holds the same values in
every output, and affine against general path.
"""
import copy
import functools

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse, bal
from ceres_amd.problem import ResidualGroup
import oracle_py as O
from parity_util import COST_RTOL, assert_parity

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 256, 260, 700, 1028]
SCALES = (0.25, 1.0, 4.0)
LOSSES = {
    "huber": ca.Loss.huber(1.0),
    "cauchy": ca.Loss.cauchy(1.0),
    "scaled_trivial": ca.Loss.trivial().scaled_by(1.0),
    "scaled_huber": ca.Loss.huber(1.0).scaled_by(1.0),
}
FORMATS = {"bsm": ca.BLOCK_SPARSE, "crs": ca.COMPRESSED_ROW}


def _counts(n):
    return max(6, min(40, n // 8 + 2)), max(1, min(n, n // 5 + 1)), n


def _oracle_program(prog, ld, **kw):
    """The oracle's per-block loss arrays filled in place with ld (the
    program's one group is contiguous from block 0)."""
    ex = prog.with_explicit_manifolds()
    op = O.OracleProgram.from_program(ex, **kw)
    if ld is not None:
        g = prog.groups[0]
        idx = g.index if g.index is not None else np.arange(g.first, g.first + g.n)
        op.a["la"][idx] = ld[:, 0]
        op.a["ls"][idx] = ld[:, 1]
    return ex, op


def _oracle(prog, ld, **kw):
    ex, op = _oracle_program(prog, ld)
    return op.evaluate(ex.state, ex.constant_state if ex.constant_state.size else None,
                       num_threads=8, **kw)


def _block_norms(prog):
    """|r_i| of every block without the loss (oracle)."""
    ex, op = _oracle_program(prog, None, apply_loss_function=False)
    r = op.evaluate(ex.state, ex.constant_state if ex.constant_state.size else None, num_threads=8,
                    gradient=False, jacobian=False)[2]
    nr = _cse.functor_shape(prog.groups[0].kind)[0]
    return np.linalg.norm(r.reshape(-1, nr), axis=1)


def _loss_data(prog, loss):
    """(n, 2) per-block (a, scale) as the module docstring describes, and
    the check that both Huber branches occur."""
    norms = _block_norms(prog)
    n = norms.size
    q = np.percentile(norms, [25, 50, 75])
    a = q[np.arange(n) % 3] if loss.kind != _cse.LOSS_TRIVIAL else np.ones(n)
    s = np.asarray(SCALES)[np.arange(n) % 3] if loss.scaled else np.ones(n)
    if loss.kind == _cse.LOSS_HUBER:
        out = norms ** 2 > a ** 2
        if n >= 64:
            assert 0.1 * n <= out.sum() <= 0.9 * n, (n, out.sum())
        elif n > 1:
            assert 0 < out.sum() < n, (n, out.sum())
    return np.ascontiguousarray(np.column_stack([a, s]))


@functools.lru_cache(maxsize=None)
def _case(n, lname, fname="bsm", seed=11, **kw):
    """(merged program, its (n, 2) loss data, oracle outputs), built once and
    shared; nothing mutates them."""
    loss, fmt = LOSSES[lname], FORMATS[fname]
    plain = bal.synthetic_program(_counts(n), loss=loss, format=fmt, seed=seed, **kw)
    ld = _loss_data(plain, loss)
    prog = bal.synthetic_program(_counts(n), loss=loss, format=fmt, seed=seed, loss_data=ld, **kw)
    assert len(prog.groups) == 1 and prog.groups[0].loss_data is not None
    return prog, ld, _oracle(prog, ld)


def _split(prog):
    """The same blocks as one group per distinct (a, scale): today's path."""
    g = prog.groups[0]
    values, inverse = np.unique(g.loss_data, axis=0, return_inverse=True)
    inverse = np.ravel(inverse)
    groups = []
    for k, (a, s) in enumerate(values):
        sel = np.flatnonzero(inverse == k)
        loss = ca.Loss(g.loss.kind, float(a), g.loss.scaled, float(s) if g.loss.scaled else 1.0)
        groups.append(ResidualGroup(g.kind, loss, g.ids[sel], g.data[sel], sel.astype(np.int64) + g.first, 0))
    out = copy.copy(prog)
    out.groups = groups
    out._keep = []
    return out


def _uniform(prog, a, s):
    g = prog.groups[0]
    out = copy.copy(prog)
    out.groups = [ResidualGroup(g.kind, ca.Loss(g.loss.kind, a, g.loss.scaled, s), g.ids, g.data,
                                g.index, g.first)]
    out._keep = []
    return out


def _with_loss_data(prog, ld):
    out = copy.copy(prog)
    out.groups = [copy.copy(prog.groups[0])]
    out.groups[0].loss_data = ld
    out._keep = []
    return out


def _eval(prog, outputs=(True, True, True), runs=1, **opts):
    ev = ca.Evaluator(prog, **opts)
    try:
        got = [ev.evaluate(residuals=outputs[0], gradient=outputs[1], jacobian=outputs[2])
               for _ in range(runs)]
        info = ev.info()
    finally:
        ev.close()
    return (got[0] if runs == 1 else got), info


def _same_bits(a, b, names=("residuals", "jacobian")):
    for name, k in (("residuals", 2), ("gradient", 3), ("jacobian", 4)):
        if name in names:
            assert np.array_equal(a[k], b[k]), name
    if "cost" in names:
        assert a[1] == b[1], (a[1], b[1])


# 1. Oracle parity of the merged single group, both layouts.
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("lname", list(LOSSES))
@pytest.mark.parametrize("fname", list(FORMATS))
def test_oracle_parity(gpu, n, lname, fname):
    prog, ld, ref = _case(n, lname, fname)
    got, info = _eval(prog)
    assert info.num_groups == 1  # (the policy equals the uniform twin's: checked below)
    assert_parity(got, ref, ("per-block", n, lname, fname))


# 2. Against the split program (one group per distinct value).
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("lname", list(LOSSES))
def test_against_the_split_program(gpu, n, lname):
    prog, ld, ref = _case(n, lname)
    split = _split(prog)
    distinct = len(np.unique(ld, axis=0))
    assert len(split.groups) == distinct and distinct == (min(3, n) if n > 1 else 1)
    got, _ = _eval(prog)
    old, info = _eval(split)
    assert info.num_groups == distinct
    _same_bits(got, old)
    assert abs(got[1] - old[1]) <= COST_RTOL * abs(old[1])
    assert_parity(got, old, ("merged vs split", n, lname))  # the gradient sums in another order
    assert_parity(old, ref, ("split vs oracle", n, lname))


# 3. Rows that all hold the same (a, scale): the uniform group's bits in
# every output (same kernels, same order, same arithmetic).
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("lname", list(LOSSES))
@pytest.mark.parametrize("fname", list(FORMATS))
def test_constant_rows_equal_the_uniform_group(gpu, n, lname, fname):
    prog, ld, _ = _case(n, lname, fname)
    a, s = float(np.median(ld[:, 0])), 4.0 if LOSSES[lname].scaled else 1.0
    const = _with_loss_data(prog, np.tile(np.array([[a, s]]), (n, 1)))
    uni = _uniform(prog, a, s)
    got, gi = _eval(const)
    want, wi = _eval(uni)
    _same_bits(got, want, ("residuals", "gradient", "jacobian", "cost"))
    for outputs in ((True, False, True), (True, False, False), (False, False, False)):
        g2, _ = _eval(const, outputs)
        w2, _ = _eval(uni, outputs)
        _same_bits(g2, w2, [nm for nm, on in zip(("residuals", "gradient", "jacobian"), outputs) if on] + ["cost"])
    # 7. the same plan: policy, fused gradient, and 16 bytes more per block
    assert gi.num_groups == 1 and wi.num_groups == 1
    assert gi.num_affine_groups == wi.num_affine_groups
    assert gi.num_fused_gradient_groups == wi.num_fused_gradient_groups
    assert gi.bytes_jacobian_eval == wi.bytes_jacobian_eval + 16 * n
    assert gi.bytes_residual_eval == wi.bytes_residual_eval + 16 * n


# 4. Affine against general path.
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("lname", list(LOSSES))
def test_affine_and_general_path_same_bits(gpu, n, lname):
    prog, ld, ref = _case(n, lname)
    got, gi = _eval(prog, (True, False, True))
    gen, ni = _eval(prog, (True, False, True), force_general_layout=True)
    assert gi.num_affine_groups == 1 and ni.num_affine_groups == 0
    _same_bits(got, gen)
    full, _ = _eval(prog, force_general_layout=True)  # the table kernel's gradient atomics
    assert_parity(full, ref, ("general", n, lname))


# 5. Gradient modes.
@pytest.mark.parametrize("n", [65, 260, 700])
@pytest.mark.parametrize("fname", list(FORMATS))
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_gradient_modes(gpu, n, fname, mode):
    prog, ld, ref = _case(n, "scaled_huber", fname)
    (a, b), info = _eval(prog, runs=2, gradient_mode=mode)
    assert_parity(a, ref, ("mode", mode, n, fname))
    assert_parity(b, ref, ("mode", mode, n, fname))
    if mode != 2:  # fixed summation order
        _same_bits(a, b, ("residuals", "gradient", "jacobian", "cost"))


# 6. Reduced outputs: residuals only, and the cost alone (the candidate step:
# LossAndCorrect without the Corrector).
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("lname", list(LOSSES))
def test_reduced_outputs(gpu, n, lname):
    prog, ld, ref = _case(n, lname)
    ok, cost, r, g, j = _eval(prog, (True, False, False))[0]
    assert ok and g is None and j is None
    assert_parity((ok, cost, r, None, None), (ref[0], ref[1], ref[2], None, None), ("residuals", n, lname))
    ok, cost, r, g, j = _eval(prog, (False, False, False))[0]
    assert ok and r is None
    assert abs(cost - ref[1]) <= COST_RTOL * abs(ref[1])


# 8. Other kinds and layouts, one case each.
@pytest.mark.parametrize("fname", list(FORMATS))
def test_held_cameras(gpu, fname):
    prog, ld, ref = _case(700, "scaled_huber", fname, constant_cameras=(1, 5))
    for mode in (0, 2):
        got, info = _eval(prog, gradient_mode=mode)
        assert info.num_affine_groups == 1
        assert_parity(got, ref, ("held", fname, mode))


def test_quaternion_manifold(gpu):
    prog, ld, ref = _case(700, "huber", "bsm", quaternion_manifold=True)
    got, info = _eval(prog)
    assert info.num_affine_groups == 1 and info.num_fused_gradient_groups == 1
    assert_parity(got, ref, "quaternion manifold")
    got, _ = _eval(prog, gradient_mode=1)
    assert_parity(got, ref, "quaternion manifold, post-pass")


def test_snavely_no_distortion(gpu):
    prog, ld, ref = _case(260, "cauchy", "bsm", kind=_cse.SNAVELY_NO_DISTORTION_2_7_3)
    got, info = _eval(prog)
    assert info.num_affine_groups == 1
    assert_parity(got, ref, "no distortion")
    crs, ld2, ref2 = _case(260, "cauchy", "crs", kind=_cse.SNAVELY_NO_DISTORTION_2_7_3)
    assert_parity(_eval(crs)[0], ref2, "no distortion, crs")


@pytest.mark.parametrize("general", [False, True])
def test_point_displacement_one_slot_kind(gpu, general):
    rng = np.random.default_rng(5)
    n = 130
    p = ca.ProblemCUDA()
    values = rng.normal(size=(n, 3))
    blocks = [p.add_parameter_block(v) for v in values]
    data = rng.normal(size=(n, 3))
    norms = np.linalg.norm(values - data, axis=1)  # |x - data|: the block residual norms
    ld = np.column_stack([np.percentile(norms, [25, 50, 75])[np.arange(n) % 3],
                          np.asarray(SCALES)[np.arange(n) % 3]])
    p.add_residual_blocks(_cse.POINT_DISPLACEMENT_3_3, ca.Loss.huber(1.0).scaled_by(1.0),
                          [[b] for b in blocks], data, loss_data=ld)
    prog = p.program()
    prog.compile(ca.BLOCK_SPARSE)
    assert prog.groups[0].loss_data is not None
    ref = _oracle(prog, ld)
    got, info = _eval(prog, force_general_layout=general)
    assert info.num_groups == 1 and info.num_affine_groups == (0 if general else 1)
    assert_parity(got, ref, ("point displacement", general))
    old, _ = _eval(_split(prog), force_general_layout=general)
    _same_bits(got, old)


# 9. Multi-device: two shards on device 0.
def test_multi_device_two_shards(gpu):
    prog, ld, ref = _case(700, "scaled_huber")
    one, _ = _eval(prog)
    ev = ca.Evaluator(prog, devices=[0, 0])
    try:
        first, devs = ev.shard_info()
        assert len(devs) == 2 and 0 < first[1] < 700
        two = ev.evaluate()
    finally:
        ev.close()
    _same_bits(one, two)
    assert_parity(two, one, "two shards vs one evaluator")
    assert_parity(two, ref, "two shards vs oracle")


# 10. Schur: the merged group has the structure, the split program does not.
def test_schur_structure_needs_the_single_group(gpu):
    prog, ld, _ = _case(700, "huber")
    ev = ca.Evaluator(prog)
    try:
        e_cols, f_cols = ev.schur_structure()
    finally:
        ev.close()
    cams, pts, n = _counts(700)
    assert (e_cols, f_cols) == (3 * pts, 9 * cams)
    ev = ca.Evaluator(_split(prog))
    try:
        with pytest.raises(RuntimeError, match=r"cse_schur_structure failed \(-4\)"):
            ev.schur_structure()
    finally:
        ev.close()


# 11. The Jet form has no per-block kernels: refused at create.
def test_jet_form_is_refused(gpu):
    prog, ld, _ = _case(260, "huber")
    with pytest.raises(RuntimeError, match="loss_data_size"):
        ca.Evaluator(prog, jacobian_form="jet")
    got, _ = _eval(_uniform(prog, 1.0, 1.0), jacobian_form="jet")  # a uniform group still runs
    assert got[0]
