"""Per-block loss parameters (ABI 6, cse_residual_group.loss_data_size) on the
host: the refusals of cse_create (before any HIP call, so they run without a
GPU), the grouping of ProblemCUDA.program(merge_loss_parameters=...), the
widened rows of Program.descriptor(), and the planner under
AddressSanitizer + UBSan (tests/cpp/per_block_loss_driver.cpp, a stand-alone
g++ program: plan.cpp and layout.cpp, no HIP)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import _cse, bal

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")


def test_abi_version_is_6():
    assert _cse.lib().cse_abi_version() == 6
    assert _cse.CSE_ABI_VERSION == 6
    assert dict(_cse.cse_residual_group._fields_)["loss_data_size"] is C.c_int32
    assert C.sizeof(_cse.cse_residual_group) == 136  # the field was `reserved`


def _desc(loss, kind=_cse.SNAVELY_2_9_3):
    """A small valid Snavely descriptor with per-block rows; the caller
    edits groups[0]."""
    n = 40
    ld = np.tile(np.array([[1.5, 2.0]]), (n, 1))
    ld[::2] = [0.5, 0.25]
    prog = bal.synthetic_program((6, 12, n), loss=loss, loss_data=ld, seed=3)
    d = prog.descriptor()
    assert d.groups[0].loss_data_size == 2
    d.groups[0].functor_kind = kind
    return prog, d


def _create(d, jet=False):
    L = _cse.lib()
    o = _cse.cse_options()
    L.cse_default_options(C.byref(o))
    if jet:
        o.jacobian_form = _cse.JACOBIAN_JET
    h = C.c_void_p()
    rc = L.cse_create(C.byref(d), C.byref(o), C.byref(h))
    msg = _cse.last_error()
    assert rc != _cse.CSE_OK and not h.value, "created an evaluator from a descriptor it must refuse"
    return rc, msg


HUBER_SCALED = ca.Loss.huber(1.0).scaled_by(2.0)


@pytest.mark.parametrize("case, want", [
    ("size_1", _cse.CSE_ERR_INVALID),
    ("size_3", _cse.CSE_ERR_INVALID),
    ("size_negative", _cse.CSE_ERR_INVALID),
    ("user_loss", _cse.CSE_ERR_UNSUPPORTED),
    ("user_kind", _cse.CSE_ERR_UNSUPPORTED),
    ("test_kind", _cse.CSE_ERR_UNSUPPORTED),
    ("trivial_unscaled", _cse.CSE_ERR_INVALID),
    ("jet", _cse.CSE_ERR_UNSUPPORTED),
])
def test_create_refuses_without_a_gpu(case, want):
    """Each refusal of cse.h (cse_residual_group) comes from cse_create before
    any HIP call, with its code and a message naming loss_data_size."""
    prog, d = _desc(HUBER_SCALED)
    g = d.groups[0]
    jet = False
    if case.startswith("size_"):
        g.loss_data_size = {"size_1": 1, "size_3": 3, "size_negative": -2}[case]
    elif case == "user_loss":
        g.loss.kind = _cse.LOSS_USER
    elif case == "user_kind":
        g.functor_kind = _cse.FUNCTOR_USER_FIRST + 5  # registered or not: no per-block slots
    elif case == "test_kind":
        g.functor_kind = 102  # CSE_FUNCTOR_TEST_LINEAR_2_2_3
        g.loss.kind, g.loss.scaled = _cse.LOSS_TRIVIAL, 0
    elif case == "trivial_unscaled":
        g.loss.kind, g.loss.scaled = _cse.LOSS_TRIVIAL, 0
    elif case == "jet":
        jet = True
    rc, msg = _create(d, jet=jet)
    assert rc == want, (case, rc, msg)
    assert "loss_data_size" in msg, (case, msg)


def test_descriptor_widens_the_rows():
    n = 25
    ld = np.column_stack([np.linspace(0.5, 3.0, n), np.linspace(0.25, 4.0, n)])
    prog = bal.synthetic_program((6, 9, n), loss=HUBER_SCALED, loss_data=ld, seed=5)
    g = prog.groups[0]
    assert g.data.shape == (n, 2) and np.array_equal(g.loss_data, ld)
    d = prog.descriptor()
    assert d.groups[0].loss_data_size == 2
    rows = np.ctypeslib.as_array(d.groups[0].functor_data, shape=(n, 4))
    assert np.array_equal(rows[:, :2], g.data) and np.array_equal(rows[:, 2:], ld)
    # a uniform program writes what it always wrote
    uni = bal.synthetic_program((6, 9, n), loss=HUBER_SCALED, seed=5)
    du = uni.descriptor()
    assert du.groups[0].loss_data_size == 0
    assert np.array_equal(np.ctypeslib.as_array(du.groups[0].functor_data, shape=(n, 2)), g.data)


def _interleaved_problem(losses, n=30, seed=0):
    """n Snavely blocks over 4 cameras and 10 points, block i with
    losses[i % len(losses)], one add_residual_blocks call each."""
    rng = np.random.default_rng(seed)
    p = ca.ProblemCUDA()
    pts = [p.add_parameter_block(rng.normal(size=3)) for _ in range(10)]
    cams = [p.add_parameter_block(rng.normal(size=9)) for _ in range(4)]
    obs = rng.normal(size=(n, 2))
    for i in range(n):
        p.add_residual_block(_cse.SNAVELY_2_9_3, losses[i % len(losses)], obs[i], cams[i % 4],
                             pts[(i * 3) % 10])
    return p, obs


def test_merge_three_widths_and_scales_into_one_group():
    widths, scales = (0.5, 1.0, 2.0), (0.25, 1.0, 4.0)
    losses = [ca.Loss.huber(a).scaled_by(s) for a, s in zip(widths, scales)]
    p, obs = _interleaved_problem(losses)
    prog = p.program(merge_loss_parameters=True)
    assert len(prog.groups) == 1
    g = prog.groups[0]
    assert g.loss.kind == _cse.LOSS_HUBER and g.loss.scaled
    assert g.index is None and g.first == 0 and g.n == 30  # program order
    want = np.array([[widths[i % 3], scales[i % 3]] for i in range(30)])
    assert np.array_equal(g.loss_data, want)
    assert np.array_equal(g.data, obs)
    # The default: one group per distinct value, as before.
    split = p.program()
    assert len(split.groups) == 3
    for k, g in enumerate(split.groups):
        assert g.loss_data is None
        assert (g.loss.a, g.loss.scale) == (widths[k], scales[k])
        assert np.array_equal(g.index, np.arange(k, 30, 3))
        assert np.array_equal(g.data, obs[k::3])
    assert [g.loss.key() for g in p.program(merge_loss_parameters=False).groups] == \
        [g.loss.key() for g in split.groups]


def test_merge_keeps_loss_types_apart():
    losses = [ca.Loss.huber(1.0), ca.Loss.cauchy(1.0), ca.Loss.huber(2.0), ca.Loss.cauchy(3.0),
              ca.Loss.huber(1.0).scaled_by(2.0), ca.Loss.trivial()]
    p, _ = _interleaved_problem(losses, n=36)
    prog = p.program(merge_loss_parameters=True)
    keys = [(g.loss.kind, bool(g.loss.scaled), g.loss_data is not None) for g in prog.groups]
    # Huber, Cauchy, scaled Huber (one value: uniform), the trivial loss (nothing to vary)
    assert keys == [(_cse.LOSS_HUBER, False, True), (_cse.LOSS_CAUCHY, False, True),
                    (_cse.LOSS_HUBER, True, False), (_cse.LOSS_TRIVIAL, False, False)]
    assert sorted(set(prog.groups[0].loss_data[:, 0])) == [1.0, 2.0]
    assert sorted(set(prog.groups[1].loss_data[:, 0])) == [1.0, 3.0]
    assert sum(g.n for g in prog.groups) == 36


def test_merge_of_equal_parameters_stays_uniform():
    p, _ = _interleaved_problem([ca.Loss.huber(1.5), ca.Loss.huber(1.5)])
    prog = p.program(merge_loss_parameters=True)
    assert len(prog.groups) == 1
    assert prog.groups[0].loss_data is None
    assert prog.groups[0].loss.key() == ca.Loss.huber(1.5).key()
    assert prog.compile(ca.BLOCK_SPARSE).descriptor().groups[0].loss_data_size == 0


def test_merge_ignores_the_columns_the_loss_does_not_read():
    """An unscaled Huber batch whose (ignored) scale column varies, and scaled
    trivial blocks whose (unused) a varies, have equal parameters: uniform."""
    rng = np.random.default_rng(4)
    for loss, ld, want in (
            (ca.Loss.huber(1.0), np.column_stack([np.full(12, 2.5), np.arange(12.0)]), (2.5, 1.0)),
            (ca.Loss.trivial().scaled_by(1.0), np.column_stack([np.arange(12.0), np.full(12, 3.0)]), (1.0, 3.0)),
            (ca.Loss.huber(1.0).scaled_by(1.0), np.column_stack([np.full(12, 2.5), np.full(12, 3.0)]), (2.5, 3.0))):
        p = ca.ProblemCUDA()
        pts = [p.add_parameter_block(rng.normal(size=3)) for _ in range(4)]
        cams = [p.add_parameter_block(rng.normal(size=9)) for _ in range(3)]
        p.add_residual_blocks(_cse.SNAVELY_2_9_3, loss, [[cams[i % 3], pts[i % 4]] for i in range(12)],
                              rng.normal(size=(12, 2)), loss_data=ld)
        g, = p.program(merge_loss_parameters=True).groups
        assert g.loss_data is None and (g.loss.a, g.loss.scale) == want, (loss, g.loss)
    # ... and a column that is read keeps the group per-block
    p = ca.ProblemCUDA()
    pts = [p.add_parameter_block(rng.normal(size=3)) for _ in range(4)]
    cam = p.add_parameter_block(rng.normal(size=9))
    ld = np.column_stack([np.arange(4.0) + 1.0, np.ones(4)])
    p.add_residual_blocks(_cse.SNAVELY_2_9_3, ca.Loss.huber(1.0), [[cam, x] for x in pts],
                          rng.normal(size=(4, 2)), loss_data=ld)
    g, = p.program(merge_loss_parameters=True).groups
    assert np.array_equal(g.loss_data, ld)


def test_merge_leaves_user_losses_and_user_kinds_by_value():
    p = ca.ProblemCUDA()
    a = p.add_parameter_block(np.zeros(3))
    user = [ca.Loss.user_loss(b"\x01" * 8), ca.Loss.user_loss(b"\x02" * 8)]
    for l in user + user:
        p.add_residual_blocks(_cse.POINT_DISPLACEMENT_3_3, l, [[a]], [[0.0, 0.0, 0.0]])
    prog = p.program(merge_loss_parameters=True)
    assert len(prog.groups) == 2 and all(g.loss_data is None for g in prog.groups)


def test_batch_with_per_block_parameters():
    """add_residual_blocks(..., loss_data=): a whole batch of weighted
    observations in one call."""
    rng = np.random.default_rng(1)
    p = ca.ProblemCUDA()
    pts = [p.add_parameter_block(rng.normal(size=3)) for _ in range(5)]
    cams = [p.add_parameter_block(rng.normal(size=9)) for _ in range(3)]
    n = 15
    ids = [[cams[i % 3], pts[i % 5]] for i in range(n)]
    w = np.column_stack([np.ones(n), rng.uniform(0.5, 2.0, n)])
    p.add_residual_blocks(_cse.SNAVELY_2_9_3, ca.Loss.trivial().scaled_by(1.0), ids,
                          rng.normal(size=(n, 2)), loss_data=w)
    p.add_residual_block(_cse.SNAVELY_2_9_3, ca.Loss.trivial().scaled_by(3.0), [0.0, 0.0], cams[0], pts[1])
    split = p.program()
    assert len(split.groups) == 2 and np.array_equal(split.groups[0].loss_data, w)
    merged = p.program(merge_loss_parameters=True)
    assert len(merged.groups) == 1
    assert np.array_equal(merged.groups[0].loss_data, np.vstack([w, [[1.0, 3.0]]]))
    with pytest.raises(ValueError):
        p.add_residual_blocks(_cse.SNAVELY_2_9_3, ca.Loss.trivial(), ids, np.zeros((n, 2)), loss_data=w)


def test_shard_program_slices_the_loss_data():
    from ceres_amd import shard
    cams, pts, ci, pi, obs = bal.synthetic(6, 40, 200, seed=2)
    ld = np.column_stack([np.arange(200.0) + 1.0, np.ones(200)])
    for rank in range(2):
        prog, sh = shard.shard_program(cams, pts, ci, pi, obs, rank, 2, loss=ca.Loss.huber(1.0),
                                       loss_data=ld, compile=False)
        b0, b1 = sh.blocks
        assert np.array_equal(prog.groups[0].loss_data, ld[b0:b1])
        assert np.array_equal(prog.groups[0].data, obs[b0:b1])
    prog, _ = shard.shard_program(cams, pts, ci, pi, obs, 0, 2, loss=ca.Loss.huber(1.0), compile=False)
    assert prog.groups[0].loss_data is None


def test_planner_driver_under_asan_ubsan():
    """The stand-alone planner driver, g++ -fsanitize=address,undefined with
    the sanitizer runtimes linked statically (the test preloads nothing and
    passes its environment through): a per-block Snavely group in BSM and CRS, with held
    cameras, the one-slot kind, and every refused descriptor."""
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "per_block_loss.mk", "driver"])
    out = subprocess.run([os.path.join(CPP, "build", "per_block_loss_driver")], capture_output=True,
                         text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout and "FAILED" not in out.stdout
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
