"""bench.py's plain run on the GPU: the result line's headline fields, the
plain/--full split and --dump-outputs (the last timed step's outputs as .npy,
from the seeded generator's inputs), on problem-16 (83,718 blocks: residuals
written whole, the 2,009,232 Jacobian values as the seeded sample).  The dumped
arrays are checked against the oracle at the tolerance of tests/parity_util.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ceres_amd as ca
from ceres_amd import bal, shard
import oracle_py as O
from parity_util import assert_parity

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = "problem-16-22106"


def _bench(*extra):
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
                          "--config", CONFIG, "--steps", "3", "--warmup", "1", *extra],
                         capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(gpu, tmp_path):
    import bench

    a = str(tmp_path / "dump")
    line = _bench("--dump-outputs", a)

    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "evals/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-9)
    # a plain run measures the headline alone
    assert line["full"] is False and line["secondary"] == {} and line["cpu_baseline"] is None

    names = sorted(os.listdir(a))
    assert names == ["cost.npy", "jacobian.npy", "residuals.npy"]
    got = {n[:-4]: np.load(os.path.join(a, n)) for n in names}
    assert all(v.dtype == np.float64 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20

    # The inputs are the seeded generator's: the oracle on the same problem.
    arrays = bal.synthetic(*bal.CONFIGS[CONFIG], seed=0xCE2E5)
    prog, _ = shard.shard_program(*arrays, 0, 1, loss=ca.Loss.huber(1.0))
    ok, cost, r, _, j = O.OracleProgram.from_program(prog).evaluate(prog.state, gradient=False)
    assert got["cost"].shape == (1,) and got["residuals"].shape == r.shape
    assert j.size > bench.DUMP_MAX_VALUES >= r.size
    idx = bench.sample_indices(j.size)
    assert got["jacobian"].shape == idx.shape
    assert_parity((True, float(got["cost"][0]), got["residuals"], None, got["jacobian"]),
                  (ok, cost, r, None, j[idx]), "bench --dump-outputs")
