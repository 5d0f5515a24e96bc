"""Per-block loss objects through the C++ ProblemCUDA facade
(EvaluatorCUDA::Options::merge_loss_parameters): tests/cpp/test_per_block_loss.cpp,
built with g++ against libcse.so and the oracle (tests/cpp/per_block_loss.mk),
runs its parity checks on the GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")


def build():
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "per_block_loss.mk", "facade"])
    return os.path.join(CPP, "build", "test_per_block_loss")


def test_facade_test_builds_and_links():
    assert os.access(build(), os.X_OK)


@pytest.mark.gpu
def test_facade_merges_per_block_losses(gpu):
    """300 Snavely blocks, each with its own ScaledLossCUDA<HuberLossCUDA>:
    one group and oracle parity with merge_loss_parameters, the 12 groups of
    the distinct values without."""
    exe = build()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "OK" in out.stdout
