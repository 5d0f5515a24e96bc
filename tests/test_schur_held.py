"""CPU: the implicit Schur complement's plan with held (constant) cameras and
the driver flag.

cse::PlanProgram accepts a group with held slot-0 blocks when its active
cameras tile the f columns in id order, and adds the tables that turn a block
into its F cell and a camera id into its rank among the active cameras
(csrc/plan.cpp).  Here, without a GPU: the plan against brute force, and the
refusals, in the stand-alone driver under AddressSanitizer + UBSan
(tests/cpp/schur_held_driver.cpp); the ABI version did not move; and
bundle_adjuster takes --held_cameras with iterative_schur and cgnr alone.
"""
import os
import subprocess

import pytest

from ceres_amd import _cse

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


def test_held_plan_driver_under_asan_ubsan():
    """The stand-alone driver, g++ -fsanitize=address,undefined with static
    runtimes: eligibility, e_cols / f_cols, every chunk's first F-cell rank and
    active mask, the per-perm F cells, the camera ranks, the unheld plan field
    by field, and the refusals (a held point, columns that do not tile)."""
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "schur_held.mk", "driver"])
    out = subprocess.run([os.path.join(CPP, "build", "schur_held_driver")], capture_output=True, text=True)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0
    assert out.stdout.rstrip().endswith("OK")
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    # the cases that matter ran: a chunk with no F cell, a held row on both sides of a stride
    assert "runs, boundaries held" in out.stdout and "refused" in out.stdout


def test_abi_version_is_still_6():
    assert _cse.lib().cse_abi_version() == 6 and _cse.CSE_ABI_VERSION == 6


def test_driver_takes_held_cameras_with_the_implicit_solvers_only():
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", "problem-16-22106"]
    assert bundle_adjuster.parse(base).held_cameras == 0
    args = bundle_adjuster.parse(base + ["--held_cameras", "2"])
    assert args.held_cameras == 2 and args.linear_solver == "iterative_schur"
    for extra in (["--device_pcg"], ["--preconditioner", "schur_jacobi"], ["--preconditioner", "identity"],
                  ["--jacobi_scaling"], ["--linear_solver", "cgnr"]):
        assert bundle_adjuster.parse(base + ["--held_cameras", "3"] + extra).held_cameras == 3
    for extra in (["--linear_solver", "dense_schur"], ["--use_explicit_schur_complement"]):
        with pytest.raises(SystemExit, match="held_cameras"):
            bundle_adjuster.parse(base + ["--held_cameras", "1"] + extra)
        assert bundle_adjuster.parse(base + extra).held_cameras == 0  # the flag alone is still taken
    with pytest.raises(SystemExit, match="held_cameras"):
        bundle_adjuster.parse(base + ["--held_cameras", "-1"])
