#!/usr/bin/env python3
"""What the library's dense Cholesky costs against the driver's torch path.

At n = 441 and n = 16,002 (the S of problem-49-7776 and problem-1778-993923),
on the device, with HIP events on the evaluator's stream, medians of --reps
after --warmup calls (DESIGN section 3.6a's protocol), the variants interleaved
in one process:

  fp64_factor, fp64_solve      cse_dense_cholesky_factorize / _solve, FP64
  fp32_factor                  the FP32 factor (the cast of S included)
  fp32_solve_0, fp32_solve_3   the FP32 solve with 0 and 3 refinements
  torch_factor, torch_solve    torch.linalg.cholesky_ex, torch.cholesky_solve:
                               the parent's path (bundle_adjuster.cholesky_solve)

The matrix is B B^T / n + I for a seeded normal B (well conditioned: the
timings do not depend on the values).  The FP64 factor runs in place, so the
matrix is copied back before each call, outside the events.  Launch counts are
the plan's (csrc/plan.cpp, PlanDenseCholesky): 3 T - 2 per factorization
(+ 1 for the FP32 cast), 2 T per forward and backward substitution, T = ceil(n
/ 64).  factor_tflops = n^3 / 3 / time: the trailing update is all but n^2 * 64
of those operations, so this is a lower bound of its rate; the peaks are
MI355X's f64 and f32 matrix-core rates.

--kernel_stats FILE sums a kernel trace per kernel (the CSV that `rocprofv3
--kernel-trace --output-format csv` writes: Kernel_Name, Start_Timestamp,
End_Timestamp), taken in a run of its own with --once (one call of each
variant), into the document; --stats_only writes nothing else.

Then the driver (ceres_amd.bundle_adjuster) runs --linear_solver dense_schur
with both libraries, and with mixed precision, and its "Linear solver" line is
recorded (one discarded run first: the first run of a process pays for torch's
first use of its kernels).

Writes one JSON document to --out and prints it.
"""
import argparse
import contextlib
import csv
import io
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ceres-solver-cuda_amd"))

SHAPES = {441: "problem-49-7776", 16002: "problem-1778-993923"}
CONFIGS = {"problem-49-7776": (49, 7776, 31843), "problem-1778-993923": (1778, 993923, 5001946)}
NB = 64
# MI355X matrix-core peaks, dense, TFLOP/s
PEAK_F64_TFLOPS = 78.6
PEAK_F32_TFLOPS = 157.3


def summary(times):
    times = sorted(times)
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": len(times)}


def probe(n, args):
    import torch
    import ceres_amd as ca
    from ceres_amd import _cse, bal

    dev = torch.device("cuda", 0)
    f64 = torch.float64
    prog = bal.synthetic_program((4, 30, 100), seed=3)
    ev = ca.Evaluator(prog, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(n)
    B = torch.randn((n, n), dtype=f64, device=dev, generator=gen)
    A0 = B @ B.T / n + torch.eye(n, dtype=f64, device=dev)
    del B
    A = A0.clone()
    rhs = torch.randn(n, dtype=f64, device=dev, generator=gen)
    x = torch.empty(n, dtype=f64, device=dev)
    T = (n + NB - 1) // NB
    out = {"n": n, "shape": SHAPES.get(n), "panels": T,
           "launches": {"fp64_factor": 3 * T - 2, "fp32_factor": 3 * T - 1, "fp64_solve": 2 * T + 2,
                        "fp32_solve_0": 1 + (2 * T + 2) + 1, "fp32_solve_3": 1 + 4 * (2 * T + 2) + 3 + 1},
           "workspace_bytes": {"fp64": ca.Evaluator.dense_cholesky_workspace(n, _cse.DENSE_CHOLESKY_FP64),
                               "fp32": ca.Evaluator.dense_cholesky_workspace(n, _cse.DENSE_CHOLESKY_FP32)}}
    try:
        torch.linalg.cholesky_ex(A0[:18, :18].contiguous())
        out["torch_backend"] = "device (torch.linalg.cholesky_ex)"
        have_torch = True
    except RuntimeError as e:
        out["torch_backend"] = "unavailable: " + str(e).splitlines()[0]
        have_torch = False
    state = {}

    def fp64_factor():
        ev.dense_cholesky_factorize_device(A.data_ptr(), n, None, _cse.DENSE_CHOLESKY_FP64)

    def fp32_factor():
        ev.dense_cholesky_factorize_device(A0.data_ptr(), n, None, _cse.DENSE_CHOLESKY_FP32)

    def torch_factor():
        state["L"], _ = torch.linalg.cholesky_ex(A0)

    def torch_solve():
        state["xt"] = torch.cholesky_solve(rhs.unsqueeze(1), state["L"])

    solve = lambda r: (lambda: ev.dense_cholesky_solve_device(rhs.data_ptr(), x.data_ptr(), r))
    # (name, what runs before the events, what is timed), in the order of one round
    legs = [("fp64_factor", lambda: A.copy_(A0), fp64_factor), ("fp64_solve", None, solve(0)),
            ("fp32_factor", None, fp32_factor), ("fp32_solve_0", None, solve(0)), ("fp32_solve_3", None, solve(3))]
    if have_torch:
        legs += [("torch_factor", None, torch_factor), ("torch_solve", None, torch_solve)]
    times = {name: [] for name, _, _ in legs}
    rounds = 1 if args.once else args.warmup + args.reps
    for it in range(rounds):
        for name, before, fn in legs:
            if before:
                before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if args.once or it >= args.warmup:
                times[name].append(a.elapsed_time(b))
        assert ev.dense_cholesky_info() == 0
    for name in times:
        out[name] = summary(times[name])
    # what was timed solves the system
    for name, precision, r in (("fp64", _cse.DENSE_CHOLESKY_FP64, 0), ("fp32_3", _cse.DENSE_CHOLESKY_FP32, 3)):
        A.copy_(A0)
        ev.dense_cholesky_factorize_device(A.data_ptr(), n, None, precision)
        ev.dense_cholesky_solve_device(rhs.data_ptr(), x.data_ptr(), r)
        torch.cuda.synchronize()
        out["relative_residual_" + name] = float(((rhs - A0 @ x).norm() / rhs.norm()).item())
    if have_torch:
        out["relative_residual_torch"] = float(((rhs - A0 @ state["xt"].squeeze(1)).norm() / rhs.norm()).item())
    flops = n ** 3 / 3.0
    out["fp64_factor_tflops"] = flops / (out["fp64_factor"]["median_ms"] * 1e-3) / 1e12
    out["fp32_factor_tflops"] = flops / (out["fp32_factor"]["median_ms"] * 1e-3) / 1e12
    out["fp64_share_of_f64_peak"] = out["fp64_factor_tflops"] / PEAK_F64_TFLOPS
    out["fp32_share_of_f32_peak"] = out["fp32_factor_tflops"] / PEAK_F32_TFLOPS
    if have_torch:
        t = out["torch_factor"]["median_ms"] + out["torch_solve"]["median_ms"]
        out["torch_factor_and_solve_ms"] = t
        out["fp64_over_torch"] = (out["fp64_factor"]["median_ms"] + out["fp64_solve"]["median_ms"]) / t
        out["fp32_3_over_torch"] = (out["fp32_factor"]["median_ms"] + out["fp32_solve_3"]["median_ms"]) / t
    ev.close()
    return out


def driver(name, args):
    from ceres_amd import bal, bundle_adjuster
    added = name not in bal.CONFIGS  # a named shape for this call alone
    if added:
        bal.CONFIGS[name] = CONFIGS[name]
    base = ["--synthetic", name, "--robustify", "--point_sigma", "0.05", "--num_iterations",
            str(args.num_iterations), "--linear_solver", "dense_schur"]
    cse = ["--dense_linear_algebra_library", "cse"]
    mixed = cse + ["--mixed_precision_solves", "--max_num_refinement_iterations", "3"]
    out = {}
    for label, extra in (("warmup_discarded", []), ("torch", []), ("cse", cse), ("cse_mixed_3", mixed),
                         ("torch_again", []), ("cse_again", cse)):
        text = io.StringIO()
        try:
            with contextlib.redirect_stdout(text):
                c0, c1, rows = bundle_adjuster.main(base + extra)
        except SystemExit as e:
            out[label] = {"argv": base + extra, "exit": str(e)}
            continue
        pick = lambda key: [ln.strip() for ln in text.getvalue().splitlines() if ln.strip().startswith(key)]
        out[label] = {"argv": base + extra, "initial_cost": c0, "final_cost": c1,
                      "accepted": [bool(row[7]) for row in rows],
                      "linear_solver_timer": (pick("Linear solver") or [None])[0],
                      "dense_cholesky_timer": (pick("Dense Cholesky") or [None])[0]}
    if added:
        del bal.CONFIGS[name]
    return out


def kernel_stats(path):
    total = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or ""
            if "Dc" not in name:
                continue
            name = name.split("(")[0].replace("void ", "").replace("cse::", "")
            ns = int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
            calls, tot = total.get(name, (0, 0))
            total[name] = (calls + 1, tot + ns)
    return [{"kernel": k, "calls": c, "total_ms": t / 1e6, "average_us": t / c / 1e3}
            for k, (c, t) in sorted(total.items(), key=lambda kv: -kv[1][1])]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", nargs="+", type=int, default=[441, 16002])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true", help="one call of each variant, for a kernel trace")
    ap.add_argument("--skip_driver", action="store_true")
    ap.add_argument("--driver_shapes", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--num_iterations", type=int, default=4)
    ap.add_argument("--kernel_stats", default=None)
    ap.add_argument("--stats_only", action="store_true",
                    help="add --kernel_stats to the document at --out and stop (needs no device)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.stats_only:
        with open(args.out) as f:
            doc = json.load(f)
        doc["kernel_stats"] = {"sizes": args.sizes, "kernels": kernel_stats(args.kernel_stats)}
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("dense_cholesky_probe: needs a HIP device")
    doc = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "panel_width": NB,
           "peaks_tflops": {"f64": PEAK_F64_TFLOPS, "f32": PEAK_F32_TFLOPS}, "sizes": [], "driver": {}}

    def write():
        text = json.dumps(doc, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return text

    for n in args.sizes:
        doc["sizes"].append(probe(n, args))
        write()
    if args.kernel_stats:
        doc["kernel_stats"] = {"sizes": args.sizes, "kernels": kernel_stats(args.kernel_stats)}
    for name in () if args.skip_driver else args.driver_shapes:
        doc["driver"][name] = driver(name, args)
        write()
    print(write())


if __name__ == "__main__":
    main()
