#!/usr/bin/env python3
"""What CGNR on the device (cse_cgnr_init, cse_cgnr_solve) costs against the
pieces it replaces.

At each BAL shape (synthetic; default problem-49-7776 and problem-1778-993923,
problem-13682-4456117 on request), in one process:

  kernels  by HIP events on the evaluator's stream, medians, the contenders
           interleaved round by round; D and b as the driver's first LM step:
             column_norm   cse_jacobian_squared_column_norm (the traversal the
                           block Gram follows, with S sums where that has
                           S (S + 1) / 2)
             init_jacobi   cse_cgnr_init(J, D, b, rhs, JACOBI): J^T b, the Gram,
                           AddDiagonalAndInvert
             init_identity cse_cgnr_init(J, D, b, rhs, IDENTITY): J^T b alone
             product       one cse_cgnr_multiply (with its zero fill)
             iteration     one whole iteration of cse_cgnr_solve -- the
                           difference of a 40- and a 20-iteration solve with
                           both stopping tests off, check_period 64, over 20 --
                           so iteration - product is the vector kernels (four
                           sliced kernels, and the block apply under JACOBI) and
                           their launches
  driver   ceres_amd.bundle_adjuster --linear_solver cgnr, --num_iterations 4:
           the "Linear solver" timer (host clock around the four solves,
           synchronised) and the ls_iter column, for the host loop and for
           --device_cgnr at --cgnr_check_period 1 and 4; after one discarded
           run the legs are interleaved, `--rounds` times.  The host loop's
           code is the parent commit's, so it is the baseline; its
           preconditioner is the scalar one, so the iteration counts differ.

Writes one JSON document to --out (default profiles/cgnr_solve/probe.json)
and prints it.
"""
import argparse
import contextlib
import io
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ceres-solver-cuda_amd"))

SHAPES = {
    "problem-49-7776": (49, 7776, 31843),
    "problem-1778-993923": (1778, 993923, 5001946),
    "problem-13682-4456117": (13682, 4456117, 28987644),
}
DEFAULT_SHAPES = ["problem-49-7776", "problem-1778-993923"]


def interleaved_ms(torch, legs, warmup, reps):
    """legs: {name: fn}.  One timed call of every leg per round, in turn."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    out = {}
    for name, t in times.items():
        t.sort()
        out[name] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "reps": reps}
    return out


def kernels(name, args):
    import torch
    import ceres_amd as ca
    from ceres_amd import _cse, bal

    dev = torch.device("cuda", 0)
    f64 = torch.float64
    prog = bal.synthetic_program(bal.CONFIGS[name], loss=ca.Loss.huber(1.0))
    ev = ca.Evaluator(prog, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    n, m = prog.num_effective_parameters, prog.num_residuals
    x = torch.from_numpy(prog.state).to(dev)
    cost = torch.zeros(1, dtype=f64, device=dev)
    r = torch.empty(m, dtype=f64, device=dev)
    jac = torch.empty(prog.num_jacobian_values, dtype=f64, device=dev)
    ev.evaluate_device(x.data_ptr(), cost.data_ptr(), r.data_ptr(), None, jac.data_ptr())
    assert ev.wait() == 0
    D = torch.zeros(n, dtype=f64, device=dev)
    ev.squared_column_norm_device(jac.data_ptr(), D.data_ptr())
    D = torch.sqrt(D.clamp_(min=1e-6) / 1e4)
    b = -r
    rhs = torch.empty(n, dtype=f64, device=dev)
    norm = torch.empty(n, dtype=f64, device=dev)
    v = torch.randn(n, dtype=f64, device=dev)
    y = torch.empty(n, dtype=f64, device=dev)
    xs = torch.empty(n, dtype=f64, device=dev)
    out = {"num_effective_parameters": n, "observations": int(prog.num_residual_blocks),
           "slices": (n + 2047) // 2048}

    def product():
        y.zero_()
        ev.cgnr_multiply_device(jac.data_ptr(), D.data_ptr(), v.data_ptr(), y.data_ptr())

    out["init"] = interleaved_ms(torch, {
        "column_norm": lambda: ev.squared_column_norm_device(jac.data_ptr(), norm.data_ptr()),
        "init_jacobi": lambda: ev.cgnr_init_device(jac.data_ptr(), D.data_ptr(), b.data_ptr(), rhs.data_ptr(),
                                                   _cse.CGNR_JACOBI),
        "init_identity": lambda: ev.cgnr_init_device(jac.data_ptr(), D.data_ptr(), b.data_ptr(), rhs.data_ptr(),
                                                     _cse.CGNR_IDENTITY),
    }, args.warmup, args.reps)
    for label, pre in (("jacobi", _cse.CGNR_JACOBI), ("identity", _cse.CGNR_IDENTITY)):
        ev.cgnr_init_device(jac.data_ptr(), D.data_ptr(), b.data_ptr(), rhs.data_ptr(), pre)
        ran = {}

        def solve(iters):
            o = _cse.cg_options(min_num_iterations=iters, max_num_iterations=iters, r_tolerance=-1.0,
                                q_tolerance=-1.0, residual_reset_period=iters + 1, check_period=64,
                                flags=_cse.CG_ZERO_INITIAL_GUESS)
            s = ev.cgnr_solve_device(rhs.data_ptr(), xs.data_ptr(), o)
            ran[iters] = (s.num_iterations, s.num_iterations_enqueued, s.reason)

        t = interleaved_ms(torch, {"product": product, "solve_20_iterations": lambda: solve(20),
                                   "solve_40_iterations": lambda: solve(40)}, 2, args.reps)
        it = (t["solve_40_iterations"]["median_ms"] - t["solve_20_iterations"]["median_ms"]) / 20
        t.update(iterations_run_enqueued_reason=ran, iteration_ms=it,
                 vector_kernels_ms=it - t["product"]["median_ms"])
        out[label] = t
    assert ev.wait() == 0
    ev.close()
    return out


def driver_legs(name, args):
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", name, "--robustify", "--point_sigma", "0.05", "--num_iterations",
            str(args.num_iterations), "--linear_solver", "cgnr"]
    legs = [("host_loop", [])] + [(f"device_cgnr_check_{p}", ["--device_cgnr", "--cgnr_check_period", str(p)])
                                  for p in (1, 4)]
    order = [("warmup_discarded", [])] + [(f"{label}_round{k}", extra) for k in range(args.rounds)
                                          for label, extra in legs]
    out = {}
    for label, extra in order:
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            c0, c1, rows = bundle_adjuster.main(base + extra)
        line = [ln for ln in text.getvalue().splitlines() if ln.strip().startswith("Linear solver")]
        seconds = float(line[0].split()[2]) if line else None
        out[label] = {"argv": base + extra, "final_cost": c1, "ls_iter": [row[6] for row in rows],
                      "linear_solver_s": seconds,
                      "ms_per_iteration": 1e3 * seconds / max(1, sum(row[6] for row in rows))}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES, choices=list(SHAPES))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip_driver", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--num_iterations", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cgnr_solve", "probe.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("cgnr_solve_probe: needs a HIP device")
    from ceres_amd import bal
    doc = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for name in args.shapes:
        bal.CONFIGS.setdefault(name, SHAPES[name])
        shape = {"shape": name, "kernels": kernels(name, args)}
        if not args.skip_driver:
            shape["driver"] = driver_legs(name, args)
        doc["shapes"].append(shape)
        text = json.dumps(doc, indent=1)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
