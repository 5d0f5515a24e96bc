#!/usr/bin/env python3
"""What the device-resident PCG (cse_schur_solve) costs against the driver's
torch loop on the host.

At each BAL shape (synthetic; default problem-49-7776 and problem-1778-993923,
problem-13682-4456117 on request), in one process:

  driver   ceres_amd.bundle_adjuster, --num_iterations 4: the "Linear solver"
           timer (host clock around the four solves, synchronised) and the
           ls_iter column, for the host loop and for --device_pcg at
           --pcg_check_period 1, 4 and 16; after one discarded run the legs
           are interleaved, `--rounds` times.  The host loop's code is the
           parent commit's, so it is the baseline.
  kernels  by HIP events on the evaluator's stream, D and b as the driver's
           first LM step: one product (cse_schur_multiply, and
           cse_schur_explicit_multiply where S fits --max_schur_gb), and one
           whole iteration of cse_schur_solve -- the difference of a 40- and a
           20-iteration solve with both stopping tests off, check_period 64,
           over 20 -- so iteration - product is the two vector kernels and
           their launches.

Writes one JSON document to --out and prints it.
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
# two kernels per iteration beside the product's; a reset iteration has three
# and a second product
LAUNCHES = {"implicit": "2 + 4 (SchurDiag, SchurChunk/SchurBig, GradientContrib, GradientChunkReduce)",
            "explicit": "2 + 2 (SchurExplicitRow, SchurExplicitColumn)"}


def event_ms(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def kernels(name, args, explicit_fits):
    import torch
    import ceres_amd as ca
    from ceres_amd import _cse, bal

    dev = torch.device("cuda", 0)
    f64 = torch.float64
    prog = bal.synthetic_program(bal.CONFIGS[name], loss=ca.Loss.huber(1.0))
    ev = ca.Evaluator(prog, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    n, m = prog.num_effective_parameters, prog.num_residuals
    e_cols, f_cols = ev.schur_structure()
    x = torch.from_numpy(prog.state).to(dev)
    cost = torch.zeros(1, dtype=f64, device=dev)
    r = torch.empty(m, dtype=f64, device=dev)
    jac = torch.empty(prog.num_jacobian_values, dtype=f64, device=dev)
    ev.evaluate_device(x.data_ptr(), cost.data_ptr(), r.data_ptr(), None, jac.data_ptr())
    assert ev.wait() == 0
    D = torch.zeros(n, dtype=f64, device=dev)
    ones = torch.ones(m, dtype=f64, device=dev)
    ev.left_multiply_device((jac * jac).data_ptr(), ones.data_ptr(), D.data_ptr())
    D = torch.sqrt(D.clamp_(min=1e-6) / 1e4)
    b = -r
    rhs = torch.empty(f_cols, dtype=f64, device=dev)
    ev.schur_init_device(jac.data_ptr(), D.data_ptr(), b.data_ptr(), rhs.data_ptr(), _cse.SCHUR_JACOBI)
    v = torch.randn(f_cols, dtype=f64, device=dev)
    y = torch.empty(f_cols, dtype=f64, device=dev)
    xf = torch.empty(f_cols, dtype=f64, device=dev)
    out = {"f_cols": f_cols, "observations": int(prog.num_residual_blocks)}
    operators = [("implicit", None)]
    if explicit_fits:
        ev.schur_complement_sparse_upload()
        _, num_blocks, _ = ev.schur_complement_sparse_counts()
        V = torch.empty(81 * num_blocks, dtype=f64, device=dev)
        ev.schur_complement_sparse_device(V.data_ptr())
        operators.append(("explicit", V))
    for label, V in operators:
        if V is None:
            product = lambda: ev.schur_multiply_device(v.data_ptr(), y.data_ptr())
        else:
            product = lambda V=V: ev.schur_explicit_multiply_device(V.data_ptr(), v.data_ptr(), y.data_ptr())

        ran = {}

        def solve(iters, V=V):
            o = _cse.cg_options(min_num_iterations=iters, max_num_iterations=iters, r_tolerance=-1.0,
                                q_tolerance=-1.0, residual_reset_period=iters + 1, check_period=64,
                                flags=_cse.CG_ZERO_INITIAL_GUESS)
            s = ev.schur_solve_device(rhs.data_ptr(), xf.data_ptr(), o, None if V is None else V.data_ptr())
            ran[iters] = (s.num_iterations, s.num_iterations_enqueued, s.reason)

        p = event_ms(torch, product, args.warmup, args.reps)
        t20 = event_ms(torch, lambda: solve(20), 2, args.reps)
        t40 = event_ms(torch, lambda: solve(40), 2, args.reps)
        it = (t40["median_ms"] - t20["median_ms"]) / 20
        out[label] = {"product": p, "solve_20_iterations": t20, "solve_40_iterations": t40,
                      "iterations_run_enqueued_reason": ran, "iteration_ms": it, "vector_kernels_ms": it - p["median_ms"],
                      "launches_per_iteration": LAUNCHES[label]}
    assert ev.wait() == 0
    ev.close()
    return out


def driver_legs(name, args, explicit):
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", name, "--robustify", "--point_sigma", "0.05", "--num_iterations",
            str(args.num_iterations), "--max_schur_gb", str(args.max_schur_gb)]
    if explicit:
        base.append("--use_explicit_schur_complement")
    legs = [("host_loop", [])] + [(f"device_pcg_check_{p}", ["--device_pcg", "--pcg_check_period", str(p)])
                                  for p in (1, 4, 16)]
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
    ap.add_argument("--max_schur_gb", type=float, default=16.0,
                    help="the explicit operator's legs run where the plan, the structure and S fit")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip_driver", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--num_iterations", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("schur_solve_probe: needs a HIP device")
    import ceres_amd as ca
    from ceres_amd import bal
    doc = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for name in args.shapes:
        bal.CONFIGS.setdefault(name, SHAPES[name])
        prog = bal.synthetic_program(bal.CONFIGS[name], loss=ca.Loss.huber(1.0))
        ev = ca.Evaluator(prog, device=0)
        _, _, plan_bytes = ev.schur_complement_plan()
        _, num_blocks, structure_bytes = ev.schur_complement_sparse_counts()
        ev.close()
        del prog
        fits = structure_bytes + plan_bytes + 648 * num_blocks <= args.max_schur_gb * 2 ** 30
        shape = {"shape": name, "explicit_fits": bool(fits), "kernels": kernels(name, args, fits)}
        if not args.skip_driver:
            shape["driver_implicit"] = driver_legs(name, args, False)
            if fits:
                shape["driver_explicit"] = driver_legs(name, args, True)
        doc["shapes"].append(shape)
        text = json.dumps(doc, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
