#!/usr/bin/env python3
"""What a held camera costs the implicit Schur operators.

At a BAL shape (synthetic; default problem-13682-4456117), two evaluators in one
process -- every camera free, and camera 0 held constant -- each with its own
Jacobian, D and b as the driver's first LM step.  cse_schur_init (JACOBI),
cse_schur_multiply and cse_schur_back_substitute are timed per call by HIP
events on the evaluator's stream, the two evaluators interleaved round by
round (`--rounds` rounds of `--reps` calls each after a warm-up), so that both
see the same clocks.  The unheld legs run the kernels the parent commit ran;
the held legs run the kHeld instantiations (csrc/schur_kernels.hpp).

Writes one JSON document to --out and prints it.
"""
import argparse
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


def event_ms(torch, fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def bound(name, held):
    """An evaluator with its Schur operators bound, and the calls to time."""
    import torch
    import ceres_amd as ca
    from ceres_amd import _cse, bal

    dev = torch.device("cuda", 0)
    f64 = torch.float64
    prog = bal.synthetic_program(SHAPES[name], loss=ca.Loss.huber(1.0), constant_cameras=range(held))
    ev = ca.Evaluator(prog, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    n, m = prog.num_effective_parameters, prog.num_residuals
    e_cols, f_cols = ev.schur_structure()
    x = torch.from_numpy(prog.state).to(dev)
    cost = torch.zeros(1, dtype=f64, device=dev)
    r = torch.empty(m, dtype=f64, device=dev)
    jac = torch.empty(prog.num_jacobian_values, dtype=f64, device=dev)
    ev.evaluate_device(x.data_ptr(), cost.data_ptr(), r.data_ptr(), None, jac.data_ptr())
    assert ev.wait() == 0
    D = torch.empty(n, dtype=f64, device=dev)
    ev.squared_column_norm_device(jac.data_ptr(), D.data_ptr())
    D = torch.sqrt(D.clamp_(min=1e-6) / 1e4)
    b = -r
    rhs = torch.empty(f_cols, dtype=f64, device=dev)
    v = torch.randn(f_cols, dtype=f64, device=dev)
    y = torch.empty(f_cols, dtype=f64, device=dev)
    step = torch.empty(n, dtype=f64, device=dev)
    keep = (prog, x, cost, r, jac, D, b, rhs, v, y, step)
    calls = {
        "init": lambda: ev.schur_init_device(jac.data_ptr(), D.data_ptr(), b.data_ptr(), rhs.data_ptr(),
                                             _cse.SCHUR_JACOBI),
        "multiply": lambda: ev.schur_multiply_device(v.data_ptr(), y.data_ptr()),
        "back_substitute": lambda: ev.schur_back_substitute_device(v.data_ptr(), step.data_ptr()),
    }
    calls["init"]()
    assert ev.wait() == 0
    return ev, calls, {"f_cols": f_cols, "observations": int(prog.num_residual_blocks)}, keep


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shape", default="problem-13682-4456117", choices=list(SHAPES))
    ap.add_argument("--held", type=int, default=1, help="cameras 0 .. N-1 held in the held leg")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("schur_held_probe: needs a HIP device")
    legs = {"unheld": bound(args.shape, 0), "held": bound(args.shape, args.held)}
    times = {leg: {op: [] for op in ("init", "multiply", "back_substitute")} for leg in legs}
    for leg, (ev, calls, _, _) in legs.items():
        for fn in calls.values():
            for _ in range(args.warmup):
                fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for op in ("init", "multiply", "back_substitute"):
            for leg, (ev, calls, _, _) in legs.items():
                times[leg][op] += event_ms(torch, calls[op], args.reps)
    doc = {"device": torch.cuda.get_device_name(0), "shape": args.shape, "held_cameras": args.held,
           "rounds": args.rounds, "reps": args.reps}
    for leg, (ev, calls, info, _) in legs.items():
        assert ev.wait() == 0
        doc[leg] = dict(info)
        for op, t in times[leg].items():
            t = sorted(t)
            doc[leg][op] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "calls": len(t)}
        ev.close()
    doc["held_over_unheld_median"] = {op: doc["held"][op]["median_ms"] / doc["unheld"][op]["median_ms"]
                                      for op in ("init", "multiply", "back_substitute")}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
