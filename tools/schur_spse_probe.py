#!/usr/bin/env python3
"""What a term of the power series expansion (cse_schur_power_series) costs
against one product, and what the series buys a solve.

At each BAL shape (synthetic; default problem-49-7776 and problem-1778-993923,
problem-13682-4456117 on request), in one process:

  kernels  by HIP events on the evaluator's stream, D and b as the driver's
           first LM step, on one evaluator, interleaved round by round: one
           product (cse_schur_multiply) and one term of the series -- the
           difference of a 12- and a 2-term series with tolerance 0, over 10:
           the kSchurSeries point pass, the zeroing of t, the contribution
           reduce and the fused block apply.  A term moves a product's bytes
           plus 648 bytes per camera of blocks, so it should equal the product
           within the spread of the product's own repeats, which is reported.
  driver   ceres_amd.bundle_adjuster --device_pcg, --num_iterations 4, to the
           driver's eta: the "Linear solver" timer (host clock around the four
           solves, synchronised) and the ls_iter column for jacobi,
           schur_jacobi, schur_power_series_expansion with
           --max_num_spse_iterations 1, 2 and 5, and jacobi from the series'
           start (--use_spse_initialization); after one discarded run the legs
           are interleaved, `--rounds` times.  products = what a solve's
           iterations cost in S-product passes: ls_iter x (1 + m).

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


def event_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(times):
    t = sorted(times)
    return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "reps": len(t)}


def kernels(name, args):
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
    legs = {
        "product": lambda: ev.schur_multiply_device(v.data_ptr(), y.data_ptr()),
        "series_2_terms": lambda: ev.schur_power_series_device(v.data_ptr(), y.data_ptr(), 2, 0.0),
        "series_12_terms": lambda: ev.schur_power_series_device(v.data_ptr(), y.data_ptr(), 12, 0.0),
    }
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            times[k].append(event_ms(torch, fn))
    out = {"f_cols": f_cols, "observations": int(prog.num_residual_blocks)}
    out.update({k: stats(t) for k, t in times.items()})
    term = [(b12 - b2) / 10 for b2, b12 in zip(times["series_2_terms"], times["series_12_terms"])]
    out["term"] = stats(term)
    p = out["product"]
    out["product_spread_ms"] = p["max_ms"] - p["min_ms"]
    out["term_minus_product_ms"] = out["term"]["median_ms"] - p["median_ms"]
    out["block_bytes"] = 648 * (f_cols // 9)
    assert ev.wait() == 0
    ev.close()
    return out


def driver_legs(name, args):
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", name, "--robustify", "--point_sigma", "0.05", "--num_iterations",
            str(args.num_iterations), "--device_pcg"]
    series = ["--preconditioner", "schur_power_series_expansion", "--max_num_spse_iterations"]
    legs = [("jacobi", [], 0), ("schur_jacobi", ["--preconditioner", "schur_jacobi"], 0)]
    legs += [(f"spse_{m}", series + [str(m)], m) for m in (1, 2, 5)]
    legs += [("jacobi_spse_start", ["--use_spse_initialization"], 0)]
    order = [("warmup_discarded", [], 0)] + [(f"{label}_round{k}", extra, m) for k in range(args.rounds)
                                             for label, extra, m in legs]
    out = {}
    for label, extra, m in order:
        print(f"{name}: {label}", file=sys.stderr, flush=True)
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            c0, c1, rows = bundle_adjuster.main(base + extra)
        line = [ln for ln in text.getvalue().splitlines() if ln.strip().startswith("Linear solver")]
        seconds = float(line[0].split()[2]) if line else None
        its = [row[6] for row in rows]
        out[label] = {"argv": base + extra, "final_cost": c1, "ls_iter": its, "linear_solver_s": seconds,
                      "products": sum(its) * (1 + m)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES, choices=list(SHAPES))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip_driver", action="store_true")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--num_iterations", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("schur_spse_probe: needs a HIP device")
    from ceres_amd import bal
    doc = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for name in args.shapes:
        bal.CONFIGS.setdefault(name, SHAPES[name])
        shape = {"shape": name, "kernels": kernels(name, args)}
        if not args.skip_driver:
            shape["driver_device_pcg"] = driver_legs(name, args)
        doc["shapes"].append(shape)
        text = json.dumps(doc, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
