#!/usr/bin/env python3
"""What cse_jacobian_squared_column_norm and cse_jacobian_scale_columns cost.

At each BAL shape (synthetic; default problem-1778-993923 and
problem-13682-4456117) and Jacobian layout, in one process, by HIP events on
the evaluator's stream, after a warm-up of every timed call, the legs of a
comparison interleaved:

  norm    the new call against the parent commit's way to the same vector:
          torch.mul(jac, jac, out=jac2), a zero fill and
          cse_jacobian_left_multiply with a vector of ones; the device memory
          the second way needs on top (jac2);
  scale   the call's time and its fraction of 8 TB/s on its algorithmic bytes
          (the Jacobian once in and once out, the ids, the scale vector),
          beside a plain in-place torch mul_ over the same buffer: the copy
          ceiling of the same box.  The scale vector holds 0.5 and 2.0 and is
          swapped with its reciprocal every call, so the values stay finite.
  driver  (first shape only) ceres_amd.bundle_adjuster --num_iterations 4 with
          and without --jacobi_scaling: its timers.

Writes one JSON document to --out and prints it.
"""
import argparse
import contextlib
import io
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ceres-solver-cuda_amd"))

DEFAULT_SHAPES = ["problem-1778-993923", "problem-13682-4456117"]
PEAK_BYTES_PER_S = 8e12  # HBM, datasheet


def interleaved_ms(torch, legs, warmup, reps):
    """legs: {name: fn}.  Every leg warmed up, then `reps` rounds of all legs in turn."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    out = {}
    for k, t in times.items():
        t.sort()
        out[k] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "reps": reps}
    return out


def kernels(name, fmt_name, args):
    import torch
    import ceres_amd as ca
    from ceres_amd import bal

    dev = torch.device("cuda", 0)
    f64 = torch.float64
    fmt = ca.BLOCK_SPARSE if fmt_name == "block_sparse" else ca.COMPRESSED_ROW
    prog = bal.synthetic_program(bal.CONFIGS[name], loss=ca.Loss.huber(1.0), format=fmt)
    ev = ca.Evaluator(prog, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    n, m, nv = prog.num_effective_parameters, prog.num_residuals, prog.num_jacobian_values
    x = torch.from_numpy(prog.state).to(dev)
    cost = torch.zeros(1, dtype=f64, device=dev)
    r = torch.empty(m, dtype=f64, device=dev)
    jac = torch.empty(nv, dtype=f64, device=dev)
    ev.evaluate_device(x.data_ptr(), cost.data_ptr(), r.data_ptr(), None, jac.data_ptr())
    assert ev.wait() == 0
    out = {"observations": int(prog.num_residual_blocks), "num_jacobian_values": int(nv),
           "jacobian_bytes": 8 * int(nv), "columns": int(n)}

    # ---- norm
    D_new = torch.empty(n, dtype=f64, device=dev)
    D_old = torch.empty(n, dtype=f64, device=dev)
    ones = torch.ones(m, dtype=f64, device=dev)
    before = torch.cuda.memory_allocated(dev)
    jac2 = torch.empty_like(jac)
    out["norm_parent_extra_device_bytes"] = int(torch.cuda.memory_allocated(dev) - before)

    def parent_way():
        torch.mul(jac, jac, out=jac2)
        D_old.zero_()
        ev.left_multiply_device(jac2.data_ptr(), ones.data_ptr(), D_old.data_ptr())

    out["norm"] = interleaved_ms(torch, {
        "cse_jacobian_squared_column_norm": lambda: ev.squared_column_norm_device(jac.data_ptr(), D_new.data_ptr()),
        "parent_mul_and_left_multiply": parent_way}, args.warmup, args.reps)
    torch.cuda.synchronize()
    rel = ((D_new - D_old).abs() / D_old.clamp(min=1e-300)).max().item()
    out["norm_max_relative_difference_to_parent_way"] = rel
    del jac2

    # ---- scale
    scale = torch.where(torch.rand(n, device=dev) < 0.5, 0.5, 2.0).to(f64)
    inv = 1.0 / scale
    flip = {"k": 0, "t": 0}

    def scale_call():
        s = scale if flip["k"] % 2 == 0 else inv
        flip["k"] += 1
        ev.scale_columns_device(jac.data_ptr(), s.data_ptr())

    def torch_mul():
        c = 2.0 if flip["t"] % 2 == 0 else 0.5
        flip["t"] += 1
        jac.mul_(c)

    reps = args.reps + args.reps % 2  # an even number of calls restores the values
    warm = args.warmup + args.warmup % 2
    t = interleaved_ms(torch, {"cse_jacobian_scale_columns": scale_call, "torch_mul_in_place": torch_mul},
                       warm, reps)
    nb = len(prog.groups[0].ids[0])
    alg = 2 * 8 * int(nv) + 4 * nb * int(prog.num_residual_blocks) + 8 * int(n)
    t["algorithmic_bytes"] = alg
    for k in ("cse_jacobian_scale_columns", "torch_mul_in_place"):
        byts = alg if k.startswith("cse") else 2 * 8 * int(nv)
        t[k]["TB_per_s"] = byts / (t[k]["median_ms"] * 1e-3) / 1e12
        t[k]["fraction_of_8TBps"] = byts / (t[k]["median_ms"] * 1e-3) / PEAK_BYTES_PER_S
    out["scale"] = t
    ev.close()
    return out


def driver(name, args):
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", name, "--robustify", "--point_sigma", "0.05", "--num_iterations", "4"]
    out = {}
    for label, extra in (("discarded", []), ("off", []), ("on", ["--jacobi_scaling"]), ("off_2", []),
                         ("on_2", ["--jacobi_scaling"])):
        print(f"driver {name} {label} ...", file=sys.stderr, flush=True)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            c0, c1, rows = bundle_adjuster.main(base + extra)
        if label == "discarded":
            continue
        timers = {k.strip(): (float(v), int(c)) for k, v, c in
                  re.findall(r"^  (.{34})\s*([0-9.]+) \((\d+)\)$", buf.getvalue(), flags=re.M)}
        loop = sum(v for k, (v, _) in timers.items() if k != "Preprocessor")
        out[label] = {"timers_s": timers, "loop_s_per_iteration": loop / len(rows),
                      "column_ops_share": (timers.get("Jacobi scaling", (0, 0))[0] +
                                           timers.get("LM diagonal", (0, 0))[0]) / loop,
                      "final_cost": c1, "accepted": [bool(r[-1]) for r in rows]}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", nargs="*", default=DEFAULT_SHAPES)
    ap.add_argument("--formats", nargs="*", default=["block_sparse", "compressed_row"])
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no_driver", action="store_true")
    ap.add_argument("--out", default="column_ops_probe.json")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("column_ops_probe needs a HIP device")
    doc = {"device": torch.cuda.get_device_name(0), "shapes": {}}
    for name in args.shapes:
        doc["shapes"][name] = {}
        for f in args.formats:
            print(f"{name} {f} ...", file=sys.stderr, flush=True)
            doc["shapes"][name][f] = kernels(name, f, args)
    if not args.no_driver and args.shapes:
        doc["driver"] = {args.shapes[0]: driver(args.shapes[0], args)}
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
