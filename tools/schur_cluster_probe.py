#!/usr/bin/env python3
"""What CLUSTER_JACOBI (cse_schur_cluster_jacobi) costs to build and to apply
against SCHUR_JACOBI, and what it buys a solve.

At each BAL shape (synthetic; default problem-49-7776 and problem-1778-993923),
with the camera partition `blocks` of 4 and of 16 (consecutive runs of that
many cameras), in one process:

  kernels  by HIP events on the evaluator's stream, D and b as the driver's
           first LM step, on one evaluator, interleaved round by round, medians
           of --reps after --warmup calls:
             init_schur_jacobi     cse_schur_init with SCHUR_JACOBI
             init_identity         cse_schur_init with IDENTITY (what precedes
                                   a cluster build)
             cluster_build_<k>     cse_schur_cluster_jacobi: the filtered pair
                                   kernel, the finish, the factor
             apply_schur_jacobi    cse_schur_precondition under SCHUR_JACOBI
                                   (SchurPrecondApplyKernel)
             apply_cluster_<k>     cse_schur_precondition under the clusters
                                   (ClusterApplyKernel)
           plan_s: the host time of cse_schur_set_clusters, which builds and
           uploads the partition's structure.
  driver   ceres_amd.bundle_adjuster --device_pcg, --num_iterations 4, to the
           driver's eta: the "Linear solver" timer (host clock around the
           solves, synchronised) and the ls_iter column for jacobi,
           schur_jacobi and cluster_jacobi with blocks of 4 and 16; after one
           discarded run the legs are interleaved, `--rounds` times.

Writes one JSON document to --out and prints it.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ceres-solver-cuda_amd"))

SHAPES = {
    "problem-49-7776": (49, 7776, 31843),
    "problem-1778-993923": (1778, 993923, 5001946),
}
SIZES = (4, 16)


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
    from ceres_amd import _cse, bal, clustering

    dev = torch.device("cuda", 0)
    f64 = torch.float64
    prog = bal.synthetic_program(bal.CONFIGS[name], loss=ca.Loss.huber(1.0))
    ev = ca.Evaluator(prog, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    n, m = prog.num_effective_parameters, prog.num_residuals
    e_cols, f_cols = ev.schur_structure()
    cameras = f_cols // 9
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
    v = torch.randn(f_cols, dtype=f64, device=dev)
    y = torch.zeros(f_cols, dtype=f64, device=dev)

    def init(precond):
        ev.schur_init_device(jac.data_ptr(), D.data_ptr(), b.data_ptr(), rhs.data_ptr(), precond)

    def apply():
        ev.schur_precondition_device(v.data_ptr(), y.data_ptr())

    out = {"f_cols": f_cols, "cameras": cameras, "observations": int(prog.num_residual_blocks)}
    # The inits and the SCHUR_JACOBI apply.
    times = {"init_schur_jacobi": [], "init_identity": [], "apply_schur_jacobi": []}
    for k in range(args.warmup + args.reps):
        t_sj = event_ms(torch, lambda: init(_cse.SCHUR_SCHUR_JACOBI))
        t_ap = event_ms(torch, apply)
        t_id = event_ms(torch, lambda: init(_cse.SCHUR_IDENTITY))
        if k >= args.warmup:
            times["init_schur_jacobi"].append(t_sj)
            times["apply_schur_jacobi"].append(t_ap)
            times["init_identity"].append(t_id)
    # The cluster build and apply, per size (the evaluator keeps one partition).
    for size in SIZES:
        labels = clustering.blocks(cameras, size)
        t0 = time.perf_counter()
        ev.schur_set_clusters(labels)  # builds and uploads the structure
        out[f"plan_s_{size}"] = time.perf_counter() - t0
        build, app = [], []
        for k in range(args.warmup + args.reps):
            t_b = event_ms(torch, ev.schur_cluster_jacobi_device)
            t_a = event_ms(torch, apply)
            if k >= args.warmup:
                build.append(t_b)
                app.append(t_a)
        times[f"cluster_build_{size}"] = build
        times[f"apply_cluster_{size}"] = app
        out[f"clusters_{size}"] = int(labels.max()) + 1
    assert ev.wait() == 0
    out.update({k: stats(t) for k, t in times.items()})
    ev.close()
    return out


def driver_legs(name, args):
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", name, "--robustify", "--point_sigma", "0.05", "--num_iterations",
            str(args.num_iterations), "--device_pcg"]
    cluster = ["--preconditioner", "cluster_jacobi", "--visibility_clustering", "blocks", "--max_cluster_cameras"]
    legs = [("jacobi", []), ("schur_jacobi", ["--preconditioner", "schur_jacobi"])]
    legs += [(f"cluster_jacobi_{size}", cluster + [str(size)]) for size in SIZES]
    order = [("warmup_discarded", [])] + [(f"{label}_round{k}", extra) for k in range(args.rounds)
                                          for label, extra in legs]
    out = {}
    for label, extra in order:
        print(f"{name}: {label}", file=sys.stderr, flush=True)
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            c0, c1, rows = bundle_adjuster.main(base + extra)
        line = [ln for ln in text.getvalue().splitlines() if ln.strip().startswith("Linear solver")]
        seconds = float(line[0].split()[2]) if line else None
        out[label] = {"argv": base + extra, "final_cost": c1, "ls_iter": [row[6] for row in rows],
                      "accepted": [bool(row[7]) for row in rows], "linear_solver_s": seconds}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--skip_driver", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--num_iterations", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("schur_cluster_probe: needs a HIP device")
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
