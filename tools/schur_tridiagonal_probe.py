#!/usr/bin/env python3
"""What CLUSTER_TRIDIAGONAL (cse_schur_cluster_tridiagonal) costs to build and
to apply against CLUSTER_JACOBI and SCHUR_JACOBI, and what it buys a solve, on
uniform and on local visibility.

At each shape -- the uniform synthetic problem-49-7776 and problem-1778-993923
and banded problems of the same counts with windows of 8 and 16 cameras
(bal.synthetic_banded) -- with the camera partition `blocks` of --size (8)
cameras and the degree-2 maximum spanning forest of its cluster graph, in one
process:

  kernels  by HIP events on the evaluator's stream, D and b as the driver's
           first LM step, on one evaluator, interleaved round by round, medians
           of --reps after --warmup calls:
             init_schur_jacobi      cse_schur_init with SCHUR_JACOBI
             init_identity          cse_schur_init with IDENTITY (what precedes
                                    a cluster build)
             build_cluster_jacobi   cse_schur_cluster_jacobi
             build_tridiagonal      cse_schur_cluster_tridiagonal: the filtered
                                    pair kernel, the finish, both factor launches
             apply_schur_jacobi, apply_cluster_jacobi, apply_tridiagonal
                                    cse_schur_precondition under each
           plan_s_*: the host time of cse_schur_set_clusters and of
           cse_schur_set_cluster_forest; forest_s: the cluster graph and the
           forest in numpy; paths, longest_path, scaled (whether the factor ran
           its second pass).
  driver   ceres_amd.bundle_adjuster --device_pcg, --num_iterations 4, to the
           driver's eta: the "Linear solver" timer and the ls_iter column for
           jacobi, schur_jacobi, cluster_jacobi and cluster_tridiagonal on the
           same partition; after one discarded run the legs are interleaved,
           `--rounds` times.

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
DEFAULT = ["problem-49-7776", "banded-49-7776-31843-w8", "banded-49-7776-31843-w16",
           "problem-1778-993923", "banded-1778-993923-5001946-w8", "banded-1778-993923-5001946-w16"]


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
    import numpy as np
    import torch
    import ceres_amd as ca
    from ceres_amd import _cse, bal, clustering

    dev = torch.device("cuda", 0)
    f64 = torch.float64
    cams, pts, ci, pi, obs = bal.synthetic_named(name)
    prog = bal.program(cams, pts, ci, pi, obs, loss=ca.Loss.huber(1.0))
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
    scaled = torch.zeros(1, dtype=torch.int32, device=dev)

    def init(precond):
        ev.schur_init_device(jac.data_ptr(), D.data_ptr(), b.data_ptr(), rhs.data_ptr(), precond)

    def apply():
        ev.schur_precondition_device(v.data_ptr(), y.data_ptr())

    out = {"f_cols": f_cols, "cameras": cameras, "observations": int(prog.num_residual_blocks),
           "cluster_cameras": args.size}
    labels = clustering.blocks(cameras, args.size)
    sizes = np.bincount(labels)
    t0 = time.perf_counter()
    forest = clustering.degree2_maximum_spanning_forest(len(sizes), *clustering.cluster_graph(ci, pi, labels),
                                                        sizes=sizes)
    out["forest_s"] = time.perf_counter() - t0
    paths = clustering.forest_paths(len(sizes), forest)
    out.update(clusters=len(sizes), forest_edges=len(forest), paths=len(paths),
               longest_path=max(len(p) for p in paths))
    t0 = time.perf_counter()
    ev.schur_set_clusters(labels)
    out["plan_s_clusters"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    ev.schur_set_cluster_forest(forest)
    out["plan_s_forest"] = time.perf_counter() - t0
    names = ("init_schur_jacobi", "apply_schur_jacobi", "init_identity", "build_cluster_jacobi",
             "apply_cluster_jacobi", "build_tridiagonal", "apply_tridiagonal")
    times = {k: [] for k in names}
    for k in range(args.warmup + args.reps):
        t = [event_ms(torch, lambda: init(_cse.SCHUR_SCHUR_JACOBI)), event_ms(torch, apply),
             event_ms(torch, lambda: init(_cse.SCHUR_IDENTITY)),
             event_ms(torch, ev.schur_cluster_jacobi_device), event_ms(torch, apply),
             event_ms(torch, lambda: ev.schur_cluster_tridiagonal_device(None, scaled.data_ptr())),
             event_ms(torch, apply)]
        if k >= args.warmup:
            for key, value in zip(names, t):
                times[key].append(value)
    out["status"] = int(ev.wait())
    out["scaled"] = int(scaled.item())
    out.update({k: stats(t) for k, t in times.items()})
    ev.close()
    return out


def driver_legs(name, args):
    from ceres_amd import bundle_adjuster
    base = ["--synthetic", name, "--robustify", "--point_sigma", "0.05", "--num_iterations",
            str(args.num_iterations), "--device_pcg"]
    blocks = ["--visibility_clustering", "blocks", "--max_cluster_cameras", str(args.size)]
    legs = [("jacobi", []), ("schur_jacobi", ["--preconditioner", "schur_jacobi"]),
            ("cluster_jacobi", ["--preconditioner", "cluster_jacobi"] + blocks),
            ("cluster_tridiagonal", ["--preconditioner", "cluster_tridiagonal"] + blocks)]
    order = [("warmup_discarded", [])] + [(f"{label}_round{k}", extra) for k in range(args.rounds)
                                          for label, extra in legs]
    out = {}
    for label, extra in order:
        print(f"{name}: {label}", file=sys.stderr, flush=True)
        text, stats_ = io.StringIO(), {}
        with contextlib.redirect_stdout(text):
            c0, c1, rows = bundle_adjuster.main(base + extra, stats_)
        line = [ln for ln in text.getvalue().splitlines() if ln.strip().startswith("Linear solver")]
        seconds = float(line[0].split()[2]) if line else None
        out[label] = {"argv": base + extra, "final_cost": c1, "ls_iter": [row[6] for row in rows],
                      "accepted": [bool(row[7]) for row in rows], "linear_solver_s": seconds}
        if "scaled_solves" in stats_:
            out[label]["scaled_solves"] = list(stats_["scaled_solves"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", nargs="+", default=DEFAULT)
    ap.add_argument("--size", type=int, default=8, help="cameras a cluster (blocks)")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--skip_driver", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--num_iterations", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("schur_tridiagonal_probe: needs a HIP device")
    from ceres_amd import bal
    for name, counts in SHAPES.items():
        bal.CONFIGS.setdefault(name, counts)
    doc = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for name in args.shapes:
        bal.synthetic_name(name)
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
