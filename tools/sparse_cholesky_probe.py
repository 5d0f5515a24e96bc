#!/usr/bin/env python3
"""What the library's block-sparse Cholesky costs against its dense one.

On the S of three problems -- banded-1778-993923-5001946-w16 (local
visibility: S is a band), problem-49-7776 and problem-1778-993923 (uniform
visibility: S is full) -- built on the device by cse_schur_complement_sparse
from the problem's first Jacobian (lambda = 1e-4):

  analysis                     cse_sparse_cholesky_analyze on the host, once
                               per ordering (wall clock)
  sparse_factor, sparse_solve  cse_sparse_cholesky_factorize / _solve
  sparse_solve_1               the solve with one refinement
  dense_factor, dense_solve    cse_dense_cholesky_factorize / _solve (FP64) on
                               the dense S of the same problem
                               (cse_schur_complement)

with HIP events on the evaluator's stream, medians of --reps after --warmup
calls, the variants interleaved in one process.  A factorization that takes
longer than --slow_ms is timed --slow_reps times.  The level and launch counts
are the plan's: a factorization is the gather, per level the diagonal kernel
and (where the level has off-diagonal blocks) the target kernel, and the info
reduce; a solve is load, one kernel per level forward and backward, store.

Then the driver (ceres_amd.bundle_adjuster) runs --linear_solver sparse_schur
against dense_schur --dense_linear_algebra_library cse, and on the banded shape
against iterative_schur --preconditioner cluster_tridiagonal, and its "Linear
solver" line is recorded (one discarded run first).

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

CONFIGS = {"problem-49-7776": (49, 7776, 31843), "problem-1778-993923": (1778, 993923, 5001946)}
SHAPES = ["banded-1778-993923-5001946-w16", "problem-49-7776", "problem-1778-993923"]


def summary(times):
    times = sorted(times)
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": len(times)}


def timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(legs, args, torch):
    """legs: (name, fn); the first leg's first time decides the repetitions."""
    times = {name: [] for name, _ in legs}
    first = timed(legs[0][1], torch)
    slow = first > args.slow_ms
    warmup, reps = (0, args.slow_reps) if slow else (args.warmup, args.reps)
    for it in range(warmup + reps):
        for name, fn in legs:
            t = timed(fn, torch)
            if it >= warmup:
                times[name].append(t)
    return {name: summary(ts) for name, ts in times.items()}


def probe(name, args):
    import numpy as np
    import torch
    import ceres_amd as ca
    from ceres_amd import _cse, bal

    dev = torch.device("cuda", 0)
    f64 = torch.float64
    added = name in CONFIGS and name not in bal.CONFIGS
    if added:
        bal.CONFIGS[name] = CONFIGS[name]
    prog = bal.synthetic_program(name, loss=ca.Loss.huber(1.0))
    if added:
        del bal.CONFIGS[name]
    ev = ca.Evaluator(prog, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    n, m = prog.num_effective_parameters, prog.num_residuals
    x = torch.from_numpy(prog.state).to(dev)
    cost = torch.zeros(1, dtype=f64, device=dev)
    r = torch.empty(m, dtype=f64, device=dev)
    jac = torch.empty(prog.num_jacobian_values, dtype=f64, device=dev)
    ev.evaluate_device(x.data_ptr(), cost.data_ptr(), r.data_ptr(), None, jac.data_ptr())
    assert ev.wait() == 0
    e_cols, f_cols = ev.schur_structure()
    D = torch.zeros(n, dtype=f64, device=dev)
    ev.left_multiply_device((jac * jac).data_ptr(), torch.ones(m, dtype=f64, device=dev).data_ptr(), D.data_ptr())
    sqrt_lam_d = torch.sqrt(1e-4 * D.clamp_(min=1e-6))
    rhs = torch.empty(f_cols, dtype=f64, device=dev)
    neg_r = -r
    ev.schur_init_device(jac.data_ptr(), sqrt_lam_d.data_ptr(), neg_r.data_ptr(), rhs.data_ptr(), _cse.SCHUR_IDENTITY)
    row_begin, block_col, _ = ev.schur_complement_sparse_structure()
    values = torch.empty(81 * len(block_col), dtype=f64, device=dev)
    ev.schur_complement_sparse_device(values.data_ptr())
    xs = torch.empty(f_cols, dtype=f64, device=dev)
    out = {"shape": name, "cameras": len(row_begin) - 1, "f_cols": f_cols, "orderings": {}}
    for label, ordering in (("minimum_degree", _cse.SPARSE_ORDERING_MINIMUM_DEGREE),
                            ("natural", _cse.SPARSE_ORDERING_NATURAL)):
        t0 = time.perf_counter()
        s = ev.sparse_cholesky_analyze(row_begin, block_col, ordering)
        analysis_ms = 1e3 * (time.perf_counter() - t0)
        level = ev.sparse_cholesky_structure()[4]
        parent_levels = int(level.max()) + 1
        target_levels = int(np.count_nonzero(np.bincount(level[ev.sparse_cholesky_structure()[3] >= 0],
                                                         minlength=parent_levels)))
        doc = {"analysis_ms": analysis_ms, "num_input_blocks": s.num_input_blocks,
               "num_factor_blocks": s.num_factor_blocks, "num_block_products": s.num_block_products,
               "device_bytes": s.device_bytes, "num_levels": s.num_levels, "max_level_columns": s.max_level_columns,
               "launches": {"factor": 2 + s.num_levels + target_levels, "solve": 2 + 2 * s.num_levels,
                            "solve_1": 2 + 2 * s.num_levels + 1 + 2 * s.num_levels + 2}}
        legs = [("sparse_factor", lambda: ev.sparse_cholesky_factorize_device(values.data_ptr())),
                ("sparse_solve", lambda: ev.sparse_cholesky_solve_device(rhs.data_ptr(), xs.data_ptr(), 0)),
                ("sparse_solve_1", lambda: ev.sparse_cholesky_solve_device(rhs.data_ptr(), xs.data_ptr(), 1))]
        doc.update(measure(legs, args, torch))
        assert ev.sparse_cholesky_info() == 0
        ev.sparse_cholesky_solve_device(rhs.data_ptr(), xs.data_ptr(), 0)
        y = torch.empty_like(xs)
        ev.schur_explicit_multiply_device(values.data_ptr(), xs.data_ptr(), y.data_ptr())
        doc["relative_residual"] = float(((rhs - y).norm() / rhs.norm()).item())
        out["orderings"][label] = doc
    # the dense factorization of the same S
    S = torch.empty((f_cols, f_cols), dtype=f64, device=dev)
    S0 = torch.empty_like(S)
    ev.schur_complement_device(S0.data_ptr())
    xd = torch.empty(f_cols, dtype=f64, device=dev)

    def dense_factor():
        ev.dense_cholesky_factorize_device(S.data_ptr(), f_cols)

    S.copy_(S0)
    times = {"dense_factor": [], "dense_solve": []}
    for it in range(args.warmup + args.reps):
        S.copy_(S0)
        tf = timed(dense_factor, torch)
        ts = timed(lambda: ev.dense_cholesky_solve_device(rhs.data_ptr(), xd.data_ptr(), 0), torch)
        if it >= args.warmup:
            times["dense_factor"].append(tf)
            times["dense_solve"].append(ts)
    assert ev.dense_cholesky_info() == 0
    out.update({k: summary(v) for k, v in times.items()})
    out["dense_bytes"] = 8 * f_cols * f_cols
    out["relative_difference_to_dense"] = float(((xs - xd).norm() / xd.norm()).item())
    ev.close()
    return out


def driver(name, args):
    from ceres_amd import bal, bundle_adjuster
    added = name in CONFIGS and name not in bal.CONFIGS
    if added:
        bal.CONFIGS[name] = CONFIGS[name]
    base = ["--synthetic", name, "--robustify", "--point_sigma", "0.05", "--num_iterations", str(args.num_iterations)]
    sparse = ["--linear_solver", "sparse_schur"]
    dense = ["--linear_solver", "dense_schur", "--dense_linear_algebra_library", "cse"]
    runs = [("warmup_discarded", sparse), ("sparse_schur", sparse),
            ("sparse_schur_natural", sparse + ["--sparse_ordering", "natural"]), ("dense_schur_cse", dense)]
    if name.startswith("banded"):
        runs.append(("iterative_schur_cluster_tridiagonal",
                     ["--linear_solver", "iterative_schur", "--preconditioner", "cluster_tridiagonal",
                      "--visibility_clustering", "blocks"]))
    out = {}
    for label, extra in runs:
        text = io.StringIO()
        try:
            with contextlib.redirect_stdout(text):
                c0, c1, rows = bundle_adjuster.main(base + extra)
        except SystemExit as e:
            out[label] = {"argv": base + extra, "exit": str(e)}
            continue
        pick = lambda key: [ln.strip() for ln in text.getvalue().splitlines() if ln.strip().startswith(key)]
        out[label] = {"argv": base + extra, "initial_cost": c0, "final_cost": c1,
                      "accepted": [bool(row[7]) for row in rows], "ls_iter": [int(row[6]) for row in rows],
                      "linear_solver_timer": (pick("Linear solver") or [None])[0],
                      "sparse_cholesky_timer": (pick("Sparse Cholesky factor") or [None])[0],
                      "analysis_timer": (pick("Sparse Cholesky analysis") or [None])[0],
                      "dense_cholesky_timer": (pick("Dense Cholesky") or [None])[0]}
    if added:
        del bal.CONFIGS[name]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", nargs="+", default=SHAPES)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--slow_ms", type=float, default=200.0)
    ap.add_argument("--slow_reps", type=int, default=3)
    ap.add_argument("--skip_driver", action="store_true")
    ap.add_argument("--skip_kernels", action="store_true")
    ap.add_argument("--num_iterations", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sparse_cholesky_probe: needs a HIP device")
    doc = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "shapes": [], "driver": {}}
    if args.out and os.path.exists(args.out):  # shapes measured in an earlier call stay
        with open(args.out) as f:
            doc = json.load(f)

    def write():
        text = json.dumps(doc, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return text

    for name in () if args.skip_kernels else args.shapes:
        doc["shapes"] = [s for s in doc["shapes"] if s["shape"] != name] + [probe(name, args)]
        write()
    for name in () if args.skip_driver else args.shapes:
        doc["driver"][name] = driver(name, args)
        write()
    print(write())


if __name__ == "__main__":
    main()
