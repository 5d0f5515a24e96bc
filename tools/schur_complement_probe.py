#!/usr/bin/env python3
"""What the explicit Schur complement costs against the implicit one.

At a BAL shape (default: problem-49-7776 with 31,843 observations and
problem-1778-993923 with 5,001,946, synthetic), on the device, with HIP
events after warm-up, on the evaluator's stream:

  init        cse_schur_init (JACOBI)
  multiply    one cse_schur_multiply
  complement  cse_schur_complement into a dense S (the plan already uploaded;
              the first call, which builds and uploads it, is timed apart by
              the host clock)
  cholesky    the driver's cholesky_solve of S x = rhs (bundle_adjuster.py)

D = sqrt(diag(J^T J) / radius) with the driver's initial radius 1e4, b = -r at
the problem's start.  Then the driver itself (ceres_amd.bundle_adjuster) runs
--linear_solver iterative_schur and dense_schur at the same shape and the
ls_iter column, the final costs and the "Linear solver" timer are recorded.

break_even_iterations = (complement + cholesky) / multiply: the PCG iterations
per solve above which forming and factoring S is the cheaper solve.
dense_products_ms = f_cols / 9 implicit products, the cost of building S from
cse_schur_multiply alone (nine columns of one camera per product is the most a
caller could batch).  Algorithmic bytes of the complement are counted from the
plan (see complement_bytes).

--sparse measures the block-sparse complement instead (same protocol, same
process, same init): num_blocks and the bytes of its values;
cse_schur_complement_sparse against the dense cse_schur_complement where the
dense S fits --max_dense_gb; cse_schur_explicit_multiply against
cse_schur_multiply, and its rate over its algorithmic bytes (explicit_bytes);
the driver's "Linear solver" timer with and without
--use_explicit_schur_complement (after one discarded driver run, the two
interleaved twice).  A shape whose plan, structure and values
exceed --max_sparse_gb gets its counts alone.

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
    "problem-13682-4456117": (13682, 4456117, 28987644),
}
DEFAULT_SHAPES = ["problem-49-7776", "problem-1778-993923"]


def complement_bytes(n_pairs, n_chunks, n_blocks, f_cols):
    """Bytes the algorithm needs: per pair two F cells (144 each), two E
    cells (48 each), M_p (48), the pair record (8) and the point id (4); per
    chunk its 9 x 9 partial written and read back (648 each); per block the
    block and its mirror written; the dense S zeroed once."""
    return (n_pairs * (2 * 144 + 2 * 48 + 48 + 8 + 4) + n_chunks * 2 * 648 + n_blocks * 2 * 648 +
            8 * f_cols * f_cols)


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


def probe(name, args):
    import numpy as np
    import torch
    import ceres_amd as ca
    from ceres_amd import _cse, bal, bundle_adjuster

    bal.CONFIGS.setdefault(name, SHAPES[name])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
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
    # D as the driver's first LM step: diag(J^T J) by one left multiply
    D = torch.zeros(n, dtype=f64, device=dev)
    ones = torch.ones(m, dtype=f64, device=dev)
    ev.left_multiply_device((jac * jac).data_ptr(), ones.data_ptr(), D.data_ptr())
    D = torch.sqrt(D.clamp_(min=1e-6) / 1e4)
    b = -r
    rhs = torch.empty(f_cols, dtype=f64, device=dev)
    v = torch.randn(f_cols, dtype=f64, device=dev)
    y = torch.empty(f_cols, dtype=f64, device=dev)

    t0 = time.perf_counter()
    n_blocks, n_pairs, plan_bytes = ev.schur_complement_plan()
    count_s = time.perf_counter() - t0
    out = {"shape": name, "observations": int(prog.num_residual_blocks), "f_cols": f_cols,
           "e_cols": e_cols, "num_blocks": n_blocks, "num_pairs": n_pairs, "plan_bytes": plan_bytes,
           "S_bytes": 8 * f_cols * f_cols, "plan_count_host_s": count_s}
    init = lambda: ev.schur_init_device(jac.data_ptr(), D.data_ptr(), b.data_ptr(), rhs.data_ptr(),
                                        _cse.SCHUR_JACOBI)
    init()
    S = torch.empty((f_cols, f_cols), dtype=f64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.schur_complement_device(S.data_ptr())
    torch.cuda.synchronize()
    out["first_complement_with_plan_build_s"] = time.perf_counter() - t0
    out["init"] = event_ms(torch, init, args.warmup, args.reps)
    out["multiply"] = event_ms(torch, lambda: ev.schur_multiply_device(v.data_ptr(), y.data_ptr()),
                               args.warmup, args.reps)
    out["complement"] = event_ms(torch, lambda: ev.schur_complement_device(S.data_ptr()),
                                 args.warmup, args.reps)
    try:  # which side the driver's cholesky_solve runs on here
        torch.linalg.cholesky_ex(S[:18, :18].contiguous())
        out["cholesky_backend"] = "device (torch.linalg.cholesky_ex)"
    except RuntimeError as e:
        out["cholesky_backend"] = "host numpy: " + str(e).splitlines()[0]
    out["cholesky"] = event_ms(torch, lambda: bundle_adjuster.cholesky_solve(S, rhs),
                               min(args.warmup, 2), max(3, args.reps // 4))
    assert ev.wait() == 0
    # the matrix just timed is the operator just timed
    Sv = S @ v
    ev.schur_multiply_device(v.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()
    out["S_times_v_vs_multiply_rel"] = float(((Sv - y).norm() / y.norm()).item())
    ev.close()
    del S, jac

    # the chunk count, from plan_bytes = 24 blocks + 16 + 8 pairs + (4 + 648) chunks (plan.cpp)
    n_chunks = (plan_bytes - 24 * n_blocks - 16 - 8 * n_pairs) // 652
    out["num_chunks"] = n_chunks
    nbytes = complement_bytes(n_pairs, n_chunks, n_blocks, f_cols)
    cm, mm, ch = out["complement"]["median_ms"], out["multiply"]["median_ms"], out["cholesky"]["median_ms"]
    out["complement_algorithmic_bytes"] = nbytes
    out["complement_TB_per_s"] = nbytes / (cm * 1e-3) / 1e12
    out["break_even_iterations"] = (cm + ch) / mm
    out["dense_products_ms"] = f_cols / 9 * mm
    out["complement_slower_than_f_cols_over_9_products"] = cm > out["dense_products_ms"]

    # the driver at this shape, both solvers
    for solver in ("iterative_schur", "dense_schur"):
        argv = ["--synthetic", name, "--robustify", "--point_sigma", "0.05", "--num_iterations",
                str(args.num_iterations), "--linear_solver", solver]
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            c0, c1, rows = bundle_adjuster.main(argv)
        line = [ln for ln in text.getvalue().splitlines() if ln.strip().startswith("Linear solver")]
        out["driver_" + solver] = {"argv": argv, "initial_cost": c0, "final_cost": c1,
                                   "ls_iter": [row[6] for row in rows],
                                   "accepted": [bool(row[7]) for row in rows],
                                   "linear_solver_timer": line[0].strip() if line else None}
    its = out["driver_iterative_schur"]["ls_iter"]
    out["iterative_ms_per_solve_at_measured_iterations"] = sum(its) / len(its) * mm
    out["dense_ms_per_solve"] = cm + ch
    return out


def explicit_bytes(num_blocks, f_cols):
    """Bytes the product needs: every block once, x and y once, and the index
    tables it walks (row_begin and col_begin, block_col, col_block).  The
    72-byte column contribution each block leaves for the second kernel
    (written once, read once) is the implementation's, not counted here."""
    cams = f_cols // 9
    return 648 * num_blocks + 2 * 8 * f_cols + 2 * 8 * (cams + 1) + 4 * num_blocks + 4 * (num_blocks - cams)


def probe_sparse(name, args):
    import torch
    import ceres_amd as ca
    from ceres_amd import _cse, bal, bundle_adjuster

    bal.CONFIGS.setdefault(name, SHAPES[name])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    f64 = torch.float64
    prog = bal.synthetic_program(bal.CONFIGS[name], loss=ca.Loss.huber(1.0))
    ev = ca.Evaluator(prog, device=0, stream=torch.cuda.current_stream(dev).cuda_stream)
    n, m = prog.num_effective_parameters, prog.num_residuals
    e_cols, f_cols = ev.schur_structure()
    t0 = time.perf_counter()
    plan_blocks, n_pairs, plan_bytes = ev.schur_complement_plan()
    cams, num_blocks, structure_bytes = ev.schur_complement_sparse_counts()
    count_s = time.perf_counter() - t0
    need = structure_bytes + plan_bytes + 648 * num_blocks
    out = {"shape": name, "observations": int(prog.num_residual_blocks), "f_cols": f_cols, "cameras": cams,
           "num_blocks": num_blocks, "plan_blocks": plan_blocks, "num_pairs": n_pairs,
           "upper_triangle_fill": num_blocks / (cams * (cams + 1) / 2),
           "values_bytes": 648 * num_blocks, "structure_device_bytes": structure_bytes,
           "plan_bytes": plan_bytes, "device_bytes_needed": need, "dense_S_bytes": 8 * f_cols * f_cols,
           "counts_host_s": count_s}
    out["fits"] = need <= args.max_sparse_gb * 2 ** 30
    if not out["fits"]:
        ev.close()
        return out
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
    y = torch.empty(f_cols, dtype=f64, device=dev)
    ye = torch.empty(f_cols, dtype=f64, device=dev)
    init = lambda: ev.schur_init_device(jac.data_ptr(), D.data_ptr(), b.data_ptr(), rhs.data_ptr(),
                                        _cse.SCHUR_JACOBI)
    init()
    V = torch.empty(81 * num_blocks, dtype=f64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.schur_complement_sparse_device(V.data_ptr())
    torch.cuda.synchronize()
    out["first_sparse_complement_with_plan_build_s"] = time.perf_counter() - t0
    out["multiply"] = event_ms(torch, lambda: ev.schur_multiply_device(v.data_ptr(), y.data_ptr()),
                               args.warmup, args.reps)
    out["explicit_multiply"] = event_ms(
        torch, lambda: ev.schur_explicit_multiply_device(V.data_ptr(), v.data_ptr(), ye.data_ptr()),
        args.warmup, args.reps)
    out["sparse_complement"] = event_ms(torch, lambda: ev.schur_complement_sparse_device(V.data_ptr()),
                                        args.warmup, args.reps)
    assert ev.wait() == 0
    out["explicit_vs_multiply_rel"] = float(((ye - y).norm() / y.norm()).item())
    nbytes = explicit_bytes(num_blocks, f_cols)
    em = out["explicit_multiply"]["median_ms"]
    out["explicit_algorithmic_bytes"] = nbytes
    out["explicit_TB_per_s"] = nbytes / (em * 1e-3) / 1e12
    out["explicit_over_implicit"] = em / out["multiply"]["median_ms"]
    if 8 * f_cols * f_cols <= args.max_dense_gb * 2 ** 30:
        S = torch.empty((f_cols, f_cols), dtype=f64, device=dev)
        out["dense_complement"] = event_ms(torch, lambda: ev.schur_complement_device(S.data_ptr()),
                                           args.warmup, args.reps)
        out["sparse_over_dense_complement"] = (out["sparse_complement"]["median_ms"] /
                                               out["dense_complement"]["median_ms"])
        del S
    # PCG iterations per solve above which forming S pays for itself
    gain = out["multiply"]["median_ms"] - em
    out["break_even_iterations"] = out["sparse_complement"]["median_ms"] / gain if gain > 0 else None
    ev.close()
    del V, jac

    # The first driver run of a process pays for torch's first use of its
    # vector kernels inside the "Linear solver" timer: one run is discarded,
    # and the implicit leg runs on both sides of the explicit one.
    flag = ["--use_explicit_schur_complement"]
    legs = (("warmup_discarded", []), ("implicit", []), ("explicit", flag), ("implicit_again", []),
            ("explicit_again", flag))
    for label, extra in () if args.skip_driver else legs:
        argv = ["--synthetic", name, "--robustify", "--point_sigma", "0.05", "--num_iterations",
                str(args.num_iterations), "--max_schur_gb", str(args.max_sparse_gb)] + extra
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            c0, c1, rows = bundle_adjuster.main(argv)
        line = [ln for ln in text.getvalue().splitlines() if ln.strip().startswith("Linear solver")]
        out["driver_" + label] = {"argv": argv, "initial_cost": c0, "final_cost": c1,
                                  "ls_iter": [row[6] for row in rows],
                                  "accepted": [bool(row[7]) for row in rows],
                                  "linear_solver_timer": line[0].strip() if line else None}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--shapes", nargs="+", default=DEFAULT_SHAPES, choices=list(SHAPES))
    ap.add_argument("--sparse", action="store_true", help="the block-sparse complement's legs")
    ap.add_argument("--max_sparse_gb", type=float, default=200.0)
    ap.add_argument("--max_dense_gb", type=float, default=16.0)
    ap.add_argument("--skip_driver", action="store_true", help="--sparse: the kernels' legs alone")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--num_iterations", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("schur_complement_probe: needs a HIP device")
    doc = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for name in args.shapes:
        doc["shapes"].append(probe_sparse(name, args) if args.sparse else probe(name, args))
        text = json.dumps(doc, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
