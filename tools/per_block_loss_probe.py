#!/usr/bin/env python3
"""What per-block loss parameters cost and buy: kernel times of the
residual+Jacobian evaluation (BlockSparseMatrix, Huber, device-resident
buffers, HIP events through options.profile) of one problem-13682-shaped
Program in four forms, interleaved in one process:

  A  uniform Huber(1)                      one group, GroupArgs::loss
  B  per-block Huber, a = 1 in every row   the same arithmetic plus the
                                           16-byte-per-block record stream
  C  three widths, one merged group        loss_data_size 2
  D  the same blocks as three groups       one group per distinct value

C and D assign the widths either by thirds of the block range (every split
group stays affine: the best case for D) or round-robin (--assign
interleaved: the split groups lose the affine layout and take the table
kernel).  Every leg is warmed (--warmup evaluations, the clock ramp of DESIGN
section 5) before each timed window of --steps evaluations; --rounds
rounds, legs alternating inside each round.  Outputs of B are compared bit for
bit with A's, and D's residuals and Jacobian with C's.

  --only A --package-dir DIR --label NAME   time leg A alone with the package
      (and its lib/libcse.so) under DIR: another build of the library, e.g.
      the parent commit's.  NAME is recorded in place of the directory.
  --alternate DIR --processes K --out-dir OUT   leg A of the build under DIR
      ("parent") and of this one ("this"), each in a fresh child process of
      this script, alternating, K times each: OUT/legA_parent_<k>.json and
      OUT/legA_this_<k>.json.  Stops at the first child that fails.
  --summarize OUT   print the summary of the JSON files in OUT (no GPU).

Writes one JSON document to --out and prints it.  Which kernel a group ran
and whether its plan is grad_exact are not reported by the library: the
"inferred" entries are worked out here from the layout formulas and the
group count (see the code), not observed.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alternate(args):
    """Leg A of two builds in alternating fresh processes."""
    os.makedirs(args.out_dir, exist_ok=True)
    common = [sys.executable, os.path.abspath(__file__), "--only", "A", "--config", args.config,
              "--rounds", str(args.rounds), "--steps", str(args.steps), "--warmup", str(args.warmup)]
    for k in range(1, args.processes + 1):
        for label, pkg in (("parent", args.alternate), ("this", args.package_dir)):
            out = os.path.join(args.out_dir, f"legA_{label}_{k}.json")
            rc = subprocess.call(common + ["--package-dir", pkg, "--label", label, "--out", out],
                                 timeout=600)
            if rc != 0:
                sys.exit(f"leg A of {label} (process {k}) failed with status {rc}")


def summarize(out_dir):
    import numpy as np

    def leg_a(label):
        per = [json.load(open(f))["times_ms"]["A"]
               for f in sorted(glob.glob(os.path.join(out_dir, f"legA_{label}_*.json")))]
        return np.array([t for x in per for t in x]), [float(np.median(x)) for x in per]

    tp, pp = leg_a("parent")
    tn, pn = leg_a("this")
    if tp.size and tn.size:
        print(f"Leg A (uniform Huber, residual+Jacobian kernel ms), alternating processes, {len(pp)} each:")
        for name, t, per in (("parent commit's build", tp, pp), ("this build", tn, pn)):
            print(f"  {name:22s} median {np.median(t):.4f}  min {t.min():.4f}  max {t.max():.4f}  "
                  f"per-process medians {' '.join('%.4f' % x for x in per)}")
        print(f"  difference of medians {np.median(tn) - np.median(tp):+.4f} ms "
              f"({(np.median(tn) / np.median(tp) - 1) * 100:+.2f} %); the parent's own spread "
              f"{tp.max() - tp.min():.4f} ms ({(tp.max() / tp.min() - 1) * 100:.2f} %)")
    for f in sorted(glob.glob(os.path.join(out_dir, "legs_*.json"))):
        x = json.load(open(f))
        print(f"{os.path.basename(f)}: widths by {x['assign']}, {len(next(iter(x['times_ms'].values())))} "
              f"rounds x {x['steps']} evaluations, median [min, max] ms:")
        for leg, med in x["median_ms"].items():
            i = x["info"][leg]
            print(f"  {leg}: {med:.4f} [{x['spread_ms'][leg][0]:.4f}, {x['spread_ms'][leg][1]:.4f}]  "
                  f"groups {i['num_groups']} affine {i['num_affine_groups']} fused "
                  f"{i['num_fused_gradient_groups']}  inferred: group store {i['group_store_inferred']}, "
                  f"grad_exact {i['grad_exact_inferred']}")
        for key in ("B_over_A", "B_over_A_by_bytes", "D_over_C"):
            if key in x:
                print(f"  {key} = {x[key]:.4f}")
        print(f"  outputs {x['outputs']}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="problem-13682-4456117")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=25)
    ap.add_argument("--assign", default="thirds", choices=["thirds", "interleaved"])
    ap.add_argument("--only", default="ABCD", help="legs to run, e.g. A or ABCD")
    ap.add_argument("--package-dir", default=os.path.join(REPO, "ceres-solver-cuda_amd"))
    ap.add_argument("--label", default=None, help="recorded as the build's name instead of --package-dir")
    ap.add_argument("--out", default=None)
    ap.add_argument("--alternate", default=None, metavar="DIR", help="package dir of the other build")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--summarize", default=None, metavar="OUT")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    if args.alternate:
        return alternate(args)
    sys.path.insert(0, os.path.abspath(args.package_dir))
    import numpy as np
    import torch
    import ceres_amd as ca
    from ceres_amd import _cse, bal
    from ceres_amd.problem import ResidualGroup

    assert torch.cuda.is_available(), "the probe measures on a HIP device"
    counts = bal.CONFIGS[args.config] if args.config in bal.CONFIGS else tuple(
        int(x) for x in args.config.split(","))
    t0 = time.time()
    cams, pts, ci, pi, obs = bal.synthetic(*counts)
    n = len(ci)
    huber = ca.Loss.huber(1.0)

    def program(**kw):
        return bal.program(cams, pts, ci, pi, obs, loss=huber, format=ca.BLOCK_SPARSE, **kw)

    widths = np.array([0.5, 1.0, 2.0])
    which = (np.arange(n) * 3 // n) if args.assign == "thirds" else np.arange(n) % 3
    progs = {}
    if "A" in args.only:
        progs["A"] = program()
    if "B" in args.only:
        progs["B"] = program(loss_data=np.tile(np.array([[1.0, 1.0]]), (n, 1)))
    if "C" in args.only:
        progs["C"] = program(loss_data=np.column_stack([widths[which], np.ones(n)]))
    if "D" in args.only:
        import copy
        d = copy.copy(progs["C"] if "C" in progs else program())
        g = d.groups[0]
        d.groups = []
        for k in range(3):
            sel = np.flatnonzero(which == k)
            contiguous = sel.size and sel[-1] - sel[0] + 1 == sel.size
            d.groups.append(ResidualGroup(g.kind, ca.Loss.huber(float(widths[k])), g.ids[sel], g.data[sel],
                                          None if contiguous else sel.astype(np.int64),
                                          int(sel[0]) if contiguous else 0))
        d._keep = []
        progs["D"] = d
    print(f"# built {args.config} ({n} blocks) in {time.time() - t0:.1f} s", flush=True)

    dev = torch.device("cuda", 0)
    f64 = torch.float64
    any_prog = next(iter(progs.values()))
    state = torch.from_numpy(any_prog.state).to(dev)
    cost = torch.zeros(1, dtype=f64, device=dev)
    res = torch.empty(any_prog.num_residuals, dtype=f64, device=dev)
    jac = torch.empty(any_prog.num_jacobian_values, dtype=f64, device=dev)
    stream = torch.cuda.current_stream(dev)
    evs, infos = {}, {}
    for leg, prog in progs.items():
        t0 = time.time()
        evs[leg] = ca.Evaluator(prog, device=0, profile=True, stream=stream.cuda_stream)
        inf = evs[leg].info()
        # Inferred, not observed: EvaluateAffineChunksGroupStore's condition
        # (GroupStoreEligible) restated for 64-byte-aligned output buffers
        # and the BlockSparseMatrix layout -- residuals at 2 b, E cells at
        # 6 b, F cells at 6 n + 18 b (doubles) for a contiguous group whose
        # first block is b -- and grad_exact's need for the program's one
        # group with the fused gradient (plan.hpp).
        starts = [g.first if g.index is None else None for g in prog.groups]
        store = [s is not None and (2 * s) % 8 == 0 and (6 * s) % 8 == 0 and (6 * n + 18 * s) % 8 == 0
                 for s in starts]
        infos[leg] = {"num_groups": inf.num_groups, "num_affine_groups": inf.num_affine_groups,
                      "num_fused_gradient_groups": inf.num_fused_gradient_groups,
                      "bytes_jacobian_eval": inf.bytes_jacobian_eval,
                      "group_store_inferred": store,
                      "grad_exact_inferred": inf.num_groups == 1 and inf.num_fused_gradient_groups == 1,
                      "create_s": round(time.time() - t0, 2)}
        print(f"# leg {leg}: {infos[leg]}", flush=True)

    def run(leg, count):
        ev = evs[leg]
        for _ in range(count):
            ev.evaluate_device(state.data_ptr(), cost.data_ptr(), res.data_ptr(), None, jac.data_ptr())
        assert ev.wait() == 0

    # Outputs: B against A in every bit, D against C in residuals and Jacobian.
    same = {}
    kept = {}
    for leg in progs:
        run(leg, 1)
        torch.cuda.synchronize()
        kept[leg] = (res.clone(), jac.clone(), float(cost.item()))
    if "A" in kept and "B" in kept:
        same["B_equals_A"] = bool(torch.equal(kept["A"][0], kept["B"][0]) and
                                  torch.equal(kept["A"][1], kept["B"][1]) and kept["A"][2] == kept["B"][2])
    if "C" in kept and "D" in kept:
        same["D_equals_C_residuals_jacobian"] = bool(torch.equal(kept["C"][0], kept["D"][0]) and
                                                     torch.equal(kept["C"][1], kept["D"][1]))
        same["cost_C_D"] = [kept["C"][2], kept["D"][2]]
    kept.clear()
    print(f"# outputs: {same}", flush=True)

    times = {leg: [] for leg in progs}
    for rnd in range(args.rounds):
        for leg in progs:
            run(leg, args.warmup)
            evs[leg].reset_kernel_stats()
            run(leg, args.steps)
            _, total, count = evs[leg].kernel_stats()
            times[leg].append(total / count)
            print(f"round {rnd} leg {leg}: {total / count:.4f} ms", flush=True)
    for ev in evs.values():
        ev.close()
    med = {leg: float(np.median(t)) for leg, t in times.items()}
    out = {"config": args.config, "blocks": n, "assign": args.assign, "steps": args.steps,
           "warmup": args.warmup, "abi": _cse.CSE_ABI_VERSION,
           "build": args.label or os.path.relpath(os.path.abspath(args.package_dir), REPO),
           "info": infos, "outputs": same, "times_ms": times, "median_ms": med,
           "spread_ms": {leg: [float(np.min(t)), float(np.max(t))] for leg, t in times.items()}}
    if "A" in med and "B" in med:
        out["B_over_A"] = med["B"] / med["A"]
        out["B_over_A_by_bytes"] = infos["B"]["bytes_jacobian_eval"] / infos["A"]["bytes_jacobian_eval"]
    if "C" in med and "D" in med:
        out["D_over_C"] = med["D"] / med["C"]
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
