#!/usr/bin/env python3
"""Benchmark: residual+Jacobian evaluations/sec on BAL problem-13682 (MI355X).

One "step" = one residual+Jacobian evaluation of a problem-13682-shaped
Program (13,682 cameras, 4,456,117 points, 28,987,644 SnavelyReprojectionError
<2,9,3> residual blocks, HuberLoss(1.0), BlockSparseMatrix with the points
eliminated first: BASELINE.json configs[3]) through the C ABI's
device-resident entry point (cse_evaluate_device: residuals, Jacobian values
and cost written to HBM; inputs already resident when the clock starts).

Multi-GPU (BASELINE.json configs[4]), one process per GPU:
  `bench.py --gpus N` starts the N ranks itself (torch.distributed.run in a
  child process, before anything touches a GPU) unless it already runs under
  a launcher (WORLD_SIZE set, which must equal N).
  --scaling strong (default) the one problem-13682 is cut into N point-bucket
                   shards (ceres_amd.shard / ceres_amd.distributed); each rank
                   evaluates its shard and writes its contiguous Jacobian
                   strips; the cost (and, with the gradient, the camera rows)
                   is all-reduced over RCCL.  value = whole-problem
                   evaluations / s.
  --scaling weak   every rank evaluates its own problem-13682-sized replica
                   (a distinct seed); value = N * steps / time.
  With more ranks than visible GPUs (a rehearsal on a 1-GPU box) the ranks
  share the devices and the exchange runs over gloo; the line says so.

A plain run (`bench.py --gpus N --steps K --warmup W`) builds the problem,
runs W untimed and K timed headline steps, writes the last timed step's
outputs if --dump-outputs DIR is given (DIR/<name>.npy: cost, residuals,
jacobian, ...; float64, arrays above DUMP_MAX_VALUES values as the fixed
sample_indices elements; the inputs are the seeded generator's, identical from
run to run) and prints the line.

With --full the line also carries secondary legs measured in the same run
after the headline (each with its own barrier-bracketed timing, max over
ranks):
  gradient       residual+Jacobian+gradient J^T r (what the trust-region
                 minimizer requests, trust_region_minimizer.cc:242-255)
  same_point     the headline evaluation with new_evaluation_point = false
                 (CSE_EVAL_SAME_POINT: the Jacobian at a just-accepted
                 candidate, trust_region_minimizer.cc:822-826; no repack)
  residual_only  residuals + cost (trust_region_minimizer.cc:770-788)
  jet            the headline evaluation with the Jacobian by Jet<double, 12>
                 (cse_options.jacobian_form; the headline uses the closed form)
  user_functor   the same workload with a *user* functor, BundlerResidual
                 (bundle_adjustment_test_util.h:188-227), compiled in a user
                 TU against ceres_amd/autodiff_cuda.h
                 (examples/build/libuser_functors.so) and registered through
                 cse_register_functor: the reference's usage model
  host_strips    evaluation + D2H of each rank's residual and Jacobian
                 strips into pinned host memory (the reference's seam,
                 README.md:198-200; PCIe-inclusive, never `value`)
and, on rank 0 at N=1, the CPU baseline (the oracle, oracle/, built
-O3 -march=native on this host) on every physical core of the affinity mask,
at the box's CPU share (the cgroup quota) and at 1 thread, for
residual+Jacobian and residual-only; its value (and `speedup_vs_cpu`) is the
fastest residual+Jacobian leg.

Data is synthetic (no BAL file is available offline; see ceres_amd/bal.py for
the generator), with the exact BAL header counts.  Rank 0 prints one JSON
line; DESIGN.md §5 documents every field.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "ceres-solver-cuda_amd"))

if "--lib" in sys.argv:  # A/B runs (tools/): another build of the same ABI
    from ceres_amd import _cse  # noqa: E402
    _cse.use_library(os.path.abspath(sys.argv[sys.argv.index("--lib") + 1]))
import ceres_amd as ca  # noqa: E402
from ceres_amd import bal  # noqa: E402

PEAK_HBM_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
METRIC = "residual+Jacobian evaluations/sec on BAL problem-13682; achieved HBM GB/s"
DUMP_MAX_VALUES = 1 << 20  # --dump-outputs, per array: 8 MB of float64, at most 4 arrays a mode
DUMP_SEED = 0xD0C5


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=25)
    ap.add_argument("--config", default="problem-13682-4456117", choices=list(bal.CONFIGS))
    ap.add_argument("--loss", default="huber", choices=["trivial", "huber", "cauchy"])
    ap.add_argument("--format", default="block_sparse", choices=["block_sparse", "compressed_row"])
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"])
    ap.add_argument("--gradient", action="store_true",
                    help="the headline step also produces the gradient J^T r")
    ap.add_argument("--gradient-mode", type=int, default=0, choices=[0, 1, 2, 3],
                    help="cse_options.gradient_mode: 0 fused, camera rows re-evaluated in camera "
                         "order (default), 1 post-pass, 2 atomics, 3 fused with block-order "
                         "camera contributions")
    ap.add_argument("--mode", default="jacobian",
                    choices=["jacobian", "residual", "candidate", "spmv", "cgnr", "schur"],
                    help="jacobian: residual+Jacobian evaluation (the headline metric); "
                         "residual: residuals+cost only; candidate: the trust-region candidate "
                         "step, Plus(x, delta) then cost-only evaluation "
                         "(trust_region_minimizer.cc:770-788); spmv: one CGNR iteration's "
                         "products J p and J^T (J p); cgnr: the one-pass normal operator; "
                         "schur: one product with the implicit Schur complement (cse_schur_multiply)")
    ap.add_argument("--camera", default="angle_axis", choices=["angle_axis", "quaternion"],
                    help="angle_axis: SnavelyReprojectionError<2,9,3> (the headline); quaternion: "
                         "SnavelyReprojectionErrorWithQuaternions<2,10,3> with every camera on "
                         "ProductManifold<QuaternionManifold, EuclideanManifold<6>> "
                         "(bundle_adjuster --use_quaternions --use_manifolds)")
    ap.add_argument("--held-cameras", type=int, default=0,
                    help="hold the first K cameras constant (SetParameterBlockConstant, e.g. the "
                         "gauge): their blocks have no F cell (BlockSparseMatrix); not the headline")
    ap.add_argument("--full", action="store_true",
                    help="after the headline's timed steps also run the secondary legs and the CPU "
                         "baseline (each with its own timing); a plain run sets up, warms up, times "
                         "--steps steps and prints the line with `secondary` empty and "
                         "`cpu_baseline` null")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step of the headline left "
                         "in its output buffers (rank 0's) as DIR/<name>.npy, float64; an array of "
                         "more than DUMP_MAX_VALUES values is written as a fixed sample of its "
                         "elements (sample_indices: they depend only on the array's length)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the gradient / residual-only / host-strip legs")
    ap.add_argument("--secondary-steps", type=int, default=20)
    ap.add_argument("--settle", type=float, default=0.0,
                    help="seconds of untimed steps before the --warmup steps (default 0: the "
                         "headline keeps the plain W-warm-up protocol; the clock ramp it then "
                         "includes is documented in DESIGN.md section 5); reported as "
                         "settle_steps")
    ap.add_argument("--host-steps", type=int, default=5)
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-only", action="store_true",
                    help="BASELINE.json configs[0]: problem-16 on the CPU ProgramEvaluator "
                         "restatement at num_threads=1 (no GPU); prints its own JSON line")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="threads of the CPU baseline's all-core leg; 0 = one per physical core "
                         "of the affinity mask (legs at the box's CPU share -- the cgroup quota, "
                         "else $OMP_NUM_THREADS -- and at 1 thread are timed beside it; value = "
                         "the fastest)")
    ap.add_argument("--seed", type=int, default=0xCE2E5)
    ap.add_argument("--lib", default=None, help="load this build of libcse.so (A/B runs)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="N > 1: order each cost all-reduce before the next evaluation instead of "
                         "overlapping it (the default runs it on RCCL's stream beside the next "
                         "evaluation and waits for all of them inside the timed region)")
    ap.add_argument("--shard-of", type=int, default=0,
                    help="single process: evaluate only rank 0's shard of an N-way point-bucket "
                         "cut (the per-rank work of an N-GPU strong-scaling run, without the "
                         "collectives); reported with value = shard evaluations/s, not the headline")
    return ap.parse_args()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(args):
    """Start args.gpus ranks of this script under torch.distributed.run, as a
    child process (this process has not touched a GPU), and return its exit
    code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--master-addr=127.0.0.1",
           f"--master-port={_free_port()}", os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


def sample_indices(n):
    """The sorted element indices --dump-outputs keeps of an array of
    n > DUMP_MAX_VALUES values: seeded, a function of n alone, so two builds
    run with the same arguments write the same elements."""
    rng = np.random.default_rng([DUMP_SEED, n])
    return np.sort(rng.integers(0, n, size=DUMP_MAX_VALUES))


def dump_outputs(path, outputs, rank):
    """--dump-outputs: every device tensor of `outputs` (name -> tensor) as
    path/<name>.npy in float64 (path/<name>.rank<r>.npy on a rank r > 0),
    whole or as the sample_indices elements."""
    import torch
    os.makedirs(path, exist_ok=True)
    for name, t in outputs.items():
        t = t.detach().reshape(-1)
        if t.numel() > DUMP_MAX_VALUES:
            t = t[torch.from_numpy(sample_indices(t.numel())).to(t.device)]
        np.save(os.path.join(path, f"{name}{f'.rank{rank}' if rank else ''}.npy"),
                t.cpu().numpy().astype(np.float64, copy=False))


def make_loss(name):
    return {"trivial": ca.Loss.trivial(), "huber": ca.Loss.huber(1.0),
            "cauchy": ca.Loss.cauchy(1.0)}[name]


# ---------------------------------------------------------------------------
# CPU baseline (rank 0, N = 1): the oracle restatement of ProgramEvaluator
# ---------------------------------------------------------------------------
def _host_info():
    """CPU model, sockets and physical cores of the host, and the physical
    cores inside this process's affinity mask (the cores the all-core leg
    may use: one thread per physical core, SMT siblings left idle, as the
    reference's benchmark sweeps num_threads up to the core count,
    evaluation_benchmark.cc:206-210)."""
    model, phys, cpu_core = None, set(), {}
    pid, proc = None, None
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                k, _, v = line.partition(":")
                k, v = k.strip(), v.strip()
                if k == "processor":
                    proc = int(v)
                elif k == "model name" and model is None:
                    model = v
                elif k == "physical id":
                    pid = v
                elif k == "core id":
                    phys.add((pid, v))
                    if proc is not None:
                        cpu_core[proc] = (pid, v)
    except OSError:
        pass
    aff = os.sched_getaffinity(0)
    in_mask = {cpu_core[c] for c in aff if c in cpu_core}
    quota, quota_src = _cpu_quota()
    return {"cpu_model": model, "logical_cpus": os.cpu_count(),
            "sockets": len({p for p, _ in phys}) or None, "physical_cores": len(phys) or None,
            "affinity_cpus": len(aff), "physical_cores_in_affinity": len(in_mask) or len(aff),
            "cgroup_cpu_quota": quota, "cgroup_cpu_quota_source": quota_src,
            "omp_num_threads": os.environ.get("OMP_NUM_THREADS")}


def _cpu_quota():
    """CPUs the cgroup's CFS quota grants this process (quota / period), or
    None when unlimited or unreadable; and the file it came from."""
    try:  # cgroup v2
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, per = fh.read().split()[:2]
        if q != "max":
            return float(q) / float(per), "/sys/fs/cgroup/cpu.max"
        return None, "/sys/fs/cgroup/cpu.max (max)"
    except (OSError, ValueError):
        pass
    try:  # cgroup v1
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as fh:
            q = int(fh.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
            per = int(fh.read())
        if q > 0:
            return q / per, "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"
        return None, "/sys/fs/cgroup/cpu/cpu.cfs_quota_us (-1)"
    except (OSError, ValueError):
        return None, None


def _oracle_module():
    """oracle_py bound to a -O3 -march=native build made on this host (into
    /tmp), else the portable prebuilt one."""
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import oracle_py as O
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"cse_oracle_native_{os.getpid()}")
    try:
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "oracle"), "native",
                        f"NATIVE_OUT={out}"], check=True, capture_output=True, timeout=120)
        O.use_library(os.path.join(out, "liboracle_native.so"))
        build = "g++ -O3 -march=native (oracle/Makefile native, built on this host)"
    except Exception as e:  # noqa: BLE001 - a missing compiler leaves the portable build
        build = f"portable prebuilt build (-O3, no -march=native; native build failed: {e!r})"
    return O, build


def user_functor_kind(name):
    """A kind of the example user functor library (examples/user_functors.hip),
    loaded into this process's libcse.so."""
    import ctypes
    lib = ca.load_functor_library(os.path.join(REPO, "examples", "build", "libuser_functors.so"))
    lib.cse_example_kind_name.restype = ctypes.c_char_p
    kinds = (ctypes.c_int32 * 64)()
    n = lib.cse_example_register(kinds, 64)
    if n < 0:
        raise RuntimeError("cse_example_register: " + ca._cse.last_error())
    names = [lib.cse_example_kind_name(i).decode() for i in range(n)]
    return kinds[names.index(name)]


def group_store_eligible(res_ptr, jac_ptr, nblocks):
    """The library's choice of the Snavely BlockSparse residual+Jacobian
    kernel for a shard-local evaluator (GroupStoreEligible,
    csrc/group_store_kernel.hpp): residuals, E cells (at 0) and F cells (at
    6 n doubles) on 64-byte boundaries -> EvaluateAffineChunksGroupStore,
    else the one-wave EvaluateAffineChunksTwoRoundW1."""
    return (res_ptr % 64 == 0 and jac_ptr % 64 == 0 and (jac_ptr + 48 * nblocks) % 64 == 0)


def cpu_baseline(args, arrays, threads, share):
    """The oracle on bounded, point-bucket-aligned samples of the workload:
    residual+Jacobian and residual-only at `threads` (one per physical core
    of the affinity mask), at `share` (the box's CPU share: the cgroup quota,
    else $OMP_NUM_THREADS) and at 1 thread -- the reference's own benchmark
    sweeps num_threads (evaluation_benchmark.cc:203-212).  value = the
    FASTEST residual+Jacobian leg, in whole-workload evaluations per second
    (blocks per second / the workload's blocks); `threads` = the thread count
    that produced it, `cores` = the CPUs those threads could use (capped by
    the cgroup quota)."""
    O, build = _oracle_module()
    cams, pts, ci, pi, obs = arrays
    total = len(ci)

    cache = {}

    def sample(nblocks):
        if nblocks in cache:
            return cache[nblocks]
        S = min(nblocks, total)
        last_pt = int(pi[S - 1])
        S = int(np.searchsorted(pi, last_pt, side="right"))
        prog = bal.program(cams, pts[:last_pt + 1], ci[:S], pi[:S], obs[:S],
                           loss=make_loss(args.loss), format=args.format)
        cache[nblocks] = (S, prog)
        return S, prog

    legs = {}
    counts = sorted({threads, share, 1}, reverse=True)
    for jac in (True, False):
        for nt in counts:
            # about 1 s per timed evaluation or less: the whole workload
            # multithreaded, a 1/16 (Jacobian) or 1/8 (residual-only) sample on
            # one thread
            S, prog = sample(total if nt > 1 else total // (16 if jac else 8))
            ev = O.OracleProgram.from_program(prog).evaluator(nt)
            r = np.empty(prog.num_residuals)
            j = np.empty(prog.num_jacobian_values) if jac else None
            ev.run(prog.state, None, r, None, j)  # warm-up (page faults)
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                ok, _ = ev.run(prog.state, None, r, None, j)
                times.append(time.perf_counter() - t0)
                assert ok
            ev.close()
            t = float(np.median(times))
            legs[f"{'jacobian' if jac else 'residual'}_{nt}t"] = {
                "evals_per_s": S / t / total, "blocks_per_s": S / t, "threads": nt,
                "sample_blocks": S, "median_s": t}
            del r, j
    host = _host_info()
    best = max((v for k, v in legs.items() if k.startswith("jacobian_")),
               key=lambda v: v["evals_per_s"])
    quota = host["cgroup_cpu_quota"]
    cores = best["threads"] if quota is None else max(1, min(best["threads"], int(round(quota))))
    return {"value": best["evals_per_s"], "unit": "evals/s", "cores": cores,
            "threads": best["threads"], "kind": "port",
            "sample": (f"residual+Jacobian of all {total:,} residual blocks of the same workload, "
                       f"median of 3 after a warm-up, at {sorted(set(counts))} threads "
                       f"({threads} = one per physical core of the affinity mask, {share} = the "
                       f"box's CPU share; 1-thread runs on the first 1/16 (Jacobian) or 1/8 "
                       f"(residual-only) of the blocks, cut at a point bucket); value = the "
                       f"fastest Jacobian leg ({best['threads']} threads), blocks/s / {total:,}; "
                       f"cores = the CPUs that leg could use (cgroup quota "
                       f"{quota if quota is not None else 'none'})"),
            "build": build, "host": host, "legs": legs,
            "configs0": configs0(O, build, args.seed)}


def configs0(O, build, seed, reps=10):
    """BASELINE.json configs[0]: problem-16-22106 (16 cameras, 22,106 points,
    83,718 SnavelyReprojectionError<2,9,3> blocks), no loss, BlockSparseMatrix,
    the CPU ProgramEvaluator restated (oracle/) at num_threads = 1 -- the
    reference's plumbing configuration, no GPU.  Residual+Jacobian and
    residual-only, median of `reps` after a warm-up, as the reference's
    evaluation benchmark times them (evaluation_benchmark.cc:203-266)."""
    prog = bal.synthetic_program("problem-16-22106", seed=seed)
    ev = O.OracleProgram.from_program(prog).evaluator(1)
    out = {}
    for jac in (True, False):
        r = np.empty(prog.num_residuals)
        j = np.empty(prog.num_jacobian_values) if jac else None
        ev.run(prog.state, None, r, None, j)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ok, cost = ev.run(prog.state, None, r, None, j)
            times.append(time.perf_counter() - t0)
            assert ok
        t = float(np.median(times))
        out["jacobian" if jac else "residual_only"] = {
            "value": 1.0 / t, "unit": "evals/s", "median_s": t, "reps": reps, "cost": cost}
    ev.close()
    out.update({"workload": "problem-16-22106 SnavelyReprojectionError<2,9,3>, no loss, "
                            "block_sparse, CPU ProgramEvaluator restatement (oracle/), "
                            "num_threads=1 (BASELINE.json configs[0])",
                "blocks": prog.num_residual_blocks, "threads": 1, "build": build})
    return out


def cpu_only(args):
    """--cpu-only: BASELINE.json configs[0] alone, on this host's CPU (no GPU,
    no torch): one JSON line."""
    O, build = _oracle_module()
    c0 = configs0(O, build, args.seed, reps=max(3, args.steps))
    line = {"metric": "residual+Jacobian evaluations/sec on BAL problem-16 (CPU ProgramEvaluator, "
                      "num_threads=1; BASELINE.json configs[0], not the headline)",
            "value": c0["jacobian"]["value"], "unit": "evals/s", "n_gpus": 0,
            "steps": c0["jacobian"]["reps"], "higher_is_better": True, "dtype": "f64",
            "data": "synthetic (BAL-shaped: exact header counts, seeded generator)",
            "config": {"workload": c0["workload"], "blocks": c0["blocks"]},
            "residual_only": c0["residual_only"], "build": build, "host": _host_info()}
    print(json.dumps(line), flush=True)
    return line


# ---------------------------------------------------------------------------
def main():
    args = parse()
    if args.cpu_only:
        return cpu_only(args)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    import torch.distributed as dist
    from ceres_amd import distributed

    ndev = torch.cuda.device_count()
    if ndev == 0:
        raise SystemExit("bench.py needs a HIP device")
    rehearsal = world > ndev  # several ranks per device: gloo, not RCCL
    dev_index = local_rank % ndev
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    backend = os.environ.get("CSE_DIST_BACKEND", "gloo" if rehearsal else "nccl")
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    def reduce_max(vals):
        if world == 1:
            return vals
        on_host = backend == "gloo"
        t = torch.tensor(vals, dtype=torch.float64, device="cpu" if on_host else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return [float(v) for v in t.cpu()]

    def barrier():
        if world > 1:
            dist.barrier()

    strong = args.scaling == "strong"
    t_build = time.perf_counter()
    counts = bal.CONFIGS[args.config]
    arrays = bal.synthetic(*counts, seed=args.seed + (0 if strong else rank))
    quat = args.camera == "quaternion"
    if quat:
        arrays = (bal.to_quaternion_cameras(arrays[0]),) + tuple(arrays[1:])
    srank, sworld = (rank, world) if strong else (0, 1)
    if args.shard_of > 1:
        if world != 1:
            raise SystemExit("--shard-of is a single-process measurement")
        srank, sworld = 0, args.shard_of
    stream = torch.cuda.current_stream(dev)
    se = distributed.ShardedEvaluator(*arrays, srank, sworld, device=dev_index,
                                      loss=make_loss(args.loss), format=args.format,
                                      gradient=True, gradient_mode=args.gradient_mode,
                                      stream=stream, quaternion_manifold=quat,
                                      constant_cameras=tuple(range(args.held_cameras)))
    variant = quat or args.held_cameras > 0
    if not (args.full and rank == 0 and world == 1 and not args.no_cpu_baseline
            and args.mode == "jacobian" and not variant):
        del arrays
        arrays = None
    build_s = time.perf_counter() - t_build
    ev, prog = se.evaluator, se.program
    info = ev.info()
    f64 = torch.float64
    units = world if not strong else 1  # whole-problem evaluations per step

    def run_leg(step, steps, warmup, settle_s=0.0):
        """Warm-up, then `steps` timed steps between barrier + synchronize;
        returns (elapsed_s, kernel_ms_local, kernel_ms_max) maxed over ranks.
        settle_s: before the `warmup` steps, untimed steps until that many
        seconds have passed (the GPU's clocks ramp over tens of ms after the
        idle problem build: profiles/round6/ramp)."""
        t_s, n_s = time.perf_counter(), 0
        while settle_s > 0:  # rounds of 8 steps; every rank runs the same count
            for _ in range(8):
                step()
            n_s += 8
            torch.cuda.synchronize(dev)
            if reduce_max([time.perf_counter() - t_s])[0] >= settle_s:
                break
        settle[0] += n_s
        for _ in range(warmup):
            step()
        se.wait_exchange()
        torch.cuda.synchronize(dev)
        if se.wait() != 0:
            raise SystemExit(f"rank {rank}: evaluation failed during warm-up")
        ev.reset_kernel_stats()
        barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        se.wait_exchange()  # every overlapped all-reduce finishes inside the timed region
        torch.cuda.synchronize(dev)
        barrier()
        elapsed = time.perf_counter() - t0
        status = se.wait()
        _, total_ms, launches = ev.kernel_stats()
        kernel_ms = total_ms / max(launches, 1)
        elapsed_max, kernel_max, status_max = reduce_max([elapsed, kernel_ms, float(status)])
        if status_max != 0:
            raise SystemExit(f"evaluation failed (status {status_max})")
        return elapsed_max, kernel_ms, kernel_max

    # ---- the headline step -------------------------------------------------
    if args.mode in ("spmv", "cgnr"):
        se.evaluate(residuals=True, jacobian=True, gradient=False)
        ne = prog.num_effective_parameters
        pvec = torch.ones(ne, dtype=f64, device=dev)
        dvec = torch.full((ne,), 0.5, dtype=f64, device=dev)
        jp = torch.zeros(prog.num_residuals, dtype=f64, device=dev)
        jtjp = torch.zeros(ne, dtype=f64, device=dev)
    if args.mode == "schur":
        se.evaluate(residuals=True, jacobian=True, gradient=False)
        e_cols, f_cols = ev.schur_structure()
        ne = prog.num_effective_parameters
        dvec = torch.full((ne,), 0.5, dtype=f64, device=dev)
        bvec = -se.residuals
        srhs = torch.empty(f_cols, dtype=f64, device=dev)
        torch.cuda.synchronize(dev)
        t_init = time.perf_counter()
        ev.schur_init_device(se.jacobian.data_ptr(), dvec.data_ptr(), bvec.data_ptr(),
                             srhs.data_ptr(), ca._cse.SCHUR_JACOBI)
        torch.cuda.synchronize(dev)
        schur_init_ms = (time.perf_counter() - t_init) * 1e3
        sx = torch.ones(f_cols, dtype=f64, device=dev)
        sy = torch.empty(f_cols, dtype=f64, device=dev)
    if args.mode == "candidate":
        delta = torch.full((prog.num_effective_parameters,), 1e-6, dtype=f64, device=dev)
        cand = torch.empty_like(se.state)

    overlap = world > 1 and backend == "nccl" and not args.no_overlap
    cost_ring = torch.zeros(64, dtype=f64, device=dev)  # one cost slot per in-flight step
    ring = [0]

    def step():
        if args.mode == "jacobian":
            k = ring[0] % cost_ring.numel()
            if overlap and k == 0:
                se.wait_exchange()  # the slots are about to be reused
            ring[0] += 1
            se.evaluate(residuals=True, jacobian=True, gradient=args.gradient,
                        cost=cost_ring[k:k + 1], overlap=overlap)
        elif args.mode == "residual":
            se.evaluate(residuals=True, jacobian=False, gradient=False)
        elif args.mode == "candidate":
            ev.plus_device(se.state.data_ptr(), delta.data_ptr(), cand.data_ptr())
            ev.evaluate_device(cand.data_ptr(), se.cost.data_ptr(), None, None, None)
            if se.exchange:
                se._all_reduce(se.cost)
        elif args.mode == "schur":
            ev.schur_multiply_device(sx.data_ptr(), sy.data_ptr())
        elif args.mode == "cgnr":  # one pass: J^T J p + D^2 p (cse_cgnr_multiply)
            ev.cgnr_multiply_device(se.jacobian.data_ptr(), dvec.data_ptr(), pvec.data_ptr(),
                                    jtjp.data_ptr())
        else:
            ev.right_multiply_device(se.jacobian.data_ptr(), pvec.data_ptr(), jp.data_ptr())
            ev.left_multiply_device(se.jacobian.data_ptr(), jp.data_ptr(), jtjp.data_ptr())

    settle = [0]
    elapsed, kernel_ms, kernel_ms_max = run_leg(step, args.steps, args.warmup, args.settle)
    settle_steps = settle[0]
    if args.dump_outputs:  # before a later leg writes the same buffers
        if args.mode == "jacobian":
            last = (ring[0] - 1) % cost_ring.numel()  # the last timed step's cost slot
            outputs = {"cost": cost_ring[last:last + 1], "residuals": se.residuals,
                       "jacobian": se.jacobian}
            if args.gradient:
                outputs["gradient"] = se.gradient
        elif args.mode == "residual":
            outputs = {"cost": se.cost, "residuals": se.residuals}
        elif args.mode == "candidate":
            outputs = {"cost": se.cost, "candidate": cand}
        elif args.mode == "spmv":
            outputs = {"jp": jp, "jtjp": jtjp}
        elif args.mode == "cgnr":
            outputs = {"jtjp": jtjp}
        else:
            outputs = {"sy": sy}
        dump_outputs(args.dump_outputs, outputs, rank)
    if args.mode in ("spmv", "cgnr", "schur"):  # no evaluate launches in the loop: the step time
        kernel_ms = kernel_ms_max = elapsed / args.steps * 1e3

    # Compulsory bytes per launch on this rank (SURVEY.md §8 d).
    ne, nres, nj = prog.num_effective_parameters, prog.num_residuals, prog.num_jacobian_values
    npt = se.shard.points[1] - se.shard.points[0]
    bytes_launch = {
        "jacobian": info.bytes_jacobian_eval + (8 * ne if args.gradient else 0),
        "residual": info.bytes_residual_eval,
        # the timed kernel is the cost-only evaluation (no residual stores)
        "candidate": info.bytes_residual_eval - 8 * nres,
        "spmv": 2 * 8 * nj,  # J read twice (vectors are small next to it)
        "cgnr": 8 * nj + 4 * 8 * ne,  # J once, p, D and y
        # J once, the block ids, (E^T E + D_e^2)^-1 per point, x, D_f and y
        "schur": 8 * nj + 8 * prog.num_residual_blocks + 48 * npt + 3 * 8 * (ne - 3 * npt),
    }[args.mode]
    def reduce_sum(v):
        if world == 1:
            return float(v)
        t = torch.tensor([float(v)], dtype=f64, device="cpu" if backend == "gloo" else dev)
        dist.all_reduce(t)
        return float(t.item())

    tot_bytes = reduce_sum(bytes_launch)
    nblk = se.shard.blocks[1] - se.shard.blocks[0]
    store_eligible = (args.format == "block_sparse" and args.mode == "jacobian" and
                      group_store_eligible(se.residuals.data_ptr(), se.jacobian.data_ptr(), nblk))
    # Per GPU: the ranks' bytes / N over the slowest rank's kernel time.
    achieved = tot_bytes / world / (kernel_ms_max * 1e-3) / 1e9
    value = units * args.steps / elapsed

    # ---- secondary legs --------------------------------------------------
    secondary = {}
    if args.full and args.mode == "jacobian" and not args.no_secondary:
        ks = args.secondary_steps

        def leg(name, fn, nbytes, steps, what):
            # Untimed warm-up of at least 0.1 s (the GPU's clocks settle over
            # tens of ms; a short leg right after another phase reads slow).
            t_w, n_w = time.perf_counter(), 0
            while n_w < 2 or time.perf_counter() - t_w < 0.1:
                fn()
                n_w += 1
                if n_w % 16 == 0:
                    torch.cuda.synchronize(dev)
            e, k, kmax = run_leg(fn, steps, 0)
            tb = reduce_sum(nbytes)
            ach = tb / world / (kmax * 1e-3) / 1e9
            secondary[name] = {"value": units * steps / e, "unit": "evals/s", "warmup": n_w,
                               "ms_per_step": e / steps * 1e3, "steps": steps,
                               "kernel_ms_avg": k, "kernel_ms_avg_max_rank": kmax,
                               "algorithmic_bytes_per_launch": nbytes,
                               "achieved_GBps": ach, "frac": ach / PEAK_HBM_GBPS, "what": what}

        if not args.gradient:
            leg("gradient", lambda: se.evaluate(residuals=True, jacobian=True, gradient=True),
                info.bytes_jacobian_eval + 8 * ne, ks,
                "residuals + Jacobian + gradient J^T r + cost (deterministic gradient_mode 0: "
                "point rows fused into the evaluation, camera rows re-evaluated in camera "
                "order; what TrustRegionMinimizer requests); bytes add 8 per "
                "effective parameter")
        leg("same_point", lambda: se.evaluate(residuals=True, jacobian=True, gradient=False,
                                              new_evaluation_point=False),
            info.bytes_jacobian_eval, ks,
            "the headline evaluation with new_evaluation_point = false (CSE_EVAL_SAME_POINT), "
            "as TrustRegionMinimizer evaluates the Jacobian at a just-accepted candidate "
            "(trust_region_minimizer.cc:822-826): the slot-0 table repacked for that point "
            "by the candidate's evaluation is reused")
        leg("residual_only", lambda: se.evaluate(residuals=True, jacobian=False, gradient=False),
            info.bytes_residual_eval, ks, "residuals + cost (trust-region candidate evaluation)")
        hres, hjac = se.host_buffers()

        def host_step():
            se.evaluate(residuals=True, jacobian=True, gradient=False)
            se.copy_strips_to_host(hres, hjac)

        e, _, _ = run_leg(host_step, args.host_steps, 1)
        d2h = se.d2h_bytes()
        secondary["host_strips"] = {
            "value": units * args.host_steps / e, "unit": "evals/s",
            "ms_per_step": e / args.host_steps * 1e3, "steps": args.host_steps,
            "d2h_bytes_per_rank": d2h, "d2h_GBps_per_rank": d2h * args.host_steps / e / 1e9,
            "what": "evaluation + D2H of each rank's residual and Jacobian strips into pinned "
                    "host memory every step (the reference's seam; PCIe-inclusive, not the "
                    "headline value)"}
        del hres, hjac

        if world == 1 and not variant:
            # The same evaluation with the Jacobian by forward-mode
            # Jet<double, 12> (cse_options.jacobian_form = CSE_JACOBIAN_JET),
            # as AutoDifferentiate computes it for any AutoDiffCostFunction
            # (autodiff.h:314-381): its own evaluator over the same program,
            # writing the headline's buffers.
            jev = ca.Evaluator(prog, device=dev_index, profile=True, stream=stream.cuda_stream,
                               jacobian_form="jet")
            saved = se, ev
            st_, cost_, res_, jac_ = se.state, se.cost, se.residuals, se.jacobian

            class _JetLeg:  # what run_leg needs of `se`
                def wait_exchange(self):
                    pass

                def wait(self):
                    return jev.wait()

            se, ev = _JetLeg(), jev
            try:
                leg("jet", lambda: jev.evaluate_device(st_.data_ptr(), cost_.data_ptr(), res_.data_ptr(),
                                                       None, jac_.data_ptr()),
                    info.bytes_jacobian_eval, ks,
                    "the headline evaluation with the Jacobian by forward-mode Jet<double, 12> "
                    "(cse_options.jacobian_form = CSE_JACOBIAN_JET; AutoDifferentiate, "
                    "autodiff.h:314-381) instead of the closed-form Snavely Jacobian: "
                    "EvaluateAffineChunksTwoRoundW1<SnavelyJetKind, ...>")
            finally:
                se, ev = saved
                jev.close()
            # The same workload with a user functor (BundlerResidual through
            # cse_register_functor, its kernels compiled in the example's
            # TU): the Jet<double, 12> evaluation of the user's own code,
            # the same kernel template as the library's Jet form.
            import copy
            import dataclasses
            uprog = copy.copy(prog)
            uname = {"trivial": "BundlerResidual/Trivial", "huber": "BundlerResidual/Huber"}.get(args.loss)
            if uname is not None:
                uprog.groups = [dataclasses.replace(g, kind=user_functor_kind(uname)) for g in prog.groups]
                uev = ca.Evaluator(uprog, device=dev_index, profile=True, stream=stream.cuda_stream)
                uinfo = uev.info()
                saved = se, ev

                class _UserLeg:
                    def wait_exchange(self):
                        pass

                    def wait(self):
                        return uev.wait()

                se, ev = _UserLeg(), uev
                try:
                    leg("user_functor",
                        lambda: uev.evaluate_device(st_.data_ptr(), cost_.data_ptr(), res_.data_ptr(),
                                                    None, jac_.data_ptr()),
                        uinfo.bytes_jacobian_eval, ks,
                        f"the headline workload with a user functor: {uname} "
                        "(bundle_adjustment_test_util.h:188-227) compiled in a user TU against "
                        "ceres_amd/autodiff_cuda.h (examples/user_functors.hip), registered by "
                        "cse_register_functor; residuals + Jacobian (Jet<double, 12>) + cost: "
                        "EvaluateAffineChunksTwoRoundW1<UserKind<BundlerResidual, ...>, ...>")
                    secondary["user_functor"]["affine"] = uinfo.num_affine_groups == 1
                finally:
                    se, ev = saved
                    uev.close()
        if world == 1 and args.config == "problem-13682-4456117" and not variant:
            # BASELINE.json configs[2] (problem-1778, HuberLoss,
            # CompressedRowSparseMatrix) in the same driver-timed run: its own
            # evaluator, the same timed-loop rules as the headline.
            c2 = bal.synthetic(*bal.CONFIGS["problem-1778-993923"], seed=args.seed)
            se2 = distributed.ShardedEvaluator(*c2, 0, 1, device=dev_index, loss=ca.Loss.huber(1.0),
                                               format=ca.COMPRESSED_ROW, gradient=False,
                                               stream=stream)
            del c2
            info2 = se2.evaluator.info()
            saved = se, ev
            se, ev = se2, se2.evaluator  # run_leg times the evaluator held in `se`, `ev`
            try:
                leg("configs2", lambda: se2.evaluate(residuals=True, jacobian=True, gradient=False),
                    info2.bytes_jacobian_eval, max(ks, 200),
                    "BASELINE configs[2]: problem-1778-993923 (1,778 cameras, 993,923 points, "
                    "5,001,946 blocks), SnavelyReprojectionError<2,9,3>, HuberLoss(1.0), "
                    "CompressedRowSparseMatrix, residuals + Jacobian + cost, device-resident")
            finally:
                se, ev = saved
                se2.close()
        if world == 1 and args.scaling == "strong":
            # The reference's seam served by one process over every visible
            # device (cse_create_multi): point-bucket shards, each device's
            # residual and Jacobian strips copied into the caller's one host
            # buffer (page-locked on the first call), cost and gradient summed
            # over the shards on the host.
            devices = list(range(ndev))
            mev = ca.Evaluator(prog, devices=devices, profile=True)
            bufs = (np.empty(prog.num_residuals), None, np.empty(prog.num_jacobian_values))
            hstate = np.array(prog.state)
            pinned = [hstate, bufs[0], bufs[2]]
            for a in pinned:  # page-locked by the caller (cse_host_register)
                ca.host_register(a)
            hs = max(2, args.host_steps)
            mev.evaluate(hstate, residuals=True, gradient=False, jacobian=True, out=bufs)
            t0 = time.perf_counter()
            for _ in range(hs):
                ok = mev.evaluate(hstate, residuals=True, gradient=False, jacobian=True, out=bufs)[0]
                assert ok
            e = time.perf_counter() - t0
            first, _ = mev.shard_info()
            h2d, d2h = mev.transfer_bytes()
            mev.close()
            for a in pinned:
                ca.host_unregister(a)
            secondary["host_multi"] = {
                "value": hs / e, "unit": "evals/s", "ms_per_step": e / hs * 1e3, "steps": hs,
                "devices": devices, "shard_first_blocks": [int(x) for x in first],
                "state_h2d_bytes_per_shard": [int(x) for x in h2d],
                "strips_d2h_bytes_per_shard": [int(x) for x in d2h],
                "d2h_bytes": 8 * (prog.num_residuals + prog.num_jacobian_values),
                "d2h_GBps": 8 * (prog.num_residuals + prog.num_jacobian_values) * hs / e / 1e9,
                "what": "cse_evaluate on a cse_create_multi evaluator over every visible device "
                        "(host state in, residuals + Jacobian values out in the caller's one host "
                        "buffer; PCIe-inclusive, not the headline value)"}
            del bufs

    if args.full and args.mode == "schur" and not args.no_secondary and world == 1:
        # One trust-region step's front end on the device, two ways
        # (VERDICT r5 #6): the evaluation writes the gradient (gradient_mode
        # 0, CameraGradientKernel) and cse_schur_init follows, or the
        # evaluation skips the gradient and cse_schur_init_gradient forms
        # g = J^T r from the same pass over J.  b = -r is refreshed from the
        # evaluation's residuals in both, as the minimizer would.
        ks = max(args.secondary_steps // 4, 10)
        gvec = torch.empty(ne, dtype=f64, device=dev)

        def with_gradient():
            se.evaluate(residuals=True, jacobian=True, gradient=True)
            torch.neg(se.residuals, out=bvec)
            ev.schur_init_device(se.jacobian.data_ptr(), dvec.data_ptr(), bvec.data_ptr(),
                                 srhs.data_ptr(), ca._cse.SCHUR_JACOBI)

        def init_gradient():
            se.evaluate(residuals=True, jacobian=True, gradient=False)
            torch.neg(se.residuals, out=bvec)
            ev.schur_init_gradient_device(se.jacobian.data_ptr(), dvec.data_ptr(), bvec.data_ptr(),
                                          srhs.data_ptr(), gvec.data_ptr(), ca._cse.SCHUR_JACOBI)

        def init_only():
            ev.schur_init_device(se.jacobian.data_ptr(), dvec.data_ptr(), bvec.data_ptr(),
                                 srhs.data_ptr(), ca._cse.SCHUR_JACOBI)

        def init_gradient_only():
            ev.schur_init_gradient_device(se.jacobian.data_ptr(), dvec.data_ptr(), bvec.data_ptr(),
                                          srhs.data_ptr(), gvec.data_ptr(), ca._cse.SCHUR_JACOBI)

        for name, fn, what in (
                ("eval_gradient_then_init", with_gradient,
                 "evaluation with gradient (gradient_mode 0) + b = -r + cse_schur_init"),
                ("eval_then_init_gradient", init_gradient,
                 "evaluation without gradient + b = -r + cse_schur_init_gradient (g from the "
                 "init's pass over J)"),
                ("init", init_only, "cse_schur_init alone"),
                ("init_gradient", init_gradient_only, "cse_schur_init_gradient alone")):
            for _ in range(3):
                fn()
            e, _, _ = run_leg(fn, ks, 0)
            secondary[name] = {"value": ks / e, "unit": "steps/s", "ms_per_step": e / ks * 1e3,
                               "steps": ks, "what": what}

    # Every rank's block range, gathered (the shard cuts of
    # shard.point_bucket_cuts as each rank built them): they must tile
    # [0, observations) in rank order.
    cuts = [0] * (2 * world)
    cuts[2 * rank], cuts[2 * rank + 1] = se.shard.blocks
    if world > 1:
        ct = torch.tensor(cuts, dtype=torch.int64, device="cpu" if backend == "gloo" else dev)
        dist.all_reduce(ct)
        cuts = [int(v) for v in ct.cpu()]
    block_cuts = cuts[0::2] + [cuts[-1]]
    if strong and (block_cuts[0] != 0 or block_cuts[-1] != bal.CONFIGS[args.config][2] or
                   any(cuts[2 * r + 1] != cuts[2 * r + 2] for r in range(world - 1))):
        raise SystemExit(f"shard block ranges do not tile the problem: {cuts}")

    out = None
    if rank == 0:
        cpu = None
        if arrays is not None:
            aff = len(os.sched_getaffinity(0))
            omp = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
            quota, _ = _cpu_quota()
            share = (max(1, min(int(quota), aff)) if quota is not None
                     else min(omp, aff) if omp > 0 else aff)
            threads = args.cpu_threads or _host_info()["physical_cores_in_affinity"]
            cpu = cpu_baseline(args, arrays, threads, share)
        traffic = None
        pmc_path = os.path.join(REPO, "profiles", f"pmc_{args.config}_{args.loss}_{args.format}.json")
        if (world == 1 and args.mode == "jacobian" and not args.gradient and not variant
                and os.path.exists(pmc_path)):
            with open(pmc_path) as fh:
                traffic = json.load(fh).get("hbm_bytes_per_launch")
        C_, P_, O_ = counts
        sh = se.shard
        out = {
            "metric": METRIC if args.mode == "jacobian" and not variant else
                      f"{args.mode} evaluations/sec on BAL {args.config}"
                      f"{' with quaternion cameras on their manifold' if quat else ''}"
                      f"{f' with {args.held_cameras} held camera(s)' if args.held_cameras else ''}"
                      " (not the headline)",
            "value": value,
            "unit": "evals/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "settle_steps": settle_steps,
            "ms_per_step": elapsed / args.steps * 1e3,
            "full": args.full,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic (BAL-shaped: exact header counts, seeded generator)",
            "config": {
                "workload": f"{args.config} "
                            + ("SnavelyReprojectionErrorWithQuaternions<2,10,3>, cameras on "
                               "ProductManifold<QuaternionManifold, EuclideanManifold<6>> "
                               if quat else "SnavelyReprojectionError<2,9,3> ")
                            + (f"{args.held_cameras} camera(s) held constant, " if args.held_cameras else "")
                            + f"{args.loss} {args.format} "
                            + {"jacobian": "residual+Jacobian", "residual": "residual+cost",
                               "candidate": "Plus + cost-only",
                               "spmv": "J p + J^T (J p)",
                               "cgnr": "J^T J p + D^2 p (one pass)",
                               "schur": "S p, implicit Schur complement"}[args.mode]
                            + f"{'+gradient' if args.gradient else ''}, device-resident",
                "cameras": C_, "points": P_, "observations": O_,
                "blocks_rank0": sh.blocks[1] - sh.blocks[0],
                "block_cuts": block_cuts if strong else None,
                "parallelism": (f"rank 0's shard of {args.shard_of} (one process)" if args.shard_of > 1
                                else "single GPU" if world == 1 else
                                f"point-bucket block sharding x{world}" if strong else
                                f"replica shards x{world}"),
                "exchange": (None if world == 1 else
                             f"all-reduce of the cost{' and camera gradient rows' if args.gradient else ''}"
                             f" over {'RCCL' if backend == 'nccl' else backend}"
                             + (", the cost's overlapped with the next evaluation" if overlap else "")),
                "rehearsal": (f"{world} ranks on {ndev} GPU(s), gloo" if rehearsal else None),
                "strip_rank0": {"residuals": list(sh.residual_strip),
                                "jacobian": [[g, g + n] for _, g, n in sh.jacobian_strips()]},
            },
            "roofline": {
                "bound": "hbm",
                "achieved": achieved,
                "peak": PEAK_HBM_GBPS,
                "unit": "GB/s",
                "frac": achieved / PEAK_HBM_GBPS,
                "traffic": traffic,
                "algorithmic_bytes_per_launch": tot_bytes / world,
                "kernel_ms_avg": kernel_ms,
                "kernel_ms_avg_max_rank": kernel_ms_max,
                "kernel": f"cse::EvaluateAffineChunks"
                          f"{'FusedPointsW1' if args.gradient else (('GroupStore' if not quat and not args.held_cameras and store_eligible else 'TwoRoundW1') if args.format == 'block_sparse' else 'TwoRoundCrsW1')}"
                          f"<{'SnavelyQuaternionTangentKind' if quat else 'SnavelyKind'}, {args.loss}, {args.format}> (+ repack"
                          f"{', CameraGradientKernel and the gradient tail' if args.gradient else ''})",
                "per": "GPU (bytes of all ranks / N over the slowest rank's kernel time)",
                "traffic_source": "profiles/pmc_<config>_<loss>_<format>.json (rocprofv3 "
                                  "FETCH_SIZE/WRITE_SIZE of the same kernel)",
            },
            "secondary": secondary,
            "schur_init_ms": schur_init_ms if args.mode == "schur" else None,
            "parity": ("outputs checked against the oracle (Ceres' CPU ProgramEvaluator restated, "
                       "oracle/) by tests/ at Eigen isApprox 1e-13 per vector "
                       "(evaluator_cuda_test.cu.cc:61) plus 1e-10 per element, except the Jacobian "
                       "cells and gradient rows of cameras with 0 < theta < 1e-3 (series Rodrigues "
                       "form), held to 1e-7 against the reference form and 1e-13 against 40-digit "
                       "values (DESIGN.md section 6 item 5); the synthetic workload has no such "
                       "camera"),
            "cpu_baseline": cpu,
            "speedup_vs_cpu": (value / world / cpu["value"]) if cpu else None,
            "build_s": build_s,
            "reference_published": {"value": 0.6455, "unit": "evals/s",
                                    "what": "V100 Jacobian&residual eval incl. H2D/D2H, no loss, "
                                            "README.md:189 (not the same metric)"},
        }
        print(json.dumps(out), flush=True)
    se.close()
    if world > 1:
        barrier()
        dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main()
