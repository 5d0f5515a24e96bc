"""bundle_adjuster-style driver over the MI355X evaluator.

Mirrors the flow of examples/bundle_adjuster.cu.cc around the hot path:
read a BAL file (or build a synthetic one), Normalize(), Perturb(), put the
residual blocks in Schur order, and run Levenberg-Marquardt iterations
whose every evaluation is the HIP evaluator and whose linear solve is a
preconditioned CG on the device's implicit Schur complement
(--linear_solver iterative_schur, the reference benchmark's solver, with its
jacobi / schur_jacobi / identity preconditioners) or on the normal equations
(--linear_solver cgnr), or -- DENSE_SCHUR, for up to a few hundred cameras --
the explicit dense Schur complement formed on the device and its Cholesky
factorization (--linear_solver dense_schur; --dense_linear_algebra_library cse
factors S with the library's own Cholesky, in FP64 or, with
--mixed_precision_solves, in FP32 with FP64 refinement, where the default is
torch's); no Jacobian value leaves HBM.  Prints a FullReport-style table of the evaluator timers
(solver.cc: "Residual only evaluation", "Jacobian & residual evaluation",
"Linear solver", "Plus").

The minimizer here is deliberately small (a driver that exercises the
path, not a port of Ceres' TrustRegionMinimizer, which stays Ceres'):
LM damping D = diag(J^T J) with Ceres' default radius policy
(levenberg_marquardt_strategy.cc: radius / (1 / 3 ... 2) updates), a
candidate accepted when the cost decreases.

    python -m ceres_amd.bundle_adjuster --synthetic problem-16-22106 \\
        --robustify --point_sigma 0.01 --num_iterations 5
"""
import argparse
import os
import sys
import time

import numpy as np

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ceres_amd as ca  # noqa: E402
from ceres_amd import bal  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--input", help="BAL problem file (text)")
    src.add_argument("--synthetic", type=bal.synthetic_name, metavar="SHAPE",
                     help="synthetic BAL shape: " + ", ".join(bal.CONFIGS) + ", or one with local visibility, "
                          "banded-C-P-wW (C cameras, P points, 4 P observations, each point's cameras from a "
                          "window of W consecutive ones) or banded-C-P-O-wW")
    ap.add_argument("--robustify", action="store_true", help="HuberLoss(1.0)")
    ap.add_argument("--use_quaternions", action="store_true",
                    help="10-parameter cameras {q, t, f, k1, k2} (bal_problem.cc:110-121)")
    ap.add_argument("--use_manifolds", action="store_true",
                    help="with --use_quaternions: every camera on ProductManifold<QuaternionManifold, "
                         "EuclideanManifold<6>> (bundle_adjuster.cc:337-345)")
    ap.add_argument("--format", default="block_sparse", choices=["block_sparse", "compressed_row"])
    ap.add_argument("--rotation_sigma", type=float, default=0.0)
    ap.add_argument("--translation_sigma", type=float, default=0.0)
    ap.add_argument("--point_sigma", type=float, default=0.0)
    ap.add_argument("--num_iterations", type=int, default=5)
    ap.add_argument("--max_linear_solver_iterations", type=int, default=500)
    ap.add_argument("--eta", type=float, default=1e-2, help="CG forcing tolerance")
    ap.add_argument("--initial_trust_region_radius", type=float, default=1e4)
    ap.add_argument("--linear_solver", default="iterative_schur",
                    choices=["iterative_schur", "cgnr", "dense_schur", "sparse_schur"],
                    help="iterative_schur (the reference benchmark's, README.md:143-184): PCG on "
                         "the implicit Schur complement (cse_schur_*); cgnr: PCG on the normal "
                         "equations (cse_cgnr_multiply); dense_schur: the dense reduced camera "
                         "matrix (cse_schur_complement) and its Cholesky factorization; "
                         "sparse_schur: the block-sparse reduced camera matrix "
                         "(cse_schur_complement_sparse) and its block-sparse Cholesky "
                         "factorization (cse_sparse_cholesky_*), analysed once per run")
    ap.add_argument("--sparse_ordering", default="minimum_degree", choices=["minimum_degree", "natural"],
                    help="sparse_schur: the elimination order of the cameras "
                         "(Solver::Options::linear_solver_ordering_type; minimum_degree is the library's "
                         "greedy rule, not SuiteSparse's AMD)")
    ap.add_argument("--max_schur_gb", type=float, default=16.0,
                    help="dense_schur: refuse when the plan and the dense S together take more; "
                         "--use_explicit_schur_complement: the plan, the structure and the blocks of S")
    ap.add_argument("--dense_linear_algebra_library", default="torch", choices=["torch", "cse"],
                    help="dense_schur: what factors S.  torch: torch.linalg.cholesky_ex; cse: the "
                         "library's own factorization (cse_dense_cholesky_factorize, "
                         "Solver::Options::dense_linear_algebra_library_type = CUDA), no host copy "
                         "of S or of the step")
    ap.add_argument("--mixed_precision_solves", action="store_true",
                    help="with --dense_linear_algebra_library cse: factor a float copy of S and refine "
                         "in FP64 (Solver::Options::use_mixed_precision_solves)")
    ap.add_argument("--max_num_refinement_iterations", type=int, default=0,
                    help="refinement steps of a mixed precision solve "
                         "(Solver::Options::max_num_refinement_iterations)")
    ap.add_argument("--use_explicit_schur_complement", action="store_true",
                    help="iterative_schur only (bundle_adjuster.cc's flag, Solver::Options::"
                         "use_explicit_schur_complement): form the block-sparse S once per linear solve "
                         "(cse_schur_complement_sparse) and run the PCG on it (cse_schur_explicit_multiply) "
                         "instead of on the implicit operator.  Not a faster solve on the shapes measured "
                         "(level at 49 cameras, slower beyond): see DESIGN 3.6b")
    ap.add_argument("--preconditioner", default="jacobi",
                    choices=["identity", "jacobi", "schur_jacobi", "schur_power_series_expansion",
                             "cluster_jacobi", "cluster_tridiagonal"],
                    help="iterative_schur's preconditioner (bundle_adjuster.cc default: jacobi); "
                         "cluster_jacobi: the blocks of S over the camera clusters of "
                         "--visibility_clustering, factored once per linear solve "
                         "(cse_schur_cluster_jacobi), in the host loop and with --device_pcg; not with "
                         "--held_cameras; "
                         "cluster_tridiagonal: besides those blocks the blocks of S between the clusters "
                         "that a degree-2 maximum spanning forest of the cluster graph joins, factored "
                         "along the forest's paths (cse_schur_cluster_tridiagonal), under the same flags "
                         "and refusals; "
                         "schur_power_series_expansion: --max_num_spse_iterations terms of the series "
                         "of S^-1 per application (cse_schur_power_series), in the host loop and with "
                         "--device_pcg; not with --use_explicit_schur_complement, as the reference")
    ap.add_argument("--visibility_clustering", default="single_linkage", choices=["single_linkage", "blocks"],
                    help="cluster_jacobi's camera partition.  single_linkage (the reference's): the "
                         "connected components of the visibility graph's edges with weight "
                         "|V_i n V_j| / sqrt(|V_i| |V_j|) >= --cluster_min_similarity, a larger cluster "
                         "cut into runs of --max_cluster_cameras; blocks (not the reference's): "
                         "consecutive runs of --max_cluster_cameras cameras, for the synthetic shapes, "
                         "whose uniformly drawn visibility leaves single linkage with singletons.  The "
                         "reference's canonical_views clustering is not implemented")
    ap.add_argument("--cluster_min_similarity", type=float, default=0.9,
                    help="single_linkage's threshold (the reference's 0.9)")
    ap.add_argument("--max_cluster_cameras", type=int, default=None,
                    help="cameras in a cluster at most (default 16; 8 for cluster_tridiagonal); 16 is also "
                         "the most the device takes (one cluster, or the two clusters of a forest edge, "
                         "is factored in one workgroup's LDS)")
    ap.add_argument("--max_num_spse_iterations", type=int, default=5,
                    help="terms of the power series, for the preconditioner and for "
                         "--use_spse_initialization (bundle_adjuster.cc's flag)")
    ap.add_argument("--use_spse_initialization", action="store_true",
                    help="iterative_schur only (Solver::Options::use_spse_initialization): start the PCG "
                         "from x0 = the power series of S^-1 applied to the right-hand side, up to "
                         "--max_num_spse_iterations terms or until a term's norm is below "
                         "--spse_tolerance of the first; with every preconditioner and with held cameras")
    ap.add_argument("--spse_tolerance", type=float, default=0.1,
                    help="--use_spse_initialization: stop the series at a term below this fraction of "
                         "the zeroth term's norm")
    ap.add_argument("--device_pcg", action="store_true",
                    help="iterative_schur only: the whole PCG as one call (cse_schur_solve: the "
                         "reference's ConjugateGradientsSolver with its vectors, scalars and stopping "
                         "tests on the device) instead of the torch loop on the host; with "
                         "--use_explicit_schur_complement it iterates on the block-sparse S.  Half "
                         "the host loop's time at 49 cameras, 3 %% behind it at 1,778 (DESIGN 3.6c)")
    ap.add_argument("--pcg_termination", default="residual", choices=["residual", "quadratic"],
                    help="residual: |r| <= eta |b| (the host loop's test; r_tolerance = eta, "
                         "q_tolerance = 0, no residual reset); quadratic: Ceres' LM setting, "
                         "q_tolerance = eta, r_tolerance = -1 (levenberg_marquardt_strategy.cc:98-103); "
                         "needs --device_pcg")
    ap.add_argument("--pcg_check_period", type=int, default=1,
                    help="--device_pcg: the host looks at the device state after this many enqueued "
                         "iterations.  Up to period - 1 iterations run past the end (their result is "
                         "discarded on the device): 4 where the iteration is launch-bound (best "
                         "measured at 49 cameras; 16 already loses to the trailing iterations), 1 "
                         "from about a thousand cameras on, where a product is long against a host "
                         "wait; DESIGN 3.6c")
    ap.add_argument("--device_cgnr", action="store_true",
                    help="cgnr only: CudaCgnrSolver on the device (cgnr_solver.cc:218-387) instead of the "
                         "torch loop on the host: per solve cse_cgnr_init(J, sqrt(lambda D), -r) -- the "
                         "right-hand side J^T b and the preconditioner -- and cse_cgnr_solve with "
                         "r_tolerance = eta, q_tolerance = 0 and no residual reset, from the zero start")
    ap.add_argument("--cgnr_preconditioner", default="jacobi", choices=["jacobi", "identity"],
                    help="--device_cgnr: jacobi is the reference's BlockCRSJacobiPreconditioner, per "
                         "parameter block (sum J^T J + D^2)^-1 (the host loop's is the scalar "
                         "1 / ((1 + lambda) diag J^T J))")
    ap.add_argument("--cgnr_check_period", type=int, default=1,
                    help="--device_cgnr: the host looks at the device state after this many enqueued "
                         "iterations (as --pcg_check_period)")
    ap.add_argument("--jacobi_scaling", action="store_true",
                    help="Solver::Options::jacobi_scaling (on by default in the reference, off here so "
                         "that earlier runs keep their iterates): at iteration 0 scaling = 1 / (1 + "
                         "sqrt(squared column norm)) (cse_jacobian_squared_column_norm), every Jacobian "
                         "is scaled in place (cse_jacobian_scale_columns), the LM diagonal is the norm "
                         "of the scaled Jacobian clamped to [1e-6, 1e32], the linear solver runs on the "
                         "scaled Jacobian and the step is un-scaled for Plus "
                         "(trust_region_minimizer.cc:259-275, 443-446)")
    ap.add_argument("--held_cameras", type=int, default=0,
                    help="hold cameras 0 .. N-1 constant (Problem::SetParameterBlockConstant, e.g. to fix "
                         "the gauge): they get no columns, and the Schur solvers run on the active "
                         "cameras' 9 (C - N) f columns.  With iterative_schur (host loop and --device_pcg, "
                         "every preconditioner) and cgnr; the explicit Schur complements (dense_schur, "
                         "--use_explicit_schur_complement) do not take held cameras")
    args = ap.parse_args(argv)
    if args.held_cameras < 0:
        raise SystemExit("--held_cameras must not be negative")
    if args.dense_linear_algebra_library == "cse" and args.linear_solver != "dense_schur":
        raise SystemExit(f"--dense_linear_algebra_library cse needs --linear_solver dense_schur, not "
                         f"{args.linear_solver}")
    if args.mixed_precision_solves and args.dense_linear_algebra_library != "cse":
        raise SystemExit("--mixed_precision_solves needs --dense_linear_algebra_library cse")
    if args.max_num_refinement_iterations < 0:
        raise SystemExit("--max_num_refinement_iterations must not be negative")
    if args.linear_solver == "sparse_schur":
        # What sparse_schur does not take, one message each (--dense_linear_algebra_library
        # cse and --mixed_precision_solves have met theirs above).
        if args.held_cameras:
            raise SystemExit("--held_cameras needs --linear_solver iterative_schur or cgnr, not sparse_schur "
                             "(the explicit Schur complement does not take held cameras)")
        for flag, given in (("--use_explicit_schur_complement", args.use_explicit_schur_complement),
                            ("--preconditioner " + args.preconditioner, args.preconditioner != "jacobi"),
                            ("--use_spse_initialization", args.use_spse_initialization),
                            ("--device_pcg", args.device_pcg),
                            ("--pcg_termination quadratic", args.pcg_termination == "quadratic")):
            if given:
                raise SystemExit(f"{flag} needs --linear_solver iterative_schur, not sparse_schur")
    if (args.max_num_refinement_iterations and not args.mixed_precision_solves
            and args.linear_solver != "sparse_schur"):
        raise SystemExit("--max_num_refinement_iterations needs --mixed_precision_solves (and "
                         "--dense_linear_algebra_library cse)")
    if args.held_cameras and args.linear_solver == "dense_schur":
        raise SystemExit("--held_cameras needs --linear_solver iterative_schur or cgnr, not dense_schur "
                         "(the explicit Schur complement does not take held cameras)")
    if args.held_cameras and args.use_explicit_schur_complement:
        raise SystemExit("--held_cameras does not go with --use_explicit_schur_complement "
                         "(the explicit Schur complement does not take held cameras)")
    if args.use_explicit_schur_complement and args.linear_solver != "iterative_schur":
        raise SystemExit("--use_explicit_schur_complement needs --linear_solver iterative_schur, not "
                         f"{args.linear_solver}")
    if args.max_cluster_cameras is None:
        args.max_cluster_cameras = 8 if args.preconditioner == "cluster_tridiagonal" else 16
    if args.preconditioner in ("cluster_jacobi", "cluster_tridiagonal"):
        if args.linear_solver != "iterative_schur":
            raise SystemExit(f"--preconditioner {args.preconditioner} needs --linear_solver iterative_schur, not "
                             f"{args.linear_solver}")
        if args.held_cameras:
            raise SystemExit(f"--preconditioner {args.preconditioner} does not go with --held_cameras (its pair "
                             "plan addresses F cells by block index, as the explicit Schur complement's)")
        if not 1 <= args.max_cluster_cameras <= 16:
            raise SystemExit("--max_cluster_cameras must be in [1, 16]")
        if not 0.0 <= args.cluster_min_similarity <= 1.0:
            raise SystemExit("--cluster_min_similarity must be in [0, 1]")
    series_pre = args.preconditioner == "schur_power_series_expansion"
    if (args.use_spse_initialization or series_pre) and args.linear_solver != "iterative_schur":
        raise SystemExit("--use_spse_initialization and --preconditioner schur_power_series_expansion need "
                         f"--linear_solver iterative_schur, not {args.linear_solver}")
    if args.use_spse_initialization and args.use_explicit_schur_complement:
        raise SystemExit("use_explicit_schur_complement does not support use_spse_initialization")
    if series_pre and args.use_explicit_schur_complement:
        raise SystemExit("use_explicit_schur_complement only supports SCHUR_JACOBI as the preconditioner, "
                         "not schur_power_series_expansion")
    if args.use_spse_initialization or series_pre:
        # solver.cc:277-281
        if args.max_num_spse_iterations < 1:
            raise SystemExit("--max_num_spse_iterations must be at least 1")
        if not (0.0 <= args.spse_tolerance < float("inf")):
            raise SystemExit("--spse_tolerance must be finite and not negative")
    if args.device_pcg and args.linear_solver != "iterative_schur":
        raise SystemExit(f"--device_pcg needs --linear_solver iterative_schur, not {args.linear_solver}")
    if args.pcg_termination == "quadratic" and not args.device_pcg:
        raise SystemExit("--pcg_termination quadratic needs --device_pcg")
    if args.pcg_check_period < 1:
        raise SystemExit("--pcg_check_period must be at least 1")
    if args.device_cgnr and args.linear_solver != "cgnr":
        raise SystemExit(f"--device_cgnr needs --linear_solver cgnr, not {args.linear_solver}")
    if args.cgnr_check_period < 1:
        raise SystemExit("--cgnr_check_period must be at least 1")
    return args


class Timers:
    def __init__(self):
        self.t = {}

    def add(self, name, seconds):
        tot, n = self.t.get(name, (0.0, 0))
        self.t[name] = (tot + seconds, n + 1)

    def report(self):
        lines = ["Time (in seconds):"]
        for name, (tot, n) in self.t.items():
            lines.append(f"  {name:<34s}{tot:12.6f} ({n})")
        return "\n".join(lines)


def cholesky_solve(S, rhs):
    """x with S x = rhs for the symmetric positive definite device matrix S
    (DenseSchurComplementSolver::SolveReducedLinearSystem's LLT), on the device;
    on the host with numpy where torch's device factorization is not available."""
    import torch
    try:
        L, info = torch.linalg.cholesky_ex(S)
        if int(info.item()) != 0:
            raise SystemExit(f"dense_schur: S is not positive definite (leading minor {int(info.item())})")
        return torch.cholesky_solve(rhs.unsqueeze(1), L).squeeze(1).contiguous()
    except RuntimeError:
        c = np.linalg.cholesky(S.cpu().numpy())
        y = np.linalg.solve(c, rhs.cpu().numpy())
        return torch.from_numpy(np.linalg.solve(c.T, y)).to(S.device)


def solve(args, stats=None):
    """stats (a dict, optional) receives "lm_diagonal": the (min, max) of every
    LM diagonal before its clamp, in the order they were taken, and with
    --jacobi_scaling "jacobi_scaling": the scaling's (min, max)."""
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    f64 = torch.float64
    timers = Timers()
    t0 = time.perf_counter()
    if args.input:
        cams, pts, ci, pi, obs = bal.read(args.input)
    else:
        cams, pts, ci, pi, obs = bal.synthetic_named(args.synthetic)
        cams, pts = cams.copy(), pts.copy()
    bal.normalize(cams, pts)
    bal.perturb(cams, pts, args.rotation_sigma, args.translation_sigma, args.point_sigma)
    order = bal.schur_residual_order(pi, pts.shape[0])
    loss = ca.Loss.huber(1.0) if args.robustify else None
    if args.use_quaternions:
        cams = bal.to_quaternion_cameras(cams)
    manifold = args.use_quaternions and args.use_manifolds
    if args.use_quaternions and not manifold and args.linear_solver != "cgnr":
        raise SystemExit(f"{args.linear_solver} takes 9-column cameras: add --use_manifolds or use cgnr")
    if args.held_cameras >= cams.shape[0]:
        raise SystemExit(f"--held_cameras {args.held_cameras}: the problem has {cams.shape[0]} cameras, "
                         "and one at least must stay free")
    prog = bal.program(cams, pts, ci[order], pi[order], obs[order], loss=loss, format=args.format,
                       quaternion_manifold=manifold, constant_cameras=range(args.held_cameras))
    timers.add("Preprocessor", time.perf_counter() - t0)

    stream = torch.cuda.current_stream(dev).cuda_stream
    ev = ca.Evaluator(prog, device=0, stream=stream)
    n, m = prog.num_effective_parameters, prog.num_residuals
    x = torch.from_numpy(prog.state).to(dev)
    cand = torch.empty_like(x)
    cost = torch.zeros(1, dtype=f64, device=dev)
    ccost = torch.zeros(1, dtype=f64, device=dev)
    r = torch.empty(m, dtype=f64, device=dev)
    g = torch.empty(n, dtype=f64, device=dev)
    jac = torch.empty(prog.num_jacobian_values, dtype=f64, device=dev)

    def timed(name, fn):
        torch.cuda.synchronize(dev)
        s = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        timers.add(name, time.perf_counter() - s)
        return out

    # The Schur solvers take g = J^T r from their own init (cse_schur_init_gradient,
    # every solve, before g is read); CGNR from the evaluation.
    grad_from_init = args.linear_solver != "cgnr"

    def jacobian_eval(new_point=True):
        # After an accepted step x holds the candidate just evaluated:
        # new_evaluation_point = false, as HandleSuccessfulStep passes
        # (trust_region_minimizer.cc:822-826).
        ev.evaluate_device(x.data_ptr(), cost.data_ptr(), r.data_ptr(),
                           None if grad_from_init else g.data_ptr(), jac.data_ptr(),
                           new_evaluation_point=new_point)
        return ev.wait()

    def normal_op(v, sqrt_lam_d):
        # (J^T J + lam D) v in one pass over J (cse_cgnr_multiply, the
        # CudaCgnrLinearOperator of cgnr_solver.cc:226-237).
        out = torch.zeros(n, dtype=f64, device=dev)
        ev.cgnr_multiply_device(jac.data_ptr(), sqrt_lam_d.data_ptr(), v.data_ptr(),
                                out.data_ptr())
        return out

    def cgnr(lam):
        # (J^T J + lam D) dx = -g by Jacobi-preconditioned CG on the normal
        # equations (cgnr_solver.cc), D = diag(J^T J).
        b = -g
        Minv = 1.0 / ((1.0 + lam) * D)
        sqrt_lam_d = torch.sqrt(lam * D)
        dx = torch.zeros(n, dtype=f64, device=dev)
        res = b.clone()
        z = Minv * res
        p = z.clone()
        rz = torch.dot(res, z)
        bn = b.norm()
        it = 0
        for it in range(1, args.max_linear_solver_iterations + 1):
            Ap = normal_op(p, sqrt_lam_d)
            alpha = rz / torch.dot(p, Ap)
            dx += alpha * p
            res -= alpha * Ap
            if res.norm() <= args.eta * bn:
                break
            z = Minv * res
            rz_new = torch.dot(res, z)
            p = z + (rz_new / rz) * p
            rz = rz_new
        return dx, it

    if args.device_cgnr:
        cgnr_pre = {"identity": ca._cse.CGNR_IDENTITY, "jacobi": ca._cse.CGNR_JACOBI}[args.cgnr_preconditioner]
        cgnr_rhs = torch.empty(n, dtype=f64, device=dev)
        cgnr_neg_r = torch.empty(m, dtype=f64, device=dev)
        cgnr_options = ca._cse.cg_options(r_tolerance=args.eta, q_tolerance=0.0,
                                          residual_reset_period=args.max_linear_solver_iterations + 1,
                                          max_num_iterations=args.max_linear_solver_iterations,
                                          check_period=args.cgnr_check_period,
                                          flags=ca._cse.CG_ZERO_INITIAL_GUESS)

    def cgnr_device(lam):
        # CudaCgnrSolver::SolveImpl (cgnr_solver.cc:350-387): Atb = J^T b and the
        # preconditioner (cse_cgnr_init), then ConjugateGradientsSolver from
        # x = 0 (cse_cgnr_solve), all on the device.
        torch.neg(r, out=cgnr_neg_r)
        sqrt_lam_d = torch.sqrt(lam * D)
        ev.cgnr_init_device(jac.data_ptr(), sqrt_lam_d.data_ptr(), cgnr_neg_r.data_ptr(),
                            cgnr_rhs.data_ptr(), cgnr_pre)
        dx = torch.empty(n, dtype=f64, device=dev)
        summary = ev.cgnr_solve_device(cgnr_rhs.data_ptr(), dx.data_ptr(), cgnr_options)
        if summary.termination_type == ca._cse.CG_FAILURE:
            raise SystemExit(f"device CGNR failed (reason {summary.reason})")
        # A block the JACOBI init could not factor was left zero and raised the
        # status word (that init clears it first); the next evaluation would
        # overwrite it unread.
        if cgnr_pre == ca._cse.CGNR_JACOBI and ev.wait() != 0:
            raise SystemExit("device CGNR: a block of J^T J + lambda D is not positive definite "
                             "(cse_cgnr_init raised the status word)")
        return dx, summary.num_iterations

    if args.linear_solver != "cgnr":
        e_cols, f_cols = ev.schur_structure()
        # cluster_jacobi: the init builds no preconditioner of its own (IDENTITY);
        # cse_schur_cluster_jacobi installs the cluster blocks after it.
        tridiagonal_pre = args.preconditioner == "cluster_tridiagonal"
        cluster_pre = args.preconditioner == "cluster_jacobi" or tridiagonal_pre
        pre = {"identity": ca._cse.SCHUR_IDENTITY, "jacobi": ca._cse.SCHUR_JACOBI,
               "schur_jacobi": ca._cse.SCHUR_SCHUR_JACOBI,
               "schur_power_series_expansion": ca._cse.SCHUR_POWER_SERIES_EXPANSION,
               "cluster_jacobi": ca._cse.SCHUR_IDENTITY,
               "cluster_tridiagonal": ca._cse.SCHUR_IDENTITY}[args.preconditioner]
        if cluster_pre:
            from ceres_amd import clustering
            t0 = time.perf_counter()
            labels = clustering.cluster_cameras(ci, pi, cams.shape[0], args.visibility_clustering,
                                                args.cluster_min_similarity, args.max_cluster_cameras)
            ev.schur_set_clusters(labels)
            sizes = np.bincount(labels)
            if tridiagonal_pre:
                # The cluster graph and its degree-2 maximum spanning forest
                # (visibility_based_preconditioner.cc:130-154).
                forest = clustering.degree2_maximum_spanning_forest(
                    len(sizes), *clustering.cluster_graph(ci, pi, labels), sizes=sizes)
                ev.schur_set_cluster_forest(forest)
                scaled_flag = torch.zeros(1, dtype=torch.int32, device=dev)
                scaled_solves = []
            timers.add("Visibility clustering", time.perf_counter() - t0)
            print(f"{args.preconditioner}: {len(sizes)} clusters of {sizes.min()} to {sizes.max()} cameras "
                  f"({args.visibility_clustering})")
            if tridiagonal_pre:
                paths = clustering.forest_paths(len(sizes), forest)
                print(f"cluster_tridiagonal: {len(forest)} forest edges, {len(paths)} paths, the longest of "
                      f"{max(len(p) for p in paths)} clusters")
            if stats is not None:
                stats["cluster_sizes"] = sizes
                if tridiagonal_pre:
                    stats["forest_edges"] = forest
                    stats["path_lengths"] = np.array([len(p) for p in paths])
                    stats["scaled_solves"] = scaled_solves
        if pre == ca._cse.SCHUR_POWER_SERIES_EXPANSION:
            ev.schur_set_spse_iterations(args.max_num_spse_iterations)
        rhs = torch.empty(f_cols, dtype=f64, device=dev)
        neg_r = torch.empty(m, dtype=f64, device=dev)
    if args.linear_solver == "dense_schur":
        _, _, plan_bytes = ev.schur_complement_plan()
        need = plan_bytes + 8 * f_cols * f_cols
        dense_precision = (ca._cse.DENSE_CHOLESKY_FP32 if args.mixed_precision_solves
                           else ca._cse.DENSE_CHOLESKY_FP64)
        if args.dense_linear_algebra_library == "cse":
            # The factorization's workspace: in FP32 mode the float copy of S.
            need += ca.Evaluator.dense_cholesky_workspace(f_cols, dense_precision)
        if need > args.max_schur_gb * 2 ** 30:
            raise SystemExit(f"dense_schur: the plan and the {f_cols} x {f_cols} S take "
                             f"{need / 2 ** 30:.2f} GiB, above --max_schur_gb {args.max_schur_gb:g}; "
                             "use iterative_schur")
        S = torch.empty((f_cols, f_cols), dtype=f64, device=dev)
    if args.linear_solver == "sparse_schur":
        # SparseSchurComplementSolver: InitStorage's block structure, then the
        # SparseCholesky's symbolic analysis, both once per run
        # (sparse_cholesky.h:55-56).
        _, _, plan_bytes = ev.schur_complement_plan()
        t0 = time.perf_counter()
        s_row_begin, s_block_col, structure_bytes = ev.schur_complement_sparse_structure()
        timers.add("Schur complement structure", time.perf_counter() - t0)
        t0 = time.perf_counter()
        sparse_summary = ev.sparse_cholesky_analyze(
            s_row_begin, s_block_col,
            {"minimum_degree": ca._cse.SPARSE_ORDERING_MINIMUM_DEGREE,
             "natural": ca._cse.SPARSE_ORDERING_NATURAL}[args.sparse_ordering])
        timers.add("Sparse Cholesky analysis", time.perf_counter() - t0)
        print(f"sparse_schur: {sparse_summary.num_input_blocks} blocks of S, {sparse_summary.num_factor_blocks} "
              f"of L ({args.sparse_ordering}), {sparse_summary.num_block_products} block products, "
              f"{sparse_summary.num_levels} levels of at most {sparse_summary.max_level_columns} columns")
        if stats is not None:
            stats["sparse_cholesky"] = sparse_summary
        need = structure_bytes + plan_bytes + 648 * len(s_block_col) + sparse_summary.device_bytes
        if need > args.max_schur_gb * 2 ** 30:
            raise SystemExit(f"sparse_schur: the plan, the blocks of S and its factor take "
                             f"{need / 2 ** 30:.2f} GiB, above --max_schur_gb {args.max_schur_gb:g}; "
                             "use iterative_schur")
        S_values = torch.empty(81 * len(s_block_col), dtype=f64, device=dev)
    if args.use_explicit_schur_complement:
        _, _, plan_bytes = ev.schur_complement_plan()
        _, num_blocks, structure_bytes = ev.schur_complement_sparse_counts()
        need = structure_bytes + plan_bytes + 648 * num_blocks
        if need > args.max_schur_gb * 2 ** 30:
            raise SystemExit(f"use_explicit_schur_complement: the plan, the structure and the {num_blocks} "
                             f"blocks of S take {need / 2 ** 30:.2f} GiB, above --max_schur_gb "
                             f"{args.max_schur_gb:g}; use iterative_schur without the flag")
        S_values = torch.empty(81 * num_blocks, dtype=f64, device=dev)
        # SparseSchurComplementSolver::InitStorage: the co-visibility plan and
        # the block structure, built on the host and uploaded once.
        t0 = time.perf_counter()
        ev.schur_complement_sparse_upload()
        timers.add("Schur complement structure", time.perf_counter() - t0)

        def schur_op(d_x, d_y):
            ev.schur_explicit_multiply_device(S_values.data_ptr(), d_x, d_y)
    elif args.linear_solver == "iterative_schur":
        schur_op = ev.schur_multiply_device
    if args.device_pcg:
        xf_device = torch.empty(f_cols, dtype=f64, device=dev)
        max_it = args.max_linear_solver_iterations
        if args.pcg_termination == "quadratic":
            cg_options = ca._cse.cg_options(q_tolerance=args.eta, r_tolerance=-1.0)
        else:  # the host loop's test: no residual reset, no quadratic test
            cg_options = ca._cse.cg_options(r_tolerance=args.eta, q_tolerance=0.0,
                                            residual_reset_period=max_it + 1)
        cg_options.max_num_iterations = max_it
        cg_options.check_period = args.pcg_check_period
        # use_spse_initialization: the PCG starts from the series' x0.
        cg_options.flags = 0 if args.use_spse_initialization else ca._cse.CG_ZERO_INITIAL_GUESS

    def check_cluster_factor():
        # A cluster whose factor met a pivot that is not positive was left
        # adding zeros and raised the status word (the init clears it first);
        # the next evaluation would overwrite it unread.
        if cluster_pre and ev.wait() != 0:
            raise SystemExit(f"{args.preconditioner}: a cluster block of S is not positive definite "
                             f"(cse_schur_{args.preconditioner} raised the status word)")
        if tridiagonal_pre:
            # Whether this solve's factor ran again with the edges halved.
            scaled_solves.append(int(scaled_flag.item()))
            if scaled_solves[-1]:
                print(f"cluster_tridiagonal: linear solve {len(scaled_solves)} was scaled "
                      "(M was not positive definite; every edge block halved)")

    def schur_solve(lam):
        # IterativeSchurComplementSolver (iterative_schur_complement_solver.cc:
        # 63-170): the augmented system [J; sqrt(lam diag(J^T J))] dx = [-r; 0]
        # reduced to S dx_f = rhs, PCG on S, then back substitution.
        torch.neg(r, out=neg_r)
        sqrt_lam_d = torch.sqrt(lam * D)
        ev.schur_init_gradient_device(jac.data_ptr(), sqrt_lam_d.data_ptr(), neg_r.data_ptr(),
                                      rhs.data_ptr(), g.data_ptr(), pre)
        if args.use_explicit_schur_complement:
            # SolveReducedLinearSystemUsingConjugateGradients
            # (schur_complement_solver.cc): S once, then the PCG on its blocks.
            ev.schur_complement_sparse_device(S_values.data_ptr())
        if tridiagonal_pre:
            # Preconditioner::Update: M of this S, factored along the paths.
            ev.schur_cluster_tridiagonal_device(None, scaled_flag.data_ptr())
        elif cluster_pre:
            # Preconditioner::Update: the cluster blocks of this S, factored.
            ev.schur_cluster_jacobi_device()
        if args.device_pcg:
            # ConjugateGradientsSolver and BackSubstitute in one call; the zero
            # start as IterativeSchurComplementSolver's.
            dx = torch.empty(n, dtype=f64, device=dev)
            if args.use_spse_initialization:
                ev.schur_power_series_device(rhs.data_ptr(), xf_device.data_ptr(),
                                             args.max_num_spse_iterations, args.spse_tolerance)
            summary = ev.schur_solve_device(
                rhs.data_ptr(), xf_device.data_ptr(), cg_options,
                S_values.data_ptr() if args.use_explicit_schur_complement else None, dx.data_ptr())
            if summary.termination_type == ca._cse.CG_FAILURE:
                raise SystemExit(f"device PCG failed (reason {summary.reason})")
            check_cluster_factor()
            return dx, summary.num_iterations
        if args.use_spse_initialization:
            # x0 = the series of S^-1 on rhs (iterative_schur_complement_solver.cc:
            # 108-118), r = rhs - S x0.
            xf = torch.empty(f_cols, dtype=f64, device=dev)
            ev.schur_power_series_device(rhs.data_ptr(), xf.data_ptr(),
                                         args.max_num_spse_iterations, args.spse_tolerance)
            res = torch.empty_like(xf)
            schur_op(xf.data_ptr(), res.data_ptr())
            res = rhs - res
        else:
            xf = torch.zeros(f_cols, dtype=f64, device=dev)
            res = rhs.clone()
        z = torch.zeros_like(res)
        ev.schur_precondition_device(res.data_ptr(), z.data_ptr())
        p = z.clone()
        Ap = torch.empty_like(p)
        rz = torch.dot(res, z)
        bn = rhs.norm()
        it = 0
        for it in range(1, args.max_linear_solver_iterations + 1):
            schur_op(p.data_ptr(), Ap.data_ptr())
            alpha = rz / torch.dot(p, Ap)
            xf += alpha * p
            res -= alpha * Ap
            if res.norm() <= args.eta * bn:
                break
            z.zero_()
            ev.schur_precondition_device(res.data_ptr(), z.data_ptr())
            rz_new = torch.dot(res, z)
            p = z + (rz_new / rz) * p
            rz = rz_new
        dx = torch.empty(n, dtype=f64, device=dev)
        ev.schur_back_substitute_device(xf.data_ptr(), dx.data_ptr())
        check_cluster_factor()
        return dx, it

    def cse_cholesky_solve():
        # DenseCholesky::FactorAndSolve on the device: S stays where
        # cse_schur_complement wrote it, the step comes back in a device buffer.
        ev.dense_cholesky_factorize_device(S.data_ptr(), f_cols, precision=dense_precision)
        xf = torch.empty(f_cols, dtype=f64, device=dev)
        ev.dense_cholesky_solve_device(rhs.data_ptr(), xf.data_ptr(), args.max_num_refinement_iterations)
        info = ev.dense_cholesky_info()
        if info != 0:
            raise SystemExit(f"dense_schur: S is not positive definite (leading minor {info})")
        return xf

    def dense_schur_solve(lam):
        # DenseSchurComplementSolver (schur_complement_solver.cc): the same
        # augmented system reduced to the dense S by SchurEliminator::Eliminate
        # (cse_schur_complement), S dx_f = rhs by Cholesky, back substitution.
        torch.neg(r, out=neg_r)
        sqrt_lam_d = torch.sqrt(lam * D)
        ev.schur_init_gradient_device(jac.data_ptr(), sqrt_lam_d.data_ptr(), neg_r.data_ptr(),
                                      rhs.data_ptr(), g.data_ptr(), ca._cse.SCHUR_IDENTITY)
        ev.schur_complement_device(S.data_ptr())
        if args.dense_linear_algebra_library == "cse":
            xf = timed("Dense Cholesky factor & solve", cse_cholesky_solve)
        else:
            xf = cholesky_solve(S, rhs)
        dx = torch.empty(n, dtype=f64, device=dev)
        ev.schur_back_substitute_device(xf.data_ptr(), dx.data_ptr())
        return dx, 0

    def sparse_cholesky_solve():
        # SparseCholesky::FactorAndSolve on the device: the blocks stay where
        # cse_schur_complement_sparse wrote them, the step comes back in a
        # device buffer.
        ev.sparse_cholesky_factorize_device(S_values.data_ptr())
        xf = torch.empty(f_cols, dtype=f64, device=dev)
        ev.sparse_cholesky_solve_device(rhs.data_ptr(), xf.data_ptr(), args.max_num_refinement_iterations)
        return xf, ev.sparse_cholesky_info()

    def sparse_schur_solve(lam):
        # SparseSchurComplementSolver (schur_complement_solver.cc:290-333): the
        # same augmented system reduced to the block-sparse S, S dx_f = rhs by
        # the block-sparse Cholesky factorization, back substitution; one
        # "iteration" (:329).
        torch.neg(r, out=neg_r)
        sqrt_lam_d = torch.sqrt(lam * D)
        ev.schur_init_gradient_device(jac.data_ptr(), sqrt_lam_d.data_ptr(), neg_r.data_ptr(),
                                      rhs.data_ptr(), g.data_ptr(), ca._cse.SCHUR_IDENTITY)
        ev.schur_complement_sparse_device(S_values.data_ptr())
        xf, info = timed("Sparse Cholesky factor & solve", sparse_cholesky_solve)
        if info != 0:
            # LinearSolverTerminationType::FAILURE (schur_complement_solver.cc:
            # 316-321): no step; the zero step is rejected and the radius shrinks.
            print(f"sparse_schur: S is not positive definite (permuted scalar column {info - 1}); "
                  "the step is rejected")
            return torch.zeros(n, dtype=f64, device=dev), 1
        dx = torch.empty(n, dtype=f64, device=dev)
        ev.schur_back_substitute_device(xf.data_ptr(), dx.data_ptr())
        return dx, 1

    # Solver::Options::jacobi_scaling (trust_region_minimizer.cc:259-275): the
    # scaling comes from the first Jacobian and every Jacobian is scaled in
    # place; the solvers, the LM diagonal and the model then live in the scaled
    # space (g holds the scaled gradient J_s^T r = scaling .* J^T r).
    scaling = None

    def scale_jacobian():
        nonlocal scaling
        if scaling is None:
            scaling = torch.empty(n, dtype=f64, device=dev)
            ev.squared_column_norm_device(jac.data_ptr(), scaling.data_ptr())
            scaling = 1.0 / (1.0 + torch.sqrt(scaling))
            if stats is not None:
                stats["jacobi_scaling"] = (float(scaling.min().item()), float(scaling.max().item()))
        ev.scale_columns_device(jac.data_ptr(), scaling.data_ptr())
        if not grad_from_init:
            g.mul_(scaling)

    status = timed("Jacobian & residual evaluation", jacobian_eval)
    if status != 0:
        raise SystemExit("initial evaluation failed")
    if args.jacobi_scaling:
        timed("Jacobi scaling", scale_jacobian)
    initial_cost = float(cost.item())
    radius = args.initial_trust_region_radius
    # LevenbergMarquardtStrategy (levenberg_marquardt_strategy.cc:157-170):
    # a rejected step divides the radius by decrease_factor and doubles it;
    # an accepted one resets it to 2.
    decrease_factor = 2.0
    max_radius = 1e16  # Solver::Options::max_trust_region_radius
    min_relative_decrease = 1e-3  # Solver::Options::min_relative_decrease
    rows = []
    D = torch.zeros(n, dtype=f64, device=dev)
    ones = torch.ones(m, dtype=f64, device=dev)
    jac2 = None  # squared Jacobian values, one buffer for the whole solve
    d_stale = True  # D follows J: recomputed after the initial and each accepted evaluation
    for it in range(args.num_iterations):
        # Jacobi scaling: diag(J^T J) = column sums of squared values, one
        # left-multiply of the squared Jacobian with a vector of ones.
        if d_stale and args.jacobi_scaling:
            # LevenbergMarquardtStrategy::ComputeStep (levenberg_marquardt_strategy.cc:
            # 78-94): the squared column norms of the (scaled) Jacobian, clamped to
            # [min_lm_diagonal, max_lm_diagonal].
            timed("LM diagonal", lambda: ev.squared_column_norm_device(jac.data_ptr(), D.data_ptr()))
            if stats is not None:
                stats.setdefault("lm_diagonal", []).append((float(D.min().item()), float(D.max().item())))
            D.clamp_(min=1e-6, max=1e32)
            d_stale = False
        elif d_stale:
            if jac2 is None:
                jac2 = torch.empty_like(jac)
            torch.mul(jac, jac, out=jac2)
            D.zero_()
            ev.left_multiply_device(jac2.data_ptr(), ones.data_ptr(), D.data_ptr())
            if stats is not None:
                stats.setdefault("lm_diagonal", []).append((float(D.min().item()), float(D.max().item())))
            D.clamp_(min=1e-6)
            d_stale = False
        solver = {"iterative_schur": schur_solve, "dense_schur": dense_schur_solve,
                  "sparse_schur": sparse_schur_solve,
                  "cgnr": cgnr_device if args.device_cgnr else cgnr}[args.linear_solver]
        dx, cg_iters = timed("Linear solver", lambda: solver(1.0 / radius))
        # dx is the step of the (scaled) linear system; Plus takes delta =
        # step .* scaling (trust_region_minimizer.cc:443-446).
        delta = dx * scaling if args.jacobi_scaling else dx
        timed("Plus", lambda: ev.plus_device(x.data_ptr(), delta.data_ptr(), cand.data_ptr()))

        def cand_eval():
            ev.evaluate_device(cand.data_ptr(), ccost.data_ptr(), None, None, None)
            return ev.wait()

        ok = timed("Residual only evaluation", cand_eval) == 0
        new_cost = float(ccost.item()) if ok else float("inf")
        old_cost = float(cost.item())
        # model decrease of the linearised problem: -(g.dx + 0.5 |J dx|^2)
        Jdx = torch.zeros(m, dtype=f64, device=dev)
        ev.right_multiply_device(jac.data_ptr(), dx.data_ptr(), Jdx.data_ptr())
        model = float(-(torch.dot(g, dx) + 0.5 * torch.dot(Jdx, Jdx)).item())
        rho = (old_cost - new_cost) / model if model > 0 else -1.0
        # TrustRegionMinimizer::IsStepSuccessful: relative decrease above
        # min_relative_decrease (trust_region_minimizer.cc).
        accepted = ok and rho > min_relative_decrease
        # The table shows the unscaled gradient and the step Plus took.
        gnorm = float((g / scaling).norm().item()) if args.jacobi_scaling else float(g.norm().item())
        rows.append((it, old_cost, new_cost, gnorm, float(delta.norm().item()),
                     radius, cg_iters, accepted))
        if accepted:
            x.copy_(cand)
            if timed("Jacobian & residual evaluation", lambda: jacobian_eval(False)) != 0:
                raise SystemExit(f"iteration {it}: Jacobian evaluation at the accepted point failed")
            if args.jacobi_scaling:
                timed("Jacobi scaling", scale_jacobian)
            d_stale = True
            radius = min(max_radius, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease_factor = 2.0
        else:
            radius = radius / decrease_factor
            decrease_factor *= 2.0
    del jac2
    ev.close()
    print("iter      cost      cost_new   |gradient|    |step|    tr_radius  ls_iter  accepted")
    for it, c0, c1, gn, sn, rad, li, acc in rows:
        print(f"{it:4d} {c0:12.6e} {c1:12.6e} {gn:10.3e} {sn:10.3e} {rad:10.3e} {li:6d}   {acc}")
    print(f"\nInitial cost {initial_cost:.6e}  Final cost {float(cost.item()):.6e}")
    if args.preconditioner == "cluster_tridiagonal":
        print(f"cluster_tridiagonal: {sum(scaled_solves)} of {len(scaled_solves)} linear solves were scaled")
    print(timers.report())
    return initial_cost, float(cost.item()), rows


def main(argv=None, stats=None):
    return solve(parse(argv), stats)


if __name__ == "__main__":
    main()
