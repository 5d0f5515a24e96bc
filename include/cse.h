/*
 * cse.h -- C ABI of the MI355X (gfx950) residual/Jacobian evaluator.
 *
 * "cse" = Ceres Solver Evaluator.  This is the drop-in boundary for the hot
 * path of jwmak/ceres-solver-cuda: the per-residual-block autodiff evaluator
 * behind ProblemCUDA.  Every entry point names the reference interface it
 * replaces (paths relative to the reference checkout).
 *
 * Plain C: no exceptions cross the boundary, no torch/HIP types in the
 * signatures (streams are passed as void*), every buffer is a pointer plus
 * a size.  All functions return 0 on success, a positive status for a
 * numerical failure (a residual block reported failure) and a negative
 * status for a usage or HIP error; cse_last_error() then describes it.
 *
 * Threading: an evaluator is not thread-safe (the reference's
 * RegisteredCUDAEvaluators is not either).  Distinct evaluators may be used
 * from distinct threads.
 */
#ifndef CSE_H_
#define CSE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: cse_parameter_block.manifold (was `reserved`, which had to be 0),
 *    cse_host_register / cse_host_unregister, cse_shard_transfer_bytes,
 *    shard-local state in cse_create_multi.
 * 3: cse_options.jacobian_form.
 * 4: user functor kinds (cse_register_functor, cse_functor_shape),
 *    CSE_LOSS_USER and cse_loss.user, cse_schur_init_gradient.
 * 5: cse_functor_ops.fused_points / camera_gradient (the fused gradient for
 *    user kinds) and camera_gradient_args_size (was reserved[0]).
 * 6: cse_residual_group.loss_data_size (was `reserved`, 0 in every
 *    descriptor): per-block loss parameters in the functor_data rows. */
#define CSE_ABI_VERSION 6

/* Return codes. */
#define CSE_OK 0
#define CSE_EVALUATION_FAILED 1 /* a functor returned false / non-finite output */
#define CSE_ERR_INVALID -1      /* malformed descriptor or arguments */
#define CSE_ERR_HIP -2          /* HIP runtime error */
#define CSE_ERR_OOM -3          /* device allocation failed */
#define CSE_ERR_UNSUPPORTED -4  /* functor/loss/layout not available */

/* Residual functors pre-instantiated in the library.  The reference
 * compiles user functors header-only into the user's nvcc TU
 * (include/ceres/problem_cuda.h:110-160); across a C ABI the functor is a
 * kind plus per-block constants ("functor data").
 *   kind                                  kR  blocks  data
 *   SNAVELY_2_9_3                          2  9,3     obs_x, obs_y
 *       examples/snavely_reprojection_error.h:54-105
 *   SNAVELY_NO_DISTORTION_2_7_3            2  7,3     obs_x, obs_y
 *       internal/ceres/evaluator_cuda_test.cu.cc:112-150
 *   SNAVELY_QUATERNION_2_10_3              2  10,3    obs_x, obs_y
 *       examples/snavely_reprojection_error.h:112-175
 *   POINT_DISPLACEMENT_3_3                 3  3       x, y, z
 *       internal/ceres/evaluator_cuda_test.cu.cc:84-110
 */
typedef enum cse_functor_kind {
  CSE_FUNCTOR_SNAVELY_2_9_3 = 0,
  CSE_FUNCTOR_SNAVELY_NO_DISTORTION_2_7_3 = 1,
  CSE_FUNCTOR_SNAVELY_QUATERNION_2_10_3 = 2,
  CSE_FUNCTOR_POINT_DISPLACEMENT_3_3 = 3,
  /* The functors of the reference's own known-answer tests, so that those
   * tests run through the library's kernels (general path, trivial loss
   * only).  kind                      kR  blocks      data
   *   TEST_LINEAR_<kR>_<sizes>           see name    kFactor, succeeds
   *       ParameterIgnoringCostFunction, internal/ceres/evaluator_test.cc:58-100,
   *       as r_i = (i+1) + kFactor sum_b sum_j (j+1) x_b[j] (exact at x = 0)
   *   TEST_BILINEAR_1_2_2             1   2,2         a
   *       BinaryScalarCost, autodiff_cost_function_cuda_test.cu.cc:40-51
   *   TEST_TEN_PARAMETER_1_x10        1   1 (x10)     unused
   *       TenParameterCost, autodiff_cost_function_cuda_test.cu.cc:123-139
   *   TEST_PARTIAL_OUTPUT_2_1         2   1           unused
   *       OnlyFillsOneOutputFunctor, autodiff_cost_function_cuda_test.cu.cc:224-230 */
  CSE_FUNCTOR_TEST_LINEAR_3_2_3_4 = 100,
  CSE_FUNCTOR_TEST_LINEAR_3_4_3_2 = 101,
  CSE_FUNCTOR_TEST_LINEAR_2_2_3 = 102,
  CSE_FUNCTOR_TEST_LINEAR_3_2_4 = 103,
  CSE_FUNCTOR_TEST_LINEAR_4_3_4 = 104,
  CSE_FUNCTOR_TEST_BILINEAR_1_2_2 = 110,
  CSE_FUNCTOR_TEST_TEN_PARAMETER_1_x10 = 111,
  CSE_FUNCTOR_TEST_PARTIAL_OUTPUT_2_1 = 112
} cse_functor_kind;

/* LossFunctionCUDA variants, include/ceres/loss_function_cuda.h:62-150. */
typedef enum cse_loss_kind {
  CSE_LOSS_TRIVIAL = 0, /* TrivialLossCUDA (or nullptr, problem_cuda.h:146-160) */
  CSE_LOSS_HUBER = 1,   /* HuberLossCUDA(a) */
  CSE_LOSS_CAUCHY = 2,  /* CauchyLossCUDA(a) */
  /* A user LossFunctionCUDA type (a class with
   *   __host__ __device__ void Evaluate(double s, double rho[3]) const,
   * the contract of loss_function_cuda.h:62-94), compiled into a user functor
   * kind's kernels (cse_functor_ops.loss_kind); the group's object is passed
   * as bytes in cse_loss.user.  Only with such a kind. */
  CSE_LOSS_USER = 3
} cse_loss_kind;

#define CSE_USER_LOSS_BYTES 64

typedef struct cse_loss {
  int32_t kind;   /* cse_loss_kind */
  int32_t scaled; /* 1 = wrapped in ScaledLossCUDA(rho, scale) */
  double a;       /* loss parameter a */
  double scale;   /* ScaledLossCUDA factor */
  /* CSE_LOSS_USER: the loss object's bytes (trivially copyable, at most
   * CSE_USER_LOSS_BYTES), handed to the kernels as they are. */
  double user[CSE_USER_LOSS_BYTES / 8];
} cse_loss;

/* One parameter block of the reduced Program; replaces ParameterBlockCUDA
 * (include/ceres/internal/parameter_block_cuda.h:106-116) as filled by
 * RegisteredCUDAEvaluators::SetupParameterBlocks
 * (internal/ceres/registered_cuda_evaluators.cc:123-198). */
typedef struct cse_parameter_block {
  int32_t size;                 /* ambient size */
  int32_t tangent_size;         /* == size without a manifold */
  int32_t is_constant;          /* held constant: no Jacobian, no gradient */
  int32_t manifold;             /* cse_manifold_kind (ABI 1: `reserved`, 0) */
  int64_t state_offset;         /* into state (active) / constant_state (constant) */
  int64_t delta_offset;         /* into the gradient (active only) */
  int64_t plus_jacobian_offset; /* into plus_jacobians (size x tangent row-major), -1 = none */
} cse_parameter_block;

/* How the evaluator gets a block's plus-Jacobian (Manifold::PlusJacobian).
 *   CSE_MANIFOLD_MATRIX: the size x tangent_size matrix at
 *       plus_jacobian_offset, refreshed by cse_set_plus_jacobians, as the
 *       reference uploads it (registered_cuda_evaluators.cc:139-160);
 *       plus_jacobian_offset -1 = no manifold.
 *   CSE_MANIFOLD_QUATERNION_EUCLIDEAN: ProductManifold<QuaternionManifold,
 *       EuclideanManifold<size - 4>> (Ceres order w, x, y, z first; the
 *       --use_quaternions --use_manifolds camera of examples/bundle_adjuster.cc:
 *       337-345 and evaluator_cuda_test.cu.cc:286): tangent_size = size - 1,
 *       plus_jacobian_offset must be -1.  The kernels build the plus-Jacobian
 *       (QuaternionPlusJacobianImpl, internal/ceres/manifold.cc:62-78, and an
 *       identity block) from the block's current value in registers; the
 *       result equals the dense product with that matrix.  Blocks of this kind
 *       in slot 0 of SNAVELY_QUATERNION_2_10_3 groups keep the affine (fast)
 *       kernels; cse_plus applies QuaternionPlusImpl (manifold.cc:28-59) to
 *       them and x + delta to the Euclidean part. */
typedef enum cse_manifold_kind {
  CSE_MANIFOLD_MATRIX = 0,
  CSE_MANIFOLD_QUATERNION_EUCLIDEAN = 1
} cse_manifold_kind;

/* All residual blocks of one (functor kind, loss) type; replaces one
 * AutoDiffResidualBlockCUDAEvaluator<F, Loss, kR, Ns...> and its residual
 * blocks (include/ceres/internal/autodiff_residual_block_cuda_evaluator.h:62-334,
 * registered per std::type_index in problem_cuda.h:462-468).
 *
 * The loss *type* (loss.kind, loss.scaled) is uniform over the group.  Its
 * parameters are either uniform too (loss_data_size 0: loss.a and loss.scale
 * hold for every block) or per block (loss_data_size 2), as the reference
 * keeps one loss object per residual block
 * (autodiff_residual_block_cuda_evaluator.h:100-132): every functor_data row
 * then ends with the block's own (a, scale) -- per-observation weights
 * (ScaledLossCUDA(rho, w_i)) or per-block Huber/Cauchy widths in one group,
 * one launch, with the fused gradient and the Schur operators a single group
 * gets.  Per-block parameters are for the library's Huber, Cauchy and
 * (scaled) trivial losses on the library's functor kinds with
 * cse_options.jacobian_form = CSE_JACOBIAN_CLOSED_FORM; cse_create refuses
 * them (CSE_ERR_UNSUPPORTED) with CSE_LOSS_USER, with user functor kinds
 * (>= CSE_FUNCTOR_USER_FIRST: their launch tables are fixed-size and have no
 * per-block slots, and a user loss object per block has no place in a row;
 * such groups are still split by loss value), with the TEST_* kinds and with
 * CSE_JACOBIAN_JET, and (CSE_ERR_INVALID) the unscaled trivial loss, where
 * nothing varies. */
typedef struct cse_residual_group {
  int32_t functor_kind;               /* cse_functor_kind */
  /* Trailing loss doubles of each functor_data row: 0 = none (the loss
   * parameters are loss.a, loss.scale), 2 = the block's (a, scale); loss.a
   * and loss.scale are then ignored, and the scale column too when
   * loss.scaled == 0.  Any other value: CSE_ERR_INVALID.  (ABI <= 5:
   * `reserved`, 0.) */
  int32_t loss_data_size;
  cse_loss loss;
  int64_t num_blocks;
  /* Global residual block index (program order, ResidualBlock::index())
   * of block i; NULL means first_residual_block + i. */
  const int64_t* residual_block_index;
  int64_t first_residual_block;
  /* [num_blocks][num parameter blocks of the kind], program indices. */
  const int32_t* parameter_block_ids;
  /* [num_blocks][data size of the kind + loss_data_size]: the functor
   * constants, then the block's loss parameters. */
  const double* functor_data;
} cse_residual_group;

/* The reduced Program plus the Jacobian layout the evaluator writes into:
 * the arguments of RegisteredCUDAEvaluators::Init
 * (internal/ceres/registered_cuda_evaluators.cc:226-280), with int64 offsets
 * (the reference's int32 overflows past ~89M observations). */
typedef struct cse_problem_desc {
  int32_t abi_version; /* CSE_ABI_VERSION */
  int32_t num_groups;
  const cse_residual_group* groups;

  int64_t num_parameter_blocks;
  const cse_parameter_block* parameter_blocks;
  int64_t num_parameters;           /* Program::NumParameters (state size) */
  int64_t num_effective_parameters; /* Program::NumEffectiveParameters */
  int64_t num_constant_parameters;  /* Program::NumConstantParameters */
  const double* constant_state;     /* host, copied once (registered_cuda_evaluators.cc:237-248) */
  int64_t num_plus_jacobian_values;
  const double* plus_jacobians;     /* host; refresh with cse_set_plus_jacobians */

  int64_t num_residual_blocks;
  int64_t num_residuals;
  /* ProgramEvaluatorCUDA::BuildResidualLayout (program_evaluator_cuda.h:159-170). */
  const int64_t* residual_layout;
  /* {BlockJacobianWriter,CompressedRowJacobianWriter}::CreateJacobianPerResidualLayout
   * (block_jacobian_writer.cc:154-160, compressed_row_jacobian_writer.cc:240-300). */
  const int64_t* jacobian_per_residual_layout;
  const int64_t* jacobian_per_residual_offsets;
  int64_t num_jacobian_per_residual_offsets;
  int64_t num_jacobian_values; /* SparseMatrix::num_nonzeros() */
} cse_problem_desc;

typedef struct cse_options {
  int32_t device;               /* HIP device ordinal; -1 = current device */
  int32_t check_finite;         /* reject non-finite r/J (residual_block.cc:110-129) */
  int32_t apply_loss_function;  /* Evaluator::EvaluateOptions::apply_loss_function */
  int32_t force_general_layout; /* never take the affine fast path (testing) */
  int32_t profile;              /* time every evaluate kernel with HIP events */
  int32_t use_stream;           /* 1: run on `stream` as given, even NULL (the null stream) */
  void* stream;                 /* hipStream_t to run on; NULL and use_stream 0 =
                                   an evaluator-owned stream */
  int32_t gradient_mode;        /* how g = J^T r is summed when the residuals and
                                   Jacobian are requested too: 0 (default) = fused
                                   where eligible (slot-1 rows in the evaluation,
                                   slot-0 rows by re-evaluation in slot-0 order),
                                   else 1; 1 = a fixed-order post-pass over the
                                   written Jacobian; 2 = in-kernel FP64 atomics,
                                   as cuda_evaluator_kernel.h:149-160; 3 = fused,
                                   slot-0 contributions written in block order and
                                   summed per block (the round-2 form), else 1.
                                   0, 1 and 3 are bit-deterministic.  With
                                   jacobian_form CSE_JACOBIAN_JET, and for user
                                   kinds, 3 runs as 1. */
  int32_t jacobian_form;        /* cse_jacobian_form: how the SnavelyReprojectionError
                                   Jacobian is differentiated (every other kind always
                                   uses Jet<double, N>, AutoDifferentiate) */
} cse_options;

/* cse_options.jacobian_form.  Both give the Jacobian of the same functor to
 * within the parity bounds; the closed form is faster (fewer FP64 operations,
 * fewer registers). */
typedef enum cse_jacobian_form {
  /* Snavely<2,9,3>: the forward-mode product rule written out once in closed
   * form (SnavelyJacobianByHand); the default. */
  CSE_JACOBIAN_CLOSED_FORM = 0,
  /* Forward-mode dual numbers Jet<double, 12> seeded per parameter, as
   * AutoDiffCostFunction / AutoDifferentiate (autodiff.h:314-381,
   * autodiff_cost_function_cuda.h:55-71). */
  CSE_JACOBIAN_JET = 1
} cse_jacobian_form;

typedef struct cse_evaluator cse_evaluator;

/* Fills *options with the defaults: device -1, check_finite 1,
 * apply_loss_function 1, everything else 0 (an evaluator-owned stream). */
void cse_default_options(cse_options* options);

/* Replaces RegisteredCUDAEvaluators::Init + each
 * AutoDiffResidualBlockCUDAEvaluator::Init (uploads topology, layouts and
 * constants once).  The descriptor's host arrays are copied; they may be
 * freed after the call. */
int cse_create(const cse_problem_desc* desc, const cse_options* options,
               cse_evaluator** out);

/* Replaces RegisteredCUDAEvaluators::Evaluate
 * (include/ceres/internal/registered_cuda_evaluators.h:75-79): host
 * pointers, any output except cost may be NULL, synchronous.  Returns
 * CSE_OK, CSE_EVALUATION_FAILED (Evaluate returning false) or an error. */
int cse_evaluate(cse_evaluator* ev, const double* state, double* cost,
                 double* residuals, double* gradient, double* jacobian_values);

/* Device-resident variant (no host copies; the roofline path): all pointers
 * are device pointers on the evaluator's device, d_cost is one double.
 * Asynchronous on the evaluator's stream; call cse_wait for the status. */
int cse_evaluate_device(cse_evaluator* ev, const double* d_state, double* d_cost,
                        double* d_residuals, double* d_gradient,
                        double* d_jacobian_values);

/* Evaluate flags.  CSE_EVAL_SAME_POINT carries
 * Evaluator::EvaluateOptions::new_evaluation_point == false
 * (internal/ceres/evaluator.h:106-107): the state has the same values as at
 * the previous evaluation on this evaluator, as when TrustRegionMinimizer
 * evaluates the Jacobian at a just-accepted candidate
 * (trust_region_minimizer.cc:822-826).  The library then reuses what it
 * derived from the state last time: the state already copied to the device
 * (cse_evaluate_ex, the multi-device evaluator) and the repacked slot-0
 * table of the affine kernels.  The state pointer may differ; its values
 * must not.  Ignored when there is no previous evaluation to reuse. */
#define CSE_EVAL_SAME_POINT 1u

/* cse_evaluate / cse_evaluate_device with flags (0 = the plain call). */
int cse_evaluate_ex(cse_evaluator* ev, const double* state, double* cost,
                    double* residuals, double* gradient, double* jacobian_values,
                    uint32_t flags);
int cse_evaluate_device_ex(cse_evaluator* ev, const double* d_state, double* d_cost,
                           double* d_residuals, double* d_gradient,
                           double* d_jacobian_values, uint32_t flags);

/* ---- User functor kinds -------------------------------------------------
 * The reference evaluates any AutoDiffCostFunction functor: the user's nvcc
 * TU instantiates EvaluateKernel<CostFunctor, LossFunctionCUDA, kR, Ns...>
 * and ProblemCUDA::AddResidualBlock registers one
 * AutoDiffResidualBlockCUDAEvaluator per such type
 * (include/ceres/problem_cuda.h:423-474, README.md:19-33).  Here the user's
 * hipcc TU instantiates this library's kernels for its functor
 * (include/ceres_amd/autodiff_cuda.h, header-only: RegisterAutoDiffFunctor
 * or ProblemCUDA::AddResidualBlock) and registers them as a table of launch
 * functions; the kind returned is then used in cse_residual_group.
 * functor_kind like a built-in one.  Kinds are process-wide and stay
 * registered until the library is unloaded.
 *
 * The launch functions receive the library's kernel argument blocks, whose
 * layout both sides take from the same headers (ceres-solver-cuda_amd/csrc/
 * kernel_common.hpp, operator_kernels.hpp); kernel_args_size, gradient_args_size
 * and kernel_args_tag must equal the library's or registration fails. */
#define CSE_FUNCTOR_USER_FIRST 1000
#define CSE_MAX_PARAMETER_BLOCKS 10

/* Evaluation: kernel_args -> the group's arguments, stream = hipStream_t. */
typedef void (*cse_kernel_launch_fn)(const void* kernel_args, int64_t num_workgroups, void* stream);
/* which: 0 = y += J x on the affine layout, 1 = y += J x (general),
 * 2 = y += J^T x (general). */
typedef void (*cse_multiply_launch_fn)(const void* kernel_args, int32_t which, const double* x,
                                       double* y, void* stream);
/* The gradient post-pass of one slot; form 0 = identity order, 1 = chunked,
 * 2 = one lane per parameter block. */
typedef void (*cse_gradient_launch_fn)(const void* gradient_args, const void* chunks, int32_t form,
                                       void* stream);
/* The fused gradient's slot-0 rows: one wave per chunk of a slot-0 block's
 * residual blocks, re-evaluated in slot-0 order (camera_gradient_args ->
 * the library's CamGradArgs); num_slots = waves to launch. */
typedef void (*cse_camera_gradient_launch_fn)(const void* camera_gradient_args, int64_t num_slots,
                                              void* stream);

typedef struct cse_functor_ops {
  int32_t abi_version;          /* CSE_ABI_VERSION */
  int32_t num_residuals;        /* kNumResiduals */
  int32_t num_parameter_blocks; /* sizeof...(Ns) */
  int32_t parameter_block_sizes[CSE_MAX_PARAMETER_BLOCKS];
  int32_t data_size;            /* doubles of functor data per residual block */
  int32_t loss_kind;            /* the cse_loss_kind the kernels apply; groups must match */
  int32_t loss_size;            /* CSE_LOSS_USER: bytes of the loss object */
  int32_t kernel_args_size;
  int32_t gradient_args_size;
  int32_t camera_gradient_args_size; /* with camera_gradient; else 0 */
  int32_t reserved;             /* 0 */
  uint64_t kernel_args_tag;
  const char* name;             /* copied; for messages and cse_functor_name */
  cse_kernel_launch_fn table[2];        /* general kernel [0 residuals/cost, 1 + Jacobian] */
  cse_kernel_launch_fn affine[2][2][2]; /* [CompressedRow][Jacobian][LDS-DMA gather]; NULL = none */
  cse_multiply_launch_fn multiply;
  cse_gradient_launch_fn gradient[2];   /* per slot of an affine kind; NULL = in-kernel atomics */
  /* ABI 5, two-slot affine kinds whose slot 1 has 3 parameters (both or
   * neither): gradient_mode 0's fused form, as the library's Snavely kinds
   * take it -- the Jacobian kernel that also sums the slot-1 rows
   * [CompressedRow], and the slot-0 rows by re-evaluation.  NULL = the
   * gradient post-passes above. */
  cse_kernel_launch_fn fused_points[2];
  cse_camera_gradient_launch_fn camera_gradient;
} cse_functor_ops;

/* Registers a user functor kind; *kind receives its number
 * (>= CSE_FUNCTOR_USER_FIRST).  Registering the same table again (same name,
 * shape and launch functions) returns the same kind. */
int cse_register_functor(const cse_functor_ops* ops, int32_t* kind);

/* Shape of a built-in or registered kind; parameter_block_sizes receives
 * *num_parameter_blocks entries (room for CSE_MAX_PARAMETER_BLOCKS). */
int cse_functor_shape(int32_t kind, int32_t* num_residuals, int32_t* num_parameter_blocks,
                      int32_t* parameter_block_sizes, int32_t* data_size);

/* Synchronises the evaluator's stream and returns the status of the most
 * recent evaluation (CSE_OK / CSE_EVALUATION_FAILED) or an error. */
int cse_wait(cse_evaluator* ev);

/* Replaces RegisteredCUDAEvaluators::UpdatePlusJacobians
 * (registered_cuda_evaluators.cc:105-121): host array of
 * num_plus_jacobian_values doubles. */
int cse_set_plus_jacobians(cse_evaluator* ev, const double* plus_jacobians);

/* Replaces Evaluator::Plus -> Program::Plus (internal/ceres/program.cc:121-149,
 * internal/ceres/parameter_block.h:227-251) for problems whose active
 * parameter blocks have no manifold or the quaternion manifold:
 * x_plus_delta = x + delta block by block (state offsets vs delta offsets of
 * the descriptor), CSE_MANIFOLD_QUATERNION_EUCLIDEAN blocks by their
 * manifold's Plus.  Box constraints are not part of the descriptor, so none
 * are applied.  Returns CSE_ERR_UNSUPPORTED when an active block has an
 * explicit plus-Jacobian manifold (the caller keeps Ceres' host Plus).
 *   cse_plus_device: device pointers, asynchronous on the evaluator's stream
 *   cse_plus:        host pointers, synchronous */
int cse_plus_device(cse_evaluator* ev, const double* d_state, const double* d_delta,
                    double* d_state_plus_delta);
int cse_plus(cse_evaluator* ev, const double* state, const double* delta,
             double* state_plus_delta);

/* The Jacobian as a linear operator on the device (a consumer of
 * the evaluator's output that keeps it in HBM).  J is d_jacobian_values as
 * this evaluator writes it (the descriptor's BlockSparse or CompressedRow
 * layout); x and y are device vectors; asynchronous on the evaluator's
 * stream.
 *   cse_jacobian_right_multiply: y += J x  (x: num_effective_parameters,
 *       y: num_residuals) -- CudaSparseMatrix::RightMultiplyAndAccumulate
 *       (internal/ceres/cuda_sparse_matrix.h:77), BlockSparseMatrix::
 *       RightMultiplyAndAccumulate (block_sparse_matrix.h:76)
 *   cse_jacobian_left_multiply:  y += J^T x (x: num_residuals,
 *       y: num_effective_parameters) -- LeftMultiplyAndAccumulate
 *       (cuda_sparse_matrix.h:79, block_sparse_matrix.h:81); deterministic on
 *       the affine path (per-parameter-block ordered sums), FP64 atomics on
 *       the table path.
 * The reference copies the values to the host and back (CopyValuesFromCpu,
 * cuda_sparse_matrix.h:96); here they never leave HBM. */
int cse_jacobian_right_multiply(cse_evaluator* ev, const double* d_jacobian_values,
                                const double* d_x, double* d_y);
int cse_jacobian_left_multiply(cse_evaluator* ev, const double* d_jacobian_values,
                               const double* d_x, double* d_y);

/* The CGNR normal operator: y += J^T (J x) + D .* D .* x (d_D may be NULL),
 * device pointers, asynchronous on the evaluator's stream.  Replaces
 * CudaCgnrLinearOperator::RightMultiplyAndAccumulate
 * (internal/ceres/cgnr_solver.cc:226-237: z = A x, y += A^T z, y.DtDxpy(D, x)).
 * Groups eligible for the fused gradient (cse_info.num_fused_gradient_groups)
 * read J once and never materialise z; otherwise the two products above.
 * Deterministic on the affine path. */
int cse_cgnr_multiply(cse_evaluator* ev, const double* d_jacobian_values, const double* d_D,
                      const double* d_x, double* d_y);

/* The two column operations the trust-region loop runs on every Jacobian
 * between Evaluate and LinearSolver::Solve, on the values in HBM: device
 * pointers, asynchronous on the evaluator's stream, single-device evaluators
 * with a Jacobian layout only.  Null arguments return CSE_ERR_INVALID.
 *
 *   cse_jacobian_squared_column_norm: d_x[c] = sum over rows of J[r][c]^2,
 *       num_effective_parameters entries -- SparseMatrix::SquaredColumnNorm
 *       (internal/ceres/sparse_matrix.h:81, block_sparse_matrix.cc:342,
 *       compressed_row_sparse_matrix.cc:378), which TrustRegionMinimizer calls
 *       for jacobi_scaling (trust_region_minimizer.cc:259-275) and
 *       LevenbergMarquardtStrategy::ComputeStep for the LM diagonal
 *       (levenberg_marquardt_strategy.cc:78-94).  d_x is ASSIGNED, as the
 *       reference zeroes x first: the call zero-fills it and every group then
 *       adds its columns' sums, so a column no cell touches reads 0 and
 *       columns that several groups share are complete.  Deterministic on the
 *       affine path: each parameter block sums its blocks in the fixed order of
 *       the gradient plan (points: block order; cameras: chunks, a fixed
 *       butterfly, an ordered chunk reduce) and the groups add in group order,
 *       so repeats are bit-identical.  Groups on the table path (any layout,
 *       constant blocks, tangent sizes, held cameras) and affine groups without
 *       a gradient plan add with FP64 atomics: the split
 *       cse_jacobian_left_multiply has.  J is read once; no scratch of
 *       num_jacobian_values is allocated.
 *   cse_jacobian_scale_columns: J[r][c] *= d_scale[c], in place --
 *       SparseMatrix::ScaleColumns (sparse_matrix.h:87,
 *       block_sparse_matrix.cc:418, compressed_row_sparse_matrix.cc:434).  One
 *       IEEE multiply per stored value: bit-exact value * scale[column] on every
 *       path.  Every value of every cell is touched exactly once, and nothing
 *       else in the buffer is read or written. */
int cse_jacobian_squared_column_norm(cse_evaluator* ev, const double* d_jacobian_values,
                                     double* d_x);
int cse_jacobian_scale_columns(cse_evaluator* ev, double* d_jacobian_values,
                               const double* d_scale);

/* ---- ITERATIVE_SCHUR on the device -------------------------------------
 * The implicit Schur complement of the Jacobian this evaluator wrote, for
 * the linear solve of a Schur-ordered bundle adjustment problem: replaces
 * ImplicitSchurComplement (internal/ceres/implicit_schur_complement.h:
 * 86-160) and the preconditioners IterativeSchurComplementSolver builds
 * (iterative_schur_complement_solver.cc:172-204).  With the Jacobian
 * A = [E F] (e blocks = the points, slot 1; f blocks = the cameras, slot 0),
 * a per-column diagonal D and the right-hand side b, the system
 * (A^T A + D^2) [y_e; y_f] = A^T b is reduced to
 *     S y_f = rhs,  S = F^T F + D_f^2 - F^T E (E^T E + D_e^2)^-1 E^T F,
 *     rhs = F^T (b - E (E^T E + D_e^2)^-1 E^T b).
 * Requires (CSE_ERR_UNSUPPORTED otherwise) one group of the Snavely shape
 * (2 residuals, a camera of 9 tangent parameters, a point of 3: the
 * library's Snavely kinds or a user kind; the operators read only the
 * Jacobian) on the affine BlockSparseMatrix path whose points occupy the effective columns
 * [0, num_cols_e) and cameras the rest, as ITERATIVE_SCHUR's elimination
 * ordering gives.  Held cameras (constant slot-0 blocks,
 * Problem::SetParameterBlockConstant) are allowed when the active cameras'
 * columns tile [num_cols_e, num_effective_parameters) in id order, 9 each: a
 * held camera has no row or column anywhere, num_cols_f = 9 x (active
 * cameras), and a block with a held camera enters only the point sums
 * (F_b = 0).  Any other constant parameter block (a held point) is refused,
 * and on a program with held cameras so are the explicit complements below
 * (cse_schur_complement*, cse_schur_explicit_multiply, cse_schur_solve with
 * d_S_values).  All device pointers, asynchronous on the evaluator's
 * stream, deterministic. */
enum cse_schur_preconditioner {
  CSE_SCHUR_IDENTITY = 0,     /* IDENTITY: M^-1 = I */
  CSE_SCHUR_JACOBI = 1,       /* JACOBI: block diagonal (F^T F + D_f^2)^-1 */
  CSE_SCHUR_SCHUR_JACOBI = 2, /* SCHUR_JACOBI: block diagonal of S, inverted
                                 (schur_jacobi_preconditioner.cc:89-98) */
  CSE_SCHUR_POWER_SERIES_EXPANSION = 3 /* SCHUR_POWER_SERIES_EXPANSION: the
                                 truncated series of cse_schur_power_series with
                                 cse_schur_set_spse_iterations terms and
                                 tolerance 0 (power_series_expansion_
                                 preconditioner.cc); its init is JACOBI's */
};

/* The column split: num_cols_e (points) and num_cols_f (cameras). */
int cse_schur_structure(cse_evaluator* ev, int64_t* num_cols_e, int64_t* num_cols_f);

/* ImplicitSchurComplement::Init(A, D, b) (implicit_schur_complement.cc:
 * 53-99) plus Preconditioner::Update: binds d_jacobian_values, d_D
 * (num_effective_parameters entries, may be NULL) and d_b (num_residuals)
 * -- they must stay valid until the next init -- computes the per-point
 * (E^T E + D_e^2)^-1, writes rhs (num_cols_f) and builds the preconditioner.
 * With d_D NULL a block can be singular (a point seen by one residual block,
 * a camera without observations): a Cholesky pivot that is not positive
 * leaves that block's inverse zero and makes the next cse_wait return
 * CSE_EVALUATION_FAILED, where Eigen's LLT would spread NaN silently. */
int cse_schur_init(cse_evaluator* ev, const double* d_jacobian_values, const double* d_D,
                   const double* d_b, double* d_rhs, int preconditioner);

/* cse_schur_init, and also the gradient g = J^T r of the bound Jacobian into
 * d_gradient (num_effective_parameters entries, assigned), taking r = -b --
 * the trust-region step's b (TrustRegionMinimizer::EvaluateGradientAndJacobian
 * evaluates g = J^T r beside J, trust_region_minimizer.cc:242-255) -- in the
 * same passes over J: the e rows from the E^T b sums the init forms anyway,
 * the f rows -F^T b in the camera-order pass that forms F^T u and the
 * preconditioner, from b_b stored beside u_b.  Then the evaluation before it
 * needs no gradient (no CameraGradientKernel).  Deterministic; equals the
 * evaluation's gradient (gradient_mode 0) to rounding (a different
 * summation order). */
int cse_schur_init_gradient(cse_evaluator* ev, const double* d_jacobian_values, const double* d_D,
                            const double* d_b, double* d_rhs, int preconditioner,
                            double* d_gradient);

/* y = S x (ImplicitSchurComplement::RightMultiplyAndAccumulate, :101-141,
 * which assigns y); x and y have num_cols_f entries. */
int cse_schur_multiply(cse_evaluator* ev, const double* d_x, double* d_y);

/* y += M^-1 x for the preconditioner chosen at init.  Under
 * CSE_SCHUR_POWER_SERIES_EXPANSION y += series(x) with the iteration count of
 * cse_schur_set_spse_iterations and tolerance 0; x and y may not overlap then
 * (CSE_ERR_INVALID).  Note the difference: this call ACCUMULATES into y,
 * cse_schur_power_series ASSIGNS y. */
int cse_schur_precondition(cse_evaluator* ev, const double* d_x, double* d_y);

/* ---- SCHUR_POWER_SERIES_EXPANSION ----------------------------------------
 * S^-1 = sum_i (P^-1 Q)^i P^-1 with P = blockdiag(F^T F + D_f^2) and
 * Q = P - S = F^T E (E^T E + D_e^2)^-1 E^T F, truncated: the reference's
 * preconditioner SCHUR_POWER_SERIES_EXPANSION and its initial guess
 * Solver::Options::use_spse_initialization (iterative_schur_complement_
 * solver.cc:108-118, :186-189).  A term is the passes of one S product on the
 * same cells (InversePowerSeriesOperatorRightMultiplyAccumulate,
 * implicit_schur_complement.cc:146-174) and a 9x9 block apply. */
typedef struct cse_spse_summary {
  int32_t num_terms;      /* series terms added after the zeroth: 1 .. max_num_iterations */
  int32_t reserved;
  double  norm_first;     /* |(FtF+D^2)^-1 x|, the threshold's base */
  double  norm_last;      /* |last term added| */
} cse_spse_summary;

/* PowerSeriesExpansionPreconditioner::RightMultiplyAndAccumulate (:51-72), which
 * despite its name ASSIGNS y (it zeroes y first; cse_schur_precondition
 * accumulates):
 *   y = P^-1 x;  prev = y;  threshold = tolerance * |y|
 *   for i = 1, 2, ...:  term = P^-1 Q prev;  y += term;
 *                       stop if i >= max_num_iterations or |term| < threshold;  prev = term
 * x and y have num_cols_f entries and may not overlap.  Needs cse_schur_init
 * with ANY preconditioner, on every program the implicit operators serve (held
 * cameras included).  After a JACOBI or POWER_SERIES_EXPANSION init the P^-1
 * blocks are the init's; after IDENTITY or SCHUR_JACOBI the first call that
 * follows the init builds them into a buffer of its own, by the pass a JACOBI
 * init runs (the same blocks bit for bit), and cse_schur_precondition keeps
 * applying the init's preconditioner.  The zeroth term is what
 * cse_schur_precondition gives under a JACOBI init.
 * All max_num_iterations terms are enqueued without a host wait; the norms and
 * the stop test run on the device, and once the series has stopped the terms
 * enqueued behind it change nothing, so the result is the same bits whether or
 * not the host looks.  tolerance 0 never stops early.  summary NULL: the call
 * is asynchronous on the evaluator's stream; else it waits once on that stream
 * and fills the summary.  Deterministic.
 * CSE_ERR_INVALID: no cse_schur_init; NULL d_x or d_y; max_num_iterations < 1;
 * a tolerance that is negative or not finite (solver.cc:277-281); d_x
 * overlapping d_y.  CSE_ERR_UNSUPPORTED on a cse_create_multi handle.  Two
 * num_cols_f vectors, the state, a pinned copy of it and (after IDENTITY or
 * SCHUR_JACOBI) the block buffer are allocated by the first call, kept, and
 * released by cse_destroy.
 * use_spse_initialization is this call into d_x (max_num_spse_iterations,
 * spse_tolerance, rhs) followed by cse_schur_solve without
 * CSE_CG_ZERO_INITIAL_GUESS. */
int cse_schur_power_series(cse_evaluator* ev, int32_t max_num_iterations, double tolerance,
                           const double* d_x, double* d_y, cse_spse_summary* summary /* may be NULL */);

/* max_num_spse_iterations of the POWER_SERIES_EXPANSION preconditioner
 * (default 5, linear_solver.h:172): what cse_schur_precondition and
 * cse_schur_solve run under that init.  Kept across inits.  CSE_ERR_INVALID
 * below 1. */
int cse_schur_set_spse_iterations(cse_evaluator* ev, int32_t max_num_iterations);

/* ---- CLUSTER_JACOBI -------------------------------------------------------
 * The reference's visibility-based preconditioner CLUSTER_JACOBI
 * (visibility_based_preconditioner.cc): M = blockdiag(M_g), M_g = S restricted
 * to the cameras of cluster g, factored M_g = L_g L_g^T and applied by a
 * forward and a backward substitution (:424-431).  The partition is the
 * caller's (ceres_amd/clustering.py computes the reference's single-linkage
 * one).  One cluster is factored in the LDS of one workgroup, which caps a
 * cluster at CSE_SCHUR_MAX_CLUSTER_CAMERAS cameras (144 columns: one triangle
 * of 9x9 tiles takes 88,128 B of the 163,840 B a workgroup may declare). */
#define CSE_SCHUR_MAX_CLUSTER_CAMERAS 16

/* Host pointer.  cluster_of_camera[c] for camera c = 0 .. num_cameras-1 in
 * f-column order (num_cameras = num_cols_f / 9), labels in [0, num_clusters),
 * every label used.  Kept across inits; replaces an earlier partition.  When
 * the partition changed, the call builds the cluster-filtered pair plan on the
 * host and uploads it (it waits on the evaluator's stream); the same partition
 * again costs a comparison.  Needs no cse_schur_init.  A CHANGED partition
 * also deactivates a factor that cse_schur_cluster_jacobi built for the
 * earlier one: until the next cse_schur_cluster_jacobi,
 * cse_schur_precondition and cse_schur_solve apply the init's own
 * preconditioner again.  The same partition again leaves the factor active.
 * CSE_ERR_INVALID: NULL cluster_of_camera, wrong num_cameras, a label out of
 * range, an unused label.  CSE_ERR_UNSUPPORTED: a cluster of more than
 * CSE_SCHUR_MAX_CLUSTER_CAMERAS cameras (the message names the cluster and
 * its size); a program with held cameras (the pair plan addresses F cells by
 * block index); a cse_create_multi handle; a program that is not
 * Schur-eligible. */
int cse_schur_set_clusters(cse_evaluator* ev, const int32_t* cluster_of_camera,
                           int64_t num_cameras, int32_t num_clusters);

/* Needs cse_schur_init (any preconditioner) and cse_schur_set_clusters.  Reads
 * the bound Jacobian, D and the per-point inverses the init left; for every
 * cluster g with cameras c0 < c1 < ... forms M_g = S[g, g] (each 9x9 cell the
 * bits of cse_schur_complement's), factors it and makes the result the active
 * preconditioner: until the next cse_schur_init, cse_schur_precondition
 * accumulates y += M^-1 x and cse_schur_solve uses the same apply for
 * z = M^-1 r, on the implicit operator and on d_S_values.  The next
 * cse_schur_init restores the init's own preconditioner: call this again after
 * it, once per linear solve, as Preconditioner::Update is.
 * d_matrices non-NULL: the UNFACTORED matrices are written too, cluster g as
 * a dense row-major n_g x n_g matrix with both triangles, n_g = 9 |g|, at
 * offset sum_{h<g} n_h^2, clusters in label order and cameras ascending inside
 * a cluster.
 * Asynchronous on the evaluator's stream, deterministic, no atomics.  A pivot
 * that is not positive leaves that cluster's apply adding zeros and makes the
 * next cse_wait return CSE_EVALUATION_FAILED (the init's convention).  The
 * filtered plan, the factors and the partials are allocated by
 * cse_schur_set_clusters, kept, and released by cse_destroy.
 * CSE_ERR_INVALID: no init, no partition.  CSE_ERR_UNSUPPORTED as
 * cse_schur_set_clusters. */
int cse_schur_cluster_jacobi(cse_evaluator* ev, double* d_matrices /* may be NULL */);

/* ---- CLUSTER_TRIDIAGONAL ---------------------------------------------------
 * The reference's second visibility-based preconditioner
 * (visibility_based_preconditioner.cc:130-154, 318-390): besides the cluster
 * blocks M_gg = S[g, g] it keeps M_gh = S[g, h] for the edges (g, h) of a
 * forest over the clusters in which no cluster has more than two edges
 * (Degree2MaximumSpanningForest; ceres_amd/clustering.py computes it).  Every
 * tree of such a forest is a path, and along a path M is block tridiagonal; one
 * workgroup factors a path and one applies it.  One elimination step holds
 * the two clusters of an edge in the LDS of one workgroup: the two clusters of
 * EVERY EDGE have at most CSE_SCHUR_MAX_CLUSTER_CAMERAS cameras together (a
 * cluster without an edge may have that many alone).
 *
 * Host pointer: edges[e] = (g, h), cluster labels of the partition that
 * cse_schur_set_clusters installed.  num_edges = 0 is legal (every path is
 * one cluster).  Builds and uploads the filtered plan when the forest changed.
 * A changed partition DROPS the forest; a changed partition or forest
 * deactivates a factor that cse_schur_cluster_tridiagonal built.
 * cse_schur_cluster_jacobi's plan and results do not depend on the forest.
 * CSE_ERR_INVALID: NULL edges with num_edges > 0, a label out of range, g = h,
 * an edge given twice (in either orientation), no partition.
 * CSE_ERR_UNSUPPORTED (the message names the cluster or edge): a cluster with
 * three edges, a cycle, an edge whose clusters hold more than
 * CSE_SCHUR_MAX_CLUSTER_CAMERAS cameras together; and cse_schur_set_clusters'
 * own: held cameras, cse_create_multi, a program that is not Schur-eligible. */
int cse_schur_set_cluster_forest(cse_evaluator* ev, const int32_t* edges /* [num_edges][2], host */,
                                 int32_t num_edges);

/* Needs cse_schur_init (any preconditioner), cse_schur_set_clusters and
 * cse_schur_set_cluster_forest.  Forms M's cells (each with the bits
 * cse_schur_complement gives it), factors every path and makes the factor the
 * active preconditioner of cse_schur_precondition and cse_schur_solve
 * (implicit operator and d_S_values) until the next cse_schur_init or cluster
 * build.  Asynchronous on the evaluator's stream, no atomics, bit-identical
 * run to run.
 * M need not be positive definite.  As the reference does, the factor is tried
 * on M as it is; if any pivot is not positive, EVERY off-diagonal block M_gh,
 * of every path, is multiplied by 0.5 and all paths are factored again -- on
 * the device, without a host wait.  d_scaled (device, may be NULL) receives 0
 * or 1: whether that second pass ran.  A pivot that is not positive in the
 * second pass too leaves that path's apply adding zeros and makes the next
 * cse_wait return CSE_ERR_INVALID.
 * d_matrices (device, may be NULL) receives the UNSCALED, UNFACTORED cells:
 * first the cluster matrices exactly as cse_schur_cluster_jacobi lays them
 * out, then per edge, in the order and orientation cse_schur_set_cluster_forest
 * received them, S[g, h] dense row-major (9 n_g) x (9 n_h), cameras ascending
 * inside each cluster. */
int cse_schur_cluster_tridiagonal(cse_evaluator* ev, double* d_matrices /* may be NULL */,
                                  int32_t* d_scaled /* may be NULL */);

/* ImplicitSchurComplement::BackSubstitute(x, y) (:216-238): y
 * (num_effective_parameters) = [(E^T E + D_e^2)^-1 E^T (b - F x); x]. */
int cse_schur_back_substitute(cse_evaluator* ev, const double* d_x, double* d_y);

/* SchurEliminator::Eliminate's lhs (schur_eliminator_impl.h) into a dense
 * BlockRandomAccessDenseMatrix-like buffer, for DENSE_SCHUR
 * (schur_complement_solver.cc).  Needs cse_schur_init (any preconditioner) on
 * this evaluator: uses the Jacobian, D and M_p it bound/computed.  Assigns all
 * f_cols x f_cols entries of row-major d_S with leading dimension ld >= f_cols
 * (zeros where two cameras share no point), both triangles; entries
 * [row][f_cols..ld) are not touched.  Asynchronous on the evaluator's stream,
 * deterministic.  A point that sees one camera in several residual blocks is
 * fine (its cross terms land in the diagonal block).  The first call builds
 * the co-visibility plan on the host and uploads it (CSE_ERR_OOM when it does
 * not fit); later calls, after any cse_schur_init, reuse it. */
int cse_schur_complement(cse_evaluator* ev, double* d_S, int64_t ld);

/* Counts only, no allocation: the non-zero 9x9 blocks of S's upper triangle
 * (co-visible camera pairs, diagonal included), the pair records of the plan
 * and the device bytes the plan will take; any pointer may be NULL. */
int cse_schur_complement_plan(cse_evaluator* ev, int64_t* num_blocks,
                              int64_t* num_pairs, int64_t* plan_bytes);

/* The same S as 9x9 blocks of its upper triangle, the cells of the
 * BlockRandomAccessSparseMatrix that SchurEliminator::Eliminate fills for
 * SPARSE_SCHUR (schur_complement_solver.cc) and that ITERATIVE_SCHUR multiplies
 * by under Solver::Options::use_explicit_schur_complement.  Cameras are indexed
 * 0..C-1, C = num_cols_f / 9, in f-column order.  Same eligibility and
 * refusals as cse_schur_complement.
 *
 * Structure of S's upper triangle as block-compressed rows: for camera c the
 * blocks [row_begin[c], row_begin[c+1]) with ascending block_col >= c, the
 * diagonal block first.  EVERY camera has its diagonal block, observed or not
 * (BlockRandomAccessSparseMatrix always holds the diagonal); off-diagonal
 * blocks are exactly the co-visible pairs.  Host arrays, any pointer may be
 * NULL (counts only: nothing is allocated on the device; with row_begin or
 * block_col the plan and the structure are built and uploaded as the first
 * cse_schur_complement_sparse would, CSE_ERR_OOM when they do not fit).  Needs
 * no cse_schur_init.  device_bytes = what cse_schur_complement_sparse and
 * cse_schur_explicit_multiply will hold on the device besides the values and
 * cse_schur_complement_plan's plan_bytes. */
int cse_schur_complement_sparse_structure(cse_evaluator* ev, int64_t* num_block_rows,
                                          int64_t* num_blocks, int64_t* device_bytes,
                                          int64_t* row_begin /*[C+1]*/, int32_t* block_col /*[num_blocks]*/);

/* The values: d_values[k][9][9], row-major per block, in structure order;
 * 81 * num_blocks doubles, every one assigned (a camera without residual
 * blocks: diag(D^2), or zeros without D).  Each block equals the same block
 * of cse_schur_complement's dense S bit for bit; diagonal blocks are
 * symmetric bit for bit.  Needs cse_schur_init (any preconditioner).
 * Asynchronous on the evaluator's stream, deterministic. */
int cse_schur_complement_sparse(cse_evaluator* ev, double* d_values);

/* y = S x (assigned, as cse_schur_multiply) from values laid out as above;
 * x, y: num_cols_f entries that do not overlap (CSE_ERR_INVALID when they
 * do).  Asynchronous, deterministic, no atomics. */
int cse_schur_explicit_multiply(cse_evaluator* ev, const double* d_values,
                                const double* d_x, double* d_y);

/* The solver over these operators: ConjugateGradientsSolver
 * (internal/ceres/conjugate_gradients_solver.h:108-305) statement for
 * statement, as IterativeSchurComplementSolver runs it
 * (iterative_schur_complement_solver.cc:63-170), with every vector, scalar and
 * stopping test on the device.  The host enqueues check_period iterations,
 * copies the 96-byte state back, waits once and stops or goes on; iterations
 * enqueued past the end change nothing, so the result does not depend on
 * check_period. */
enum cse_cg_termination {       /* = LinearSolverTerminationType */
  CSE_CG_SUCCESS = 0,
  CSE_CG_NO_CONVERGENCE = 1,
  CSE_CG_FAILURE = 2
};

enum cse_cg_reason {            /* the statement of the reference that ended it */
  CSE_CG_REASON_MAX_ITERATIONS = 0,    /* :299-301 */
  CSE_CG_REASON_ZERO_RHS = 1,          /* :131-136, |b| = 0: x = 0 */
  CSE_CG_REASON_INITIAL_RESIDUAL = 2,  /* :147-152, min_num_iterations == 0 */
  CSE_CG_REASON_RHO = 3,               /* :168-172, FAILURE */
  CSE_CG_REASON_BETA = 4,              /* :178-187, FAILURE */
  CSE_CG_REASON_INDEFINITE = 5,        /* :196-205, p'q <= 0: NO_CONVERGENCE */
  CSE_CG_REASON_ALPHA = 6,             /* :208-216, FAILURE */
  CSE_CG_REASON_Q_TOLERANCE = 7,       /* :273-283 */
  CSE_CG_REASON_R_TOLERANCE = 8        /* :288-297 */
};

#define CSE_CG_ZERO_INITIAL_GUESS 1u /* x = 0, r = rhs: no initial product; d_x's
                                        contents on entry are not read */

typedef struct cse_cg_options {
  int32_t min_num_iterations;     /* 1   (linear_solver.h:165) */
  int32_t max_num_iterations;     /* caller sets; cse_cg_default_options: 500 */
  int32_t residual_reset_period;  /* 10  (linear_solver.h:211) */
  int32_t check_period;           /* 1: the host looks at the device state after
                                     every check_period iterations */
  double  r_tolerance;            /* |r| <= r_tolerance |b|;  <0 disables */
  double  q_tolerance;            /* i (Q_i - Q_{i-1}) / Q_i < q_tolerance */
  uint32_t flags;                 /* CSE_CG_ZERO_INITIAL_GUESS */
  int32_t reserved;               /* 0, checked */
} cse_cg_options;

typedef struct cse_cg_summary {
  int32_t termination_type;       /* cse_cg_termination */
  int32_t reason;                 /* cse_cg_reason */
  int32_t num_iterations;         /* the reference's summary.num_iterations */
  int32_t num_iterations_enqueued;
  int32_t num_synchronizations;   /* host waits on the stream in this call */
  int32_t reserved;
  double norm_rhs, norm_r, q, zeta, rho, pq;   /* as last computed (q: Q_i) */
} cse_cg_summary;

/* min 1, max 500, reset period 10, check period 1, r_tolerance -1,
 * q_tolerance 0, no flags. */
void cse_cg_default_options(cse_cg_options* options);

/* Solves S x = rhs by preconditioned conjugate gradients.  Needs
 * cse_schur_init, whose preconditioner it applies (IDENTITY: z = r;
 * POWER_SERIES_EXPANSION: each iteration enqueues z = series(r) and a direction
 * step that takes z as given; d_S_values is refused with CSE_ERR_UNSUPPORTED
 * then, the reference allows only SCHUR_JACOBI on the explicit complement).
 *   d_S_values  NULL: the implicit operator (cse_schur_multiply); else the
 *               values cse_schur_complement_sparse wrote
 *               (cse_schur_explicit_multiply); the structure must be uploaded
 *   d_rhs       num_cols_f, cse_schur_init's d_rhs
 *   d_x         num_cols_f; in: the initial guess (not read under
 *               CSE_CG_ZERO_INITIAL_GUESS), out: the solution; may not overlap d_rhs
 *   d_step      NULL, or num_effective_parameters: cse_schur_back_substitute(x)
 *               when the termination type is not FAILURE, left alone when it
 *               is; queued on the stream after the last wait, as that call
 * Returns CSE_OK for every termination type (the summary says which) after
 * waiting for the last state on the evaluator's stream; negative for usage
 * and HIP errors.  CSE_ERR_INVALID: a NULL options, summary, d_rhs or d_x;
 * check_period, residual_reset_period or max_num_iterations < 1;
 * min_num_iterations < 0; reserved != 0; unknown flags; d_x overlapping d_rhs;
 * d_S_values before the sparse structure is uploaded; no cse_schur_init.
 * CSE_ERR_UNSUPPORTED on a cse_create_multi handle.  Four num_cols_f vectors
 * and the state are allocated by the first call and kept; deterministic: two
 * calls with the same inputs give the same bits. */
int cse_schur_solve(cse_evaluator* ev, const cse_cg_options* options,
                    const double* d_S_values, const double* d_rhs, double* d_x,
                    double* d_step, cse_cg_summary* summary);

/* ---- CGNR on the device --------------------------------------------------
 * CudaCgnrSolver (internal/ceres/cgnr_solver.cc:218-387), the one linear
 * solver the reference runs on the GPU, over this evaluator's Jacobian values
 * in HBM: the operator (cse_cgnr_multiply = CudaCgnrLinearOperator, :218-243),
 * an IDENTITY or JACOBI preconditioner (:245-280), the right-hand side A^T b
 * (:365-367) and ConjugateGradientsSolver over four scratch vectors (:375-383).
 * Every single-device evaluator with a Jacobian layout is served -- several
 * groups, the table path, any shape, held blocks, both layouts: whatever
 * cse_cgnr_multiply serves.
 *
 * JACOBI is BlockCRSJacobiPreconditioner (block_jacobi_preconditioner.cc:
 * 116-224): per non-constant parameter block the tangent_size x tangent_size
 * matrix (sum over its cells of J_cell^T J_cell + diag(D^2))^-1 by Cholesky
 * (:208-221), stored as packed row-major blocks in delta-offset order (:133-145).
 * The reference computes it on the CPU and copies it over on every solve
 * (cgnr_solver.cc:267-270); here it is built on the device from the values.
 * Deterministic on affine groups with gradient plans (each parameter block adds
 * its cells in the plan's fixed order, the groups in group order); FP64 atomics
 * for every other group, the split cse_jacobian_squared_column_norm has.  A
 * block whose pivot is not positive and finite (an unobserved block with
 * D = NULL) is left zero and the next cse_wait returns CSE_EVALUATION_FAILED,
 * as cse_schur_init documents.  JACOBI is refused (CSE_ERR_UNSUPPORTED) when
 * the non-constant blocks do not tile [0, num_effective_parameters) exactly or
 * one has more than 16 tangent columns; IDENTITY never is. */
enum cse_cgnr_preconditioner { CSE_CGNR_IDENTITY = 0, CSE_CGNR_JACOBI = 1 };

/* Binds J and D (D may be NULL; both must stay valid until the next init).
 * d_b / d_rhs: both NULL, or rhs = J^T b assigned (d_b: num_residuals, d_rhs:
 * num_effective_parameters; cgnr_solver.cc:365-367).  JACOBI: builds the
 * block-diagonal inverse described above.  Asynchronous on the evaluator's
 * stream.  CSE_ERR_INVALID: a NULL evaluator or d_jacobian_values, one of
 * d_b / d_rhs alone, an unknown preconditioner, no Jacobian layout. */
int cse_cgnr_init(cse_evaluator* ev, const double* d_jacobian_values, const double* d_D,
                  const double* d_b, double* d_rhs, int preconditioner);

/* y += M^-1 x, num_effective_parameters entries (IDENTITY: y += x;
 * cgnr_solver.cc:249-251, :272-274).  x and y may not overlap.  Needs
 * cse_cgnr_init. */
int cse_cgnr_precondition(cse_evaluator* ev, const double* d_x, double* d_y);

/* (J^T J + D^2) x = rhs by the reference's ConjugateGradientsSolver
 * (conjugate_gradients_solver.h:108-305), every vector, scalar and stopping
 * test on the device, as cse_schur_solve: the same options, summary and
 * CSE_CG_ZERO_INITIAL_GUESS, the same argument checks, CSE_OK for every
 * termination type, deterministic and independent of check_period.  d_rhs,
 * d_x: num_effective_parameters entries that do not overlap.  CSE_ERR_INVALID
 * without a prior cse_cgnr_init; CSE_ERR_UNSUPPORTED on a cse_create_multi
 * handle.  The vector kernels are sliced (one workgroup per 2048 entries, the
 * slice sums combined in a fixed order by the workgroup that finishes last);
 * four num_effective_parameters vectors, the slice partials and the state are
 * allocated by the first call and kept. */
int cse_cgnr_solve(cse_evaluator* ev, const cse_cg_options* options, const double* d_rhs,
                   double* d_x, cse_cg_summary* summary);

/* ---- Dense Cholesky on the device ----------------------------------------
 * DenseCholesky's device forms (internal/ceres/dense_cholesky.h:195-302,
 * dense_cholesky.cc:348-640): CUDADenseCholesky, an FP64 potrf/potrs, and
 * CUDADenseCholeskyMixedPrecision, an FP32 factor with FP64 iterative
 * refinement; what Solver::Options::dense_linear_algebra_library_type = CUDA,
 * use_mixed_precision_solves and max_num_refinement_iterations select.  No
 * vendor library: a blocked right-looking factorization in HIP, 64 columns per
 * panel, the trailing update on the matrix cores.  The evaluator supplies the
 * device and the stream and owns the workspace; nothing here needs a
 * Schur-eligible program, and n is the caller's.  Everything is asynchronous
 * on the evaluator's stream (no host wait in factorize or solve), uses no
 * atomics and is bit-identical from run to run.  CSE_ERR_UNSUPPORTED on a
 * cse_create_multi handle. */
enum { CSE_DENSE_CHOLESKY_FP64 = 0, CSE_DENSE_CHOLESKY_FP32 = 1 };

/* DenseCholesky::Factorize (dense_cholesky.h:67-75; CUDADenseCholesky::Factorize
 * dense_cholesky.cc:364-407, CUDADenseCholeskyMixedPrecision::Factorize
 * :543-560).  d_A: row-major n x n, leading dimension ld >= n, symmetric
 * positive definite; only the lower triangle, diagonal included, is ever read
 * (dense_cholesky.h:67-69); the strict upper triangle and the entries
 * [row][n..ld) are neither read nor written.  cse_schur_complement's output is
 * a valid input as it stands.
 *   CSE_DENSE_CHOLESKY_FP64: in place, the lower triangle of d_A receives L
 *     (A = L L^T); d_A must stay valid and unmodified until the last solve.
 *   CSE_DENSE_CHOLESKY_FP32: d_A is not written; its lower triangle is cast to
 *     float into the workspace and factored there in single precision (the
 *     reference's Spotrf).  A refining solve reads d_A again, so it must stay
 *     unchanged until the last solve (bound as cse_schur_init binds the
 *     Jacobian).
 * A pivot that is not positive and finite stops the factorization's effect
 * (the panels before it are done: in FP64 d_A's lower triangle is then
 * unspecified, partly L and partly updated, as after LAPACK's potrf)
 * (LAPACK's info > 0, LinearSolverTerminationType::FAILURE at
 * dense_cholesky.cc:397-403): cse_dense_cholesky_info reports it, the
 * evaluator's status word and cse_wait are not affected.  CSE_ERR_INVALID: a
 * null pointer, n < 1, ld < n, an unknown precision.  CSE_ERR_OOM: the
 * workspace (cse_dense_cholesky_workspace) does not fit; it is kept across
 * calls, grown when needed and released by cse_destroy. */
int cse_dense_cholesky_factorize(cse_evaluator* ev, int64_t n, double* d_A, int64_t ld, int32_t precision);

/* DenseCholesky::Solve (CUDADenseCholesky::Solve dense_cholesky.cc:409-450:
 * x = L^-T L^-1 rhs; CUDADenseCholeskyMixedPrecision::Solve :594-637, statement
 * for statement: x = 0, r = rhs; for i = 0 .. max_num_refinement_iterations:
 * r32 = (float) r, c = L32^-T L32^-1 r32 in FP32, x += (double) c; and, if
 * i < max, r = rhs - A x in FP64 from the lower triangle of d_A).  d_rhs, d_x:
 * n entries, the same buffer or disjoint.  After a failed factorization d_x is
 * assigned zeros.  CSE_ERR_INVALID: a null pointer, a negative refinement
 * count, no prior factorize, d_x overlapping d_rhs partially.
 * CSE_ERR_UNSUPPORTED: FP64 with a refinement count other than 0 (the factor
 * has overwritten the matrix a residual would need; RefinedDenseCholesky is
 * not provided). */
int cse_dense_cholesky_solve(cse_evaluator* ev, const double* d_rhs, double* d_x,
                             int32_t max_num_refinement_iterations);

/* potrf's info (dense_cholesky.cc:386-403): waits on the stream; 0 after a
 * success, else the 1-based order of the first leading minor that is not
 * positive definite.  A later factorize starts again from 0.  CSE_ERR_INVALID
 * before any factorize. */
int cse_dense_cholesky_info(cse_evaluator* ev, int32_t* info);

/* The device bytes a factorize of this n and precision holds (potrf's
 * bufferSize query, dense_cholesky.cc:372-383, plus the float copy and the
 * refinement vectors of :543-592); allocates nothing, needs no evaluator. */
int cse_dense_cholesky_workspace(int64_t n, int32_t precision, int64_t* device_bytes);

/* ---- Block-sparse Cholesky on the device ---------------------------------
 * The SparseCholesky behind SPARSE_SCHUR: SparseSchurComplementSolver::
 * SolveReducedLinearSystem (internal/ceres/schur_complement_solver.cc:290-333)
 * hands BlockRandomAccessSparseMatrix's cells to a SparseCholesky
 * (sparse_cholesky.h:72-113) whose symbolic analysis is done once, every later
 * Factorize having the same structure (sparse_cholesky.h:55-56), wrapped in
 * RefinedSparseCholesky when max_num_refinement_iterations > 0
 * (sparse_cholesky.h:119).  No vendor library: a host-only symbolic plan, then
 * a left-looking factorization of 9 x 9 blocks in HIP, one level of the
 * elimination tree at a time, the block products on the matrix cores.  The
 * evaluator supplies the device and the stream and owns the tables, L and the
 * solve vectors; nothing here needs a Schur-eligible program, the matrix is
 * the caller's.  Factorize and solve are asynchronous on the evaluator's
 * stream (no host wait), use no atomics on floating-point data and are
 * bit-identical from run to run.  CSE_ERR_UNSUPPORTED on a cse_create_multi
 * handle. */
enum { CSE_SPARSE_ORDERING_NATURAL = 0, CSE_SPARSE_ORDERING_MINIMUM_DEGREE = 1, CSE_SPARSE_ORDERING_GIVEN = 2 };
typedef struct cse_sparse_cholesky_summary {
  int64_t num_block_rows, num_input_blocks, num_factor_blocks, num_block_products;
  int64_t device_bytes;             /* tables + factor values + per-solve vectors */
  int32_t num_levels, max_level_columns;
} cse_sparse_cholesky_summary;

/* The symbolic analysis (sparse_cholesky.h:55-56: once per structure).  The
 * upper triangle of a symmetric matrix of 9 x 9 blocks as block-compressed
 * rows, host arrays, exactly what cse_schur_complement_sparse_structure
 * returns: block k of row r, k in [row_begin[r], row_begin[r + 1]), is
 * A(r, block_col[k]); every row starts with its diagonal block and block_col
 * ascends.  ordering: NATURAL, the identity; MINIMUM_DEGREE, the greedy rule
 * (repeatedly the block row with the fewest uneliminated neighbours in the
 * elimination graph, fill edges included, the lowest index on ties; it stands
 * where the reference's linear_solver_ordering_type AMD does and is not
 * SuiteSparse's AMD); GIVEN, permutation[k] = the original block row placed at
 * position k (ignored otherwise, may then be NULL).  Builds the elimination
 * tree, L's block structure with fill and the level tables on the host and
 * uploads them; a second analyze replaces the first and drops its factor.
 * num_block_products is the sum over columns of m (m + 1) / 2, m = the
 * column's blocks below its diagonal.  summary may be NULL.  CSE_ERR_INVALID:
 * null pointers, a row without its leading diagonal, columns not ascending or
 * out of range, a GIVEN array that is not a permutation, an unknown ordering.
 * CSE_ERR_UNSUPPORTED: 2^31 or more factor blocks.  CSE_ERR_OOM.  Value
 * offsets are 64-bit throughout. */
int cse_sparse_cholesky_analyze(cse_evaluator* ev, int64_t num_block_rows, const int64_t* row_begin,
                                const int32_t* block_col, int32_t ordering, const int32_t* permutation,
                                cse_sparse_cholesky_summary* summary);

/* Host copies of what the analysis decided; any pointer may be NULL.
 * permutation [num_block_rows]; L's block rows in the permuted order,
 * factor_row_begin [num_block_rows + 1] and factor_block_col
 * [num_factor_blocks], a row's columns ascending and its diagonal last; the
 * elimination tree's parent, -1 at a root; each column's level, 0 at a leaf,
 * else 1 + the largest level of a child: every column that column j reads
 * lies on a lower level.  CSE_ERR_INVALID before any analyze. */
int cse_sparse_cholesky_structure(cse_evaluator* ev, int32_t* permutation, int64_t* factor_row_begin,
                                  int32_t* factor_block_col, int32_t* parent, int32_t* level);

/* SparseCholesky::Factorize (sparse_cholesky.h:72-113).  d_values:
 * [num_input_blocks][9][9] row-major as cse_schur_complement_sparse writes
 * them (diagonal blocks whole and symmetric); read only.  It is bound as
 * cse_schur_init binds the Jacobian: a refining solve reads it again.  L goes
 * into storage the evaluator owns, allocated by the first factorize after an
 * analyze, kept for the later ones and released by the next analyze or by
 * cse_destroy.  A pivot that is not positive and finite
 * (LinearSolverTerminationType::FAILURE, schur_complement_solver.cc:316-321)
 * shows in cse_sparse_cholesky_info; the evaluator's status word and cse_wait
 * are not affected.  CSE_ERR_INVALID: a null pointer, no prior analyze. */
int cse_sparse_cholesky_factorize(cse_evaluator* ev, const double* d_values);

/* L's values, [num_factor_blocks][9][9] row-major in cse_sparse_cholesky_
 * structure's order, copied to d_L on the stream; a diagonal block's strict
 * upper triangle is zero.  CSE_ERR_INVALID: null, no prior factorize. */
int cse_sparse_cholesky_factor_values(cse_evaluator* ev, double* d_L);

/* SparseCholesky::Solve (schur_complement_solver.cc:323-331; one "iteration",
 * :329): x = A^-1 rhs in the original order, 9 num_block_rows entries each,
 * the same buffer or disjoint.  max_num_refinement_iterations > 0 is
 * RefinedSparseCholesky (sparse_cholesky.h:119), SparseIterativeRefiner's
 * loop: that many times r = rhs - A x in FP64 from d_values, x += L^-T L^-1 r;
 * d_values must therefore stay unchanged until the last refining solve.  After
 * a failed factorization x is assigned zeros.  CSE_ERR_INVALID: a null
 * pointer, no prior factorize, a negative count, partial overlap. */
int cse_sparse_cholesky_solve(cse_evaluator* ev, const double* d_rhs, double* d_x,
                              int32_t max_num_refinement_iterations);

/* Waits on the stream; 0 after a success, else 1 + the smallest permuted
 * scalar column whose pivot failed: a column fed NaN by a failed descendant
 * has a larger index than that descendant, so this is what a sequential
 * factorization in the permuted order reports.  A later factorize starts again
 * from 0.  CSE_ERR_INVALID before any factorize. */
int cse_sparse_cholesky_info(cse_evaluator* ev, int32_t* info);

/* ---- One host solve, several GPUs --------------------------------------
 * The reference evaluates on one device (ContextImpl's single stream,
 * include/ceres/internal/cuda_buffer.h:98) and Ceres' host solve calls one
 * RegisteredCUDAEvaluators::Evaluate with host pointers
 * (include/ceres/internal/registered_cuda_evaluators.h:75-79).
 * cse_create_multi builds such an evaluator over several devices (SURVEY.md
 * §8(b) "device list", §8(e)): the residual blocks are cut into num_devices
 * contiguous shards at point-bucket boundaries (a block whose last parameter
 * block differs from the previous block's; multiples of 4 blocks where
 * possible), each shard is evaluated on devices[k] (repeats allowed: several
 * shards on one device) holding only the parameter blocks its residual blocks
 * use (a BAL shard: every camera it sees plus its own point slice), and
 * cse_evaluate on the returned handle
 *   - copies each shard's slices of the state to its device (only those
 *     slices: cse_shard_transfer_bytes);
 *   - copies each shard's residual and Jacobian-value strips straight into
 *     disjoint regions of the caller's one residuals / jacobian_values
 *     buffers, concurrently per device when the buffers are page-locked
 *     (cse_host_register, or the caller's own hipHostMalloc), synchronously
 *     otherwise -- the library never pins a caller buffer by itself;
 *   - sums the cost and the gradient over the shards in shard order on the
 *     host (deterministic; a parameter block used by several shards, e.g. a
 *     camera, gets the sum of their rows).
 * On an error every copy already queued is finished before the call returns.
 * options->use_stream and options->stream must be 0 (each device gets its
 * own stream).  On such a handle cse_evaluate, cse_wait (returns CSE_OK),
 * cse_plus, cse_set_plus_jacobians, cse_get_info (sizes of the whole
 * problem; bytes summed over the shards), cse_kernel_stats (the slowest
 * shard), cse_shard_info, cse_shard_transfer_bytes and cse_destroy work; the
 * device-pointer entry points return CSE_ERR_UNSUPPORTED. */
int cse_create_multi(const cse_problem_desc* desc, const cse_options* options,
                     const int32_t* devices, int32_t num_devices, cse_evaluator** out);

/* The shards of an evaluator: *num_shards; first_block[num_shards + 1] (may be
 * NULL) = the residual-block ranges [first_block[k], first_block[k+1]);
 * devices[num_shards] (may be NULL).  A cse_create evaluator has one shard. */
int cse_shard_info(cse_evaluator* ev, int32_t* num_shards, int64_t* first_block,
                   int32_t* devices);

/* Bytes one cse_evaluate moves per shard: state_h2d_bytes[num_shards] (the
 * state slices the shard's device receives), strips_d2h_bytes[num_shards]
 * (its residual and Jacobian-value strips); either may be NULL.  A cse_create
 * evaluator has one shard (the whole state and outputs). */
int cse_shard_transfer_bytes(cse_evaluator* ev, int64_t* state_h2d_bytes,
                             int64_t* strips_d2h_bytes);

/* Page-locks [p, p + bytes) of the caller's memory (hipHostRegister) for
 * asynchronous copies until cse_host_unregister(p) with the same p; the
 * multi-device evaluator then copies state slices and strips to and from
 * buffers inside the range without staging.  The caller owns the range:
 * unregister before freeing it.  (The reference pins inside its ContextImpl
 * buffers, include/ceres/internal/cuda_buffer.h:98; here the caller's Ceres
 * arrays are the transfer buffers.) */
int cse_host_register(void* p, size_t bytes);
int cse_host_unregister(void* p);

void cse_destroy(cse_evaluator* ev);

/* Thread-local description of the last error. */
const char* cse_last_error(void);

typedef struct cse_info {
  int64_t num_residual_blocks;
  int64_t num_residuals;
  int64_t num_parameters;
  int64_t num_effective_parameters;
  int64_t num_jacobian_values;
  int32_t num_groups;
  int32_t num_affine_groups;  /* groups on the table-free fast path */
  int32_t device;
  int32_t num_fused_gradient_groups; /* groups whose gradient is fused into the
                                        evaluation (options.gradient_mode 0) */
  /* Compulsory HBM bytes of one residual+Jacobian evaluation (SURVEY.md
   * §8(d)): per block functor data + parameter ids + residuals + Jacobian
   * values, plus each distinct parameter block read once. */
  int64_t bytes_jacobian_eval;
  int64_t bytes_residual_eval; /* same without the Jacobian values */
} cse_info;

int cse_get_info(cse_evaluator* ev, cse_info* info);

/* Kernel time of the evaluate kernels (HIP events on the evaluator's
 * stream, needs options.profile): last launch and running totals. */
int cse_kernel_stats(cse_evaluator* ev, double* last_ms, double* total_ms,
                     int64_t* launches);
int cse_reset_kernel_stats(cse_evaluator* ev);

/* Host-side layout builders for callers that do not have Ceres' writers
 * (restating internal/ceres/block_jacobian_writer.cc:62-160 and
 * compressed_row_jacobian_writer.cc:93-193,240-300).
 *
 * Inputs: parameter blocks (program order) and, per residual block in
 * program order, its parameter block ids (CSR: param_begin[nrb+1]) and
 * residual count.  Outputs the residual layout, per-residual layout and
 * offsets (sized by the *_count queries) and the value count.  For CRS,
 * crs_rows[num_residuals+1] and crs_cols[num_values] are optional. */
int cse_block_sparse_layout(int64_t num_parameter_blocks,
                            const cse_parameter_block* parameter_blocks,
                            int64_t num_residual_blocks, const int64_t* param_begin,
                            const int32_t* param_ids, const int32_t* num_residuals,
                            int64_t num_eliminate_blocks, int64_t* residual_layout,
                            int64_t* jacobian_per_residual_layout,
                            int64_t* jacobian_per_residual_offsets,
                            int64_t* num_jacobian_values);
int cse_compressed_row_layout(int64_t num_parameter_blocks,
                              const cse_parameter_block* parameter_blocks,
                              int64_t num_residual_blocks, const int64_t* param_begin,
                              const int32_t* param_ids, const int32_t* num_residuals,
                              int64_t* residual_layout,
                              int64_t* jacobian_per_residual_layout,
                              int64_t* jacobian_per_residual_offsets,
                              int64_t* num_jacobian_values, int64_t* crs_rows,
                              int64_t* crs_cols);
/* Number of jacobian_per_residual_offsets entries for either layout. */
int64_t cse_layout_offsets_count(int64_t num_parameter_blocks,
                                 const cse_parameter_block* parameter_blocks,
                                 int64_t num_residual_blocks, const int64_t* param_begin,
                                 const int32_t* param_ids, const int32_t* num_residuals);

/* Library identification: ABI version and the gfx target it was built for. */
int cse_abi_version(void);
const char* cse_build_info(void);

#ifdef __cplusplus
}
#endif

#endif /* CSE_H_ */
