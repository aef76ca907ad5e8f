/*
 * ilqr_amd.h -- C ABI of libilqr_amd.so, the MI355X-native batched iLQR hot path.
 *
 * This is the drop-in boundary for the hot path of kazuotani14/iLQR ("the reference"):
 * forward rollout, finite-difference derivatives, backward Riccati recursion with the
 * per-timestep box-QP, and the line search / lambda schedule that strings them together,
 * for B independent trajectories at once.  Every entry point names the reference interface
 * (file:line, relative to the reference repository) it replaces.  The reference has no FFI
 * of its own (it is one C++ process); INTEGRATION.md shows the few-line binding that routes
 * class iLQR through this library.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; nothing is thrown across the boundary.
 *     Every function returns 0 on success or a negative ilqr_status_code; ilqr_last_error()
 *     gives the message of the calling thread's last failure.
 *   - T is the number of transitions (= u0.size(), src/ilqr_core.cpp:12); state arrays have
 *     T+1 knot points.  "acrobot T=500" of BASELINE.json is T = 499 here (500 knots).
 *   - Host-side array layouts ("canonical"), all double (also for fp32 handles), row-major over the leading indices:
 *         x0 [B][nx]          u0,us,k [B][T][nu]        xs [B][T+1][nx]
 *         K  [B][T][nu*nx]    each K_t column-major nu x nx  (Eigen MatrixXd default)
 *         fx,cxx [B][T+1][nx*nx]   fu,cxu [B][T+1][nx*nu]   cuu [B][T+1][nu*nu]   (column-major)
 *         cx [B][T+1][nx]     cu [B][T+1][nu]
 *     so that a dump of the reference's std::vector<VectorXd/MatrixXd> members compares
 *     element for element.  Device-side storage is private to the handle.
 *   - All work is enqueued on the handle's HIP stream; getters synchronise that stream.
 *   - A handle is independent of every other handle (the reference's file-static
 *     lambda/dlambda, include/ilqr.h:17-18, are per-trajectory state here, reset to (1,1) by
 *     ilqr_init_traj -- i.e. each fresh solve behaves like a fresh reference process).
 *   - There is no CPU fallback: without a HIP device ilqr_create fails with ILQR_ERR_NO_DEVICE.
 *     A descriptor ilqr_create refuses is refused before any device is looked for, with its own code.
 */
#ifndef ILQR_AMD_H_
#define ILQR_AMD_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ILQR_AMD_ABI_VERSION 6 /* 2: ilqr_desc.dtype; 3: ILQR_MODEL_USER, ilqr_desc.user_params; 4: ilqr_desc.route, assume_cus (the library reads no environment);
                                  5: results into device memory / in one asynchronous call (ilqr_copy_trajectory_to_device, ilqr_copy_gains_to_device,
                                     ilqr_get_results_async, ilqr_host_register); route bit 128 (ILQR_ROUTE_BACKWARD_LDS, round 1's LDS kernel) retired;
                                  6: receding-horizon steps on the device (ilqr_shift_horizon, ilqr_mpc_step, ilqr_copy_controls_to_device).  ilqr_desc
                                     is unchanged: ilqr_create accepts abi_version 5 as well */

typedef struct ilqr_batch ilqr_batch; /* opaque: owns all device memory of one batch */

enum ilqr_status_code {
  ILQR_OK = 0,
  ILQR_ERR_INVALID = -1,   /* bad argument / size mismatch (the reference asserts: boxqp.cpp:29-33, ilqr_core.cpp:66,80-82) */
  ILQR_ERR_NO_DEVICE = -2, /* no HIP device / runtime failure at create */
  ILQR_ERR_HIP = -3,       /* a HIP call failed; see ilqr_last_error() */
  ILQR_ERR_STATE = -4,     /* call order violated (e.g. warm start before any solve, ilqr_core.cpp:66) */
  ILQR_ERR_UNSUPPORTED = -5
};

/* Device models: compile-time twins of the reference's Model subclasses (include/model.h:6-21).
 * A Model whose dynamics/cost exist only as host virtuals uses ILQR_MODEL_HOST: its rollouts and
 * finite differences stay with the caller (the C++ facade does it), the rest runs here. */
enum ilqr_model_id {
  ILQR_MODEL_ACROBOT = 0,           /* include/acrobot.h            nx=4 nu=1 */
  ILQR_MODEL_DOUBLE_INTEGRATOR = 1, /* include/double_integrator.h  nx=4 nu=2 */
  ILQR_MODEL_LQ = 2,                /* synthetic LQ (BASELINE.json configs[4]): xdot = A x + B u, cost .5(x'Qx + u'Ru),
                                       final .5 x'Qf x, nx<=32 nu<=32 (more than 16: generic thread-per-rollout and point-by-point kernels, fp64); device twin, runs end to end (lq_* of the desc);
                                       fp32 up to nu = 16 (the search then runs the thread-per-rollout kernel: the matrix-core one is fp64) */
  ILQR_MODEL_HOST = 3,              /* a Model that exists only as host code, nx<=32 nu<=32 (at exactly 32 free controls the box-QP factors
                                       with Eigen's UNBLOCKED LLT, as below 32; Eigen 3.3.4 itself switches to its blocked LLT there: rounding,
                                       and the partial factor of an indefinite block, may differ from the reference's): the caller evaluates its
                                       rollouts and finite differences (ilqr_set_trajectory, ilqr_set_derivatives,
                                       ilqr_accept_candidates), the backward pass / box-QPs / accept logic run on the
                                       device; rollout and finite-difference entry points return ILQR_ERR_UNSUPPORTED */
  ILQR_MODEL_USER = 4               /* the caller's OWN device twin (nx<=32 nu<=32; nx = 4 with nu in {1,2} runs every kernel of the
                                       nx = 4 path, both dtypes; other sizes the generic kernels, both dtypes up to nu = 16), compiled into a build of this
                                       library from a header that is not part of it: -DILQR_USER_MODEL_HEADER='"file.hpp"'
                                       (ilqr_amd/csrc/models.hpp states the contract, INTEGRATION.md 5 the recipe).  A build without such a header
                                       answers ILQR_ERR_UNSUPPORTED; ilqr_has_user_model() tells which one is loaded. */
};

/* Arithmetic of the device models (BASELINE.json configs[3] asks for fp32; the reference is fp64 only).
 * ILQR_DTYPE_F32 (acrobot, double integrator): every per-knot quantity -- states, controls, gains, derivative
 * records, the Riccati recursion and the box-QP -- is stored and computed in float; the per-trajectory
 * scalars (cost, dV, gradient norm, lambda) stay double, and the finite differences are taken in double
 * from the float knot (eps = 1e-3 second differences of an O(1e3) cost are pure rounding noise in float)
 * and rounded to float when stored.  The ABI's arrays are double in both modes; the conversion happens on
 * the device when they are packed into / unpacked from the handle's layout.
 * ILQR_DTYPE_F32 on the generic path (ILQR_MODEL_LQ and ILQR_MODEL_USER of other sizes, nu <= 16): the same storage, the rollouts
 * in float; the finite differences, exact derivatives and the whole backward pass in double on the widened float values, the results
 * rounded when stored.  Not with ILQR_MODEL_HOST, ILQR_ROUTE_BACKWARD_W2 or ILQR_ROUTE_TWO_CONTROL_TILES (ILQR_ERR_UNSUPPORTED). */
enum ilqr_dtype { ILQR_DTYPE_F64 = 0, ILQR_DTYPE_F32 = 1 };

/* where a trajectory's outer loop stands (src/ilqr_core.cpp:103-288) */
enum ilqr_traj_status {
  ILQR_RUNNING = 0,
  ILQR_CONVERGED_GRAD = 1, /* "SUCCESS: gradient norm < tolGrad", ilqr_core.cpp:154-159 */
  ILQR_CONVERGED_COST = 2, /* "SUCCESS: cost change < tolFun",   ilqr_core.cpp:257-262 */
  ILQR_LAMBDA_MAX = 3,     /* "EXIT: lambda > lambdaMax",         ilqr_core.cpp:276-281 */
  ILQR_MAX_ITER = 4        /* maxIter iterations done,            ilqr_core.cpp:103 */
};

enum ilqr_flags {
  /* Bench mode: every iteration runs derivatives + backward + all line-search rollouts for
   * every trajectory and the three termination tests are disabled, so B*T*iters is exactly the
   * work done.  Accept/reject and the lambda schedule stay as in the reference. */
  ILQR_FLAG_FIXED_WORK = 1,
  /* Backward-pass kernel of the stage call ilqr_backward_pass and of the two-kernel route (nx = 4 models; see
   * DESIGN.md): the default is four lanes per trajectory; this flag selects one thread per trajectory (the cross-check).
   * (4 was an experiment kernel of round 2 and is ignored.) */
  ILQR_FLAG_BACKWARD_THREAD_PER_TRAJ = 2,
  /* ilqr_iterate / ilqr_solve normally run the derivative sweep and the backward pass of an
   * iteration in one kernel (nx = 4 models: the sweep uses the SIMDs the backward pass leaves
   * idle).  This flag launches them as two kernels, as the stage calls do.  Same results. */
  ILQR_FLAG_UNFUSED = 8,
  /* Opt-in (the reference has nothing like it): the derivative sweep takes the device
   * model's exact derivatives of the Euler map and of the costs instead of eps = 1e-3 central
   * differences.  Results then differ from the reference's by its finite differences' truncation and
   * rounding error (~1e-6 relative on the records), so parity claims are made WITHOUT this flag. */
  ILQR_FLAG_ANALYTIC_DERIVATIVES = 16,
  /* ilqr_iterate / ilqr_solve normally run whole iterations of a 16-trajectory tile in ONE persistent kernel
   * (batches of up to 16 x #CU trajectories of an nx = 4 model: tiles never wait for each other).  This flag
   * launches the stages of every iteration as kernels of their own instead (fused sweep + backward, then
   * rollouts + accept), as larger batches do.  Same results bit for bit. */
  ILQR_FLAG_STAGED = 32,
  /* Opt-in, OFF by default because it changes results: two things the reference's own
   * comments call for.  (1) The rollout clamps every control into [u_min, u_max] and stores / integrates the
   * clamped one -- src/ilqr_core.cpp:327-329, "This is the right way" (the reference adds K (x - xs) to the
   * box-QP's clamped feed-forward without re-clamping, README.md:9 "control-limited part not working").
   * (2) A failed Cholesky factorisation of Quu on the free subspace ends the box-QP with result -1 and the
   * backward pass reports divergence at that step (lambda is raised) -- src/boxqp.cpp:85-88 never looks at
   * info() and goes on with the partial factor.  Every model: the nx = 4 device models, the generic twins, and host-evaluated
   * models (ILQR_MODEL_HOST: (2) on the device; (1) is applied by whoever rolls out -- the C++ facade's host rollouts clamp
   * under this flag).  The CPU oracle has the same switch. */
  ILQR_FLAG_REFERENCE_FIXES = 64,
  /* Opt-in, OFF by default (third part of SURVEY.md 8f-4): lambda regularises the value Hessian instead of Quu --
   * [Tassa 2012] eq. 10a/10b, Quu_reg = cuu + fu'(Vxx' + lambda I) fu, Qux_reg = cxu' + fu'(Vxx' + lambda I) fx --
   * where the reference adds lambda I to Quu and notes "regularization is different" (src/ilqr_core.cpp:365-367).
   * The value update keeps the unregularised Quu, Qux as in the reference.  Every model: the nx = 4 kernels, the
   * tiled kernels of a small twin, and k_backward_w3 on the generic path (n <= 32, m <= 16; host-evaluated models
   * included: the backward pass is what they run on the device) -- not with ILQR_ROUTE_BACKWARD_W2, nor with more than
   * 16 controls (ILQR_ERR_UNSUPPORTED). */
  ILQR_FLAG_REGULARIZE_VXX = 128
};

/* Solver tunables = the compile-time constants of include/ilqr.h:14-24 (defaults shown). */
typedef struct ilqr_params {
  int max_iter;          /* 100   maxIter */
  double tol_fun;        /* 1e-6  tolFun */
  double tol_grad;       /* 1e-6  tolGrad */
  double lambda_init;    /* 1     lambda */
  double dlambda_init;   /* 1     dlambda */
  double lambda_factor;  /* 1.6   lambdaFactor */
  double lambda_max;     /* 1e11  lambdaMax */
  double lambda_min;     /* 1e-8  lambdaMin */
  double z_min;          /* 0     zMin */
} ilqr_params;

typedef struct ilqr_desc {
  int abi_version; /* ILQR_AMD_ABI_VERSION */
  int model;       /* enum ilqr_model_id */
  int nx, nu;      /* Model::x_dims, Model::u_dims (include/model.h:19-20) */
  int T;           /* transitions */
  int B;           /* trajectories in this batch (this rank's shard) */
  double dt;       /* iLQR::dt, include/ilqr.h:30 */
  int device;      /* HIP device ordinal */
  int flags;       /* enum ilqr_flags */
  int dtype;       /* enum ilqr_dtype; 0 = fp64, the reference's arithmetic */
  const double* u_min; /* [nu] Model::u_min (include/model.h:17); NULL = the model's default */
  const double* u_max; /* [nu] */
  const double* goal;  /* [nx] DoubleIntegrator(goal) (double_integrator.h:14); NULL = (1,.5,0,0); acrobot ignores it */
  const double *lq_A, *lq_B, *lq_Q, *lq_R, *lq_Qf; /* ILQR_MODEL_LQ: row-major [nx][nx],[nx][nu],[nx][nx],[nu][nu],[nx][nx] */
  void* stream;             /* hipStream_t to enqueue on; NULL = the library creates one */
  const ilqr_params* params; /* NULL = reference defaults */
  const double* user_params; /* ILQR_MODEL_USER: [n_user_params] handed to UserModelT::set_params (its constructor's arguments) */
  int n_user_params;
  int route;       /* enum ilqr_route bits; 0 = the library picks the kernels by batch size (what every caller wants) */
  int assume_cus;  /* 0 = the device's CU count; > 0: choose routes as if the device had this many (the tests exercise the
                      batch-size thresholds on small batches) */
} ilqr_desc;

/* Which of several equivalent kernels a handle uses.  Every choice leaves the same bits (tests/test_gpu_fused_sweep.py,
 * scripts/soak.py): these exist for A/B measurements and for those tests.  The library reads NO environment variables. */
enum ilqr_route {
  /* What ILQR_ROUTE_AUTO means for the arithmetic: on the nx = 4 path every route computes every element by the same expression in the
   * same order (bit-identical, tests/test_gpu_fused_sweep.py).  On the GENERIC path (n <= 32, m <= 16: LQ model, larger user twins,
   * host-evaluated models; 16 < m <= 32: host-evaluated models, on k_backward_w3 with two control tiles and the literal box-QP in every step) the default backward kernel k_backward_w3 does NOT follow the reference's operation order: the box-QP's
   * inverse comes from a Newton-Schulz refinement of the previous knot's inverse (the literal Cholesky of src/boxqp.cpp:80-119 is its
   * fallback), the upper Vxx tile is the transpose of the lower one, matrix-vector products are per-lane sums.  Its gains equal the
   * reference-order kernel's and the oracle's to rounding (1e-9 on well-conditioned steps; the 1e-6 per-knot tolerance is what is
   * tested), and where fp64 itself does not determine a pass (an indefinite Quu) only its discrete outcome.  The kernel that keeps
   * the reference's order of operations, bit for bit what round 1's LDS kernel computed, is opt-in: ILQR_ROUTE_BACKWARD_W2. */
  ILQR_ROUTE_AUTO = 0,
  ILQR_ROUTE_TILE_PER_CU = 1,       /* ilqr_iterate: persistent 16-trajectory tiles, one per CU (k_solve_hex for m = 1 without opt-in fixes, else k_solve_tile<..,1>) */
  ILQR_ROUTE_TWO_TILES_PER_CU = 2,  /* ... two per CU (k_solve_tile<..,2>; with ILQR_FLAG_STAGED the one-producer k_sweep_backward) */
  ILQR_ROUTE_WIDE_TILES = 3,        /* ... 64-trajectory wide tiles (k_solve_wide / k_solve_wide2; m <= 2 without opt-in fixes, else as 2) */
  ILQR_ROUTE_WIDE_ONE_PER_CU = 4,   /* wide tiles: one per CU whatever the batch size */
  ILQR_ROUTE_WIDE_TWO_PER_CU = 8,   /* wide tiles (m = 1, k_solve_wide): two per CU whatever the batch size.  The m = 2 wide tiles (k_solve_wide2) always run
                                       one per CU: ilqr_create answers ILQR_ERR_UNSUPPORTED to this bit on an nx = 4, nu = 2 handle */
  ILQR_ROUTE_NO_COMPACTION = 16,    /* ilqr_generate_trajectory without re-packing running trajectories between chunks */
  ILQR_ROUTE_FULL_RECORDS = 32,     /* LQ model, exact derivatives: whole per-knot records instead of one shared copy of the constant blocks */
  ILQR_ROUTE_LQ_THREAD_ROLLOUT = 64,/* LQ model: thread-per-rollout k_rollout_g instead of the matrix-core k_rollout_lq */
  /* (128 was ILQR_ROUTE_BACKWARD_LDS, round 1's LDS kernel k_backward_w: retired in ABI 5 -- ILQR_ROUTE_BACKWARD_W2 gives the same bits;
   *  ilqr_create answers ILQR_ERR_UNSUPPORTED to the bit) */
  ILQR_ROUTE_QUAD_CHAIN = 256,      /* one tile per CU: the 4-lane DPP chain (k_solve_tile<..,1>) also where the matrix-core chains (k_solve_hex: m = 1, no opt-in fixes) would run */
  ILQR_ROUTE_LQ_RECOMMIT = 512,     /* LQ model: no candidate buffers (11 x the nominal trajectory); the accepted rollout is run again to commit it */
  ILQR_ROUTE_LQ_DENSE_FD = 2048,    /* LQ model, finite differences: every perturbed point's quadratic forms evaluated densely on the matrix cores
                                       (k_derivatives_g) instead of by what moved (k_derivatives_lq: Q p = Q x + delta_i Q[:,i] + delta_j Q[:,j]) */
  ILQR_ROUTE_WAVE_PER_TRAJECTORY = 4096, /* a small user twin (even nx <= 8, nu <= 4): the generic wavefront-per-trajectory kernels instead of the tiled
                                            thread-per-trajectory ones it runs in by default (cross-check of the tiled kernels; fp64 only,
                                            although the generic kernels have an fp32 mode for the twins that have no tiled kernels) */
  ILQR_ROUTE_BACKWARD_W2 = 1024,    /* generic path: round 2's register kernel k_backward_w2 (literal Cholesky in every box-QP, per-knot cx / cu records)
                                       instead of k_backward_w3 (matrix-core refinement of the previous knot's inverse; LQ model with exact
                                       derivatives: no record array at all) */
  ILQR_ROUTE_TWO_CONTROL_TILES = 8192 /* generic path, nu <= 16: the backward kernel of 16 < nu <= 32, k_backward_w3 with two 16-column control
                                       tiles and the literal box-QP in every step (stage name k_backward_w3w), instead of its one-tile step
                                       (cross-check; not with ILQR_ROUTE_BACKWARD_W2 or ILQR_FLAG_REGULARIZE_VXX) */
};

const char* ilqr_last_error(void);
int ilqr_abi_version(void);
int ilqr_has_user_model(void); /* 1 if this build carries a user device model (ILQR_MODEL_USER), else 0 */
void ilqr_default_params(ilqr_params* p);

/* iLQR::iLQR(Model*, double), include/ilqr.h:30-44 */
int ilqr_create(const ilqr_desc* desc, ilqr_batch** out);
void ilqr_destroy(ilqr_batch* h);
int ilqr_set_stream(ilqr_batch* h, void* hip_stream);
int ilqr_synchronize(ilqr_batch* h);

/* ---- whole-solve entry points ------------------------------------------------------------ */
/* iLQR::init_traj(x0,u0), src/ilqr_core.cpp:11-56: open-loop rollout, zero all derivative and
 * gain arrays, lambda=dlambda=initial.  cost_out [B] may be NULL. */
int ilqr_init_traj(ilqr_batch* h, const double* x0, const double* u0, double* cost_out);
/* iLQR::generate_trajectory(), src/ilqr_core.cpp:79-302, on the state left by init_traj /
 * previous calls.  Runs until every trajectory has left its loop (max_iter each). */
int ilqr_generate_trajectory(ilqr_batch* h);
/* iLQR::generate_trajectory(x0,u0), src/ilqr_core.cpp:59-62 (= BASELINE.json's "iLQR::solve()") */
int ilqr_solve(ilqr_batch* h, const double* x0, const double* u0);
/* iLQR::generate_trajectory(x0) (warm start), src/ilqr_core.cpp:65-76: re-roll the stored
 * controls with the stored gains from new x0 [B][nx]; lambda/dlambda persist as in the reference. */
int ilqr_warm_start(ilqr_batch* h, const double* x0);
/* n_iters bodies of the outer for-loop (src/ilqr_core.cpp:103-288) for every trajectory that
 * is still running; asynchronous (no host synchronisation inside). */
int ilqr_iterate(ilqr_batch* h, int n_iters);

/* ---- model-predictive control on the device (ABI 6) ------------------------------------------------------------------------------
 * A receding-horizon loop whose state never leaves the GPU: advance the stored nominal by `shift` control periods, warm-start it from the
 * new state and run a fixed budget of iterations, then read the next controls into device memory.  Every call is enqueued on the handle's
 * stream and returns without waiting for it: a caller whose x0 comes from, or whose controls go to, work on another stream (a simulator in
 * torch) hands that stream to ilqr_desc.stream / ilqr_set_stream, and stream order does the rest.
 *
 * What the shift does to every trajectory's stored nominal (s = shift, T transitions; knots t < T - s of us / k / K and t <= T - s of xs
 * take the values s knots later):
 *     array   tail knots, ILQR_TAIL_HOLD    tail knots, ILQR_TAIL_ZERO
 *     us      us[T-1]                       0
 *     K       K[T-1]                        0
 *     k       0                             0          (the next backward pass's box-QP warm start)
 *     xs      xs[T]                         xs[T]
 * so that HOLD keeps the final gain around the final state.  Cost, lambda, status and iteration counts are not touched; an accepted candidate
 * still waiting to be copied into xs / us is copied first, and the candidate buffers belong to nobody afterwards (ilqr_get_candidate:
 * ILQR_ERR_STATE). */
enum ilqr_tail { ILQR_TAIL_HOLD = 0, ILQR_TAIL_ZERO = 1 };
/* Shift every trajectory's stored nominal (xs, us, k, K) by `shift` knots, 0 <= shift < T, in place (shift = 0 changes nothing).  Any handle
 * that stores a trajectory, host-evaluated models included.  ILQR_ERR_STATE before ilqr_init_traj / ilqr_set_trajectory. */
int ilqr_shift_horizon(ilqr_batch* h, int shift, int tail);
/* One receding-horizon step: ilqr_shift_horizon(shift, tail), then x0, then the warm start's rollout (u = us[t] + K[t](x - xs[t])) written
 * into xs / us, then a new outer loop (status, iteration counts and flgChange restart; lambda and dlambda persist), then n_iters iterations
 * (ilqr_iterate; n_iters = 0 stops after the warm start's rollout).  It leaves bit for bit the state that shifting on the host,
 * ilqr_set_trajectory + ilqr_set_gains and ilqr_warm_start(x0) on a handle with params.max_iter = n_iters leave (status and iteration
 * counts too when this handle's own max_iter is n_iters), with no host synchronisation: no wait for x0, no wait per chunk, no
 * compaction of finished trajectories.  Exactly one of x0 (host, [B][nx] double) and x0_device (device memory of this handle's device,
 * [B][nx] double) is non-NULL.  A host x0 is the call's one host-to-device transfer: from page-locked memory (ilqr_host_register) it is
 * asynchronous -- the array must then stay unchanged until the stream has passed the step -- from pageable memory the runtime may wait
 * to stage it.  ILQR_ERR_UNSUPPORTED for ILQR_MODEL_HOST (its rollouts are the caller's, as for ilqr_warm_start).
 * The warm rollout is committed unconditionally, also when it is not finite: a trajectory whose rollout overflowed (a new x0 far from the
 * nominal under explicit Euler) holds NaN or inf in xs, us and cost from then on, and no later step of this call repairs it --
 * ilqr_mpc_step_reset below does, on the device. */
int ilqr_mpc_step(ilqr_batch* h, const double* x0, const void* x0_device, int shift, int tail, int n_iters);
/* us[:, t0 : t0 + n_knots, :] as canonical double [B][n_knots][nu] into caller-owned device memory, on the handle's stream (the controls to
 * apply: t0 = 0, n_knots = the shift of the next step).  The window lies inside [0, T) and holds at least one knot. */
int ilqr_copy_controls_to_device(ilqr_batch* h, int t0, int n_knots, void* u_device);

/* ---- single trajectories start over inside the loop (additive under ABI 6) ---------------------------------------------------------
 * In a batch of simulated environments episodes end one by one, and a warm rollout that overflows once poisons its trajectory for good.
 * These calls reset SELECTED trajectories on the device, enqueued on the handle's stream like the step itself; a trajectory that is not
 * selected keeps its bits.  Resetting trajectory b means:
 *     us[b]  = the reset controls of b (ilqr_set_reset_controls; zeros by default), rounded to the handle's storage type
 *     k[b] = 0, K[b] = 0
 *     xs[b]  = 0      (a finite placeholder: with K = 0 the next rollout computes u = us[t] exactly and overwrites xs)
 *     lambda[b] = params.lambda_init, dlambda[b] = params.dlambda_init
 *     status running, iterations 0, flgChange 1, alpha index -1, dV = gnorm = 0
 *     cost[b] and the derivative records stay: the next rollout / sweep writes them (ilqr_get_derivatives keeps its meaning)
 * Old values are overwritten, never read.  Masks and flags are int32 [B] in the caller's trajectory order. */
enum ilqr_reset_rule { ILQR_RESET_NONFINITE = 1, ILQR_RESET_LAMBDA_MAX = 2 };                    /* bits of `rules` */
enum ilqr_reset_why { ILQR_WAS_MASKED = 1, ILQR_WAS_NONFINITE = 2, ILQR_WAS_LAMBDA_MAX = 4 };   /* bits of a reset flag */
/* The controls a reset trajectory starts from: canonical double [B][T][nu], host or device (at most one non-NULL; both NULL = back to
 * zeros, the default).  Kept in the handle in the layout and storage type of us (allocated by the first non-NULL call); enqueued, no
 * synchronisation (a host array from page-locked memory stays unchanged until the stream has passed the call). */
int ilqr_set_reset_controls(ilqr_batch* h, const double* u0, const void* u0_device);
/* Reset now, outside a step.  Trajectory b is selected when mask[b] != 0 (mask: int32 [B], host or device, at most one non-NULL, both NULL =
 * rules only), or rules & ILQR_RESET_NONFINITE and cost[b] is NaN or inf, or rules & ILQR_RESET_LAMBDA_MAX and status[b] == ILQR_LAMBDA_MAX.
 * An accepted candidate still waiting to be copied is copied first and the candidate buffers belong to nobody afterwards (as for
 * ilqr_shift_horizon).  Any handle that stores a trajectory, ILQR_MODEL_HOST included.  ILQR_ERR_INVALID: two masks, unknown rule bits;
 * ILQR_ERR_STATE before ilqr_init_traj / ilqr_set_trajectory. */
int ilqr_reset_trajectories(ilqr_batch* h, const int* mask, const void* mask_device, int rules);
/* ilqr_mpc_step with resets, in this order: shift; reset whom the mask or (under ILQR_RESET_LAMBDA_MAX) a lambda_max exit of the previous
 * step selects -- after the shift, so reset controls are not shifted --; x0; the warm rollout, committed; only under ILQR_RESET_NONFINITE:
 * reset every trajectory whose NEW cost is not finite and roll those out again; the new outer loop; n_iters iterations.  It leaves bit
 * for bit what ilqr_shift_horizon, overwriting the selected rows on the host (ilqr_set_trajectory + ilqr_set_gains + ilqr_set_lambda) and
 * ilqr_mpc_step(shift = 0) leave; with no mask and rules = 0, what ilqr_mpc_step leaves.  Same handles and refusals as ilqr_mpc_step, and
 * ILQR_ERR_INVALID for two masks or unknown rule bits.  Which rule when: ILQR_RESET_NONFINITE costs one more selection and rollout per
 * step and is what keeps a loop alive unattended; ILQR_RESET_LAMBDA_MAX suits callers who would rather restart a trajectory from the reset
 * controls than keep its last accepted solution when the regularisation ran out. */
int ilqr_mpc_step_reset(ilqr_batch* h, const double* x0, const void* x0_device, int shift, int tail, int n_iters, const int* mask,
                        const void* mask_device, int rules);
/* Why each trajectory was reset by the LAST of the two calls above (0 = it was not; before any such call: all 0): int32 [B] */
int ilqr_get_reset_flags(ilqr_batch* h, int* flags);                    /* synchronises */
int ilqr_copy_reset_flags_to_device(ilqr_batch* h, void* flags_device); /* enqueued on the handle's stream */

/* ---- multi-start groups: the best trajectory of a group, cloned over the others (additive under ABI 6) ------------------------------
 * iLQR is a local method; the usual remedy on a non-convex problem is several plans per environment (B = environments x plans, a group
 * = G consecutive trajectories), the best of which replaces the others after every step, often with a perturbation added.  These calls
 * do that on the device, enqueued on the handle's stream like the step itself.  Maps and flags are int32 [B] in the caller's trajectory
 * order.  DEFINITION -- trajectory b takes the state of trajectory s = src[b] (b is CLONED) when
 *     0 <= s < B,  s != b,  and the source keeps itself: src[s] == s or src[s] < 0;
 * src[b] < 0 or src[b] == b: b keeps its bits (flag 0); anything else -- src[b] >= B, a source that is itself asked to change -- is REFUSED
 * and b keeps its bits too.  The device is the one judge of a map (a map in device memory cannot be checked without waiting for it), so
 * the same rule holds for a host map.  No source is a destination: the copy runs in place, with no scratch copy.  Cloning b from s means:
 *     x0[b], xs[b], k[b], K[b] = the source's, bit for bit, in the handle's storage type
 *     us[b] = us[s]                                            without du
 *     us[b][t][e] = (storage type)((double)us[s][t][e] + du[b][t][e])      with du: canonical double [B][T][nu] in device memory; rows of
 *                                                               trajectories that are not cloned are not read
 *     cost, lambda, dlambda, dV, gnorm, status, iteration count, alpha index, and the divergence / backward-pass marks = the source's
 *     flgChange[b] = 1: the derivative records stay the slot's own, so the next sweep recomputes them from the copied nominal (the bits
 *                  the source's own records hold) instead of taking the slot's old records for them
 * From then on b is its source: later iterations leave the two identical, bit for bit.  A perturbation du does NOT re-evaluate the stored
 * cost or trajectory: xs, k, K and cost stay the source's, and a caller who perturbs calls ilqr_warm_start or ilqr_mpc_step next (both roll
 * u = us + K(x - xs) out and cost again).  NOT copied, because they belong to the slot: per-trajectory model parameters
 * (ilqr_set_trajectory_params), the reset controls (ilqr_set_reset_controls), and the derivative records -- on the record-keeping generic
 * routes they stay what the slot's own last sweep left (as after a reset or a shift): a caller who wants ilqr_get_derivatives or
 * ilqr_get_value of a cloned trajectory calls ilqr_compute_derivatives first.  An accepted candidate still waiting to be copied is copied
 * first and the candidate buffers belong to nobody afterwards (as for ilqr_shift_horizon).  Any handle that stores a trajectory,
 * ILQR_MODEL_HOST included, both dtypes.  Every refusal happens before anything is enqueued. */
enum ilqr_clone_why { ILQR_WAS_CLONED = 1, ILQR_CLONE_REFUSED = 2 };
/* src[b] = the winner of b's group for every b: the member with the lowest finite cost (a NaN or inf never wins; among equal costs the
 * lowest index; a group without a finite cost maps every member to itself).  group >= 1 divides B.  Exactly one of src (host: synchronises)
 * and src_device (int32 [B] in device memory: enqueued, nothing waited for) is non-NULL.  Reads cost only and changes nothing in the handle.
 * ILQR_ERR_INVALID: both or neither pointer, group < 1, B % group != 0; ILQR_ERR_STATE before ilqr_init_traj / ilqr_set_trajectory. */
int ilqr_select_best(ilqr_batch* h, int group, int* src, void* src_device);
/* Clone by the map src (the definition above).  Exactly one of src (host; copied to a buffer of the handle on the stream) and src_device is
 * non-NULL; du_device may be NULL.  ILQR_ERR_INVALID: both or neither map; ILQR_ERR_STATE before ilqr_init_traj / ilqr_set_trajectory. */
int ilqr_clone_trajectories(ilqr_batch* h, const int* src, const void* src_device, const void* du_device);
/* ilqr_select_best into a buffer of the handle, then ilqr_clone_trajectories by it (the best-of-group map always satisfies the source rule):
 * both enqueued, no host synchronisation.  Refusals as the two calls'. */
int ilqr_clone_best(ilqr_batch* h, int group, const void* du_device);
/* What the LAST clone call did to each trajectory (0 = it kept its bits unasked; before any such call: all 0): int32 [B] */
int ilqr_get_clone_flags(ilqr_batch* h, int* flags);                    /* synchronises */
int ilqr_copy_clone_flags_to_device(ilqr_batch* h, void* flags_device); /* enqueued on the handle's stream */

/* ---- the value model of the stored policy (additive under ABI 6) -------------------------------------------------------------------
 * The reference's backward pass leaves a quadratic cost-to-go model Vx[t], Vxx[t] at every knot beside the gains (members Vx, Vxx;
 * src/ilqr_core.cpp:353-354, 391-393).  The kernels here carry it in registers and drop it; these calls recompute it on the device for a
 * window of knots.  DEFINITION -- from the derivative records ilqr_get_derivatives would return at this moment (see there for which
 * trajectory they describe) and the stored gains k, K:
 *     Vx[T] = cx[T],  Vxx[T] = cxx[T]                                       (as stored: knot T is not symmetrised)
 *     t = T-1 .. 0:   Qx = cx + fx'Vx[t+1],  Qu = cu + fu'Vx[t+1],  Qxx = cxx + fx'Vxx[t+1] fx,  Qux = cxu' + fu'Vxx[t+1] fx,
 *                     Quu = cuu + fu'Vxx[t+1] fu                            (src/ilqr_core.cpp:359-363; Quu without lambda)
 *                     Vx[t]  = Qx  + K'Quu k + K'Qu  + Qux'k
 *                     Vxx[t] = Qxx + K'Quu K + K'Qux + Qux'K,  then (Vxx[t] + Vxx[t]')/2
 * No lambda, no box-QP, no divergence test: a pure function of (records, k, K) -- the value model of the policy the handle STORES, whoever
 * stored it (a backward pass, ilqr_set_gains, a receding-horizon shift).  After ilqr_compute_derivatives + ilqr_backward_pass with
 * diverge == 0 it equals the reference's members to rounding.  The recursion runs in double on every handle (an fp32 handle's stored float
 * records and gains are widened), and the output is canonical double on every handle:
 *     Vx  [B][n_knots][nx]        Vxx [B][n_knots][nx*nx], column-major per knot
 * Only the window [t0, t0 + n_knots) is stored: it lies inside [0, T] and holds at least one knot (V is carried from knot T down to t0;
 * Vx[0] is the gradient of the cost-to-go model in the measured state, Vxx[t] at a late knot a terminal cost for a shorter horizon).
 * Either output may be NULL, not both.  Every model, ILQR_MODEL_HOST included (its records are what the caller set).  The call leaves the
 * handle as ilqr_get_derivatives at the same point does: later iterations are bit for bit those of a handle that called neither.
 * ILQR_ERR_INVALID: a bad window, two NULL outputs; ILQR_ERR_STATE: before ilqr_init_traj / ilqr_set_trajectory. */
/* into host arrays: a window-sized device buffer, copied out; synchronises */
int ilqr_get_value(ilqr_batch* h, int t0, int n_knots, double* Vx, double* Vxx);
/* into caller-owned device memory of this handle's device: enqueued on the handle's stream, not waited for (as ilqr_copy_gains_to_device) */
int ilqr_copy_value_to_device(ilqr_batch* h, int t0, int n_knots, void* Vx_device, void* Vxx_device);

/* ---- the closed-loop covariance of the stored policy (additive under ABI 6) --------------------------------------------------------
 * The forward twin of the value model: how far the closed loop u = us[t] + K[t](x - xs[t]) drifts from the nominal under an uncertain
 * initial state and additive process noise, knot by knot, and what that costs in expectation -- the linear-Gaussian part (the G) of iLQG,
 * which the reference does not have.  DEFINITION -- from the derivative records ilqr_get_derivatives would return at this moment (see
 * there for which trajectory they describe) and the stored gains K; k, us and xs are not read:
 *     Sigma[0] = Sigma0[b]                                                  (as given, not symmetrised; NULL = zero)
 *     t = 0 .. T-1:   A     = fx[t] + fu[t] K[t]
 *                     Z     = Sigma[t] K[t]'                                (n x m)
 *                     Su[t] = sym(K[t] Z)                                   (m x m;  sym(M) = (M + M')/2)
 *                     J    += 1/2 (<cxx[t], Sigma[t]> + <cuu[t], Su[t]> + 2 <cxu[t], Z>)     (<,> = sum of elementwise products)
 *                     Sigma[t+1] = sym(A Sigma[t] A' + W[b])                (W NULL = zero)
 *     J += 1/2 <cxx[T], Sigma[T]>
 * Sigma[t] is the covariance of x[t] - xs[t], Su[t] that of the feedback part of u[t], J the expected cost above the nominal's, to
 * second order.  What this is NOT: it is the covariance of the LINEARISED closed loop about the nominal.  Rows of K that the box-QP
 * zeroed (clamped controls) are in K already, but saturation of the feedback itself is not modelled -- Su[t] beside the control box tells
 * how likely it is.  Noise enters through the state only and is the same at every knot.  A pure function of (records, K, Sigma0, W);
 * by the identity J = 1/2 <Vxx[0], Sigma0> + 1/2 sum_t <Vxx[t+1], W> it agrees with ilqr_get_value.
 * The recursion runs in double on every handle (an fp32 handle's stored float records and gains are widened); every array is canonical
 * double on every handle, matrices column-major:
 *     Sigma0, W [B][nx*nx]     Sigma [B][n_knots][nx*nx]     Su [B][n_knots][nu*nu]     expected_cost [B]
 * Only the window [t0, t0 + n_knots) of Sigma and Su is stored: it lies inside [0, T] and holds at least one knot; with Su requested it
 * lies inside [0, T) (knot T has no control).  The recursion runs from knot 0 to the last knot anything needs: T when expected_cost is
 * requested, else t0 + n_knots - 1.  Any output may be NULL, not all three.  Every model, ILQR_MODEL_HOST included (its records are what
 * the caller set), both dtypes.  The call leaves the handle as ilqr_get_derivatives at the same point does: later iterations are bit for
 * bit those of a handle that never asked.
 * ILQR_ERR_INVALID: a bad window, a window with knot T when Su is requested, three NULL outputs; ILQR_ERR_STATE: before ilqr_init_traj /
 * ilqr_set_trajectory.  Every refusal happens before anything is enqueued. */
/* host arrays: a call-sized device buffer takes Sigma0 / W up and the window down; synchronises */
int ilqr_get_covariance(ilqr_batch* h, int t0, int n_knots, const double* Sigma0, const double* W, double* Sigma, double* Su,
                        double* expected_cost);
/* device memory of this handle's device: enqueued on the handle's stream, nothing waited for (as ilqr_copy_value_to_device) */
int ilqr_copy_covariance_to_device(ilqr_batch* h, int t0, int n_knots, const void* Sigma0_device, const void* W_device, void* Sigma_device,
                                   void* Su_device, void* expected_cost_device);

/* ---- the tangent and the adjoint of the stored closed loop (additive under ABI 6) ----------------------------------------------------
 * The piece under the value, covariance and evaluation calls: the closed loop u = us[t] + K[t](x - xs[t]), linearised about the nominal,
 * as a LINEAR OPERATOR applied to the caller's own vectors in both directions.  The tangent (forward, a Jacobian-vector product) says how
 * a perturbation dx0 of the measured state and perturbations dv[t] of the stored controls move every later state and control; the
 * adjoint (backward, a vector-Jacobian product) takes gx[t] = dL/dxs[t], gu[t] = dL/dus[t] of a caller's scalar loss L to dL/dx0 and
 * dL/dv[t] -- what the backward of an autograd function around ilqr_mpc_step needs.  DEFINITION -- from the derivative records
 * ilqr_get_derivatives would return at this moment (see there for which trajectory they describe) and the stored gains K; k, us, xs,
 * the costs and the cost records are not read.  n_dirs >= 1 independent directions (columns) per trajectory;
 * nku = min(t0 + n_knots, T) - t0 is the number of knots of the window [t0, t0 + n_knots) that have a control.
 *   TANGENT   dx[0] = dx0[b]                                                 (NULL = zero)
 *             t = 0 .. T-1:   du[t]   = K[t] dx[t] + dv[b][t]                (dv NULL = zero)
 *                             dx[t+1] = fx[t] dx[t] + fu[t] du[t]
 *     in:  dx0 [B][n_dirs][nx]           dv  [B][T][n_dirs][nu]    (the whole horizon)
 *     out: dxs [B][n_knots][n_dirs][nx]  dus [B][nku][n_dirs][nu]  (the window only)
 *     The recursion runs from knot 0 to the last knot anything needs.  dx0 and dv both NULL is refused (the answer would be zero), dxs and
 *     dus both NULL is refused, dus non-NULL with nku == 0 is refused (knot T has no control).
 *   ADJOINT   a[t] = 0 for t past the window;  gx, gu = 0 outside the window
 *             t = last .. 0:  w[t] = gu[t] + fu[t]'a[t+1]                                      (t < T)
 *                             a[t] = gx[t] + fx[t]'a[t+1] + K[t]'w[t]                          (a[T] = gx[T])
 *             g_x0 = a[0],   g_v[t] = w[t]
 *     in:  gx [B][n_knots][n_dirs][nx]   gu  [B][nku][n_dirs][nu]  (over the window; NULL = zero)
 *     out: g_x0 [B][n_dirs][nx]          g_v [B][T][n_dirs][nu]    (us-shaped: the knots after the window are WRITTEN as exact zeros, the
 *                                                                   caller's buffer is not assumed cleared)
 *     gx and gu both NULL is refused, gu non-NULL with nku == 0 is refused; either output may be NULL, not both.
 * The two calls are each other's transposes:  sum_t <gx[t], dx[t]> + sum_t <gu[t], du[t]> = <g_x0, dx0> + sum_t <g_v[t], dv[t]>.
 * Per direction a vector; [n_dirs][nx] row-major is an nx x n_dirs column-major matrix: with dx0 = I (n_dirs = nx), dxs[t] is the state
 * transition matrix Phi[t] and dus[t] is K[t] Phi[t], the first-order change of the whole plan with the measured state, both in this
 * header's column-major convention.  With gx = cx, gu = cu the adjoint is the gradient of the trajectory cost in the controls under the
 * stored feedback (and a[t] is ilqr_get_value's Vx[t] when k = 0); with K = 0 the plain open-loop cost gradient.
 * The recursion runs in double on every handle (an fp32 handle's stored float records and gains are widened); every array is canonical
 * double on every handle.  Every model, ILQR_MODEL_HOST included (its records are what the caller set), both dtypes.  The calls are
 * read-only: they leave the handle as ilqr_get_derivatives at the same point does, later iterations are bit for bit those of a handle
 * that never asked.  A window is a slice of the full call, bit for bit (for the adjoint: of the full call with gx, gu zero outside the
 * window).  Column s of every output depends on column s of the inputs only, BIT FOR BIT: a direction computed alone (n_dirs = 1) and
 * the same direction as column 20 of 33 give the same bits.
 * The four arrays of a call do not overlap.
 * What this is NOT: it is the first-order map of the LINEARISED closed loop about the nominal.  Rows of K that the box-QP zeroed are in
 * K already, but saturation of the feedback and the model's second derivatives are not modelled; K Phi is the Gauss-Newton sensitivity
 * of a converged plan, not the exact one.
 * ILQR_ERR_INVALID: null handle, a bad window, n_dirs < 1, B * (T + 1) * n_dirs * max(nx, nu) beyond INT_MAX, the NULL combinations
 * above; ILQR_ERR_STATE: before ilqr_init_traj / ilqr_set_trajectory.  Every refusal happens before anything is enqueued. */
/* host arrays: a call-sized device buffer takes the inputs up and the outputs down; synchronises */
int ilqr_get_tangent(ilqr_batch* h, int t0, int n_knots, int n_dirs, const double* dx0, const double* dv, double* dxs, double* dus);
/* device memory of this handle's device: enqueued on the handle's stream, nothing waited for (as ilqr_copy_covariance_to_device) */
int ilqr_copy_tangent_to_device(ilqr_batch* h, int t0, int n_knots, int n_dirs, const void* dx0_device, const void* dv_device, void* dxs_device,
                                void* dus_device);
int ilqr_get_adjoint(ilqr_batch* h, int t0, int n_knots, int n_dirs, const double* gx, const double* gu, double* g_x0, double* g_v);
int ilqr_copy_adjoint_to_device(ilqr_batch* h, int t0, int n_knots, int n_dirs, const void* gx_device, const void* gu_device, void* g_x0_device,
                                void* g_v_device);

/* ---- the LQ subproblem of the records, solved for caller-given linear terms (additive under ABI 6) -----------------------------------
 * The calls above take the stored gains K as given; this one answers how the OPTIMAL plan moves when the problem moves.  It solves the
 * equality-constrained LQ subproblem the handle holds (fx, fu, cxx, cxu, cuu of the records) for the caller's linear cost terms gx, gu and
 * initial perturbation dx0: the Newton / iLQR step (gx = cx, gu = cu), the backward pass of a differentiable MPC layer (gx = dL/dxs,
 * gu = dL/dus), the first-order re-plan for a shifted goal (gx = -cxx dgoal), the exact LQ response to a measured-state change (dx0 = I).
 * DEFINITION -- from the derivative records ilqr_get_derivatives would return at this moment, and from the stored K ONLY to decide which
 * controls are held.  n_dirs >= 1 independent directions (columns) per trajectory, the whole horizon, no windows.
 *   HELD SET  with ILQR_LQ_HOLD_CLAMPED control e of knot t is held when every element of row e of K[t] is exactly zero (how the box-QP
 *             leaves a clamped control); without the flag nothing is held.  F = the free controls of the knot.
 *   GAINS     P[T] = cxx[T];  t = T-1 .. 0:
 *               Qxx = cxx + fx'P[t+1] fx,   Qux = cxu' + fu'P[t+1] fx,   Quu = cuu + fu'P[t+1] fu + mu I
 *               Quu_FF = L L'   lower Cholesky over F in index order; a pivot <= 0 or not finite ends this trajectory: info[b] = t + 1
 *               Kd_F = -Quu_FF^-1 Qux_F, held rows of Kd zero;   P[t] = sym(Qxx + Qux'Kd)
 *             (a knot with no free control factors nothing and cannot fail)
 *   BACKWARD  per direction:  v[T] = gx[T];   w = gu[t] + fu'v[t+1];   kd_F = -Quu_FF^-1 w_F, held rows zero;
 *                             v[t] = gx[t] + fx'v[t+1] + Kd'w
 *   FORWARD   per direction:  dx[0] = dx0;   du[t] = Kd dx[t] + kd[t];   dx[t+1] = fx dx[t] + fu du[t];   dlam[t] = P[t] dx[t] + v[t]
 *     in:  dx0 [B][n_dirs][nx]   gx [B][T+1][n_dirs][nx]   gu [B][T][n_dirs][nu]        (NULL = zero, not all three)
 *     out: dxs, dlam [B][T+1][n_dirs][nx]   dus [B][T][n_dirs][nu]   info int32 [B]       (any may be NULL, not all of dxs, dus, dlam)
 * For symmetric cxx, cuu, (dxs, dus) minimises  sum_t 1/2 [dx; du]'[cxx cxu; cxu' cuu + mu I][dx; du] + gx'dx + gu'du  subject to the
 * linearised dynamics, dx[0] = dx0 and held controls = 0; dlam holds the multipliers of the dynamics (dlam[T] = cxx[T] dx[T] + gx[T],
 * dlam[t] = gx[t] + cxx dx[t] + cxu du[t] + fx'dlam[t+1]).  info[b] = 0: solved.  A failed trajectory gets quiet NaNs in all of its
 * outputs and changes no other trajectory's bits.  Held dus entries are exact zeros; dxs[:, 0] is dx0 to the bit; column s of every output
 * depends on column s of the inputs only, BIT FOR BIT.  All arithmetic is double on every handle (an fp32 handle's stored floats are
 * widened), every array canonical double.  Every model, ILQR_MODEL_HOST included, both dtypes.  Read-only: later iterations are bit for
 * bit those of a handle that never asked.  The arrays of a call do not overlap.
 * SCRATCH: the handle keeps one device buffer for these calls, allocated by the first call and kept while the next one's fits, of
 *     Bs * (T * (nu * nx + nu * nu) + [dlam asked for] (T + 1) * nx * nx) + [dus NULL] B * T * n_dirs * nu + ceil(Bs / 2)   doubles,
 * Bs = B on the generic layout, B rounded up to 64 on the nx = 4 kernels' layout: Kd, the masked -Quu^-1, P, kd.  At nx = 32, nu = 16,
 * B = 8192, T = 200 that is 10 GB without dlam and 23 GB with it (nu = 32: 27 / 40 GB), next to the 44 GB of records.
 * ILQR_ERR_INVALID: null handle, n_dirs < 1, unknown flag bits, mu negative or not finite, dx0, gx and gu all NULL, dxs, dus and dlam all
 * NULL, B * (T + 1) * n_dirs * max(nx, nu) beyond INT_MAX; ILQR_ERR_STATE: before ilqr_init_traj / ilqr_set_trajectory.  Every refusal
 * happens before anything is enqueued. */
enum ilqr_lq_flags { ILQR_LQ_HOLD_CLAMPED = 1 };
/* host arrays: a call-sized device buffer takes the inputs up and the outputs down; synchronises */
int ilqr_solve_lq(ilqr_batch* h, int n_dirs, int flags, double mu, const double* dx0, const double* gx, const double* gu, double* dxs, double* dus,
                  double* dlam, int* info);
/* device memory of this handle's device: enqueued on the handle's stream, nothing waited for */
int ilqr_solve_lq_on_device(ilqr_batch* h, int n_dirs, int flags, double mu, const void* dx0_device, const void* gx_device, const void* gu_device,
                            void* dxs_device, void* dus_device, void* dlam_device, void* info_device);

/* ---- the Kalman filter of the stored linearisation and the covariance of the output-feedback loop (additive under ABI 6) --------------
 * ilqr_get_covariance answers for a controller that sees the true state.  A real loop measures y = H x + v, v ~ (0, V), and feeds back on
 * an estimate: u = us[t] + K[t](xhat[t] - xs[t]).  These calls give the time-varying Kalman gains L[t] along the stored linearisation, the
 * estimate-error covariances before (Pp) and after (Pf) the measurement of each knot, and the covariance and expected cost of the loop that
 * actually runs -- the other half of iLQG.  DEFINITION -- from the derivative records ilqr_get_derivatives would return at this moment
 * (see there for which trajectory they describe) and the stored gains K; k, us, xs, cx and cu are not read.  ny is the number of measured
 * outputs, 1 <= ny <= nx; sym(M) = (M + M')/2:
 *     Pp[0] = P0[b]                                        (as given, not symmetrised; NULL = zero)
 *     Xh    = 0                                            (covariance of the estimate's deviation from xs; the plan starts at the prior mean)
 *     t = 0 .. T:
 *         S      = sym(H Pp[t] H' + V)                     (ny x ny)
 *         S      = R R'   lower Cholesky in index order; a pivot <= 0 or not finite ends this trajectory: info[b] = t + 1
 *         L[t]   = Pp[t] H' S^-1                           (nx x ny; by forward and back substitution with R, not an explicit inverse)
 *         G      = I - L[t] H
 *         Pf[t]  = sym(G Pp[t] G' + L[t] V L[t]')          (Joseph form)
 *         N      = sym(L[t] S L[t]')
 *         Xh     = sym(N)  if t == 0  else  sym(A Xh A' + N)          (A of the previous knot)
 *         Sigma[t] = Xh + Pf[t]
 *         J     += 1/2 <cxx[t], Sigma[t]>
 *         if t < T:
 *             Z = Xh K[t]',  Su[t] = sym(K[t] Z),  J += 1/2 (<cuu[t], Su[t]> + 2 <cxu[t], Z>)
 *             A = fx[t] + fu[t] K[t]
 *             Pp[t+1] = sym(fx[t] Pf[t] fx[t]' + W)        (W NULL = zero)
 * Pp, Pf and L are the filter and do not depend on K.  Sigma[t] is the covariance of x[t] - xs[t], Su[t] that of the feedback part of
 * u[t], J the expected cost above the nominal's, to second order, when the feedback acts on the filtered estimate.  The estimation error
 * of the optimal filter is orthogonal to the estimate, which is why the covariance of the true state splits into the two n x n recursions
 * Xh and Pf and no 2n x 2n joint covariance is formed.
 * What this is NOT: it is the filter of the LINEARISATION ABOUT THE NOMINAL, not an EKF relinearised at the estimate.  H, W and V are the
 * same at every knot.  Saturation of the feedback is not modelled.  The split Sigma = Xh + Pf holds for the gain L defined here and for no
 * other.
 * Every array is canonical double on every handle, matrices column-major:
 *     in:  H [B][ny*nx] (ny rows)   P0, W [B][nx*nx]   V [B][ny*ny]                                  (H and V are required)
 *     out: Pp, Pf, Sigma [B][n_knots][nx*nx]   L [B][n_knots][nx*ny]   Su [B][n_knots][nu*nu]   expected_cost [B]   info int32 [B]
 * Any output may be NULL, not all of Pp, Pf, L, Sigma, Su and expected_cost.  Only the window [t0, t0 + n_knots) is stored: it lies inside
 * [0, T] and holds at least one knot; with Su requested it lies inside [0, T) (knot T has no control).  The recursion runs from knot 0 to
 * the last knot anything needs: T when expected_cost is requested, else t0 + n_knots - 1.
 * All arithmetic is double on every handle (an fp32 handle's stored floats are widened).  Every model, ILQR_MODEL_HOST included, both
 * dtypes.  Read-only: later iterations are bit for bit those of a handle that never asked.  What is computed at a knot does not depend on
 * which outputs were asked for, only on whether it is computed: a window is a slice of the full call, bit for bit, and Pp, Pf and L have
 * the same bits whether or not Sigma, Su or expected_cost are requested.  Pp[0] is P0 to the bit; Pf, Sigma, Su and Pp[t >= 1] are
 * symmetric to the bit.  A failed trajectory gets quiet NaNs in every output it has, over the whole window, plus its info[b]; it changes no
 * other trajectory's bits (a pivot past the last knot the recursion reaches is not met: info[b] = 0).  The arrays of a call do not overlap.
 * SCRATCH: the handle keeps one device buffer for these calls, allocated by the first call and kept while the next one's fits, of
 *     ceil(B / 2) + [generic layout, and Sigma, Su or expected_cost asked for] 2 * B * (last + 1) * nx * nx   doubles,
 * last the last knot the recursion reaches: the failure marks, and Pf and N of every knot on their way from the filter sweep to the
 * closed-loop sweep (the nx = 4 kernels' layout runs one sweep and keeps them in registers).  At nx = 32, B = 8192, T = 200 with the
 * expected cost that is 27 GB.
 * ILQR_ERR_INVALID: null handle, ny outside [1, nx], NULL H or V, a bad window, a window with knot T when Su is requested, all six outputs
 * NULL, B * (T + 1) * nx * nx beyond INT_MAX; ILQR_ERR_STATE: before ilqr_init_traj / ilqr_set_trajectory.  Every refusal happens before
 * anything is enqueued. */
/* host arrays: a call-sized device buffer takes the inputs up and the window down; synchronises */
int ilqr_get_estimator(ilqr_batch* h, int t0, int n_knots, int ny, const double* H, const double* P0, const double* W, const double* V,
                       double* Pp, double* Pf, double* L, double* Sigma, double* Su, double* expected_cost, int* info);
/* device memory of this handle's device: enqueued on the handle's stream, nothing waited for (as ilqr_copy_covariance_to_device) */
int ilqr_copy_estimator_to_device(ilqr_batch* h, int t0, int n_knots, int ny, const void* H_device, const void* P0_device, const void* W_device,
                                  const void* V_device, void* Pp_device, void* Pf_device, void* L_device, void* Sigma_device, void* Su_device,
                                  void* expected_cost_device, void* info_device);

/* ---- the risk-sensitive (LEQG) gains and value of the stored LQ model (additive under ABI 6) -----------------------------------------
 * Every query above is risk-neutral: noise changes the expected cost they report, never the controller (certainty equivalence: the gains
 * ilqr_solve_lq computes are the same for any W).  These calls give the controller for which the noise matters: (K, k) minimise
 * (1/theta) log E exp(theta J) over feedback policies for the LQ model of the records with full state observation (Jacobson 1973,
 * Whittle 1981; iLEQG: Farshidian and Buchli 2015).  theta > 0 is risk-averse: the saddle point of the game in which a disturbance xi is
 * penalised by |xi|^2 / (2 theta), the soft-constrained H-infinity problem with gamma^2 = 1/theta; its gains are stiffer where the noise
 * hurts and its feed-forward is pessimistic.  theta < 0 is risk-seeking and never breaks down for convex records.  theta = 0 gives the gains
 * ilqr_solve_lq computes internally, with risk_cost the expected cost above the nominal's of the Newton step under the noise.
 * DEFINITION -- the LQ model of the records about the nominal with dx[t+1] = fx dx + fu du + C[b] xi[t], xi ~ N(0, I_nw), 1 <= nw <= nx;
 * W = C C' is the process noise of ilqr_get_covariance (a factor is asked for, not W, so that rank-deficient noise needs no factorisation
 * of a singular W).  From the derivative records ilqr_get_derivatives would return at this moment; the stored K is read only to decide the
 * held set, as in ilqr_solve_lq; k, us, xs are not read.  sym(M) = (M + M')/2; the value at knot t is 1/2 dx'P[t]dx + v[t]'dx + s[t]:
 *     P[T] = cxx[T] (as stored), v[T] = cx[T], s[T] = 0
 *     t = T-1 .. 0, with P = P[t+1], v = v[t+1], s = s[t+1]:
 *         G  = P C                                (nx x nw)
 *         M  = I - theta * sym(C'G)               (nw x nw)
 *         M  = R R'   lower Cholesky in index order; a pivot <= 0 or not finite ends this trajectory: info[b] = -(t + 1)   (breakdown)
 *         Y  = R^-1 G'  (nw x nx),  y = R^-1 (C'v)            forward substitution, no explicit inverse
 *         Pt = P + theta * Y'Y,     vt = v + theta * Y'y
 *         st = s + theta/2 * y'y - (1/theta) * sum_j log R(j,j)          theta != 0
 *         st = s + 1/2 * trace(C'G)                                      theta == 0 exactly
 *         Qx = cx + fx'vt,  Qu = cu + fu'vt,  Qxx = cxx + fx'Pt fx,  Qux = cxu' + fu'Pt fx,  Quu = cuu + fu'Pt fu + mu I
 *         held set as ilqr_solve_lq (ILQR_LQ_HOLD_CLAMPED, the only flag bit: rows of the stored K[t] that are exactly zero); F the rest
 *         Quu_FF = L L'  lower Cholesky over F in index order; a pivot <= 0 or not finite: info[b] = t + 1
 *         K[t]_F = -Quu_FF^-1 Qux_F,  k[t]_F = -Quu_FF^-1 Qu_F,  held rows exact zeros   (a knot with no free control factors nothing)
 *         P[t] = sym(Qxx + Qux'K[t]),  v[t] = Qx + K[t]'Qu,  s[t] = st + 1/2 Qu'k[t]
 *     risk_cost[b] = s[0]
 * BREAKDOWN is an answer, not an error: info[b] < 0 says that the risk-sensitive cost at that theta is infinite -- the chosen risk aversion
 * is more than the plan can bear.  risk_cost loses digits as eps/|theta| for tiny non-zero theta.
 * What this is NOT: it is the LEQG of the LINEARISATION ABOUT THE NOMINAL.  The noise is the same at every knot.  Saturation is not
 * modelled.  Output feedback is not modelled: the LEQG separation through ilqr_get_estimator is not claimed.
 * How it is used: ilqr_set_gains(k, K) installs the result, ilqr_rollout_candidates / ilqr_line_search then take the step, and
 * ilqr_get_covariance and ilqr_evaluate_policy report how the robust gains do.  Installing gains from device memory is out of scope here.
 * Every array is canonical double on every handle, matrices column-major:
 *     in:  C [B][nx*nw] (nx rows; required)
 *     out: K [B][T][nu*nx] (as ilqr_get_gains)   k [B][T][nu]   Vx [B][T+1][nx] = v   Vxx [B][T+1][nx*nx] = P   risk_cost [B]   info int32 [B]
 * The whole horizon, no windows.  Any output may be NULL, not all of K, k, Vx, Vxx and risk_cost.
 * All arithmetic is double on every handle (an fp32 handle's stored floats are widened).  Every model, ILQR_MODEL_HOST included, both
 * dtypes.  Read-only: later iterations are bit for bit those of a handle that never asked.  A failed trajectory gets quiet NaNs in every
 * output it has, over the whole horizon; the sign of info[b] says which factorisation failed; no other trajectory's bits change.  Vxx[t] is
 * symmetric to the bit for t < T; Vxx[T] and Vx[T] are the records' bits; held rows are exact zeros.  Outputs do not depend on which other
 * outputs were requested.  The arrays of a call do not overlap.  The only scratch is B failure marks, kept by the handle.
 * ILQR_ERR_INVALID: null handle, nw outside [1, nx], NULL C, unknown flag bits, mu negative or not finite, theta not finite, all five of
 * K, k, Vx, Vxx and risk_cost NULL, B * (T + 1) * nx * nx beyond INT_MAX; ILQR_ERR_STATE: before ilqr_init_traj / ilqr_set_trajectory.
 * Every refusal happens before anything is enqueued. */
/* host arrays: a call-sized device buffer takes C up and the outputs down; synchronises */
int ilqr_get_risk_sensitive(ilqr_batch* h, int nw, double theta, int flags, double mu, const double* C, double* K, double* k, double* Vx,
                            double* Vxx, double* risk_cost, int* info);
/* device memory of this handle's device: enqueued on the handle's stream, nothing waited for */
int ilqr_copy_risk_sensitive_to_device(ilqr_batch* h, int nw, double theta, int flags, double mu, const void* C_device, void* K_device,
                                       void* k_device, void* Vx_device, void* Vxx_device, void* risk_cost_device, void* info_device);

/* ---- the stored feedback policy applied to caller-given states (additive under ABI 6) -----------------------------------------------
 * What a solve leaves for a controller is the time-varying law u = us[t] + K[t](x - xs[t]).  These calls apply it to states the CALLER
 * holds -- n_samples of them per trajectory, at knot t0 -- and roll it through the handle's device model for n_knots knots; a read-only
 * query: the nominal is read, only the outputs are written.  DEFINITION -- with xs, us, K as ilqr_get_trajectory / ilqr_get_gains would
 * return them at this moment (an accepted candidate still waiting to be copied is copied first), for trajectory b and sample s:
 *     x_{t0} = x[b][s]
 *     t = t0 .. t0 + n_knots - 1:   u_t = us[b][t] + K[b][t](x_t - xs[b][t])          (src/ilqr_core.cpp:316 without alpha k: k is not part of the policy)
 *                                   clamp:  u_t = min(max(u_t, u_min), u_max)         (ILQR_EVAL_CLAMP, or a handle with ILQR_FLAG_REFERENCE_FIXES)
 *                                   cost += model.cost(x_t, u_t),  x_{t+1} = x_t + dt model.dynamics(x_t, u_t)
 *     t0 + n_knots == T:            cost += model.final_cost(x_T)                      (a shorter window carries running costs only)
 *     cost[b][s],   x_end[b][s] = x_{t0 + n_knots},   u_first[b][s] = u_{t0}  (the clamped value under the clamp)
 * The arithmetic is the handle's rollout arithmetic, expression for expression: (t0 = 0, n_knots = T, one sample) gives the bits
 * ilqr_mpc_step(x, shift = 0, n_iters = 0) leaves in cost, xs[T] and us[0].  An fp32 handle rounds x to float where it is loaded, keeps
 * states and controls in float and sums the costs in double.  Every output is canonical double on every handle:
 *     x [B][n_samples][nx]     cost [B][n_samples]     x_end [B][n_samples][nx]     u_first [B][n_samples][nu]
 * Any output may be NULL, not all three.  With per-trajectory parameters set, every sample of trajectory b uses row b.  A rollout that
 * overflows leaves inf or NaN in its own outputs and nothing else.  x0, cost, the candidates, lambda and status are not touched: later
 * iterations are bit for bit those of a handle that never called.  Uses: n_knots = 1 -- u_first is the control for a measured state
 * between re-plans; n_knots = shift -- x_end is a model-based plant's next x0, handed to ilqr_mpc_step(x0_device); n_knots = T - t0 with
 * many samples -- the closed-loop cost of the policy from perturbed states.
 * ILQR_ERR_INVALID: null x, three NULL outputs, a window outside [0, T] or without a knot, n_samples < 1, B * n_samples beyond INT_MAX,
 * unknown flag bits; ILQR_ERR_STATE: before ilqr_init_traj / ilqr_set_trajectory; ILQR_ERR_UNSUPPORTED: ILQR_MODEL_HOST (its model
 * exists on the host only, as for ilqr_warm_start).  Every refusal happens before anything is enqueued. */
enum ilqr_eval_flags { ILQR_EVAL_CLAMP = 1 };
/* host arrays: x goes up into a device buffer of the call's size, the outputs come back from it; synchronises */
int ilqr_evaluate_policy(ilqr_batch* h, int t0, int n_knots, int n_samples, int flags, const double* x, double* cost, double* x_end,
                         double* u_first);
/* device memory of this handle's device: enqueued on the handle's stream, nothing waited for, no staging buffer */
int ilqr_evaluate_policy_on_device(ilqr_batch* h, int t0, int n_knots, int n_samples, int flags, const void* x_device, void* cost_device,
                                   void* x_end_device, void* u_first_device);

/* ---- per-trajectory model parameters (additive under ABI 6) ----------------------------------------------------------------------
 * A user device twin may declare NTP parameters that differ from trajectory to trajectory (csrc/models.hpp: NTP, set_trajectory_params) --
 * a target that moves between receding-horizon steps, a perturbed model per trajectory.  Once set, every later rollout, derivative sweep
 * and ilqr_mpc_step of the handle evaluates trajectory b's model with row b; what a model's set_trajectory_params does not write keeps the
 * handle-wide values of ilqr_create (user_params, u_min / u_max).  An fp32 handle uses the rows' float-rounded values in both of its twins,
 * as it does for user_params.  Setting parameters does NOT re-evaluate the stored cost or trajectory: a caller who changes them in the
 * middle of a solve calls ilqr_warm_start or ilqr_mpc_step next (both roll out and cost again).  ilqr_get_derivatives returns what the last
 * sweep left.  Only ILQR_MODEL_USER handles on the generic wavefront-per-trajectory kernels take them: ILQR_ERR_UNSUPPORTED for every other
 * model, for a twin without the two members, for an nx = 4 twin (persistent tiled kernels) and for a small twin created without
 * ILQR_ROUTE_WAVE_PER_TRAJECTORY; ilqr_last_error() names which. */
int ilqr_trajectory_params_count(void); /* NTP of this build's user model, 0 = none; needs no device */
/* p [B][n] double, n == NTP.  Exactly one of p (host) and p_device (this handle's device) is non-NULL.  Enqueued on the handle's stream,
 * no synchronisation; a host array from page-locked memory must stay unchanged until the stream has passed the call (as x0 of
 * ilqr_mpc_step).  The first call on a handle allocates the rows. */
int ilqr_set_trajectory_params(ilqr_batch* h, const double* p, const void* p_device, int n);
int ilqr_get_trajectory_params(ilqr_batch* h, double* p, int n); /* the rows as they were set; synchronises; ILQR_ERR_STATE while none are set (or per-knot rows are) */
/* back to the handle-wide parameters of ilqr_create for every trajectory (clears per-knot rows as well) */
int ilqr_clear_trajectory_params(ilqr_batch* h);

/* ---- per-knot model parameters (additive under ABI 6) ------------------------------------------------------------------------------
 * The same NTP parameters, one row per KNOT of every trajectory: reference tracking, gait and contact schedules, time-varying cost
 * weights, a disturbance preview, a model that changes inside the horizon.  A handle's model rows are in one of three states: none, one
 * row per trajectory (above), or one row per knot.  With knot rows P[b][t][0..NTP), t = 0..T, the model copy of trajectory b is set from row
 * t through the twin's set_trajectory_params before anything is evaluated at knot t: cost(x_t, u_t) and dynamics(x_t, u_t) use row t;
 * final_cost(x_T) and the t = T special cases of the derivative record use row T.  Fields the twin does not write keep ilqr_create's
 * values; an fp32 handle uses the rows' float-rounded values in both of its twins.  The limits the backward pass's box-QP sees stay the
 * handle's (u_min / u_max of ilqr_create), exactly as with per-trajectory rows: a twin whose set_trajectory_params writes its limit
 * fields changes what an opt-in clamp of the rollouts sees, never the box-QP.  No twin changes: any header with NTP and
 * set_trajectory_params takes knot rows.
 * THE SOURCE ARRAY p / p_device is [B][n_knots][n] double with n == NTP, a reference of any length; exactly one of the two pointers is
 * non-NULL.  THE WINDOW: the handle takes the T + 1 rows starting at k0 -- row t of the handle is source row min(k0 + t, n_knots - 1), so
 * the horizon's tail holds the last row of a reference that ends.  Tracking MPC is two calls per step with no re-packing by the caller:
 *     ilqr_set_knot_params(h, NULL, ref_device, NTP, L, k);   ilqr_mpc_step(..., shift = s, ...);   k += s;
 * The handle owns a copy [B][T+1][NTP] double, allocated on first use and kept (B = 4096, T = 200, NTP = 8: 52 MB); a gather kernel fills
 * it on the handle's stream and nothing is waited for.  A host p goes up whole into a scratch buffer of B * n_knots * NTP doubles the
 * handle keeps while the next call's fits, then through the same gather; a host array from page-locked memory must stay unchanged until
 * the stream has passed the call (as x0 of ilqr_mpc_step).
 * The setter switches the handle to knot mode, ilqr_set_trajectory_params back to one row per trajectory, ilqr_clear_trajectory_params
 * clears either.  As with per-trajectory rows, setting does NOT re-evaluate the stored cost or trajectory: the next ilqr_warm_start /
 * ilqr_mpc_step does.  ilqr_shift_horizon does not move the rows -- the caller names the window --, and the ilqr_clone_* calls copy no
 * rows of either kind.  In knot mode ilqr_get_trajectory_params answers ILQR_ERR_STATE, and ilqr_get_param_gradient /
 * ilqr_param_gradient_on_device answer ILQR_ERR_UNSUPPORTED (the gradient is defined for per-trajectory rows; they never read rows of an
 * earlier mode).
 * Refusals, before anything is enqueued, in this order (ilqr_last_error() names each): ILQR_ERR_INVALID without needing a handle for not
 * exactly one of p / p_device, n_knots < 1, k0 outside [0, n_knots); a null handle; ILQR_ERR_UNSUPPORTED for every handle
 * ilqr_set_trajectory_params refuses; ILQR_ERR_INVALID for n != NTP and for B * (T + 1) * NTP beyond INT_MAX. */
int ilqr_set_knot_params(ilqr_batch* h, const double* p, const void* p_device, int n, int n_knots, int k0);
/* [B][T+1][NTP] as the kernels see them (the window, not the source); synchronises; ILQR_ERR_STATE outside knot mode */
int ilqr_get_knot_params(ilqr_batch* h, double* p, int n);

/* ---- the gradient of a caller's loss with respect to the per-trajectory parameters (additive under ABI 6) ----------------------------
 * ilqr_solve_lq turns gx = dL/dxs, gu = dL/dus into dxs, dus and the multipliers dlam; these calls turn those three into dL/dp, the
 * gradient of the loss in the rows of ilqr_set_trajectory_params the solve ran under (masses, dampings, cost weights, targets: system
 * identification and cost learning through MPC), in one sweep over the horizon with 6 * NTP model evaluations per knot and direction
 * instead of 2 * NTP whole re-solves.  With the KKT residual r(z, lambda; p) of the nominal problem and ilqr_solve_lq's convention
 * (K [dz; dlambda] = -[g; 0]) the implicit-function theorem gives dL/dp = d/dp G(p),
 *     G(p) = sum_{t<T} [ grad_{x,u}(c_t + lam[t+1].F_t)(x_t, u_t; p).(dx_t, du_t) + dlam[t+1].F_t(x_t, u_t; p) ] + grad c_T(x_T; p).dx_T
 * with F the Euler map x + dt * dynamics(x, u), lam the nominal costate, and (x, u, lam, dx, du, dlam) held fixed while p moves: a
 * contraction of model derivatives along caller-given vectors, which is how it is defined here.
 * DEFINITION -- xs, us as ilqr_get_trajectory would return them at this moment (an accepted candidate still waiting to be copied is copied
 * first), the derivative records as ilqr_get_derivatives would return them, p the rows as they were set (an fp32 handle: their
 * float-rounded values).  n_dirs directions per trajectory:
 *     in:  dxs, dlam [B][T+1][n_dirs][nx]   dus [B][T][n_dirs][nu]       (the layouts ilqr_solve_lq writes; dlam[:, 0] is not read)
 *     out: gp [B][n_dirs][NTP]   lam [B][T+1][nx]
 * An input that is NULL is zero, not all three; either output may be NULL, not both.
 *     lam[T] = cx[T],   lam[t] = cx[t] + fx[t]' lam[t+1]                 (t = T-1 .. 0; each sum over r ascending)
 * For trajectory b, direction s, parameter j:  h = eps_p * max(1, |p[b][j]|) (eps_p = 0 means 1e-3);  M+, M- the handle's model with the
 * row p[b] + h e_j, p[b] - h e_j applied through set_trajectory_params on the kernel's own copy;  eps = 1e-3, the records' own step.
 *     t < T:  z = (xs[t], us[t]),  d = (dxs[t][s], dus[t][s]),  n = |d|_2
 *             Psi(M, sigma) = M.cost(z + sigma (eps / n) d) + lam[t+1] . F_M(z + sigma (eps / n) d)
 *             A_t = (Psi(M+,+) - Psi(M+,-) - Psi(M-,+) + Psi(M-,-)) * n / (4 eps h),  zero when n = 0
 *             B_t = dlam[t+1][s] . (F_{M+}(z) - F_{M-}(z)) / (2 h)
 *     t = T:  A_T the same stencil of final_cost along dxs[T][s]; no B_T
 *     gp[b][s][j] = sum_t (A_t + B_t)
 * All arithmetic is double, in UserModelT<double>, on every handle (an fp32 handle's stored floats are widened).  The sum over t runs in a
 * fixed order (ascending inside chunks of 16 knots, then the chunks ascending) and no atomics are used: repeated calls give the same bits.
 * Column s of gp depends on column s of the inputs only, bit for bit.  A non-finite evaluation poisons only its own gp[b][s][:].
 * Read-only: later iterations are bit for bit those of a handle that never asked.  The arrays of a call do not overlap.
 * What this is NOT: with (dxs, dus, dlam) from ilqr_solve_lq the result is the gradient through the equality-constrained LQ subproblem the
 * records hold (fx, fu, cxx, cxu, cuu).  That model is Gauss-Newton -- cxx carries no lam.F_zz term --, so the result is exact when the
 * dynamics are linear in (x, u) and approximate otherwise (pendulum chain, T = 20, a random linear loss, against central differences
 * over whole re-solves: within 1.6e-5 relative at g/l = 0, inside the re-solves' own step-size noise; off by 0.1 to 19 % at g/l = 9.81).
 * SCRATCH: the handle keeps one device buffer for these calls, allocated by the first call and kept while the next one's fits, of
 *     [lam NULL] B * (T + 1) * nx + [gp given] B * ceil((T + 1) / 16) * n_dirs * NTP   doubles.
 * ILQR_ERR_INVALID (checked first, in this order; the first five need no handle): n_dirs < 1, unknown flag bits, eps_p negative or not
 * finite, all three inputs NULL, both outputs NULL, a null handle; then B * (T + 1) * n_dirs * max(nx, nu, NTP) beyond INT_MAX.
 * ILQR_ERR_UNSUPPORTED: every handle on which ilqr_set_trajectory_params is refused -- a build without a user model or whose twin has no
 * NTP, ILQR_MODEL_HOST and the built-in models, the tiled nx = 4 and small-twin kernels.  ILQR_ERR_STATE: before ilqr_init_traj /
 * ilqr_set_trajectory, or while no per-trajectory rows are set (the handle-wide user_params have no defined mapping onto the NTP fields).
 * Every refusal happens before anything is enqueued and ilqr_last_error() names it. */
enum ilqr_param_gradient_flags { ILQR_PARAM_GRADIENT_NO_FLAGS = 0 }; /* none yet: unknown bits are refused */
/* host arrays: a call-sized device buffer takes the inputs up and the outputs down; synchronises */
int ilqr_get_param_gradient(ilqr_batch* h, int n_dirs, int flags, double eps_p, const double* dxs, const double* dus, const double* dlam,
                            double* gp, double* lam);
/* device memory of this handle's device: enqueued on the handle's stream, nothing waited for */
int ilqr_param_gradient_on_device(ilqr_batch* h, int n_dirs, int flags, double eps_p, const void* dxs_device, const void* dus_device,
                                  const void* dlam_device, void* gp_device, void* lam_device);

/* ---- single stages (teacher-forced parity tests, host-model fallback) --------------------- */
/* STEP 1, src/ilqr_core.cpp:115-120 = src/derivatives.cpp:15-144 over t = 0..T, all trajectories */
int ilqr_compute_derivatives(ilqr_batch* h);
/* one iLQR::backward_pass(), src/ilqr_core.cpp:350-401, at the current lambda (no retry).
 * diverge_out [B] (may be NULL) receives its return value. Also refreshes dV. */
int ilqr_backward_pass(ilqr_batch* h, int* diverge_out);
/* STEP 2 incl. the lambda-increase retry loop and the gradient-norm test, ilqr_core.cpp:136-159 */
int ilqr_backward_step(ilqr_batch* h);
/* iLQR::forward_pass(x0,u) for u = us + alpha*k, src/ilqr_core.cpp:305-337 with :188-190:
 * all 11 alphas of include/ilqr.h:24 are rolled out concurrently; cost_out [B][11] may be NULL. */
int ilqr_rollout_candidates(ilqr_batch* h, double* cost_out);
/* STEP 3 + STEP 4, src/ilqr_core.cpp:175-282: candidates, first-accept selection in the
 * reference's serial order, lambda update, termination tests, commit of the accepted one. */
int ilqr_line_search(ilqr_batch* h);
/* Host-evaluated models (ILQR_MODEL_HOST): the caller rolled the 11 candidates out itself
 * (forward_pass needs Model::dynamics/cost, host virtuals) and hands over their costs
 * cost_c [B][11]; the device applies STEP 3/4 of src/ilqr_core.cpp:184-282 to them -- first
 * accepted alpha in the reference's serial order, cost_s, lambda schedule, termination tests,
 * iteration count -- and reports the accepted alpha index per trajectory (accepted [B], -1 =
 * none).  The caller then stores the accepted rollout with ilqr_set_trajectory. */
int ilqr_accept_candidates(ilqr_batch* h, const double* cost_c, int* accepted);
/* For callers that produce the first rollout themselves (host-evaluated models) and pass it in
 * with ilqr_set_trajectory.
 *   warm = 0: the non-rollout part of iLQR::init_traj (src/ilqr_core.cpp:23-48 and the statics of
 *             include/ilqr.h:17-18): zero the derivative and gain arrays, lambda = dlambda =
 *             initial values, every trajectory running with zero iterations.
 *   warm = 1: a new outer loop on the stored solution (warm start, src/ilqr_core.cpp:65-76):
 *             status, iteration count and flgChange restart; lambda, dlambda, gains and
 *             derivatives persist. */
int ilqr_reset_state(ilqr_batch* h, int warm);

/* ---- state exchange (canonical host layouts, see top) -------------------------------------- */
int ilqr_set_trajectory(ilqr_batch* h, const double* x0, const double* xs, const double* us, const double* cost);
int ilqr_set_gains(ilqr_batch* h, const double* k, const double* K);
int ilqr_set_derivatives(ilqr_batch* h, const double* fx, const double* fu, const double* cx,
                         const double* cu, const double* cxx, const double* cxu, const double* cuu);
int ilqr_set_lambda(ilqr_batch* h, const double* lambda, const double* dlambda); /* [B] each, NULL = keep */

int ilqr_get_trajectory(ilqr_batch* h, double* xs, double* us); /* either may be NULL */
int ilqr_get_gains(ilqr_batch* h, double* k, double* K);
/* The derivative records.  WHICH trajectory they describe depends on the route, as the reference's members do on where its loop stands
 * (src/ilqr_core.cpp:115-120 refreshes fx ... cuu at the top of an iteration, :210-213 accepts a new trajectory at its end):
 *   - after a stage call (ilqr_compute_derivatives, ilqr_set_derivatives): the records that call left;
 *   - nx = 4 handles after ilqr_iterate: the persistent kernels keep no records in memory; the getter computes those of the CURRENT
 *     nominal trajectory on demand (zeros after ilqr_init_traj, as ilqr_core.cpp:39-45 leaves them);
 *   - LQ model with exact derivatives on the default route: likewise recomputed for the current nominal trajectory (k_analytic_lq);
 *   - generic handles on the record-keeping routes (finite differences, ILQR_ROUTE_BACKWARD_W2, ILQR_ROUTE_FULL_RECORDS, user twins,
 *     host-evaluated models): what the LAST sweep left, i.e. the records of the trajectory the last iteration STARTED from -- one
 *     accepted step behind the nominal trajectory, exactly as the reference's members are after generate_trajectory().
 * A caller that needs one definite meaning calls ilqr_compute_derivatives first: then every route returns the current trajectory's. */
int ilqr_get_derivatives(ilqr_batch* h, double* fx, double* fu, double* cx, double* cu,
                         double* cxx, double* cxu, double* cuu);
int ilqr_get_cost(ilqr_batch* h, double* cost);                     /* [B] cost_s */
int ilqr_get_lambda(ilqr_batch* h, double* lambda, double* dlambda); /* [B] */
int ilqr_get_dV(ilqr_batch* h, double* dV);                         /* [B][2] */
int ilqr_get_gnorm(ilqr_batch* h, double* gnorm);                   /* [B] */
int ilqr_get_status(ilqr_batch* h, int* status, int* iters, int* alpha_idx); /* [B] each, any NULL */
/* one alpha's rollout of the LAST line search (ilqr_rollout_candidates / ilqr_line_search / ilqr_iterate).  The candidate
 * buffers are scratch of the line search (the reference keeps x_new/u_new as locals of its loop, src/ilqr_core.cpp:184-186):
 * ILQR_ERR_STATE when none has been rolled out yet or when ilqr_generate_trajectory re-packed running trajectories
 * (compaction), which leaves the buffers behind. */
int ilqr_get_candidate(ilqr_batch* h, int alpha_idx, double* xs, double* us);
int ilqr_count_running(ilqr_batch* h, int* n_running);
/* device-to-device copy of the per-trajectory costs [B] into caller-owned device memory
 * (the payload of the multi-GPU gather).  Enqueued on the handle's stream:
 * ilqr_synchronize before handing the buffer to work on another stream (a collective). */
int ilqr_copy_cost_to_device(ilqr_batch* h, void* dst_device);
/* ---- results without a host round trip per array (ABI 5) ------------------------------------------------------------------------
 * The reference hands its caller xs / us / K / k as members (include/ilqr.h:48-56); a batched caller of the getters above pays one
 * unpack kernel + one device-to-host copy + one stream synchronisation per array, and for an 11 ms job (B = 4096, 20 iterations)
 * 164 MB of results are 3-10 ms of that.  Two ways around it:
 * (1) Callers that stay on the GPU (MPC: the next warm start, src/ilqr_core.cpp:65-76, a learned policy's loss, ...): the canonical
 *     layouts of the top of this file as double, written into CALLER-OWNED DEVICE memory on this handle's device.  Enqueued on the handle's
 *     stream, not waited for (ilqr_synchronize, or stream order, before another stream reads them).  Any pointer may be NULL. */
int ilqr_copy_trajectory_to_device(ilqr_batch* h, void* xs_device, void* us_device);
int ilqr_copy_gains_to_device(ilqr_batch* h, void* k_device, void* K_device);
/* (2) Host callers: every requested array (NULL = skip) in ONE call -- the unpack kernels and the device-to-host copies follow each
 *     other on the handle's stream with NO synchronisation; the arrays are valid after ilqr_synchronize.  With page-locked destinations
 *     (ilqr_host_register once per buffer a caller reuses, or hipHostMalloc) the copies are DMA at PCIe rate and the call returns at
 *     once; with pageable memory the runtime stages them and the call may block, the result is the same. */
int ilqr_get_results_async(ilqr_batch* h, double* xs, double* us, double* k, double* K, double* cost);
/* hipHostRegister / hipHostUnregister for callers that do not link the HIP runtime themselves */
int ilqr_host_register(void* ptr, size_t bytes);
int ilqr_host_unregister(void* ptr);

/* ---- several shards of one batch, one process ----------------------------------
 * The path partitions by trajectory: shard i = a handle of its own (any device, ilqr_desc.device) holding the contiguous block
 * [offset_i, offset_i + B_i) of the global batch; there is no data-path collective.  A group names the shards of one job and
 * performs its ONE exchange, the gather of the per-trajectory costs in global order:
 *   - shards on n > 1 DISTINCT devices: one RCCL communicator per device (ncclCommInitAll, one process) and one
 *     ncclAllGather of the padded shards over xGMI -- every device ends up with the whole vector (librccl.so is loaded when the
 *     first such group is created, not by ilqr_create);
 *   - shards that share a device (N logical shards on one GPU): device-to-host copies, shard by shard.
 * The reference has no counterpart (one trajectory per process, src/run_ilqr.cpp:27-59); a caller of it who solves many
 * problems loops over them -- this is that loop's gather. */
typedef struct ilqr_group ilqr_group;
/* flags: 1 = use RCCL even for a single device / a single shard (tests) */
int ilqr_group_create(ilqr_batch* const* shards, int n_shards, int flags, ilqr_group** out);
void ilqr_group_destroy(ilqr_group* g);
/* cost_out: host [sum of the shards' B], global order.  Synchronises every shard. */
int ilqr_group_gather_costs(ilqr_group* g, double* cost_out);
/* 1 if the group's gather runs over RCCL, 0 if it copies; *n_ranks = communicators in use (0 without RCCL) */
int ilqr_group_uses_rccl(ilqr_group* g, int* n_ranks);

/* ---- measurement --------------------------------------------------------------------------- */
enum ilqr_stage { ILQR_STAGE_DERIVATIVES = 0, ILQR_STAGE_BACKWARD = 1, ILQR_STAGE_ROLLOUT = 2,
                  ILQR_STAGE_ACCEPT = 3, ILQR_STAGE_SOLVE = 4, ILQR_NUM_STAGES = 5 };
/* HIP-event timing of every kernel launch of a stage, accumulated on the handle's stream.  ILQR_STAGE_SOLVE is the
 * persistent per-tile kernel of ilqr_iterate (one launch = all the iterations of the call); while it runs, the
 * BACKWARD and ROLLOUT slots receive the kernel's own per-phase clocks (mean over tiles, one "launch" per
 * iteration) so that the split stays visible. */
int ilqr_profile_enable(ilqr_batch* h, int enable);
int ilqr_profile_reset(ilqr_batch* h);
/* total milliseconds and launch count per stage since the last reset (synchronises) */
int ilqr_profile_read(ilqr_batch* h, double ms_out[ILQR_NUM_STAGES], int launches_out[ILQR_NUM_STAGES]);
/* The clock the CUs ran at during the persistent kernel's launches since the last reset, in MHz: shader cycles (s_memtime)
 * over constant-rate ticks, summed over tiles.  MI355X lowers its clock with the number of busy SIMDs, so issue-rate
 * figures derived from a launch duration need the clock of THAT launch (bench.py: roofline_issue). */
int ilqr_profile_shader_clock(ilqr_batch* h, double* mhz_out);
/* name of the kernel a stage launches (as rocprofv3 reports it), for bench.py's roofline line: looked up from the route plan the handle
 * fixed at ilqr_create, the one its launchers switch on */
const char* ilqr_stage_kernel_name(ilqr_batch* h, int stage);

#ifdef __cplusplus
}
#endif
#endif /* ILQR_AMD_H_ */
