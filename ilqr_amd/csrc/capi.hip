// capi.hip -- the entry points of the C ABI of include/ilqr_amd.h (creation, whole solves, stage calls, state exchange) on top of the
// HIP kernels.  The handle and its helpers: handle.hpp; which kernels a handle runs: route.hpp; kernel launchers: launch.hpp; shard groups (RCCL):
// group.hpp; measurement: profile.hpp -- one translation unit (every kernel template is instantiated where it is launched).
// No CPU compute path exists: every entry point either launches kernels or moves bytes.
#include "../../include/ilqr_amd.h"

#include <stdarg.h>
#include <stdio.h>
#include <limits.h>
#include <string.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "backward_wave.hpp"
#include "backward_wave2.hpp"
#include "backward_wave3.hpp"
#include "generic.hpp"
#include "kernels_wide.hpp"
#include "kernels_wide2.hpp"
#include "kernels.hpp"
#include "value_thread.hpp"
#include "value_wave.hpp"
#include "covariance_thread.hpp"
#include "covariance_wave.hpp"
#include "sensitivity_thread.hpp"
#include "sensitivity_wave.hpp"
#include "lq_solve_thread.hpp"
#include "lq_solve_wave.hpp"
#include "estimator_thread.hpp"
#include "estimator_wave.hpp"
#include "risk_thread.hpp"
#include "risk_wave.hpp"
#include "evaluate.hpp"
#include "param_gradient.hpp"
#include "clone.hpp"

using namespace ilqr;

#include "route.hpp"
#include "staging.hpp"
#include "handle.hpp"
#include "launch.hpp"

// ------------------------------------------------------------------------------------------
// public API
// ------------------------------------------------------------------------------------------
extern "C" {

const char* ilqr_last_error(void) { return g_err; }
int ilqr_abi_version(void) { return ILQR_AMD_ABI_VERSION; }
int ilqr_has_user_model(void) {
#ifdef ILQR_HAVE_USER_MODEL
  return 1;
#else
  return 0;
#endif
}

void ilqr_default_params(ilqr_params* p) {  // include/ilqr.h:14-24
  p->max_iter = 100;
  p->tol_fun = 1e-6;
  p->tol_grad = 1e-6;
  p->lambda_init = 1;
  p->dlambda_init = 1;
  p->lambda_factor = 1.6;
  p->lambda_max = 1e11;
  p->lambda_min = 1e-8;
  p->z_min = 0;
}

void ilqr_destroy(ilqr_batch* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
#ifdef ILQR_W2_TIMING
  if (h->aos) {  // experiment build: what the first wavefront of every k_backward_w2 launch spent where (backward_wave.hpp)
    long long st[8], qp[8], cnt[4];
    if (hipMemcpyFromSymbol(st, HIP_SYMBOL(g_w2_cycles), sizeof(st)) == hipSuccess && hipMemcpyFromSymbol(qp, HIP_SYMBOL(g_q_cycles), sizeof(qp)) == hipSuccess &&
        hipMemcpyFromSymbol(cnt, HIP_SYMBOL(g_q_counts), sizeof(cnt)) == hipSuccess && cnt[0] > 0) {
      const double q = (double)cnt[0];  // (literal box-QPs; on the k_backward_w3 route the step sections are per LITERAL QP too: scale by the counts below)
      fprintf(stderr, "[k_backward_w2, wavefront 0] shader cycles per step: load+Qx/Qu %.0f  Vxx'fx,Vxx'fu %.0f  Qxx/Qux/Quu %.0f  box-QP %.0f  K %.0f  dV+T1+Vx %.0f  Vn+symmetrise+stores %.0f  (loop top %.0f)\n",
              st[0] / q, st[1] / q, st[2] / q, st[3] / q, st[4] / q, st[5] / q, st[6] / q, st[7] / q);
      fprintf(stderr, "[box-QP] per QP: %.2f iterations, %.2f factorisations, %.2f Armijo trips beyond the first; cycles: gradient+clamp set %.0f  Cholesky %.0f  inverse+R^-1R^-T %.0f  direction %.0f  line search %.0f  rest %.0f\n",
              cnt[1] / q, cnt[2] / q, cnt[3] / q, qp[0] / q, qp[1] / q, qp[2] / q, qp[3] / q, qp[4] / q, qp[5] / q);
    }
    long long w3[4];
    if (hipMemcpyFromSymbol(w3, HIP_SYMBOL(g_w3_counts), sizeof(w3)) == hipSuccess && w3[0] + w3[1] > 0)
      fprintf(stderr, "[k_backward_w3, wavefront 0] box-QPs on the matrix-core path %lld, handed to the literal path %lld, Newton-Schulz iterations per refinement %.2f\n",
              w3[0], w3[1], (double)w3[2] / (double)(w3[0] > 0 ? w3[0] : 1));
  }
#endif
  for (void* p : h->allocs) (void)hipFree(p);
  if (h->staging) (void)hipFree(h->staging);
  if (h->lq_scratch) (void)hipFree(h->lq_scratch);
  if (h->est_scratch) (void)hipFree(h->est_scratch);
  if (h->pg_scratch) (void)hipFree(h->pg_scratch);
  if (h->knot_stage) (void)hipFree(h->knot_stage);
  if (h->d_perm) (void)hipFree(h->d_perm);
  if (h->perm_scratch) (void)hipFree(h->perm_scratch);
  (void)timers_drain(h);  // (every event back into the pool, each once)
  for (hipEvent_t e : h->event_pool) (void)hipEventDestroy(e);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

// Every refusal of ilqr_create, on the descriptor and this build's user twin alone: no HIP call, so before any device is looked for.
// When several apply, the first one below wins.
static int check_desc(const ilqr_desc* d) {
  // (ABI 6 added entry points only: ilqr_desc is ABI 5's, and a caller built against ABI 5 keeps working)
  REQUIRE(d->abi_version == ILQR_AMD_ABI_VERSION || d->abi_version == 5, "ABI version %d, library is %d (accepts 5 and %d)", d->abi_version,
          ILQR_AMD_ABI_VERSION, ILQR_AMD_ABI_VERSION);
  REQUIRE(d->B >= 1 && d->T >= 1 && d->nx >= 1 && d->nu >= 1, "B, T, nx, nu must be positive");
  REQUIRE(d->nx <= MAXN && d->nu <= kMaxControls, "nx <= %d and nu <= %d", MAXN, kMaxControls);
  REQUIRE(d->dt > 0, "dt must be positive");
  if (d->route & 128)  // (ILQR_ROUTE_BACKWARD_LDS of ABI <= 4)
    return fail(ILQR_ERR_UNSUPPORTED, "route bit 128 (round 1's LDS kernel k_backward_w) was retired in ABI 5: ILQR_ROUTE_BACKWARD_W2 gives the same bits");
  if ((d->route & ILQR_ROUTE_WIDE_TWO_PER_CU) && d->nu == 2 && d->nx == 4)
    return fail(ILQR_ERR_UNSUPPORTED, "ILQR_ROUTE_WIDE_TWO_PER_CU: the m = 2 wide tiles (k_solve_wide2) run one tile per CU (four wavefronts at <= 512 registers); the bit applies to k_solve_wide (m = 1)");
  if (d->dtype != ILQR_DTYPE_F64 && d->dtype != ILQR_DTYPE_F32) return fail(ILQR_ERR_INVALID, "dtype %d: ILQR_DTYPE_F64 or ILQR_DTYPE_F32", d->dtype);
  if (d->nu > WM) {  // 16 < nu <= 32: the generic backward pass with two control tiles (k_backward_w3, MT = 2); what is not widened says so
    const char* what = (d->dtype == ILQR_DTYPE_F32) ? "fp32" : (d->route & ILQR_ROUTE_BACKWARD_W2) ? "ILQR_ROUTE_BACKWARD_W2" : (d->route & ILQR_ROUTE_LQ_DENSE_FD) ? "ILQR_ROUTE_LQ_DENSE_FD"
                       : (d->flags & ILQR_FLAG_REGULARIZE_VXX) ? "ILQR_FLAG_REGULARIZE_VXX" : nullptr;
    if (what) return fail(ILQR_ERR_UNSUPPORTED, "%s supports at most %d controls (nu = %d)", what, WM, d->nu);
  }
  if ((d->route & ILQR_ROUTE_TWO_CONTROL_TILES) && (d->route & ILQR_ROUTE_BACKWARD_W2))
    return fail(ILQR_ERR_UNSUPPORTED, "ILQR_ROUTE_TWO_CONTROL_TILES and ILQR_ROUTE_BACKWARD_W2 name two different backward kernels");
  if ((d->route & ILQR_ROUTE_TWO_CONTROL_TILES) && (d->flags & ILQR_FLAG_REGULARIZE_VXX))
    return fail(ILQR_ERR_UNSUPPORTED, "ILQR_FLAG_REGULARIZE_VXX is implemented in k_backward_w3 (at most 16 controls): drop ILQR_ROUTE_TWO_CONTROL_TILES");
  const bool aos = generic_layout(d->model, d->route, kUserTiled, kUserSmall);
  if (d->dtype == ILQR_DTYPE_F32 && aos) {  // fp32 on the generic path: the device models, k_backward_w3 with one control tile
    if (d->model == ILQR_MODEL_HOST)
      return fail(ILQR_ERR_UNSUPPORTED, "fp32 is not available for ILQR_MODEL_HOST: the caller evaluates the model and owns its records (fp64)");
    if (d->route & ILQR_ROUTE_BACKWARD_W2)
      return fail(ILQR_ERR_UNSUPPORTED, "fp32 is not available on ILQR_ROUTE_BACKWARD_W2 (the literal-order fp64 cross-check): fp32 handles run k_backward_w3");
    if (d->route & ILQR_ROUTE_TWO_CONTROL_TILES)
      return fail(ILQR_ERR_UNSUPPORTED, "fp32 is not available on ILQR_ROUTE_TWO_CONTROL_TILES: fp32 handles run k_backward_w3 with one control tile");
  }
  if (d->model == ILQR_MODEL_ACROBOT) {
    REQUIRE(d->nx == 4 && d->nu == 1, "acrobot is nx=4 nu=1 (include/acrobot.h:27-28), got %d/%d", d->nx, d->nu);
  } else if (d->model == ILQR_MODEL_DOUBLE_INTEGRATOR) {
    REQUIRE(d->nx == 4 && d->nu == 2, "double integrator is nx=4 nu=2 (include/double_integrator.h:16-17), got %d/%d", d->nx, d->nu);
#ifdef ILQR_HAVE_USER_MODEL
  } else if (d->model == ILQR_MODEL_USER) {
    using UM = UserModelT<double>;
    REQUIRE(d->nx == UM::NX && d->nu == UM::NU, "this build's user model is nx=%d nu=%d, got %d/%d", UM::NX, UM::NU, d->nx, d->nu);
    REQUIRE(d->u_min && d->u_max, "ILQR_MODEL_USER needs u_min/u_max (Model::u_min/u_max, include/model.h:17)");
    REQUIRE(!(d->flags & ILQR_FLAG_ANALYTIC_DERIVATIVES) || has_analytic_record<UM>::value, "this user model has no analytic_record()");
    // not a tiled shape -- or a small one asked to take the generic route: the generic kernels (fp64), trajectory-contiguous layout like the LQ model's
    // (a small twin asked onto the generic kernels -- ILQR_ROUTE_WAVE_PER_TRAJECTORY -- is the fp64 cross-check of its tiled kernels)
    if (aos && kUserSmall) REQUIRE(d->dtype == ILQR_DTYPE_F64, "ILQR_ROUTE_WAVE_PER_TRAJECTORY on a small twin is the fp64 cross-check of its tiled kernels: fp64 only");
    REQUIRE(d->n_user_params >= 0 && (d->n_user_params == 0 || d->user_params), "ILQR_MODEL_USER: n_user_params = %d with user_params = %p", d->n_user_params, (const void*)d->user_params);
#endif
  } else if (d->model == ILQR_MODEL_HOST || d->model == ILQR_MODEL_LQ) {
    // Generic dimensions: trajectory-contiguous layout, one wavefront per trajectory in the backward
    // pass.  Host-evaluated models receive their derivatives through ilqr_set_derivatives; the LQ
    // model has a device twin (generic.hpp) and runs end to end.
    REQUIRE(d->nx <= WN && d->nu <= WMW, "generic kernels: nx <= %d, nu <= %d", WN, WMW);
    REQUIRE(d->u_min && d->u_max, "generic handles need u_min/u_max (Model::u_min/u_max, include/model.h:17)");
    if (d->model == ILQR_MODEL_LQ)
      REQUIRE(d->lq_A && d->lq_B && d->lq_Q && d->lq_R && d->lq_Qf, "ILQR_MODEL_LQ needs lq_A, lq_B, lq_Q, lq_R, lq_Qf");
  } else {
    return fail(ILQR_ERR_UNSUPPORTED, "model id %d is not available in this build", d->model);
  }
  // generic handles: ILQR_FLAG_REFERENCE_FIXES -- models with a device twin: their rollouts clamp, their box-QP reports a failed factorisation; the
  // host-evaluated route: the box-QP likewise, the rollouts belong to the caller (the facade clamps).  ILQR_FLAG_REGULARIZE_VXX is the backward pass's alone (k_backward_w3<.., REGV>), on any model
  if ((d->flags & ILQR_FLAG_REGULARIZE_VXX) && aos && (d->route & ILQR_ROUTE_BACKWARD_W2))
    return fail(ILQR_ERR_UNSUPPORTED, "ILQR_FLAG_REGULARIZE_VXX on the generic path is implemented in k_backward_w3: drop ILQR_ROUTE_BACKWARD_W2");
  // (a host-evaluated model under ILQR_FLAG_REFERENCE_FIXES: part (2), the failed factorisation that ends the box-QP, is the device's -- k_backward_w3 /
  //  k_backward_w2 honour sp.fixes & 2 --; part (1), the clamped rollout, belongs to whoever rolls out: the C++ facade's host_forward does it)
  return 0;
}

static void copy_desc(const ilqr_desc* d, ilqr_batch* h) {
  // route choices come with the descriptor (ilqr_desc.route, include/ilqr_amd.h): the library reads no environment
  h->lq_wide = d->model == ILQR_MODEL_LQ && d->nu > WM;  // the LQ twin beyond 16 controls: LqModelW on the generic kernels
  h->route.full_records = (d->route & ILQR_ROUTE_FULL_RECORDS) != 0;
  h->route.no_compaction = (d->route & ILQR_ROUTE_NO_COMPACTION) != 0;
  h->route.wide_occ = (d->route & ILQR_ROUTE_WIDE_ONE_PER_CU) ? 1 : (d->route & ILQR_ROUTE_WIDE_TWO_PER_CU) ? 2 : 0;
  h->aos = generic_layout(d->model, d->route, kUserTiled, kUserSmall);
  h->model = d->model; h->dtype = d->dtype; h->flags = d->flags;
  h->nx = d->nx; h->nu = d->nu; h->T = d->T; h->B = d->B; h->dt = d->dt;
  h->Bp = ((d->B + 63) / 64) * 64;
  h->ntiles = h->Bp / TW;
  if (d->params)
    h->params = *d->params;
  else
    ilqr_default_params(&h->params);
}

static int open_device(const ilqr_desc* d, ilqr_batch* h) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(ILQR_ERR_NO_DEVICE, "no HIP device visible: libilqr_amd has no CPU path");
  if (d->device < 0 || d->device >= ndev) return fail(ILQR_ERR_NO_DEVICE, "device %d out of range (%d visible)", d->device, ndev);
  HIPCHK(hipSetDevice(d->device));
  h->device = d->device;
  HIPCHK(hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, d->device));
  if (d->assume_cus > 0) h->num_cus = d->assume_cus;
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, d->device) == hipSuccess && khz > 0) h->wall_clock_khz = khz;
  h->stream = (hipStream_t)d->stream;
  h->own_stream = !d->stream;
  if (h->own_stream) HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  return 0;
}

// the models' parameters (the constructor bodies of acrobot.h:14-40, double_integrator.h:14-27); an fp32 handle's float models, and
// their parameters' float values in the double twins
static void set_model_params(const ilqr_desc* d, ilqr_batch* h) {
  if (d->model == ILQR_MODEL_ACROBOT) {
    AcrobotModel& m = h->acrobot;
    m.goal[0] = 3.1415;
    m.goal[1] = m.goal[2] = m.goal[3] = 0;
    m.u_min[0] = d->u_min ? d->u_min[0] : -5.0;
    m.u_max[0] = d->u_max ? d->u_max[0] : 5.0;
    if (h->dtype == ILQR_DTYPE_F32) {  // the float model, and its parameters' float values in the double twin
      AcrobotModelT<float>& f = h->acrobot_f;
      for (int i = 0; i < 4; i++) m.goal[i] = (double)(f.goal[i] = (float)m.goal[i]);
      m.u_min[0] = (double)(f.u_min[0] = (float)m.u_min[0]);
      m.u_max[0] = (double)(f.u_max[0] = (float)m.u_max[0]);
    }
  } else if (d->model == ILQR_MODEL_DOUBLE_INTEGRATOR) {
    DoubleIntegratorModel& m = h->dint;
    const double g0[4] = {1.0, 0.5, 0.0, 0.0};
    for (int i = 0; i < 4; i++) m.goal[i] = d->goal ? d->goal[i] : g0[i];
    for (int j = 0; j < 2; j++) {
      m.u_min[j] = d->u_min ? d->u_min[j] : -0.5;
      m.u_max[j] = d->u_max ? d->u_max[j] : 0.5;
    }
    if (h->dtype == ILQR_DTYPE_F32) {
      DoubleIntegratorModelT<float>& f = h->dint_f;
      for (int i = 0; i < 4; i++) m.goal[i] = (double)(f.goal[i] = (float)m.goal[i]);
      for (int j = 0; j < 2; j++) {
        m.u_min[j] = (double)(f.u_min[j] = (float)m.u_min[j]);
        m.u_max[j] = (double)(f.u_max[j] = (float)m.u_max[j]);
      }
    }
#ifdef ILQR_HAVE_USER_MODEL
  } else if (d->model == ILQR_MODEL_USER) {
    using UM = UserModelT<double>;
    h->user_f.set_params(d->user_params, d->n_user_params);
    if (h->dtype == ILQR_DTYPE_F32) {  // the twin the finite differences are taken in: built from the parameters' FLOAT values, like the shipped models'
      std::vector<double> p32(d->user_params, d->user_params + (d->user_params ? d->n_user_params : 0));
      for (double& q : p32) q = (double)(float)q;
      h->user.set_params(p32.data(), (int)p32.size());
    } else {
      h->user.set_params(d->user_params, d->n_user_params);
    }
    for (int j = 0; j < UM::NU; j++) {
      h->user_f.u_min[j] = (float)d->u_min[j];
      h->user_f.u_max[j] = (float)d->u_max[j];
      // fp32 handle: the double twin carries the float model's limits (its other parameters are whatever set_params made of them)
      h->user.u_min[j] = (h->dtype == ILQR_DTYPE_F32) ? (double)h->user_f.u_min[j] : d->u_min[j];
      h->user.u_max[j] = (h->dtype == ILQR_DTYPE_F32) ? (double)h->user_f.u_max[j] : d->u_max[j];
    }
    static_cast<UM&>(h->user_g) = h->user;  // the generic kernels' copy: parameters AND limits (a model's cost may read its own u_min / u_max)
    static_cast<UserModelT<float>&>(h->user_gf) = h->user_f;  // ... and on an fp32 handle the float twin its rollouts integrate
#endif
  }
}

// every device array of the handle, zero-filled on its stream
static int alloc_arrays(const ilqr_desc* d, ilqr_batch* h) {
  const size_t nt = h->ntiles, T = h->T, T1 = h->T + 1, nx = h->nx, nu = h->nu, REC = rec_of(h), Bp = h->Bp;
  BatchView& v = h->v;
  v.B = h->B; v.Bp = h->Bp; v.ntiles = h->ntiles; v.T = h->T; v.dt = h->dt;
  v.analytic = (h->flags & ILQR_FLAG_ANALYTIC_DERIVATIVES) ? 1 : 0;
  v.D = nullptr;  // on first use (ensure_records): the fused LQ route never needs it
  int rc = 0;
  if (h->aos) {
    const size_t Bn = h->B;
    v.nch = 0;
    rc |= dev_alloc_real(h, &v.x0, Bn * nx);  // (fp32 handles: float arrays)
    rc |= dev_alloc_real(h, &v.xs, Bn * T1 * nx);
    rc |= dev_alloc_real(h, &v.us, Bn * T * nu);
    rc |= dev_alloc_real(h, &v.kff, Bn * T * nu);
    rc |= dev_alloc_real(h, &v.Kfb, Bn * T * nu * nx);
    // (double on every handle; GN zeros behind the two records: the knot k_analytic_lq forms knot T's unused cx from at creation)
    rc |= dev_alloc(h, &h->const_rec, 2 * REC + GN);
    rc |= dev_alloc(h, &h->d_umin, nu);
    rc |= dev_alloc(h, &h->d_umax, nu);
    v.cand_u = nullptr;
    v.cand_x = nullptr;
    if (lq_matrix_core_search(d->model, d->nu, d->route) && !(d->route & ILQR_ROUTE_LQ_RECOMMIT) && d->dtype == ILQR_DTYPE_F64) {
      // the eleven rollouts of the matrix-core search, whole ([b][alpha][t][row]): the commit is then a copy, not a twelfth rollout
      // (11 x the nominal trajectory, ~7 GB at configs[4]: if the device cannot spare them the handle works without -- the ILQR_ROUTE_LQ_RECOMMIT route)
      void *cx = nullptr, *cu = nullptr;
      if (hipMalloc(&cx, Bn * NALPHA * T1 * nx * sizeof(double)) == hipSuccess && hipMalloc(&cu, Bn * NALPHA * T * nu * sizeof(double)) == hipSuccess) {
        h->allocs.push_back(cx);
        h->allocs.push_back(cu);
        v.cand_x = (double*)cx;
        v.cand_u = (double*)cu;
      } else {
        if (cx) (void)hipFree(cx);
        (void)hipGetLastError();  // (clears the allocation error)
      }
    }
  } else {
    rc |= dev_alloc_real(h, &v.x0, nt * nx * TW);
    // (+ the spare rows the shared-row rollouts prefetch from past T - 1, rollout.hpp)
    const size_t slack = rollout_fetch_slack_elems(h->nx, h->nu);
    rc |= dev_alloc_real(h, &v.xs, nt * T1 * nx * TW + slack);
    rc |= dev_alloc_real(h, &v.us, nt * T * nu * TW + slack);
    rc |= dev_alloc_real(h, &v.kff, nt * T * nu * TW + slack);
    rc |= dev_alloc_real(h, &v.Kfb, nt * T * nu * nx * TW + slack);
    v.nch = h->T / CT + 1;
    // (one plane more than there are alphas: where the rollout lanes without a rollout of their own put their stores, rollout.hpp)
    // (the matrix-core kernel keeps its candidates in groups of CG controls, a plane row padded to whole chunks past T - 1: rollout.hpp, cand_g_u)
    rc |= dev_alloc_real(h, &v.cand_u, (size_t)(NALPHA + 1) * nt * (size_t)(cand_groups(T) * CG) * nu * TW);
    rc |= dev_alloc_real(h, &v.cand_x, (size_t)(NALPHA + 1) * nt * v.nch * nx * TW);
  }
  rc |= dev_alloc(h, &v.cost_c, (size_t)NALPHA * Bp);  // the 11 candidate costs (device or caller-evaluated)
  // the per-trajectory scalars
  for (double** p : {&v.cost, &v.lambda, &v.dlambda, &v.gnorm}) rc |= dev_alloc(h, p, Bp);
  for (int** p : {&v.status, &v.iters, &v.flg_change, &v.alpha_idx, &v.diverge, &v.backpass_done, &h->commit_idx}) rc |= dev_alloc(h, p, Bp);
  rc |= dev_alloc(h, &v.dV, 2 * Bp);
  rc |= dev_alloc(h, &v.n_running, 1);
  rc |= dev_alloc(h, &h->x0_stage, (size_t)h->B * nx);
  rc |= dev_alloc(h, &h->phase_ticks, 5 * (size_t)h->ntiles);
  if (rc) return ILQR_ERR_HIP;
  HIPCHK(hipMemsetAsync(h->commit_idx, 0xFF, Bp * sizeof(int), h->stream));
  sync_float_view(h);
  return 0;
}

// generic handles: the LQ model's matrices, zero-padded to the kernels' maximum dimensions, and the limits
static int upload_generic_model(const ilqr_desc* d, ilqr_batch* h) {
  if (!h->aos) return 0;
  const size_t nx = h->nx, nu = h->nu;
  // (hp, hf, lim: alive until the synchronisation below)
  std::vector<double> hp;
  std::vector<float> hf;
  if (d->model == ILQR_MODEL_LQ) {
    // B and R: GM columns, or GMW for the wide twin
    const size_t GMC = h->lq_wide ? GMW : GM;
    const size_t nA = GN * GN, nB = GN * GMC, nR = GMC * GMC, tot = 3 * nA + nB + nR;
    double* pad = nullptr;
    if (int rc = dev_alloc(h, &pad, tot)) return rc;
    hp.assign(tot, 0.0);
    double *pA = hp.data(), *pB = pA + nA, *pQ = pB + nB, *pR = pQ + nA, *pQf = pR + nR;
    for (size_t i = 0; i < nx; i++) {
      for (size_t j = 0; j < nx; j++) {
        pA[i * GN + j] = d->lq_A[i * nx + j];
        pQ[i * GN + j] = d->lq_Q[i * nx + j];
        pQf[i * GN + j] = d->lq_Qf[i * nx + j];
      }
      for (size_t j = 0; j < nu; j++) pB[i * GMC + j] = d->lq_B[i * nu + j];
    }
    for (size_t i = 0; i < nu; i++)
      for (size_t j = 0; j < nu; j++) pR[i * GMC + j] = d->lq_R[i * nu + j];
    // fp32 handle: the float matrices its rollouts integrate, and their values in the double twin (finite differences, exact
    // derivatives, backward pass), as set_model_params does for the other models' parameters
    if (h->dtype == ILQR_DTYPE_F32) {
      float* padf = nullptr;
      if (int rc = dev_alloc(h, &padf, tot)) return rc;
      hf.resize(tot);
      for (size_t e = 0; e < tot; e++) hp[e] = (double)(hf[e] = (float)hp[e]);
      HIPCHK(hipMemcpyAsync(padf, hf.data(), tot * sizeof(float), hipMemcpyHostToDevice, h->stream));
      bind_lq(h->lq_f, padf, GMC, h);
    }
    // on the handle's stream, behind dev_alloc's zero fill of the same buffer (a copy on the null
    // stream could be overtaken by it: the stream is non-blocking)
    HIPCHK(hipMemcpyAsync(pad, hp.data(), tot * sizeof(double), hipMemcpyHostToDevice, h->stream));
    bind_lq(h->lq, pad, GMC, h);
    bind_lq(h->lq_w, pad, GMC, h);
  }
  // fp32 handle: the limits' float values (the float rollouts clamp to them, the double backward pass boxes with them)
  std::vector<double> lim(d->u_min, d->u_min + nu);
  lim.insert(lim.end(), d->u_max, d->u_max + nu);
  if (h->dtype == ILQR_DTYPE_F32)
    for (double& q : lim) q = (double)(float)q;
  HIPCHK(hipMemcpyAsync(h->d_umin, lim.data(), nu * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_umax, lim.data() + nu, nu * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// the kernels of every stage, the solver parameters, and every trajectory's state reset (plus the LQ model's constant records)
static int plan_and_reset(const ilqr_desc* d, ilqr_batch* h) {
  h->plan = plan_route({d->model, d->nx, d->nu, d->flags, d->route, h->ntiles, h->num_cus, kUserTiled, kUserSmall, h->v.cand_x != nullptr, d->dtype});
  SolverParams& sp = h->sp;
  const ilqr_params& p = h->params;
  sp.max_iter = p.max_iter; sp.tol_fun = p.tol_fun; sp.tol_grad = p.tol_grad; sp.z_min = p.z_min;
  sp.lambda_factor = p.lambda_factor; sp.lambda_max = p.lambda_max; sp.lambda_min = p.lambda_min;
  sp.fixed_work = (h->flags & ILQR_FLAG_FIXED_WORK) ? 1 : 0;
  sp.fixes = ((h->flags & ILQR_FLAG_REFERENCE_FIXES) ? 3 : 0) | ((h->flags & ILQR_FLAG_REGULARIZE_VXX) ? 4 : 0);
  if (int rc = launch_per_slot(h, k_reset_state<double>, h->v, p.lambda_init, p.dlambda_init)) return rc;
  if (h->plan.derivatives == Derivatives::fused_lq) {  // both constant records, once (what = 3), in double on every handle
    BatchView cv = h->v;
    if (h->dtype == ILQR_DTYPE_F32) cv.xs = h->const_rec + 2 * rec_of(h);  // (an fp32 handle's xs holds floats: the zero knot behind the records)
    hipLaunchKernelGGL(k_analytic_lq<double>, dim3(1), dim3(64), 0, h->stream, cv, h->lq, 1, 3, h->const_rec, kAnalyticChunk);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

static int create_impl(const ilqr_desc* d, ilqr_batch* h) {
  copy_desc(d, h);
  if (int rc = open_device(d, h)) return rc;
  set_model_params(d, h);
  if (int rc = alloc_arrays(d, h)) return rc;
  if (int rc = upload_generic_model(d, h)) return rc;
  return plan_and_reset(d, h);
}

int ilqr_create(const ilqr_desc* d, ilqr_batch** out) {
  if (!d || !out) return fail(ILQR_ERR_INVALID, "null argument");
  *out = nullptr;
  if (int rc = check_desc(d)) return rc;
  ilqr_batch* h = new ilqr_batch();
  const int rc = create_impl(d, h);
  if (rc) {
    char keep[sizeof(g_err)];
    memcpy(keep, g_err, sizeof(keep));
    if (rc != ILQR_ERR_NO_DEVICE) ilqr_destroy(h); else delete h;
    memcpy(g_err, keep, sizeof(keep));
    return rc;
  }
  *out = h;
  return 0;
}

int ilqr_set_stream(ilqr_batch* h, void* s) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->own_stream) {
    HIPCHK(hipStreamDestroy(h->stream));
    h->own_stream = false;
  }
  if (s) {
    h->stream = (hipStream_t)s;
  } else {
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
  }
  return 0;
}

int ilqr_synchronize(ilqr_batch* h) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---- whole-solve entry points --------------------------------------------------------------
int ilqr_init_traj(ilqr_batch* h, const double* x0, const double* u0, double* cost_out) {
  if (!h || !x0 || !u0) return fail(ILQR_ERR_INVALID, "null argument");
  if (host_model(h)) return no_device_model();
  HIPCHK(hipSetDevice(h->device));
  if (int rc = upload(h, x0, {h->v.x0, 1, h->nx})) return rc;
  if (int rc = upload(h, u0, {h->v.us, h->T, h->nu})) return rc;  // us = u_0, ilqr_core.cpp:17
  if (int rc = fresh_trajectory(h)) return rc;
  // ilqr_core.cpp:20: open-loop rollout (K is empty); writes xs, us, cost in place
  AlphaSet al = line_search_alphas();
  if (int rc = launch_rollout(h, false, false, al, 1, h->v.cost, 0)) return rc;
  h->initialised = true;
  if (cost_out) return scalars_to_host(h, h->v.cost, cost_out);
  return 0;
}

int ilqr_iterate(ilqr_batch* h, int n_iters) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (host_model(h)) return no_device_model();
  if (!h->initialised) return fail(ILQR_ERR_STATE, "ilqr_iterate before ilqr_init_traj/ilqr_set_trajectory");
  HIPCHK(hipSetDevice(h->device));
  struct Chain {  // stage timers share their boundary events for the duration of this call
    ilqr_batch* h;
    explicit Chain(ilqr_batch* hh) : h(hh) { h->chain_timers = true; h->chain_event = nullptr; }
    ~Chain() { h->chain_timers = false; h->chain_event = nullptr; }
  } chain(h);
  if (n_iters > 0) h->cands = (h->active_tiles > 0 && h->active_tiles < h->ntiles) ? Cands::none : Cands::planes;  // (a compacted chunk rolls out the leading tiles only)
  if (h->plan.solve != Solve::none && n_iters > 0) {
    if (int rc = launch_solve_tiles(h, n_iters)) return rc;
    return flush_commit(h);
  }
  for (int it = 0; it < n_iters; it++) {
    if (h->plan.sweep != Sweep::none) {
      if (int rc = launch_sweep_backward(h, 1, h->sp.fixed_work)) return rc;  // STEP 1 + STEP 2
    } else {
      if (int rc = launch_derivatives(h, h->sp.fixed_work)) return rc;  // STEP 1
      if (int rc = launch_backward(h, 1)) return rc;                    // STEP 2
    }
    if (h->plan.rollout == Rollout::tiled || h->plan.rollout == Rollout::lq_accept) {
      // STEP 3 + STEP 3/4 in one launch: the rollout block of a tile, or k_rollout_lq<RG_SEARCH, true>, also accepts
      if (int rc = launch_rollout(h, true, true, line_search_alphas(), NALPHA, h->v.cost_c, 1, true)) return rc;
      h->commit_pending = true;
    } else {
      if (int rc = do_rollout_candidates(h, 1)) return rc;              // STEP 3
      if (int rc = launch_accept(h)) return rc;                         // STEP 3/4
    }
  }
  if (!h->aos && n_iters > 0) h->recs = ilqr_batch::REC_STALE;  // (D lags the nominal after an accept, on every route)
  return flush_commit(h);  // the last iteration's accepted trajectories
}

int ilqr_count_running(ilqr_batch* h, int* n) {
  if (!h || !n) return fail(ILQR_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  std::vector<int> st(h->B);
  if (int rc = scalars_to_host(h, h->v.status, st.data())) return rc;
  int c = 0;
  for (int s : st) c += (s == 0);
  *n = c;
  return 0;
}

// Slot j <- slot perm[j] for every per-trajectory array a running solve carries (tiled: x0, xs, us, k, K; scalars: cost,
// lambda, dlambda, dV, gnorm, status, iters, flgChange, alpha index, diverge, backpass_done).  Candidates and derivative
// records are not moved: no accept is pending between ilqr_iterate calls, the records are recomputed when asked for, and
// the candidates are marked as nobody's (ilqr_get_candidate then fails with ILQR_ERR_STATE until the next rollout).
static int apply_permutation(ilqr_batch* h, const std::vector<int>& perm) {
  const size_t es = elem_size(h), Bp = (size_t)h->Bp;
  const size_t biggest = std::max<size_t>((size_t)h->ntiles * (h->T + 1) * h->nx * TW, (size_t)h->ntiles * h->T * h->nu * h->nx * TW) * es;
  const size_t need = std::max<size_t>(biggest, 2 * Bp * sizeof(double));
  if (h->perm_scratch_bytes < need) {
    if (h->perm_scratch) HIPCHK(hipFree(h->perm_scratch));
    h->perm_scratch = nullptr;
    HIPCHK(hipMalloc(&h->perm_scratch, need));
    h->perm_scratch_bytes = need;
  }
  if (!h->d_perm) HIPCHK(hipMalloc((void**)&h->d_perm, Bp * sizeof(int)));
  HIPCHK(hipMemcpyAsync(h->d_perm, perm.data(), Bp * sizeof(int), hipMemcpyHostToDevice, h->stream));
  auto tiled = [&](void* arr, int S, int E) -> int {
    const size_t n = (size_t)h->ntiles * S * E * TW;
    with_real(h, [&](auto r) {
      using real = decltype(r);
      hipLaunchKernelGGL(k_permute_tiled<real>, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, (const real*)arr, (real*)h->perm_scratch, h->d_perm, h->ntiles, S, E);
      return 0;
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(arr, h->perm_scratch, n * es, hipMemcpyDeviceToDevice, h->stream));
    return 0;
  };
  auto scalar = [&](auto* arr, size_t n) -> int {
    using T = std::remove_pointer_t<decltype(arr)>;
    hipLaunchKernelGGL(k_permute_scalar<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const T*)arr, (T*)h->perm_scratch, h->d_perm, (int)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(arr, h->perm_scratch, n * sizeof(T), hipMemcpyDeviceToDevice, h->stream));
    return 0;
  };
  BatchView& v = h->v;
  int rc = 0;
  rc |= tiled(v.x0, 1, h->nx);
  rc |= tiled(v.xs, h->T + 1, h->nx);
  rc |= tiled(v.us, h->T, h->nu);
  rc |= tiled(v.kff, h->T, h->nu);
  rc |= tiled(v.Kfb, h->T, h->nu * h->nx);
  rc |= scalar(v.cost, Bp);
  rc |= scalar(v.lambda, Bp);
  rc |= scalar(v.dlambda, Bp);
  rc |= scalar(v.dV, Bp);
  rc |= scalar(v.dV + Bp, Bp);
  rc |= scalar(v.gnorm, Bp);
  rc |= scalar(v.status, Bp);
  rc |= scalar(v.iters, Bp);
  rc |= scalar(v.flg_change, Bp);
  rc |= scalar(v.alpha_idx, Bp);
  rc |= scalar(v.diverge, Bp);
  rc |= scalar(v.backpass_done, Bp);
  if (rc) return rc;
  h->recs = ilqr_batch::REC_STALE;
  h->cands = Cands::none;  // the candidates stayed where they were
  return 0;
}

int ilqr_generate_trajectory(ilqr_batch* h) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (!h->initialised) return fail(ILQR_ERR_STATE, "generate_trajectory needs x0/xs/us (asserts of ilqr_core.cpp:80-82)");
  // Intra-tile compaction (the reference's own TODO, notes.md:16): a tile costs what its slowest trajectory costs, and with
  // more tiles than the device holds at once (ntiles > #CU) every tile that still has ONE running trajectory takes a slot.
  // So a big batch is solved in chunks of iterations; after a chunk, if the running trajectories would fit into at most
  // half of the tiles that are still launched, they are re-packed into the leading tiles (one permutation pass over
  // the per-trajectory arrays, ~0.1 ms per 4096 trajectories), and only those tiles are launched from then on.  The
  // original order is restored before returning.  Trajectories never interact and no kernel's arithmetic depends on a
  // trajectory's slot: statuses, iteration counts and costs are bit-identical (tests/test_gpu_full_solves.py).
  const bool persistent = h->plan.solve != Solve::none;
  const bool compacting = persistent && h->ntiles > h->num_cus && !(h->sp.fixed_work) && !h->route.no_compaction;
  int done_iters = 0;
  const int chunk = persistent ? (compacting ? std::min(std::max(1, h->params.max_iter), 8) : std::max(1, h->params.max_iter)) : 10;  // (a persistent tile stops by itself)
  std::vector<int> slot_orig;  // slot j currently holds original trajectory slot_orig[j] (empty: identity)
  h->active_tiles = h->ntiles;
  // Every exit of the chunk loop -- also a failing HIP call -- goes through the restore below: the handle is never left
  // with permuted slots or a subset of tiles behind the caller's back.
  auto chunks = [&]() -> int {
  while (done_iters < h->params.max_iter) {
    const int n = std::min(chunk, h->params.max_iter - done_iters);
    if (int rc = ilqr_iterate(h, n)) return rc;
    done_iters += n;
    int running = 0;
    HIPCHK(hipMemcpyAsync(&running, h->v.n_running, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (running == 0) break;
    if (compacting && done_iters < h->params.max_iter && 2 * ((running + TW - 1) / TW) <= h->active_tiles && h->active_tiles > 1) {
      std::vector<int> st(h->Bp);
      HIPCHK(hipMemcpyAsync(st.data(), h->v.status, (size_t)h->Bp * sizeof(int), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      if (slot_orig.empty()) {
        slot_orig.resize(h->Bp);
        for (int j = 0; j < h->Bp; j++) slot_orig[j] = j;
      }
      std::vector<int> perm;
      perm.reserve(h->Bp);
      for (int j = 0; j < h->Bp; j++)
        if (st[j] == 0) perm.push_back(j);
      const int n_run = (int)perm.size();
      for (int j = 0; j < h->Bp; j++)
        if (st[j] != 0) perm.push_back(j);
      if (int rc = apply_permutation(h, perm)) {
        h->initialised = false;  // a half-applied permutation: the arrays no longer describe one batch
        return rc;
      }
      std::vector<int> so(h->Bp);
      for (int j = 0; j < h->Bp; j++) so[j] = slot_orig[perm[j]];
      slot_orig.swap(so);
      h->active_tiles = std::max(1, (n_run + TW - 1) / TW);
    }
  }
  return 0;
  };
  const int rc_out = chunks();
  h->active_tiles = h->ntiles;
  if (!slot_orig.empty() && h->initialised) {  // back to the caller's order: slot o <- the slot that holds original trajectory o
    std::vector<int> back(h->Bp);
    for (int j = 0; j < h->Bp; j++) back[slot_orig[j]] = j;
    if (int rc = apply_permutation(h, back)) {
      h->initialised = false;  // (stage calls and getters of trajectories then fail with ILQR_ERR_STATE instead of reporting the wrong order)
      return rc_out ? rc_out : rc;
    }
  }
  return rc_out;
}

int ilqr_solve(ilqr_batch* h, const double* x0, const double* u0) {
  if (int rc = ilqr_init_traj(h, x0, u0, nullptr)) return rc;
  return ilqr_generate_trajectory(h);
}

// The warm rollout, forward_pass(x_0, us) with the stored gains: u = us[t] + K[t](x - xs[t]) (every alpha 0), written into xs / us -- by the
// rollout itself on the generic path (slot commit_idx = 0 of `al` for everyone), by a commit of slot 0 on the tiled one.  repeat
// (ilqr_mpc_step_reset's second pass): commit_idx already says who is rolled out again (k_select_reset); a tiled rollout scores whole
// tiles, so its costs go through a scratch row (cost_c's first plane: the candidates are nobody's during a step)
static int warm_rollout_commit(ilqr_batch* h, bool repeat) {
  AlphaSet al;
  for (int i = 0; i < NALPHA; i++) al.a[i] = 0.0;
  if (h->plan.commit != Commit::tiled) {
    if (!repeat) HIPCHK(hipMemsetAsync(h->commit_idx, 0, (size_t)h->Bp * sizeof(int), h->stream));
    if (int rc = launch_rollout(h, true, true, al, 1, h->v.cost, 0)) return rc;
  } else {
    if (int rc = launch_rollout(h, true, true, al, 1, repeat ? h->v.cost_c : h->v.cost, 0)) return rc;
    if (!repeat) HIPCHK(hipMemsetAsync(h->commit_idx, 0, (size_t)h->Bp * sizeof(int), h->stream));
    if (int rc = launch_commit(h)) return rc;
    if (repeat) {
      hipLaunchKernelGGL(k_take_reset_cost, dim3((h->B + 255) / 256), dim3(256), 0, h->stream, h->v.cost_c, reset_sel(h), h->v.cost, h->B);
      HIPCHK(hipGetLastError());
    }
  }
  HIPCHK(hipMemsetAsync(h->commit_idx, 0xFF, (size_t)h->Bp * sizeof(int), h->stream));
  return 0;
}

int ilqr_warm_start(ilqr_batch* h, const double* x0) {
  if (!h || !x0) return fail(ILQR_ERR_INVALID, "null argument");
  if (host_model(h)) return no_device_model();
  if (!h->initialised) return fail(ILQR_ERR_STATE, "warm start needs a previous solve (assert us.size()>0, ilqr_core.cpp:66)");
  HIPCHK(hipSetDevice(h->device));
  if (int rc = upload(h, x0, {h->v.x0, 1, h->nx})) return rc;
  if (int rc = warm_rollout_commit(h, false)) return rc;
  // a new outer loop starts: status/iters/flgChange reset, lambda & dlambda persist (file statics)
  if (int rc = launch_per_slot(h, k_warm_reset<double>, h->v)) return rc;
  return ilqr_generate_trajectory(h);
}

// ---- receding horizon (ABI 6) ----------------------------------------------------------------
// Every per-knot array of the nominal (xs, us, k, K) moves `shift` knots toward t = 0 in place (k_shift_horizon, layout.hpp); the tail rule of
// include/ilqr_amd.h.  Cost, lambda, status and iteration counts stay.  Enqueued on the handle's stream, nothing waited for.
static int shift_nominal(ilqr_batch* h, int shift, int tail) {
  if (int rc = nominal_changes(h)) return rc;
  if (shift == 0) return 0;
  const NominalArrays n = nominal_arrays(h);
  const int tails[4] = {SHIFT_TAIL_HOLD, tail, SHIFT_TAIL_ZERO, tail};  // xs[T] is repeated under either tail, k's is zero
  ShiftSet set;
  for (int i = 0; i < 4; i++) set.arr[i] = {n.arr[i].p, n.arr[i].S, n.arr[i].W, tails[i]};
  set.nseg = n.nseg;
  set.shift = shift;
  const dim3 grid((unsigned)std::min(set.nseg, 65535), 4), block(256);
  with_real(h, [&](auto r) {
    hipLaunchKernelGGL(k_shift_horizon<decltype(r)>, grid, block, 0, h->stream, set);
    return 0;
  });
  HIPCHK(hipGetLastError());
  return 0;
}
static int check_shift(ilqr_batch* h, int shift, int tail) {
  REQUIRE(shift >= 0 && shift < h->T, "shift %d: 0 <= shift < T = %d", shift, h->T);
  REQUIRE(tail == ILQR_TAIL_HOLD || tail == ILQR_TAIL_ZERO, "tail %d: ILQR_TAIL_HOLD or ILQR_TAIL_ZERO", tail);
  return 0;
}

int ilqr_shift_horizon(ilqr_batch* h, int shift, int tail) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (int rc = check_shift(h, shift, tail)) return rc;
  if (!h->initialised) return fail(ILQR_ERR_STATE, "shift_horizon before ilqr_init_traj/ilqr_set_trajectory: there is no nominal to shift");
  HIPCHK(hipSetDevice(h->device));
  return shift_nominal(h, shift, tail == ILQR_TAIL_HOLD ? SHIFT_TAIL_HOLD : SHIFT_TAIL_ZERO);
}

int ilqr_copy_controls_to_device(ilqr_batch* h, int t0, int n_knots, void* u_device) {
  if (!h || !u_device) return fail(ILQR_ERR_INVALID, "null argument");
  REQUIRE(t0 >= 0 && n_knots >= 1 && t0 + n_knots <= h->T, "control window [%d, %d): inside [0, T = %d), at least one knot", t0, t0 + n_knots, h->T);
  if (!h->initialised) return fail(ILQR_ERR_STATE, "copy_controls_to_device before ilqr_init_traj/ilqr_set_trajectory");
  HIPCHK(hipSetDevice(h->device));
  return to_canonical(h, {h->v.us, h->T, h->nu, t0, n_knots}, (double*)u_device);
}

// ---- single trajectories start over (additive under ABI 6; reset.hpp) ---------------
static int check_reset_args(const int* mask, const void* mask_device, int rules, const char* who) {
  REQUIRE(!(mask && mask_device), "%s: at most one of mask (host) and mask_device", who);
  REQUIRE((rules & ~(ILQR_RESET_NONFINITE | ILQR_RESET_LAMBDA_MAX)) == 0, "%s: rules %d: bits of ILQR_RESET_NONFINITE | ILQR_RESET_LAMBDA_MAX", who, rules);
  return 0;
}
// the mask where the kernels read it: a host mask goes to the handle's own buffer on the stream, a device mask is read where it lies
static int stage_reset_mask(ilqr_batch* h, const int* mask, const void* mask_device, const int** out) {
  if (!h->reset_ints)
    if (int rc = dev_alloc(h, &h->reset_ints, 3 * (size_t)h->Bp)) return rc;
  *out = (const int*)mask_device;
  if (mask) {
    HIPCHK(hipMemcpyAsync(reset_mask_stage(h), mask, (size_t)h->B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    *out = reset_mask_stage(h);
  }
  return 0;
}
// k_select_reset, then k_reset_nominal for whom it selected.  repeat: the pass after a warm rollout (non-finite costs only; commit_idx says
// whom the repeated rollout takes).
static int select_and_reset(ilqr_batch* h, const int* d_mask, int rules, int repeat) {
  if (int rc = launch_per_slot(h, k_select_reset<double>, h->v, d_mask, rules, repeat, h->params.lambda_init, h->params.dlambda_init, reset_sel(h),
                               reset_flags(h), h->commit_idx))
    return rc;
  const NominalArrays n = nominal_arrays(h);
  const void* const src[4] = {nullptr, h->reset_us_set ? h->reset_us : nullptr, nullptr, nullptr};  // what a selected element becomes (null: zero)
  ResetSet set;
  for (int i = 0; i < 4; i++) set.arr[i] = {n.arr[i].p, src[i], n.arr[i].S, n.arr[i].W};
  set.sel = reset_sel(h);
  set.nseg = n.nseg;  // (sel holds Bp = 16 ntiles >= B slots)
  set.lanes = n.lanes;
  const dim3 grid((unsigned)std::min(set.nseg, 65535), 4), block(256);
  with_real(h, [&](auto r) {
    hipLaunchKernelGGL(k_reset_nominal<decltype(r)>, grid, block, 0, h->stream, set);
    return 0;
  });
  HIPCHK(hipGetLastError());
  h->reset_flags_valid = true;
  return 0;
}

int ilqr_set_reset_controls(ilqr_batch* h, const double* u0, const void* u0_device) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  REQUIRE(!(u0 && u0_device), "ilqr_set_reset_controls: at most one of u0 (host) and u0_device");
  if (!u0 && !u0_device) {  // back to zeros (the buffer stays for the next set)
    h->reset_us_set = false;
    return 0;
  }
  HIPCHK(hipSetDevice(h->device));
  if (!h->reset_us)
    if (int rc = dev_alloc_real(h, &h->reset_us, dev_elems(h, h->T, h->nu))) return rc;
  const DevArray dst{h->reset_us, h->T, h->nu};
  const double* src = (const double*)u0_device;
  if (u0) {  // the host array's one transfer: straight into place where the handle stores the canonical array, else through a buffer of its own
    double* stage = h->reset_us;
    if (!stored_canonical(h, dst)) {
      if (!h->reset_us_stage)
        if (int rc = dev_alloc(h, &h->reset_us_stage, (size_t)h->B * h->T * h->nu)) return rc;
      stage = h->reset_us_stage;
    }
    HIPCHK(hipMemcpyAsync(stage, u0, (size_t)h->B * h->T * h->nu * sizeof(double), hipMemcpyHostToDevice, h->stream));
    src = stage;
  }
  if (int rc = from_canonical(h, src, dst)) return rc;
  h->reset_us_set = true;
  return 0;
}

int ilqr_reset_trajectories(ilqr_batch* h, const int* mask, const void* mask_device, int rules) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (int rc = check_reset_args(mask, mask_device, rules, "ilqr_reset_trajectories")) return rc;
  if (!h->initialised) return fail(ILQR_ERR_STATE, "reset_trajectories before ilqr_init_traj/ilqr_set_trajectory: there is no trajectory to reset");
  HIPCHK(hipSetDevice(h->device));
  if (int rc = nominal_changes(h)) return rc;
  const int* d_mask = nullptr;
  if (int rc = stage_reset_mask(h, mask, mask_device, &d_mask)) return rc;
  return select_and_reset(h, d_mask, rules, 0);
}

// ---- the MPC step (ABI 6), with or without a reset of single trajectories ------------------------------
// x0 into the handle's layout: the host array's one transfer goes to a buffer of its own (the shared staging buffer may be reallocated,
// which waits); a device x0 is read where it lies
static int stage_x0(ilqr_batch* h, const double* x0, const void* x0_device) {
  const DevArray X0{h->v.x0, 1, h->nx};
  const double* src = (const double*)x0_device;
  if (x0) {
    double* dst = stored_canonical(h, X0) ? h->v.x0 : h->x0_stage;
    HIPCHK(hipMemcpyAsync(dst, x0, (size_t)h->B * h->nx * sizeof(double), hipMemcpyHostToDevice, h->stream));
    src = dst;
  }
  return from_canonical(h, src, X0);
}
// every refusal the two step calls share, in the order tests/test_mpc_abi.py pins; each goes on with its own checks
static int check_step_args(ilqr_batch* h, const double* x0, const void* x0_device, int shift, int tail, int n_iters, const char* who) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (host_model(h)) return fail(ILQR_ERR_UNSUPPORTED, "%s: a host-evaluated model's rollouts run on the host (as for ilqr_warm_start)", who);
  REQUIRE((x0 != nullptr) != (x0_device != nullptr), "%s: exactly one of x0 (host) and x0_device", who);
  if (int rc = check_shift(h, shift, tail)) return rc;
  REQUIRE(n_iters >= 0, "n_iters %d must be >= 0", n_iters);
  return 0;
}
// The step: shift -> [reset of the selected] -> x0 -> ilqr_warm_start's rollout and commit -> [under ILQR_RESET_NONFINITE: reset and roll out
// again those whose warm rollout did not stay finite] -> the warm reset -> n_iters iterations.  Everything is enqueued, nothing waited for.
// reset: null for the plain step, which then touches neither reset_ints nor reset_flags_valid and launches no reset kernel.
struct ResetRequest {
  const int* mask;
  const void* mask_device;
  int rules;
};
static int warm_restart(ilqr_batch* h, const double* x0, const void* x0_device, int shift, int tail, int n_iters, const ResetRequest* reset) {
  HIPCHK(hipSetDevice(h->device));
  if (int rc = shift_nominal(h, shift, tail == ILQR_TAIL_HOLD ? SHIFT_TAIL_HOLD : SHIFT_TAIL_ZERO)) return rc;
  if (reset) {  // after the shift: the reset controls are a fresh horizon's, not shifted.  The cost rule waits for the new cost.
    const int* d_mask = nullptr;
    if (int rc = stage_reset_mask(h, reset->mask, reset->mask_device, &d_mask)) return rc;
    if (int rc = select_and_reset(h, d_mask, reset->rules & ILQR_RESET_LAMBDA_MAX, 0)) return rc;
  }
  if (int rc = stage_x0(h, x0, x0_device)) return rc;
  if (int rc = warm_rollout_commit(h, false)) return rc;
  if (reset && (reset->rules & ILQR_RESET_NONFINITE)) {
    if (int rc = select_and_reset(h, nullptr, ILQR_RESET_NONFINITE, 1)) return rc;
    if (int rc = warm_rollout_commit(h, true)) return rc;
  }
  if (int rc = launch_per_slot(h, k_warm_reset<double>, h->v)) return rc;
  return n_iters ? ilqr_iterate(h, n_iters) : 0;
}

// the state ilqr_warm_start leaves on a handle with max_iter = n_iters, without one host synchronisation (ilqr_warm_start waits for its
// x0 and per chunk of iterations)
int ilqr_mpc_step(ilqr_batch* h, const double* x0, const void* x0_device, int shift, int tail, int n_iters) {
  if (int rc = check_step_args(h, x0, x0_device, shift, tail, n_iters, "ilqr_mpc_step")) return rc;
  if (!h->initialised) return fail(ILQR_ERR_STATE, "mpc_step needs a previous solve (assert us.size()>0, ilqr_core.cpp:66)");
  return warm_restart(h, x0, x0_device, shift, tail, n_iters, nullptr);
}

int ilqr_mpc_step_reset(ilqr_batch* h, const double* x0, const void* x0_device, int shift, int tail, int n_iters, const int* mask,
                        const void* mask_device, int rules) {
  if (int rc = check_step_args(h, x0, x0_device, shift, tail, n_iters, "ilqr_mpc_step_reset")) return rc;
  if (int rc = check_reset_args(mask, mask_device, rules, "ilqr_mpc_step_reset")) return rc;
  if (!h->initialised) return fail(ILQR_ERR_STATE, "mpc_step_reset needs a previous solve (assert us.size()>0, ilqr_core.cpp:66)");
  const ResetRequest reset{mask, mask_device, rules};
  return warm_restart(h, x0, x0_device, shift, tail, n_iters, &reset);
}

int ilqr_copy_reset_flags_to_device(ilqr_batch* h, void* flags_device) {
  if (!h || !flags_device) return fail(ILQR_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  if (!h->reset_flags_valid) {  // no reset call yet: nobody was reset
    HIPCHK(hipMemsetAsync(flags_device, 0, (size_t)h->B * sizeof(int), h->stream));
    return 0;
  }
  HIPCHK(hipMemcpyAsync(flags_device, reset_flags(h), (size_t)h->B * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  return 0;
}
int ilqr_get_reset_flags(ilqr_batch* h, int* flags) {
  if (!h || !flags) return fail(ILQR_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  if (!h->reset_flags_valid) {
    for (int b = 0; b < h->B; b++) flags[b] = 0;
    return 0;
  }
  return scalars_to_host(h, (const int*)reset_flags(h), flags);
}

// ---- multi-start groups: the best of a group, cloned over the others (additive under ABI 6; clone.hpp) ---------------
static int check_group(const ilqr_batch* h, int group, const char* who) {
  REQUIRE(group >= 1 && h->B % group == 0, "%s: group %d: at least 1, and a divisor of B = %d", who, group, h->B);
  return 0;
}
static int ensure_clone_ints(ilqr_batch* h) {
  if (h->clone_ints) return 0;
  return dev_alloc(h, &h->clone_ints, 3 * (size_t)h->Bp);
}
// k_select_best into d_src (int32 [B], device memory): one wavefront per group
static int launch_select_best(ilqr_batch* h, int group, int* d_src) {
  const int ngroups = h->B / group;
  hipLaunchKernelGGL(k_select_best, dim3((ngroups + 3) / 4), dim3(256), 0, h->stream, (const double*)h->v.cost, h->B, group, d_src);
  HIPCHK(hipGetLastError());
  return 0;
}
// k_select_clone on the map d_src (who is cloned, and the scalars), then k_clone_nominal for whom it selected
static int select_and_clone(ilqr_batch* h, const int* d_src, const double* du) {
  if (int rc = nominal_changes(h)) return rc;
  if (int rc = launch_per_slot(h, k_select_clone<double>, h->v, d_src, clone_sel(h), clone_flags(h))) return rc;
  const NominalArrays n = nominal_arrays(h);
  CloneSet set;
  set.arr[0] = {h->v.x0, 1, h->nx * n.lanes, nullptr};
  for (int i = 0; i < 4; i++) set.arr[i + 1] = {n.arr[i].p, n.arr[i].S, n.arr[i].W, i == 1 ? du : nullptr};  // (du: the controls' alone)
  set.sel = clone_sel(h);
  set.nseg = n.nseg;  // (sel holds Bp = 16 ntiles >= B slots)
  set.lanes = n.lanes;
  const dim3 grid((unsigned)std::min(set.nseg, 65535), 5), block(256);
  with_real(h, [&](auto r) {
    hipLaunchKernelGGL(k_clone_nominal<decltype(r)>, grid, block, 0, h->stream, set);
    return 0;
  });
  HIPCHK(hipGetLastError());
  h->clone_flags_valid = true;
  return 0;
}

int ilqr_select_best(ilqr_batch* h, int group, int* src, void* src_device) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  REQUIRE((src != nullptr) != (src_device != nullptr), "ilqr_select_best: exactly one of src (host) and src_device");
  if (int rc = check_group(h, group, "ilqr_select_best")) return rc;
  if (!h->initialised) return fail(ILQR_ERR_STATE, "select_best before ilqr_init_traj/ilqr_set_trajectory: there is no cost to compare");
  HIPCHK(hipSetDevice(h->device));
  if (src_device) return launch_select_best(h, group, (int*)src_device);
  if (int rc = ensure_clone_ints(h)) return rc;
  if (int rc = launch_select_best(h, group, clone_map(h))) return rc;
  return scalars_to_host(h, (const int*)clone_map(h), src);
}

int ilqr_clone_trajectories(ilqr_batch* h, const int* src, const void* src_device, const void* du_device) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  REQUIRE((src != nullptr) != (src_device != nullptr), "ilqr_clone_trajectories: exactly one of src (host) and src_device");
  if (!h->initialised) return fail(ILQR_ERR_STATE, "clone_trajectories before ilqr_init_traj/ilqr_set_trajectory: there is no trajectory to clone");
  HIPCHK(hipSetDevice(h->device));
  if (int rc = ensure_clone_ints(h)) return rc;
  const int* d_src = (const int*)src_device;
  if (src) {  // a host map goes to the handle's own buffer on the stream (as stage_reset_mask)
    HIPCHK(hipMemcpyAsync(clone_map(h), src, (size_t)h->B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    d_src = clone_map(h);
  }
  return select_and_clone(h, d_src, (const double*)du_device);
}

int ilqr_clone_best(ilqr_batch* h, int group, const void* du_device) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (int rc = check_group(h, group, "ilqr_clone_best")) return rc;
  if (!h->initialised) return fail(ILQR_ERR_STATE, "clone_best before ilqr_init_traj/ilqr_set_trajectory: there is no trajectory to clone");
  HIPCHK(hipSetDevice(h->device));
  if (int rc = ensure_clone_ints(h)) return rc;
  if (int rc = launch_select_best(h, group, clone_map(h))) return rc;
  return select_and_clone(h, clone_map(h), (const double*)du_device);
}

int ilqr_copy_clone_flags_to_device(ilqr_batch* h, void* flags_device) {
  if (!h || !flags_device) return fail(ILQR_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  if (!h->clone_flags_valid) {  // no clone call yet: nobody was cloned
    HIPCHK(hipMemsetAsync(flags_device, 0, (size_t)h->B * sizeof(int), h->stream));
    return 0;
  }
  HIPCHK(hipMemcpyAsync(flags_device, clone_flags(h), (size_t)h->B * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  return 0;
}
int ilqr_get_clone_flags(ilqr_batch* h, int* flags) {
  if (!h || !flags) return fail(ILQR_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  if (!h->clone_flags_valid) {
    for (int b = 0; b < h->B; b++) flags[b] = 0;
    return 0;
  }
  return scalars_to_host(h, (const int*)clone_flags(h), flags);
}

// ---- the value model of the stored policy (additive under ABI 6) ---------------------------------
// every refusal the two calls share, then the records as ilqr_get_derivatives would return them now
static int prepare_value(ilqr_batch* h, int t0, int n_knots, const void* Vx, const void* Vxx, const char* who) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  REQUIRE(t0 >= 0 && n_knots >= 1 && t0 <= h->T && n_knots <= h->T + 1 - t0, "%s: window [%d, %d): inside [0, T = %d], at least one knot", who, t0, t0 + n_knots, h->T);
  REQUIRE(Vx || Vxx, "%s: Vx and Vxx are both null", who);
  if (!h->initialised) return fail(ILQR_ERR_STATE, "%s before ilqr_init_traj/ilqr_set_trajectory: no policy is stored", who);
  HIPCHK(hipSetDevice(h->device));
  return materialise_records(h);
}
static int run_value(ilqr_batch* h, int t0, int n_knots, double* Vx, double* Vxx, const char* who) {
  return run_launch(who, [&](const char** kernel) { return launch_value(h, t0, n_knots, Vx, Vxx, kernel); });
}

int ilqr_copy_value_to_device(ilqr_batch* h, int t0, int n_knots, void* Vx_device, void* Vxx_device) {
  if (int rc = prepare_value(h, t0, n_knots, Vx_device, Vxx_device, "ilqr_copy_value_to_device")) return rc;
  return run_value(h, t0, n_knots, (double*)Vx_device, (double*)Vxx_device, "ilqr_copy_value_to_device");
}

int ilqr_get_value(ilqr_batch* h, int t0, int n_knots, double* Vx, double* Vxx) {
  if (int rc = prepare_value(h, t0, n_knots, Vx, Vxx, "ilqr_get_value")) return rc;
  // a window-sized device buffer (the staging buffer, laid out by staging.hpp), copied out and waited for
  StagePlan p = stage_value(stage_dims(h), n_knots, Vx, Vxx);
  if (int rc = stage_up(h, p)) return rc;
  if (int rc = run_value(h, t0, n_knots, p.dev(0), p.dev(1), "ilqr_get_value")) return rc;
  return stage_down(h, p);
}

// ---- the closed-loop covariance of the stored policy (additive under ABI 6; covariance_wave.hpp) ------
// every refusal the two calls share -- before anything is enqueued --, then the records as ilqr_get_derivatives would return them now
static int prepare_covariance(ilqr_batch* h, int t0, int n_knots, const void* Sigma, const void* Su, const void* expected_cost, const char* who) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  REQUIRE(t0 >= 0 && n_knots >= 1 && t0 <= h->T && n_knots <= h->T + 1 - t0, "%s: window [%d, %d): inside [0, T = %d], at least one knot", who, t0, t0 + n_knots, h->T);
  REQUIRE(!Su || n_knots <= h->T - t0, "%s: window [%d, %d) with Su: knot T = %d has no control", who, t0, t0 + n_knots, h->T);
  REQUIRE(Sigma || Su || expected_cost, "%s: Sigma, Su and expected_cost are all null", who);
  if (!h->initialised) return fail(ILQR_ERR_STATE, "%s before ilqr_init_traj/ilqr_set_trajectory: no policy is stored", who);
  HIPCHK(hipSetDevice(h->device));
  return materialise_records(h);
}
static int run_covariance(ilqr_batch* h, const CovArgs& q, const char* who) {
  return run_launch(who, [&](const char** kernel) { return launch_covariance(h, q, kernel); });
}

int ilqr_copy_covariance_to_device(ilqr_batch* h, int t0, int n_knots, const void* Sigma0_device, const void* W_device, void* Sigma_device,
                                   void* Su_device, void* expected_cost_device) {
  const char* who = "ilqr_copy_covariance_to_device";
  if (int rc = prepare_covariance(h, t0, n_knots, Sigma_device, Su_device, expected_cost_device, who)) return rc;
  return run_covariance(h, {t0, n_knots, (const double*)Sigma0_device, (const double*)W_device, (double*)Sigma_device, (double*)Su_device, (double*)expected_cost_device}, who);
}

int ilqr_get_covariance(ilqr_batch* h, int t0, int n_knots, const double* Sigma0, const double* W, double* Sigma, double* Su, double* expected_cost) {
  const char* who = "ilqr_get_covariance";
  if (int rc = prepare_covariance(h, t0, n_knots, Sigma, Su, expected_cost, who)) return rc;
  // a call-sized device buffer (the staging buffer, laid out by staging.hpp), the inputs copied up, the outputs copied out and waited for
  StagePlan p = stage_covariance(stage_dims(h), n_knots, Sigma0, W, Sigma, Su, expected_cost);
  if (int rc = stage_up(h, p)) return rc;
  if (int rc = run_covariance(h, {t0, n_knots, p.dev(0), p.dev(1), p.dev(2), p.dev(3), p.dev(4)}, who)) return rc;
  return stage_down(h, p);
}

// ---- the tangent and the adjoint of the stored closed loop (additive under ABI 6; sensitivity_wave.hpp) ------
// every refusal the four calls share -- before anything is enqueued --, then the records as ilqr_get_derivatives would return them now.
// in_x, in_u: the two inputs (dx0, dv / gx, gu), not both null; out_x, out_u: the two outputs, not both null; `windowed_u`: the
// control-sized array that covers the window's nku knots (dus / gu) and so cannot exist when nku == 0.
static int prepare_sensitivity(ilqr_batch* h, int t0, int n_knots, int n_dirs, const void* in_x, const void* in_u, const void* out_x, const void* out_u,
                               const void* windowed_u, const char* in_names, const char* out_names, const char* windowed_name, const char* who) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  REQUIRE(t0 >= 0 && n_knots >= 1 && t0 <= h->T && n_knots <= h->T + 1 - t0, "%s: window [%d, %d): inside [0, T = %d], at least one knot", who, t0, t0 + n_knots, h->T);
  REQUIRE(n_dirs >= 1, "%s: n_dirs %d must be >= 1", who, n_dirs);
  const long long widest = (long long)h->B * (h->T + 1) * n_dirs * std::max(h->nx, h->nu);
  REQUIRE(widest <= (long long)INT_MAX, "%s: B * (T + 1) * n_dirs * max(nx, nu) = %lld elements do not fit an int", who, widest);
  REQUIRE(in_x || in_u, "%s: %s are both null: the answer would be zero", who, in_names);
  REQUIRE(out_x || out_u, "%s: %s are both null", who, out_names);
  REQUIRE(!windowed_u || t0 < h->T, "%s: window [%d, %d) with %s: knot T = %d has no control", who, t0, t0 + n_knots, windowed_name, h->T);
  if (!h->initialised) return fail(ILQR_ERR_STATE, "%s before ilqr_init_traj/ilqr_set_trajectory: no policy is stored", who);
  HIPCHK(hipSetDevice(h->device));
  return materialise_records(h);
}
static int prepare_tangent(ilqr_batch* h, int t0, int n_knots, int n_dirs, const void* dx0, const void* dv, const void* dxs, const void* dus, const char* who) {
  return prepare_sensitivity(h, t0, n_knots, n_dirs, dx0, dv, dxs, dus, dus, "dx0 and dv", "dxs and dus", "dus", who);
}
static int prepare_adjoint(ilqr_batch* h, int t0, int n_knots, int n_dirs, const void* gx, const void* gu, const void* g_x0, const void* g_v, const char* who) {
  return prepare_sensitivity(h, t0, n_knots, n_dirs, gx, gu, g_x0, g_v, gu, "gx and gu", "g_x0 and g_v", "gu", who);
}
static int run_tangent(ilqr_batch* h, const TangentArgs& q, const char* who) {
  return run_launch(who, [&](const char** kernel) { return launch_tangent(h, q, kernel); });
}
static int run_adjoint(ilqr_batch* h, const AdjointArgs& q, const char* who) {
  return run_launch(who, [&](const char** kernel) { return launch_adjoint(h, q, kernel); });
}

int ilqr_copy_tangent_to_device(ilqr_batch* h, int t0, int n_knots, int n_dirs, const void* dx0_device, const void* dv_device, void* dxs_device,
                                void* dus_device) {
  const char* who = "ilqr_copy_tangent_to_device";
  if (int rc = prepare_tangent(h, t0, n_knots, n_dirs, dx0_device, dv_device, dxs_device, dus_device, who)) return rc;
  return run_tangent(h, {t0, n_knots, n_dirs, (const double*)dx0_device, (const double*)dv_device, (double*)dxs_device, (double*)dus_device}, who);
}

int ilqr_get_tangent(ilqr_batch* h, int t0, int n_knots, int n_dirs, const double* dx0, const double* dv, double* dxs, double* dus) {
  const char* who = "ilqr_get_tangent";
  if (int rc = prepare_tangent(h, t0, n_knots, n_dirs, dx0, dv, dxs, dus, who)) return rc;
  StagePlan p = stage_tangent(stage_dims(h), t0, n_knots, n_dirs, dx0, dv, dxs, dus);
  if (int rc = stage_up(h, p)) return rc;
  if (int rc = run_tangent(h, {t0, n_knots, n_dirs, p.dev(0), p.dev(1), p.dev(2), p.dev(3)}, who)) return rc;
  return stage_down(h, p);
}

int ilqr_copy_adjoint_to_device(ilqr_batch* h, int t0, int n_knots, int n_dirs, const void* gx_device, const void* gu_device, void* g_x0_device,
                                void* g_v_device) {
  const char* who = "ilqr_copy_adjoint_to_device";
  if (int rc = prepare_adjoint(h, t0, n_knots, n_dirs, gx_device, gu_device, g_x0_device, g_v_device, who)) return rc;
  return run_adjoint(h, {t0, n_knots, n_dirs, (const double*)gx_device, (const double*)gu_device, (double*)g_x0_device, (double*)g_v_device}, who);
}

int ilqr_get_adjoint(ilqr_batch* h, int t0, int n_knots, int n_dirs, const double* gx, const double* gu, double* g_x0, double* g_v) {
  const char* who = "ilqr_get_adjoint";
  if (int rc = prepare_adjoint(h, t0, n_knots, n_dirs, gx, gu, g_x0, g_v, who)) return rc;
  StagePlan p = stage_adjoint(stage_dims(h), t0, n_knots, n_dirs, gx, gu, g_x0, g_v);
  if (int rc = stage_up(h, p)) return rc;
  if (int rc = run_adjoint(h, {t0, n_knots, n_dirs, p.dev(0), p.dev(1), p.dev(2), p.dev(3)}, who)) return rc;
  return stage_down(h, p);
}

// ---- the LQ subproblem of the records, solved for the caller's linear terms (additive under ABI 6; lq_solve_wave.hpp) ------
// every refusal the two calls share -- before anything is enqueued --, then the records as ilqr_get_derivatives would return them now
static int prepare_lq_solve(ilqr_batch* h, int n_dirs, int flags, double mu, const void* dx0, const void* gx, const void* gu, const void* dxs, const void* dus,
                            const void* dlam, const char* who) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  REQUIRE(n_dirs >= 1, "%s: n_dirs %d must be >= 1", who, n_dirs);
  REQUIRE((flags & ~ILQR_LQ_HOLD_CLAMPED) == 0, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~ILQR_LQ_HOLD_CLAMPED));
  REQUIRE(mu >= 0.0 && mu <= 1.7976931348623157e308, "%s: mu %g must be finite and >= 0", who, mu);
  REQUIRE(dx0 || gx || gu, "%s: dx0, gx and gu are all null: the answer would be zero", who);
  REQUIRE(dxs || dus || dlam, "%s: dxs, dus and dlam are all null", who);
  const long long widest = (long long)h->B * (h->T + 1) * n_dirs * std::max(h->nx, h->nu);
  REQUIRE(widest <= (long long)INT_MAX, "%s: B * (T + 1) * n_dirs * max(nx, nu) = %lld elements do not fit an int", who, widest);
  if (!h->initialised) return fail(ILQR_ERR_STATE, "%s before ilqr_init_traj/ilqr_set_trajectory: no records are stored", who);
  HIPCHK(hipSetDevice(h->device));
  return materialise_records(h);
}
// The scratch of one call (include/ilqr_amd.h states the formula), carved up; then the three kernels.  Bs: trajectories the scratch is laid
// out for (the tiled kernels index [knot][element][Bp]).
static int run_lq_solve(ilqr_batch* h, int n_dirs, int flags, double mu, const double* dx0, const double* gx, const double* gu, double* dxs, double* dus,
                        double* dlam, int* info, const char* who) {
  const size_t Bs = h->aos ? (size_t)h->B : (size_t)h->Bp, T = (size_t)h->T, n = (size_t)h->nx, m = (size_t)h->nu;
  const size_t n_fail = (Bs + 1) / 2, n_kd = Bs * T * m * n, n_mi = Bs * T * m * m, n_p = dlam ? Bs * (T + 1) * n * n : 0,
               n_kdir = dus ? 0 : (size_t)h->B * T * n_dirs * m;
  if (int rc = ensure_lq_scratch(h, n_fail + n_kd + n_mi + n_p + n_kdir)) return rc;
  double* s = h->lq_scratch;
  LqArgs q;
  q.nd = n_dirs, q.hold = (flags & ILQR_LQ_HOLD_CLAMPED) ? 1 : 0, q.mu = mu;
  q.dx0 = dx0, q.gx = gx, q.gu = gu, q.dxs = dxs, q.dus = dus, q.dlam = dlam, q.info = info;
  q.fail = (int*)s;
  q.Kd = s + n_fail;
  q.Mi = q.Kd + n_kd;
  q.P = dlam ? q.Mi + n_mi : nullptr;
  q.kd = dus ? dus : q.Mi + n_mi + n_p;
  return run_launch(who, [&](const char** kernel) { return launch_lq_solve(h, q, kernel); });
}

int ilqr_solve_lq_on_device(ilqr_batch* h, int n_dirs, int flags, double mu, const void* dx0_device, const void* gx_device, const void* gu_device,
                            void* dxs_device, void* dus_device, void* dlam_device, void* info_device) {
  const char* who = "ilqr_solve_lq_on_device";
  if (int rc = prepare_lq_solve(h, n_dirs, flags, mu, dx0_device, gx_device, gu_device, dxs_device, dus_device, dlam_device, who)) return rc;
  return run_lq_solve(h, n_dirs, flags, mu, (const double*)dx0_device, (const double*)gx_device, (const double*)gu_device, (double*)dxs_device,
                      (double*)dus_device, (double*)dlam_device, (int*)info_device, who);
}

int ilqr_solve_lq(ilqr_batch* h, int n_dirs, int flags, double mu, const double* dx0, const double* gx, const double* gu, double* dxs, double* dus,
                  double* dlam, int* info) {
  const char* who = "ilqr_solve_lq";
  if (int rc = prepare_lq_solve(h, n_dirs, flags, mu, dx0, gx, gu, dxs, dus, dlam, who)) return rc;
  // a call-sized device buffer (the staging buffer, laid out by staging.hpp), the inputs copied up, the outputs copied out and waited for
  StagePlan p = stage_lq_solve(stage_dims(h), n_dirs, dx0, gx, gu, dxs, dus, dlam, info);
  if (int rc = stage_up(h, p)) return rc;
  if (int rc = run_lq_solve(h, n_dirs, flags, mu, p.dev(0), p.dev(1), p.dev(2), p.dev(3), p.dev(4), p.dev(5), (int*)p.dev(6), who)) return rc;
  return stage_down(h, p);
}

// ---- the Kalman filter of the stored linearisation and the output-feedback covariance (additive under ABI 6; estimator_wave.hpp) ------
// every refusal the two calls share -- before anything is enqueued --, then the records as ilqr_get_derivatives would return them now
static int prepare_estimator(ilqr_batch* h, int t0, int n_knots, int ny, const void* H, const void* V, const void* Pp, const void* Pf, const void* L,
                             const void* Sigma, const void* Su, const void* expected_cost, const char* who) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  REQUIRE(ny >= 1 && ny <= h->nx, "%s: ny %d must be in [1, nx = %d]", who, ny, h->nx);
  REQUIRE(H && V, "%s: H and V are required", who);
  REQUIRE(t0 >= 0 && n_knots >= 1 && t0 <= h->T && n_knots <= h->T + 1 - t0, "%s: window [%d, %d): inside [0, T = %d], at least one knot", who, t0, t0 + n_knots, h->T);
  REQUIRE(!Su || n_knots <= h->T - t0, "%s: window [%d, %d) with Su: knot T = %d has no control", who, t0, t0 + n_knots, h->T);
  REQUIRE(Pp || Pf || L || Sigma || Su || expected_cost, "%s: Pp, Pf, L, Sigma, Su and expected_cost are all null", who);
  const long long widest = (long long)h->B * (h->T + 1) * h->nx * h->nx;
  REQUIRE(widest <= (long long)INT_MAX, "%s: B * (T + 1) * nx * nx = %lld elements do not fit an int", who, widest);
  if (!h->initialised) return fail(ILQR_ERR_STATE, "%s before ilqr_init_traj/ilqr_set_trajectory: no records are stored", who);
  HIPCHK(hipSetDevice(h->device));
  return materialise_records(h);
}
// The scratch of one call (include/ilqr_amd.h states the formula), carved up; then the kernels.
static int run_estimator(ilqr_batch* h, EstArgs q, const char* who) {
  const size_t n_fail = ((size_t)h->B + 1) / 2;
  const size_t n_mat = (h->aos && est_closed(q)) ? (size_t)h->B * (est_last_knot(q, h->T) + 1) * h->nx * h->nx : 0;
  if (int rc = ensure_est_scratch(h, n_fail + 2 * n_mat)) return rc;
  q.fail = (int*)h->est_scratch;
  q.Pfs = n_mat ? h->est_scratch + n_fail : nullptr;
  q.Ns = n_mat ? q.Pfs + n_mat : nullptr;
  return run_launch(who, [&](const char** kernel) { return launch_estimator(h, q, kernel); });
}

int ilqr_copy_estimator_to_device(ilqr_batch* h, int t0, int n_knots, int ny, const void* H_device, const void* P0_device, const void* W_device,
                                  const void* V_device, void* Pp_device, void* Pf_device, void* L_device, void* Sigma_device, void* Su_device,
                                  void* expected_cost_device, void* info_device) {
  const char* who = "ilqr_copy_estimator_to_device";
  if (int rc = prepare_estimator(h, t0, n_knots, ny, H_device, V_device, Pp_device, Pf_device, L_device, Sigma_device, Su_device, expected_cost_device, who)) return rc;
  return run_estimator(h, {t0, n_knots, ny, (const double*)H_device, (const double*)P0_device, (const double*)W_device, (const double*)V_device,
                           (double*)Pp_device, (double*)Pf_device, (double*)L_device, (double*)Sigma_device, (double*)Su_device,
                           (double*)expected_cost_device, (int*)info_device, nullptr, nullptr, nullptr}, who);
}

int ilqr_get_estimator(ilqr_batch* h, int t0, int n_knots, int ny, const double* H, const double* P0, const double* W, const double* V, double* Pp,
                       double* Pf, double* L, double* Sigma, double* Su, double* expected_cost, int* info) {
  const char* who = "ilqr_get_estimator";
  if (int rc = prepare_estimator(h, t0, n_knots, ny, H, V, Pp, Pf, L, Sigma, Su, expected_cost, who)) return rc;
  // a call-sized device buffer (the staging buffer, laid out by staging.hpp), the inputs copied up, the outputs copied out and waited for
  StagePlan p = stage_estimator(stage_dims(h), n_knots, ny, H, P0, W, V, Pp, Pf, L, Sigma, Su, expected_cost, info);
  if (int rc = stage_up(h, p)) return rc;
  if (int rc = run_estimator(h, {t0, n_knots, ny, p.dev(0), p.dev(1), p.dev(2), p.dev(3), p.dev(4), p.dev(5), p.dev(6), p.dev(7), p.dev(8), p.dev(9),
                                 (int*)p.dev(10), nullptr, nullptr, nullptr}, who))
    return rc;
  return stage_down(h, p);
}

// ---- the risk-sensitive (LEQG) gains and value of the records' LQ model (additive under ABI 6; risk_wave.hpp) ------
// every refusal the two calls share -- before anything is enqueued --, then the records as ilqr_get_derivatives would return them now
static int prepare_risk(ilqr_batch* h, int nw, double theta, int flags, double mu, const void* C, const void* K, const void* k, const void* Vx,
                        const void* Vxx, const void* risk_cost, const char* who) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  REQUIRE(nw >= 1 && nw <= h->nx, "%s: nw %d must be in [1, nx = %d]", who, nw, h->nx);
  REQUIRE(C != nullptr, "%s: C is required", who);
  REQUIRE((flags & ~ILQR_LQ_HOLD_CLAMPED) == 0, "%s: unknown flag bits 0x%x", who, (unsigned)(flags & ~ILQR_LQ_HOLD_CLAMPED));
  REQUIRE(mu >= 0.0 && mu <= 1.7976931348623157e308, "%s: mu %g must be finite and >= 0", who, mu);
  REQUIRE(theta >= -1.7976931348623157e308 && theta <= 1.7976931348623157e308, "%s: theta %g must be finite", who, theta);
  REQUIRE(K || k || Vx || Vxx || risk_cost, "%s: K, k, Vx, Vxx and risk_cost are all null", who);
  const long long widest = (long long)h->B * (h->T + 1) * h->nx * h->nx;
  REQUIRE(widest <= (long long)INT_MAX, "%s: B * (T + 1) * nx * nx = %lld elements do not fit an int", who, widest);
  if (!h->initialised) return fail(ILQR_ERR_STATE, "%s before ilqr_init_traj/ilqr_set_trajectory: no records are stored", who);
  HIPCHK(hipSetDevice(h->device));
  return materialise_records(h);
}
// The failure marks are the only scratch; then the kernel.
static int run_risk(ilqr_batch* h, RiskArgs q, const char* who) {
  if (!h->risk_fail)
    if (int rc = dev_alloc(h, &h->risk_fail, (size_t)h->Bp)) return rc;
  q.fail = h->risk_fail;
  return run_launch(who, [&](const char** kernel) { return launch_risk(h, q, kernel); });
}

int ilqr_copy_risk_sensitive_to_device(ilqr_batch* h, int nw, double theta, int flags, double mu, const void* C_device, void* K_device, void* k_device,
                                       void* Vx_device, void* Vxx_device, void* risk_cost_device, void* info_device) {
  const char* who = "ilqr_copy_risk_sensitive_to_device";
  if (int rc = prepare_risk(h, nw, theta, flags, mu, C_device, K_device, k_device, Vx_device, Vxx_device, risk_cost_device, who)) return rc;
  return run_risk(h, {nw, (flags & ILQR_LQ_HOLD_CLAMPED) ? 1 : 0, theta, mu, (const double*)C_device, (double*)K_device, (double*)k_device,
                      (double*)Vx_device, (double*)Vxx_device, (double*)risk_cost_device, (int*)info_device, nullptr}, who);
}

int ilqr_get_risk_sensitive(ilqr_batch* h, int nw, double theta, int flags, double mu, const double* C, double* K, double* k, double* Vx, double* Vxx,
                            double* risk_cost, int* info) {
  const char* who = "ilqr_get_risk_sensitive";
  if (int rc = prepare_risk(h, nw, theta, flags, mu, C, K, k, Vx, Vxx, risk_cost, who)) return rc;
  // a call-sized device buffer (the staging buffer, laid out by staging.hpp), C copied up, the outputs copied out and waited for
  StagePlan p = stage_risk(stage_dims(h), nw, C, K, k, Vx, Vxx, risk_cost, info);
  if (int rc = stage_up(h, p)) return rc;
  if (int rc = run_risk(h, {nw, (flags & ILQR_LQ_HOLD_CLAMPED) ? 1 : 0, theta, mu, p.dev(0), p.dev(1), p.dev(2), p.dev(3), p.dev(4), p.dev(5),
                            (int*)p.dev(6), nullptr}, who))
    return rc;
  return stage_down(h, p);
}

// ---- the stored policy applied to caller-given states (additive under ABI 6; evaluate.hpp) ------
// every refusal the two calls share -- before anything is enqueued --, then an accepted candidate still waiting is copied (as shift_nominal)
static int prepare_evaluate(ilqr_batch* h, int t0, int n_knots, int n_samples, int flags, const void* x, const void* cost, const void* x_end,
                            const void* u_first, const char* who) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  REQUIRE(x != nullptr, "%s: null x", who);
  REQUIRE(cost || x_end || u_first, "%s: cost, x_end and u_first are all null", who);
  REQUIRE(t0 >= 0 && n_knots >= 1 && t0 <= h->T && n_knots <= h->T - t0, "%s: window [%d, %d): inside [0, T = %d], at least one knot", who, t0, t0 + n_knots, h->T);
  REQUIRE(n_samples >= 1, "%s: n_samples %d must be >= 1", who, n_samples);
  REQUIRE((long long)h->B * n_samples <= (long long)INT_MAX, "%s: B * n_samples = %d * %d rollouts do not fit an int", who, h->B, n_samples);
  REQUIRE((flags & ~ILQR_EVAL_CLAMP) == 0, "%s: flags %d: bits of ILQR_EVAL_CLAMP", who, flags);
  if (host_model(h)) return fail(ILQR_ERR_UNSUPPORTED, "%s: a host-evaluated model exists on the host only (as for ilqr_warm_start)", who);
  if (!h->initialised) return fail(ILQR_ERR_STATE, "%s before ilqr_init_traj/ilqr_set_trajectory: no policy is stored", who);
  HIPCHK(hipSetDevice(h->device));
  return flush_commit(h);
}
static int run_evaluate(ilqr_batch* h, const EvalArgs& e, const char* who) {
  return run_launch(who, [&](const char** kernel) { return launch_evaluate(h, e, kernel); });
}
static int eval_clamp(const ilqr_batch* h, int flags) { return ((flags & ILQR_EVAL_CLAMP) || (h->sp.fixes & 1)) ? 1 : 0; }

int ilqr_evaluate_policy_on_device(ilqr_batch* h, int t0, int n_knots, int n_samples, int flags, const void* x_device, void* cost_device,
                                   void* x_end_device, void* u_first_device) {
  const char* who = "ilqr_evaluate_policy_on_device";
  if (int rc = prepare_evaluate(h, t0, n_knots, n_samples, flags, x_device, cost_device, x_end_device, u_first_device, who)) return rc;
  return run_evaluate(h, {t0, n_knots, n_samples, eval_clamp(h, flags), (const double*)x_device, (double*)cost_device, (double*)x_end_device, (double*)u_first_device}, who);
}

int ilqr_evaluate_policy(ilqr_batch* h, int t0, int n_knots, int n_samples, int flags, const double* x, double* cost, double* x_end,
                         double* u_first) {
  const char* who = "ilqr_evaluate_policy";
  if (int rc = prepare_evaluate(h, t0, n_knots, n_samples, flags, x, cost, x_end, u_first, who)) return rc;
  // a call-sized device buffer (the staging buffer, laid out by staging.hpp), x copied up, the outputs copied out and waited for
  StagePlan p = stage_evaluate(stage_dims(h), n_samples, x, cost, x_end, u_first);
  if (int rc = stage_up(h, p)) return rc;
  if (int rc = run_evaluate(h, {t0, n_knots, n_samples, eval_clamp(h, flags), p.dev(0), p.dev(1), p.dev(2), p.dev(3)}, who)) return rc;
  return stage_down(h, p);
}

// ---- per-trajectory model parameters (additive under ABI 6) ------------------------------------
int ilqr_trajectory_params_count(void) { return kUserNTP; }

// every refusal the three handle calls share; 0: this handle's kernels take per-trajectory rows
static int check_trajectory_params(const ilqr_batch* h, const char* who) {
  if (h->model != ILQR_MODEL_USER)
    return fail(ILQR_ERR_UNSUPPORTED, "%s: per-trajectory parameters belong to a user device twin (ILQR_MODEL_USER); this handle's model is %d", who, h->model);
  if (!h->aos) {
    if (h->nx == 4)
      return fail(ILQR_ERR_UNSUPPORTED, "%s: an nx = 4 twin runs the persistent tiled kernels, which keep one model for all trajectories; per-trajectory "
                                        "parameters need the generic wavefront-per-trajectory kernels (a twin of another shape)", who);
    return fail(ILQR_ERR_UNSUPPORTED, "%s: this handle runs the tiled small-twin kernels, which keep one model for all trajectories; create it with "
                                      "ILQR_ROUTE_WAVE_PER_TRAJECTORY (the generic wavefront-per-trajectory kernels)", who);
  }
  if (kUserNTP == 0)
    return fail(ILQR_ERR_UNSUPPORTED, "%s: this build's user model declares no per-trajectory parameters (NTP, set_trajectory_params: csrc/models.hpp)", who);
  if (!takes_trajectory_params(h->plan))
    return fail(ILQR_ERR_UNSUPPORTED, "%s: this handle's route does not run k_rollout_g / k_derivatives_g", who);
  return 0;
}

int ilqr_set_trajectory_params(ilqr_batch* h, const double* p, const void* p_device, int n) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (int rc = check_trajectory_params(h, "ilqr_set_trajectory_params")) return rc;
  REQUIRE((p != nullptr) != (p_device != nullptr), "ilqr_set_trajectory_params: exactly one of p (host) and p_device");
  REQUIRE(n == kUserNTP, "ilqr_set_trajectory_params: n = %d, this build's user model takes NTP = %d parameters per trajectory", n, kUserNTP);
  HIPCHK(hipSetDevice(h->device));
  const size_t elems = (size_t)h->B * kUserNTP;
  if (!h->traj_params)
    if (int rc = dev_alloc(h, &h->traj_params, elems)) return rc;
  HIPCHK(hipMemcpyAsync(h->traj_params, p ? (const void*)p : p_device, elems * sizeof(double), p ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->stream));
  h->plan.traj_params = ModelRows::per_trajectory;  // (out of knot mode, if the handle was in it: its window stays allocated)
  return 0;
}

int ilqr_get_trajectory_params(ilqr_batch* h, double* p, int n) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (int rc = check_trajectory_params(h, "ilqr_get_trajectory_params")) return rc;
  REQUIRE(p != nullptr, "ilqr_get_trajectory_params: null array");
  REQUIRE(n == kUserNTP, "ilqr_get_trajectory_params: n = %d, this build's user model takes NTP = %d parameters per trajectory", n, kUserNTP);
  if (h->plan.traj_params == ModelRows::per_knot)
    return fail(ILQR_ERR_STATE, "ilqr_get_trajectory_params: per-knot rows are set (ilqr_set_knot_params): ilqr_get_knot_params returns them");
  if (h->plan.traj_params != ModelRows::per_trajectory)
    return fail(ILQR_ERR_STATE, "ilqr_get_trajectory_params: no per-trajectory parameters are set (every trajectory uses ilqr_create's)");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(p, h->traj_params, (size_t)h->B * kUserNTP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

int ilqr_clear_trajectory_params(ilqr_batch* h) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (int rc = check_trajectory_params(h, "ilqr_clear_trajectory_params")) return rc;
  h->plan.traj_params = ModelRows::none;  // (either mode; the rows stay allocated for the next set)
  return 0;
}

// ---- per-knot model parameters (additive under ABI 6) ---------------------------
int ilqr_set_knot_params(ilqr_batch* h, const double* p, const void* p_device, int n, int n_knots, int k0) {
  REQUIRE((p != nullptr) != (p_device != nullptr), "ilqr_set_knot_params: exactly one of p (host) and p_device");
  REQUIRE(n_knots >= 1, "ilqr_set_knot_params: n_knots %d must be >= 1", n_knots);
  REQUIRE(k0 >= 0 && k0 < n_knots, "ilqr_set_knot_params: k0 %d outside [0, n_knots = %d)", k0, n_knots);
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (int rc = check_trajectory_params(h, "ilqr_set_knot_params")) return rc;
  REQUIRE(n == kUserNTP, "ilqr_set_knot_params: n = %d, this build's user model takes NTP = %d parameters per knot", n, kUserNTP);
  const long long window = (long long)h->B * (h->T + 1) * kUserNTP;
  REQUIRE(window <= (long long)INT_MAX, "ilqr_set_knot_params: B * (T + 1) * NTP = %lld elements do not fit an int", window);
  HIPCHK(hipSetDevice(h->device));
  if (!h->knot_params)
    if (int rc = dev_alloc(h, &h->knot_params, (size_t)window)) return rc;
  const double* src = (const double*)p_device;
  if (p) {  // the whole reference up into the handle's scratch, then the same gather
    const size_t elems = (size_t)h->B * n_knots * kUserNTP;
    if (int rc = ensure_knot_stage(h, elems)) return rc;
    HIPCHK(hipMemcpyAsync(h->knot_stage, p, elems * sizeof(double), hipMemcpyHostToDevice, h->stream));
    src = h->knot_stage;
  }
  hipLaunchKernelGGL(k_gather_knot_params, dim3((unsigned)((window + 255) / 256)), dim3(256), 0, h->stream, h->knot_params, src, h->B, h->T + 1,
                     kUserNTP, n_knots, k0);
  HIPCHK(hipGetLastError());
  h->plan.traj_params = ModelRows::per_knot;
  return 0;
}

int ilqr_get_knot_params(ilqr_batch* h, double* p, int n) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (int rc = check_trajectory_params(h, "ilqr_get_knot_params")) return rc;
  REQUIRE(p != nullptr, "ilqr_get_knot_params: null array");
  REQUIRE(n == kUserNTP, "ilqr_get_knot_params: n = %d, this build's user model takes NTP = %d parameters per knot", n, kUserNTP);
  if (h->plan.traj_params != ModelRows::per_knot)
    return fail(ILQR_ERR_STATE, "ilqr_get_knot_params: no per-knot rows are set (ilqr_set_knot_params)");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(p, h->knot_params, (size_t)h->B * (h->T + 1) * kUserNTP * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---- the gradient of a caller's loss with respect to the per-trajectory parameters (additive under ABI 6; param_gradient.hpp) ------
// every refusal the two calls share -- before anything is enqueued; the argument checks need no handle and come first --, then the nominal
// and the records as ilqr_get_trajectory / ilqr_get_derivatives would return them now
static int prepare_param_gradient(ilqr_batch* h, int n_dirs, int flags, double eps_p, const void* dxs, const void* dus, const void* dlam, const void* gp,
                                  const void* lam, const char* who) {
  REQUIRE(n_dirs >= 1, "%s: n_dirs %d must be >= 1", who, n_dirs);
  REQUIRE(flags == 0, "%s: unknown flag bits 0x%x", who, (unsigned)flags);
  REQUIRE(eps_p >= 0.0 && eps_p <= 1.7976931348623157e308, "%s: eps_p %g must be finite and >= 0", who, eps_p);
  REQUIRE(dxs || dus || dlam, "%s: dxs, dus and dlam are all null: the answer would be zero", who);
  REQUIRE(gp || lam, "%s: gp and lam are both null", who);
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (int rc = check_trajectory_params(h, who)) return rc;
  const long long widest = (long long)h->B * (h->T + 1) * n_dirs * std::max(std::max(h->nx, h->nu), kUserNTP);
  REQUIRE(widest <= (long long)INT_MAX, "%s: B * (T + 1) * n_dirs * max(nx, nu, NTP) = %lld elements do not fit an int", who, widest);
  if (!h->initialised) return fail(ILQR_ERR_STATE, "%s before ilqr_init_traj/ilqr_set_trajectory: no trajectory is stored", who);
  if (h->plan.traj_params == ModelRows::per_knot)  // (never the per-trajectory buffer of an earlier mode)
    return fail(ILQR_ERR_UNSUPPORTED, "%s: per-knot rows are set (ilqr_set_knot_params); the gradient is defined for per-trajectory rows only", who);
  if (h->plan.traj_params != ModelRows::per_trajectory)
    return fail(ILQR_ERR_STATE, "%s: no per-trajectory parameters are set (ilqr_create's user_params have no mapping onto the NTP fields)", who);
  HIPCHK(hipSetDevice(h->device));
  if (int rc = flush_commit(h)) return rc;
  return materialise_records(h);
}
// The scratch of one call (include/ilqr_amd.h states the formula), carved up; then the kernels
static int run_param_gradient(ilqr_batch* h, int n_dirs, double eps_p, const double* dxs, const double* dus, const double* dlam, double* gp, double* lam,
                              const char* who) {
  const size_t nchunk = ((size_t)h->T + 1 + kPgChunk - 1) / kPgChunk;
  const size_t n_lam = lam ? 0 : (size_t)h->B * (h->T + 1) * h->nx, n_part = gp ? (size_t)h->B * nchunk * n_dirs * kUserNTP : 0;
  if (int rc = ensure_pg_scratch(h, n_lam + n_part)) return rc;
  PgArgs a;
  a.nd = n_dirs, a.nchunk = (int)nchunk, a.eps_p = eps_p == 0.0 ? 1e-3 : eps_p;
  a.dxs = dxs, a.dus = dus, a.dlam = dlam, a.gp = gp;
  a.lam = lam ? lam : h->pg_scratch;
  a.part = h->pg_scratch + n_lam;
  return run_launch(who, [&](const char** kernel) { return launch_param_gradient(h, a, kernel); });
}

int ilqr_param_gradient_on_device(ilqr_batch* h, int n_dirs, int flags, double eps_p, const void* dxs_device, const void* dus_device,
                                  const void* dlam_device, void* gp_device, void* lam_device) {
  const char* who = "ilqr_param_gradient_on_device";
  if (int rc = prepare_param_gradient(h, n_dirs, flags, eps_p, dxs_device, dus_device, dlam_device, gp_device, lam_device, who)) return rc;
  return run_param_gradient(h, n_dirs, eps_p, (const double*)dxs_device, (const double*)dus_device, (const double*)dlam_device, (double*)gp_device,
                            (double*)lam_device, who);
}

int ilqr_get_param_gradient(ilqr_batch* h, int n_dirs, int flags, double eps_p, const double* dxs, const double* dus, const double* dlam, double* gp,
                            double* lam) {
  const char* who = "ilqr_get_param_gradient";
  if (int rc = prepare_param_gradient(h, n_dirs, flags, eps_p, dxs, dus, dlam, gp, lam, who)) return rc;
  // a call-sized device buffer (the staging buffer, laid out by staging.hpp), the inputs copied up, the outputs copied out and waited for
  StagePlan p = stage_param_gradient(stage_dims(h), n_dirs, dxs, dus, dlam, gp, lam);
  if (int rc = stage_up(h, p)) return rc;
  if (int rc = run_param_gradient(h, n_dirs, eps_p, p.dev(0), p.dev(1), p.dev(2), p.dev(3), p.dev(4), who)) return rc;
  return stage_down(h, p);
}

// ---- stages --------------------------------------------------------------------------------
// what every stage call checks first; device_model: the stage runs the model on the device, which a host-evaluated handle has not got
static int begin_stage(ilqr_batch* h, bool device_model) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (device_model && host_model(h)) return no_device_model();
  HIPCHK(hipSetDevice(h->device));
  if (!h->initialised) return fail(ILQR_ERR_STATE, "stage call before ilqr_init_traj/ilqr_set_trajectory (the reference asserts, ilqr_core.cpp:80-82)");
  return 0;
}
int ilqr_compute_derivatives(ilqr_batch* h) {
  if (int rc = begin_stage(h, true)) return rc;
  return launch_derivatives(h, 1);
}

int ilqr_backward_pass(ilqr_batch* h, int* diverge_out) {
  if (int rc = begin_stage(h, false)) return rc;
  if (int rc = launch_backward(h, 0)) return rc;
  if (diverge_out) return scalars_to_host(h, h->v.diverge, diverge_out);
  return 0;
}

int ilqr_backward_step(ilqr_batch* h) {
  if (int rc = begin_stage(h, false)) return rc;
  return launch_backward(h, 1);
}

int ilqr_rollout_candidates(ilqr_batch* h, double* cost_out) {
  if (int rc = begin_stage(h, true)) return rc;
  if (int rc = do_rollout_candidates(h, 0)) return rc;
  if (cost_out) {
    std::vector<double> tmp((size_t)NALPHA * h->Bp);
    HIPCHK(hipMemcpyAsync(tmp.data(), h->v.cost_c, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int b = 0; b < h->B; b++)
      for (int a = 0; a < NALPHA; a++) cost_out[(size_t)b * NALPHA + a] = tmp[(size_t)a * h->Bp + b];
  }
  return 0;
}

int ilqr_line_search(ilqr_batch* h) {
  if (int rc = begin_stage(h, true)) return rc;
  if (int rc = flush_commit(h)) return rc;
  if (int rc = do_rollout_candidates(h, 1)) return rc;
  if (int rc = launch_accept(h)) return rc;
  return flush_commit(h);
}

int ilqr_accept_candidates(ilqr_batch* h, const double* cost_c, int* accepted) {
  if (!h || !cost_c || !accepted) return fail(ILQR_ERR_INVALID, "null argument");
  if (!h->v.cost_c) return fail(ILQR_ERR_UNSUPPORTED, "this handle has no candidate-cost buffer");
  if (int rc = begin_stage(h, false)) return rc;
  if (int rc = flush_commit(h)) return rc;
  std::vector<double> tmp((size_t)NALPHA * h->Bp, 0.0);
  for (int b = 0; b < h->B; b++)
    for (int a = 0; a < NALPHA; a++) tmp[(size_t)a * h->Bp + b] = cost_c[(size_t)b * NALPHA + a];
  HIPCHK(hipMemcpyAsync(h->v.cost_c, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->v.n_running, 0, sizeof(int), h->stream));  // (the device sweeps do this for k_accept)
  if (int rc = launch_accept(h)) return rc;
  std::vector<int> ci(h->Bp);
  HIPCHK(hipMemcpyAsync(ci.data(), h->commit_idx, (size_t)h->Bp * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemsetAsync(h->commit_idx, 0xFF, (size_t)h->Bp * sizeof(int), h->stream));  // the caller commits
  HIPCHK(hipStreamSynchronize(h->stream));
  h->commit_pending = false;
  for (int b = 0; b < h->B; b++) accepted[b] = ci[b];
  return 0;
}

int ilqr_reset_state(ilqr_batch* h, int warm) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  if (int rc = flush_commit(h)) return rc;
  // warm: a new outer loop on the stored solution -- lambda, dlambda and the gains persist, on the device (k_warm_reset)
  return warm ? launch_per_slot(h, k_warm_reset<double>, h->v) : fresh_trajectory(h);
}

// ---- state exchange --------------------------------------------------------------------------
int ilqr_set_trajectory(ilqr_batch* h, const double* x0, const double* xs, const double* us, const double* cost) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  if (x0) if (int rc = upload(h, x0, {h->v.x0, 1, h->nx})) return rc;
  if (xs) if (int rc = upload(h, xs, {h->v.xs, h->T + 1, h->nx})) return rc;
  if (us) if (int rc = upload(h, us, {h->v.us, h->T, h->nu})) return rc;
  if (cost) if (int rc = scalars_to_dev(h, cost, h->v.cost)) return rc;
  h->initialised = true;
  return 0;
}
int ilqr_set_gains(ilqr_batch* h, const double* k, const double* K) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  if (k) if (int rc = upload(h, k, {h->v.kff, h->T, h->nu})) return rc;
  if (K) if (int rc = upload(h, K, {h->v.Kfb, h->T, h->nu * h->nx})) return rc;
  return 0;
}
int ilqr_set_derivatives(ilqr_batch* h, const double* fx, const double* fu, const double* cx, const double* cu,
                         const double* cxx, const double* cxu, const double* cuu) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  int off[7], len[7];
  rec_offsets(h->nx, h->nu, off, len);
  const double* srcs[7] = {fx, fu, cx, cu, cxx, cxu, cuu};
  for (int i = 0; i < 7; i++)
    if (srcs[i]) if (int rc = upload_rec(h, srcs[i], off[i], len[i])) return rc;
  return 0;
}
int ilqr_set_lambda(ilqr_batch* h, const double* lambda, const double* dlambda) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  if (lambda) if (int rc = scalars_to_dev(h, lambda, h->v.lambda)) return rc;
  if (dlambda) if (int rc = scalars_to_dev(h, dlambda, h->v.dlambda)) return rc;
  return 0;
}

int ilqr_get_trajectory(ilqr_batch* h, double* xs, double* us) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  if (xs) if (int rc = download(h, {h->v.xs, h->T + 1, h->nx}, xs)) return rc;
  if (us) if (int rc = download(h, {h->v.us, h->T, h->nu}, us)) return rc;
  return 0;
}
int ilqr_get_gains(ilqr_batch* h, double* k, double* K) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  if (k) if (int rc = download(h, {h->v.kff, h->T, h->nu}, k)) return rc;
  if (K) if (int rc = download(h, {h->v.Kfb, h->T, h->nu * h->nx}, K)) return rc;
  return 0;
}
int ilqr_get_derivatives(ilqr_batch* h, double* fx, double* fu, double* cx, double* cu, double* cxx, double* cxu,
                         double* cuu) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  int off[7], len[7];
  rec_offsets(h->nx, h->nu, off, len);
  double* dsts[7] = {fx, fu, cx, cu, cxx, cxu, cuu};
  if (int rc = materialise_records(h)) return rc;
  for (int i = 0; i < 7; i++)
    if (dsts[i]) if (int rc = download(h, rec_block(h, off[i], len[i]), dsts[i])) return rc;
  return 0;
}
int ilqr_get_cost(ilqr_batch* h, double* cost) {
  if (!h || !cost) return fail(ILQR_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  return scalars_to_host(h, h->v.cost, cost);
}
int ilqr_get_lambda(ilqr_batch* h, double* lambda, double* dlambda) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  if (lambda) if (int rc = scalars_to_host(h, h->v.lambda, lambda)) return rc;
  if (dlambda) if (int rc = scalars_to_host(h, h->v.dlambda, dlambda)) return rc;
  return 0;
}
int ilqr_get_dV(ilqr_batch* h, double* dV) {
  if (!h || !dV) return fail(ILQR_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  std::vector<double> tmp(2 * (size_t)h->Bp);
  HIPCHK(hipMemcpyAsync(tmp.data(), h->v.dV, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int b = 0; b < h->B; b++) {
    dV[2 * b] = tmp[b];
    dV[2 * b + 1] = tmp[h->Bp + b];
  }
  return 0;
}
int ilqr_get_gnorm(ilqr_batch* h, double* g) {
  if (!h || !g) return fail(ILQR_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  return scalars_to_host(h, h->v.gnorm, g);
}
int ilqr_get_status(ilqr_batch* h, int* status, int* iters, int* alpha_idx) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  if (status) if (int rc = scalars_to_host(h, h->v.status, status)) return rc;
  if (iters) if (int rc = scalars_to_host(h, h->v.iters, iters)) return rc;
  if (alpha_idx) if (int rc = scalars_to_host(h, h->v.alpha_idx, alpha_idx)) return rc;
  return 0;
}
int ilqr_get_candidate(ilqr_batch* h, int a, double* xs, double* us) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  if (host_model(h)) return no_device_model();
  REQUIRE(a >= 0 && a < NALPHA, "alpha index %d out of range", a);
  if (h->cands == Cands::none)
    return fail(ILQR_ERR_STATE, "no candidates: none rolled out yet, or the solve re-packed running trajectories (compaction) and left the "
                                "candidate buffers behind -- call ilqr_rollout_candidates / ilqr_iterate first");
  HIPCHK(hipSetDevice(h->device));
  if (h->aos) {  // generic handles keep candidates only on the LQ matrix-core route: [b][alpha][t][row], whole trajectories
    if (!(h->plan.commit == Commit::lq_copy && h->lq_cands_kept))
      return fail(ILQR_ERR_UNSUPPORTED, "this handle's line search keeps no candidate trajectories (only their costs: ilqr_rollout_candidates)");
    const size_t wx = (size_t)(h->T + 1) * h->nx * sizeof(double), wu = (size_t)h->T * h->nu * sizeof(double);
    if (xs) HIPCHK(hipMemcpy2DAsync(xs, wx, (const char*)h->v.cand_x + (size_t)a * wx, (size_t)NALPHA * wx, wx, h->B, hipMemcpyDeviceToHost, h->stream));
    if (us) HIPCHK(hipMemcpy2DAsync(us, wu, (const char*)h->v.cand_u + (size_t)a * wu, (size_t)NALPHA * wu, wu, h->B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  }
  const size_t nx_el = (size_t)h->B * (h->T + 1) * h->nx, nu_el = (size_t)h->B * h->T * h->nu;
  if (int rc = ensure_staging(h, nx_el + nu_el)) return rc;
  double* dxs = h->staging;
  double* dus = h->staging + nx_el;
  const dim3 grid(grid_for((size_t)h->B * (h->T + 1), 256)), block(256);
  if (int rc = with_model(h, [&](auto& v, auto& m, auto&) {
        using MM = std::decay_t<decltype(m)>;
        constexpr bool kHexModel = MM::NX == 4 && MM::NU == 1;  // k_solve_hex's, the one kernel that groups its candidates
        return with_bool(h->cands == Cands::grouped, [&](auto grouped) {
          hipLaunchKernelGGL((k_unpack_cand<MM, kHexModel && decltype(grouped)::value>), grid, block, 0, h->stream, v, m, a, dxs, dus);
          return 0;
        });
      }))
    return rc;
  HIPCHK(hipGetLastError());
  if (xs) HIPCHK(hipMemcpyAsync(xs, dxs, nx_el * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (us) HIPCHK(hipMemcpyAsync(us, dus, nu_el * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
int ilqr_copy_cost_to_device(ilqr_batch* h, void* dst) {
  if (!h || !dst) return fail(ILQR_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(dst, h->v.cost, (size_t)h->B * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  return 0;
}
int ilqr_copy_trajectory_to_device(ilqr_batch* h, void* xs_dev, void* us_dev) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  if (xs_dev) if (int rc = to_canonical(h, {h->v.xs, h->T + 1, h->nx}, (double*)xs_dev)) return rc;
  if (us_dev) if (int rc = to_canonical(h, {h->v.us, h->T, h->nu}, (double*)us_dev)) return rc;
  return 0;
}
int ilqr_copy_gains_to_device(ilqr_batch* h, void* k_dev, void* K_dev) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  if (k_dev) if (int rc = to_canonical(h, {h->v.kff, h->T, h->nu}, (double*)k_dev)) return rc;
  if (K_dev) if (int rc = to_canonical(h, {h->v.Kfb, h->T, h->nu * h->nx}, (double*)K_dev)) return rc;
  return 0;
}
int ilqr_get_results_async(ilqr_batch* h, double* xs, double* us, double* k, double* K, double* cost) {
  if (!h) return fail(ILQR_ERR_INVALID, "null handle");
  HIPCHK(hipSetDevice(h->device));
  struct Item { DevArray src; double* dst; };
  const Item items[4] = {{{h->v.xs, h->T + 1, h->nx}, xs}, {{h->v.us, h->T, h->nu}, us}, {{h->v.kff, h->T, h->nu}, k}, {{h->v.Kfb, h->T, h->nu * h->nx}, K}};
  // a handle that stores the canonical arrays themselves: straight to the host.  Otherwise every array is converted into a stretch of the
  // staging buffer of its own: the kernels and the copies follow each other on the stream without a host synchronisation in between (the
  // staging buffer is only ever touched by work enqueued on this stream: a later upload is ordered behind these copies)
  size_t total = 0;
  for (const Item& it : items)
    if (it.dst && !stored_canonical(h, it.src)) total += (size_t)h->B * it.src.S * it.src.E;
  if (total)
    if (int rc = ensure_staging(h, total)) return rc;
  size_t off = 0;
  for (const Item& it : items) {
    if (!it.dst) continue;
    const size_t n = (size_t)h->B * it.src.S * it.src.E;
    const double* dev = (const double*)it.src.p;
    if (!stored_canonical(h, it.src)) {
      if (int rc = to_canonical(h, it.src, h->staging + off)) return rc;
      dev = h->staging + off;
      off += n;
    }
    HIPCHK(hipMemcpyAsync(it.dst, dev, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  if (cost) HIPCHK(hipMemcpyAsync(cost, h->v.cost, (size_t)h->B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return 0;
}
int ilqr_host_register(void* ptr, size_t bytes) {
  if (!ptr || !bytes) return fail(ILQR_ERR_INVALID, "null argument");
  HIPCHK(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
  return 0;
}
int ilqr_host_unregister(void* ptr) {
  if (!ptr) return fail(ILQR_ERR_INVALID, "null argument");
  HIPCHK(hipHostUnregister(ptr));
  return 0;
}

}  // extern "C"

#include "group.hpp"
#include "profile.hpp"
