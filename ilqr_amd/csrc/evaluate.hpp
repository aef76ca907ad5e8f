// evaluate.hpp -- the stored feedback policy u = us[t] + K[t](x - xs[t]) applied to caller-given states and rolled through the device
// model (ilqr_evaluate_policy / ilqr_evaluate_policy_on_device; the definition: include/ilqr_amd.h).  One THREAD per rollout on either
// layout.  Rollout r = b S + s is sample s of trajectory b: consecutive lanes take consecutive r, so the per-sample input and outputs
// ([B][S][..] canonical double) are contiguous along the lanes and the lanes of one trajectory read the SAME nominal address (one fetch,
// broadcast).  Nothing is stored per step and nothing of the handle is written: the B S independent rollouts hide the load latency, no
// prefetch ring.  The step of each kernel is the step of the rollout kernel of its layout (rollout_tile's do_step, k_rollout_g's loop
// body) without the alpha k term, through the same device functions: (t0 = 0, n = T) gives the warm start's bits.
#pragma once
#include "generic.hpp"

namespace ilqr {

struct EvalArgs {
  int t0, n, S;     // the window [t0, t0 + n) inside [0, T]; samples per trajectory
  int clamp;        // u clamped to the model's limits before it is costed and integrated (ILQR_EVAL_CLAMP or the handle's fixes bit 0)
  const double* x;  // [B][S][nx]
  double* cost;     // [B][S]       (any of the three may be null)
  double* x_end;    // [B][S][nx]
  double* u_first;  // [B][S][nu]
};

// tiled layout [tile][slot][E][16]: nx = 4 models and twins, small twins; fp64 and fp32 storage
template <class M>
__global__ __launch_bounds__(64) void k_evaluate_t(BatchViewT<typename M::real> v, M model, EvalArgs e) {
  using real = typename M::real;
  constexpr int NX = M::NX, NU = M::NU;
  const size_t r = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= (size_t)v.B * e.S) return;
  const int b = (int)(r / e.S);
  const int tile = b / TW, l = b % TW;
  const int T = v.T;
  const real dt = (real)v.dt;
  real x[NX];
#pragma unroll
  for (int i = 0; i < NX; i++) x[i] = (real)e.x[r * NX + i];
  double total = 0;
  const WithTrigConsts<M> rmodel(model);
  const int t1 = e.t0 + e.n;
  for (int t = e.t0; t < t1; t++) {
    real u[NU], K[NU * NX], xnom[NX];
#pragma unroll
    for (int j = 0; j < NU; j++) u[j] = v.us[tidx(tile, t, j, l, T, NU)];
#pragma unroll
    for (int q = 0; q < NU * NX; q++) K[q] = v.Kfb[tidx(tile, t, q, l, T, NU * NX)];
#pragma unroll
    for (int i = 0; i < NX; i++) xnom[i] = v.xs[tidx(tile, t, i, l, T + 1, NX)];
#pragma unroll
    for (int j = 0; j < NU; j++) {
      real acc = 0;
#pragma unroll
      for (int i = 0; i < NX; i++) acc += K[j + NU * i] * (x[i] - xnom[i]);
      u[j] += acc;  // :316
    }
    if (e.clamp) {
#pragma unroll
      for (int j = 0; j < NU; j++) u[j] = min_of(max_of(u[j], model.u_min[j]), model.u_max[j]);
    }
    if (t == e.t0 && e.u_first) {
#pragma unroll
      for (int j = 0; j < NU; j++) e.u_first[r * NU + j] = (double)u[j];
    }
    total += (double)model.cost(x, u);  // :324
    real x1[NX];
    integrate_dynamics(rmodel, x, u, dt, x1);  // :325
#pragma unroll
    for (int i = 0; i < NX; i++) x[i] = x1[i];
  }
  if (t1 == T) total += (double)model.final_cost(x);  // :335
  if (e.cost) e.cost[r] = total;
  if (e.x_end) {
#pragma unroll
    for (int i = 0; i < NX; i++) e.x_end[r * NX + i] = (double)x[i];
  }
}

// trajectory-contiguous layout: the LQ twins, user twins on the generic kernels; M as k_rollout_g takes it (the float twin on an fp32
// handle).  PT: every sample of trajectory b evaluates the model with row b of the handle's per-trajectory parameters.  PK: with row
// t0 + i of trajectory b's per-knot window at the window's knot i, row T for final_cost (KnotRows, as k_rollout_g walks them).
template <class M, int PT = ROWS_NONE>
__global__ __launch_bounds__(64) void k_evaluate_g(BatchViewT<typename M::real> v, model_arg_t<M, PT> model, EvalArgs e) {
  using real = typename M::real;
  constexpr int NX = M::NX, NU = M::NU;
  const int nx = model.nx, nu = model.nu, T = v.T;
  const size_t r = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (r >= (size_t)v.B * e.S) return;
  const int b = (int)(r / e.S);
  const real dt = (real)v.dt;
  if constexpr (PT == PT_ROWS) {
    double p[M::NTP];
#pragma unroll
    for (int i = 0; i < M::NTP; i++) p[i] = model.traj_params[(size_t)b * M::NTP + i];
    model.set_trajectory_params(p);
  }
  real x[NX];
#pragma unroll
  for (int i = 0; i < NX; i++) x[i] = (i < nx) ? (real)e.x[r * nx + i] : (real)0;
  double total = 0;
  const real* xsb = v.xs + (size_t)b * (T + 1) * nx;
  const real* usb = v.us + (size_t)b * T * nu;
  const real* Kb = v.Kfb + (size_t)b * T * nu * nx;
  const int t1 = e.t0 + e.n;
  KnotRows<M, PT> rows(model, b, T, e.t0);
  for (int t = e.t0; t < t1; t++) {
    rows.next(model);
    real u[NU];
#pragma unroll
    for (int j = 0; j < NU; j++) u[j] = (j < nu) ? usb[(size_t)t * nu + j] : (real)0;
    real d[NX];
#pragma unroll
    for (int i = 0; i < NX; i++) d[i] = (i < nx) ? x[i] - xsb[(size_t)t * nx + i] : (real)0;
    const real* Kt = Kb + (size_t)t * nu * nx;
#pragma unroll
    for (int j = 0; j < NU; j++) {
      if (j < nu) {
        real acc = 0;
#pragma unroll
        for (int i = 0; i < NX; i++)
          if (i < nx) acc += Kt[j + nu * i] * d[i];
        u[j] += acc;  // :316
      }
    }
    if (e.clamp) {
#pragma unroll
      for (int j = 0; j < NU; j++)
        if (j < nu) u[j] = fmin(fmax(u[j], model.limit_lo(j)), model.limit_hi(j));
    }
    if (t == e.t0 && e.u_first) {
#pragma unroll
      for (int j = 0; j < NU; j++)
        if (j < nu) e.u_first[r * nu + j] = (double)u[j];
    }
    total += model.cost(x, u);  // :324
    real x1[NX];
    integrate_dynamics(model, x, u, dt, x1);  // :325
#pragma unroll
    for (int i = 0; i < NX; i++) x[i] = x1[i];
  }
  if (t1 == T) {
    rows.last(model);
    total += model.final_cost(x);  // :335
  }
  if (e.cost) e.cost[r] = total;
  if (e.x_end) {
#pragma unroll
    for (int i = 0; i < NX; i++)
      if (i < nx) e.x_end[r * nx + i] = (double)x[i];
  }
}

}  // namespace ilqr
