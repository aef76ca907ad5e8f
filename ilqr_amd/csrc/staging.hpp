// staging.hpp -- how each host getter of the stored-model queries lays its arrays out in the handle's staging buffer, as plain data: a
// getter declares its segments (inputs, then outputs, info last), handle.hpp's stage_up / stage_down do every copy.  Host code only:
// tests/test_staging_plan.py builds it with a host compiler.
#pragma once
#include <stddef.h>

namespace ilqr {

// One caller array of a getter.  host null: not given -- no room, no copy, a null device pointer.  An int segment of n ints takes
// (n + 1) / 2 doubles of the buffer and copies n * sizeof(int) bytes.
struct StageSeg {
  void* host;
  size_t count;   // elements copied (0: host is null)
  size_t offset;  // doubles from the start of the buffer: the counts before it, summed in declaration order
  bool up, ints;
  double* dev;    // set by resolve()
  size_t doubles() const { return ints ? (count + 1) / 2 : count; }
  size_t bytes() const { return count * (ints ? sizeof(int) : sizeof(double)); }
};

struct StagePlan {
  static constexpr int kMaxSegs = 11;  // ilqr_get_estimator's
  StageSeg seg[kMaxSegs];
  int n = 0;
  size_t total = 0;  // doubles
  void add(const void* host, size_t count, bool up, bool ints) {
    seg[n] = {const_cast<void*>(host), host ? count : 0, total, up, ints, nullptr};  // (an input is only ever read through host)
    total += seg[n++].doubles();
  }
  void up(const double* host, size_t count) { add(host, count, true, false); }
  void down(double* host, size_t count) { add(host, count, false, false); }
  void down_ints(int* host, size_t count) { add(host, count, false, true); }
  // the segments' device pointers in a buffer of at least `total` doubles
  void resolve(double* base) {
    for (int i = 0; i < n; i++) seg[i].dev = seg[i].host ? base + seg[i].offset : nullptr;
  }
  double* dev(int i) const { return seg[i].dev; }
};

// the sizes every declaration below is written in (ntp: the build's per-trajectory parameter count)
struct StageDims {
  size_t B, T, nx, nu, ntp;
};

// ilqr_get_value: Vx, Vxx
inline StagePlan stage_value(const StageDims& d, size_t nk, double* Vx, double* Vxx) {
  StagePlan p;
  p.down(Vx, d.B * nk * d.nx), p.down(Vxx, d.B * nk * d.nx * d.nx);
  return p;
}
// ilqr_get_covariance: Sigma0, W; Sigma, Su, expected_cost
inline StagePlan stage_covariance(const StageDims& d, size_t nk, const double* Sigma0, const double* W, double* Sigma, double* Su, double* expected_cost) {
  const size_t nn = d.B * d.nx * d.nx;
  StagePlan p;
  p.up(Sigma0, nn), p.up(W, nn), p.down(Sigma, nn * nk), p.down(Su, d.B * nk * d.nu * d.nu), p.down(expected_cost, d.B);
  return p;
}
// the element counts of the four arrays of a tangent or adjoint call: state-sized over one knot, control-sized over the horizon, state-sized
// over the window, control-sized over the window's knots with a control (tangent: dx0, dv, dxs, dus; adjoint: g_x0, g_v, gx, gu)
struct SensSizes {
  size_t x_one, u_all, x_win, u_win;
};
inline SensSizes sensitivity_sizes(const StageDims& d, size_t t0, size_t nk, size_t nd) {
  const size_t per_x = d.B * nd * d.nx, per_u = d.B * nd * d.nu;
  return {per_x, per_u * d.T, per_x * nk, per_u * ((t0 + nk < d.T ? t0 + nk : d.T) - t0)};
}
// ilqr_get_tangent: dx0, dv; dxs, dus
inline StagePlan stage_tangent(const StageDims& d, size_t t0, size_t nk, size_t nd, const double* dx0, const double* dv, double* dxs, double* dus) {
  const SensSizes s = sensitivity_sizes(d, t0, nk, nd);
  StagePlan p;
  p.up(dx0, s.x_one), p.up(dv, s.u_all), p.down(dxs, s.x_win), p.down(dus, s.u_win);
  return p;
}
// ilqr_get_adjoint: gx, gu; g_x0, g_v
inline StagePlan stage_adjoint(const StageDims& d, size_t t0, size_t nk, size_t nd, const double* gx, const double* gu, double* g_x0, double* g_v) {
  const SensSizes s = sensitivity_sizes(d, t0, nk, nd);
  StagePlan p;
  p.up(gx, s.x_win), p.up(gu, s.u_win), p.down(g_x0, s.x_one), p.down(g_v, s.u_all);
  return p;
}
// ilqr_solve_lq: dx0, gx, gu; dxs, dus, dlam, info
inline StagePlan stage_lq_solve(const StageDims& d, size_t nd, const double* dx0, const double* gx, const double* gu, double* dxs, double* dus, double* dlam,
                                int* info) {
  const size_t per_x = d.B * nd * d.nx, per_u = d.B * nd * d.nu;
  StagePlan p;
  p.up(dx0, per_x), p.up(gx, per_x * (d.T + 1)), p.up(gu, per_u * d.T);
  p.down(dxs, per_x * (d.T + 1)), p.down(dus, per_u * d.T), p.down(dlam, per_x * (d.T + 1)), p.down_ints(info, d.B);
  return p;
}
// ilqr_get_estimator: H, P0, W, V; Pp, Pf, L, Sigma, Su, expected_cost, info
inline StagePlan stage_estimator(const StageDims& d, size_t nk, size_t ny, const double* H, const double* P0, const double* W, const double* V, double* Pp,
                                 double* Pf, double* L, double* Sigma, double* Su, double* expected_cost, int* info) {
  const size_t nn = d.B * d.nx * d.nx;
  StagePlan p;
  p.up(H, d.B * ny * d.nx), p.up(P0, nn), p.up(W, nn), p.up(V, d.B * ny * ny);
  p.down(Pp, nn * nk), p.down(Pf, nn * nk), p.down(L, d.B * nk * d.nx * ny), p.down(Sigma, nn * nk), p.down(Su, d.B * nk * d.nu * d.nu);
  p.down(expected_cost, d.B), p.down_ints(info, d.B);
  return p;
}
// ilqr_get_risk_sensitive: C; K, k, Vx, Vxx, risk_cost, info
inline StagePlan stage_risk(const StageDims& d, size_t nw, const double* C, double* K, double* k, double* Vx, double* Vxx, double* risk_cost, int* info) {
  StagePlan p;
  p.up(C, d.B * d.nx * nw), p.down(K, d.B * d.T * d.nu * d.nx), p.down(k, d.B * d.T * d.nu), p.down(Vx, d.B * (d.T + 1) * d.nx);
  p.down(Vxx, d.B * (d.T + 1) * d.nx * d.nx), p.down(risk_cost, d.B), p.down_ints(info, d.B);
  return p;
}
// ilqr_evaluate_policy: x; cost, x_end, u_first
inline StagePlan stage_evaluate(const StageDims& d, size_t n_samples, const double* x, double* cost, double* x_end, double* u_first) {
  const size_t R = d.B * n_samples;
  StagePlan p;
  p.up(x, R * d.nx), p.down(cost, R), p.down(x_end, R * d.nx), p.down(u_first, R * d.nu);
  return p;
}
// ilqr_get_param_gradient: dxs, dus, dlam; gp, lam
inline StagePlan stage_param_gradient(const StageDims& d, size_t nd, const double* dxs, const double* dus, const double* dlam, double* gp, double* lam) {
  const size_t per_x = d.B * nd * d.nx, per_u = d.B * nd * d.nu;
  StagePlan p;
  p.up(dxs, per_x * (d.T + 1)), p.up(dus, per_u * d.T), p.up(dlam, per_x * (d.T + 1)), p.down(gp, d.B * nd * d.ntp), p.down(lam, d.B * (d.T + 1) * d.nx);
  return p;
}

}  // namespace ilqr
