// lq_solve_thread.hpp -- ilqr_solve_lq on the tiled layout (nx = 4 models and twins, small twins; fp64 and fp32 storage): the definition
// of include/ilqr_amd.h in registers, stored floats widened where they are loaded, the recursion double.
//     k_lq_gain_t  one THREAD per trajectory: the Riccati sweep with the fixed-size factorisation of lq_solve_wave.hpp (a held control is
//                  an identity row and column with a zero right-hand side), Kd, Mi = -Quu^-1 masked and P into scratch [knot][element][Bp]
//                  -- consecutive lanes, consecutive addresses
//     k_lq_dir_t   one thread per (trajectory, direction), the direction by block as k_tangent_t: v, w, kd backward, then dx, du, dlam
//                  forward; kd rests in the caller's dus (or scratch), v in the caller's dlam, each read by the thread that wrote it
// Every thread runs the same expressions in the same order: column s of the outputs depends on column s of the inputs alone, bit for bit.
#pragma once
#include "common.hpp"
#include "lq_solve_wave.hpp"

namespace ilqr {

template <class M>
__global__ __launch_bounds__(64) void k_lq_gain_t(BatchViewT<typename M::real> v, LqArgs q) {
  using real = typename M::real;
  constexpr int NX = M::NX, NU = M::NU;
  using R = Rec<NX, NU>;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= v.B) return;
  const int tile = b / TW, l = b % TW;
  const int T = v.T;
  const size_t Bs = (size_t)v.Bp;
  const real* Dt = v.D + didx(tile, 0, 0, l, T + 1, R::SIZE);
  auto rec = [&](int t, int e) { return (double)Dt[((size_t)t * (R::SIZE / 2) + (e >> 1)) * (2 * TW) + (e & 1)]; };
  double P[NX * NX];
#pragma unroll
  for (int e = 0; e < NX * NX; e++) P[e] = rec(T, R::CXX + e);
  if (q.P) {
#pragma unroll
    for (int e = 0; e < NX * NX; e++) q.P[((size_t)T * NX * NX + e) * Bs + b] = P[e];
  }
  int failed = 0;
  for (int t = T - 1; t >= 0; t--) {
    double fx[NX * NX], fu[NX * NU], A1[NX * NX], A2[NX * NU], Qxx[NX * NX], Qux[NU * NX], Quu[NU * NU];
    bool held[NU];
#pragma unroll
    for (int e = 0; e < NX * NX; e++) fx[e] = rec(t, R::FX + e);
#pragma unroll
    for (int e = 0; e < NX * NU; e++) fu[e] = rec(t, R::FU + e);
#pragma unroll
    for (int j = 0; j < NU; j++) {
      bool any = !q.hold;
#pragma unroll
      for (int c = 0; c < NX; c++) any = any || !((double)v.Kfb[tidx(tile, t, j + NU * c, l, T, NU * NX)] == 0.0);
      held[j] = !any;
    }
    // A1 = P fx, A2 = P fu
#pragma unroll
    for (int c = 0; c < NX; c++)
#pragma unroll
      for (int a = 0; a < NX; a++) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < NX; r++) s = __builtin_fma(P[a + NX * r], fx[r + NX * c], s);
        A1[a + NX * c] = s;
      }
#pragma unroll
    for (int j = 0; j < NU; j++)
#pragma unroll
      for (int a = 0; a < NX; a++) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < NX; r++) s = __builtin_fma(P[a + NX * r], fu[r + NX * j], s);
        A2[a + NX * j] = s;
      }
    // Qxx = cxx + fx'A1 ; Qux = cxu' + fu'A1 ; Quu = cuu + fu'A2 + mu I
#pragma unroll
    for (int c = 0; c < NX; c++) {
#pragma unroll
      for (int a = 0; a < NX; a++) {
        double s = rec(t, R::CXX + a + NX * c);
#pragma unroll
        for (int r = 0; r < NX; r++) s = __builtin_fma(fx[r + NX * a], A1[r + NX * c], s);
        Qxx[a + NX * c] = s;
      }
#pragma unroll
      for (int j = 0; j < NU; j++) {
        double s = rec(t, R::CXU + c + NX * j);
#pragma unroll
        for (int r = 0; r < NX; r++) s = __builtin_fma(fu[r + NX * j], A1[r + NX * c], s);
        Qux[j + NU * c] = s;
      }
    }
#pragma unroll
    for (int j = 0; j < NU; j++)
#pragma unroll
      for (int i = 0; i < NU; i++) {
        double s = rec(t, R::CUU + i + NU * j);
#pragma unroll
        for (int r = 0; r < NX; r++) s = __builtin_fma(fu[r + NX * i], A2[r + NX * j], s);
        if (i == j) s += q.mu;
        Quu[i + NU * j] = (held[i] || held[j]) ? (i == j ? 1.0 : 0.0) : s;
      }
    // Cholesky, lower, in index order (Lc(i, j) in Quu's lower triangle, the reciprocal diagonal beside it)
    double dinv[NU];
#pragma unroll
    for (int j = 0; j < NU; j++) {
      double piv = Quu[j + NU * j];
#pragma unroll
      for (int k = 0; k < j; k++) piv = __builtin_fma(-Quu[j + NU * k], Quu[j + NU * k], piv);
      if (!failed && (!(piv > 0.0) || piv > 1.7976931348623157e308)) failed = t + 1;
      const double rinv = 1.0 / __builtin_sqrt(piv);
      dinv[j] = rinv;
      Quu[j + NU * j] = piv * rinv;
#pragma unroll
      for (int i = j + 1; i < NU; i++) {
        double s = Quu[i + NU * j];
#pragma unroll
        for (int k = 0; k < j; k++) s = __builtin_fma(-Quu[i + NU * k], Quu[j + NU * k], s);
        Quu[i + NU * j] = s * rinv;
      }
    }
    if (failed) break;
    // column by column: x = -(L L')^-1 rhs for the NX columns of Qux (held rows zero) and the NU of the identity (held columns zero)
    auto solve = [&](double(&y)[NU]) {
#pragma unroll
      for (int i = 0; i < NU; i++) {
        double s = y[i];
#pragma unroll
        for (int k = 0; k < i; k++) s = __builtin_fma(-Quu[i + NU * k], y[k], s);
        y[i] = s * dinv[i];
      }
#pragma unroll
      for (int i = NU - 1; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < NU; k++) s = __builtin_fma(-Quu[k + NU * i], y[k], s);
        y[i] = s * dinv[i];
      }
#pragma unroll
      for (int i = 0; i < NU; i++) y[i] = 0.0 - y[i];
    };
    double Kd[NU * NX];
#pragma unroll
    for (int c = 0; c < NX; c++) {
      double y[NU];
#pragma unroll
      for (int j = 0; j < NU; j++) y[j] = held[j] ? 0.0 : Qux[j + NU * c];
      solve(y);
#pragma unroll
      for (int j = 0; j < NU; j++) {
        Kd[j + NU * c] = y[j];
        q.Kd[((size_t)t * NU * NX + j + NU * c) * Bs + b] = y[j];
      }
    }
#pragma unroll
    for (int c = 0; c < NU; c++) {
      double y[NU];
#pragma unroll
      for (int j = 0; j < NU; j++) y[j] = (j == c && !held[j]) ? 1.0 : 0.0;
      solve(y);
#pragma unroll
      for (int j = 0; j < NU; j++) q.Mi[((size_t)t * NU * NU + j + NU * c) * Bs + b] = y[j];
    }
    // P = sym(Qxx + Qux'Kd)
    double Pn[NX * NX];
#pragma unroll
    for (int c = 0; c < NX; c++)
#pragma unroll
      for (int a = 0; a < NX; a++) {
        double s = Qxx[a + NX * c];
#pragma unroll
        for (int j = 0; j < NU; j++) s = __builtin_fma(Qux[j + NU * a], Kd[j + NU * c], s);
        Pn[a + NX * c] = s;
      }
#pragma unroll
    for (int c = 0; c < NX; c++)
#pragma unroll
      for (int a = 0; a < NX; a++) P[a + NX * c] = 0.5 * (Pn[a + NX * c] + Pn[c + NX * a]);
    if (q.P) {
#pragma unroll
      for (int e = 0; e < NX * NX; e++) q.P[((size_t)t * NX * NX + e) * Bs + b] = P[e];
    }
  }
  q.fail[b] = failed;
  if (q.info) q.info[b] = failed;
}

template <class M>
__global__ __launch_bounds__(64) void k_lq_dir_t(BatchViewT<typename M::real> v, LqArgs q) {
  using real = typename M::real;
  constexpr int NX = M::NX, NU = M::NU;
  using R = Rec<NX, NU>;
  const int blk = blockIdx.x / q.nd, s = blockIdx.x - blk * q.nd;
  const int b = blk * 64 + threadIdx.x;
  if (b >= v.B) return;
  const int tile = b / TW, l = b % TW;
  const int T = v.T;
  const size_t Bs = (size_t)v.Bp;
  const real* Dt = v.D + didx(tile, 0, 0, l, T + 1, R::SIZE);
  auto rec = [&](int t, int e) { return (double)Dt[((size_t)t * (R::SIZE / 2) + (e >> 1)) * (2 * TW) + (e & 1)]; };
  auto vec_of = [&](auto* base, int slots, int slot, int len) { return base + (((size_t)b * slots + slot) * q.nd + s) * len; };
  if (q.fail[b]) {  // a failed trajectory: quiet NaNs in every output
    const double qnan = __builtin_nan("");
    for (int t = 0; t <= T; t++) {
#pragma unroll
      for (int c = 0; c < NX; c++) {
        if (q.dxs) vec_of(q.dxs, T + 1, t, NX)[c] = qnan;
        if (q.dlam) vec_of(q.dlam, T + 1, t, NX)[c] = qnan;
      }
      if (q.dus && t < T) {
#pragma unroll
        for (int j = 0; j < NU; j++) vec_of(q.dus, T, t, NU)[j] = qnan;
      }
    }
    return;
  }
  // backward: v[T] = gx[T]; w = gu + fu'v; kd = Mi'w; v[t] = gx + fx'v + Kd'w
  double a[NX];
#pragma unroll
  for (int c = 0; c < NX; c++) a[c] = 0.0;
  for (int t = T; t >= 0; t--) {
    double Kd[NU * NX], Mi[NU * NU], fx[NX * NX], fu[NX * NU], an[NX], w[NU], kd[NU];
#pragma unroll
    for (int c = 0; c < NX; c++) an[c] = q.gx ? vec_of(q.gx, T + 1, t, NX)[c] : 0.0;
    if (t < T) {
#pragma unroll
      for (int j = 0; j < NU; j++) w[j] = q.gu ? vec_of(q.gu, T, t, NU)[j] : 0.0;
#pragma unroll
      for (int e = 0; e < NU * NX; e++) Kd[e] = q.Kd[((size_t)t * NU * NX + e) * Bs + b];
#pragma unroll
      for (int e = 0; e < NU * NU; e++) Mi[e] = q.Mi[((size_t)t * NU * NU + e) * Bs + b];
#pragma unroll
      for (int e = 0; e < NX * NX; e++) fx[e] = rec(t, R::FX + e);
#pragma unroll
      for (int e = 0; e < NX * NU; e++) fu[e] = rec(t, R::FU + e);
#pragma unroll
      for (int j = 0; j < NU; j++)
#pragma unroll
        for (int c = 0; c < NX; c++) w[j] = __builtin_fma(fu[c + NX * j], a[c], w[j]);
#pragma unroll
      for (int c = 0; c < NX; c++) {
#pragma unroll
        for (int r = 0; r < NX; r++) an[c] = __builtin_fma(fx[r + NX * c], a[r], an[c]);
#pragma unroll
        for (int j = 0; j < NU; j++) an[c] = __builtin_fma(Kd[j + NU * c], w[j], an[c]);
      }
#pragma unroll
      for (int j = 0; j < NU; j++) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < NU; i++) acc = __builtin_fma(Mi[i + NU * j], w[i], acc);
        kd[j] = acc;
      }
      double* o = vec_of(q.kd, T, t, NU);
#pragma unroll
      for (int j = 0; j < NU; j++) o[j] = kd[j];
    }  // (knot T has no control: v[T] = gx[T])
    if (q.dlam) {
      double* o = vec_of(q.dlam, T + 1, t, NX);
#pragma unroll
      for (int c = 0; c < NX; c++) o[c] = an[c];
    }
#pragma unroll
    for (int c = 0; c < NX; c++) a[c] = an[c];
  }
  // forward: du = kd + Kd dx; dx[t+1] = fx dx + fu du; dlam[t] = v[t] + P[t] dx[t]
  double x[NX];
#pragma unroll
  for (int c = 0; c < NX; c++) x[c] = q.dx0 ? vec_of(q.dx0, 1, 0, NX)[c] : 0.0;
  const int last = (q.dxs || q.dlam) ? T : T - 1;
  for (int t = 0; t <= last; t++) {
    const bool prop = t < last, ctrl = t < T;
    double Kd[NU * NX], fx[NX * NX], fu[NX * NU], u[NU];
    if (ctrl) {
      const double* kdv = vec_of(q.kd, T, t, NU);
#pragma unroll
      for (int j = 0; j < NU; j++) u[j] = kdv[j];
#pragma unroll
      for (int e = 0; e < NU * NX; e++) Kd[e] = q.Kd[((size_t)t * NU * NX + e) * Bs + b];
      if (prop) {
#pragma unroll
        for (int e = 0; e < NX * NX; e++) fx[e] = rec(t, R::FX + e);
#pragma unroll
        for (int e = 0; e < NX * NU; e++) fu[e] = rec(t, R::FU + e);
      }
    }
    if (q.dxs) {
      double* o = vec_of(q.dxs, T + 1, t, NX);
#pragma unroll
      for (int c = 0; c < NX; c++) o[c] = x[c];
    }
    if (q.dlam) {
      double* o = vec_of(q.dlam, T + 1, t, NX);
      double lam[NX];
#pragma unroll
      for (int r = 0; r < NX; r++) lam[r] = o[r];
#pragma unroll
      for (int r = 0; r < NX; r++)
#pragma unroll
        for (int c = 0; c < NX; c++) lam[r] = __builtin_fma(q.P[((size_t)t * NX * NX + r + NX * c) * Bs + b], x[c], lam[r]);
#pragma unroll
      for (int r = 0; r < NX; r++) o[r] = lam[r];
    }
    if (!ctrl) break;
#pragma unroll
    for (int j = 0; j < NU; j++)
#pragma unroll
      for (int c = 0; c < NX; c++) u[j] = __builtin_fma(Kd[j + NU * c], x[c], u[j]);
    if (q.dus) {
      double* o = vec_of(q.dus, T, t, NU);
#pragma unroll
      for (int j = 0; j < NU; j++) o[j] = u[j];
    }
    if (!prop) break;
    double xn[NX];
#pragma unroll
    for (int r = 0; r < NX; r++) {
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < NX; c++) acc = __builtin_fma(fx[r + NX * c], x[c], acc);
#pragma unroll
      for (int j = 0; j < NU; j++) acc = __builtin_fma(fu[r + NX * j], u[j], acc);
      xn[r] = acc;
    }
#pragma unroll
    for (int r = 0; r < NX; r++) x[r] = xn[r];
  }
}

}  // namespace ilqr
