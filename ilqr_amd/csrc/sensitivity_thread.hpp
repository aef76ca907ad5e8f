// sensitivity_thread.hpp -- the tangent and the adjoint of the stored closed loop on the tiled layout (nx = 4 models and twins, small
// twins; fp64 and fp32 storage), one THREAD per (trajectory, direction), B * n_dirs of them, the matrix-vector recursion in registers: the
// definitions of include/ilqr_amd.h (ilqr_get_tangent / ilqr_get_adjoint), pure functions of (records, K) and the caller's vectors.
// Stored floats are widened where they are loaded; the recursion is double.  Consecutive lanes are consecutive TRAJECTORIES of one
// direction (the records' 128-byte lines are read whole, as k_covariance_t reads them); a block's direction is blockIdx.x % n_dirs, so
// the directions of 64 trajectories run side by side and share their records in L2.  Every thread runs the same expressions in the same
// order: column s of the outputs depends on column s of the inputs alone, bit for bit.  As in sensitivity_wave.hpp, what is computed at
// a knot does not depend on which outputs were asked for.
#pragma once
#include "common.hpp"
#include "sensitivity_wave.hpp"

namespace ilqr {

template <class M>
__global__ __launch_bounds__(64) void k_tangent_t(BatchViewT<typename M::real> v, TangentArgs q) {
  using real = typename M::real;
  constexpr int NX = M::NX, NU = M::NU;
  using R = Rec<NX, NU>;
  const int blk = blockIdx.x / q.nd, s = blockIdx.x - blk * q.nd;
  const int b = blk * 64 + threadIdx.x;
  if (b >= v.B) return;
  const int tile = b / TW, l = b % TW;
  const int T = v.T;
  const int t0 = q.t0, nk = q.nk;
  const int nku = (t0 + nk < T ? t0 + nk : T) - t0;
  const real* Dt = v.D + didx(tile, 0, 0, l, T + 1, R::SIZE);
  auto rec = [&](int t, int e) { return (double)Dt[((size_t)t * (R::SIZE / 2) + (e >> 1)) * (2 * TW) + (e & 1)]; };
  // this direction's vector of knot slot `slot` in an array [B][slots][n_dirs][len]
  auto vec_of = [&](auto* base, int slots, int slot, int len) { return base + (((size_t)b * slots + slot) * q.nd + s) * len; };
  double x[NX];
#pragma unroll
  for (int c = 0; c < NX; c++) x[c] = q.dx0 ? vec_of(q.dx0, 1, 0, NX)[c] : 0.0;
  const int last = tangent_last_state(q, T);
  for (int t = 0; t <= last; t++) {
    const bool prop = t < last;                          // dx[t + 1] is needed
    const bool ctrl = prop || (q.dus && t < t0 + nku);  // du[t] is needed
    // every load of the knot before its first store: the knot waits for memory once
    double K[NU * NX], fx[NX * NX], fu[NX * NU], u[NU];
    if (ctrl) {
#pragma unroll
      for (int j = 0; j < NU; j++) u[j] = q.dv ? vec_of(q.dv, T, t, NU)[j] : 0.0;
#pragma unroll
      for (int e = 0; e < NU * NX; e++) K[e] = (double)v.Kfb[tidx(tile, t, e, l, T, NU * NX)];
      if (prop) {
#pragma unroll
        for (int e = 0; e < NX * NX; e++) fx[e] = rec(t, R::FX + e);
#pragma unroll
        for (int e = 0; e < NX * NU; e++) fu[e] = rec(t, R::FU + e);
      }
    }
    if (q.dxs && t >= t0) {
      double* o = vec_of(q.dxs, nk, t - t0, NX);
#pragma unroll
      for (int c = 0; c < NX; c++) o[c] = x[c];
    }
    if (!ctrl) break;
    // du = dv + K dx
#pragma unroll
    for (int j = 0; j < NU; j++)
#pragma unroll
      for (int c = 0; c < NX; c++) u[j] = __builtin_fma(K[j + NU * c], x[c], u[j]);
    if (q.dus && t >= t0 && t < t0 + nku) {
      double* o = vec_of(q.dus, nku, t - t0, NU);
#pragma unroll
      for (int j = 0; j < NU; j++) o[j] = u[j];
    }
    if (!prop) break;
    // dx[t + 1] = fx dx + fu du
    double xn[NX];
#pragma unroll
    for (int a = 0; a < NX; a++) {
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < NX; c++) acc = __builtin_fma(fx[a + NX * c], x[c], acc);
#pragma unroll
      for (int j = 0; j < NU; j++) acc = __builtin_fma(fu[a + NX * j], u[j], acc);
      xn[a] = acc;
    }
#pragma unroll
    for (int a = 0; a < NX; a++) x[a] = xn[a];
  }
}

template <class M>
__global__ __launch_bounds__(64) void k_adjoint_t(BatchViewT<typename M::real> v, AdjointArgs q) {
  using real = typename M::real;
  constexpr int NX = M::NX, NU = M::NU;
  using R = Rec<NX, NU>;
  const int blk = blockIdx.x / q.nd, s = blockIdx.x - blk * q.nd;
  const int b = blk * 64 + threadIdx.x;
  if (b >= v.B) return;
  const int tile = b / TW, l = b % TW;
  const int T = v.T;
  const int t0 = q.t0, nk = q.nk;
  const int nku = (t0 + nk < T ? t0 + nk : T) - t0;
  const real* Dt = v.D + didx(tile, 0, 0, l, T + 1, R::SIZE);
  auto rec = [&](int t, int e) { return (double)Dt[((size_t)t * (R::SIZE / 2) + (e >> 1)) * (2 * TW) + (e & 1)]; };
  auto vec_of = [&](auto* base, int slots, int slot, int len) { return base + (((size_t)b * slots + slot) * q.nd + s) * len; };
  const int top = t0 + nk - 1;  // the last knot with a cotangent: a[t] = 0 past it
  // g_v of the knots after the window: exact zeros, whatever the caller's buffer held
  if (q.gv)
    for (int t = top + 1; t < T; t++) {
      double* o = vec_of(q.gv, T, t, NU);
#pragma unroll
      for (int j = 0; j < NU; j++) o[j] = 0.0;
    }
  double a[NX];
#pragma unroll
  for (int c = 0; c < NX; c++) a[c] = 0.0;
  for (int t = top; t >= 0; t--) {
    const bool has_gx = q.gx && t >= t0, has_gu = q.gu && t >= t0 && t < t0 + nku;
    // every load of the knot before its first store
    double K[NU * NX], fx[NX * NX], fu[NX * NU], an[NX], w[NU];
#pragma unroll
    for (int c = 0; c < NX; c++) an[c] = has_gx ? vec_of(q.gx, nk, t - t0, NX)[c] : 0.0;
    if (t < T) {
#pragma unroll
      for (int j = 0; j < NU; j++) w[j] = has_gu ? vec_of(q.gu, nku, t - t0, NU)[j] : 0.0;
#pragma unroll
      for (int e = 0; e < NU * NX; e++) K[e] = (double)v.Kfb[tidx(tile, t, e, l, T, NU * NX)];
#pragma unroll
      for (int e = 0; e < NX * NX; e++) fx[e] = rec(t, R::FX + e);
#pragma unroll
      for (int e = 0; e < NX * NU; e++) fu[e] = rec(t, R::FU + e);
      // w = gu + fu'a
#pragma unroll
      for (int j = 0; j < NU; j++)
#pragma unroll
        for (int c = 0; c < NX; c++) w[j] = __builtin_fma(fu[c + NX * j], a[c], w[j]);
      // a[t] = gx + fx'a + K'w
#pragma unroll
      for (int c = 0; c < NX; c++) {
#pragma unroll
        for (int r = 0; r < NX; r++) an[c] = __builtin_fma(fx[r + NX * c], a[r], an[c]);
#pragma unroll
        for (int j = 0; j < NU; j++) an[c] = __builtin_fma(K[j + NU * c], w[j], an[c]);
      }
      if (q.gv) {
        double* o = vec_of(q.gv, T, t, NU);
#pragma unroll
        for (int j = 0; j < NU; j++) o[j] = w[j];
      }
    }  // (knot T has no control: a[T] = gx[T])
#pragma unroll
    for (int c = 0; c < NX; c++) a[c] = an[c];
  }
  if (q.gx0) {
    double* o = vec_of(q.gx0, 1, 0, NX);
#pragma unroll
    for (int c = 0; c < NX; c++) o[c] = a[c];
  }
}

}  // namespace ilqr
