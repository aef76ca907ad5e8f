// risk_thread.hpp -- ilqr_get_risk_sensitive on the tiled layout (nx = 4 models and twins, small twins; fp64 and fp32 storage): k_risk_t,
// one THREAD per trajectory, the definition of include/ilqr_amd.h in registers, fully unrolled; stored floats are widened where they are
// loaded, the recursion is double.  The noise dimension keeps the fixed size NX, as k_estimator_t keeps its output dimension: C is padded
// with zero columns and M with the identity outside nw, so the indices < nw meet the pivots of the nw x nw matrix in index order (a padded
// pivot is exactly 1, its logarithm exactly 0).  The control dimension keeps NU as in k_lq_gain_t: a held control is an identity row and
// column with a zero right-hand side.  Outputs go straight into the caller's canonical arrays.
#pragma once
#include "common.hpp"
#include "risk_wave.hpp"

namespace ilqr {

template <class M>
__global__ __launch_bounds__(64) void k_risk_t(BatchViewT<typename M::real> v, RiskArgs q) {
  using real = typename M::real;
  constexpr int NX = M::NX, NU = M::NU, NW = NX;
  using R = Rec<NX, NU>;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= v.B) return;
  const int tile = b / TW, l = b % TW;
  const int T = v.T, nw = q.nw;
  const double theta = q.theta;
  const real* Dt = v.D + didx(tile, 0, 0, l, T + 1, R::SIZE);
  auto rec = [&](int t, int e) { return (double)Dt[((size_t)t * (R::SIZE / 2) + (e >> 1)) * (2 * TW) + (e & 1)]; };
  double* const Ko = q.K ? q.K + (size_t)b * T * NU * NX : nullptr;
  double* const ko = q.k ? q.k + (size_t)b * T * NU : nullptr;
  double* const vxo = q.Vx ? q.Vx + (size_t)b * (T + 1) * NX : nullptr;
  double* const vxxo = q.Vxx ? q.Vxx + (size_t)b * (T + 1) * NX * NX : nullptr;
  // C (a, j) at a + NX j, columns >= nw zero
  double C[NX * NW];
#pragma unroll
  for (int j = 0; j < NW; j++)
#pragma unroll
    for (int a = 0; a < NX; a++) {
      const bool in = j < nw;
      const double cv = q.C[(size_t)b * NX * nw + (in ? a + NX * j : 0)];
      C[a + NX * j] = in ? cv : 0.0;
    }
  double P[NX * NX], vv[NX];
#pragma unroll
  for (int e = 0; e < NX * NX; e++) P[e] = rec(T, R::CXX + e);
#pragma unroll
  for (int c = 0; c < NX; c++) vv[c] = rec(T, R::CX + c);
  if (vxxo) {
#pragma unroll
    for (int e = 0; e < NX * NX; e++) vxxo[(size_t)T * NX * NX + e] = P[e];
  }
  if (vxo) {
#pragma unroll
    for (int c = 0; c < NX; c++) vxo[(size_t)T * NX + c] = vv[c];
  }
  double sc = 0.0;
  int failed = 0;
  for (int t = T - 1; t >= 0; t--) {
    // every load of the knot before its first store
    double fx[NX * NX], fu[NX * NU], cxx[NX * NX], cxu[NX * NU], cuu[NU * NU], cx[NX], cu[NU];
    bool held[NU];
#pragma unroll
    for (int e = 0; e < NX * NX; e++) fx[e] = rec(t, R::FX + e);
#pragma unroll
    for (int e = 0; e < NX * NU; e++) fu[e] = rec(t, R::FU + e);
#pragma unroll
    for (int e = 0; e < NX * NX; e++) cxx[e] = rec(t, R::CXX + e);
#pragma unroll
    for (int e = 0; e < NX * NU; e++) cxu[e] = rec(t, R::CXU + e);
#pragma unroll
    for (int e = 0; e < NU * NU; e++) cuu[e] = rec(t, R::CUU + e);
#pragma unroll
    for (int c = 0; c < NX; c++) cx[c] = rec(t, R::CX + c);
#pragma unroll
    for (int j = 0; j < NU; j++) cu[j] = rec(t, R::CU + j);
#pragma unroll
    for (int j = 0; j < NU; j++) {
      bool any = !q.hold;
#pragma unroll
      for (int c = 0; c < NX; c++) any = any || !((double)v.Kfb[tidx(tile, t, j + NU * c, l, T, NU * NX)] == 0.0);
      held[j] = !any;
    }
    // ---- the noise: G = P C, M = I - theta sym(C'G) = R R', Y = R^-1 G', y = R^-1 C'v ----
    double G[NX * NW], Mm[NW * NW], Y[NW * NX], y[NW], dinv[NW];
#pragma unroll
    for (int j = 0; j < NW; j++)
#pragma unroll
      for (int a = 0; a < NX; a++) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < NX; r++) s = __builtin_fma(P[a + NX * r], C[r + NX * j], s);
        G[a + NX * j] = s;
      }
    double tr = 0.0;
    {
      double CtG[NW * NW];
#pragma unroll
      for (int j = 0; j < NW; j++)
#pragma unroll
        for (int i = 0; i < NW; i++) {
          double s = 0.0;
#pragma unroll
          for (int r = 0; r < NX; r++) s = __builtin_fma(C[r + NX * i], G[r + NX * j], s);
          CtG[i + NW * j] = s;
        }
#pragma unroll
      for (int j = 0; j < NW; j++)
#pragma unroll
        for (int i = 0; i < NW; i++) {
          const double sv = 0.5 * (CtG[i + NW * j] + CtG[j + NW * i]);
          const double id = i == j ? 1.0 : 0.0;
          Mm[i + NW * j] = (i < nw && j < nw) ? id - theta * sv : id;
          if (i == j) tr += sv;
        }
    }
#pragma unroll
    for (int j = 0; j < NW; j++) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < NX; r++) s = __builtin_fma(C[r + NX * j], vv[r], s);
      y[j] = s;
    }
    // Cholesky, lower, in index order (the factor in Mm's lower triangle, the reciprocal diagonal beside it)
    double logsum = 0.0;
#pragma unroll
    for (int j = 0; j < NW; j++) {
      double piv = Mm[j + NW * j];
#pragma unroll
      for (int k = 0; k < j; k++) piv = __builtin_fma(-Mm[j + NW * k], Mm[j + NW * k], piv);
      if (!failed && (!(piv > 0.0) || piv > 1.7976931348623157e308)) failed = -(t + 1);
      const double root = __builtin_sqrt(piv);
      const double rinv = 1.0 / root;
      logsum += log(root);
      dinv[j] = rinv;
#pragma unroll
      for (int i = j + 1; i < NW; i++) {
        double s = Mm[i + NW * j];
#pragma unroll
        for (int k = 0; k < j; k++) s = __builtin_fma(-Mm[i + NW * k], Mm[j + NW * k], s);
        Mm[i + NW * j] = s * rinv;
      }
    }
    if (failed) break;
    // forward substitution alone, column by column: R Y = G', R y = C'v
    auto forward = [&](double(&x)[NW]) {
#pragma unroll
      for (int i = 0; i < NW; i++) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < i; k++) s = __builtin_fma(-Mm[i + NW * k], x[k], s);
        x[i] = s * dinv[i];
      }
    };
#pragma unroll
    for (int c = 0; c < NX; c++) {
      double x[NW];
#pragma unroll
      for (int j = 0; j < NW; j++) x[j] = G[c + NX * j];
      forward(x);
#pragma unroll
      for (int j = 0; j < NW; j++) Y[j + NW * c] = x[j];
    }
    forward(y);
    // Pt = P + theta Y'Y, vt = v + theta Y'y, st
    double Pt[NX * NX], vt[NX];
#pragma unroll
    for (int c = 0; c < NX; c++) {
#pragma unroll
      for (int a = 0; a < NX; a++) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < NW; j++) s = __builtin_fma(Y[j + NW * a], Y[j + NW * c], s);
        Pt[a + NX * c] = P[a + NX * c] + theta * s;
      }
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < NW; j++) s = __builtin_fma(Y[j + NW * c], y[j], s);
      vt[c] = vv[c] + theta * s;
    }
    if (theta != 0.0) {
      double yy = 0.0;
#pragma unroll
      for (int j = 0; j < NW; j++) yy = __builtin_fma(y[j], y[j], yy);
      sc = sc + 0.5 * theta * yy - logsum / theta;
    } else {
      sc = sc + 0.5 * tr;
    }
    // ---- the gain step of k_lq_gain_t on (Pt, vt) ----
    double A1[NX * NX], A2[NX * NU], Qxx[NX * NX], Qux[NU * NX], Quu[NU * NU], Qx[NX], Qu[NU];
#pragma unroll
    for (int c = 0; c < NX; c++)
#pragma unroll
      for (int a = 0; a < NX; a++) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < NX; r++) s = __builtin_fma(Pt[a + NX * r], fx[r + NX * c], s);
        A1[a + NX * c] = s;
      }
#pragma unroll
    for (int j = 0; j < NU; j++)
#pragma unroll
      for (int a = 0; a < NX; a++) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < NX; r++) s = __builtin_fma(Pt[a + NX * r], fu[r + NX * j], s);
        A2[a + NX * j] = s;
      }
#pragma unroll
    for (int c = 0; c < NX; c++) {
      double sx = cx[c];
#pragma unroll
      for (int r = 0; r < NX; r++) sx = __builtin_fma(fx[r + NX * c], vt[r], sx);
      Qx[c] = sx;
#pragma unroll
      for (int a = 0; a < NX; a++) {
        double s = cxx[a + NX * c];
#pragma unroll
        for (int r = 0; r < NX; r++) s = __builtin_fma(fx[r + NX * a], A1[r + NX * c], s);
        Qxx[a + NX * c] = s;
      }
#pragma unroll
      for (int j = 0; j < NU; j++) {
        double s = cxu[c + NX * j];
#pragma unroll
        for (int r = 0; r < NX; r++) s = __builtin_fma(fu[r + NX * j], A1[r + NX * c], s);
        Qux[j + NU * c] = s;
      }
    }
#pragma unroll
    for (int j = 0; j < NU; j++) {
      double su = cu[j];
#pragma unroll
      for (int r = 0; r < NX; r++) su = __builtin_fma(fu[r + NX * j], vt[r], su);
      Qu[j] = su;
#pragma unroll
      for (int i = 0; i < NU; i++) {
        double s = cuu[i + NU * j];
#pragma unroll
        for (int r = 0; r < NX; r++) s = __builtin_fma(fu[r + NX * i], A2[r + NX * j], s);
        if (i == j) s += q.mu;
        Quu[i + NU * j] = (held[i] || held[j]) ? (i == j ? 1.0 : 0.0) : s;
      }
    }
    double linv[NU];
#pragma unroll
    for (int j = 0; j < NU; j++) {
      double piv = Quu[j + NU * j];
#pragma unroll
      for (int k = 0; k < j; k++) piv = __builtin_fma(-Quu[j + NU * k], Quu[j + NU * k], piv);
      if (!failed && (!(piv > 0.0) || piv > 1.7976931348623157e308)) failed = t + 1;
      const double rinv = 1.0 / __builtin_sqrt(piv);
      linv[j] = rinv;
#pragma unroll
      for (int i = j + 1; i < NU; i++) {
        double s = Quu[i + NU * j];
#pragma unroll
        for (int k = 0; k < j; k++) s = __builtin_fma(-Quu[i + NU * k], Quu[j + NU * k], s);
        Quu[i + NU * j] = s * rinv;
      }
    }
    if (failed) break;
    // column by column: x = -(L L')^-1 rhs for the NX columns of Qux and for Qu, held rows zero
    auto solve = [&](double(&x)[NU]) {
#pragma unroll
      for (int i = 0; i < NU; i++) {
        double s = x[i];
#pragma unroll
        for (int k = 0; k < i; k++) s = __builtin_fma(-Quu[i + NU * k], x[k], s);
        x[i] = s * linv[i];
      }
#pragma unroll
      for (int i = NU - 1; i >= 0; i--) {
        double s = x[i];
#pragma unroll
        for (int k = i + 1; k < NU; k++) s = __builtin_fma(-Quu[k + NU * i], x[k], s);
        x[i] = s * linv[i];
      }
#pragma unroll
      for (int i = 0; i < NU; i++) x[i] = 0.0 - x[i];
    };
    double Kd[NU * NX], kd[NU];
#pragma unroll
    for (int c = 0; c < NX; c++) {
      double x[NU];
#pragma unroll
      for (int j = 0; j < NU; j++) x[j] = held[j] ? 0.0 : Qux[j + NU * c];
      solve(x);
#pragma unroll
      for (int j = 0; j < NU; j++) Kd[j + NU * c] = x[j];
    }
#pragma unroll
    for (int j = 0; j < NU; j++) kd[j] = held[j] ? 0.0 : Qu[j];
    solve(kd);
    // P[t] = sym(Qxx + Qux'K), v[t] = Qx + K'Qu, s[t] = st + 1/2 Qu'k
    double Pn[NX * NX];
#pragma unroll
    for (int c = 0; c < NX; c++) {
#pragma unroll
      for (int a = 0; a < NX; a++) {
        double s = Qxx[a + NX * c];
#pragma unroll
        for (int j = 0; j < NU; j++) s = __builtin_fma(Qux[j + NU * a], Kd[j + NU * c], s);
        Pn[a + NX * c] = s;
      }
      double s = Qx[c];
#pragma unroll
      for (int j = 0; j < NU; j++) s = __builtin_fma(Kd[j + NU * c], Qu[j], s);
      vv[c] = s;
    }
#pragma unroll
    for (int c = 0; c < NX; c++)
#pragma unroll
      for (int a = 0; a < NX; a++) P[a + NX * c] = 0.5 * (Pn[a + NX * c] + Pn[c + NX * a]);
    {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < NU; j++) s = __builtin_fma(Qu[j], kd[j], s);
      sc = sc + 0.5 * s;
    }
    if (Ko) {
#pragma unroll
      for (int e = 0; e < NU * NX; e++) Ko[(size_t)t * NU * NX + e] = Kd[e];
    }
    if (ko) {
#pragma unroll
      for (int j = 0; j < NU; j++) ko[(size_t)t * NU + j] = kd[j];
    }
    if (vxxo) {
#pragma unroll
      for (int e = 0; e < NX * NX; e++) vxxo[(size_t)t * NX * NX + e] = P[e];
    }
    if (vxo) {
#pragma unroll
      for (int c = 0; c < NX; c++) vxo[(size_t)t * NX + c] = vv[c];
    }
  }
  if (failed) {  // quiet NaNs in every output over the whole horizon, the knots this thread has written included
    const double qnan = __builtin_nan("");
    if (Ko)
      for (int e = 0; e < T * NU * NX; e++) Ko[e] = qnan;
    if (ko)
      for (int e = 0; e < T * NU; e++) ko[e] = qnan;
    if (vxo)
      for (int e = 0; e < (T + 1) * NX; e++) vxo[e] = qnan;
    if (vxxo)
      for (int e = 0; e < (T + 1) * NX * NX; e++) vxxo[e] = qnan;
  }
  if (q.J) q.J[b] = failed ? __builtin_nan("") : sc;
  q.fail[b] = failed;
  if (q.info) q.info[b] = failed;
}

}  // namespace ilqr
