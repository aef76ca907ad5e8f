// estimator_thread.hpp -- the Kalman filter of the stored linearisation and the covariance of the output-feedback loop on the tiled
// layout (nx = 4 models and twins, small twins; fp64 and fp32 storage), one THREAD per trajectory, the whole algebra in registers: the
// definition of include/ilqr_amd.h (ilqr_get_estimator), a pure function of (records, K, H, P0, W, V).  Stored floats are widened where
// they are loaded; the recursion is double.  The output dimension keeps the fixed size NX, as k_lq_gain_t keeps NU: H is padded with zero
// rows and S with the identity outside ny, so every loop unrolls, the indices < ny meet the pivots of the ny x ny matrix in index order
// and the padded columns of L are exact zeros.  As in estimator_wave.hpp, what is computed at a knot does not depend on which outputs
// were asked for; the filter does not read K.
#pragma once
#include "common.hpp"
#include "estimator_wave.hpp"

namespace ilqr {

template <class M>
__global__ __launch_bounds__(64) void k_estimator_t(BatchViewT<typename M::real> v, EstArgs q) {
  using real = typename M::real;
  constexpr int NX = M::NX, NU = M::NU;
  using R = Rec<NX, NU>;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= v.B) return;
  const int tile = b / TW, l = b % TW;
  const int T = v.T;
  const int t0 = q.t0, nk = q.nk, ny = q.ny;
  const real* Dt = v.D + didx(tile, 0, 0, l, T + 1, R::SIZE);
  auto rec = [&](int t, int e) { return (double)Dt[((size_t)t * (R::SIZE / 2) + (e >> 1)) * (2 * TW) + (e & 1)]; };
  const bool wantJ = q.J != nullptr;
  const bool closed = est_closed(q);
  // H (j, c) at j + NX c, rows >= ny zero; V (i, j) at i + NX j, zero outside ny; P = Pp[t]; W
  double H[NX * NX], V[NX * NX], P[NX * NX], Wm[NX * NX];
#pragma unroll
  for (int c = 0; c < NX; c++)
#pragma unroll
    for (int j = 0; j < NX; j++) {
      const bool in = j < ny;
      const double hv = q.H[(size_t)b * ny * NX + (in ? j + ny * c : 0)];
      H[j + NX * c] = in ? hv : 0.0;
      const bool vin = j < ny && c < ny;
      const double vv = q.V[(size_t)b * ny * ny + (vin ? j + ny * c : 0)];
      V[j + NX * c] = vin ? vv : 0.0;
    }
#pragma unroll
  for (int e = 0; e < NX * NX; e++) {
    P[e] = q.P0 ? q.P0[(size_t)b * NX * NX + e] : 0.0;
    Wm[e] = q.W ? q.W[(size_t)b * NX * NX + e] : 0.0;
  }
  auto slot = [&](int t) { return (size_t)b * nk + (t - t0); };
  auto store_nn = [&](double* out, int t, const double (&X)[NX * NX]) {
    if (!out || t < t0 || t >= t0 + nk) return;
#pragma unroll
    for (int e = 0; e < NX * NX; e++) out[slot(t) * NX * NX + e] = X[e];
  };
  store_nn(q.Pp, 0, P);
  double Xh[NX * NX], A[NX * NX];  // A of the previous knot
  double j2 = 0.0;                 // 2 J
  int failed = 0;
  const int last = est_last_knot(q, T);
  for (int t = 0; t <= last; t++) {
    const bool in_window = t >= t0 && t < t0 + nk;
    const bool step = t < last;                                   // Pp[t + 1] (and A) are needed
    const bool ctrl = closed && t < T && (wantJ || (q.Su && in_window));  // Z and Su are needed
    // Every load of the knot before its first store (the compiler cannot move a load across a store to the caller's arrays): the
    // knot waits for memory once.
    double K[NU * NX], fx[NX * NX], fu[NX * NU], cxx[NX * NX], cxu[NX * NU], cuu[NU * NU];
    if (step) {
#pragma unroll
      for (int e = 0; e < NX * NX; e++) fx[e] = rec(t, R::FX + e);
    }
    if (closed && t < T) {
#pragma unroll
      for (int e = 0; e < NU * NX; e++) K[e] = (double)v.Kfb[tidx(tile, t, e, l, T, NU * NX)];
#pragma unroll
      for (int e = 0; e < NX * NU; e++) fu[e] = rec(t, R::FU + e);
    }
    if (wantJ) {
#pragma unroll
      for (int e = 0; e < NX * NX; e++) cxx[e] = rec(t, R::CXX + e);
      if (t < T) {
#pragma unroll
        for (int e = 0; e < NX * NU; e++) cxu[e] = rec(t, R::CXU + e);
#pragma unroll
        for (int e = 0; e < NU * NU; e++) cuu[e] = rec(t, R::CUU + e);
      }
    }
    // PH = Pp H' (a, j) ; S = sym(H Pp H' + V), the identity outside ny
    double PH[NX * NX], S0[NX * NX], Sm[NX * NX];
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int j = 0; j < NX; j++) {
        double acc = 0;
#pragma unroll
        for (int r = 0; r < NX; r++) acc += P[a + NX * r] * H[j + NX * r];
        PH[a + NX * j] = acc;
      }
#pragma unroll
    for (int i = 0; i < NX; i++)
#pragma unroll
      for (int j = 0; j < NX; j++) {
        double acc = 0;
#pragma unroll
        for (int r = 0; r < NX; r++) acc += H[i + NX * r] * PH[r + NX * j];
        S0[i + NX * j] = acc + V[i + NX * j];
      }
#pragma unroll
    for (int i = 0; i < NX; i++)
#pragma unroll
      for (int j = 0; j < NX; j++) Sm[i + NX * j] = 0.5 * (S0[i + NX * j] + S0[j + NX * i]);
    // S = R R', lower, in index order; the padded indices are the identity
    double Rf[NX * NX], dinv[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) {
      double s = (j < ny) ? Sm[j + NX * j] : 1.0;
#pragma unroll
      for (int k = 0; k < j; k++) s = __builtin_fma(-Rf[j + NX * k], Rf[j + NX * k], s);
      if (!failed && (!(s > 0.0) || s > 1.7976931348623157e308)) failed = t + 1;
      const double rinv = 1.0 / __builtin_sqrt(s);
      dinv[j] = rinv;
      Rf[j + NX * j] = s * rinv;
#pragma unroll
      for (int i = j + 1; i < NX; i++) {
        double e = (i < ny && j < ny) ? Sm[i + NX * j] : 0.0;
#pragma unroll
        for (int k = 0; k < j; k++) e = __builtin_fma(-Rf[i + NX * k], Rf[j + NX * k], e);
        Rf[i + NX * j] = e * rinv;
      }
    }
    if (failed) break;
    // L = Pp H' S^-1: row a of L solves R R' x = (row a of PH)', forward then back
    double Lm[NX * NX];
#pragma unroll
    for (int a = 0; a < NX; a++) {
      double x[NX];
#pragma unroll
      for (int r = 0; r < NX; r++) {
        double s = PH[a + NX * r];
#pragma unroll
        for (int k = 0; k < r; k++) s = __builtin_fma(-Rf[r + NX * k], x[k], s);
        x[r] = s * dinv[r];
      }
#pragma unroll
      for (int r = NX - 1; r >= 0; r--) {
        double s = x[r];
#pragma unroll
        for (int k = r + 1; k < NX; k++) s = __builtin_fma(-Rf[k + NX * r], x[k], s);
        x[r] = s * dinv[r];
      }
#pragma unroll
      for (int r = 0; r < NX; r++) Lm[a + NX * r] = x[r];
    }
    if (q.L && in_window) {
#pragma unroll
      for (int j = 0; j < NX; j++)
#pragma unroll
        for (int a = 0; a < NX; a++)
          if (j < ny) q.L[slot(t) * NX * ny + a + NX * j] = Lm[a + NX * j];
    }
    // G = I - L H ; Pf = sym(G Pp G' + L V L')
    double G[NX * NX], Y[NX * NX], VL[NX * NX], Pn[NX * NX], Pf[NX * NX];
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) {
        double acc = 0;
#pragma unroll
        for (int j = 0; j < NX; j++) acc += Lm[a + NX * j] * H[j + NX * c];
        G[a + NX * c] = (a == c ? 1.0 : 0.0) - acc;
      }
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) {  // Y = Pp G'
        double acc = 0;
#pragma unroll
        for (int r = 0; r < NX; r++) acc += P[a + NX * r] * G[c + NX * r];
        Y[a + NX * c] = acc;
      }
#pragma unroll
    for (int i = 0; i < NX; i++)
#pragma unroll
      for (int c = 0; c < NX; c++) {  // VL = V L'
        double acc = 0;
#pragma unroll
        for (int j = 0; j < NX; j++) acc += V[i + NX * j] * Lm[c + NX * j];
        VL[i + NX * c] = acc;
      }
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) {
        double acc = 0;
#pragma unroll
        for (int r = 0; r < NX; r++) acc += G[a + NX * r] * Y[r + NX * c];
#pragma unroll
        for (int j = 0; j < NX; j++) acc += Lm[a + NX * j] * VL[j + NX * c];
        Pn[a + NX * c] = acc;
      }
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) Pf[a + NX * c] = 0.5 * (Pn[a + NX * c] + Pn[c + NX * a]);
    store_nn(q.Pf, t, Pf);
    if (closed) {
      // N = sym(L S L') ; Xh = N (t = 0) else sym(A Xh A' + N) ; Sigma = Xh + Pf
      double SL[NX * NX], Nn[NX * NX], Sg[NX * NX];
#pragma unroll
      for (int i = 0; i < NX; i++)
#pragma unroll
        for (int c = 0; c < NX; c++) {  // S L' (S zero outside ny: the padded columns of L are zero either way)
          double acc = 0;
#pragma unroll
          for (int j = 0; j < NX; j++) acc += ((i < ny && j < ny) ? Sm[i + NX * j] : 0.0) * Lm[c + NX * j];
          SL[i + NX * c] = acc;
        }
#pragma unroll
      for (int a = 0; a < NX; a++)
#pragma unroll
        for (int c = 0; c < NX; c++) {
          double acc = 0;
#pragma unroll
          for (int j = 0; j < NX; j++) acc += Lm[a + NX * j] * SL[j + NX * c];
          Pn[a + NX * c] = acc;
        }
#pragma unroll
      for (int a = 0; a < NX; a++)
#pragma unroll
        for (int c = 0; c < NX; c++) Nn[a + NX * c] = 0.5 * (Pn[a + NX * c] + Pn[c + NX * a]);
      if (t == 0) {
#pragma unroll
        for (int e = 0; e < NX * NX; e++) Xh[e] = Nn[e];
      } else {
        double Ya[NX * NX];  // Xh A'
#pragma unroll
        for (int a = 0; a < NX; a++)
#pragma unroll
          for (int c = 0; c < NX; c++) {
            double acc = 0;
#pragma unroll
            for (int r = 0; r < NX; r++) acc += Xh[a + NX * r] * A[c + NX * r];
            Ya[a + NX * c] = acc;
          }
#pragma unroll
        for (int a = 0; a < NX; a++)
#pragma unroll
          for (int c = 0; c < NX; c++) {
            double acc = 0;
#pragma unroll
            for (int r = 0; r < NX; r++) acc += A[a + NX * r] * Ya[r + NX * c];
            Pn[a + NX * c] = acc + Nn[a + NX * c];
          }
#pragma unroll
        for (int a = 0; a < NX; a++)
#pragma unroll
          for (int c = 0; c < NX; c++) Xh[a + NX * c] = 0.5 * (Pn[a + NX * c] + Pn[c + NX * a]);
      }
#pragma unroll
      for (int e = 0; e < NX * NX; e++) Sg[e] = Xh[e] + Pf[e];
      store_nn(q.Sigma, t, Sg);
      double xx = 0;
      if (wantJ) {
#pragma unroll
        for (int e = 0; e < NX * NX; e++) xx += cxx[e] * Sg[e];
      }
      if (ctrl) {
        double Z[NX * NU], KZ[NU * NU];  // Z = Xh K' ; K Z
#pragma unroll
        for (int a = 0; a < NX; a++)
#pragma unroll
          for (int j = 0; j < NU; j++) {
            double acc = 0;
#pragma unroll
            for (int r = 0; r < NX; r++) acc += Xh[a + NX * r] * K[j + NU * r];
            Z[a + NX * j] = acc;
          }
#pragma unroll
        for (int i = 0; i < NU; i++)
#pragma unroll
          for (int j = 0; j < NU; j++) {
            double acc = 0;
#pragma unroll
            for (int r = 0; r < NX; r++) acc += K[i + NU * r] * Z[r + NX * j];
            KZ[i + NU * j] = acc;
          }
        double uu = 0, xu = 0;
#pragma unroll
        for (int i = 0; i < NU; i++)
#pragma unroll
          for (int j = 0; j < NU; j++) {
            const double su = 0.5 * (KZ[i + NU * j] + KZ[j + NU * i]);
            if (q.Su && in_window) q.Su[slot(t) * NU * NU + i + NU * j] = su;
            if (wantJ) uu += cuu[i + NU * j] * su;
          }
        if (wantJ) {
#pragma unroll
          for (int e = 0; e < NX * NU; e++) xu += cxu[e] * Z[e];
          xx = (xx + uu) + 2.0 * xu;
        }
      }
      if (wantJ) j2 += xx;
      if (step) {  // A = fx + fu K, for the next knot's Xh
#pragma unroll
        for (int a = 0; a < NX; a++)
#pragma unroll
          for (int c = 0; c < NX; c++) {
            double acc = 0;
#pragma unroll
            for (int j = 0; j < NU; j++) acc += fu[a + NX * j] * K[j + NU * c];
            A[a + NX * c] = fx[a + NX * c] + acc;
          }
      }
    }
    if (!step) break;
    // Pp[t + 1] = sym(fx Pf fx' + W)
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) {  // Y = Pf fx'
        double acc = 0;
#pragma unroll
        for (int r = 0; r < NX; r++) acc += Pf[a + NX * r] * fx[c + NX * r];
        Y[a + NX * c] = acc;
      }
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) {
        double acc = 0;
#pragma unroll
        for (int r = 0; r < NX; r++) acc += fx[a + NX * r] * Y[r + NX * c];
        Pn[a + NX * c] = acc + Wm[a + NX * c];
      }
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) P[a + NX * c] = 0.5 * (Pn[a + NX * c] + Pn[c + NX * a]);
    store_nn(q.Pp, t + 1, P);
  }
  if (failed) {  // quiet NaNs in every output over the whole window (this thread wrote the knots before the failure: program order)
    const double qnan = __builtin_nan("");
    for (int s = 0; s < nk; s++) {
      const size_t o = (size_t)b * nk + s;
      for (int e = 0; e < NX * NX; e++) {
        if (q.Pp) q.Pp[o * NX * NX + e] = qnan;
        if (q.Pf) q.Pf[o * NX * NX + e] = qnan;
        if (q.Sigma) q.Sigma[o * NX * NX + e] = qnan;
      }
      if (q.L)
        for (int e = 0; e < NX * ny; e++) q.L[o * NX * ny + e] = qnan;
      if (q.Su)
        for (int e = 0; e < NU * NU; e++) q.Su[o * NU * NU + e] = qnan;
    }
    if (wantJ) q.J[b] = qnan;
  } else if (wantJ) {
    q.J[b] = 0.5 * j2;
  }
  if (q.info) q.info[b] = failed;
}

}  // namespace ilqr
