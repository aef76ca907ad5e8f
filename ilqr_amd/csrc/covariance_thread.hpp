// covariance_thread.hpp -- the closed-loop state covariance of the stored policy on the tiled layout (nx = 4 models and twins, small
// twins; fp64 and fp32 storage), one THREAD per trajectory, the whole algebra in registers: the definition of include/ilqr_amd.h
// (ilqr_get_covariance), a pure function of (records, K, Sigma0, W).  Stored floats are widened where they are loaded; the recursion is
// double.  As in covariance_wave.hpp, what is computed at a knot does not depend on which outputs were asked for.
#pragma once
#include "common.hpp"
#include "covariance_wave.hpp"

namespace ilqr {

template <class M>
__global__ __launch_bounds__(64) void k_covariance_t(BatchViewT<typename M::real> v, CovArgs q) {
  using real = typename M::real;
  constexpr int NX = M::NX, NU = M::NU;
  using R = Rec<NX, NU>;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= v.B) return;
  const int tile = b / TW, l = b % TW;
  const int T = v.T;
  const int t0 = q.t0, nk = q.nk;
  const real* Dt = v.D + didx(tile, 0, 0, l, T + 1, R::SIZE);
  auto rec = [&](int t, int e) { return (double)Dt[((size_t)t * (R::SIZE / 2) + (e >> 1)) * (2 * TW) + (e & 1)]; };
  const bool wantJ = q.J != nullptr;
  double Sg[NX * NX], Wm[NX * NX];
#pragma unroll
  for (int e = 0; e < NX * NX; e++) {
    Sg[e] = q.Sigma0 ? q.Sigma0[(size_t)b * NX * NX + e] : 0.0;
    Wm[e] = q.W ? q.W[(size_t)b * NX * NX + e] : 0.0;
  }
  auto store_sigma = [&](int t) {
    if (!q.Sigma || t < t0 || t >= t0 + nk) return;
    const size_t s = (size_t)b * nk + (t - t0);
#pragma unroll
    for (int e = 0; e < NX * NX; e++) q.Sigma[s * NX * NX + e] = Sg[e];
  };
  // <cxx[t], Sigma[t]>
  auto cxx_term = [&](const double (&cxx)[NX * NX]) {
    double acc = 0;
#pragma unroll
    for (int e = 0; e < NX * NX; e++) acc += cxx[e] * Sg[e];
    return acc;
  };
  store_sigma(0);
  double j2 = 0.0;  // 2 J

  const int last = cov_last_step(q, T);
  for (int t = 0; t <= last; t++) {
    const bool in_window = t >= t0 && t < t0 + nk;
    const bool prop = wantJ || t < t0 + nk - 1;       // Sigma[t + 1] is needed
    const bool ctrl = wantJ || (q.Su && in_window);  // Z and Su are needed
    // Every load of the knot before its first store (the compiler cannot move a load across a store to the caller's arrays): the
    // knot waits for memory once.
    double K[NU * NX], fx[NX * NX], fu[NX * NU], cxx[NX * NX], cxu[NX * NU], cuu[NU * NU];
#pragma unroll
    for (int e = 0; e < NU * NX; e++) K[e] = (double)v.Kfb[tidx(tile, t, e, l, T, NU * NX)];
    if (prop) {
#pragma unroll
      for (int e = 0; e < NX * NX; e++) fx[e] = rec(t, R::FX + e);
#pragma unroll
      for (int e = 0; e < NX * NU; e++) fu[e] = rec(t, R::FU + e);
    }
    if (wantJ) {
#pragma unroll
      for (int e = 0; e < NX * NX; e++) cxx[e] = rec(t, R::CXX + e);
#pragma unroll
      for (int e = 0; e < NX * NU; e++) cxu[e] = rec(t, R::CXU + e);
#pragma unroll
      for (int e = 0; e < NU * NU; e++) cuu[e] = rec(t, R::CUU + e);
    }
    if (ctrl) {
      double Z[NX * NU], KZ[NU * NU];  // Z = Sigma K' ; K Z
#pragma unroll
      for (int a = 0; a < NX; a++)
#pragma unroll
        for (int j = 0; j < NU; j++) {
          double acc = 0;
#pragma unroll
          for (int r = 0; r < NX; r++) acc += Sg[a + NX * r] * K[j + NU * r];
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
          if (q.Su && in_window) q.Su[((size_t)b * nk + (t - t0)) * NU * NU + i + NU * j] = su;
          if (wantJ) uu += cuu[i + NU * j] * su;
        }
      if (wantJ) {
#pragma unroll
        for (int e = 0; e < NX * NU; e++) xu += cxu[e] * Z[e];
        j2 += (cxx_term(cxx) + uu) + 2.0 * xu;
      }
    }
    if (!prop) break;
    // A = fx + fu K ; Y = Sigma A' ; Sigma[t + 1] = sym(A Y + W)
    double A[NX * NX], Y[NX * NX], Sn[NX * NX];
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) {
        double acc = 0;
#pragma unroll
        for (int j = 0; j < NU; j++) acc += fu[a + NX * j] * K[j + NU * c];
        A[a + NX * c] = fx[a + NX * c] + acc;
      }
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) {
        double acc = 0;
#pragma unroll
        for (int r = 0; r < NX; r++) acc += Sg[a + NX * r] * A[c + NX * r];
        Y[a + NX * c] = acc;
      }
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) {
        double acc = 0;
#pragma unroll
        for (int r = 0; r < NX; r++) acc += A[a + NX * r] * Y[r + NX * c];
        Sn[a + NX * c] = acc + Wm[a + NX * c];
      }
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) Sg[a + NX * c] = 0.5 * (Sn[a + NX * c] + Sn[c + NX * a]);
    store_sigma(t + 1);
  }
  if (wantJ) {
    double cxx[NX * NX];
#pragma unroll
    for (int e = 0; e < NX * NX; e++) cxx[e] = rec(T, R::CXX + e);
    q.J[b] = 0.5 * (j2 + cxx_term(cxx));
  }
}

}  // namespace ilqr
