// value_thread.hpp -- the value model (Vx, Vxx) of the stored policy on the tiled layout (nx = 4 models and twins, small twins; fp64 and
// fp32 storage), one THREAD per trajectory, the whole algebra in registers: backward_thread.hpp's recursion (src/ilqr_core.cpp:353-363,
// 391-393) with the stored gains in the box-QP's place.  No lambda, no divergence test: a pure function of (records, k, K), the
// definition of include/ilqr_amd.h (ilqr_get_value).  Stored floats are widened where they are loaded; the recursion is double.
#pragma once
#include "common.hpp"

namespace ilqr {

// V is carried from knot T down to t0; the knots of the window [t0, t0 + nk) are written as canonical double, Vx_out [B][nk][NX],
// Vxx_out [B][nk][NX * NX] column-major (either may be null).
template <class M>
__global__ __launch_bounds__(64) void k_value_t(BatchViewT<typename M::real> v, int t0, int nk, double* __restrict__ Vx_out, double* __restrict__ Vxx_out) {
  using real = typename M::real;
  constexpr int NX = M::NX, NU = M::NU;
  using R = Rec<NX, NU>;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= v.B) return;
  const int tile = b / TW, l = b % TW;
  const int T = v.T;
  const real* Dt = v.D + didx(tile, 0, 0, l, T + 1, R::SIZE);
  auto rec = [&](int t, int e) { return (double)Dt[((size_t)t * (R::SIZE / 2) + (e >> 1)) * (2 * TW) + (e & 1)]; };
  double Vx[NX], Vxx[NX * NX];
  auto store = [&](int t) {
    if (t >= t0 + nk) return;
    const size_t s = (size_t)b * nk + (t - t0);
    if (Vx_out) {
#pragma unroll
      for (int a = 0; a < NX; a++) Vx_out[s * NX + a] = Vx[a];
    }
    if (Vxx_out) {
#pragma unroll
      for (int e = 0; e < NX * NX; e++) Vxx_out[s * NX * NX + e] = Vxx[e];
    }
  };
#pragma unroll
  for (int a = 0; a < NX; a++) Vx[a] = rec(T, R::CX + a);  // :353
#pragma unroll
  for (int e = 0; e < NX * NX; e++) Vxx[e] = rec(T, R::CXX + e);  // :354
  store(T);

  for (int i = T - 1; i >= t0; i--) {
    double fx[NX * NX], fu[NX * NU], k[NU], K[NU * NX];
#pragma unroll
    for (int e = 0; e < NX * NX; e++) fx[e] = rec(i, R::FX + e);
#pragma unroll
    for (int e = 0; e < NX * NU; e++) fu[e] = rec(i, R::FU + e);
#pragma unroll
    for (int j = 0; j < NU; j++) k[j] = (double)v.kff[tidx(tile, i, j, l, T, NU)];
#pragma unroll
    for (int e = 0; e < NU * NX; e++) K[e] = (double)v.Kfb[tidx(tile, i, e, l, T, NU * NX)];

    double Qx[NX], Qu[NU], Qxx[NX * NX], Qux[NU * NX], Quu[NU * NU];
    double A1[NX * NX], A2[NX * NU];  // Vxx fx, Vxx fu
    // :359-360
#pragma unroll
    for (int a = 0; a < NX; a++) {
      double acc = 0;
#pragma unroll
      for (int q = 0; q < NX; q++) acc += fx[q + NX * a] * Vx[q];
      Qx[a] = rec(i, R::CX + a) + acc;
    }
#pragma unroll
    for (int a = 0; a < NU; a++) {
      double acc = 0;
#pragma unroll
      for (int q = 0; q < NX; q++) acc += fu[q + NX * a] * Vx[q];
      Qu[a] = rec(i, R::CU + a) + acc;
    }
#pragma unroll
    for (int a = 0; a < NX; a++) {
#pragma unroll
      for (int c = 0; c < NX; c++) {
        double acc = 0;
#pragma unroll
        for (int q = 0; q < NX; q++) acc += Vxx[a + NX * q] * fx[q + NX * c];
        A1[a + NX * c] = acc;
      }
#pragma unroll
      for (int c = 0; c < NU; c++) {
        double acc = 0;
#pragma unroll
        for (int q = 0; q < NX; q++) acc += Vxx[a + NX * q] * fu[q + NX * c];
        A2[a + NX * c] = acc;
      }
    }
    // :361 Qxx = cxx + fx'A1 ; :362 Qux = cxu' + fu'A1 ; :363 Quu = cuu + fu'A2
#pragma unroll
    for (int c = 0; c < NX; c++) {
#pragma unroll
      for (int a = 0; a < NX; a++) {
        double acc = 0;
#pragma unroll
        for (int q = 0; q < NX; q++) acc += fx[q + NX * a] * A1[q + NX * c];
        Qxx[a + NX * c] = rec(i, R::CXX + a + NX * c) + acc;
      }
#pragma unroll
      for (int a = 0; a < NU; a++) {
        double acc = 0;
#pragma unroll
        for (int q = 0; q < NX; q++) acc += fu[q + NX * a] * A1[q + NX * c];
        Qux[a + NU * c] = rec(i, R::CXU + c + NX * a) + acc;
      }
    }
#pragma unroll
    for (int c = 0; c < NU; c++)
#pragma unroll
      for (int a = 0; a < NU; a++) {
        double acc = 0;
#pragma unroll
        for (int q = 0; q < NX; q++) acc += fu[q + NX * a] * A2[q + NX * c];
        Quu[a + NU * c] = rec(i, R::CUU + a + NU * c) + acc;
      }
    // w = Quu k + Qu ; W = Quu K + Qux
    double w[NU], Wm[NU * NX];
#pragma unroll
    for (int a = 0; a < NU; a++) {
      double acc = 0;
#pragma unroll
      for (int q = 0; q < NU; q++) acc += Quu[a + NU * q] * k[q];
      w[a] = acc + Qu[a];
#pragma unroll
      for (int c = 0; c < NX; c++) {
        double acc2 = 0;
#pragma unroll
        for (int q = 0; q < NU; q++) acc2 += Quu[a + NU * q] * K[q + NU * c];
        Wm[a + NU * c] = acc2 + Qux[a + NU * c];
      }
    }
    // :391 Vx = Qx + K'(Quu k + Qu) + Qux'k ; :392 Vn = Qxx + K'(Quu K + Qux) + Qux'K ; :393 Vxx = (Vn + Vn')/2
    double Vn[NX * NX];
#pragma unroll
    for (int a = 0; a < NX; a++) {
      double t1 = 0, t2 = 0;
#pragma unroll
      for (int q = 0; q < NU; q++) {
        t1 += K[q + NU * a] * w[q];
        t2 += Qux[q + NU * a] * k[q];
      }
      Vx[a] = (Qx[a] + t1) + t2;
#pragma unroll
      for (int c = 0; c < NX; c++) {
        double s1 = 0, s2 = 0;
#pragma unroll
        for (int q = 0; q < NU; q++) {
          s1 += K[q + NU * a] * Wm[q + NU * c];
          s2 += Qux[q + NU * a] * K[q + NU * c];
        }
        Vn[a + NX * c] = (Qxx[a + NX * c] + s1) + s2;
      }
    }
#pragma unroll
    for (int a = 0; a < NX; a++)
#pragma unroll
      for (int c = 0; c < NX; c++) Vxx[a + NX * c] = 0.5 * (Vn[a + NX * c] + Vn[c + NX * a]);
    store(i);
  }
}

}  // namespace ilqr
