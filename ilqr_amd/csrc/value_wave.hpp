// value_wave.hpp -- the value model (Vx, Vxx) of the stored policy on the trajectory-contiguous layout of the generic path (n <= 32,
// m <= 32; double or float storage), one WAVEFRONT per trajectory, every n x n / n x m / m x m product on v_mfma_f64_16x16x4_f64.
//
// The definition (include/ilqr_amd.h, ilqr_get_value): the backward pass's recursion (src/ilqr_core.cpp:353-363, 391-393) with the stored
// gains k, K where the box-QP stands -- no lambda, no divergence test, a pure function of (records, k, K).
//
// Operands as in backward_wave3.hpp: a matrix X lives in "natural" registers X[ti][tj][r] = X(16 ti + 4 r + g, 16 tj + p), g = lane >> 4,
// p = lane & 15 -- what an MFMA leaves in its accumulator -- and a natural register is at once the B operand of X (k-slab 4 r .. 4 r + 3
// of its rows) and the A operand of X'.  So  sum_ks mfma(X[ks], Y[ks]) = X'Y  for any two natural matrices with equal row counts, the
// result natural again: the whole step chains through registers,
//     A1 = Vxx fx, A2 = Vxx fu                      (Vxx is symmetric: its natural registers are its own A operand)
//     Qxx = cxx + fx'A1, Qux = cxu' + fu'A1, Quu = cuu + fu'A2
//     W = Quu'K + Qux                               (Quu's natural registers as the A operand)
//     Vn = Qxx + K'W + Qux'K,  Vxx = (Vn + Vn')/2   (the one trip through LDS: the transposed read)
// K'Quu'K is the transpose of the definition's K'Quu K: the two agree after the symmetrisation, exactly when cuu is symmetric.  Knot T's
// Vxx = cxx[T] is NOT symmetrised by the definition: it is loaded transposed, so that the first step multiplies by cxx[T] itself.
// Matrix-vector products (Qx, Qu, Vx) are per-lane sums over the natural registers and one reduction over the four row groups in LDS.
// Sizes that are no multiple of 16 take bounds-predicated loads (a zero outside the model adds exact zeros to every sum).
//
// Resources (hipcc's kernel-resource-usage remarks, gfx950; LDS: ValueLds): DESIGN.md 3.12.
#pragma once
#include "backward_wave.hpp"

namespace ilqr {

template <int NT>
struct ValueLds {
  static constexpr int N = 16 * NT, LD = N + 1;
  double S[LD * N];           // Vn, for the transposed read of the symmetrisation
  double red[4 * (N + WMW)];  // partial sums of the matrix-vector products, [row group][column]
  double Vx[N], Qx[N], Qu[WMW], k[WMW];
};

// Wavefronts per SIMD: chosen by the register count the compiler reports, not by a measurement.
template <int NT, int MT>
constexpr int kValueWaves = (NT == 2 && MT == 2) ? 1 : 2;

// n <= 16 NT, m <= 16 MT; whole records in v.D (an exact-derivative LQ handle: materialise_records first).  V is carried in registers from
// knot T down to t0; the knots of the window [t0, t0 + nk) are written as canonical double, Vx_out [B][nk][n], Vxx_out [B][nk][n * n]
// column-major (either may be null).
template <int NT, int MT, class S>
__global__ __launch_bounds__(64, (kValueWaves<NT, MT>)) void k_value_w(BatchViewT<S> v, int n, int m, int t0, int nk, double* __restrict__ Vx_out,
                                                                      double* __restrict__ Vxx_out) {
  using Lds = ValueLds<NT>;
  __shared__ Lds L;
  constexpr int N = 16 * NT, W = 16 * MT, LDX = Lds::LD, RS = N + W;
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= v.B) return;
  const int T = v.T;
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0, oFU = oFX + n * n, oCX = oFU + n * m, oCXX = oCX + n, oCXU = oCXX + n * n, oCU = oCXU + n * m, oCUU = oCU + m;
  const S* __restrict__ Db = v.D + (size_t)b * (T + 1) * REC;
  const S* __restrict__ kb = v.kff + (size_t)b * T * m;
  const S* __restrict__ Kb = v.Kfb + (size_t)b * T * m * n;
  double* const vxo = Vx_out ? Vx_out + (size_t)b * nk * n : nullptr;
  double* const vxxo = Vxx_out ? Vxx_out + (size_t)b * nk * n * n : nullptr;
  const int g = lane >> 4, p = lane & 15;
  {
    double* z = reinterpret_cast<double*>(&L);
    const int nz = (int)(sizeof(Lds) / sizeof(double));
    for (int e = lane; e < nz; e += 64) z[e] = 0.0;
  }
  lds_sync();
  double* const red = L.red;
  auto mfma = [](double a, double b2, double4_t c) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b2, c, 0, 0, 0);
  };
  const double4_t zero4 = {0.0, 0.0, 0.0, 0.0};
  // element `off` of a record / gain block if `in`, else an exact zero (the address of an element that exists is loaded either way)
  auto ldm = [](const S* r, bool in, int off) __attribute__((always_inline)) {
    const double val = (double)r[in ? off : 0];
    return in ? val : 0.0;
  };
  auto row_in = [&](int ti, int rr) __attribute__((always_inline)) { return 16 * ti + 4 * rr + g < n; };
  auto col_in = [&](int tj) __attribute__((always_inline)) { return 16 * tj + p < n; };
  auto mrow_in = [&](int mt, int rr) __attribute__((always_inline)) { return 16 * mt + 4 * rr + g < m; };
  auto mcol_in = [&](int mt) __attribute__((always_inline)) { return 16 * mt + p < m; };
  auto red4 = [&](int stride, int col) __attribute__((always_inline)) {
    return ((red[col] + red[stride + col]) + red[2 * stride + col]) + red[3 * stride + col];
  };

  // :353-354  Vx = cx[T]; Vxx = cxx[T], held transposed (Vt(a, c) = cxx(c, a)): mfma(Vt, .) multiplies by Vt' = cxx[T]
  double Vt[NT][NT][4];
  {
    const S* rT = Db + (size_t)T * REC;
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++)
          Vt[ti][tj][rr] = ldm(rT, row_in(ti, rr) && col_in(tj), oCXX + (16 * tj + p) + n * (16 * ti + 4 * rr + g));
    if (lane < n) L.Vx[lane] = (double)rT[oCX + lane];
    if (t0 + nk == T + 1) {  // knot T is the window's last
      const size_t s = (size_t)(T - t0);
      if (vxo && lane < n) vxo[s * n + lane] = (double)rT[oCX + lane];
      if (vxxo)
        for (int e = lane; e < n * n; e += 64) vxxo[s * n * n + e] = (double)rT[oCXX + e];
    }
  }
  for (int i = T - 1; i >= t0; i--) {
    const S* rk = Db + (size_t)i * REC;
    double fx[NT][NT][4], fu[NT][MT][4];
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int a = 16 * ti + 4 * rr + g;
        const bool ain = row_in(ti, rr);
#pragma unroll
        for (int tj = 0; tj < NT; tj++) fx[ti][tj][rr] = ldm(rk, ain && col_in(tj), oFX + a + n * (16 * tj + p));
#pragma unroll
        for (int mt = 0; mt < MT; mt++) fu[ti][mt][rr] = ldm(rk, ain && mcol_in(mt), oFU + a + n * (16 * mt + p));
      }
    const double kx = (lane < n) ? (double)rk[oCX + lane] : 0.0;                    // cx on lanes < n
    const double ku = (lane >= N && lane - N < m) ? (double)rk[oCU + lane - N] : 0.0;  // cu on lanes N .. N + m - 1
    if (lane < m) L.k[lane] = (double)kb[(size_t)i * m + lane];
    lds_sync();
    // :359-360 the partial sums of fx'Vx and fu'Vx over this lane's rows (16 ti + 4 r + g); reduced over g below
    double px[NT], pu[MT];
    {
      double vxr[NT][4];
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) vxr[ti][rr] = L.Vx[16 * ti + 4 * rr + g];
#pragma unroll
      for (int tj = 0; tj < NT; tj++) px[tj] = 0;
#pragma unroll
      for (int mt = 0; mt < MT; mt++) pu[mt] = 0;
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
#pragma unroll
          for (int tj = 0; tj < NT; tj++) px[tj] = __builtin_fma(fx[ti][tj][rr], vxr[ti][rr], px[tj]);
#pragma unroll
          for (int mt = 0; mt < MT; mt++) pu[mt] = __builtin_fma(fu[ti][mt][rr], vxr[ti][rr], pu[mt]);
        }
    }
#pragma unroll
    for (int tj = 0; tj < NT; tj++) red[g * RS + 16 * tj + p] = px[tj];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) red[g * RS + N + 16 * mt + p] = pu[mt];
    // A1 = Vxx fx (n x n), A2 = Vxx fu (n x m)
    double4_t a1[NT][NT], a2[NT][MT];
#pragma unroll
    for (int ti = 0; ti < NT; ti++) {
#pragma unroll
      for (int tj = 0; tj < NT; tj++) a1[ti][tj] = zero4;
#pragma unroll
      for (int mt = 0; mt < MT; mt++) a2[ti][mt] = zero4;
    }
#pragma unroll
    for (int ks = 0; ks < 4 * NT; ks++)
#pragma unroll
      for (int ti = 0; ti < NT; ti++) {
#pragma unroll
        for (int tj = 0; tj < NT; tj++) a1[ti][tj] = mfma(Vt[ks >> 2][ti][ks & 3], fx[ks >> 2][tj][ks & 3], a1[ti][tj]);
#pragma unroll
        for (int mt = 0; mt < MT; mt++) a2[ti][mt] = mfma(Vt[ks >> 2][ti][ks & 3], fu[ks >> 2][mt][ks & 3], a2[ti][mt]);
      }
    // Qx = cx + fx'Vx, Qu = cu + fu'Vx
    lds_sync();
    if (lane < N) L.Qx[lane] = kx + red4(RS, lane);
    else if (lane < N + W) L.Qu[lane - N] = ku + red4(RS, lane);
    // :361 Qxx = cxx + fx'A1 ; :362 Qux = cxu' + fu'A1 ; :363 Quu = cuu + fu'A2
    double Qxx[NT][NT][4], Qux[MT][NT][4], Quu[MT][MT][4];
#pragma unroll
    for (int tj = 0; tj < NT; tj++) {
      double4_t qxx[NT], qux[MT];
#pragma unroll
      for (int ti = 0; ti < NT; ti++) qxx[ti] = zero4;
#pragma unroll
      for (int mt = 0; mt < MT; mt++) qux[mt] = zero4;
#pragma unroll
      for (int ks = 0; ks < 4 * NT; ks++) {
#pragma unroll
        for (int ti = 0; ti < NT; ti++) qxx[ti] = mfma(fx[ks >> 2][ti][ks & 3], a1[ks >> 2][tj][ks & 3], qxx[ti]);
#pragma unroll
        for (int mt = 0; mt < MT; mt++) qux[mt] = mfma(fu[ks >> 2][mt][ks & 3], a1[ks >> 2][tj][ks & 3], qux[mt]);
      }
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
          Qxx[ti][tj][rr] = ldm(rk, row_in(ti, rr) && col_in(tj), oCXX + (16 * ti + 4 * rr + g) + n * (16 * tj + p)) + qxx[ti][rr];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)  // Qux(a, c) starts from cxu(c, a): offset c + n a
          Qux[mt][tj][rr] = ldm(rk, mrow_in(mt, rr) && col_in(tj), oCXU + (16 * tj + p) + n * (16 * mt + 4 * rr + g)) + qux[mt][rr];
      }
    }
#pragma unroll
    for (int mj = 0; mj < MT; mj++) {
      double4_t quu[MT];
#pragma unroll
      for (int mi = 0; mi < MT; mi++) quu[mi] = zero4;
#pragma unroll
      for (int ks = 0; ks < 4 * NT; ks++)
#pragma unroll
        for (int mi = 0; mi < MT; mi++) quu[mi] = mfma(fu[ks >> 2][mi][ks & 3], a2[ks >> 2][mj][ks & 3], quu[mi]);
#pragma unroll
      for (int mi = 0; mi < MT; mi++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++)
          Quu[mi][mj][rr] = ldm(rk, mrow_in(mi, rr) && mcol_in(mj), oCUU + (16 * mi + 4 * rr + g) + m * (16 * mj + p)) + quu[mi][rr];
    }
    // the stored gains, natural: K[mt][tj][r] = K(16 mt + 4 r + g, 16 tj + p)
    double K[MT][NT][4];
    {
      const S* Ki = Kb + (size_t)i * m * n;
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) K[mt][tj][rr] = ldm(Ki, mrow_in(mt, rr) && col_in(tj), (16 * mt + 4 * rr + g) + m * (16 * tj + p));
    }
    // W = Quu'K + Qux (m x n)
    double Wm[MT][NT][4];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double4_t acc = zero4;
#pragma unroll
        for (int kt = 0; kt < MT; kt++)
#pragma unroll
          for (int ks = 0; ks < 4; ks++) acc = mfma(Quu[kt][mt][ks], K[kt][tj][ks], acc);
#pragma unroll
        for (int rr = 0; rr < 4; rr++) Wm[mt][tj][rr] = acc[rr] + Qux[mt][tj][rr];
      }
    // :391 Vx = Qx + (K'Quu k + Qux'k) + K'Qu = Qx + W'k + K'Qu: per-lane partial sums over the rows 16 mt + 4 r + g
    lds_sync();  // (Qx, Qu written; the first reduction's sums read)
    {
      double kq[MT][4], qq[MT][4];
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          kq[mt][rr] = L.k[16 * mt + 4 * rr + g];
          qq[mt][rr] = L.Qu[16 * mt + 4 * rr + g];
        }
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double s1 = 0, s2 = 0;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            s1 = __builtin_fma(Wm[mt][tj][rr], kq[mt][rr], s1);
            s2 = __builtin_fma(K[mt][tj][rr], qq[mt][rr], s2);
          }
        red[g * N + 16 * tj + p] = s1 + s2;
      }
    }
    // :392 Vn = Qxx + K'W + Qux'K ; :393 Vxx = (Vn + Vn')/2, the transpose read back from LDS
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double4_t acc = zero4;
#pragma unroll
        for (int kt = 0; kt < MT; kt++)
#pragma unroll
          for (int ks = 0; ks < 4; ks++) {
            acc = mfma(K[kt][ti][ks], Wm[kt][tj][ks], acc);
            acc = mfma(Qux[kt][ti][ks], K[kt][tj][ks], acc);
          }
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const double vn = Qxx[ti][tj][rr] + acc[rr];
          Vt[ti][tj][rr] = vn;
          L.S[(16 * ti + 4 * rr + g) + LDX * (16 * tj + p)] = vn;
        }
      }
    lds_sync();
    const bool out = i < t0 + nk;
    const size_t s = (size_t)(i - t0);
    if (lane < N) {
      const double vx = L.Qx[lane] + red4(N, lane);
      L.Vx[lane] = vx;  // (columns outside the model: sums of exact zeros)
      if (out && vxo && lane < n) vxo[s * n + lane] = vx;
    }
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int a = 16 * ti + 4 * rr + g, c = 16 * tj + p;
          const double val = 0.5 * (Vt[ti][tj][rr] + L.S[c + LDX * a]);  // Vn(a, c) + Vn(c, a): the same bits at (c, a)
          Vt[ti][tj][rr] = val;
          // written as element (c, a): consecutive lanes, consecutive addresses
          if (out && vxxo && a < n && c < n) vxxo[s * n * n + c + (size_t)n * a] = val;
        }
    lds_sync();
  }
}

}  // namespace ilqr
