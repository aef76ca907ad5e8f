// covariance_wave.hpp -- the closed-loop state covariance of the stored policy on the trajectory-contiguous layout of the generic path
// (n <= 32, m <= 32; double or float storage), one WAVEFRONT per trajectory, every n x n / n x m / m x m product on
// v_mfma_f64_16x16x4_f64.  The forward twin of value_wave.hpp: Vxx goes backward over (records, k, K), Sigma forward over (records, K).
//
// The definition (include/ilqr_amd.h, ilqr_get_covariance):
//     Sigma[0] = Sigma0;   A = fx + fu K,  Z = Sigma K',  Su = sym(K Z),
//     J += 1/2 (<cxx, Sigma> + <cuu, Su> + 2 <cxu, Z>),  Sigma[t+1] = sym(A Sigma A' + W);   J += 1/2 <cxx[T], Sigma[T]>
//
// Operands as in value_wave.hpp: a matrix X lives in "natural" registers X[ti][tj][r] = X(16 ti + 4 r + g, 16 tj + p), g = lane >> 4,
// p = lane & 15, and  sum_ks mfma(X[ks], Y[ks]) = X'Y  for two natural matrices with equal row counts, natural again.  That one
// primitive suffices without an LDS transpose because the loader can index a stored matrix either way:
//     fx' (n x n), fu' (m x n), K (m x n) natural:    At = A' = fx' + K'fu' = fx' + mfma(K, fu')
//     St = Sigma' natural:                            Y  = Sigma At = mfma(St, At),   A Sigma A' = At'Y = mfma(At, Y)
//     Kt = K' (n x m) natural:                        Z  = Sigma K' = mfma(St, Kt),   K Z = Kt'Z = mfma(Kt, Z)
// Sigma is carried TRANSPOSED (St): from knot 1 on it is symmetric to the bit and the two are one; Sigma0 is taken as given, not
// symmetrised, so it is loaded transposed and the first step multiplies by Sigma0 itself (as k_value_w does for cxx[T]).
// The inner products of J are elementwise products on natural registers (cxx loaded transposed, against St), summed per lane over the
// whole horizon, and one wave reduction at the end.  The two symmetrisations are the only trips through LDS.  Sizes that are no multiple
// of 16 take bounds-predicated loads (a zero outside the model adds exact zeros to every sum).  One wavefront has nothing to do while
// it waits for a knot's operands, so every load of a knot is issued before the knot's first product (kCovLoadAllFirst).
//
// What is computed at a knot does not depend on which outputs were asked for, only whether it is computed: a window is a slice of the
// full call and a J-only call gives the full call's J, bit for bit.
//
// Resources (hipcc's kernel-resource-usage remarks, gfx950; LDS: CovLds): DESIGN.md 3.16.
#pragma once
#include "backward_wave.hpp"

namespace ilqr {

// Canonical double in device memory (include/ilqr_amd.h): Sigma0, W [B][nx * nx] (null = zero); the knots [t0, t0 + nk) of
// Sigma [B][nk][nx * nx] and Su [B][nk][nu * nu]; J [B].  Any output may be null (the caller refuses three nulls).
struct CovArgs {
  int t0, nk;
  const double* Sigma0;
  const double* W;
  double* Sigma;
  double* Su;
  double* J;
};
// the last knot whose step (Z, Su, the propagation to the next knot) anything needs
__host__ __device__ inline int cov_last_step(const CovArgs& q, int T) { return q.J ? T - 1 : q.Su ? q.t0 + q.nk - 1 : q.t0 + q.nk - 2; }

template <int NT, int MT>
struct CovLds {
  static constexpr int D = 16 * (NT > MT ? NT : MT), LD = D + 1;
  double S[LD * D];  // A Sigma A' + W, then K Z: for the transposed read of the symmetrisations
};

// Wavefronts per SIMD: chosen by the register count the compiler reports.  A knot's operands are all loaded before its
// first product (one wait for memory per knot: the kernel's time is that wait), which takes registers: only <1, 1> stays under the 256 of
// two wavefronts per SIMD; the others get one wavefront's 512 and no variant has scratch.
template <int NT, int MT>
constexpr int kCovWaves = (NT == 2 || MT == 2) ? 1 : 2;
// <2, 2> would spill even at 512 registers with every operand in flight at once (804 bytes of scratch per lane): it loads K' first and
// every other operand where it is used (several waits per knot).
template <int NT, int MT>
constexpr bool kCovLoadAllFirst = !(NT == 2 && MT == 2);

// n <= 16 NT, m <= 16 MT; whole records in v.D (materialise_records first), the stored gains in v.Kfb.
template <int NT, int MT, class S>
__global__ __launch_bounds__(64, (kCovWaves<NT, MT>)) void k_covariance_w(BatchViewT<S> v, int n, int m, CovArgs q) {
  using Lds = CovLds<NT, MT>;
  __shared__ Lds L;
  constexpr int LDX = Lds::LD;
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= v.B) return;
  const int T = v.T;
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0, oFU = oFX + n * n, oCX = oFU + n * m, oCXX = oCX + n, oCXU = oCXX + n * n, oCU = oCXU + n * m, oCUU = oCU + m;
  const S* __restrict__ Db = v.D + (size_t)b * (T + 1) * REC;
  const S* __restrict__ Kb = v.Kfb + (size_t)b * T * m * n;
  const double* __restrict__ Wb = q.W ? q.W + (size_t)b * n * n : nullptr;
  double* const sgo = q.Sigma ? q.Sigma + (size_t)b * q.nk * n * n : nullptr;
  double* const suo = q.Su ? q.Su + (size_t)b * q.nk * m * m : nullptr;
  const bool wantJ = q.J != nullptr;
  const int t0 = q.t0, nk = q.nk;
  const int g = lane >> 4, p = lane & 15;
  auto mfma = [](double a, double b2, double4_t c) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b2, c, 0, 0, 0);
  };
  const double4_t zero4 = {0.0, 0.0, 0.0, 0.0};
  // element `off` of a record / gain block if `in`, else an exact zero (the address of an element that exists is loaded either way)
  auto ldm = [](const auto* r, bool in, int off) __attribute__((always_inline)) {
    const double val = (double)r[in ? off : 0];
    return in ? val : 0.0;
  };
  auto row_in = [&](int ti, int rr) __attribute__((always_inline)) { return 16 * ti + 4 * rr + g < n; };
  auto col_in = [&](int tj) __attribute__((always_inline)) { return 16 * tj + p < n; };
  auto mrow_in = [&](int mt, int rr) __attribute__((always_inline)) { return 16 * mt + 4 * rr + g < m; };
  auto mcol_in = [&](int mt) __attribute__((always_inline)) { return 16 * mt + p < m; };

  // Sigma[0] = Sigma0 as given, held transposed (St(a, c) = Sigma0(c, a)): mfma(St, .) multiplies by St' = Sigma0
  double St[NT][NT][4];
  {
    const double* s0 = q.Sigma0 ? q.Sigma0 + (size_t)b * n * n : nullptr;
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++)
          St[ti][tj][rr] = s0 ? ldm(s0, row_in(ti, rr) && col_in(tj), (16 * tj + p) + n * (16 * ti + 4 * rr + g)) : 0.0;
    if (sgo && t0 == 0)
      for (int e = lane; e < n * n; e += 64) sgo[e] = s0 ? s0[e] : 0.0;
  }
  double jl = 0.0;  // this lane's share of 2 J
  // cxx[t] transposed, for <cxx[t], Sigma[t]> against St
  auto load_cxxT = [&](const S* rk, double (&cxxT)[NT][NT][4]) __attribute__((always_inline)) {
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++)
          cxxT[ti][tj][rr] = ldm(rk, row_in(ti, rr) && col_in(tj), oCXX + (16 * tj + p) + n * (16 * ti + 4 * rr + g));
  };
  auto cxx_term = [&](const double (&cxxT)[NT][NT][4]) __attribute__((always_inline)) {
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) jl = __builtin_fma(cxxT[ti][tj][rr], St[ti][tj][rr], jl);
  };

  const int last = cov_last_step(q, T);
  for (int t = 0; t <= last; t++) {
    const S* rk = Db + (size_t)t * REC;
    const S* Ki = Kb + (size_t)t * m * n;
    const bool in_window = t >= t0 && t < t0 + nk;
    const bool prop = wantJ || t < t0 + nk - 1;     // Sigma[t + 1] is needed
    const bool ctrl = wantJ || (suo && in_window);  // Z and Su are needed
    // Every load of the knot is issued here, before the first product (kCovLoadAllFirst): the knot waits for memory once, not once
    // per phase.  Kt = K' (n x m): Kt(c, j) = K(j, c); cuu, cxu as stored, cxx transposed;
    // K (m x n) as stored, fu' (m x n) and fx' by transposed indexing, W as stored
    double Kt[NT][MT][4], cuu[MT][MT][4], cxu[NT][MT][4], cxxT[NT][NT][4];
    double K[MT][NT][4], fut[MT][NT][4], fxt[NT][NT][4], Wn[NT][NT][4];
    if (ctrl) {
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Kt[ti][mt][rr] = ldm(Ki, row_in(ti, rr) && mcol_in(mt), (16 * mt + p) + m * (16 * ti + 4 * rr + g));
    }
    auto load_cuu = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int mi = 0; mi < MT; mi++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++)
            cuu[mi][mt][rr] = ldm(rk, mrow_in(mi, rr) && mcol_in(mt), oCUU + (16 * mi + 4 * rr + g) + m * (16 * mt + p));
    };
    auto load_cxu = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++)
            cxu[ti][mt][rr] = ldm(rk, row_in(ti, rr) && mcol_in(mt), oCXU + (16 * ti + 4 * rr + g) + n * (16 * mt + p));
    };
    if (wantJ && kCovLoadAllFirst<NT, MT>) {
      load_cuu();
      load_cxxT(rk, cxxT);
      load_cxu();
    }
    auto load_K_fut = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int j = 16 * mt + 4 * rr + g;
            K[mt][tj][rr] = ldm(Ki, mrow_in(mt, rr) && col_in(tj), j + m * (16 * tj + p));
            fut[mt][tj][rr] = ldm(rk, mrow_in(mt, rr) && col_in(tj), oFU + (16 * tj + p) + n * j);
          }
    };
    auto load_fxt = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++)
            fxt[ti][tj][rr] = ldm(rk, row_in(ti, rr) && col_in(tj), oFX + (16 * tj + p) + n * (16 * ti + 4 * rr + g));
    };
    auto load_W = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++)
            Wn[ti][tj][rr] = Wb ? ldm(Wb, row_in(ti, rr) && col_in(tj), (16 * ti + 4 * rr + g) + n * (16 * tj + p)) : 0.0;
    };
    if (prop && kCovLoadAllFirst<NT, MT>) {
      load_K_fut();
      load_fxt();
      load_W();
    }
    if (ctrl) {
      // Z = Sigma K' (n x m)
      double4_t Z[NT][MT];
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(St[ks >> 2][ti][ks & 3], Kt[ks >> 2][mt][ks & 3], acc);
          Z[ti][mt] = acc;
        }
      // K Z = Kt'Z (m x m), to LDS for the transposed read
#pragma unroll
      for (int mi = 0; mi < MT; mi++)
#pragma unroll
        for (int mj = 0; mj < MT; mj++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(Kt[ks >> 2][mi][ks & 3], Z[ks >> 2][mj][ks & 3], acc);
#pragma unroll
          for (int rr = 0; rr < 4; rr++) L.S[(16 * mi + 4 * rr + g) + LDX * (16 * mj + p)] = acc[rr];
        }
      lds_sync();
      if (wantJ && !kCovLoadAllFirst<NT, MT>) load_cuu();
#pragma unroll
      for (int mi = 0; mi < MT; mi++)
#pragma unroll
        for (int mj = 0; mj < MT; mj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int a = 16 * mi + 4 * rr + g, c = 16 * mj + p;
            const double su = 0.5 * (L.S[a + LDX * c] + L.S[c + LDX * a]);  // the same bits at (c, a)
            // written as element (c, a): consecutive lanes, consecutive addresses
            if (suo && in_window && a < m && c < m) suo[(size_t)(t - t0) * m * m + c + (size_t)m * a] = su;
            if (wantJ) jl = __builtin_fma(cuu[mi][mj][rr], su, jl);
          }
      if (wantJ) {
        if (!kCovLoadAllFirst<NT, MT>) load_cxxT(rk, cxxT);
        cxx_term(cxxT);
        if (!kCovLoadAllFirst<NT, MT>) load_cxu();
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
#pragma unroll
          for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) jl = __builtin_fma(2.0 * cxu[ti][mt][rr], Z[ti][mt][rr], jl);
      }
      lds_sync();  // (K Z has been read: S may take the next Sigma)
    }
    if (!prop) break;
    if (!kCovLoadAllFirst<NT, MT>) {
      load_K_fut();
      load_fxt();
    }
    // At = A' = fx' + K'fu' (n x n)
    double At[NT][NT][4];
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double4_t acc = zero4;
#pragma unroll
        for (int ks = 0; ks < 4 * MT; ks++) acc = mfma(K[ks >> 2][ti][ks & 3], fut[ks >> 2][tj][ks & 3], acc);
#pragma unroll
        for (int rr = 0; rr < 4; rr++) At[ti][tj][rr] = fxt[ti][tj][rr] + acc[rr];
      }
    // Y = Sigma At
    double4_t Y[NT][NT];
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double4_t acc = zero4;
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(St[ks >> 2][ti][ks & 3], At[ks >> 2][tj][ks & 3], acc);
        Y[ti][tj] = acc;
      }
    if (!kCovLoadAllFirst<NT, MT>) load_W();
    // Sn = A Sigma A' + W = At'Y + W ; Sigma[t + 1] = (Sn + Sn')/2, the transpose read back from LDS
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double4_t acc = zero4;
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(At[ks >> 2][ti][ks & 3], Y[ks >> 2][tj][ks & 3], acc);
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const double sn = Wb ? acc[rr] + Wn[ti][tj][rr] : acc[rr];
          St[ti][tj][rr] = sn;
          L.S[(16 * ti + 4 * rr + g) + LDX * (16 * tj + p)] = sn;
        }
      }
    lds_sync();
    const bool out = sgo && t + 1 >= t0 && t + 1 < t0 + nk;
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int a = 16 * ti + 4 * rr + g, c = 16 * tj + p;
          const double val = 0.5 * (St[ti][tj][rr] + L.S[c + LDX * a]);  // Sn(a, c) + Sn(c, a): the same bits at (c, a)
          St[ti][tj][rr] = val;
          // written as element (c, a): consecutive lanes, consecutive addresses
          if (out && a < n && c < n) sgo[(size_t)(t + 1 - t0) * n * n + c + (size_t)n * a] = val;
        }
    lds_sync();
  }
  if (wantJ) {
    double cxxT[NT][NT][4];
    load_cxxT(Db + (size_t)T * REC, cxxT);
    cxx_term(cxxT);
    const double j2 = wave_sum(jl);
    if (lane == 0) q.J[b] = 0.5 * j2;
  }
}

}  // namespace ilqr
