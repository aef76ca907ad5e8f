// lq_solve_wave.hpp -- the equality-constrained LQ subproblem the handle's records hold, solved for the caller's linear terms, on the
// trajectory-contiguous layout of the generic path (n <= 32, m <= 32; double or float storage).  Three kernels on one stream:
//     k_lq_gain_w   one WAVEFRONT per trajectory: the Riccati sweep that factors Quu on the free controls, once per call
//     k_lq_back_w   one wavefront per (trajectory, 16 directions): v, w backward, kd = -Quu_FF^-1 w_F
//     k_lq_fwd_w    one wavefront per (trajectory, 16 directions): dx, du forward, dlam = P dx + v
//
// The definition (include/ilqr_amd.h, ilqr_solve_lq):
//     gain sweep:  P[T] = cxx[T];  Qxx = cxx + fx'P fx, Qux = cxu' + fu'P fx, Quu = cuu + fu'P fu + mu I;  Quu_FF = L L';
//                  Kd_F = -Quu_FF^-1 Qux_F, held rows zero;  P[t] = sym(Qxx + Qux'Kd)
//     backward:    v[T] = gx[T];  w = gu + fu'v[t+1];  kd_F = -Quu_FF^-1 w_F, held rows zero;  v[t] = gx + fx'v[t+1] + Kd'w
//     forward:     dx[0] = dx0;  du = Kd dx + kd;  dx[t+1] = fx dx + fu du;  dlam[t] = P[t] dx[t] + v[t]
//
// Gain sweep.  The products are k_value_w's (value_wave.hpp: natural registers, sum_ks mfma(X[ks], Y[ks]) = X'Y).  The factorisation keeps
// the fixed size M = 16 MT: a held control -- and every index >= m -- is embedded as an identity row and column with a zero right-hand
// side, so the free indices meet the same pivots in the same order as a compacted Quu_FF would, and the held rows of every solution are
// exact zeros.  Cholesky in place in LDS: lane r owns row r; step j forms column j, lane j publishes the pivot and every lane reads it (so
// the "pivot <= 0 or not finite" exit is wavefront-uniform) and scales its element.  Then ONE LANE PER RIGHT-HAND SIDE: lanes 0 .. N - 1
// solve for the N columns of Qux, lanes N .. N + M - 1 for the columns of the identity (the masked inverse), forward and back substitution
// on a column that rests in LDS and that only its own lane touches, every element of L a broadcast LDS read.  What leaves the kernel per
// knot: Kd (m x n), Mi = -Quu^-1 masked (m x m: held rows and columns zero) and, if dlam is asked for, P[t] (n x n) -- so the two
// direction sweeps are pure matrix products.
//
// Direction sweeps: SensTile's moves of the caller's tiles (sensitivity_wave.hpp), columns = directions, and so its column independence:
// column p of an MFMA result depends on column p of its B operand and accumulator alone.  The backward sweep leaves kd in the caller's
// dus (or in scratch when dus is not asked for) and v in the caller's dlam; the forward sweep reads each block before it overwrites it.
// A trajectory whose gain sweep failed (fail[b] != 0) gets quiet NaNs in every output from the forward sweep; nobody else's bits change.
//
// Resources (hipcc's kernel-resource-usage remarks, gfx950): DESIGN.md 3.18.
#pragma once
#include "sensitivity_wave.hpp"
#include "value_wave.hpp"

namespace ilqr {

// Canonical double in device memory (include/ilqr_amd.h).  The scratch pointers are the handle's (capi.hip, run_lq_solve carves them).
struct LqArgs {
  int nd, hold;
  double mu;
  const double* dx0;  // [B][nd][nx]        null = zero
  const double* gx;   // [B][T+1][nd][nx]   null = zero
  const double* gu;   // [B][T][nd][nu]     null = zero
  double* dxs;        // [B][T+1][nd][nx]   any output may be null
  double* dus;        // [B][T][nd][nu]
  double* dlam;       // [B][T+1][nd][nx]
  int* info;          // [B]                may be null
  // scratch: generic layout [B][T][..] per trajectory; tiled layout [T][..][B] (consecutive lanes, consecutive trajectories)
  double* Kd;  // m x n per knot, column-major as the stored K
  double* Mi;  // m x m per knot: -Quu^-1 on the free controls, zero rows and columns on the held ones
  double* P;   // n x n per knot, T + 1 of them; null unless dlam is asked for
  double* kd;  // [B][T][nd][nu]: the caller's dus if there is one
  int* fail;   // [B]: 0 or (knot of the failed pivot) + 1
};

template <int NT, int MT>
struct LqGainLds {
  static constexpr int N = 16 * NT, M = 16 * MT, LDX = N + 1, LDA = M + 1, LDR = N + M + 1;
  double S[LDX * N];  // Qxx, then Pn for the transposed read of the symmetrisation
  double A[M * LDA];  // masked Quu, then its factor L (lower)
  double R[M * LDR];  // right-hand sides [row][Qux | I], then the negated solutions
  double dinv[M];     // 1 / L(j, j)
  int nz[M];          // row j of the stored K has a nonzero (always, without ILQR_LQ_HOLD_CLAMPED)
};

template <int NT, int MT>
constexpr int kLqGainWaves = (NT == 2 || MT == 2) ? 1 : 2;

template <int NT, int MT, class S>
__global__ __launch_bounds__(64, (kLqGainWaves<NT, MT>)) void k_lq_gain_w(BatchViewT<S> v, int n, int m, LqArgs q) {
  using Lds = LqGainLds<NT, MT>;
  __shared__ Lds L;
  constexpr int N = 16 * NT, M = 16 * MT, LDX = Lds::LDX, LDA = Lds::LDA, LDR = Lds::LDR;
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= v.B) return;
  const int T = v.T;
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0, oFU = oFX + n * n, oCX = oFU + n * m, oCXX = oCX + n, oCXU = oCXX + n * n, oCU = oCXU + n * m, oCUU = oCU + m;
  const S* __restrict__ Db = v.D + (size_t)b * (T + 1) * REC;
  const S* __restrict__ Kb = v.Kfb + (size_t)b * T * m * n;
  double* const Kdb = q.Kd + (size_t)b * T * m * n;
  double* const Mib = q.Mi + (size_t)b * T * m * m;
  double* const Pb = q.P ? q.P + (size_t)b * (T + 1) * n * n : nullptr;
  const int g = lane >> 4, p = lane & 15;
  {
    double* z = reinterpret_cast<double*>(&L);
    const int nz = (int)(sizeof(Lds) / sizeof(double));
    for (int e = lane; e < nz; e += 64) z[e] = 0.0;
  }
  lds_sync();
  auto mfma = [](double a, double b2, double4_t c) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b2, c, 0, 0, 0);
  };
  const double4_t zero4 = {0.0, 0.0, 0.0, 0.0};
  auto ldm = [](const S* r, bool in, int off) __attribute__((always_inline)) {
    const double val = (double)r[in ? off : 0];
    return in ? val : 0.0;
  };
  auto row_in = [&](int ti, int rr) __attribute__((always_inline)) { return 16 * ti + 4 * rr + g < n; };
  auto col_in = [&](int tj) __attribute__((always_inline)) { return 16 * tj + p < n; };
  auto mrow_in = [&](int mt, int rr) __attribute__((always_inline)) { return 16 * mt + 4 * rr + g < m; };
  auto mcol_in = [&](int mt) __attribute__((always_inline)) { return 16 * mt + p < m; };

  // P[T] = cxx[T], held transposed (Vt(a, c) = cxx(c, a)): mfma(Vt, .) multiplies by Vt' = cxx[T]
  double Vt[NT][NT][4];
  {
    const S* rT = Db + (size_t)T * REC;
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) Vt[ti][tj][rr] = ldm(rT, row_in(ti, rr) && col_in(tj), oCXX + (16 * tj + p) + n * (16 * ti + 4 * rr + g));
    if (Pb)
      for (int e = lane; e < n * n; e += 64) Pb[(size_t)T * n * n + e] = (double)rT[oCXX + e];
  }
  int failed = 0;
  for (int i = T - 1; i >= 0; i--) {
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
    // A1 = P fx (n x n), A2 = P fu (n x m)
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
    // Qxx = cxx + fx'A1 ; Qux = cxu' + fu'A1 ; Quu = cuu + fu'A2 + mu I
    double Qux[MT][NT][4], Quu[MT][MT][4];  // (Qxx rests in L.S until Pn is formed)
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
          L.S[(16 * ti + 4 * rr + g) + LDX * (16 * tj + p)] =
              ldm(rk, row_in(ti, rr) && col_in(tj), oCXX + (16 * ti + 4 * rr + g) + n * (16 * tj + p)) + qxx[ti][rr];
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
        for (int rr = 0; rr < 4; rr++) {
          const int row = 16 * mi + 4 * rr + g, col = 16 * mj + p;
          const double val = ldm(rk, mrow_in(mi, rr) && mcol_in(mj), oCUU + row + m * col) + quu[mi][rr];
          Quu[mi][mj][rr] = (row == col && row < m) ? val + q.mu : val;
        }
    }
    // which controls are held: row j of the stored K is exactly zero (every row counts as nonzero without the flag)
    if (lane < M) L.nz[lane] = q.hold ? 0 : 1;
    lds_sync();
    if (q.hold) {
      const S* Ki = Kb + (size_t)i * m * n;
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          bool any = false;
#pragma unroll
          for (int tj = 0; tj < NT; tj++) {
            const double kv = ldm(Ki, mrow_in(mt, rr) && col_in(tj), (16 * mt + 4 * rr + g) + m * (16 * tj + p));
            any = any || !(kv == 0.0);
          }
          if (any) L.nz[16 * mt + 4 * rr + g] = 1;
        }
    }
    // The fixed-size system: held controls and the indices >= m as identity rows and columns with zero right-hand sides
    lds_sync();  // (nz written)
#pragma unroll
    for (int mi = 0; mi < MT; mi++)
#pragma unroll
      for (int rr = 0; rr < 4; rr++) {
        const int row = 16 * mi + 4 * rr + g;
        const bool hrow = row >= m || L.nz[row] == 0;
#pragma unroll
        for (int mj = 0; mj < MT; mj++) {
          const int col = 16 * mj + p;
          const bool hcol = col >= m || L.nz[col] == 0;
          L.A[row * LDA + col] = (hrow || hcol) ? (row == col ? 1.0 : 0.0) : Quu[mi][mj][rr];
          L.R[row * LDR + N + col] = (row == col && !hrow) ? 1.0 : 0.0;
        }
#pragma unroll
        for (int tj = 0; tj < NT; tj++) L.R[row * LDR + 16 * tj + p] = hrow ? 0.0 : Qux[mi][tj][rr];
      }
    lds_sync();
    // Cholesky, lower, in index order, in place in L.A: lane r owns row r; step j forms column j from the finished columns k < j (row j's
    // a broadcast read), lane j publishes the pivot, every lane reads it -- so the exit is wavefront-uniform -- and scales its element.
    // Rows >= m are the identity already.  The loops run to m, not M, and index LDS: a handful of registers whatever M is; unrolled by
    // eight so that the LDS reads of eight terms travel together (the sum itself stays one chain, in index order).
    for (int j = 0; j < m; j++) {
      double s = 0.0;
      if (lane >= j && lane < M) {
        s = L.A[lane * LDA + j];
#pragma unroll 8
        for (int k = 0; k < j; k++) s = __builtin_fma(-L.A[lane * LDA + k], L.A[j * LDA + k], s);
        if (lane == j) L.A[j * LDA + j] = s;
      }
      lds_sync();
      const double piv = L.A[j * LDA + j];
      if (!(piv > 0.0) || piv > 1.7976931348623157e308) {  // <= 0 or not finite: the same value on every lane
        failed = i + 1;
        break;
      }
      const double rinv = 1.0 / __builtin_sqrt(piv);
      if (lane >= j && lane < M) L.A[lane * LDA + j] = s * rinv;
      if (lane == 0) L.dinv[j] = rinv;
      lds_sync();
    }
    if (failed) break;
    // L L' x = rhs, one lane per right-hand side, the column in place in L.R (only its own lane touches it); the solutions negated
    if (lane < N + M) {
      for (int r = 0; r < m; r++) {
        double s = L.R[r * LDR + lane];
#pragma unroll 8
        for (int k = 0; k < r; k++) s = __builtin_fma(-L.A[r * LDA + k], L.R[k * LDR + lane], s);
        L.R[r * LDR + lane] = s * L.dinv[r];
      }
      for (int r = m - 1; r >= 0; r--) {
        double s = L.R[r * LDR + lane];
#pragma unroll 8
        for (int k = r + 1; k < m; k++) s = __builtin_fma(-L.A[k * LDA + r], L.R[k * LDR + lane], s);
        L.R[r * LDR + lane] = s * L.dinv[r];
      }
      for (int r = 0; r < m; r++) L.R[r * LDR + lane] = 0.0 - L.R[r * LDR + lane];  // (an exact zero stays +0)
    }
    lds_sync();
    // Kd = -Quu^-1 Qux natural, and out: Kd (m x n) and Mi (m x m), consecutive lanes to consecutive addresses
    double Kd[MT][NT][4];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) Kd[mt][tj][rr] = L.R[(16 * mt + 4 * rr + g) * LDR + 16 * tj + p];
    {
      double* Ko = Kdb + (size_t)i * m * n;
      for (int e = lane; e < m * n; e += 64) {
        const int c = e / m, j = e - c * m;
        Ko[e] = L.R[j * LDR + c];
      }
      double* Mo = Mib + (size_t)i * m * m;
      for (int e = lane; e < m * m; e += 64) {
        const int c = e / m, j = e - c * m;
        Mo[e] = L.R[j * LDR + N + c];
      }
    }
    // Pn = Qxx + Qux'Kd ; P = (Pn + Pn')/2, the transpose read back from LDS
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double4_t acc = zero4;
#pragma unroll
        for (int kt = 0; kt < MT; kt++)
#pragma unroll
          for (int ks = 0; ks < 4; ks++) acc = mfma(Qux[kt][ti][ks], Kd[kt][tj][ks], acc);
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          double* const at = &L.S[(16 * ti + 4 * rr + g) + LDX * (16 * tj + p)];  // Qxx(a, c), written by this lane; Pn(a, c) in its place
          const double vn = *at + acc[rr];
          Vt[ti][tj][rr] = vn;
          *at = vn;
        }
      }
    lds_sync();
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int a = 16 * ti + 4 * rr + g, c = 16 * tj + p;
          const double val = 0.5 * (Vt[ti][tj][rr] + L.S[c + LDX * a]);
          Vt[ti][tj][rr] = val;
          if (Pb && a < n && c < n) Pb[(size_t)i * n * n + c + (size_t)n * a] = val;  // symmetric to the bit: (a, c) written at (c, a)
        }
    lds_sync();
  }
  if (lane == 0) {
    q.fail[b] = failed;
    if (q.info) q.info[b] = failed;
  }
}

template <int NT, int MT>
constexpr int kLqDirWaves = (NT == 2 && MT == 2) ? 1 : (NT == 2 || MT == 2) ? 2 : 3;

// v[T] = gx[T]; w = gu + fu'v; kd = Mi'w; v[t] = gx + fx'v + Kd'w.  kd -> q.kd, v[t] -> q.dlam (if asked for).
template <int NT, int MT, class S>
__global__ __launch_bounds__(64, (kLqDirWaves<NT, MT>)) void k_lq_back_w(BatchViewT<S> v, int n, int m, LqArgs q) {
  using Lds = SensLds<NT, MT>;
  using Tile = SensTile<NT, MT>;
  __shared__ Lds L;
  const int lane = threadIdx.x;
  const int tiles = (q.nd + 15) >> 4;
  const int b = blockIdx.x / tiles, s0 = 16 * (blockIdx.x - b * tiles);
  if (b >= v.B) return;
  if (q.fail[b]) return;  // (the forward sweep writes this trajectory's NaNs)
  const int nd = q.nd - s0 < 16 ? q.nd - s0 : 16;
  const int T = v.T;
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0, oFU = oFX + n * n;
  const S* __restrict__ Db = v.D + (size_t)b * (T + 1) * REC;
  const double* __restrict__ Kdb = q.Kd + (size_t)b * T * m * n;
  const double* __restrict__ Mib = q.Mi + (size_t)b * T * m * m;
  const int g = lane >> 4, p = lane & 15;
  auto block_of = [&](auto* base, int slots, int slot, int len) __attribute__((always_inline)) {
    return base + (((size_t)b * slots + slot) * q.nd + s0) * len;
  };
  {
    double* z = reinterpret_cast<double*>(&L);
    for (int e = lane; e < (int)(sizeof(Lds) / sizeof(double)); e += 64) z[e] = 0.0;
  }
  lds_sync();
  auto mfma = [](double a, double b2, double4_t c) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b2, c, 0, 0, 0);
  };
  const double4_t zero4 = {0.0, 0.0, 0.0, 0.0};
  auto ldm = [](const auto* r, bool in, int off) __attribute__((always_inline)) {
    const double val = (double)r[in ? off : 0];
    return in ? val : 0.0;
  };
  auto row_in = [&](int ti, int rr) __attribute__((always_inline)) { return 16 * ti + 4 * rr + g < n; };
  auto col_in = [&](int tj) __attribute__((always_inline)) { return 16 * tj + p < n; };
  auto mrow_in = [&](int mt, int rr) __attribute__((always_inline)) { return 16 * mt + 4 * rr + g < m; };
  auto mcol_in = [&](int mt) __attribute__((always_inline)) { return 16 * mt + p < m; };

  double4_t A[NT];
#pragma unroll
  for (int ti = 0; ti < NT; ti++) A[ti] = zero4;
  for (int t = T; t >= 0; t--) {
    double rx[4 * NT], ru[4 * MT];
    double fu[NT][MT][4], fx[NT][NT][4], K[MT][NT][4];
    if (q.gx) Tile::template fetch<NT>(block_of(q.gx, T + 1, t, n), nd * n, lane, rx);
    if (q.gu && t < T) Tile::template fetch<MT>(block_of(q.gu, T, t, m), nd * m, lane, ru);
    if (t < T) {
      const S* rk = Db + (size_t)t * REC;
      const double* Ki = Kdb + (size_t)t * m * n;
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int a = 16 * ti + 4 * rr + g;
          const bool ain = row_in(ti, rr);
#pragma unroll
          for (int mt = 0; mt < MT; mt++) fu[ti][mt][rr] = ldm(rk, ain && mcol_in(mt), oFU + a + n * (16 * mt + p));
#pragma unroll
          for (int tj = 0; tj < NT; tj++) fx[ti][tj][rr] = ldm(rk, ain && col_in(tj), oFX + a + n * (16 * tj + p));
        }
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) K[mt][tj][rr] = ldm(Ki, mrow_in(mt, rr) && col_in(tj), (16 * mt + 4 * rr + g) + m * (16 * tj + p));
    }
    double4_t An[NT], W[MT];
    if (q.gx) {
      Tile::template to_natural<NT>(L.in[0], n, nd * n, lane, rx, An);
    } else {
#pragma unroll
      for (int ti = 0; ti < NT; ti++) An[ti] = zero4;
    }
    if (t < T) {
      if (q.gu) {
        Tile::template to_natural<MT>(L.in[1], m, nd * m, lane, ru, W);
      } else {
#pragma unroll
        for (int mt = 0; mt < MT; mt++) W[mt] = zero4;
      }
      // W = gu + fu'A (m x 16)
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ks++) W[mt] = mfma(fu[ks >> 2][mt][ks & 3], A[ks >> 2][ks & 3], W[mt]);
      // An = gx + fx'A + Kd'W (n x 16)
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ks++) An[tj] = mfma(fx[ks >> 2][tj][ks & 3], A[ks >> 2][ks & 3], An[tj]);
#pragma unroll
        for (int ks = 0; ks < 4 * MT; ks++) An[tj] = mfma(K[ks >> 2][tj][ks & 3], W[ks >> 2][ks & 3], An[tj]);
      }
      // kd = Mi'W (m x 16): Mi natural as stored, loaded after the products above (its registers are theirs)
      const double* Mk = Mib + (size_t)t * m * m;
      double4_t Kf[MT];
#pragma unroll
      for (int mj = 0; mj < MT; mj++) {
        double Mn[MT][4];
#pragma unroll
        for (int mi = 0; mi < MT; mi++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Mn[mi][rr] = ldm(Mk, mrow_in(mi, rr) && mcol_in(mj), (16 * mi + 4 * rr + g) + m * (16 * mj + p));
        double4_t acc = zero4;
#pragma unroll
        for (int ks = 0; ks < 4 * MT; ks++) acc = mfma(Mn[ks >> 2][ks & 3], W[ks >> 2][ks & 3], acc);
        Kf[mj] = acc;
      }
      Tile::template store<MT>(L.out, block_of(q.kd, T, t, m), m, nd * m, lane, Kf);
    }  // (knot T has no control: v[T] = gx[T])
    if (q.dlam) Tile::template store<NT>(L.out, block_of(q.dlam, T + 1, t, n), n, nd * n, lane, An);
#pragma unroll
    for (int ti = 0; ti < NT; ti++) A[ti] = An[ti];
  }
}

// (the forward sweep of float records with two state tiles would spill 11 registers at two wavefronts per SIMD: one)
template <int NT, int MT, class S>
constexpr int kLqFwdWaves = (NT == 2 && MT == 1 && std::is_same<S, float>::value) ? 1 : kLqDirWaves<NT, MT>;

// dx[0] = dx0; du = kd + Kd dx; dx[t+1] = fx dx + fu du; dlam[t] = v[t] + P[t] dx[t].  kd is read from q.kd, v from q.dlam, block by
// block, before the same block is written.
template <int NT, int MT, class S>
__global__ __launch_bounds__(64, (kLqFwdWaves<NT, MT, S>)) void k_lq_fwd_w(BatchViewT<S> v, int n, int m, LqArgs q) {
  using Lds = SensLds<NT, MT>;
  using Tile = SensTile<NT, MT>;
  __shared__ Lds L;
  const int lane = threadIdx.x;
  const int tiles = (q.nd + 15) >> 4;
  const int b = blockIdx.x / tiles, s0 = 16 * (blockIdx.x - b * tiles);
  if (b >= v.B) return;
  const int nd = q.nd - s0 < 16 ? q.nd - s0 : 16;
  const int T = v.T;
  auto block_of = [&](auto* base, int slots, int slot, int len) __attribute__((always_inline)) {
    return base + (((size_t)b * slots + slot) * q.nd + s0) * len;
  };
  if (q.fail[b]) {  // a failed trajectory: quiet NaNs in every output
    const double qnan = __builtin_nan("");
    for (int t = 0; t <= T; t++) {
      if (q.dxs) {
        double* o = block_of(q.dxs, T + 1, t, n);
        for (int e = lane; e < nd * n; e += 64) o[e] = qnan;
      }
      if (q.dlam) {
        double* o = block_of(q.dlam, T + 1, t, n);
        for (int e = lane; e < nd * n; e += 64) o[e] = qnan;
      }
      if (q.dus && t < T) {
        double* o = block_of(q.dus, T, t, m);
        for (int e = lane; e < nd * m; e += 64) o[e] = qnan;
      }
    }
    return;
  }
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0, oFU = oFX + n * n;
  const S* __restrict__ Db = v.D + (size_t)b * (T + 1) * REC;
  const double* __restrict__ Kdb = q.Kd + (size_t)b * T * m * n;
  const double* __restrict__ Pb = q.dlam ? q.P + (size_t)b * (T + 1) * n * n : nullptr;
  const int g = lane >> 4, p = lane & 15;
  {
    double* z = reinterpret_cast<double*>(&L);
    for (int e = lane; e < (int)(sizeof(Lds) / sizeof(double)); e += 64) z[e] = 0.0;
  }
  lds_sync();
  auto mfma = [](double a, double b2, double4_t c) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b2, c, 0, 0, 0);
  };
  const double4_t zero4 = {0.0, 0.0, 0.0, 0.0};
  auto ldm = [](const auto* r, bool in, int off) __attribute__((always_inline)) {
    const double val = (double)r[in ? off : 0];
    return in ? val : 0.0;
  };
  auto row_in = [&](int ti, int rr) __attribute__((always_inline)) { return 16 * ti + 4 * rr + g < n; };
  auto col_in = [&](int tj) __attribute__((always_inline)) { return 16 * tj + p < n; };
  auto mrow_in = [&](int mt, int rr) __attribute__((always_inline)) { return 16 * mt + 4 * rr + g < m; };
  auto mcol_in = [&](int mt) __attribute__((always_inline)) { return 16 * mt + p < m; };

  double4_t X[NT];
  if (q.dx0) {
    double r0[4 * NT];
    Tile::template fetch<NT>(block_of(q.dx0, 1, 0, n), nd * n, lane, r0);
    Tile::template to_natural<NT>(L.in[0], n, nd * n, lane, r0, X);
  } else {
#pragma unroll
    for (int ti = 0; ti < NT; ti++) X[ti] = zero4;
  }
  // the last knot whose state somebody needs
  const int last = (q.dxs || q.dlam) ? T : T - 1;
  for (int t = 0; t <= last; t++) {
    const bool prop = t < last;
    const bool ctrl = t < T;
    if (q.dlam) {
      // dlam = v + P X (n x 16), before the knot's records are asked for (their registers are not shared with this): Pt = P' by transposed
      // indexing, a tile column at a time
      const double* Pk = Pb + (size_t)t * n * n;
      double rl[4 * NT];
      double4_t Lm[NT];
      Tile::template fetch<NT>(block_of((const double*)q.dlam, T + 1, t, n), nd * n, lane, rl);
      Tile::template to_natural<NT>(L.in[0], n, nd * n, lane, rl, Lm);
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double Pt[NT][4];
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Pt[ti][rr] = ldm(Pk, row_in(ti, rr) && col_in(tj), (16 * tj + p) + n * (16 * ti + 4 * rr + g));
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ks++) Lm[tj] = mfma(Pt[ks >> 2][ks & 3], X[ks >> 2][ks & 3], Lm[tj]);
      }
      Tile::template store<NT>(L.out, block_of(q.dlam, T + 1, t, n), n, nd * n, lane, Lm);
    }
    double rv[4 * MT];
    double Kt[NT][MT][4], fxt[NT][NT][4], fut[MT][NT][4];
    if (ctrl) {
      const S* rk = Db + (size_t)t * REC;
      const double* Ki = Kdb + (size_t)t * m * n;
      Tile::template fetch<MT>(block_of((const double*)q.kd, T, t, m), nd * m, lane, rv);
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Kt[ti][mt][rr] = ldm(Ki, row_in(ti, rr) && mcol_in(mt), (16 * mt + p) + m * (16 * ti + 4 * rr + g));
      if (prop) {
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
#pragma unroll
          for (int tj = 0; tj < NT; tj++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++)
              fxt[ti][tj][rr] = ldm(rk, row_in(ti, rr) && col_in(tj), oFX + (16 * tj + p) + n * (16 * ti + 4 * rr + g));
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int tj = 0; tj < NT; tj++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++)
              fut[mt][tj][rr] = ldm(rk, mrow_in(mt, rr) && col_in(tj), oFU + (16 * tj + p) + n * (16 * mt + 4 * rr + g));
      }
    }
    if (q.dxs) Tile::template store<NT>(L.out, block_of(q.dxs, T + 1, t, n), n, nd * n, lane, X);
    if (!ctrl) break;
    // U = kd + Kd X (m x 16)
    double4_t U[MT];
    Tile::template to_natural<MT>(L.in[1], m, nd * m, lane, rv, U);
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int ks = 0; ks < 4 * NT; ks++) U[mt] = mfma(Kt[ks >> 2][mt][ks & 3], X[ks >> 2][ks & 3], U[mt]);
    if (q.dus) Tile::template store<MT>(L.out, block_of(q.dus, T, t, m), m, nd * m, lane, U);
    if (!prop) break;
    // Xn = fx X + fu U (n x 16)
    double4_t Xn[NT];
#pragma unroll
    for (int tj = 0; tj < NT; tj++) {
      double4_t acc = zero4;
#pragma unroll
      for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(fxt[ks >> 2][tj][ks & 3], X[ks >> 2][ks & 3], acc);
#pragma unroll
      for (int ks = 0; ks < 4 * MT; ks++) acc = mfma(fut[ks >> 2][tj][ks & 3], U[ks >> 2][ks & 3], acc);
      Xn[tj] = acc;
    }
#pragma unroll
    for (int tj = 0; tj < NT; tj++) X[tj] = Xn[tj];
  }
}

}  // namespace ilqr
