// risk_wave.hpp -- the risk-sensitive (LEQG) gains and value of the LQ model the handle's records hold, on the trajectory-contiguous layout
// of the generic path (n <= 32, m <= 32, nw <= n; double or float storage): k_risk_w, one WAVEFRONT per trajectory, one backward sweep,
// every matrix product on v_mfma_f64_16x16x4_f64.  k_lq_gain_w's Riccati sweep (lq_solve_wave.hpp) with the value model adjusted for the
// noise before every step, and with the linear terms carried along.
//
// The definition (include/ilqr_amd.h, ilqr_get_risk_sensitive):
//     P[T] = cxx[T], v[T] = cx[T], s[T] = 0
//     G = P C;  M = I - theta sym(C'G) = R R';  Y = R^-1 G', y = R^-1 C'v;  Pt = P + theta Y'Y, vt = v + theta Y'y,
//     st = s + theta/2 y'y - (1/theta) sum_j log R(j, j)      (theta == 0: st = s + 1/2 trace(C'G))
//     Qx = cx + fx'vt, Qu = cu + fu'vt, Qxx = cxx + fx'Pt fx, Qux = cxu' + fu'Pt fx, Quu = cuu + fu'Pt fu + mu I;  Quu_FF = L L'
//     K_F = -Quu_FF^-1 Qux_F, k_F = -Quu_FF^-1 Qu_F, held rows zero;  P[t] = sym(Qxx + Qux'K), v[t] = Qx + K'Qu, s[t] = st + 1/2 Qu'k
//
// Operands as in value_wave.hpp: natural registers, sum_ks mfma(X[ks], Y[ks]) = X'Y.  P is carried transposed (Vt), as k_lq_gain_w carries
// it: from knot T - 1 on it is symmetric to the bit and the two are one; cxx[T] is taken as stored, so it is loaded transposed and
// G = mfma(Vt, C) multiplies by cxx[T] itself.  Y'Y is symmetric to the bit (element (a, c) and (c, a) sum the same products in the same
// order), so Pt' = Vt + theta mfma(Y, Y), and the gain step reads it where k_lq_gain_w reads Vt.
//
// Both factorisations keep a fixed size in LDS (16 WT for M, 16 MT for Quu; they share L.A and L.R): the indices >= nw, the indices
// >= m and the held controls are identity rows and columns with zero right-hand sides, so the others meet the pivots of the compacted
// matrix in index order.  Lane r owns row r; step j forms column j, lane j publishes the pivot and every lane reads it, so either exit is
// wavefront-uniform.  Then one lane per right-hand side, the column at rest in LDS: lanes 0 .. N - 1 take the columns of G' (forward
// substitution alone) or of Qux (forward and back), lane N takes C'v or Qu -- the linear terms are one more column, not a second pass.
// Matrix-vector products (C'v, Y'y, fx'vt, fu'vt, K'Qu) are per-lane sums over the natural registers and one reduction over the four row
// groups in LDS, as in k_value_w.  The scalar s is computed by every lane from broadcast LDS reads: the same bits on each.
//
// Outputs go straight into the caller's canonical arrays.  A wavefront whose factorisation failed overwrites its own outputs with quiet
// NaNs before it leaves (after a fence: the knots it has written are among them); nobody else's bits change.
//
// Resources (hipcc's kernel-resource-usage remarks, gfx950): DESIGN.md 3.20.
#pragma once
#include "value_wave.hpp"

namespace ilqr {

// Canonical double in device memory (include/ilqr_amd.h).  Any output may be null.
struct RiskArgs {
  int nw, hold;
  double theta, mu;
  const double* C;  // [B][nx * nw] column-major
  double* K;        // [B][T][nu * nx] column-major per knot
  double* k;        // [B][T][nu]
  double* Vx;       // [B][T+1][nx]
  double* Vxx;      // [B][T+1][nx * nx]
  double* J;        // [B]: s[0]
  int* info;        // [B]
  int* fail;        // [B], the handle's: 0, (knot of the failed pivot of Quu) + 1 or -((knot of the failed pivot of M) + 1)
};

template <int NT, int MT, int WT>
struct RiskLds {
  static constexpr int N = 16 * NT, M = 16 * MT, W = 16 * WT, F = M > W ? M : W, LDX = N + 1, LDA = F + 1, LDR = N + 3, RS = N + M;
  double S[LDX * N];  // C'G, then Qxx, then Pn: the transposed reads of the symmetrisations
  double A[F * LDA];  // M, then masked Quu: each with the identity outside, then its lower factor
  double R[F * LDR];  // right-hand sides [row][G' | C'v], then [row][Qux | Qu]; the solutions in their place
  double dinv[F];     // 1 / (diagonal of the factor)
  double red[4 * RS];  // partial sums of the matrix-vector products, [row group][column]
  double v[N], Qx[N], Qu[M], tr[W];
  int nz[M];  // row j of the stored K has a nonzero (always, without ILQR_LQ_HOLD_CLAMPED)
};

// Wavefronts per SIMD by the register count the compiler reports.
template <int NT, int MT, int WT>
constexpr int kRiskWaves = (NT == 2 && MT == 2) ? 1 : 2;

// n <= 16 NT, m <= 16 MT, nw <= 16 WT <= 16 NT; whole records in v.D (materialise_records first).
template <int NT, int MT, int WT, class S>
__global__ __launch_bounds__(64, (kRiskWaves<NT, MT, WT>)) void k_risk_w(BatchViewT<S> v, int n, int m, RiskArgs q) {
  static_assert(WT <= NT, "nw <= nx");
  using Lds = RiskLds<NT, MT, WT>;
  __shared__ Lds L;
  constexpr int N = Lds::N, M = Lds::M, W = Lds::W, LDX = Lds::LDX, LDA = Lds::LDA, LDR = Lds::LDR, RS = Lds::RS;
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= v.B) return;
  const int T = v.T, nw = q.nw;
  const double theta = q.theta;
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0, oFU = oFX + n * n, oCX = oFU + n * m, oCXX = oCX + n, oCXU = oCXX + n * n, oCU = oCXU + n * m, oCUU = oCU + m;
  const S* __restrict__ Db = v.D + (size_t)b * (T + 1) * REC;
  const S* __restrict__ Kb = v.Kfb + (size_t)b * T * m * n;
  const double* __restrict__ Cb = q.C + (size_t)b * n * nw;
  double* const Ko = q.K ? q.K + (size_t)b * T * m * n : nullptr;
  double* const ko = q.k ? q.k + (size_t)b * T * m : nullptr;
  double* const vxo = q.Vx ? q.Vx + (size_t)b * (T + 1) * n : nullptr;
  double* const vxxo = q.Vxx ? q.Vxx + (size_t)b * (T + 1) * n * n : nullptr;
  int g = lane >> 4, p = lane & 15;  // (not const: phase() below)
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
  // element `off` of a stored matrix if `in`, else an exact zero (the address of an element that exists is loaded either way)
  auto ldm = [](const auto* r, bool in, int off) __attribute__((always_inline)) {
    const double val = (double)r[in ? off : 0];
    return in ? val : 0.0;
  };
  auto row_in = [&](int ti, int rr) __attribute__((always_inline)) { return 16 * ti + 4 * rr + g < n; };
  auto col_in = [&](int tj) __attribute__((always_inline)) { return 16 * tj + p < n; };
  auto mrow_in = [&](int mt, int rr) __attribute__((always_inline)) { return 16 * mt + 4 * rr + g < m; };
  auto mcol_in = [&](int mt) __attribute__((always_inline)) { return 16 * mt + p < m; };
  auto wcol_in = [&](int wt) __attribute__((always_inline)) { return 16 * wt + p < nw; };
  auto red4 = [&](int stride, int col) __attribute__((always_inline)) {
    return ((red[col] + red[stride + col]) + red[2 * stride + col]) + red[3 * stride + col];
  };
  // Between the phases of a knot the scheduler is kept from gathering a later phase's loads above an earlier one, and the lane's row and
  // column pass through an empty asm, so that the predicated offsets of every load -- invariant over the knots, sixteen registers per
  // operand -- are formed again where they are used rather than kept for the whole sweep (estimator_wave.hpp, k_est_loop_w: together the
  // two are what spills in the variants with two tiles).
  auto phase = [&]() __attribute__((always_inline)) {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" : "+v"(g), "+v"(p));
  };
  // Cholesky of the `dim` leading rows and columns of L.A, lower, in index order, in place (as k_lq_gain_w): returns false at a pivot
  // <= 0 or not finite, the same answer on every lane.  logsum: sum_j log of the factor's diagonal, if asked for.
  auto cholesky = [&](int dim, double* logsum) __attribute__((always_inline)) {
    for (int j = 0; j < dim; j++) {
      double s = 0.0;
      if (lane >= j && lane < dim) {
        s = L.A[lane * LDA + j];
#pragma unroll 8
        for (int k = 0; k < j; k++) s = __builtin_fma(-L.A[lane * LDA + k], L.A[j * LDA + k], s);
        if (lane == j) L.A[j * LDA + j] = s;
      }
      lds_sync();
      const double piv = L.A[j * LDA + j];
      if (!(piv > 0.0) || piv > 1.7976931348623157e308) return false;
      const double root = __builtin_sqrt(piv);
      const double rinv = 1.0 / root;
      if (logsum) *logsum += log(root);
      if (lane >= j && lane < dim) L.A[lane * LDA + j] = s * rinv;
      if (lane == 0) L.dinv[j] = rinv;
      lds_sync();
    }
    return true;
  };

  // P[T] = cxx[T], held transposed (Vt(a, c) = cxx(c, a)): mfma(Vt, .) multiplies by Vt' = cxx[T];  v[T] = cx[T]
  double Vt[NT][NT][4];
  {
    const S* rT = Db + (size_t)T * REC;
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) Vt[ti][tj][rr] = ldm(rT, row_in(ti, rr) && col_in(tj), oCXX + (16 * tj + p) + n * (16 * ti + 4 * rr + g));
    if (lane < n) {
      L.v[lane] = (double)rT[oCX + lane];
      if (vxo) vxo[(size_t)T * n + lane] = (double)rT[oCX + lane];
    }
    if (vxxo)
      for (int e = lane; e < n * n; e += 64) vxxo[(size_t)T * n * n + e] = (double)rT[oCXX + e];
  }
  lds_sync();
  double sc = 0.0;  // s, the same on every lane
  int failed = 0;
  for (int i = T - 1; i >= 0; i--) {
    // ---- the noise: G = P C, M = I - theta sym(C'G) = R R', Y = R^-1 G', y = R^-1 C'v ----
    double Yn[WT][NT][4];
    phase();
    {
      double Cn[NT][WT][4];
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int wt = 0; wt < WT; wt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Cn[ti][wt][rr] = ldm(Cb, row_in(ti, rr) && wcol_in(wt), (16 * ti + 4 * rr + g) + n * (16 * wt + p));
      {  // the partial sums of C'v over this lane's rows
        double pc[WT];
#pragma unroll
        for (int wt = 0; wt < WT; wt++) pc[wt] = 0.0;
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const double vr = L.v[16 * ti + 4 * rr + g];
#pragma unroll
            for (int wt = 0; wt < WT; wt++) pc[wt] = __builtin_fma(Cn[ti][wt][rr], vr, pc[wt]);
          }
#pragma unroll
        for (int wt = 0; wt < WT; wt++) red[g * RS + 16 * wt + p] = pc[wt];
      }
      double4_t G[NT][WT];
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int wt = 0; wt < WT; wt++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(Vt[ks >> 2][ti][ks & 3], Cn[ks >> 2][wt][ks & 3], acc);
          G[ti][wt] = acc;
        }
      double Sn[WT][WT][4];
#pragma unroll
      for (int wi = 0; wi < WT; wi++)
#pragma unroll
        for (int wj = 0; wj < WT; wj++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(Cn[ks >> 2][wi][ks & 3], G[ks >> 2][wj][ks & 3], acc);
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            Sn[wi][wj][rr] = acc[rr];
            L.S[(16 * wi + 4 * rr + g) + LDX * (16 * wj + p)] = acc[rr];
          }
        }
      lds_sync();
      // M into L.A with the identity outside nw; the right-hand sides G' (and C'v beside them) into L.R
#pragma unroll
      for (int wi = 0; wi < WT; wi++)
#pragma unroll
        for (int wj = 0; wj < WT; wj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int a = 16 * wi + 4 * rr + g, c = 16 * wj + p;
            const double sv = 0.5 * (Sn[wi][wj][rr] + L.S[c + LDX * a]);
            const double id = a == c ? 1.0 : 0.0;
            L.A[a * LDA + c] = (a < nw && c < nw) ? id - theta * sv : id;
            if (a == c) L.tr[a] = sv;
          }
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int wt = 0; wt < WT; wt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) L.R[(16 * wt + p) * LDR + 16 * ti + 4 * rr + g] = G[ti][wt][rr];
      if (lane < W) L.R[lane * LDR + N] = red4(RS, lane);
    }
    lds_sync();
    double logsum = 0.0;
    if (!cholesky(nw, &logsum)) {
      failed = -(i + 1);
      break;
    }
    if (lane < N + 1) {  // forward substitution alone: R Y = G'
      for (int r = 0; r < nw; r++) {
        double s = L.R[r * LDR + lane];
#pragma unroll 8
        for (int k = 0; k < r; k++) s = __builtin_fma(-L.A[r * LDA + k], L.R[k * LDR + lane], s);
        L.R[r * LDR + lane] = s * L.dinv[r];
      }
    }
    lds_sync();
#pragma unroll
    for (int wt = 0; wt < WT; wt++)
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) Yn[wt][ti][rr] = L.R[(16 * wt + 4 * rr + g) * LDR + 16 * ti + p];
    // st = s + theta/2 y'y - (1/theta) sum log R(j, j), or s + 1/2 trace(C'G) at theta == 0
    {
      double acc = 0.0;
      if (theta != 0.0) {
        for (int j = 0; j < nw; j++) {
          const double yj = L.R[j * LDR + N];
          acc = __builtin_fma(yj, yj, acc);
        }
        sc = sc + 0.5 * theta * acc - logsum / theta;
      } else {
        for (int j = 0; j < nw; j++) acc += L.tr[j];
        sc = sc + 0.5 * acc;
      }
    }
    // the partial sums of Y'y over this lane's rows; Pt' = Vt + theta Y'Y
    {
      double yr[WT][4];
#pragma unroll
      for (int wt = 0; wt < WT; wt++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) yr[wt][rr] = L.R[(16 * wt + 4 * rr + g) * LDR + N];
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double s = 0.0;
#pragma unroll
        for (int wt = 0; wt < WT; wt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) s = __builtin_fma(Yn[wt][tj][rr], yr[wt][rr], s);
        red[g * RS + 16 * tj + p] = s;
      }
    }
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double4_t acc = zero4;
#pragma unroll
        for (int ks = 0; ks < 4 * WT; ks++) acc = mfma(Yn[ks >> 2][ti][ks & 3], Yn[ks >> 2][tj][ks & 3], acc);
#pragma unroll
        for (int rr = 0; rr < 4; rr++) Vt[ti][tj][rr] = Vt[ti][tj][rr] + theta * acc[rr];
      }
    lds_sync();
    if (lane < N) L.v[lane] = L.v[lane] + theta * red4(RS, lane);  // vt
    lds_sync();

    // ---- the gain step of k_lq_gain_w on (Pt, vt) ----
    const S* rk = Db + (size_t)i * REC;
    double fx[NT][NT][4], fu[NT][MT][4];
    phase();
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
    const double kx = (lane < n) ? (double)rk[oCX + lane] : 0.0;  // cx on lanes < n
    {  // the partial sums of fx'vt and fu'vt over this lane's rows
      double px[NT], pu[MT];
#pragma unroll
      for (int tj = 0; tj < NT; tj++) px[tj] = 0.0;
#pragma unroll
      for (int mt = 0; mt < MT; mt++) pu[mt] = 0.0;
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const double vr = L.v[16 * ti + 4 * rr + g];
#pragma unroll
          for (int tj = 0; tj < NT; tj++) px[tj] = __builtin_fma(fx[ti][tj][rr], vr, px[tj]);
#pragma unroll
          for (int mt = 0; mt < MT; mt++) pu[mt] = __builtin_fma(fu[ti][mt][rr], vr, pu[mt]);
        }
#pragma unroll
      for (int tj = 0; tj < NT; tj++) red[g * RS + 16 * tj + p] = px[tj];
#pragma unroll
      for (int mt = 0; mt < MT; mt++) red[g * RS + N + 16 * mt + p] = pu[mt];
    }
    // A1 = Pt fx (n x n), A2 = Pt fu (n x m)
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
    // Qx = cx + fx'vt, Qu = cu + fu'vt
    lds_sync();
    if (lane < N) L.Qx[lane] = kx + red4(RS, lane);
    if (lane < M) L.Qu[lane] = ((lane < m) ? (double)rk[oCU + lane] : 0.0) + red4(RS, N + lane);
    // Qxx = cxx + fx'A1 ; Qux = cxu' + fu'A1 ; Quu = cuu + fu'A2 + mu I
    double Qux[MT][NT][4], Quu[MT][MT][4];  // (Qxx rests in L.S until Pn is formed)
    phase();
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
    phase();
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
    phase();
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
    // The fixed-size system: held controls as identity rows and columns with zero right-hand sides (the rows >= m are never read)
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
        }
#pragma unroll
        for (int tj = 0; tj < NT; tj++) L.R[row * LDR + 16 * tj + p] = hrow ? 0.0 : Qux[mi][tj][rr];
      }
    if (lane < M) L.R[lane * LDR + N] = (lane >= m || L.nz[lane] == 0) ? 0.0 : L.Qu[lane];
    lds_sync();
    if (!cholesky(m, nullptr)) {
      failed = i + 1;
      break;
    }
    // L L' x = rhs, one lane per right-hand side, the column in place in L.R (only its own lane touches it); the solutions negated
    if (lane < N + 1) {
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
    phase();
    // K = -Quu^-1 Qux natural, k beside it; out, consecutive lanes to consecutive addresses
    double Kd[MT][NT][4];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) Kd[mt][tj][rr] = L.R[(16 * mt + 4 * rr + g) * LDR + 16 * tj + p];
    if (Ko) {
      double* o = Ko + (size_t)i * m * n;
      for (int e = lane; e < m * n; e += 64) {
        const int c = e / m, j = e - c * m;
        o[e] = L.R[j * LDR + c];
      }
    }
    if (ko && lane < m) ko[(size_t)i * m + lane] = L.R[lane * LDR + N];
    // s[t] = st + 1/2 Qu'k ; the partial sums of K'Qu over this lane's rows
    {
      double acc = 0.0;
      for (int j = 0; j < m; j++) acc = __builtin_fma(L.Qu[j], L.R[j * LDR + N], acc);
      sc = sc + 0.5 * acc;
      double qq[MT][4];
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) qq[mt][rr] = L.Qu[16 * mt + 4 * rr + g];
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double s = 0.0;
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) s = __builtin_fma(Kd[mt][tj][rr], qq[mt][rr], s);
        red[g * RS + 16 * tj + p] = s;
      }
    }
    // Pn = Qxx + Qux'K ; P = (Pn + Pn')/2, the transpose read back from LDS
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
    if (lane < N) {
      const double vx = L.Qx[lane] + red4(RS, lane);
      L.v[lane] = vx;  // (columns outside the model: sums of exact zeros)
      if (vxo && lane < n) vxo[(size_t)i * n + lane] = vx;
    }
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int a = 16 * ti + 4 * rr + g, c = 16 * tj + p;
          const double val = 0.5 * (Vt[ti][tj][rr] + L.S[c + LDX * a]);
          Vt[ti][tj][rr] = val;
          if (vxxo && a < n && c < n) vxxo[(size_t)i * n * n + c + (size_t)n * a] = val;  // symmetric to the bit: (a, c) written at (c, a)
        }
    lds_sync();
  }
  if (failed) {  // quiet NaNs in every output over the whole horizon, the knots this wavefront has written included (the fence: after those stores)
    __threadfence();
    const double qnan = __builtin_nan("");
    if (Ko)
      for (int e = lane; e < T * m * n; e += 64) Ko[e] = qnan;
    if (ko)
      for (int e = lane; e < T * m; e += 64) ko[e] = qnan;
    if (vxo)
      for (int e = lane; e < (T + 1) * n; e += 64) vxo[e] = qnan;
    if (vxxo)
      for (int e = lane; e < (T + 1) * n * n; e += 64) vxxo[e] = qnan;
  }
  if (lane == 0) {
    if (q.J) q.J[b] = failed ? __builtin_nan("") : sc;
    q.fail[b] = failed;
    if (q.info) q.info[b] = failed;
  }
}

}  // namespace ilqr
