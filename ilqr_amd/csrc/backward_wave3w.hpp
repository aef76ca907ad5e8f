// backward_wave3w.hpp -- the generic backward pass for 16 < m <= 32: k_backward_w3's step with TWO 16-column control tiles.
//
// One wavefront per trajectory, n <= 16 NT, m <= 32.  The control-side blocks are 2 x 16 rows in the same natural-register /
// MFMA layout k_backward_w3 uses (X[.][.][r] = X(16 t + 4 r + g, 16 t' + p), g = lane >> 4, p = lane & 15): fu (n x m), A2' = Vxx' fu,
// Qux (m x n), K (m x n), T1' = Quu' K, cuu / Quu (2 x 2 tiles), cxu; the matrix-vector products stay per-lane FMA chains over the
// natural registers + one reduction of the four row groups through LDS, as in k_backward_w3.
//
// The box-QP is the literal one in every step: w_box_qp<., WMW> (backward_wave.hpp) -- Eigen's unblocked LLT with partial and stale
// factors, boxqp.cpp:26-139 as written, 32 lanes wide.  (k_backward_w3's Newton-Schulz refinement of the previous knot's inverse
// is not carried over: its contraction test 16 x max|I - M X| < 1/2 would need a bound of its own at m = 32, and the literal QP
// is the reference's algorithm.  Where the refinement pays at m = 32 is a measurement for later.)
//
// Masks: a free set of 32 controls is a full 32-bit word, so no `(1u << m) - 1u` appears here; everything indexed by a control
// is reduced over lanes 0..31 (wave_sum_ctrl<WMW>, the 32-lane max of the gradient norm).
//
// LDS (Wave3WLds<NT>, <= 40 KB so that four wavefronts -- one per SIMD -- fit a CU): S holds QuuF | Minv (32 x 33 each) until the
// gains, then Vn for the symmetrisation; Quu, needed after the box-QP only for dV, waits in Kbuf (the K buffer of the stale-factor
// path, written after dV is taken); Tbuf holds Ri / the scattered inverse / Qux for the stale-factor path.
//
// What this kernel restates of k_backward_w3 (a fix to one of these sections belongs in both): the record loads and the Vxx[T] start,
// the fx'Vx / fu'Vx partial sums and their reduction, the A1' / A2' / Qxx / Qux products, the gains' stale-factor / nothing-free LDS path
// and the re-scattered inverse, dV, the Vx update, Vn and its symmetrisation through S, the stores, the lambda loop and the gradient norm.
// They are kept apart, not templated on the tile count, so that the nu <= 16 instantiations stay instruction for instruction what they were.
#pragma once
#include "backward_wave2.hpp"

namespace ilqr {

template <int NT>  // NT = 16-row tiles covering n: 1 (n <= 16) or 2 (n <= 32)
struct Wave3WLds {
  static constexpr int N = 16 * NT, LD = N + 1;
  static constexpr int S_LEN = (LD * N > 2 * LDMW * WMW) ? LD * N : 2 * LDMW * WMW;
  double S[S_LEN];          // QuuF | Minv (m x m, ld LDMW) until the gains; then Vn (ld LD) for the symmetrisation
  double Kbuf[LDMW * WMW];  // Quu (ld LDMW) from before the box-QP until dV; then K (m x n, ld LDMW) on the stale-factor path; reduction scratch
  double Tbuf[LDMW * WMW];  // Ri / the scattered Minv (m x m, ld LDMW); Qux (m x n) for the stale-factor path
  __device__ __forceinline__ double* K() { return Kbuf; }
  __device__ __forceinline__ double* Quu() { return Kbuf; }
  __device__ __forceinline__ double* QuuF() { return S; }
  __device__ __forceinline__ double* Minv() { return S + LDMW * WMW; }
  __device__ __forceinline__ double* Qf() { return Tbuf; }
  __device__ __forceinline__ double* Ri() { return Tbuf; }
  double Vx[N], cx[N], Qx[N];
  double Qu[WMW], x[WMW], grad[WMW], gc[WMW], search[WMW], lo[WMW], hi[WMW], clamped[WMW], xc[WMW], tmp[WMW], kprev[WMW],
      gfree[WMW], xfree[WMW];
  int vfree[WMW], idx[WMW];
};
static_assert(sizeof(Wave3WLds<2>) <= 40 * 1024, "one wavefront on every SIMD: 4 x LDS <= 160 KB");

// n <= 16 NT, m <= 32.  Arguments as k_backward_w3 (const_rec: the constant matrix blocks of a record, or null).  One wavefront per
// SIMD: up to 512 VGPR + AGPR per lane.
template <int NT>
__global__ __launch_bounds__(64, 1) void k_backward_w3w(BatchView v, int n, int m, const double* __restrict__ u_min,
                                                        const double* __restrict__ u_max, SolverParams sp, int mode,
                                                        const double* __restrict__ const_rec) {
  constexpr int MT = 2;  // 16-column control tiles
  __shared__ Wave3WLds<NT> L;
  constexpr int N = 16 * NT;
  constexpr int LDX = Wave3WLds<NT>::LD;
  constexpr int RS = N + WMW;  // stride of one row group's partial sums in the reduction scratch
  static_assert(4 * RS <= LDMW * WMW && 3 * 4 * N <= LDMW * WMW, "reduction scratch lives in Kbuf");
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= v.B) return;
  if (mode == 1 && v.status[b] != 0) return;
  const int T = v.T;
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0, oFU = oFX + n * n, oCX = oFU + n * m, oCXX = oCX + n, oCXU = oCXX + n * n, oCU = oCXU + n * m,
            oCUU = oCU + m;
  const double* __restrict__ Db = v.D + (size_t)b * (T + 1) * REC;
  const double* __restrict__ usb = v.us + (size_t)b * T * m;
  double* __restrict__ kb = v.kff + (size_t)b * T * m;
  double* __restrict__ Kb = v.Kfb + (size_t)b * T * m * n;
  double lambda = v.lambda[b], dlambda = v.dlambda[b];
  const int g = lane >> 4, p = lane & 15;
  {
    double* z = reinterpret_cast<double*>(&L);
    const int nz = (int)(sizeof(Wave3WLds<NT>) / sizeof(double));
    for (int e = lane; e < nz; e += 64) z[e] = 0.0;
  }
  lds_sync();
  double* const red = L.Kbuf;  // partial sums of the matrix-vector products, [row group][column]

  auto mfma = [](double a, double b2, double4_t c) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b2, c, 0, 0, 0);
  };
  const double4_t zero4 = {0.0, 0.0, 0.0, 0.0};
  // lane parts of the record addresses, made opaque once per step (k_backward_w2's note on hoisted addresses)
  unsigned lb_nn = (unsigned)(g + n * p);
  unsigned lb_tn = (unsigned)(p + n * g);
  unsigned lb_mm = (unsigned)(g + m * p);
  auto ldm = [](const double* r, bool in, unsigned off) __attribute__((always_inline)) {
    const double val = r[in ? off : 0u];
    return in ? val : 0.0;
  };
  auto row_in = [&](int a0) __attribute__((always_inline)) { return a0 + g < n; };          // state row a0 + g
  auto col_in = [&](int tj) __attribute__((always_inline)) { return 16 * tj + p < n; };     // state column 16 tj + p
  auto mrow_in = [&](int mt, int rr) __attribute__((always_inline)) { return 16 * mt + 4 * rr + g < m; };  // control row
  auto mcol_in = [&](int mt) __attribute__((always_inline)) { return 16 * mt + p < m; };    // control column
  auto red4 = [&](int col) __attribute__((always_inline)) { return ((red[col] + red[RS + col]) + red[2 * RS + col]) + red[3 * RS + col]; };

  int diverge = 0;
  bool done = false;
  double dV0 = 0, dV1 = 0;
#ifdef ILQR_W2_TIMING
  W2Clock clk;  // (experiment builds: the box-QP's sections and counts; the step is not divided into sections here)
  clk.start();
#endif
  while (true) {
    double Vxx[NT][NT][4];
    {  // :353-354
      const double* r = Db + (size_t)T * REC;
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int a0 = 16 * ti + 4 * rr;
            Vxx[ti][tj][rr] = ldm(r, row_in(a0) && col_in(tj), lb_nn + (unsigned)(oCXX + a0 + n * 16 * tj));
          }
      for (int e = lane; e < n; e += 64) L.Vx[e] = r[oCX + e];
      if (lane < m) L.kprev[lane] = kb[(size_t)(T - 1) * m + lane];
    }
    dV0 = dV1 = 0;
    diverge = 0;
    lds_sync();
    for (int i = T - 1; i >= 0; i--) {
      const double* rk = Db + (size_t)i * REC;        // this knot's record (cx, cu, and the matrices unless const_rec has them)
      const double* rm = const_rec ? const_rec : rk;  // ... its matrix blocks
      double fx[NT][NT][4], fu[NT][MT][4];
      double kx = 0, ku = 0;  // cx on lanes < n, cu on lanes N .. N + m - 1
      {
        asm volatile("" : "+v"(lb_nn));
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int a0 = 16 * ti + 4 * rr;
            const bool ain = row_in(a0);
#pragma unroll
            for (int tj = 0; tj < NT; tj++) fx[ti][tj][rr] = ldm(rm, ain && col_in(tj), lb_nn + (unsigned)(oFX + a0 + n * 16 * tj));
#pragma unroll
            for (int mt = 0; mt < MT; mt++) fu[ti][mt][rr] = ldm(rm, ain && mcol_in(mt), lb_nn + (unsigned)(oFU + a0 + n * 16 * mt));
          }
        const double us_l = (lane < m) ? usb[(size_t)i * m + lane] : 0.0;
        kx = (lane < n) ? rk[oCX + lane] : 0.0;
        ku = (lane >= N && lane - N < m) ? rk[oCU + lane - N] : 0.0;
        if (lane < m) {
          L.lo[lane] = u_min[lane] - us_l;  // :369
          L.hi[lane] = u_max[lane] - us_l;
        }
      }
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
      // A1' = Vxx' fx (n x n), A2' = Vxx' fu (n x m)
      double4_t a1t[NT][NT], a2t[NT][MT];
#pragma unroll
      for (int ti = 0; ti < NT; ti++) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++) a2t[ti][mt] = zero4;
#pragma unroll
        for (int tj = 0; tj < NT; tj++) a1t[ti][tj] = zero4;
      }
#pragma unroll
      for (int ks = 0; ks < 4 * NT; ks++) {
#pragma unroll
        for (int ti = 0; ti < NT; ti++) {
#pragma unroll
          for (int tj = 0; tj < NT; tj++) a1t[ti][tj] = mfma(Vxx[ks >> 2][ti][ks & 3], fx[ks >> 2][tj][ks & 3], a1t[ti][tj]);
#pragma unroll
          for (int mt = 0; mt < MT; mt++) a2t[ti][mt] = mfma(Vxx[ks >> 2][ti][ks & 3], fu[ks >> 2][mt][ks & 3], a2t[ti][mt]);
        }
      }
      // :361 Qxx = cxx + A1 fx ; :362 Qux = cxu' + A2 fx ; :363/:367 Quu, QuuF = cuu (+ lambda I) + A2 fu
      double Qxx[NT][NT][4], Qux[MT][NT][4], quu_nat[MT][MT][4];
      {  // Quu: 2 x 2 tiles
        asm volatile("" : "+v"(lb_mm));
#pragma unroll
        for (int mi = 0; mi < MT; mi++)
#pragma unroll
          for (int mj = 0; mj < MT; mj++) {
            double4_t quu = zero4;
#pragma unroll
            for (int ks = 0; ks < 4 * NT; ks++) quu = mfma(a2t[ks >> 2][mi][ks & 3], fu[ks >> 2][mj][ks & 3], quu);
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
              const int a = 16 * mi + 4 * rr + g, c = 16 * mj + p;
              const bool in = mrow_in(mi, rr) && mcol_in(mj);
              const double cu2 = ldm(rm, in, lb_mm + (unsigned)(oCUU + 16 * mi + 4 * rr + m * 16 * mj));
              quu_nat[mi][mj][rr] = in ? cu2 + quu[rr] : 0.0;
              L.QuuF()[a + LDMW * c] = in ? (cu2 + ((a == c) ? lambda : 0.0)) + quu[rr] : 0.0;
            }
          }
      }
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {  // one 16-column block of the outputs at a time (registers)
        __builtin_amdgcn_sched_barrier(0);
        double cxx[NT][4], cxu[MT][4];
        {
          asm volatile("" : "+v"(lb_nn), "+v"(lb_tn));
#pragma unroll
          for (int ti = 0; ti < NT; ti++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
              const int a0 = 16 * ti + 4 * rr;
              cxx[ti][rr] = ldm(rm, row_in(a0) && col_in(tj), lb_nn + (unsigned)(oCXX + a0 + n * 16 * tj));
            }
#pragma unroll
          for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++)  // Qux(a, c) starts from cxu(c, a): offset c + n a
              cxu[mt][rr] = ldm(rm, mrow_in(mt, rr) && col_in(tj), lb_tn + (unsigned)(oCXU + 16 * tj + n * (16 * mt + 4 * rr)));
        }
        __builtin_amdgcn_sched_barrier(0);
        double4_t qxx[NT], qux[MT];
#pragma unroll
        for (int ti = 0; ti < NT; ti++) qxx[ti] = zero4;
#pragma unroll
        for (int mt = 0; mt < MT; mt++) qux[mt] = zero4;
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ks++) {
#pragma unroll
          for (int ti = tj; ti < NT; ti++) qxx[ti] = mfma(a1t[ks >> 2][ti][ks & 3], fx[ks >> 2][tj][ks & 3], qxx[ti]);  // (tiles on and below the diagonal: see Vn)
#pragma unroll
          for (int mt = 0; mt < MT; mt++) qux[mt] = mfma(a2t[ks >> 2][mt][ks & 3], fx[ks >> 2][tj][ks & 3], qux[mt]);
        }
#pragma unroll
        for (int ti = tj; ti < NT; ti++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const double val = cxx[ti][rr] + qxx[ti][rr];
            Qxx[ti][tj][rr] = (row_in(16 * ti + 4 * rr) && col_in(tj)) ? val : 0.0;
          }
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const double val = cxu[mt][rr] + qux[mt][rr];
            Qux[mt][tj][rr] = (mrow_in(mt, rr) && col_in(tj)) ? val : 0.0;
          }
      }
      // Qx = cx + fx'Vx, Qu = cu + fu'Vx: the four row groups' partial sums through the scratch
#pragma unroll
      for (int tj = 0; tj < NT; tj++) red[g * RS + 16 * tj + p] = px[tj];
#pragma unroll
      for (int mt = 0; mt < MT; mt++) red[g * RS + N + 16 * mt + p] = pu[mt];
      lds_sync();
      if (lane < N) {
        const double s = red4(lane);
        L.Qx[lane] = (lane < n) ? kx + s : 0.0;
      } else if (lane < N + WMW) {
        const double s = red4(lane);
        L.Qu[lane - N] = (lane - N < m) ? ku + s : 0.0;
      }
      lds_sync();
      // Quu for dV, into the scratch that the sums above have left
#pragma unroll
      for (int mi = 0; mi < MT; mi++)
#pragma unroll
        for (int mj = 0; mj < MT; mj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) L.Quu()[(16 * mi + 4 * rr + g) + LDMW * (16 * mj + p)] = quu_nat[mi][mj][rr];
      lds_sync();
      int nfR = 0, nfact = 0;
      const int result = w_box_qp<Wave3WLds<NT>, WMW>(m, L, lane, nfR ILQR_W2CLOCK_PASS, &nfact, sp.fixes);
      const unsigned free_mask = (unsigned)__ballot(lane < m && L.vfree[lane]);
      if (result < 1) {  // :371
        diverge = i;
        break;
      }
      // :388-389 (Quu still in Kbuf: taken before the gains may overwrite it)
      {
        const double d0 = wave_sum_ctrl<WMW>(lane < m ? L.x[lane] * L.Qu[lane] : 0.0);
        double part = 0;
        if (lane < m) {
          const double rr = dot_padded<WMW>([&](int a) { return 0.5 * L.x[a]; }, [&](int a) { return L.Quu()[a + LDMW * lane]; });
          part = rr * L.x[lane];
        }
        dV0 += d0;
        dV1 += wave_sum_ctrl<WMW>(part);
      }
      lds_sync();
      // :373-385  K rows of free dims, natural registers K[mt][tj][r] = K(16 mt + 4 r + g, 16 tj + p)
      double K[MT][NT][4];
      const int nf = __popc(free_mask);
      const unsigned long long fm64 = free_mask;
      if (nf > 0 && nf == nfR) {
        double* MF = L.Qf();
        if (nf == m) {
          MF = L.Minv();
        } else {
          if (lane < m && L.vfree[lane]) L.idx[__popcll(fm64 & ((1ull << lane) - 1ull))] = lane;
          for (int e = lane; e < LDMW * WMW; e += 64) MF[e] = 0.0;
          lds_sync();
          for (int e = lane; e < nf * nf; e += 64) {
            const int a = e % nf, b2 = e / nf;
            MF[L.idx[a] + LDMW * L.idx[b2]] = L.Minv()[a + LDMW * b2];
          }
          lds_sync();
        }
        // K = -MF Qux: MF symmetric, tile (mt, kt) as the A operand; zero rows / columns outside the free set add exact zeros
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
          double aM[MT][4];
#pragma unroll
          for (int kt = 0; kt < MT; kt++) ld_operand<4>([&](int i2, int k) { return MF[(16 * mt + i2) + LDMW * (16 * kt + k)]; }, lane, aM[kt]);
#pragma unroll
          for (int tj = 0; tj < NT; tj++) {
            double4_t acc = zero4;
#pragma unroll
            for (int kt = 0; kt < MT; kt++)
#pragma unroll
              for (int ks = 0; ks < 4; ks++) acc = mfma(aM[kt][ks], Qux[kt][tj][ks], acc);
#pragma unroll
            for (int rr = 0; rr < 4; rr++) K[mt][tj][rr] = -acc[rr];
          }
        }
      } else {  // nothing free, or a stale factor of another size (:80): through LDS, as k_backward_w3 does
        if (lane < m && L.vfree[lane]) L.idx[__popcll(fm64 & ((1ull << lane) - 1ull))] = lane;
        for (int e = lane; e < LDMW * N; e += 64) L.K()[e] = 0;  // (every column read back below: Kbuf held Quu until dV)
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int tj = 0; tj < NT; tj++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) L.Tbuf[(16 * mt + 4 * rr + g) + LDMW * (16 * tj + p)] = Qux[mt][tj][rr];
        lds_sync();
        if (nf > 0) {
          const int nuse = (nf < nfR) ? nf : nfR;
          for (int e = lane; e < nuse * n; e += 64) {
            const int rr = e % nuse, c = e / nuse;
            double acc = 0;
            for (int l2 = 0; l2 < nuse; l2++) acc += -L.Minv()[rr + LDMW * l2] * L.Tbuf[L.idx[l2] + LDMW * c];
            L.K()[L.idx[rr] + LDMW * c] = acc;
          }
        }
        lds_sync();
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int tj = 0; tj < NT; tj++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) K[mt][tj][rr] = L.K()[(16 * mt + 4 * rr + g) + LDMW * (16 * tj + p)];
      }
      lds_sync();
      // T1' = Quu' K (m x n): Quu's natural registers are its A operand
      double4_t t1t[MT][NT];
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          t1t[mt][tj] = zero4;
#pragma unroll
          for (int kt = 0; kt < MT; kt++)
#pragma unroll
            for (int ks = 0; ks < 4; ks++) t1t[mt][tj] = mfma(quu_nat[kt][mt][ks], K[kt][tj][ks], t1t[mt][tj]);
        }
      // :391 Vx = ((Qx + T1 k) + K'Qu) + Qux'k: per-lane partial sums over the rows 16 mt + 4 r + g, three sums kept apart
      {
        double xq[MT][4], qq[MT][4];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            xq[mt][rr] = L.x[16 * mt + 4 * rr + g];
            qq[mt][rr] = L.Qu[16 * mt + 4 * rr + g];
          }
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          double s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
          for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
              s1 = __builtin_fma(t1t[mt][tj][rr], xq[mt][rr], s1);
              s2 = __builtin_fma(K[mt][tj][rr], qq[mt][rr], s2);
              s3 = __builtin_fma(Qux[mt][tj][rr], xq[mt][rr], s3);
            }
          red[(0 * 4 + g) * N + 16 * tj + p] = s1;
          red[(1 * 4 + g) * N + 16 * tj + p] = s2;
          red[(2 * 4 + g) * N + 16 * tj + p] = s3;
        }
        lds_sync();
        if (lane < N) {
          auto sum4 = [&](int q) __attribute__((always_inline)) {
            return ((red[(q * 4 + 0) * N + lane] + red[(q * 4 + 1) * N + lane]) + red[(q * 4 + 2) * N + lane]) + red[(q * 4 + 3) * N + lane];
          };
          const double vx = ((L.Qx[lane] + sum4(0)) + sum4(1)) + sum4(2);
          L.Vx[lane] = (lane < n) ? vx : 0.0;
        }
      }
      lds_sync();  // (QuuF, Minv have been read: S may take Vn)
      // :392 Vn = ((Qxx + T1 K) + K'Qux) + Qux'K ; :393 Vxx = (Vn + Vn')/2 through S -- the tiles on and below the diagonal, as k_backward_w3
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj <= ti; tj++) {
          double4_t p1 = zero4, p2 = zero4, p3 = zero4;
#pragma unroll
          for (int kt = 0; kt < MT; kt++)
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
              p1 = mfma(t1t[kt][ti][ks], K[kt][tj][ks], p1);
              p2 = mfma(K[kt][ti][ks], Qux[kt][tj][ks], p2);
              p3 = mfma(Qux[kt][ti][ks], K[kt][tj][ks], p3);
            }
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const double vn = ((Qxx[ti][tj][rr] + p1[rr]) + p2[rr]) + p3[rr];
            Vxx[ti][tj][rr] = vn;
            L.S[(16 * ti + 4 * rr + g) + LDX * (16 * tj + p)] = vn;
          }
        }
      lds_sync();
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const double tr = L.S[(16 * tj + p) + LDX * (16 * ti + 4 * rr + g)];  // Vn(column, row)
            if (ti == tj) Vxx[ti][tj][rr] = 0.5 * (Vxx[ti][tj][rr] + tr);
            else if (ti < tj) Vxx[ti][tj][rr] = tr;   // (ti > tj: Vn itself)
          }
      // :396-397
      if (lane < m) {
        kb[(size_t)i * m + lane] = L.x[lane];
        L.kprev[lane] = L.x[lane];
      }
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            if (mrow_in(mt, rr) && col_in(tj)) Kb[(size_t)i * m * n + (16 * mt + 4 * rr + g) + m * (16 * tj + p)] = K[mt][tj][rr];
          }
      lds_sync();
    }
    if (mode == 0) {
      done = (diverge == 0);
      break;
    }
    if (diverge != 0) {  // :142-148
      dlambda = fmax(dlambda * sp.lambda_factor, sp.lambda_factor);
      lambda = fmax(lambda * dlambda, sp.lambda_min);
      if (lambda > sp.lambda_max) break;
      continue;
    }
    done = true;
    break;
  }
#ifdef ILQR_W2_TIMING
  clk.flush();
#endif
  // :153 / :405-412 gradient norm: mean_t max_j |k_j| / (|u_j| + 1), ascending t -- the max over lanes 0..31
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0);
  double acc = 0;
  for (int t = 0; t < T; t++) {
    double val = -1.0;
    if (lane < m) val = fabs(kb[(size_t)t * m + lane]) / (fabs(usb[(size_t)t * m + lane]) + 1);
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) val = fmax(val, __shfl_xor(val, off, 64));
    acc += __shfl(val, 0, 64);
  }
  const double gnorm = acc / T;
  if (lane == 0) {
    v.dV[b] = dV0;
    v.dV[v.Bp + b] = dV1;
    v.diverge[b] = diverge;
    v.backpass_done[b] = done ? 1 : 0;
    v.gnorm[b] = gnorm;
    if (mode == 1) {
      v.lambda[b] = lambda;
      v.dlambda[b] = dlambda;
      if (!sp.fixed_work && gnorm < sp.tol_grad && lambda < 1e-5) {
        v.status[b] = 1;
        v.iters[b] += 1;
      }
    }
  }
}

}  // namespace ilqr
