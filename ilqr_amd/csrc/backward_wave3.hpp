// backward_wave3.hpp -- the generic backward pass (n <= 32, m <= 32; one wavefront per trajectory) with the fp64 pipe's
// cycles counted: k_backward_w2's register layout, minus the work that layout does not need.
//
// What bounds k_backward_w2 (profiles/r05a_w2_sections.txt, scripts/ubench/coissue.hip): on gfx950 a v_mfma_f64_16x16x4_f64
// occupies the SIMD's fp64 datapath for 64.8 cycles -- exactly the 16 v_fma_f64 issue slots its 1024 multiply-adds are worth --
// and fp64 VALU instructions of the OTHER wavefront on that SIMD do not issue meanwhile (one MFMA + one FMA wavefront per SIMD:
// the FMA loop waits for the MFMA loop to end).  A step's cost is therefore the SUM of its MFMAs x 64.8 and its VALU
// instructions x ~4.5 cycles, whatever overlaps in time: 216 MFMAs + 3650 VALU + 690 SALU instructions per step in
// k_backward_w2<2>.  This kernel removes pipe cycles, not latency:
//   * matrix-VECTOR products (Qx, Qu, the Vx update: 48 MFMAs whose B operand was one vector in 16 identical columns) are
//     per-lane FMA chains over the natural registers + one cross-row-group reduction through LDS: ~80 VALU instructions;
//   * the box-QP's factorisation (Cholesky row by row over v_readlane broadcasts, triangular inverse, R^-1 R^-T: ~1450 VALU
//     instructions on 16 of 64 lanes, 28 % of a step) is replaced, when the free set is the previous step's, by a
//     NEWTON-SCHULZ REFINEMENT OF THE PREVIOUS STEP'S INVERSE ON THE MATRIX CORES: X <- X + X (I - M X), two 16x16x16
//     products = 8 MFMAs per iteration, everything in natural registers (M and X are symmetric: a natural register set is its
//     own A operand), two or three iterations from a neighbour's inverse.  Quu changes by a few per cent from one knot to the
//     next, the residual I - M X measures exactly how much, and anything that does not contract (a changed free set, a
//     non-positive-definite block, an ill-conditioned one) takes the literal path (w_box_qp: Eigen's unblocked LLT, partial
//     factors, stale factors, boxqp.cpp:80-119 as written), after which the inverse is re-seeded.  Convergence from a positive
//     definite neighbour with ||I - M X|| < 1/2 implies M positive definite, so the cases where the reference's LLT stops
//     early are never taken here.  The result differs from R^-1 R^-T by rounding (both are M^-1 to ~1e-16 cond(M));
//   * free / clamped sets as MASKS (clamped rows and columns of M replaced by the identity, of the inverse by zeros): no
//     compaction, no scatter -- masked-out terms add exact zeros to the same ascending sums;
//   * FULL (n = 16 NT, m = 16: BASELINE configs[4]): no bounds predicates on loads, sums or stores;
//   * LQF (LQ model with exact derivatives): the record's constant blocks come from const_rec as before, and cx = cxx x_t,
//     cu = cuu u_t are formed here from the knot -- per-lane FMAs on the cxx / cuu registers the step loads anyway, folded
//     into the same reduction as fx'Vx -- so no record array exists at all for that mode (44 GB at configs[4]) and no sweep
//     kernel runs; knot T's cxx (= sym(Qf)) is a second constant record.
// Everything else (operand maps, transposed products, the symmetrisation through LDS, the lambda-retry loop, the gradient
// norm) is k_backward_w2's; gains agree with it to rounding, not to the bit (tests/test_gpu_generic_backward.py).
//
// 16 < m <= 32 (and ILQR_ROUTE_TWO_CONTROL_TILES on m <= 16; the handle reports the stage as "k_backward_w3w"): the same step with
// MT = 2 control tiles -- fu, A2', Qux, K, T1', cxu in two 16-row tiles, cuu / Quu as 2 x 2 tiles, everything indexed by a control
// reduced over lanes 0..31.  Its box-QP is the literal one in every step, w_box_qp<., 32>: the refinement's contraction test
// 16 x max|I - M X| < 1/2 would need a bound of its own at m = 32, and the literal QP is the reference's algorithm.  A free set of
// 32 controls is a full 32-bit word, so that route never forms `(1u << m) - 1u` (only the refinement does).  Its LDS is Wave3WLds.
#pragma once
#include <type_traits>

#include "backward_wave2.hpp"

namespace ilqr {

constexpr int kQpBail = -100;        // the fast box-QP hands the QP to the literal path
constexpr double kNsStart = 0.03;    // max |I - M X| entry a warm start may have: ||I - M X||_2 <= 16 x that < 1/2
constexpr double kNsDone = 1e-9;     // ... below which one more update leaves a residual of ~(16 x 1e-9)^2
constexpr double kNsExact = 4e-15;   // ... and below which the update would change nothing (|I - M X| at rounding level)
constexpr int kNsMaxIter = 6;

#ifdef ILQR_W2_TIMING
__device__ long long g_w3_counts[4];  // QPs on the fast path, QPs handed to the literal path, Newton-Schulz iterations, (free)
#define ILQR_W3COUNT(k, n_) { if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((unsigned long long*)&g_w3_counts[k], (unsigned long long)(n_)); }
#else
#define ILQR_W3COUNT(k, n_)
#endif

// max over the 64 lanes (result in all lanes); NaN-propagating enough for a guard: a NaN anywhere makes `rho < bound` false
__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, dpp_f64<0xB1>(v));
  v = fmax(v, dpp_f64<0x4E>(v));
  v = fmax(v, dpp_f64<0x141>(v));
  v = fmax(v, dpp_f64<0x140>(v));
  auto row = [&](int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
  };
  return fmax(fmax(row(0), row(16)), fmax(row(32), row(48)));
}

// The warm start of the inverse and the state that says what it is the inverse of.
struct NsState {
  unsigned mask = 0;   // free set (bit i = control i free) the stored X belongs to
  bool valid = false;
};

// Newton-Schulz refinement of the stored inverse for the free set `fmask` of Q (m x m in LDS, ld LDM).  M~ = Q on the free
// rows / columns, the identity elsewhere.  On success: Xm = the masked inverse (zeros on clamped rows / columns) in natural
// registers (row 4 r + g, column p), also written to L.Minv(); the unmasked X back to Xw.  False: did not contract.
template <class LDS>
__device__ __forceinline__ bool ns_refine(LDS& L, const double* Q, double* Xw, unsigned fmask, int lane, double (&Xm)[4]) {
  const int g = lane >> 4, p = lane & 15;
  const bool fp = (fmask >> p) & 1u;
  double negM[4], X[4], id[4];
  bool fa[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int a = 4 * r + g;
    fa[r] = (fmask >> a) & 1u;
    id[r] = (a == p) ? 1.0 : 0.0;
    const double q = Q[a + LDM * p];
    negM[r] = (fa[r] && fp) ? -q : -id[r];
    X[r] = Xw[64 * r + lane];
  }
  bool done = false;
  int its = 0;
#pragma unroll 1
  for (int it = 0; it < kNsMaxIter; it++) {
    double4_t R = {id[0], id[1], id[2], id[3]};
#pragma unroll
    for (int ks = 0; ks < 4; ks++) R = __builtin_amdgcn_mfma_f64_16x16x4f64(negM[ks], X[ks], R, 0, 0, 0);  // I - M X
    const double rho = wave_max(fmax(fmax(fabs(R[0]), fabs(R[1])), fmax(fabs(R[2]), fabs(R[3]))));
    if (!(rho < kNsStart)) break;  // not a contraction (or NaN): the literal factorisation
    if (rho < kNsExact) {          // X is M's inverse to rounding already (a recursion that has reached its fixed point)
      done = true;
      break;
    }
    double4_t Xn = {X[0], X[1], X[2], X[3]};
#pragma unroll
    for (int ks = 0; ks < 4; ks++) Xn = __builtin_amdgcn_mfma_f64_16x16x4f64(X[ks], R[ks], Xn, 0, 0, 0);  // X + X R
#pragma unroll
    for (int r = 0; r < 4; r++) X[r] = Xn[r];
    its++;
    if (rho < kNsDone) {
      done = true;
      break;
    }
  }
  ILQR_W3COUNT(2, its)
  if (!done) return false;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    Xw[64 * r + lane] = X[r];
    Xm[r] = (fa[r] && fp) ? X[r] : 0.0;
    L.Minv()[(4 * r + g) + LDM * p] = Xm[r];
  }
  return true;
}

// src/boxqp.cpp:26-139 for one trajectory per wavefront, free / clamped sets as masks, the factorisation replaced by
// ns_refine.  Inputs in LDS as w_box_qp's (QuuF, Qu, kprev, lo, hi).  Returns the reference's result code -- then L.x holds the
// solution, free_out the free set at the exit, Xm the masked inverse of the last factor (all zero if nothing is free) -- or
// kQpBail: the caller runs w_box_qp on the same inputs.  The vector arithmetic is w_box_qp's expression for expression (same
// LDS operands, same sums); what it skips are recomputations of values it already holds (the gradient inside the slope, the
// old value after the first iteration, Q (x .* clamped) when nothing is clamped).
template <class LDS>
__device__ int w3_box_qp_fast(int m, LDS& L, int lane, double* Xw, NsState& ns, double (&Xm)[4], unsigned& free_out) {
  const double* Q = L.QuuF();
  const double* c = L.Qu;
  const bool mine = lane < m;
  double x = 0, lo = 0, hi = 0, cc = 0;
  if (mine) {
    lo = L.lo[lane];
    hi = L.hi[lane];
    cc = c[lane];
    const double k0 = L.kprev[lane];
    const double a = (k0 < lo) ? lo : k0;  // :35
    x = (hi < a) ? hi : a;
    L.x[lane] = x;
  }
#pragma unroll
  for (int r = 0; r < 4; r++) Xm[r] = 0.0;
  lds_sync();
  double val;  // :36 x'Qx + x.c (no 1/2)
  {
    double part = 0, lin = 0;
    if (mine) {
      const double r = dot_padded([&](int i) { return L.x[i]; }, [&](int i) { return Q[i + LDM * lane]; });
      part = r * x;
      lin = x * cc;
    }
    val = wave_sum_row0(part) + wave_sum_row0(lin);
  }
  double oldvalue = 0;
  int result = 0;
  unsigned clamped_mask = 0, fmask_factor = 0;
  for (int iter = 0; iter <= kQpMaxIter; iter++) {
    if (iter > 0 && (oldvalue - val) < kMinRelImprove * fabs(oldvalue)) {  // :54-57
      result = 4;
      break;
    }
    // :58 grad = Qx + c ; :62-71 clamped set
    double gr = 0;
    bool isc = false;
    if (mine) {
      const double s = dot_padded([&](int j) { return Q[lane + LDM * j]; }, [&](int j) { return L.x[j]; });
      gr = s + cc;
      isc = (fabs(x - lo) < kClampTol && gr > 0) || (fabs(x - hi) < kClampTol && gr < 0);
    }
    oldvalue = val;
    const unsigned free_mask = (unsigned)__ballot(mine && !isc);
    const unsigned new_clamped = (unsigned)__ballot(mine && isc);
    const bool count_changed = __popc(clamped_mask) != __popc(new_clamped);  // sum(old_clamped - clamped) != 0, :80
    clamped_mask = new_clamped;
    if (free_mask == 0) {  // :74-77
      result = 6;
      break;
    }
    if (iter == 0 || count_changed) {  // :80
      if (!(ns.valid && ns.mask == free_mask)) return kQpBail;
      if (!ns_refine(L, Q, Xw, free_mask, lane, Xm)) {
        ns.valid = false;
        return kQpBail;
      }
      fmask_factor = free_mask;
      lds_sync();
    } else if (fmask_factor != free_mask) {
      return kQpBail;  // a stale factor of another set of equal size (:80): the literal path knows how the reference misuses it
    }
    // :93-97
    {
      const double gn2 = wave_sum_row0((mine && !isc) ? gr * gr : 0.0);
      if (grad_norm_below_min(gn2)) {
        result = 5;
        break;
      }
    }
    // :100 grad_clamped = Q (x .* clamped) + c
    double gcv = cc;
    if (new_clamped != 0) {
      if (mine) L.tmp[lane] = x * (isc ? 1.0 : 0.0);
      lds_sync();
      if (mine) {
        const double s = dot_padded([&](int j) { return Q[lane + LDM * j]; }, [&](int j) { return L.tmp[j]; });
        gcv = s + cc;
      }
    }
    if (mine) L.gc[lane] = gcv;
    lds_sync();
    // :103-119 search(free) = -(R^-1 R^-T) gc(free) - x(free), 0 elsewhere: the masked inverse has zero rows / columns there
    double srch = 0;
    if (mine) {
      const double s = dot_padded([&](int l2) { return -L.Minv()[lane + LDM * l2]; }, [&](int l2) { return L.gc[l2]; });
      srch = isc ? 0.0 : s - x;
      L.search[lane] = srch;
    }
    lds_sync();
    // :121 quadclamp_line_search (src/boxqp.cpp:143-178)
    bool failed = false;
    double v = 0, xcv = 0;
    {
      const double slope = wave_sum_row0(mine ? srch * gr : 0.0);  // search . (Q x + c): the gradient above, same expression
      if (slope >= 0) {
        failed = true;
      } else {
        double step = 1;
        if (mine) {
          const double xr = x + step * srch;
          const double a = (xr < lo) ? lo : xr;
          xcv = (hi < a) ? hi : a;
          L.xc[lane] = xcv;
        }
        lds_sync();
        v = w_quad_cost(m, Q, c, L.xc, lane);
        const double old_v = (iter == 0) ? w_quad_cost(m, Q, c, L.x, lane) : val;  // (iter > 0: val IS quadCost(x), the last search's)
        while ((v - old_v) > kArmijo * (step * slope)) {
          step *= kStepDec;
          lds_sync();
          if (mine) {
            const double xr = x + step * srch;
            const double a = (xr < lo) ? lo : xr;
            xcv = (hi < a) ? hi : a;
            L.xc[lane] = xcv;
          }
          lds_sync();
          v = w_quad_cost(m, Q, c, L.xc, lane);
          if (step < kMinStep) {
            failed = true;
            break;
          }
        }
      }
    }
    if (failed) {  // :122-125, x not updated
      result = 2;
      break;
    }
    lds_sync();
    if (mine) {
      x = xcv;  // :133-134
      L.x[lane] = x;
    }
    val = v;
    lds_sync();
  }
  lds_sync();
  free_out = ((1u << m) - 1u) & ~clamped_mask;
  if (free_out == 0) {
#pragma unroll
    for (int r = 0; r < 4; r++) Xm[r] = 0.0;
  }
  return result;
}

// m <= 2 (what most models outside configs[4] have: one or two controls): the box-QP as the thread-level solvers of boxqp.hpp that the
// nx = 4 kernels use (box_qp_scalar / box_qp2: registers, no LDS round trips), every lane on the same values; the outputs go where
// w_box_qp leaves its own (L.x, L.vfree, the compact R^-1 R^-T in L.Minv()), so the step continues exactly as after the literal path.
// A sixteen-lane wave-level QP for a 1 x 1 or 2 x 2 block was 10-15 K cycles of a 30 K-cycle step at n = 6, m = 2.
template <class LDS>
__device__ __forceinline__ int w3_box_qp_small(int m, LDS& L, int lane, int& nfR_out, int fixes) {
  const double* Qm = L.QuuF();
  int result, nfR;
  if (m == 1) {
    double x;
    int fr;
    double minv;
    const double Q1 = Qm[0], c1 = L.Qu[0], k0 = L.kprev[0], lo1 = L.lo[0], hi1 = L.hi[0];
    result = box_qp_scalar(Q1, c1, k0, lo1, hi1, x, fr, minv);
    if (fixes & 2) {  // opt-in: a failed factorisation ends the QP (boxqp.cpp:85-88 with info() checked).  The 1 x 1 block is factored in
      // iteration 0 unless the start is clamped there (:62-77)
      const double xs0 = (hi1 < ((k0 < lo1) ? lo1 : k0)) ? hi1 : ((k0 < lo1) ? lo1 : k0), g0 = Q1 * xs0 + c1;
      const bool clamped0 = (fabs(xs0 - lo1) < kClampTol && g0 > 0) || (fabs(xs0 - hi1) < kClampTol && g0 < 0);
      if (!clamped0 && !(Q1 > 0.0)) result = -1;
    }
    nfR = 1;  // (the factor the solver holds at its exit is 1 x 1 whenever one was formed; nothing free: K = 0 below)
    lds_sync();
    for (int e = lane; e < LDM * WM; e += 64) L.Minv()[e] = 0.0;  // (the tile is read whole by the K product: S's leftovers are not zeros)
    lds_sync();
    if (lane == 0) {
      L.x[0] = x;
      L.vfree[0] = fr;
      L.Minv()[0] = minv;
    }
  } else {
    const double Q2[4] = {Qm[0], Qm[1], Qm[LDM], Qm[1 + LDM]};
    const double c2[2] = {L.Qu[0], L.Qu[1]}, x02[2] = {L.kprev[0], L.kprev[1]}, lo2[2] = {L.lo[0], L.lo[1]}, hi2[2] = {L.hi[0], L.hi[1]};
    BoxQP2Result<double> r;
    box_qp2(Q2, c2, x02, lo2, hi2, r, (fixes & 2) != 0);
    result = r.result;
    nfR = r.nfR;
    lds_sync();
    for (int e = lane; e < LDM * WM; e += 64) L.Minv()[e] = 0.0;
    lds_sync();
    if (lane == 0) {
      L.x[0] = r.x[0];
      L.x[1] = r.x[1];
      L.vfree[0] = r.free0 ? 1 : 0;
      L.vfree[1] = r.free1 ? 1 : 0;
      L.Minv()[0] = r.m00;
      L.Minv()[1] = r.m01;
      L.Minv()[LDM] = r.m01;
      L.Minv()[1 + LDM] = r.m11;
    }
  }
  lds_sync();
  nfR_out = nfR;
  return result;
}

// ILQR_TILES(v) ... ILQR_TILES_END(v): the statements between, for the control tiles v = 0 .. MT - 1 (unrolled).  At MT = 1 the front
// end emits them once, v the constant 0: no loop reaches the optimiser, not even one of a single trip, which LICM and SROA would see
// before unrolling it -- that moved the register allocation of every single-tile instantiation.  So MT = 1 compiles instruction for
// instruction as the step did before it had control tiles.
#define ILQR_TILES(v) { int v##_it = 0; _Pragma("unroll") do { const int v = (MT == 1) ? 0 : v##_it;
#define ILQR_TILES_END(v) } while (MT > 1 && ++v##_it < MT); }

// The LDS of the two-tile step (MT = 2), <= 40 KB so that four wavefronts -- one per SIMD -- fit a CU.  S has room for QuuF | Minv
// (32 x 33 each) but not for Quu beside them, so Quu waits in Kbuf behind the first reduction's partial sums, from the products to dV,
// and the stale-factor path writes K into QuuF's place, dead once the box-QP has returned.
template <int NT>  // NT = 16-row tiles covering n: 1 (n <= 16) or 2 (n <= 32)
struct Wave3WLds {
  static constexpr int N = 16 * NT, LD = N + 1;
  static constexpr int S_LEN = (LD * N > 2 * LDMW * WMW) ? LD * N : 2 * LDMW * WMW;
  static constexpr int RED = 4 * (N + WMW);  // the partial sums of Qx, Qu
  double S[S_LEN];                // QuuF (K on the stale-factor path) | Minv (m x m, ld LDMW) until the gains; then Vn (ld LD)
  double Kbuf[RED + LDMW * WMW];  // reduction scratch; Quu (ld LDMW) behind the first reduction's sums until dV
  double Tbuf[LDMW * WMW];        // Ri / the scattered Minv (m x m, ld LDMW); Qux (m x n) for the stale-factor path
  __device__ __forceinline__ double* K() { return S; }
  __device__ __forceinline__ double* Quu() { return Kbuf + RED; }
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

// n <= 16 NT, m <= 16 MT.  Arguments as k_backward_w2; LQF: const_rec holds TWO records (the constant blocks of the knots t < T,
// then knot T's) and v.D is not touched.
// REGV (ILQR_FLAG_REGULARIZE_VXX, opt-in): lambda regularises Vxx' ([Tassa 2012] eq. 10) instead of Quu -- QuuF = Quu + lambda fu'fu and the
// gains' Qux_reg = Qux + lambda fu'fx, two more transposed products per 16-column block on the operands the step holds anyway; the value
// update keeps Quu, Qux (as backward_thread.hpp does for the tiled kernels).  Instantiated without FULL / LQF.
// MT = 2 (16 < m <= 32, and ILQR_ROUTE_TWO_CONTROL_TILES): the control-indexed blocks -- fu, A2', Qux, K, T1', cxu -- in two 16-row tiles,
// cuu / Quu as 2 x 2 tiles, everything indexed by a control reduced over lanes 0..31; the LDS is Wave3WLds.  Instantiated without
// FULL / LQF / REGV.
// Wavefronts per SIMD.  n <= 16 (NT = 1): TWO since round 6 -- at three (168 registers) the kernel kept 308 bytes of scratch per lane and its
// step went through memory: the pendulum chain's pass (n = 16, m = 4, B = 4096) 7.4 -> 4.8 ms with 254 registers and no scratch (four: the
// compiler gives up on the bound).  n > 16 (NT = 2): two, 256 registers and 170-260 bytes of scratch; one wavefront per SIMD with the
// accumulation registers as spill space was measured too (ILQR_W3_NT2_WAVES=1: profiles/README.md, round 6).  MT = 2: one (its LDS).
#ifndef ILQR_W3_NT1_WAVES
#define ILQR_W3_NT1_WAVES 2
#endif
#ifndef ILQR_W3_NT2_WAVES
#define ILQR_W3_NT2_WAVES 2
#endif
template <int NT, bool FULL, bool LQF, bool REGV = false, int MT = 1, class S = double>
__global__ __launch_bounds__(64, MT == 2 ? 1 : NT == 2 ? ILQR_W3_NT2_WAVES : ILQR_W3_NT1_WAVES) void k_backward_w3(BatchViewT<S> v, int n, int m, const double* __restrict__ u_min,
                                                                    const double* __restrict__ u_max, SolverParams sp, int mode,
                                                                    const double* __restrict__ const_rec) {
  static_assert(MT == 1 || (MT == 2 && !FULL && !LQF && !REGV), "two control tiles: whole records, the bounds-checked step");
  static_assert(MT == 1 || std::is_same<S, double>::value, "two control tiles: fp64 only");
  // S = float (fp32 handles): knots, gains and records are stored as float -- widened where they are loaded (ldm and the vector loads
  // below), the gains rounded where they are stored; every operation between is the fp64 instantiation's.  The records the LQF route
  // takes from const_rec are double on both.  fp32 handles pass const_rec on the LQF route only.
  using RT = std::conditional_t<LQF, double, S>;  // what the record pointers point at
  using Lds = std::conditional_t<MT == 1, Wave2Lds<NT>, Wave3WLds<NT>>;
  __shared__ Lds L;
  constexpr int N = 16 * NT;
  constexpr int W = 16 * MT;   // controls the layout holds
  constexpr int LDW = W + 1;   // ... and the leading dimension of its m x m / m x n LDS matrices
  constexpr int LDX = Lds::LD;
  constexpr int RS = N + W;  // stride of one row group's partial sums in the reduction scratch
  static_assert(4 * RS <= sizeof(Lds::Kbuf) / sizeof(double) && 3 * 4 * N <= sizeof(Lds::Kbuf) / sizeof(double), "reduction scratch lives in Kbuf");
  static_assert(256 <= LDM * N, "the inverse's warm start lives in Tbuf");
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (LQF && b == 0 && lane == 0) *v.n_running = 0;  // (no sweep kernel on this route: k_accept of this iteration recounts)
  if (b >= v.B) return;
  if (mode == 1 && v.status[b] != 0) return;
  const int T = v.T;
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0, oFU = oFX + n * n, oCX = oFU + n * m, oCXX = oCX + n, oCXU = oCXX + n * n, oCU = oCXU + n * m,
            oCUU = oCU + m;
  const RT* __restrict__ Db;
  if constexpr (LQF) Db = const_rec; else Db = v.D + (size_t)b * (T + 1) * REC;
  const S* __restrict__ xsb = v.xs + (size_t)b * (T + 1) * n;
  const S* __restrict__ usb = v.us + (size_t)b * T * m;
  S* __restrict__ kb = v.kff + (size_t)b * T * m;
  S* __restrict__ Kb = v.Kfb + (size_t)b * T * m * n;
  double lambda = v.lambda[b], dlambda = v.dlambda[b];
  const int g = lane >> 4, p = lane & 15;
  {
    double* z = reinterpret_cast<double*>(&L);
    const int nz = (int)(sizeof(Lds) / sizeof(double));
    for (int e = lane; e < nz; e += 64) z[e] = 0.0;
  }
  lds_sync();
  double* const red = L.Kbuf;    // partial sums of the matrix-vector products, [row group][column]
  double* const Xw = L.Tbuf;    // the inverse's warm start, natural layout [r][lane]

  auto mfma = [](double a, double b2, double4_t c) __attribute__((always_inline)) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b2, c, 0, 0, 0);
  };
  const double4_t zero4 = {0.0, 0.0, 0.0, 0.0};
  // natural registers: X[ti][tj][r] = X(16 ti + 4 r + g, 16 tj + p); control-indexed blocks carry the control tile mt first
  unsigned lb_nn = (unsigned)(g + n * p);
  unsigned lb_tn = (unsigned)(p + n * g);
  unsigned lb_mm = (unsigned)(g + m * p);
  auto ldm = [](const RT* r, bool in, unsigned off) __attribute__((always_inline)) {
    if (FULL) return (double)r[off];
    const double val = r[in ? off : 0u];
    return in ? val : 0.0;
  };
  auto row_in = [&](int a0) __attribute__((always_inline)) { return FULL || a0 + g < n; };
  auto col_in = [&](int tj) __attribute__((always_inline)) { return FULL || 16 * tj + p < n; };
  auto mrow_in = [&](int mt, int rr) __attribute__((always_inline)) { return FULL || 16 * mt + 4 * rr + g < m; };
  const bool mcol0 = FULL || p < m;  // (formed once: what the single-tile step has always done)
  auto mcol_in = [&](int mt) __attribute__((always_inline)) { return mt == 0 ? mcol0 : FULL || 16 * mt + p < m; };

  // the four-way sum over the row groups of one column of the reduction scratch, group 0 first
  auto red4 = [&](int col) __attribute__((always_inline)) { return ((red[col] + red[RS + col]) + red[2 * RS + col]) + red[3 * RS + col]; };

  int diverge = 0;
  bool done = false;
  double dV0 = 0, dV1 = 0;
  NsState ns;
#ifdef ILQR_W2_TIMING
  W2Clock clk;
  clk.start();
#endif
  while (true) {
    double Vxx[NT][NT][4];
    {  // :353-354
      const RT* r = LQF ? Db + REC : Db + (size_t)T * REC;
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int a0 = 16 * ti + 4 * rr;
            Vxx[ti][tj][rr] = ldm(r, row_in(a0) && col_in(tj), lb_nn + (unsigned)(oCXX + a0 + n * 16 * tj));
          }
      if (LQF) {  // Vx = cx[T] = cxx[T] x_T
        for (int e = lane; e < n; e += 64) L.cx[e] = xsb[(size_t)T * n + e];
        lds_sync();
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          double part = 0;
#pragma unroll
          for (int ti = 0; ti < NT; ti++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) part = __builtin_fma(Vxx[ti][tj][rr], L.cx[16 * ti + 4 * rr + g], part);
          red[g * RS + 16 * tj + p] = part;
        }
        lds_sync();
        if (lane < N) L.Vx[lane] = (FULL || lane < n) ? red4(lane) : 0.0;
      } else {
        for (int e = lane; e < n; e += 64) L.Vx[e] = r[oCX + e];
      }
      if (lane < m) L.kprev[lane] = kb[(size_t)(T - 1) * m + lane];
    }
    dV0 = dV1 = 0;
    diverge = 0;
    ns.valid = false;
    lds_sync();
    for (int i = T - 1; i >= 0; i--) {
      ILQR_W2MARK(7)
      const RT* rk = LQF ? Db : Db + (size_t)i * REC;                   // this knot's record (cx, cu, and the matrices unless const_rec has them)
      const RT* rm;                                                     // ... its matrix blocks
      if constexpr (std::is_same<RT, double>::value) rm = (LQF || const_rec) ? const_rec : rk; else rm = rk;
      double fx[NT][NT][4], fu[NT][MT][4];
      double kx = 0, ku = 0;  // non-LQF: cx on lanes < n, cu on lanes N .. N + m - 1
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
            ILQR_TILES(mt) fu[ti][mt][rr] = ldm(rm, ain && mcol_in(mt), lb_nn + (unsigned)(oFU + a0 + n * 16 * mt)); ILQR_TILES_END(mt)
          }
        const double us_l = (lane < m) ? usb[(size_t)i * m + lane] : 0.0;
        if (LQF) {
          const double xk = (lane < n) ? xsb[(size_t)i * n + lane] : 0.0;
          if (lane < n) L.cx[lane] = xk;   // the knot, for cx = cxx x_t
          if (lane < m) L.tmp[lane] = us_l;  // ... and cu = cuu u_t
        } else {
          kx = (lane < n) ? rk[oCX + lane] : 0.0;
          ku = (lane >= N && lane - N < m) ? rk[oCU + lane - N] : 0.0;
        }
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
        ILQR_TILES(mt) pu[mt] = 0; ILQR_TILES_END(mt)
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
#pragma unroll
            for (int tj = 0; tj < NT; tj++) px[tj] = __builtin_fma(fx[ti][tj][rr], vxr[ti][rr], px[tj]);
            ILQR_TILES(mt) pu[mt] = __builtin_fma(fu[ti][mt][rr], vxr[ti][rr], pu[mt]); ILQR_TILES_END(mt)
          }
      }
      ILQR_W2MARK(0)
      // A1' = Vxx' fx (n x n), A2' = Vxx' fu (n x m)
      double4_t a1t[NT][NT], a2t[NT][MT];
#pragma unroll
      for (int ti = 0; ti < NT; ti++) {
        ILQR_TILES(mt) a2t[ti][mt] = zero4; ILQR_TILES_END(mt)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) a1t[ti][tj] = zero4;
      }
#pragma unroll
      for (int ks = 0; ks < 4 * NT; ks++) {
#pragma unroll
        for (int ti = 0; ti < NT; ti++) {
#pragma unroll
          for (int tj = 0; tj < NT; tj++) a1t[ti][tj] = mfma(Vxx[ks >> 2][ti][ks & 3], fx[ks >> 2][tj][ks & 3], a1t[ti][tj]);
          ILQR_TILES(mt) a2t[ti][mt] = mfma(Vxx[ks >> 2][ti][ks & 3], fu[ks >> 2][mt][ks & 3], a2t[ti][mt]); ILQR_TILES_END(mt)
        }
      }
      // :361 Qxx = cxx + A1 fx ; :362 Qux = cxu' + A2 fx ; :363/:367 Quu, QuuF = cuu (+ lambda I) + A2 fu
      ILQR_W2MARK(1)
      double Qxx[NT][NT][4], Qux[MT][NT][4], quu_nat[MT][MT][4];
      double Quxr[REGV ? NT : 1][4];  // REGV: Qux + lambda fu'fx, what the gains are solved from
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {  // one 16-column block of the outputs at a time (registers)
        __builtin_amdgcn_sched_barrier(0);
        double cxx[NT][4], cxu[MT][4], cuu[MT][MT][4];
        {
          asm volatile("" : "+v"(lb_nn), "+v"(lb_tn), "+v"(lb_mm));
#pragma unroll
          for (int ti = 0; ti < NT; ti++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
              const int a0 = 16 * ti + 4 * rr;
              cxx[ti][rr] = ldm(rm, row_in(a0) && col_in(tj), lb_nn + (unsigned)(oCXX + a0 + n * 16 * tj));
            }
          ILQR_TILES(mt)
#pragma unroll
            for (int rr = 0; rr < 4; rr++)  // Qux(a, c) starts from cxu(c, a): offset c + n a   (LQ: cxu = 0)
              cxu[mt][rr] = LQF ? 0.0 : ldm(rm, mrow_in(mt, rr) && col_in(tj), lb_tn + (unsigned)(oCXU + 16 * tj + n * 16 * mt + n * 4 * rr));
          ILQR_TILES_END(mt)
          if (tj == 0) {
            ILQR_TILES(mi)
              ILQR_TILES(mj)
#pragma unroll
                for (int rr = 0; rr < 4; rr++)
                  cuu[mi][mj][rr] = ldm(rm, mrow_in(mi, rr) && mcol_in(mj), lb_mm + (unsigned)(oCUU + 16 * mi + 4 * rr + m * 16 * mj));
              ILQR_TILES_END(mj)
            ILQR_TILES_END(mi)
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (LQF) {  // cx = cxx x_t, cu = cuu u_t: partial sums over this lane's rows, into the sums they are added to
#pragma unroll
          for (int ti = 0; ti < NT; ti++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) px[tj] = __builtin_fma(cxx[ti][rr], L.cx[16 * ti + 4 * rr + g], px[tj]);
          if (tj == 0) {
#pragma unroll
            for (int rr = 0; rr < 4; rr++) pu[0] = __builtin_fma(cuu[0][0][rr], L.tmp[4 * rr + g], pu[0]);
          }
        }
        double4_t qxx[NT], qux[MT], quu[MT][MT];
#pragma unroll
        for (int ti = 0; ti < NT; ti++) qxx[ti] = zero4;
        ILQR_TILES(mi)
          qux[mi] = zero4;
          ILQR_TILES(mj) quu[mi][mj] = zero4; ILQR_TILES_END(mj)
        ILQR_TILES_END(mi)
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ks++) {
#pragma unroll
          for (int ti = tj; ti < NT; ti++) qxx[ti] = mfma(a1t[ks >> 2][ti][ks & 3], fx[ks >> 2][tj][ks & 3], qxx[ti]);  // (tiles on and below the diagonal: see Vn)
          ILQR_TILES(mt) qux[mt] = mfma(a2t[ks >> 2][mt][ks & 3], fx[ks >> 2][tj][ks & 3], qux[mt]); ILQR_TILES_END(mt)
          if (tj == 0) {
            ILQR_TILES(mi)
              ILQR_TILES(mj) quu[mi][mj] = mfma(a2t[ks >> 2][mi][ks & 3], fu[ks >> 2][mj][ks & 3], quu[mi][mj]); ILQR_TILES_END(mj)
            ILQR_TILES_END(mi)
          }
        }
#pragma unroll
        for (int ti = tj; ti < NT; ti++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const double val = cxx[ti][rr] + qxx[ti][rr];
            Qxx[ti][tj][rr] = (FULL || (row_in(16 * ti + 4 * rr) && col_in(tj))) ? val : 0.0;
            asm volatile("" : "+v"(Qxx[ti][tj][rr]));  // (computed HERE: sunk below the box-QP, both addends stay live across it)
          }
        ILQR_TILES(mt)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const double val = LQF ? qux[mt][rr] : cxu[mt][rr] + qux[mt][rr];
            Qux[mt][tj][rr] = (FULL || (mrow_in(mt, rr) && col_in(tj))) ? val : 0.0;
            asm volatile("" : "+v"(Qux[mt][tj][rr]));
          }
        ILQR_TILES_END(mt)
        double4_t fufu = zero4;
        if constexpr (REGV) {  // fu'fx, fu'fu: rows and columns outside the model are zero in fu, fx already
          double4_t fufx = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) {
            fufx = mfma(fu[ks >> 2][0][ks & 3], fx[ks >> 2][tj][ks & 3], fufx);
            if (tj == 0) fufu = mfma(fu[ks >> 2][0][ks & 3], fu[ks >> 2][0][ks & 3], fufu);
          }
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Quxr[tj][rr] = Qux[0][tj][rr] + lambda * fufx[rr];
        }
        if (tj == 0) {
          ILQR_TILES(mi)
            ILQR_TILES(mj)
#pragma unroll
              for (int rr = 0; rr < 4; rr++) {
                const int a = 16 * mi + 4 * rr + g, c = 16 * mj + p;
                const bool in = FULL || (mrow_in(mi, rr) && mcol_in(mj));
                const double cu2 = in ? cuu[mi][mj][rr] : 0.0;
                quu_nat[mi][mj][rr] = in ? cu2 + quu[mi][mj][rr] : 0.0;
                L.Quu()[a + LDW * c] = quu_nat[mi][mj][rr];
                if constexpr (REGV)
                  L.QuuF()[a + LDW * c] = in ? quu_nat[mi][mj][rr] + lambda * fufu[rr] : 0.0;
                else
                  L.QuuF()[a + LDW * c] = in ? (cu2 + ((a == c) ? lambda : 0.0)) + quu[mi][mj][rr] : 0.0;
              }
            ILQR_TILES_END(mj)
          ILQR_TILES_END(mi)
        }
      }
      // Qx = cx + fx'Vx, Qu = cu + fu'Vx: the four row groups' partial sums through the scratch
#pragma unroll
      for (int tj = 0; tj < NT; tj++) red[g * RS + 16 * tj + p] = px[tj];
      ILQR_TILES(mt) red[g * RS + N + 16 * mt + p] = pu[mt]; ILQR_TILES_END(mt)
      lds_sync();
      if (lane < N) {
        const double s = red4(lane);
        L.Qx[lane] = (FULL || lane < n) ? (LQF ? s : kx + s) : 0.0;
      } else if (lane < N + W) {
        const double s = red4(lane);
        L.Qu[lane - N] = (lane - N < m) ? (LQF ? s : ku + s) : 0.0;
      }
      lds_sync();
      ILQR_W2MARK(2)
      double Xm[4];
      unsigned free_mask = 0;
      int nfR = 0, nfact = 0;
      bool slow = false;
      int result;
      if constexpr (MT == 2) {  // two control tiles: the literal QP, 32 lanes wide, in every step (the refinement's contraction bound is
        // for 16 x 16 blocks); K by the literal path's code below
        slow = true;
        nfact = -1;  // (no warm start is kept on this route)
        result = w_box_qp<Lds, W>(m, L, lane, nfR ILQR_W2CLOCK_PASS, nullptr, sp.fixes);
        free_mask = (unsigned)__ballot(lane < m && L.vfree[lane]);
      } else if (!FULL && m <= 2) {  // one or two controls: the scalar solvers (w3_box_qp_small); K by the literal path's code below
        slow = true;
        nfact = -1;  // (no warm start for the matrix-core refinement is kept on this route)
        result = w3_box_qp_small(m, L, lane, nfR, sp.fixes);
        free_mask = (unsigned)__ballot(lane < m && L.vfree[lane]);
      } else if ((result = w3_box_qp_fast(m, L, lane, Xw, ns, Xm, free_mask)) == kQpBail) {
        slow = true;
        ns.valid = false;
        ILQR_W3COUNT(1, 1)
        result = w_box_qp(m, L, lane, nfR ILQR_W2CLOCK_PASS, &nfact, sp.fixes);
        free_mask = (unsigned)__ballot(lane < m && L.vfree[lane]);
      } else {
        ILQR_W3COUNT(0, 1)
      }
      ILQR_W2MARK(3)
      if (result < 1) {  // :371
        diverge = i;
        break;
      }
      // :373-385  K rows of free dims, natural registers K[mt][tj][r] = K(16 mt + 4 r + g, 16 tj + p)
      double K[MT][NT][4];
      const int nf = __popc(free_mask);
      auto quxk = [&](int mt, int tj, int rr) -> double {  // what the gains are solved from
        if constexpr (REGV) return Quxr[tj][rr]; else return Qux[mt][tj][rr];
      };
      if (!slow) {
        // K = -(masked inverse) Qux: clamped rows of the inverse are zero, so those rows of K are, and its zero columns add
        // exact zeros to the k-ordered sums over the free dims.  (MT = 1: the refinement's inverse is one 16 x 16 tile.)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < WM / 4; ks++) acc = mfma(Xm[ks], quxk(0, tj, ks), acc);
#pragma unroll
          for (int rr = 0; rr < 4; rr++) K[0][tj][rr] = -acc[rr];
        }
      } else {
        const unsigned long long fm64 = free_mask;
        if (nf > 0 && nf == nfR) {
          double* MF = L.Qf();
          if (nf == m) {
            MF = L.Minv();
          } else {
            if (lane < m && L.vfree[lane]) L.idx[__popcll(fm64 & ((1ull << lane) - 1ull))] = lane;
            for (int e = lane; e < LDW * W; e += 64) MF[e] = 0.0;
            lds_sync();
            for (int e = lane; e < nf * nf; e += 64) {
              const int a = e % nf, b2 = e / nf;
              MF[L.idx[a] + LDW * L.idx[b2]] = L.Minv()[a + LDW * b2];
            }
            lds_sync();
          }
          // K = -MF Qux: MF symmetric, tile (mt, kt) as the A operand; zero rows / columns outside the free set add exact zeros
          ILQR_TILES(mt)
            double aM[MT][4];
            ILQR_TILES(kt) ld_operand<4>([&](int i2, int k) { return MF[(16 * mt + i2) + LDW * (16 * kt + k)]; }, lane, aM[kt]); ILQR_TILES_END(kt)
#pragma unroll
            for (int tj = 0; tj < NT; tj++) {
              double4_t acc = zero4;
              ILQR_TILES(kt)
#pragma unroll
                for (int ks = 0; ks < 4; ks++) acc = mfma(aM[kt][ks], quxk(kt, tj, ks), acc);
              ILQR_TILES_END(kt)
#pragma unroll
              for (int rr = 0; rr < 4; rr++) K[mt][tj][rr] = -acc[rr];
            }
          ILQR_TILES_END(mt)
        } else {  // nothing free, or a stale factor of another size (:80): through LDS, as k_backward_w does
          if (lane < m && L.vfree[lane]) L.idx[__popcll(fm64 & ((1ull << lane) - 1ull))] = lane;
          // (MT = 1: the columns < n, the rest of Kbuf being reduction sums that reach K's padding only; MT = 2: all of them, QuuF's place)
          for (int c = lane >> (3 + MT); c < (MT == 1 ? n : N); c += 64 / W) L.K()[(lane & (W - 1)) + LDW * c] = 0;
          ILQR_TILES(mt)
#pragma unroll
            for (int tj = 0; tj < NT; tj++)
#pragma unroll
              for (int rr = 0; rr < 4; rr++) L.Tbuf[(16 * mt + 4 * rr + g) + LDW * (16 * tj + p)] = quxk(mt, tj, rr);
          ILQR_TILES_END(mt)
          lds_sync();
          if (nf > 0) {
            const int nuse = (nf < nfR) ? nf : nfR;
            for (int e = lane; e < nuse * n; e += 64) {
              const int rr = e % nuse, c = e / nuse;
              double acc = 0;
              for (int l2 = 0; l2 < nuse; l2++) acc += -L.Minv()[rr + LDW * l2] * L.Tbuf[L.idx[l2] + LDW * c];
              L.K()[L.idx[rr] + LDW * c] = acc;
            }
          }
          lds_sync();
          ILQR_TILES(mt)
#pragma unroll
            for (int tj = 0; tj < NT; tj++)
#pragma unroll
              for (int rr = 0; rr < 4; rr++) K[mt][tj][rr] = L.K()[(16 * mt + 4 * rr + g) + LDW * (16 * tj + p)];
          ILQR_TILES_END(mt)
        }
        // re-seed the inverse's warm start from the literal factor, if that was a complete one for this free set:
        // X = R^-1 R^-T scattered to the free rows / columns, the identity elsewhere
        lds_sync();
        if (nf > 0 && nf == nfR && nfact == nfR) {
          const bool fp = (free_mask >> p) & 1u;
          const int rp = __popc(free_mask & ((1u << p) - 1u));
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int a = 4 * rr + g;
            const bool fa = (free_mask >> a) & 1u;
            const int ra = __popc(free_mask & ((1u << a) - 1u));
            const double mv = L.Minv()[((fa && fp) ? ra : 0) + LDM * ((fa && fp) ? rp : 0)];
            Xw[64 * rr + lane] = (fa && fp) ? mv : ((a == p) ? 1.0 : 0.0);
          }
          ns.mask = free_mask;
          ns.valid = true;
        }
        lds_sync();
      }
      ILQR_W2MARK(4)
      // :388-389
      {
        const double d0 = wave_sum_ctrl<W>(lane < m ? L.x[lane] * L.Qu[lane] : 0.0);
        double part = 0;
        if (lane < m) {
          const double rr = dot_padded<W>([&](int a) { return 0.5 * L.x[a]; }, [&](int a) { return L.Quu()[a + LDW * lane]; });
          part = rr * L.x[lane];
        }
        dV0 += d0;
        dV1 += wave_sum_ctrl<W>(part);
      }
      // T1' = Quu' K (m x n): Quu's natural registers are its A operand
      double4_t t1t[MT][NT];
      ILQR_TILES(mt)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          t1t[mt][tj] = zero4;
          ILQR_TILES(kt)
#pragma unroll
            for (int ks = 0; ks < 4; ks++) t1t[mt][tj] = mfma(quu_nat[kt][mt][ks], K[kt][tj][ks], t1t[mt][tj]);
          ILQR_TILES_END(kt)
        }
      ILQR_TILES_END(mt)
      // :391 Vx = ((Qx + T1 k) + K'Qu) + Qux'k: per-lane partial sums over the rows 16 mt + 4 r + g, three sums kept apart
      {
        double xq[MT][4], qq[MT][4];
        ILQR_TILES(mt)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            xq[mt][rr] = L.x[16 * mt + 4 * rr + g];
            qq[mt][rr] = L.Qu[16 * mt + 4 * rr + g];
          }
        ILQR_TILES_END(mt)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          double s1 = 0, s2 = 0, s3 = 0;
          ILQR_TILES(mt)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
              s1 = __builtin_fma(t1t[mt][tj][rr], xq[mt][rr], s1);
              s2 = __builtin_fma(K[mt][tj][rr], qq[mt][rr], s2);
              s3 = __builtin_fma(Qux[mt][tj][rr], xq[mt][rr], s3);
            }
          ILQR_TILES_END(mt)
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
          L.Vx[lane] = (FULL || lane < n) ? vx : 0.0;
        }
      }
      lds_sync();  // (Quu, x, Qu have been read: S may take Vn)
      ILQR_W2MARK(5)
      // :392 Vn = ((Qxx + T1 K) + K'Qux) + Qux'K ; :393 Vxx = (Vn + Vn')/2 through S.  Vn is symmetric up to rounding (Qxx = cxx + fx'Vxx fx,
      // K'Quu K, and K'Qux + Qux'K as a pair), so only its 16 x 16 tiles on and below the diagonal are formed: the tile above the
      // diagonal of the new Vxx is the transpose of the one below it (read back transposed from S), where the reference averages two
      // roundings of the same number -- 20 of a step's 188 MFMAs at n = 32.
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj <= ti; tj++) {
          double4_t p1 = zero4, p2 = zero4, p3 = zero4;
          ILQR_TILES(kt)
#pragma unroll
            for (int ks = 0; ks < 4; ks++) {
              p1 = mfma(t1t[kt][ti][ks], K[kt][tj][ks], p1);
              p2 = mfma(K[kt][ti][ks], Qux[kt][tj][ks], p2);
              p3 = mfma(Qux[kt][ti][ks], K[kt][tj][ks], p3);
            }
          ILQR_TILES_END(kt)
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
      ILQR_TILES(mt)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            if (FULL || (mrow_in(mt, rr) && col_in(tj))) Kb[(size_t)i * m * n + (16 * mt + 4 * rr + g) + m * (16 * tj + p)] = K[mt][tj][rr];
          }
      ILQR_TILES_END(mt)
      lds_sync();
      ILQR_W2MARK(6)
    }
    if (mode == 0) {
      done = (diverge == 0);
      break;
    }
    if (diverge != 0) {  // :142-148
      dlambda = raised_dlambda(dlambda, sp);
      lambda = raised_lambda(lambda, dlambda, sp);
      if (lambda > sp.lambda_max) break;
      continue;
    }
    done = true;
    break;
  }
#ifdef ILQR_W2_TIMING
  clk.flush();
#endif
  // :153 / :405-412 gradient norm: mean_t max_j |k_j| / (|u_j| + 1), ascending t -- the max over the layout's W control lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_waitcnt(0);
  double acc = 0;
  for (int t = 0; t < T; t++) {
    double val = -1.0;
    if (lane < m) val = fabs((double)kb[(size_t)t * m + lane]) / (fabs((double)usb[(size_t)t * m + lane]) + 1);
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) val = fmax(val, __shfl_xor(val, off, 64));
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
      if (!sp.fixed_work && gnorm < sp.tol_grad && lambda < kLambdaConverged) {
        v.status[b] = 1;
        v.iters[b] += 1;
      }
    }
  }
}

#undef ILQR_TILES
#undef ILQR_TILES_END

}  // namespace ilqr
