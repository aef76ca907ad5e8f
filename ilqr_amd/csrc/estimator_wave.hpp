// estimator_wave.hpp -- the Kalman filter of the stored linearisation and the covariance of the output-feedback loop on the
// trajectory-contiguous layout of the generic path (n <= 32, m <= 32, ny <= n; double or float storage), one WAVEFRONT per trajectory,
// every product on v_mfma_f64_16x16x4_f64.  The forward dual of k_lq_gain_w's Riccati sweep (lq_solve_wave.hpp), in two kernels on one
// stream:
//     k_est_filter_w   over (fx, H, P0, W, V): Pp[t], L[t], Pf[t] and N[t] = sym(L S L') per knot -- the filter, which does not read K
//     k_est_loop_w     over (fx, fu, K, cxx, cxu, cuu, Pf, N): Xh, Sigma = Xh + Pf, Su and the expected cost
// Pf and N travel from the first to the second through handle scratch (capi.hip: run_estimator).  Two kernels, not one: k_covariance_w<2, 2>
// already cannot keep a knot's operands in flight, and the fused recursion carries two more n x n matrices.
//
// The definition (include/ilqr_amd.h, ilqr_get_estimator):
//     Pp[0] = P0;  S = sym(H Pp H' + V) = R R';  L = Pp H' S^-1;  G = I - L H;  Pf = sym(G Pp G' + L V L');  N = sym(L S L')
//     Xh = N (t = 0) else sym(A Xh A' + N);  Sigma = Xh + Pf;  Z = Xh K', Su = sym(K Z);  A = fx + fu K;  Pp[t+1] = sym(fx Pf fx' + W)
//     J = 1/2 sum_t <cxx, Sigma> + <cuu, Su> + 2 <cxu, Z>
//
// Operands as in value_wave.hpp and covariance_wave.hpp: a matrix X lives in "natural" registers X[ti][tj][r] = X(16 ti + 4 r + g,
// 16 tj + p), g = lane >> 4, p = lane & 15, and  sum_ks mfma(X[ks], Y[ks]) = X'Y  for two natural matrices with equal row counts.  The
// loaders index a stored matrix either way, so no product needs an LDS transpose:
//     Pt = Pp' (n x n), Hn = H' (n x ny) natural:    PHt = Pp H' = mfma(Pt, Hn),       H Pp H' = mfma(Hn, PHt)
//     Hs = H (ny x n), Lt = L' (ny x n) natural:     Gt = G' = I - H'L' = I - mfma(Hs, Lt)
//                                                    Y = Pp G' = mfma(Pt, Gt),         G Pp G' = mfma(Gt, Y)
//     Vn = V' (ny x ny) natural:                     V L' = mfma(Vn, Lt),              L V L' = mfma(Lt, V L')
//     S symmetric natural:                           S L' = mfma(S, Lt),               L S L' = mfma(Lt, S L')
//     fxt = fx' natural:                             Pf fx' = mfma(Pf, fxt),           fx Pf fx' = mfma(fxt, Pf fx')
// Pp is carried transposed (Pt): from knot 1 on it is symmetric to the bit and the two are one; P0 is taken as given, so it is loaded
// transposed and the first products multiply by P0 itself.
//
// The factorisation keeps the fixed size Y = 16 YT, as k_lq_gain_w keeps 16 MT: every index >= ny is an identity row and column with a
// zero right-hand side, so the indices < ny meet the pivots of the ny x ny matrix in index order.  Cholesky in place in LDS: lane r owns
// row r; step j forms column j, lane j publishes the pivot and every lane reads it (the "pivot <= 0 or not finite" exit is
// wavefront-uniform).  Then one lane per right-hand side: S is symmetric, so L' = S^-1 (H Pp') and lane c < 16 NT solves for column c of
// PHt' by forward and back substitution, the column at rest in LDS.
//
// Sizes that are no multiple of 16 take bounds-predicated loads (a zero outside the model adds exact zeros to every sum).  What is
// computed at a knot does not depend on which outputs were asked for, only whether it is computed: a window is a slice of the full call.
// A trajectory whose factorisation fails gets quiet NaNs in every output over the whole window: the filter's from k_est_filter_w (which
// has written the knots before the failure: the same wavefront overwrites them, after a fence), the loop's from k_est_loop_w.
//
// Resources (hipcc's kernel-resource-usage remarks, gfx950): DESIGN.md 3.19.
#pragma once
#include "backward_wave.hpp"

namespace ilqr {

// Canonical double in device memory (include/ilqr_amd.h): H [B][ny * nx], P0, W [B][nx * nx] (null = zero), V [B][ny * ny]; the knots
// [t0, t0 + nk) of Pp, Pf, Sigma [B][nk][nx * nx], L [B][nk][nx * ny], Su [B][nk][nu * nu]; J [B]; info [B].  Any output may be null.
// The scratch pointers are the handle's (capi.hip, run_estimator carves them): the generic layout alone uses them.
struct EstArgs {
  int t0, nk, ny;
  const double* H;
  const double* P0;
  const double* W;
  const double* V;
  double* Pp;
  double* Pf;
  double* L;
  double* Sigma;
  double* Su;
  double* J;
  int* info;
  double* Pfs;  // [B][est_last_knot + 1][nx * nx]: Pf of every knot, for k_est_loop_w; null unless the loop runs
  double* Ns;   // the same for N
  int* fail;    // [B]: 0 or (knot of the failed pivot) + 1
};
// the closed-loop part is asked for
__host__ __device__ inline bool est_closed(const EstArgs& q) { return q.Sigma || q.Su || q.J; }
// the last knot anything needs
__host__ __device__ inline int est_last_knot(const EstArgs& q, int T) { return q.J ? T : q.t0 + q.nk - 1; }

template <int NT, int YT>
struct EstFilterLds {
  static constexpr int N = 16 * NT, Y = 16 * YT, LDX = N + 1, LDA = Y + 1, LDR = N + 1;
  double S[LDX * N];  // an unsymmetrised n x n (or ny x ny) result, for the transposed read of the symmetrisations
  double A[Y * LDA];  // S with the identity outside ny, then its factor R (lower)
  double R[Y * LDR];  // right-hand sides [row][column of PHt'], then the solutions L'
  double dinv[Y];     // 1 / R(j, j)
};

// Wavefronts per SIMD by the register count the compiler reports: two state tiles take one wavefront's 512 registers.
template <int NT, int YT>
constexpr int kEstFilterWaves = NT == 2 ? 1 : 2;

// n <= 16 NT, ny <= 16 YT <= 16 NT; whole records in v.D (materialise_records first).
template <int NT, int YT, class S>
__global__ __launch_bounds__(64, (kEstFilterWaves<NT, YT>)) void k_est_filter_w(BatchViewT<S> v, int n, int m, EstArgs q) {
  static_assert(YT <= NT, "ny <= nx");
  using Lds = EstFilterLds<NT, YT>;
  __shared__ Lds L;
  constexpr int Y = Lds::Y, LDX = Lds::LDX, LDA = Lds::LDA, LDR = Lds::LDR;
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= v.B) return;
  const int T = v.T, ny = q.ny;
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0;
  const S* __restrict__ Db = v.D + (size_t)b * (T + 1) * REC;
  const double* __restrict__ Hb = q.H + (size_t)b * ny * n;
  const double* __restrict__ Vb = q.V + (size_t)b * ny * ny;
  const double* __restrict__ Wb = q.W ? q.W + (size_t)b * n * n : nullptr;
  const int t0 = q.t0, nk = q.nk;
  const int last = est_last_knot(q, T);
  double* const ppo = q.Pp ? q.Pp + (size_t)b * nk * n * n : nullptr;
  double* const pfo = q.Pf ? q.Pf + (size_t)b * nk * n * n : nullptr;
  double* const lo = q.L ? q.L + (size_t)b * nk * n * ny : nullptr;
  double* const pfs = q.Pfs ? q.Pfs + (size_t)b * (last + 1) * n * n : nullptr;
  double* const nso = q.Ns ? q.Ns + (size_t)b * (last + 1) * n * n : nullptr;
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
  // element `off` of a stored matrix if `in`, else an exact zero (the address of an element that exists is loaded either way)
  auto ldm = [](const auto* r, bool in, int off) __attribute__((always_inline)) {
    const double val = (double)r[in ? off : 0];
    return in ? val : 0.0;
  };
  auto row_in = [&](int ti, int rr) __attribute__((always_inline)) { return 16 * ti + 4 * rr + g < n; };
  auto col_in = [&](int tj) __attribute__((always_inline)) { return 16 * tj + p < n; };
  auto yrow_in = [&](int yt, int rr) __attribute__((always_inline)) { return 16 * yt + 4 * rr + g < ny; };
  auto ycol_in = [&](int yt) __attribute__((always_inline)) { return 16 * yt + p < ny; };
  // X <- (X + X')/2 for an n x n natural X, the transpose read back from LDS; the result at the knot `slot` of up to two arrays, written
  // as element (c, a) -- the same bits -- so that consecutive lanes write consecutive addresses
  auto sym_out = [&](double (&X)[NT][NT][4], double* o1, double* o2) __attribute__((always_inline)) {
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) L.S[(16 * ti + 4 * rr + g) + LDX * (16 * tj + p)] = X[ti][tj][rr];
    lds_sync();
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int a = 16 * ti + 4 * rr + g, c = 16 * tj + p;
          const double val = 0.5 * (X[ti][tj][rr] + L.S[c + LDX * a]);
          X[ti][tj][rr] = val;
          if (a < n && c < n) {
            if (o1) o1[c + (size_t)n * a] = val;
            if (o2) o2[c + (size_t)n * a] = val;
          }
        }
    lds_sync();
  };

  // Pp[0] = P0 as given, held transposed (Pt(a, c) = P0(c, a)): mfma(Pt, .) multiplies by Pt' = P0
  double Pt[NT][NT][4];
  {
    const double* s0 = q.P0 ? q.P0 + (size_t)b * n * n : nullptr;
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++)
          Pt[ti][tj][rr] = s0 ? ldm(s0, row_in(ti, rr) && col_in(tj), (16 * tj + p) + n * (16 * ti + 4 * rr + g)) : 0.0;
    if (ppo && t0 == 0)
      for (int e = lane; e < n * n; e += 64) ppo[e] = s0 ? s0[e] : 0.0;
  }
  int failed = 0;
  for (int t = 0; t <= last; t++) {
    const bool in_window = t >= t0 && t < t0 + nk;
    // PHt = Pp H' (n x ny), then S = H Pp H' + V (ny x ny)
    double4_t PHt[NT][YT];
    double Sn[YT][YT][4];
    {
      double Hn[NT][YT][4];  // H' : Hn(c, j) = H(j, c)
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int yt = 0; yt < YT; yt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Hn[ti][yt][rr] = ldm(Hb, row_in(ti, rr) && ycol_in(yt), (16 * yt + p) + ny * (16 * ti + 4 * rr + g));
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int yt = 0; yt < YT; yt++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(Pt[ks >> 2][ti][ks & 3], Hn[ks >> 2][yt][ks & 3], acc);
          PHt[ti][yt] = acc;
        }
#pragma unroll
      for (int yi = 0; yi < YT; yi++)
#pragma unroll
        for (int yj = 0; yj < YT; yj++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(Hn[ks >> 2][yi][ks & 3], PHt[ks >> 2][yj][ks & 3], acc);
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int a = 16 * yi + 4 * rr + g, c = 16 * yj + p;
            const double sv = acc[rr] + ldm(Vb, yrow_in(yi, rr) && ycol_in(yj), a + ny * c);
            Sn[yi][yj][rr] = sv;
            L.S[a + LDX * c] = sv;
          }
        }
    }
    lds_sync();
    // S = (S + S')/2 natural (zero outside ny); into L.A with the identity outside ny; the right-hand sides PHt' into L.R
#pragma unroll
    for (int yi = 0; yi < YT; yi++)
#pragma unroll
      for (int yj = 0; yj < YT; yj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const int a = 16 * yi + 4 * rr + g, c = 16 * yj + p;
          const double sv = 0.5 * (Sn[yi][yj][rr] + L.S[c + LDX * a]);
          Sn[yi][yj][rr] = sv;
          L.A[a * LDA + c] = (a < ny && c < ny) ? sv : (a == c ? 1.0 : 0.0);
        }
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int yt = 0; yt < YT; yt++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) L.R[(16 * yt + p) * LDR + 16 * ti + 4 * rr + g] = PHt[ti][yt][rr];
    lds_sync();
    // Cholesky, lower, in index order, in place in L.A (as k_lq_gain_w): lane r owns row r; step j forms column j from the finished
    // columns k < j, lane j publishes the pivot, every lane reads it -- so the exit is wavefront-uniform -- and scales its element.
    for (int j = 0; j < ny; j++) {
      double s = 0.0;
      if (lane >= j && lane < Y) {
        s = L.A[lane * LDA + j];
#pragma unroll 8
        for (int k = 0; k < j; k++) s = __builtin_fma(-L.A[lane * LDA + k], L.A[j * LDA + k], s);
        if (lane == j) L.A[j * LDA + j] = s;
      }
      lds_sync();
      const double piv = L.A[j * LDA + j];
      if (!(piv > 0.0) || piv > 1.7976931348623157e308) {  // <= 0 or not finite: the same value on every lane
        failed = t + 1;
        break;
      }
      const double rinv = 1.0 / __builtin_sqrt(piv);
      if (lane >= j && lane < Y) L.A[lane * LDA + j] = s * rinv;
      if (lane == 0) L.dinv[j] = rinv;
      lds_sync();
    }
    if (failed) break;
    // R R' x = rhs, one lane per right-hand side (column c of PHt': row c of Pp H'), the column in place in L.R
    if (lane < 16 * NT) {
      for (int r = 0; r < ny; r++) {
        double s = L.R[r * LDR + lane];
#pragma unroll 8
        for (int k = 0; k < r; k++) s = __builtin_fma(-L.A[r * LDA + k], L.R[k * LDR + lane], s);
        L.R[r * LDR + lane] = s * L.dinv[r];
      }
      for (int r = ny - 1; r >= 0; r--) {
        double s = L.R[r * LDR + lane];
#pragma unroll 8
        for (int k = r + 1; k < ny; k++) s = __builtin_fma(-L.A[k * LDA + r], L.R[k * LDR + lane], s);
        L.R[r * LDR + lane] = s * L.dinv[r];
      }
    }
    lds_sync();
    // Lt = L' (ny x n) natural; L[t] out (n x ny, column-major: L(c, j) at c + n j)
    double Lt[YT][NT][4];
#pragma unroll
    for (int yt = 0; yt < YT; yt++)
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) Lt[yt][ti][rr] = L.R[(16 * yt + 4 * rr + g) * LDR + 16 * ti + p];
    if (lo && in_window) {
      double* o = lo + (size_t)(t - t0) * n * ny;
      for (int e = lane; e < n * ny; e += 64) {
        const int j = e / n, c = e - j * n;
        o[e] = L.R[j * LDR + c];
      }
    }
    lds_sync();  // (L.R has been read: the next knot may write it)
    // Gt = G' = I - H'L' (n x n)
    double Gt[NT][NT][4];
    {
      double Hs[YT][NT][4];  // H as stored: Hs(j, c) = H(j, c)
#pragma unroll
      for (int yt = 0; yt < YT; yt++)
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Hs[yt][ti][rr] = ldm(Hb, yrow_in(yt, rr) && col_in(ti), (16 * yt + 4 * rr + g) + ny * (16 * ti + p));
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * YT; ks++) acc = mfma(Hs[ks >> 2][ti][ks & 3], Lt[ks >> 2][tj][ks & 3], acc);
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int a = 16 * ti + 4 * rr + g, c = 16 * tj + p;
            Gt[ti][tj][rr] = ((a == c && a < n) ? 1.0 : 0.0) - acc[rr];
          }
        }
    }
    // Pf = sym(G Pp G' + L V L') (Joseph form): Y = Pp G', V L', then both products into one accumulator
    double Pf[NT][NT][4];
    {
      double4_t Yp[NT][NT], VLt[YT][NT];
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(Pt[ks >> 2][ti][ks & 3], Gt[ks >> 2][tj][ks & 3], acc);
          Yp[ti][tj] = acc;
        }
      {
        double Vn[YT][YT][4];  // V' : Vn(a, c) = V(c, a)
#pragma unroll
        for (int yi = 0; yi < YT; yi++)
#pragma unroll
          for (int yj = 0; yj < YT; yj++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) Vn[yi][yj][rr] = ldm(Vb, yrow_in(yi, rr) && ycol_in(yj), (16 * yj + p) + ny * (16 * yi + 4 * rr + g));
#pragma unroll
        for (int yi = 0; yi < YT; yi++)
#pragma unroll
          for (int tj = 0; tj < NT; tj++) {
            double4_t acc = zero4;
#pragma unroll
            for (int ks = 0; ks < 4 * YT; ks++) acc = mfma(Vn[ks >> 2][yi][ks & 3], Lt[ks >> 2][tj][ks & 3], acc);
            VLt[yi][tj] = acc;
          }
      }
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(Gt[ks >> 2][ti][ks & 3], Yp[ks >> 2][tj][ks & 3], acc);
#pragma unroll
          for (int ks = 0; ks < 4 * YT; ks++) acc = mfma(Lt[ks >> 2][ti][ks & 3], VLt[ks >> 2][tj][ks & 3], acc);
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Pf[ti][tj][rr] = acc[rr];
        }
    }
    sym_out(Pf, (pfo && in_window) ? pfo + (size_t)(t - t0) * n * n : nullptr, pfs ? pfs + (size_t)t * n * n : nullptr);
    // N = sym(L S L'), for the loop kernel alone
    if (nso) {
      double4_t SLt[YT][NT];
      double Nn[NT][NT][4];
#pragma unroll
      for (int yi = 0; yi < YT; yi++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * YT; ks++) acc = mfma(Sn[ks >> 2][yi][ks & 3], Lt[ks >> 2][tj][ks & 3], acc);
          SLt[yi][tj] = acc;
        }
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * YT; ks++) acc = mfma(Lt[ks >> 2][ti][ks & 3], SLt[ks >> 2][tj][ks & 3], acc);
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Nn[ti][tj][rr] = acc[rr];
        }
      sym_out(Nn, nso + (size_t)t * n * n, nullptr);
    }
    if (t == last) break;
    // Pp[t + 1] = sym(fx Pf fx' + W): fxt = fx' by transposed indexing, W as stored
    {
      const S* rk = Db + (size_t)t * REC;
      double fxt[NT][NT][4];
      double4_t Y2[NT][NT];
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++)
            fxt[ti][tj][rr] = ldm(rk, row_in(ti, rr) && col_in(tj), oFX + (16 * tj + p) + n * (16 * ti + 4 * rr + g));
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(Pf[ks >> 2][ti][ks & 3], fxt[ks >> 2][tj][ks & 3], acc);
          Y2[ti][tj] = acc;
        }
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(fxt[ks >> 2][ti][ks & 3], Y2[ks >> 2][tj][ks & 3], acc);
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const double wv = Wb ? ldm(Wb, row_in(ti, rr) && col_in(tj), (16 * ti + 4 * rr + g) + n * (16 * tj + p)) : 0.0;
            Pt[ti][tj][rr] = Wb ? acc[rr] + wv : acc[rr];
          }
        }
      const bool out = ppo && t + 1 >= t0 && t + 1 < t0 + nk;
      sym_out(Pt, out ? ppo + (size_t)(t + 1 - t0) * n * n : nullptr, nullptr);
    }
  }
  if (failed) {  // quiet NaNs over the whole window, the knots this wavefront has written included (the fence: after those stores)
    __threadfence();
    const double qnan = __builtin_nan("");
    if (ppo)
      for (int e = lane; e < nk * n * n; e += 64) ppo[e] = qnan;
    if (pfo)
      for (int e = lane; e < nk * n * n; e += 64) pfo[e] = qnan;
    if (lo)
      for (int e = lane; e < nk * n * ny; e += 64) lo[e] = qnan;
  }
  if (lane == 0) {
    q.fail[b] = failed;
    if (q.info) q.info[b] = failed;
  }
}

template <int NT, int MT>
struct EstLoopLds {
  static constexpr int D = 16 * (NT > MT ? NT : MT), LD = D + 1;
  double S[LD * D];  // A Xh A' + N, then K Z: for the transposed read of the symmetrisations
};

// Wavefronts per SIMD and where a knot's operands are loaded: as k_covariance_w (kCovWaves, kCovLoadAllFirst), for the same reasons.
// This recursion reads two more n x n matrices per knot (Pf, N) than k_covariance_w: with two state tiles every operand in flight at
// once would spill even at one wavefront's 512 registers, so those variants load each operand where it is used (several waits per knot).
template <int NT, int MT>
constexpr int kEstLoopWaves = (NT == 2 || MT == 2) ? 1 : 2;
template <int NT, int MT>
constexpr bool kEstLoadAllFirst = NT == 1;

// n <= 16 NT, m <= 16 MT; whole records in v.D, the stored gains in v.Kfb, Pf and N of the knots 0 .. est_last_knot in q.Pfs, q.Ns.
template <int NT, int MT, class S>
__global__ __launch_bounds__(64, (kEstLoopWaves<NT, MT>)) void k_est_loop_w(BatchViewT<S> v, int n, int m, EstArgs q) {
  using Lds = EstLoopLds<NT, MT>;
  __shared__ Lds L;
  constexpr int LDX = Lds::LD;
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= v.B) return;
  const int T = v.T;
  const int t0 = q.t0, nk = q.nk;
  double* const sgo = q.Sigma ? q.Sigma + (size_t)b * nk * n * n : nullptr;
  double* const suo = q.Su ? q.Su + (size_t)b * nk * m * m : nullptr;
  const bool wantJ = q.J != nullptr;
  if (q.fail[b]) {  // the filter failed: quiet NaNs in every output of the loop
    const double qnan = __builtin_nan("");
    if (sgo)
      for (int e = lane; e < nk * n * n; e += 64) sgo[e] = qnan;
    if (suo)
      for (int e = lane; e < nk * m * m; e += 64) suo[e] = qnan;
    if (wantJ && lane == 0) q.J[b] = qnan;
    return;
  }
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0, oFU = oFX + n * n, oCX = oFU + n * m, oCXX = oCX + n, oCXU = oCXX + n * n, oCU = oCXU + n * m, oCUU = oCU + m;
  const S* __restrict__ Db = v.D + (size_t)b * (T + 1) * REC;
  const S* __restrict__ Kb = v.Kfb + (size_t)b * T * m * n;
  const int last = est_last_knot(q, T);
  const double* __restrict__ Pfb = q.Pfs + (size_t)b * (last + 1) * n * n;
  const double* __restrict__ Nb = q.Ns + (size_t)b * (last + 1) * n * n;
  int g = lane >> 4, p = lane & 15;  // (not const: phase() below)
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

  // Xh = sym(N[0]) = N[0], symmetric to the bit at every knot: Xh and its transpose are one.  N and Pf are symmetric too and are read as
  // element (c, a): consecutive lanes, consecutive addresses.
  double Xh[NT][NT][4];
#pragma unroll
  for (int ti = 0; ti < NT; ti++)
#pragma unroll
    for (int tj = 0; tj < NT; tj++)
#pragma unroll
      for (int rr = 0; rr < 4; rr++) Xh[ti][tj][rr] = ldm(Nb, row_in(ti, rr) && col_in(tj), (16 * tj + p) + n * (16 * ti + 4 * rr + g));
  double jl = 0.0;  // this lane's share of 2 J
  for (int t = 0; t <= last; t++) {
    const S* rk = Db + (size_t)t * REC;
    const S* Ki = Kb + (size_t)(t < T ? t : 0) * m * n;
    const double* Pk = Pfb + (size_t)t * n * n;
    const double* Nk = Nb + (size_t)(t < last ? t + 1 : t) * n * n;  // N of the NEXT knot
    const bool in_window = t >= t0 && t < t0 + nk;
    const bool prop = t < last;                                // Xh[t + 1] is needed
    const bool ctrl = t < T && (wantJ || (suo && in_window));  // Z and Su are needed
    const bool sig = wantJ || (sgo && in_window);              // Sigma[t] is needed
    double Pf[NT][NT][4], cxxT[NT][NT][4], Nn[NT][NT][4];
    double Kt[NT][MT][4], cuu[MT][MT][4], cxu[NT][MT][4];
    double K[MT][NT][4], fut[MT][NT][4], fxt[NT][NT][4];
    // where the operands are loaded where they are used, the scheduler is kept from gathering the loads of a later phase above an
    // earlier one, and the lane's row and column pass through an empty asm so that the predicated offsets of every load -- invariant
    // over the knots, sixteen registers per operand -- are formed again where they are used rather than kept for the whole sweep
    // (together the two are what spills)
    auto phase = [&]() __attribute__((always_inline)) {
      if (!kEstLoadAllFirst<NT, MT>) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" : "+v"(g), "+v"(p));
      }
    };
    phase();
    auto load_Kt = [&]() __attribute__((always_inline)) {  // Kt = K' (n x m): Kt(c, j) = K(j, c)
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Kt[ti][mt][rr] = ldm(Ki, row_in(ti, rr) && mcol_in(mt), (16 * mt + p) + m * (16 * ti + 4 * rr + g));
    };
    auto load_Pf_cxxT = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int off = (16 * tj + p) + n * (16 * ti + 4 * rr + g);
            Pf[ti][tj][rr] = ldm(Pk, row_in(ti, rr) && col_in(tj), off);
            cxxT[ti][tj][rr] = wantJ ? ldm(rk, row_in(ti, rr) && col_in(tj), oCXX + off) : 0.0;
          }
    };
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
    auto load_N = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) Nn[ti][tj][rr] = ldm(Nk, row_in(ti, rr) && col_in(tj), (16 * tj + p) + n * (16 * ti + 4 * rr + g));
    };
    if (kEstLoadAllFirst<NT, MT>) {  // every load of the knot before its first product: the knot waits for memory once
      if (ctrl) load_Kt();
      if (sig) load_Pf_cxxT();
      if (wantJ && ctrl) {
        load_cuu();
        load_cxu();
      }
      if (prop) {
        load_K_fut();
        load_fxt();
        load_N();
      }
    }
    // Sigma = Xh + Pf, and its share of J
    if (sig) {
      if (!kEstLoadAllFirst<NT, MT>) load_Pf_cxxT();
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int tj = 0; tj < NT; tj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int a = 16 * ti + 4 * rr + g, c = 16 * tj + p;
            const double sg = Xh[ti][tj][rr] + Pf[ti][tj][rr];
            // written as element (c, a): the same bits, consecutive lanes, consecutive addresses
            if (sgo && in_window && a < n && c < n) sgo[(size_t)(t - t0) * n * n + c + (size_t)n * a] = sg;
            if (wantJ) jl = __builtin_fma(cxxT[ti][tj][rr], sg, jl);
          }
    }
    phase();
    if (ctrl) {
      if (!kEstLoadAllFirst<NT, MT>) load_Kt();
      // Z = Xh K' (n x m)
      double4_t Z[NT][MT];
#pragma unroll
      for (int ti = 0; ti < NT; ti++)
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
          double4_t acc = zero4;
#pragma unroll
          for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(Xh[ks >> 2][ti][ks & 3], Kt[ks >> 2][mt][ks & 3], acc);
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
      phase();
      if (wantJ && !kEstLoadAllFirst<NT, MT>) load_cuu();
#pragma unroll
      for (int mi = 0; mi < MT; mi++)
#pragma unroll
        for (int mj = 0; mj < MT; mj++)
#pragma unroll
          for (int rr = 0; rr < 4; rr++) {
            const int a = 16 * mi + 4 * rr + g, c = 16 * mj + p;
            const double su = 0.5 * (L.S[a + LDX * c] + L.S[c + LDX * a]);  // the same bits at (c, a)
            if (suo && in_window && a < m && c < m) suo[(size_t)(t - t0) * m * m + c + (size_t)m * a] = su;
            if (wantJ) jl = __builtin_fma(cuu[mi][mj][rr], su, jl);
          }
      if (wantJ) {
        phase();
        if (!kEstLoadAllFirst<NT, MT>) load_cxu();
#pragma unroll
        for (int ti = 0; ti < NT; ti++)
#pragma unroll
          for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) jl = __builtin_fma(2.0 * cxu[ti][mt][rr], Z[ti][mt][rr], jl);
      }
      lds_sync();  // (K Z has been read: S may take the next Xh)
    }
    if (!prop) break;
    phase();
    if (!kEstLoadAllFirst<NT, MT>) {
      load_K_fut();
      load_fxt();
    }
    // At = A' = fx' + K'fu' (n x n); Y = Xh At; Xh[t + 1] = sym(At'Y + N[t + 1]), the transpose read back from LDS
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
    double4_t Y[NT][NT];
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double4_t acc = zero4;
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(Xh[ks >> 2][ti][ks & 3], At[ks >> 2][tj][ks & 3], acc);
        Y[ti][tj] = acc;
      }
    phase();
    if (!kEstLoadAllFirst<NT, MT>) load_N();
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
        double4_t acc = zero4;
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ks++) acc = mfma(At[ks >> 2][ti][ks & 3], Y[ks >> 2][tj][ks & 3], acc);
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
          const double xv = acc[rr] + Nn[ti][tj][rr];
          Xh[ti][tj][rr] = xv;
          L.S[(16 * ti + 4 * rr + g) + LDX * (16 * tj + p)] = xv;
        }
      }
    lds_sync();
#pragma unroll
    for (int ti = 0; ti < NT; ti++)
#pragma unroll
      for (int tj = 0; tj < NT; tj++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++)
          Xh[ti][tj][rr] = 0.5 * (Xh[ti][tj][rr] + L.S[(16 * tj + p) + LDX * (16 * ti + 4 * rr + g)]);
    lds_sync();
  }
  if (wantJ) {
    const double j2 = wave_sum(jl);
    if (lane == 0) q.J[b] = 0.5 * j2;
  }
}

}  // namespace ilqr
