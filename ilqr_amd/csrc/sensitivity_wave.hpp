// sensitivity_wave.hpp -- the linearised closed loop of the stored policy as a linear operator on the caller's own vectors, on the
// trajectory-contiguous layout of the generic path (n <= 32, m <= 32; double or float storage): k_tangent_w carries n_dirs directions
// forward (a Jacobian-vector product), k_adjoint_w carries n_dirs cotangents backward (a vector-Jacobian product).  One WAVEFRONT per
// (trajectory, tile of 16 directions), every product on v_mfma_f64_16x16x4_f64: a knot's fx, fu, K are read once per 16 directions.
//
// The definition (include/ilqr_amd.h, ilqr_get_tangent / ilqr_get_adjoint):
//     tangent:   du[t] = K[t] dx[t] + dv[t],              dx[t+1] = fx[t] dx[t] + fu[t] du[t]
//     adjoint:   w[t]  = gu[t] + fu[t]'a[t+1],            a[t]    = gx[t] + fx[t]'a[t+1] + K[t]'w[t];     g_x0 = a[0], g_v[t] = w[t]
//
// Operands as in value_wave.hpp / covariance_wave.hpp: a matrix X lives in "natural" registers X[ti][r] = X(16 ti + 4 r + g, p),
// g = lane >> 4, p = lane & 15, and  sum_ks mfma(A[ks], X[ks]) = A'X  for two natural matrices with equal row counts, natural again.
// Here the columns p are the 16 DIRECTIONS of the tile: dx, du, a, w are (n or m) x 16 natural matrices, one double4 per 16-row tile.
//     tangent: Kt = K' (n x m), fxt = fx' (n x n), fut = fu' (m x n) by transposed indexing (as k_covariance_w loads them):
//              U = dv + K dx = dv + mfma(Kt, X),   Xn = fx X + fu U = mfma(fxt, X) + mfma(fut, U)
//     adjoint: fu (n x m), fx (n x n), K (m x n) as stored:
//              W = gu + fu'a = gu + mfma(fu, A),   An = gx + fx'a + K'w = gx + mfma(fx, A) + mfma(K, W)
// No LDS transpose for the algebra; dv / gu / gx enter as the accumulators' initial values.  Column p of an MFMA result depends on
// column p of its B operand and accumulator alone, and sizes / direction counts that are no multiple of 16 take bounds-predicated loads
// (an exact zero outside adds exact zeros): column s of every output depends on column s of the inputs only, bit for bit, wherever in
// a tile it sits.  What is computed at a knot does not depend on which outputs were asked for: a window is a slice of the full call.
//
// The caller's arrays: [..][n_dirs][len] (len = nx or nu), so a (trajectory, knot)'s tile of nd <= 16 directions is ONE CONTIGUOUS block of
// nd * len doubles, while the lanes of a natural register are len doubles apart.  Every such block moves through an LDS image
// [16 directions][LD = 16 max(NT, MT) + 2]: the global side is lane e <-> element e of the block (whole 512-byte wavefront accesses),
// the register side is img[p][16 ti + 4 r + g] (LD = 2 mod 32: the 32 lanes of a half hit 32 distinct 8-byte banks).  The input images
// are zeroed once and only ever written inside the block, so the natural read of a ragged tile finds exact zeros outside it.
// Every load of a knot -- the caller's tile first, then the records -- is issued before the knot's first product; the caller's tile has
// returned when the records still travel, so its trip through LDS costs no second wait.
//
// Resources (hipcc's kernel-resource-usage remarks, gfx950; LDS: SensLds): DESIGN.md 3.17.
#pragma once
#include "backward_wave.hpp"

namespace ilqr {

// Canonical double in device memory (include/ilqr_amd.h).  nd = n_dirs; nku = min(t0 + nk, T) - t0.
struct TangentArgs {
  int t0, nk, nd;
  const double* dx0;  // [B][nd][nx]       null = zero
  const double* dv;   // [B][T][nd][nu]    null = zero
  double* dxs;        // [B][nk][nd][nx]   either output may be null
  double* dus;        // [B][nku][nd][nu]
};
struct AdjointArgs {
  int t0, nk, nd;
  const double* gx;  // [B][nk][nd][nx]    null = zero
  const double* gu;  // [B][nku][nd][nu]   null = zero
  double* gx0;       // [B][nd][nx]        either output may be null
  double* gv;        // [B][T][nd][nu]     the knots after the window are written as zeros
};
// the last knot whose state the tangent needs: the window's last for dxs, the last knot with a control for dus
__host__ __device__ inline int tangent_last_state(const TangentArgs& q, int T) {
  const int nku = (q.t0 + q.nk < T ? q.t0 + q.nk : T) - q.t0;
  return q.dxs ? q.t0 + q.nk - 1 : q.t0 + nku - 1;
}

template <int NT, int MT>
struct SensLds {
  static constexpr int D = 16 * (NT > MT ? NT : MT), LD = D + 2, Q = D / 4;  // Q: elements of a block per lane
  double in[2][16 * LD];  // the caller's input tiles (state-sized, control-sized); zero outside the block
  double out[16 * LD];    // an output tile on its way out
};

// Wavefronts per SIMD: chosen by the register count the compiler reports.  Every load of a knot is in flight at once, each
// with an address of its own (the bounds predicate is part of the address): <1, 1> stays under the 128 registers of four wavefronts per
// SIMD, one two-tile dimension under the 256 of two, and <2, 2> (which would spill 57 registers at 256) gets one wavefront's 512.  No
// variant has scratch.
template <int NT, int MT>
constexpr int kSensWaves = (NT == 2 && MT == 2) ? 1 : (NT == 2 || MT == 2) ? 2 : 4;

// Where element e = lane + 64 q of a contiguous block [nd][len] sits in an LDS image [16][LD]: (direction, element) walked without a
// division per element.
struct BlockWalk {
  int s, i, ds, di, len;
  __device__ __forceinline__ BlockWalk(int lane, int len_) : len(len_) {
    s = lane / len;
    i = lane - s * len;
    ds = 64 / len;
    di = 64 - ds * len;
  }
  __device__ __forceinline__ void next() {
    s += ds;
    i += di;
    if (i >= len) {
      i -= len;
      s++;
    }
  }
};

// the wavefront's shared pieces: the block <-> LDS image <-> natural register moves
template <int NT, int MT>
struct SensTile {
  using Lds = SensLds<NT, MT>;
  static constexpr int LD = Lds::LD;
  // element e of the block if it exists, else nothing: the loads of a knot's tile, issued ahead of the records'
  template <int TILES>
  static __device__ __forceinline__ void fetch(const double* __restrict__ blk, int count, int lane, double (&r)[4 * TILES]) {
#pragma unroll
    for (int qq = 0; qq < 4 * TILES; qq++) {
      const int e = lane + 64 * qq;
      const double val = blk[e < count ? e : 0];
      r[qq] = e < count ? val : 0.0;
    }
  }
  // into the image (inside the block only), and out of it as natural registers X[ti][r] = img[p][16 ti + 4 r + g]
  template <int TILES>
  static __device__ __forceinline__ void to_natural(double* img, int len, int count, int lane, const double (&r)[4 * TILES], double4_t (&X)[TILES]) {
    BlockWalk w(lane, len);
#pragma unroll
    for (int qq = 0; qq < 4 * TILES; qq++) {
      if (lane + 64 * qq < count) img[w.s * LD + w.i] = r[qq];
      w.next();
    }
    lds_sync();
    const int g = lane >> 4, p = lane & 15;
#pragma unroll
    for (int ti = 0; ti < TILES; ti++)
#pragma unroll
      for (int rr = 0; rr < 4; rr++) X[ti][rr] = img[p * LD + 16 * ti + 4 * rr + g];
    lds_sync();
  }
  // natural registers into the caller's block: through the output image
  template <int TILES>
  static __device__ __forceinline__ void store(double* img, double* __restrict__ blk, int len, int count, int lane, const double4_t (&X)[TILES]) {
    const int g = lane >> 4, p = lane & 15;
#pragma unroll
    for (int ti = 0; ti < TILES; ti++)
#pragma unroll
      for (int rr = 0; rr < 4; rr++) img[p * LD + 16 * ti + 4 * rr + g] = X[ti][rr];
    lds_sync();
    BlockWalk w(lane, len);
#pragma unroll
    for (int qq = 0; qq < 4 * TILES; qq++) {
      if (lane + 64 * qq < count) blk[lane + 64 * qq] = img[w.s * LD + w.i];
      w.next();
    }
    lds_sync();
  }
};

// n <= 16 NT, m <= 16 MT; whole records in v.D (materialise_records first), the stored gains in v.Kfb.  Block = trajectory * tiles + tile:
// the tiles of one trajectory run side by side and share its records in L2.
template <int NT, int MT, class S>
__global__ __launch_bounds__(64, (kSensWaves<NT, MT>)) void k_tangent_w(BatchViewT<S> v, int n, int m, TangentArgs q) {
  using Lds = SensLds<NT, MT>;
  using Tile = SensTile<NT, MT>;
  __shared__ Lds L;
  const int lane = threadIdx.x;
  const int tiles = (q.nd + 15) >> 4;
  const int b = blockIdx.x / tiles, s0 = 16 * (blockIdx.x - b * tiles);
  if (b >= v.B) return;
  const int nd = q.nd - s0 < 16 ? q.nd - s0 : 16;  // directions of this tile
  const int T = v.T;
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0, oFU = oFX + n * n;
  const S* __restrict__ Db = v.D + (size_t)b * (T + 1) * REC;
  const S* __restrict__ Kb = v.Kfb + (size_t)b * T * m * n;
  const int t0 = q.t0, nk = q.nk;
  const int nku = (t0 + nk < T ? t0 + nk : T) - t0;
  const int g = lane >> 4, p = lane & 15;
  // the tile's block of knot slot `slot` in an array [B][slots][n_dirs][len]
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
  // element `off` of a record / gain block if `in`, else an exact zero (the address of an element that exists is loaded either way)
  auto ldm = [](const S* r, bool in, int off) __attribute__((always_inline)) {
    const double val = (double)r[in ? off : 0];
    return in ? val : 0.0;
  };
  auto row_in = [&](int ti, int rr) __attribute__((always_inline)) { return 16 * ti + 4 * rr + g < n; };
  auto col_in = [&](int tj) __attribute__((always_inline)) { return 16 * tj + p < n; };
  auto mrow_in = [&](int mt, int rr) __attribute__((always_inline)) { return 16 * mt + 4 * rr + g < m; };
  auto mcol_in = [&](int mt) __attribute__((always_inline)) { return 16 * mt + p < m; };

  // dx[0] = dx0
  double4_t X[NT];
  if (q.dx0) {
    double r0[4 * NT];
    Tile::template fetch<NT>(block_of(q.dx0, 1, 0, n), nd * n, lane, r0);
    Tile::template to_natural<NT>(L.in[0], n, nd * n, lane, r0, X);
  } else {
#pragma unroll
    for (int ti = 0; ti < NT; ti++) X[ti] = zero4;
  }
  const int last = tangent_last_state(q, T);
  for (int t = 0; t <= last; t++) {
    const bool prop = t < last;                          // dx[t + 1] is needed
    const bool ctrl = prop || (q.dus && t < t0 + nku);  // du[t] is needed
    // Every load of the knot is issued here, before its first product: dv's tile first, then Kt = K' (n x m): Kt(c, j) = K(j, c),
    // fx' (n x n) and fu' (m x n) by transposed indexing
    double rv[4 * MT];
    double Kt[NT][MT][4], fxt[NT][NT][4], fut[MT][NT][4];
    if (ctrl) {
      const S* rk = Db + (size_t)t * REC;
      const S* Ki = Kb + (size_t)t * m * n;
      if (q.dv) Tile::template fetch<MT>(block_of(q.dv, T, t, m), nd * m, lane, rv);
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
    if (q.dxs && t >= t0) Tile::template store<NT>(L.out, block_of(q.dxs, nk, t - t0, n), n, nd * n, lane, X);
    if (!ctrl) break;
    // U = dv + K X (m x 16)
    double4_t U[MT];
    if (q.dv) {
      Tile::template to_natural<MT>(L.in[1], m, nd * m, lane, rv, U);
    } else {
#pragma unroll
      for (int mt = 0; mt < MT; mt++) U[mt] = zero4;
    }
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int ks = 0; ks < 4 * NT; ks++) U[mt] = mfma(Kt[ks >> 2][mt][ks & 3], X[ks >> 2][ks & 3], U[mt]);
    if (q.dus && t >= t0 && t < t0 + nku) Tile::template store<MT>(L.out, block_of(q.dus, nku, t - t0, m), m, nd * m, lane, U);
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

template <int NT, int MT, class S>
__global__ __launch_bounds__(64, (kSensWaves<NT, MT>)) void k_adjoint_w(BatchViewT<S> v, int n, int m, AdjointArgs q) {
  using Lds = SensLds<NT, MT>;
  using Tile = SensTile<NT, MT>;
  __shared__ Lds L;
  const int lane = threadIdx.x;
  const int tiles = (q.nd + 15) >> 4;
  const int b = blockIdx.x / tiles, s0 = 16 * (blockIdx.x - b * tiles);
  if (b >= v.B) return;
  const int nd = q.nd - s0 < 16 ? q.nd - s0 : 16;
  const int T = v.T;
  const int REC = 2 * n * n + 2 * n * m + n + m + m * m;
  const int oFX = 0, oFU = oFX + n * n;
  const S* __restrict__ Db = v.D + (size_t)b * (T + 1) * REC;
  const S* __restrict__ Kb = v.Kfb + (size_t)b * T * m * n;
  const int t0 = q.t0, nk = q.nk;
  const int nku = (t0 + nk < T ? t0 + nk : T) - t0;
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
  auto ldm = [](const S* r, bool in, int off) __attribute__((always_inline)) {
    const double val = (double)r[in ? off : 0];
    return in ? val : 0.0;
  };
  auto row_in = [&](int ti, int rr) __attribute__((always_inline)) { return 16 * ti + 4 * rr + g < n; };
  auto col_in = [&](int tj) __attribute__((always_inline)) { return 16 * tj + p < n; };
  auto mrow_in = [&](int mt, int rr) __attribute__((always_inline)) { return 16 * mt + 4 * rr + g < m; };
  auto mcol_in = [&](int mt) __attribute__((always_inline)) { return 16 * mt + p < m; };

  const int top = t0 + nk - 1;  // the last knot with a cotangent: a[t] = 0 past it
  // g_v of the knots after the window: exact zeros, whatever the caller's buffer held
  if (q.gv)
    for (int t = top + 1; t < T; t++) {
      double* blk = block_of(q.gv, T, t, m);
      for (int e = lane; e < nd * m; e += 64) blk[e] = 0.0;
    }
  double4_t A[NT];
#pragma unroll
  for (int ti = 0; ti < NT; ti++) A[ti] = zero4;
  for (int t = top; t >= 0; t--) {
    const bool has_gx = q.gx && t >= t0, has_gu = q.gu && t >= t0 && t < t0 + nku;
    // Every load of the knot is issued here, before its first product: the cotangents' tiles first, then fu (n x m), fx (n x n), K (m x n)
    // natural, as stored
    double rx[4 * NT], ru[4 * MT];
    double fu[NT][MT][4], fx[NT][NT][4], K[MT][NT][4];
    if (has_gx) Tile::template fetch<NT>(block_of(q.gx, nk, t - t0, n), nd * n, lane, rx);
    if (has_gu) Tile::template fetch<MT>(block_of(q.gu, nku, t - t0, m), nd * m, lane, ru);
    if (t < T) {
      const S* rk = Db + (size_t)t * REC;
      const S* Ki = Kb + (size_t)t * m * n;
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
    if (has_gx) {
      Tile::template to_natural<NT>(L.in[0], n, nd * n, lane, rx, An);
    } else {
#pragma unroll
      for (int ti = 0; ti < NT; ti++) An[ti] = zero4;
    }
    if (t < T) {
      if (has_gu) {
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
      // An = gx + fx'A + K'W (n x 16)
#pragma unroll
      for (int tj = 0; tj < NT; tj++) {
#pragma unroll
        for (int ks = 0; ks < 4 * NT; ks++) An[tj] = mfma(fx[ks >> 2][tj][ks & 3], A[ks >> 2][ks & 3], An[tj]);
#pragma unroll
        for (int ks = 0; ks < 4 * MT; ks++) An[tj] = mfma(K[ks >> 2][tj][ks & 3], W[ks >> 2][ks & 3], An[tj]);
      }
      if (q.gv) Tile::template store<MT>(L.out, block_of(q.gv, T, t, m), m, nd * m, lane, W);
    }  // (knot T has no control: a[T] = gx[T])
#pragma unroll
    for (int ti = 0; ti < NT; ti++) A[ti] = An[ti];
  }
  if (q.gx0) Tile::template store<NT>(L.out, block_of(q.gx0, 1, 0, n), n, nd * n, lane, A);
}

}  // namespace ilqr
