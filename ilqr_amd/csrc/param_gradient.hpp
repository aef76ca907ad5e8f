// param_gradient.hpp -- the gradient of a caller's loss with respect to the per-trajectory model parameters (ilqr_get_param_gradient /
// ilqr_param_gradient_on_device; the definition: include/ilqr_amd.h).  Generic (trajectory-contiguous) layout, user twins
// with NTP / set_trajectory_params only; all arithmetic double, in the double twin, on every handle (float storage is widened).
//   k_pg_costate   one wavefront per trajectory, serial in t: lam[T] = cx[T], lam[t] = cx[t] + fx[t]' lam[t+1] from the records
//   k_pg_contract  one wavefront per (trajectory, chunk of kPgChunk knots, group of directions): the stencil of the definition, a lane per
//                  model evaluation, summed over the chunk's knots in ascending t into one partial per (b, chunk, s, j)
//   k_pg_reduce    one thread per (b, s, j): the chunks' partials in ascending order -- no atomics anywhere, so the same bits every call
// Lanes of k_pg_contract: eight per (direction, parameter j), an octet; its lanes q = 0..3 evaluate Psi at (M+,+) (M+,-) (M-,+) (M-,-),
// q = 4, 5 the Euler map of M+ and M- at the knot itself (q = 6, 7 repeat them and are not read): every lane runs the same cost() and
// dynamics() code on its own point with its own copy of the model, as k_rollout_g's lanes do.  Eight octets per wavefront: with NTP <= 4
// a wavefront takes 8 / NTP directions side by side, with NTP > 8 it makes ceil(NTP / 8) passes (pg_shape, route.hpp).
#pragma once
#include "generic.hpp"
#include "route.hpp"

namespace ilqr {

constexpr int kPgChunk = 16;  // knots per wavefront of k_pg_contract: B * ceil((T + 1) / 16) * direction groups wavefronts

struct PgArgs {
  int nd;             // directions per trajectory
  int nchunk;         // ceil((T + 1) / kPgChunk)
  double eps_p;       // h = eps_p * max(1, |p[b][j]|)
  const double* dxs;  // [B][T+1][nd][nx]   (any of the three may be null: zero)
  const double* dus;  // [B][T][nd][nu]
  const double* dlam; // [B][T+1][nd][nx]   (knot 0 is not read)
  double* lam;        // [B][T+1][nx]: the caller's, or scratch
  double* part;       // [B][nchunk][nd][NTP] scratch
  double* gp;         // [B][nd][NTP]
};

// lane l's copy of a double held by lane `src`
__device__ __forceinline__ double pg_from_lane(double v, int src) {
  return __hiloint2double(__shfl(__double2hiint(v), src), __shfl(__double2loint(v), src));
}

// Lane i < NX holds lam[i].  The serial chain per knot is NX multiply-adds: column i of fx[t-1] (column-major: NX consecutive elements)
// and cx[t-1] are fetched before knot t's chain starts, and lam[t+1][r] reaches every lane through v_readlane, not through memory.
template <class S, int NX, int NU>
__global__ __launch_bounds__(64) void k_pg_costate(BatchViewT<S> v, double* __restrict__ lam) {
  struct R {  // the record's offsets (rec_offsets, common.hpp) at the twin's sizes
    enum { FX = 0, CX = NX * NX + NX * NU, SIZE = 2 * NX * NX + 2 * NX * NU + NX + NU + NU * NU };
  };
  const int b = blockIdx.x, lane = threadIdx.x, T = v.T;
  const S* Db = v.D + (size_t)b * (T + 1) * R::SIZE;
  double* lb = lam + (size_t)b * (T + 1) * NX;
  const bool mine = lane < NX;
  const int col = mine ? lane : 0;
  double l = (double)Db[(size_t)T * R::SIZE + R::CX + col];
  if (mine) lb[(size_t)T * NX + lane] = l;
  S fxc[NX], cx;
  auto fetch = [&](int t) __attribute__((always_inline)) {
    const S* D = Db + (size_t)t * R::SIZE;
    cx = D[R::CX + col];
#pragma unroll
    for (int r = 0; r < NX; r++) fxc[r] = D[R::FX + NX * col + r];
  };
  if (T > 0) fetch(T - 1);
  for (int t = T - 1; t >= 0; t--) {
    double acc = (double)cx, f[NX];
#pragma unroll
    for (int r = 0; r < NX; r++) f[r] = (double)fxc[r];
    if (t > 0) fetch(t - 1);
#pragma unroll
    for (int r = 0; r < NX; r++)  // r ascending
      acc += f[r] * __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(l), r), __builtin_amdgcn_readlane(__double2loint(l), r));
    l = acc;
    if (mine) lb[(size_t)t * NX + lane] = l;
  }
}

// M: GenericModelOf<UserModelT<double>>; S: the handle's storage type.  Grid: B * nchunk * ceil(nd / pg_shape(NTP).dirs) wavefronts.
template <class M, class S>
__global__ __launch_bounds__(64) void k_pg_contract(BatchViewT<S> v, PerTrajectory<M> model, PgArgs a) {
  constexpr int NX = M::NX, NU = M::NU, NTP = M::NTP;
  constexpr ParamGradientShape kShape = pg_shape(NTP);
  constexpr int DIRS = kShape.dirs, PASSES = kShape.passes, PER = NTP < 8 ? NTP : 8;  // octets per direction in one pass
  const int T = v.T, lane = threadIdx.x, q = lane & 7, oct = lane >> 3;
  const int ngroup = (a.nd + DIRS - 1) / DIRS;
  const int b = blockIdx.x / (a.nchunk * ngroup), rest = blockIdx.x - b * (a.nchunk * ngroup), chunk = rest / ngroup, group = rest - chunk * ngroup;
  const int slot = oct / PER, s = group * DIRS + slot;
  const bool dir_ok = slot < DIRS && s < a.nd;
  const double sgn_p = (q == 0 || q == 1 || q == 4 || q == 6) ? 1.0 : -1.0;  // M+ or M-
  const double sigma = (q == 0 || q == 2) ? 1.0 : (q == 1 || q == 3) ? -1.0 : 0.0;
  const int t_lo = chunk * kPgChunk, t_hi = min(t_lo + kPgChunk, T + 1);

  // the knot as every lane reads it: x, u, lam[t+1] once per wavefront; d = (dxs, dus)[t] and dlam[t+1] once per direction
  __shared__ double sx[NX], su[NU], sl[NX], sdx[DIRS][NX], sdu[DIRS][NU], sdl[DIRS][NX];

  // row b through the constant path (k_derivatives_g<.., PT>); an fp32 handle's parameters are the float-rounded values
  cmem_d* row = (cmem_d*)model.traj_params + (size_t)b * NTP;
  double base[NTP];
#pragma unroll
  for (int i = 0; i < NTP; i++) {
    base[i] = row[i];
    if constexpr (!std::is_same<S, double>::value) base[i] = (double)(float)base[i];
  }

  for (int pass = 0; pass < PASSES; pass++) {
    const int j = pass * 8 + oct % PER;
    const bool mine = dir_ok && j < NTP;
    double pj = base[0];
#pragma unroll
    for (int i = 1; i < NTP; i++) pj = (i == j) ? base[i] : pj;
    const double h = a.eps_p * fmax(1.0, fabs(pj));
    M m = static_cast<const M&>(model);
    {
      double p[NTP];
#pragma unroll
      for (int i = 0; i < NTP; i++) p[i] = (i == j) ? base[i] + sgn_p * h : base[i];
      m.set_trajectory_params(p);
    }
    double total = 0.0;
    // this lane's share of a knot's inputs, fetched one knot ahead: the loads of knot t + 1 are in flight while knot t is evaluated
    constexpr int KX = (DIRS * NX + 63) / 64, KU = (DIRS * NU + 63) / 64;
    double rx = 0, rl = 0, ru = 0, rdx[KX], rdl[KX], rdu[KU];
    auto fetch = [&](int t) __attribute__((always_inline)) {
      const bool last = t == T;
      if (lane < NX) {
        rx = (double)v.xs[((size_t)b * (T + 1) + t) * NX + lane];
        rl = last ? 0.0 : a.lam[((size_t)b * (T + 1) + t + 1) * NX + lane];
      }
      if (lane < NU) ru = last ? 0.0 : (double)v.us[((size_t)b * T + t) * NU + lane];
#pragma unroll
      for (int k = 0; k < KX; k++) {
        const int e = lane + 64 * k, d = e / NX, i = e - d * NX, sd = group * DIRS + d;
        const bool ok = e < DIRS * NX && sd < a.nd;
        rdx[k] = (ok && a.dxs) ? a.dxs[(((size_t)b * (T + 1) + t) * a.nd + sd) * NX + i] : 0.0;
        rdl[k] = (ok && a.dlam && !last) ? a.dlam[(((size_t)b * (T + 1) + t + 1) * a.nd + sd) * NX + i] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < KU; k++) {
        const int e = lane + 64 * k, d = e / NU, i = e - d * NU, sd = group * DIRS + d;
        rdu[k] = (e < DIRS * NU && sd < a.nd && a.dus && !last) ? a.dus[(((size_t)b * T + t) * a.nd + sd) * NU + i] : 0.0;
      }
    };
    fetch(t_lo);
    for (int t = t_lo; t < t_hi; t++) {
      const bool last = t == T;
      __syncthreads();  // (the previous knot's readers are done)
      if (lane < NX) sx[lane] = rx, sl[lane] = rl;
      if (lane < NU) su[lane] = ru;
#pragma unroll
      for (int k = 0; k < KX; k++)
        if (lane + 64 * k < DIRS * NX) (&sdx[0][0])[lane + 64 * k] = rdx[k], (&sdl[0][0])[lane + 64 * k] = rdl[k];
#pragma unroll
      for (int k = 0; k < KU; k++)
        if (lane + 64 * k < DIRS * NU) (&sdu[0][0])[lane + 64 * k] = rdu[k];
      __syncthreads();
      if (t + 1 < t_hi) fetch(t + 1);
      const int dsl = dir_ok ? slot : 0;
      double nn = 0.0;
#pragma unroll
      for (int i = 0; i < NX; i++) nn += sdx[dsl][i] * sdx[dsl][i];
#pragma unroll
      for (int i = 0; i < NU; i++) nn += sdu[dsl][i] * sdu[dsl][i];
      const double n = sqrt(nn);
      const double step = (n > 0.0) ? sigma * (kEps / n) : 0.0;
      double px[NX], pu[NU];
      {
#pragma clang fp contract(off)  // the point is z + (eps / n) d rounded product by product, as the definition reads
#pragma unroll
        for (int i = 0; i < NX; i++) px[i] = sx[i] + step * sdx[dsl][i];
#pragma unroll
        for (int i = 0; i < NU; i++) pu[i] = su[i] + step * sdu[dsl][i];
      }
      double val;
      if (!last) {
        double F[NX];
        const double c = m.cost(px, pu);
        integrate_dynamics(m, px, pu, v.dt, F);
        // q < 4: Psi = cost + lam[t+1] . F;   q >= 4: dlam[t+1] . (F_{M+}(z) - F_{M-}(z)), the difference taken component by component
        const bool psi = q < 4;
        val = psi ? c : 0.0;
#pragma unroll
        for (int r = 0; r < NX; r++) {
          const double other = pg_from_lane(F[r], lane ^ 1);
          const double g = psi ? F[r] : F[r] - other;
          val += (psi ? sl[r] : sdl[dsl][r]) * g;
        }
      } else {
        val = (q < 4) ? m.final_cost(px) : 0.0;  // A_T: the same stencil of final_cost along dxs[T]; no B_T
      }
      const int o = lane & ~7;
      const double v0 = pg_from_lane(val, o), v1 = pg_from_lane(val, o + 1), v2 = pg_from_lane(val, o + 2), v3 = pg_from_lane(val, o + 3),
                   v4 = pg_from_lane(val, o + 4);
      const double At = (n > 0.0) ? (v0 - v1 - v2 + v3) * n / (4 * kEps * h) : 0.0;
      const double Bt = v4 / (2 * h);
      total += At + Bt;
    }
    if (mine && q == 0) a.part[(((size_t)b * a.nchunk + chunk) * a.nd + s) * NTP + j] = total;
  }
}

// gp[b][s][j] = the partials of (b, s, j), chunk 0 first.  (A template, as the other two: a build whose twin has no NTP holds none of them.)
template <int NTP>
__global__ __launch_bounds__(256) void k_pg_reduce(int B, PgArgs a) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, per = (size_t)a.nd * NTP;
  if (e >= (size_t)B * per) return;
  const size_t b = e / per, sj = e - b * per;
  double total = 0.0;
  for (int c = 0; c < a.nchunk; c++) total += a.part[(b * a.nchunk + c) * per + sj];
  a.gp[e] = total;
}

}  // namespace ilqr
