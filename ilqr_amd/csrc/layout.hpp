// layout.hpp -- canonical [B][S][E] <-> a handle's layout (index maps, k_to_canonical / k_from_canonical), slot permutation (compaction),
// per-trajectory state reset (init_traj, src/ilqr_core.cpp:11-56) and the receding-horizon shift.  Lane mapping everywhere: consecutive lanes = consecutive trajectories of
// a tile, so each vector load / store touches whole 128-byte lines of the tiled layout (common.hpp).
#pragma once
#include <type_traits>

#include "boxqp.hpp"
#include "common.hpp"
#include "models.hpp"

namespace ilqr {

// ------------------------------------------------------------------------------------------
// layout conversion
// ------------------------------------------------------------------------------------------
// An array crosses the C ABI as canonical double [B][n][E].  A handle stores it tiled or trajectory-contiguous, as double or float
// (common.hpp); an index map says where element (b, s, e) of the canonical array lives in the handle's array.  The canonical array may
// be a window of the handle's S knots -- its knot s is the handle's knot t0 + s -- and, of the records, one block of each knot.
// LANES: trajectories interleaved in the innermost dimension of the device layout, the order k_from_canonical walks it in.
struct TiledMap {  // [tile][S][E][16]
  static constexpr int LANES = TW;
  int S, E, t0;
  __host__ __device__ size_t operator()(int b, int s, int e) const { return tidx(b / TW, t0 + s, e, b % TW, S, E); }
};
struct TiledRecMap {  // elements [off, off + E) of the pair-interleaved records [tile][S][REC/2][16][2]
  static constexpr int LANES = TW;
  int S, REC, off, t0;
  __host__ __device__ size_t operator()(int b, int s, int e) const { return didx(b / TW, t0 + s, off + e, b % TW, S, REC); }
};
struct AosMap {  // elements [off, off + E) of [b][S][stride]: a plain array (stride = E, off = 0) or a block of the records (stride = REC)
  static constexpr int LANES = 1;
  int S, stride, off, t0;
  __host__ __device__ size_t operator()(int b, int s, int e) const { return ((size_t)b * S + t0 + s) * stride + off + e; }
};
// elements of a handle's array of S knots of E elements per trajectory: what every index map above stays inside
__host__ __device__ inline size_t layout_elems(bool aos, int B, int ntiles, size_t S, size_t E) {
  return aos ? (size_t)B * S * E : (size_t)ntiles * S * E * TW;
}

// handle's array -> canonical dst[b][s][e], one thread per canonical element (the stores are coalesced; a tiled source is read
// line-strided, but this direction only serves getters)
template <class real, class Map>
__global__ void k_to_canonical(const real* __restrict__ src, double* __restrict__ dst, Map map, int B, int n, int E) {
  const size_t total = (size_t)B * n * E;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int e = (int)(i % E);
    size_t r = i / E;
    const int s = (int)(r % n);
    const int b = (int)(r / n);
    dst[i] = (double)src[map(b, s, e)];
  }
}
// canonical src[b][s][e] -> handle's array, one thread per element of the handle's array in its own order [group][s][e][lane] (the
// stores are coalesced); groups: the handle's tiles, or its trajectories.  The padding lanes b >= B are written as zero.
template <class real, class Map>
__global__ void k_from_canonical(const double* __restrict__ src, real* __restrict__ dst, Map map, int B, int groups, int n, int E) {
  constexpr int L = Map::LANES;
  const size_t total = (size_t)groups * n * E * L;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(i % L);
    size_t r = i / L;
    const int e = (int)(r % E);
    r /= E;
    const int s = (int)(r % n);
    const int b = (int)(r / n) * L + l;
    dst[map(b, s, e)] = (b < B) ? (real)src[((size_t)b * n + s) * E + e] : real(0);
  }
}

// dst slot j <- src slot perm[j], for every slot of the padded batch (compaction of running trajectories between chunks
// of a full solve, capi.hip): tiled arrays [tile][S][E][16] and per-trajectory scalars
template <class real>
__global__ void k_permute_tiled(const real* __restrict__ src, real* __restrict__ dst, const int* __restrict__ perm, int ntiles, int S, int E) {
  const size_t n = (size_t)ntiles * S * E * TW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int l = (int)(i % TW);
    size_t r = i / TW;
    const int e = (int)(r % E);
    r /= E;
    const int s = (int)(r % S);
    const int tile = (int)(r / S);
    const int p = perm[tile * TW + l];
    dst[i] = src[tidx(p / TW, s, e, p % TW, S, E)];
  }
}
template <class T>
__global__ void k_permute_scalar(const T* __restrict__ src, T* __restrict__ dst, const int* __restrict__ perm, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) dst[j] = src[perm[j]];
}

// ------------------------------------------------------------------------------------------
// per-trajectory state reset (init_traj, ilqr_core.cpp:11-56; statics of ilqr.h:17-18)
// ------------------------------------------------------------------------------------------
template <class real>
__device__ inline void reset_run_state(const BatchViewT<real>& v, int b) {  // everything k_reset_state resets but lambda / dlambda
  v.dV[b] = 0;
  v.dV[v.Bp + b] = 0;
  v.gnorm[b] = 0;
  v.status[b] = (b < v.B) ? 0 : 4;  // padding lanes never run
  v.iters[b] = 0;
  v.flg_change[b] = 1;
  v.alpha_idx[b] = -1;
  v.diverge[b] = 0;
  v.backpass_done[b] = 0;
}
template <class real>
__global__ void k_reset_state(BatchViewT<real> v, double lambda0, double dlambda0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= v.Bp) return;
  v.lambda[b] = lambda0;
  v.dlambda[b] = dlambda0;
  reset_run_state(v, b);
}
// a new outer loop on the stored solution (warm start, ilqr_core.cpp:65-76; ilqr_mpc_step): status / iteration count / flgChange restart,
// lambda and dlambda persist (the reference's file statics) -- on the device, so that an MPC step never waits for the stream
template <class real>
__global__ void k_warm_reset(BatchViewT<real> v) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= v.Bp) return;
  reset_run_state(v, b);
}

// ------------------------------------------------------------------------------------------
// receding horizon (ilqr_shift_horizon, ilqr_mpc_step)
// ------------------------------------------------------------------------------------------
// Both device layouts keep a trajectory array as segments of S knots of W contiguous elements: a tile of the tiled layout
// ([tile][S][E][16]: W = 16 E) or a trajectory of the trajectory-contiguous one ([b][S][E]: W = E).  Shifting by s knots is then, per
// segment, a forward move of s W elements -- a[i] = a[i + s W] for i < (S - s) W -- and a tail of s knots: the last knot repeated (hold)
// or zeros.  One workgroup per segment and array walks the segment upward in chunks of kShiftR x 256 elements, consecutive threads on
// consecutive elements: every chunk loads all its sources before any of its stores (a source of the chunk may be a destination of
// the same chunk), and a chunk never reads what an earlier one wrote (sources lie s W elements above the destinations).  In place, nothing
// allocated, and nothing behind a segment's S W elements touched (the kRolloutFetchSlack rows of the tiled arrays).
enum { SHIFT_TAIL_HOLD = 0, SHIFT_TAIL_ZERO = 1 };
struct ShiftArray {
  void* a;    // the array (float or double, as the handle stores it)
  int S, W;   // knots per segment, elements per knot of a segment
  int tail;   // SHIFT_TAIL_*
};
struct ShiftSet {
  ShiftArray arr[4];  // xs, us, k, K
  int nseg, shift;
};
constexpr int kShiftR = 16;  // elements per thread and chunk: 16 loads in flight per thread
// p[i] = src(i) for i in [lo, hi), all sources of a chunk read before its first store (the barrier also orders whatever the workgroup
// did before: chunks of the previous range)
template <class real, class Src>
__device__ inline void shift_range(real* p, size_t lo, size_t hi, Src src) {
  const size_t step = (size_t)kShiftR * blockDim.x;
  for (size_t base = lo; base < hi; base += step) {
    real r[kShiftR];
#pragma unroll
    for (int j = 0; j < kShiftR; j++) {
      const size_t i = base + (size_t)j * blockDim.x + threadIdx.x;
      r[j] = (i < hi) ? src(i) : real(0);
    }
    __builtin_amdgcn_s_waitcnt(0);  // this wavefront's loads have returned ...
    __syncthreads();                // ... and every other wavefront's too: now the chunk's stores may overwrite its sources
#pragma unroll
    for (int j = 0; j < kShiftR; j++) {
      const size_t i = base + (size_t)j * blockDim.x + threadIdx.x;
      if (i < hi) p[i] = r[j];
    }
  }
}
// grid (segments, 4 arrays), 256 threads; shift >= 1 (0 is no launch)
template <class real>
__global__ void __launch_bounds__(256) k_shift_horizon(ShiftSet set) {
  const ShiftArray A = set.arr[blockIdx.y];
  if (!A.a) return;
  const size_t W = (size_t)A.W, n = (size_t)A.S * W, keep = (size_t)(A.S - set.shift) * W, off = (size_t)set.shift * W;
  const size_t last = n - W;  // the last knot: only the tail writes it (keep <= last), and a held tail writes it with its own values
  for (int seg = blockIdx.x; seg < set.nseg; seg += gridDim.x) {
    real* p = (real*)A.a + (size_t)seg * n;
    shift_range(p, 0, keep, [&](size_t i) { return p[i + off]; });
    if (A.tail == SHIFT_TAIL_HOLD)
      shift_range(p, keep, n, [&](size_t i) { return p[last + (i - keep) % W]; });
    else
      shift_range(p, keep, n, [&](size_t) { return real(0); });
  }
}

}  // namespace ilqr
