// clone.hpp -- multi-start groups on the device (ilqr_select_best, ilqr_clone_trajectories, ilqr_clone_best): the winner of
// each group of G consecutive trajectories (k_select_best), who takes whose state (k_select_clone: the one judge of a map, with the
// per-trajectory scalars), and the gather of the nominal (k_clone_nominal: x0, xs, us, k, K in the handle's own layout and storage type).
// A source is never a destination (k_select_clone's rule), so the gather runs in place: the reads and writes of one launch never meet.
// Index b is the caller's trajectory everywhere, as in reset.hpp.
#pragma once
#include "common.hpp"
#include "layout.hpp"
#include "reset.hpp"

namespace ilqr {

// values of ilqr_clone_why (include/ilqr_amd.h)
enum { CLONE_WAS_CLONED = 1, CLONE_REFUSED = 2 };

// src[b] = the member of b's group (G consecutive trajectories, B % G == 0) with the lowest FINITE cost; among equal costs the lowest index;
// a group without a finite cost maps every member to itself.  One wavefront per group, 256 threads: a lane scans the members lane, lane + 64,
// ... upward with a strict < (so it keeps the lowest index of its own), then a (cost, index) min-reduction across the lanes.
__global__ void __launch_bounds__(256) k_select_best(const double* __restrict__ cost, int B, int G, int* __restrict__ src) {
  constexpr int NONE = 0x7fffffff;
  const int group = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) / 64), lane = (int)(threadIdx.x % 64);
  if (group >= B / G) return;  // (uniform per wavefront: the shuffles below see all 64 lanes)
  const int base = group * G;
  double best = 0.0;
  int at = NONE;
  for (int i = lane; i < G; i += 64) {
    const double c = cost[base + i];
    if (finite_bits(c) && (at == NONE || c < best)) {
      best = c;
      at = i;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double oc = __shfl_xor(best, m, 64);
    const int oa = __shfl_xor(at, m, 64);
    if (oa != NONE && (at == NONE || oc < best || (oc == best && oa < at))) {
      best = oc;
      at = oa;
    }
  }
  for (int i = lane; i < G; i += 64) src[base + i] = base + (at == NONE ? i : at);
}

// One thread per slot of the padded batch decides who is cloned; padding lanes b >= B are never selected and never sources.  With s = src[b]:
//   s < 0 or s == b                                     b keeps its bits, flag 0
//   0 <= s < B, s != b, and src[s] == s or src[s] < 0   b is cloned from s: sel[b] = s, flag CLONE_WAS_CLONED
//   anything else (s >= B, a source that is itself asked to change)   refused: b keeps its bits, flag CLONE_REFUSED
// A cloned slot takes the source's per-trajectory scalars here (a source's are never written: it keeps itself); its flgChange is 1, not the
// source's -- the derivative records stay the slot's own, so the next sweep must not take them for the records of the copied nominal (it
// recomputes what the source's records hold: the same nominal through the same kernel).
template <class real>
__global__ void k_select_clone(BatchViewT<real> v, const int* __restrict__ src, int* __restrict__ sel, int* __restrict__ flags) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= v.Bp) return;
  int s = -1, why = 0;
  if (b < v.B) {
    const int m = src[b];
    if (m >= 0 && m != b) {
      why = CLONE_REFUSED;
      if (m < v.B) {
        const int ms = src[m];
        if (ms == m || ms < 0) {
          s = m;
          why = CLONE_WAS_CLONED;
        }
      }
    }
  }
  sel[b] = s;
  flags[b] = why;
  if (s < 0) return;
  v.cost[b] = v.cost[s];
  v.lambda[b] = v.lambda[s];
  v.dlambda[b] = v.dlambda[s];
  v.dV[b] = v.dV[s];
  v.dV[v.Bp + b] = v.dV[v.Bp + s];
  v.gnorm[b] = v.gnorm[s];
  v.status[b] = v.status[s];
  v.iters[b] = v.iters[s];
  v.flg_change[b] = 1;
  v.alpha_idx[b] = v.alpha_idx[s];
  v.diverge[b] = v.diverge[s];
  v.backpass_done[b] = v.backpass_done[s];
}

// The nominal of the cloned trajectories, k_reset_nominal's decomposition (reset.hpp): an array is segments of S knots of W contiguous
// elements -- a tile ([S][E][16]: element i belongs to lane i % 16) or a trajectory of the trajectory-contiguous layout.  Grid (segments,
// 5 arrays), 256 threads.  A workgroup reads the segment's 16 (or 1) selections first and leaves if none is set: a step in which nobody is
// cloned costs the launch.  Otherwise consecutive threads walk consecutive destination elements and store where the owning lane is
// selected; the load comes from the same (knot, element) of the source's segment and lane.  (Sharing a segment among several workgroups
// was measured and bought nothing: DESIGN.md 3.15.)  Nothing behind a segment's S W elements is touched (the
// kRolloutFetchSlack rows of the tiled arrays).  du (the controls' array only; may be null): canonical double [B][S][W / lanes], added in
// double to the source's element before the store rounds to the storage type; only the rows of cloned trajectories are read.
struct CloneArray {
  void* a;           // the array (float or double, as the handle stores it)
  int S, W;
  const double* du;  // null: a plain copy
};
struct CloneSet {
  CloneArray arr[5];  // x0, xs, us, k, K
  const int* sel;     // [nseg * lanes]: the source, or -1
  int nseg, lanes;    // lanes: trajectories interleaved in a segment, TW or 1
};
constexpr int kCloneR = 16;  // elements per thread and chunk: 16 loads in flight per thread (k_shift_horizon's kShiftR)
template <class real>
__global__ void __launch_bounds__(256) k_clone_nominal(CloneSet set) {
  const CloneArray A = set.arr[blockIdx.y];
  if (!A.a) return;
  const size_t n = (size_t)A.S * A.W;
  const int lanes = set.lanes;
  const int mine = (int)(threadIdx.x % (unsigned)lanes);  // (256 is a multiple of TW: a thread stays on one lane of its tile)
  for (int seg = blockIdx.x; seg < set.nseg; seg += gridDim.x) {
    int any = 0, from = -1;
    for (int l = 0; l < lanes; l++) {
      const int s = set.sel[(size_t)seg * lanes + l];
      any |= s >= 0;
      if (l == mine) from = s;
    }
    if (!any) continue;  // (uniform: the whole workgroup read the same selections)
    if (from < 0) continue;
    real* p = (real*)A.a + (size_t)seg * n;
    // element i of this lane in the source's segment: the same knot and element, the source's lane
    // (i - mine is a multiple of `lanes`, never negative)
    const real* q = (const real*)A.a + (size_t)(from / lanes) * n + (from % lanes);
    const double* d = A.du ? A.du + ((size_t)seg * lanes + mine) * (n / lanes) : nullptr;
    // chunks of kCloneR x 256 elements, all loads of a chunk before its stores: source and destination are the same array to the compiler,
    // which would otherwise keep one load in flight per thread
    for (size_t base = threadIdx.x; base < n; base += (size_t)kCloneR * 256) {
      real r[kCloneR];
      double e[kCloneR];
#pragma unroll
      for (int j = 0; j < kCloneR; j++) {
        const size_t i = base + (size_t)j * 256;
        r[j] = (i < n) ? q[i - mine] : real(0);
        e[j] = (d && i < n) ? d[i / lanes] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < kCloneR; j++) {
        const size_t i = base + (size_t)j * 256;
        if (i < n) p[i] = d ? (real)((double)r[j] + e[j]) : r[j];
      }
    }
  }
}

}  // namespace ilqr
