// reset.hpp -- single trajectories start over on the device (ilqr_reset_trajectories, ilqr_mpc_step_reset): who is reset
// (k_select_reset: a caller's mask, a non-finite cost, a lambda_max exit), and the nominal of those who are (k_reset_nominal).  A reset only
// stores: no old value of a selected trajectory is read, so a NaN cannot travel through a 0 * x; a trajectory that is not selected keeps
// its bits.  Index b is the caller's trajectory everywhere (the slot: no call between two entry points leaves trajectories permuted).
#pragma once
#include "common.hpp"
#include "layout.hpp"

namespace ilqr {

// bits of ilqr_reset_rule / ilqr_reset_why (include/ilqr_amd.h), and ILQR_LAMBDA_MAX of ilqr_status
enum { RESET_RULE_NONFINITE = 1, RESET_RULE_LAMBDA_MAX = 2 };
enum { RESET_WAS_MASKED = 1, RESET_WAS_NONFINITE = 2, RESET_WAS_LAMBDA_MAX = 4 };
constexpr int kStatusLambdaMax = 3;

// finite: the exponent field is not all ones -- on the bits, not a comparison the compiler may fold under the build's floating-point options
__device__ __forceinline__ bool finite_bits(double c) {
  return ((unsigned long long)__double_as_longlong(c) >> 52 & 0x7ffull) != 0x7ffull;
}

// One thread per slot of the padded batch; padding lanes b >= B are never selected.
//   repeat = 0  the selection of a call: mask (may be null), rules on cost / status.  flags[b] = sel[b] = why (0: not selected).
//   repeat = 1  after a warm rollout (ilqr_mpc_step_reset under ILQR_RESET_NONFINITE): sel[b] = ILQR_WAS_NONFINITE where the new cost is
//               not finite, else 0; flags[b] |= sel[b]; commit_idx[b] = 0 for those, -1 for the rest -- whom the repeated rollout skips.
// A selected slot gets lambda, dlambda and the run state of a fresh trajectory (k_reset_state's); its cost stays (the next rollout's).
template <class real>
__global__ void k_select_reset(BatchViewT<real> v, const int* __restrict__ mask, int rules, int repeat, double lambda0, double dlambda0,
                               int* __restrict__ sel, int* __restrict__ flags, int* __restrict__ commit_idx) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= v.Bp) return;
  int why = 0;
  if (b < v.B) {
    if (!repeat && mask && mask[b] != 0) why |= RESET_WAS_MASKED;
    if ((rules & RESET_RULE_NONFINITE) && !finite_bits(v.cost[b])) why |= RESET_WAS_NONFINITE;
    if (!repeat && (rules & RESET_RULE_LAMBDA_MAX) && v.status[b] == kStatusLambdaMax) why |= RESET_WAS_LAMBDA_MAX;
  }
  sel[b] = why;
  if (repeat) {
    if (why) flags[b] |= why;
    commit_idx[b] = why ? 0 : -1;
  } else {
    flags[b] = why;
  }
  if (!why) return;
  v.lambda[b] = lambda0;
  v.dlambda[b] = dlambda0;
  reset_run_state(v, b);
}

// The nominal of the selected trajectories: us = the reset controls (null: zeros), xs = k = K = 0.  k_shift_horizon's decomposition
// (layout.hpp): an array is segments of S knots of W contiguous elements -- a tile ([S][E][16]: element i belongs to lane i % 16) or a
// trajectory of the trajectory-contiguous layout (every element its own).  One workgroup per segment and array reads the segment's 16 (or 1)
// selections first and leaves if none is set: a step in which nobody resets costs the launch.  Otherwise consecutive threads walk consecutive
// elements and store where the owning lane is selected.  Stores only -- the nominal is never loaded -- and none behind a segment's S W
// elements (the kRolloutFetchSlack rows of the tiled arrays).
struct ResetArray {
  void* a;          // the array (float or double, as the handle stores it)
  const void* src;  // what a selected element becomes: an array of the same layout and type, or null = zero
  int S, W;
};
struct ResetSet {
  ResetArray arr[4];  // xs, us, k, K
  const int* sel;     // [nseg * lanes]
  int nseg, lanes;    // lanes: trajectories interleaved in a segment, TW or 1
};
template <class real>
__global__ void __launch_bounds__(256) k_reset_nominal(ResetSet set) {
  const ResetArray A = set.arr[blockIdx.y];
  if (!A.a) return;
  const size_t n = (size_t)A.S * A.W;
  const int lanes = set.lanes;
  const int mine = (int)(threadIdx.x % (unsigned)lanes);  // (256 is a multiple of TW: a thread stays on one lane of its tile)
  for (int seg = blockIdx.x; seg < set.nseg; seg += gridDim.x) {
    unsigned any = 0, me = 0;
    for (int l = 0; l < lanes; l++) {
      const unsigned s = set.sel[(size_t)seg * lanes + l] != 0;
      any |= s;
      if (l == mine) me = s;
    }
    if (!any) continue;  // (uniform: the whole workgroup read the same selections)
    if (!me) continue;
    real* p = (real*)A.a + (size_t)seg * n;
    const real* s = A.src ? (const real*)A.src + (size_t)seg * n : nullptr;
    if (s) {
      for (size_t i = threadIdx.x; i < n; i += 256) p[i] = s[i];
    } else {
      for (size_t i = threadIdx.x; i < n; i += 256) p[i] = real(0);
    }
  }
}

// the repeated warm rollout of the tiled routes scores every trajectory of a tile: its costs go to a scratch row, and only the
// selected trajectories take theirs -- an unselected trajectory's cost is not rewritten
__global__ void k_take_reset_cost(const double* __restrict__ scratch, const int* __restrict__ sel, double* __restrict__ cost, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B && sel[b]) cost[b] = scratch[b];
}

}  // namespace ilqr
