// Host build of the quad rollout's lane maps (ilqr_amd/csrc/quad_lanes.hpp) and of the fetch slack (rollout.hpp), so that who rolls out
// what, who fetches which row into which LDS slot, and how far the unclamped prefetch reaches can be tested on a machine without a GPU.
// TEST INFRASTRUCTURE.
#include "../../ilqr_amd/csrc/rollout.hpp"
using namespace ilqr;

extern "C" int quad_rollout_lane_count() { return quad_rollout_lanes(NALPHA); }
extern "C" int quad_row_count(int nx, int nu) { return rollout_rows(nx, nu); }
extern "C" int quad_prefetch_depth() { return kDeepPrefetch<AcrobotModelT<double>>; }
// lane -> (alpha, trajectory of the tile) of the wavefront of pair s
extern "C" void quad_rollout_map(int s, int* alpha, int* l) {
  for (int lane = 0; lane < 64; lane++) {
    alpha[lane] = quad_lane_alpha(lane);
    l[lane] = quad_traj(s, quad_lane_q(lane));
  }
}
// lane -> (row, trajectory) it fetches and the LDS element it writes, for every lane that takes part (lane < quad_rollout_lanes)
extern "C" void quad_fetch_map(int s, int nrows, int* row, int* l, int* slot) {
  for (int lane = 0; lane < 64; lane++) {
    row[lane] = quad_fetch_row(lane, nrows);
    l[lane] = quad_traj(s, quad_lane_q(lane));
    slot[lane] = rollout_share_slot(row[lane], l[lane]);
  }
}
// the LDS elements lane `lane` of the wavefront of pair s reads per step: two per row pair
extern "C" void quad_read_slots(int s, int lane, int npair, int* slot) {
  const int l = quad_traj(s, quad_lane_q(lane));
  for (int p = 0; p < npair; p++) {
    slot[2 * p] = rollout_share_pair(p, l);
    slot[2 * p + 1] = rollout_share_pair(p, l) + 1;
  }
}
// the element of its array that lane `lane` fetches for step tt; *array says which (ROW_US, ROW_KFF, ROW_KFB, ROW_XS)
extern "C" long long quad_fetch_elem(int nx, int nu, int T, int tile, int s, int lane, int tt, int* array) {
  const RowSource r = rollout_row_source(quad_fetch_row(lane, rollout_rows(nx, nu)), nx, nu, T);
  *array = r.array;
  return (long long)rollout_row_elem(r, tile, tt, quad_traj(s, quad_lane_q(lane)));
}
// what the same (row, trajectory, step) is in the arrays' own index map (common.hpp), for tt inside the horizon
extern "C" long long quad_tidx(int tile, int s, int e, int l, int S, int E) { return (long long)tidx(tile, s, e, l, S, E); }
// elements a handle allocates for an array of S knots of E elements: the layout's, plus the spare rows of the unclamped prefetch
extern "C" long long quad_alloc_elems(int ntiles, int S, int E, int nx, int nu) {
  return (long long)(layout_elems(false, 0, ntiles, (size_t)S, (size_t)E) + rollout_fetch_slack_elems(nx, nu));
}
