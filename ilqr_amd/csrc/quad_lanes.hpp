// quad_lanes.hpp -- who does what in a QUAD rollout wavefront (rollout.hpp, rollout_tile<.., QUAD = true>: k_solve_hex).  Plain constexpr
// functions that compile on the host (tests/native/quad_lanes_host.hip).
//
// The wavefront of pair s rolls out the four trajectories l = 4 s + q of its sub-tile under ALL eleven alphas:
//     rollout  lane = 4 alpha + q   alpha 0..10, q 0..3   (44 lanes; lanes 44..63 take no part and store nothing)
// and the same lanes pass the quad's nominal rows (u, k, K, xs of step t: NROWS per trajectory) from memory through LDS:
//     fetch    lane = 4 row + q     row 0..NROWS-1        (40 lanes for the acrobot's ten rows)
// Lane j rolls out and fetches for the SAME trajectory q = j & 3.  The rollout lanes beyond the last row (40..43) repeat the last row's
// fetch: the same address and the same LDS slot as lanes 36..39, the same value -- no lane predicate in the step.
#pragma once
#include "common.hpp"

namespace ilqr {

constexpr int kQuad = 4;  // trajectories per quad (= a chain wavefront's sub-tile, backward_hex.hpp: HT)

constexpr int quad_rollout_lanes(int nalpha) { return kQuad * nalpha; }
constexpr int quad_lane_alpha(int lane) { return lane / kQuad; }
constexpr int quad_lane_q(int lane) { return lane % kQuad; }
constexpr int quad_traj(int s, int q) { return kQuad * s + q; }  // trajectory of the tile
// the row whose value lane `lane` fetches
constexpr int quad_fetch_row(int lane, int nrows) { return lane / kQuad < nrows ? lane / kQuad : nrows - 1; }

// A step's rows in a wavefront's LDS: [row pair][trajectory of the tile][2] -- a lane reads rows 2 p and 2 p + 1 of its trajectory as one
// piece of two values at rollout_share_pair(p, l).
constexpr int rollout_share_slot(int row, int l) { return ((row >> 1) * TW + l) * 2 + (row & 1); }
constexpr int rollout_share_pair(int p, int l) { return (p * TW + l) * 2; }
constexpr int rollout_rows(int nx, int nu) { return 2 * nu + nu * nx + nx; }  // u, k, K, xs

// Row `row` of the step's rows: which array, which element of its knot, elements per knot and knots per tile of that array.
enum { ROW_US = 0, ROW_KFF = 1, ROW_KFB = 2, ROW_XS = 3 };
struct RowSource {
  int array, elem, E, S;
};
constexpr RowSource rollout_row_source(int row, int nx, int nu, int T) {
  return row < nu                 ? RowSource{ROW_US, row, nu, T}
         : row < 2 * nu           ? RowSource{ROW_KFF, row - nu, nu, T}
         : row < 2 * nu + nu * nx ? RowSource{ROW_KFB, row - 2 * nu, nu * nx, T}
                                  : RowSource{ROW_XS, row - 2 * nu - nu * nx, nx, T + 1};
}
// element of its array that the fetch of (row, trajectory l of `tile`) reads for step tt (tt runs to T - 1 + PD: unclamped, into the
// arrays' spare elements) -- tidx(tile, 0, ..) plus tt knots
constexpr size_t rollout_row_elem(const RowSource& r, int tile, int tt, int l) {
  return ((((size_t)tile * r.S) * r.E + r.elem) * TW + l) + (size_t)tt * r.E * TW;
}

}  // namespace ilqr
