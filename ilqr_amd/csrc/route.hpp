// route.hpp -- which of several equivalent kernels a handle runs, decided once at ilqr_create, and the names
// ilqr_stage_kernel_name reports for it.  Host code only: tests/test_route_plan.py builds it with a host compiler.
#pragma once
#include "../../include/ilqr_amd.h"

namespace ilqr {

// ilqr_iterate's persistent kernel (nx = 4, no ILQR_FLAG_STAGED / _UNFUSED): up to one tile per CU k_solve_hex (m = 1, no opt-in fixes:
// four matrix-core chains) or k_solve_tile<.., 1>; beyond two per CU, m <= 2, no opt-in fixes, 64-trajectory wide tiles; otherwise two
// 16-trajectory tiles per CU, k_solve_tile<.., 2>.  ILQR_ROUTE_TILE_PER_CU / TWO_TILES_PER_CU / WIDE_TILES force one (A/B runs, tests).
enum class Solve { none, hex, tile1, tile2, wide, wide2 };
// ILQR_FLAG_STAGED: k_sweep_backward (records in LDS, three producers; one on a 60 KB ring at two tiles per CU), beyond that stage kernels
enum class Sweep { none, three_producers, one_producer };
// fused_lq: no sweep, k_backward_w3<.., LQF> forms cx, cu from the knot; lq: k_derivatives_lq + k_derivatives_g for knot T
enum class Derivatives { tiled, analytic_lq, lq, generic, fused_lq };
// w3_regv: ILQR_FLAG_REGULARIZE_VXX's bounds-checked k_backward_w3; w3_two_tiles: two 16-column control tiles (nu > 16 or by route bit)
enum class Backward { quad, thread, w3, w3_regv, w3_two_tiles, w2 };
// tiled: k_rollout accepts per tile; lq_accept: k_rollout_lq accepts and keeps its candidates; lq, generic: k_accept after the search
enum class Rollout { tiled, lq_accept, lq, generic };
// k_commit from the alpha planes, k_commit_lq from the LQ search's kept rollouts, or the accepted rollout run again in place
enum class Commit { tiled, lq_copy, rerun };
// the model rows the generic kernels read: none (ilqr_create's parameters for all), one per trajectory, one per knot of every trajectory
enum class ModelRows { none, per_trajectory, per_knot };

struct RoutePlan {  // (the defaults: what ilqr_stage_kernel_name reports for a null handle)
  Solve solve = Solve::none;
  Sweep sweep = Sweep::none;
  Derivatives derivatives = Derivatives::tiled;
  Backward backward = Backward::thread;
  Rollout rollout = Rollout::tiled;
  Commit commit = Commit::tiled;
  // the handle's model rows: none, one per trajectory (ilqr_set_trajectory_params) or one per knot (ilqr_set_knot_params), until
  // ilqr_clear_trajectory_params.  Every launch that hands the user twin to k_rollout_g / k_derivatives_g / k_evaluate_g takes the PT or
  // the PK instantiation accordingly (launch.hpp: with_trajectory_params).  The one part of the plan that changes after ilqr_create.
  ModelRows traj_params = ModelRows::none;
};

// Which instantiation of a wavefront-per-trajectory kernel a handle of these sizes runs, as plain data (launch.hpp turns it into template
// arguments and says which combinations are built).  nt: 16-row tiles covering nx; mt: 16-column control tiles covering nu, or two by
// route bit; full: no masked rows or columns (nx = 32, nu = 16); lqf: cx, cu formed from the knot (the fused LQ route).
struct WaveVariant {
  int nt, mt;
  bool full, lqf, regv, f32;
};
inline WaveVariant backward_wave_variant(Backward b, int nx, int nu, int dtype, bool fused) {  // k_backward_w3, and nt of k_backward_w2
  const bool plain = b == Backward::w3;
  return {nx > 16 ? 2 : 1, b == Backward::w3_two_tiles ? 2 : 1, plain && nx == 32 && nu == 16, plain && fused, b == Backward::w3_regv,
          dtype == ILQR_DTYPE_F32};
}
inline WaveVariant value_wave_variant(int nx, int nu, int dtype) {  // k_value_w
  return {nx > 16 ? 2 : 1, nu > 16 ? 2 : 1, false, false, false, dtype == ILQR_DTYPE_F32};
}
inline const char* value_kernel_name(bool aos, const WaveVariant& w) {
  static const char* const kWave[2][2] = {{"k_value_w<1, 1>", "k_value_w<1, 2>"}, {"k_value_w<2, 1>", "k_value_w<2, 2>"}};
  return aos ? kWave[w.nt - 1][w.mt - 1] : "k_value_t";
}
inline const char* covariance_kernel_name(bool aos, const WaveVariant& w) {  // k_covariance_w: the variants value_wave_variant yields
  static const char* const kWave[2][2] = {{"k_covariance_w<1, 1>", "k_covariance_w<1, 2>"}, {"k_covariance_w<2, 1>", "k_covariance_w<2, 2>"}};
  return aos ? kWave[w.nt - 1][w.mt - 1] : "k_covariance_t";
}
inline const char* tangent_kernel_name(bool aos, const WaveVariant& w) {  // k_tangent_w: the variants value_wave_variant yields
  static const char* const kWave[2][2] = {{"k_tangent_w<1, 1>", "k_tangent_w<1, 2>"}, {"k_tangent_w<2, 1>", "k_tangent_w<2, 2>"}};
  return aos ? kWave[w.nt - 1][w.mt - 1] : "k_tangent_t";
}
inline const char* adjoint_kernel_name(bool aos, const WaveVariant& w) {  // k_adjoint_w: the same variants
  static const char* const kWave[2][2] = {{"k_adjoint_w<1, 1>", "k_adjoint_w<1, 2>"}, {"k_adjoint_w<2, 1>", "k_adjoint_w<2, 2>"}};
  return aos ? kWave[w.nt - 1][w.mt - 1] : "k_adjoint_t";
}
inline const char* lq_solve_kernel_name(bool aos, const WaveVariant& w) {  // k_lq_gain_w (then k_lq_back_w, k_lq_fwd_w): the same variants
  static const char* const kWave[2][2] = {{"k_lq_gain_w<1, 1>", "k_lq_gain_w<1, 2>"}, {"k_lq_gain_w<2, 1>", "k_lq_gain_w<2, 2>"}};
  return aos ? kWave[w.nt - 1][w.mt - 1] : "k_lq_gain_t";
}
inline const char* estimator_kernel_name(bool aos, int nt, int yt) {  // k_est_filter_w by (state tiles, output tiles: ny <= 16 yt <= 16 nt)
  static const char* const kWave[2][2] = {{"k_est_filter_w<1, 1>", "k_est_filter_w<1, 2>"}, {"k_est_filter_w<2, 1>", "k_est_filter_w<2, 2>"}};
  return aos ? kWave[nt - 1][yt - 1] : "k_estimator_t";
}
inline const char* estimator_loop_kernel_name(const WaveVariant& w) {  // k_est_loop_w: the variants value_wave_variant yields
  static const char* const kWave[2][2] = {{"k_est_loop_w<1, 1>", "k_est_loop_w<1, 2>"}, {"k_est_loop_w<2, 1>", "k_est_loop_w<2, 2>"}};
  return kWave[w.nt - 1][w.mt - 1];
}
inline const char* risk_kernel_name(bool aos, const WaveVariant& w, int wt) {  // k_risk_w by (state, control, noise tiles: nw <= 16 wt <= 16 nt)
  static const char* const kWave[2][2][2] = {{{"k_risk_w<1, 1, 1>", "k_risk_w<1, 1, 2>"}, {"k_risk_w<1, 2, 1>", "k_risk_w<1, 2, 2>"}},
                                             {{"k_risk_w<2, 1, 1>", "k_risk_w<2, 1, 2>"}, {"k_risk_w<2, 2, 1>", "k_risk_w<2, 2, 2>"}}};
  return aos ? kWave[w.nt - 1][w.mt - 1][wt - 1] : "k_risk_t";
}
inline const char* evaluate_kernel_name(bool aos, ModelRows rows) {
  static const char* const kRows[] = {"k_evaluate_g", "k_evaluate_g<PT>", "k_evaluate_g<PK>"};
  return aos ? kRows[(int)rows] : "k_evaluate_t";
}
// k_pg_contract (param_gradient.hpp): how a wavefront's eight lane octets are shared out for a twin of ntp per-trajectory parameters, as
// plain data -- dirs directions side by side (ntp <= 4), or passes rounds of eight parameters for one direction (ntp > 8)
struct ParamGradientShape {
  int dirs, passes;
};
constexpr ParamGradientShape pg_shape(int ntp) { return {ntp >= 1 && ntp <= 4 ? 8 / ntp : 1, ntp > 8 ? (ntp + 7) / 8 : 1}; }
inline const char* param_gradient_kernel_name(int dtype) { return dtype == ILQR_DTYPE_F32 ? "k_pg_contract<float>" : "k_pg_contract"; }

struct RouteInputs {
  int model, nx, nu, flags, route, ntiles, num_cus;  // (num_cus after ilqr_desc.assume_cus)
  bool user_tiled, user_small;  // the build's user twin: kUserTiled, kUserSmall (models.hpp)
  bool cands_allocated;         // the LQ search's candidate buffers (not under ILQR_ROUTE_LQ_RECOMMIT, nor if the device could not spare them)
  int dtype = ILQR_DTYPE_F64;   // ilqr_desc.dtype: an fp32 LQ handle searches with the thread-per-rollout kernel (k_rollout_lq is fp64)
};

// trajectory-contiguous layout, generic kernels: host-evaluated models, the LQ model, user twins without tiled kernels or sent there
inline bool generic_layout(int model, int route, bool user_tiled, bool user_small) {
  if (model == ILQR_MODEL_LQ || model == ILQR_MODEL_HOST) return true;
  return model == ILQR_MODEL_USER && (!user_tiled || (user_small && (route & ILQR_ROUTE_WAVE_PER_TRAJECTORY)));
}
// the LQ model's line search on the matrix cores (k_rollout_lq is written for 32 x 16): what candidate buffers are allocated for
inline bool lq_matrix_core_search(int model, int nu, int route) {
  return model == ILQR_MODEL_LQ && nu <= 16 && !(route & ILQR_ROUTE_LQ_THREAD_ROLLOUT);
}

// can this plan take per-trajectory model parameters?  Only where the model is touched by k_rollout_g and k_derivatives_g alone
inline bool takes_trajectory_params(const RoutePlan& p) {
  return p.rollout == Rollout::generic && p.derivatives == Derivatives::generic && p.commit == Commit::rerun;
}

inline RoutePlan plan_route(const RouteInputs& in) {
  RoutePlan p;
  const int fl = in.flags, rt = in.route;
  if (generic_layout(in.model, rt, in.user_tiled, in.user_small)) {
    const bool lq = in.model == ILQR_MODEL_LQ, lq_wide = lq && in.nu > 16;
    p.backward = (in.nu > 16 || (rt & ILQR_ROUTE_TWO_CONTROL_TILES)) ? Backward::w3_two_tiles : (rt & ILQR_ROUTE_BACKWARD_W2) ? Backward::w2
                 : (fl & ILQR_FLAG_REGULARIZE_VXX) ? Backward::w3_regv : Backward::w3;
    const bool analytic = (fl & ILQR_FLAG_ANALYTIC_DERIVATIVES) != 0;
    if (lq && analytic && !(rt & ILQR_ROUTE_FULL_RECORDS) && p.backward == Backward::w3) p.derivatives = Derivatives::fused_lq;
    else if (lq && analytic && !lq_wide) p.derivatives = Derivatives::analytic_lq;
    else if (lq && !(rt & ILQR_ROUTE_LQ_DENSE_FD) && !lq_wide) p.derivatives = Derivatives::lq;
    else p.derivatives = Derivatives::generic;
    p.rollout = (!lq_matrix_core_search(in.model, in.nu, rt) || in.dtype == ILQR_DTYPE_F32) ? Rollout::generic : in.cands_allocated ? Rollout::lq_accept : Rollout::lq;
    p.commit = p.rollout == Rollout::lq_accept ? Commit::lq_copy : Commit::rerun;
    return p;
  }
  const bool quad = in.nx == 4 && !(fl & ILQR_FLAG_BACKWARD_THREAD_PER_TRAJ);
  p.backward = quad ? Backward::quad : Backward::thread;
  if (!quad || (fl & ILQR_FLAG_UNFUSED)) return p;
  const bool staged = (fl & ILQR_FLAG_STAGED) != 0;
  const bool wide_ok = !staged && in.nu <= 2 && !(fl & (ILQR_FLAG_REFERENCE_FIXES | ILQR_FLAG_REGULARIZE_VXX));
  const Solve one_per_cu = (wide_ok && in.nu == 1 && !(rt & ILQR_ROUTE_QUAD_CHAIN)) ? Solve::hex : Solve::tile1;
  const Solve wide = in.nu == 1 ? Solve::wide : Solve::wide2;
  Solve s;
  switch (rt & 3) {
    case ILQR_ROUTE_TILE_PER_CU: s = one_per_cu; break;
    case ILQR_ROUTE_TWO_TILES_PER_CU: s = Solve::tile2; break;
    case ILQR_ROUTE_WIDE_TILES: s = wide_ok ? wide : Solve::tile2; break;
    default:  // by batch size: a third 16-trajectory tile per CU would be a second round of tile2 (1.49 against 1.16-1.27 ms at B = 8448 .. 14336)
      s = in.ntiles <= in.num_cus ? one_per_cu : (wide_ok && in.ntiles > 2 * in.num_cus) ? wide
          : (!staged || in.ntiles <= 2 * in.num_cus) ? Solve::tile2 : Solve::none;
  }
  if (!staged) p.solve = s;
  else if (s != Solve::none) p.sweep = s == Solve::tile2 ? Sweep::one_producer : Sweep::three_producers;
  return p;
}

// as rocprofv3 reports it; persistent and fused-sweep handles report k_sweep_backward for the backward stage (what ilqr_iterate runs)
inline const char* stage_kernel_name(const RoutePlan& p, int stage) {
  static const char* const kSolve[] = {"", "k_solve_hex", "k_solve_tile", "k_solve_tile<2>", "k_solve_wide", "k_solve_wide2"};
  static const char* const kDerivatives[] = {"k_derivatives", "k_analytic_lq", "k_derivatives_lq", "k_derivatives_g", ""};
  static const char* const kBackward[] = {"k_backward_q", "k_backward_t", "k_backward_w3", "k_backward_w3", "k_backward_w3w", "k_backward_w2"};
  static const char* const kRollout[] = {"k_rollout", "k_rollout_lq", "k_rollout_lq", "k_rollout_g"};
  switch (stage) {
    case ILQR_STAGE_DERIVATIVES: return kDerivatives[(int)p.derivatives];
    case ILQR_STAGE_BACKWARD: return (p.solve != Solve::none || p.sweep != Sweep::none) ? "k_sweep_backward" : kBackward[(int)p.backward];
    case ILQR_STAGE_ROLLOUT: return kRollout[(int)p.rollout];
    case ILQR_STAGE_ACCEPT: return "k_accept";
    case ILQR_STAGE_SOLVE: return kSolve[(int)p.solve];
    default: return "";
  }
}

}  // namespace ilqr
