// launch.hpp -- kernel launchers of the C ABI.  Every kernel template is named in one launch expression; what picks its instantiation
// at launch -- the handle's device model and arithmetic, its route plan (which of several equivalent kernels it runs: route.hpp,
// DESIGN.md 3.2), its sizes -- reaches that expression as a type, through the with_* dispatchers here and in handle.hpp.  Where only
// some combinations of a kernel's switches are built, the `if constexpr` beside the launch is the list of them: a generic lambda
// instantiates whatever it is handed, so a combination that is not excluded there is compiled.  The wavefront-per-trajectory kernels of the
// stored-model queries share one such list and one dispatcher, with_wave_tiles.  Included once, by capi.hip.
#pragma once
#include "handle.hpp"

// ------------------------------------------------------------------------------------------
// kernel launchers
// ------------------------------------------------------------------------------------------
// one thread per slot of the padded batch (k_reset_state, k_warm_reset, k_select_reset, k_accept: scalars only)
template <class... P, class... A>
static int launch_per_slot(ilqr_batch* h, void (*kernel)(P...), const A&... a) {
  hipLaunchKernelGGL(kernel, dim3((h->Bp + 255) / 256), dim3(256), 0, h->stream, static_cast<P>(a)...);
  HIPCHK(hipGetLastError());
  return 0;
}

// cand = true: controls + checkpoint states go to the candidate buffers; false: straight into xs/us (init).  The candidate rollouts alone
// have deep-prefetch and accepting instantiations: the init rollout's two switches are pinned in the template arguments themselves
template <class V, class M>
static int launch_rollout_t(ilqr_batch* h, const V& v, const M& m, bool gains, bool cand, const AlphaSet& al, int n_alpha,
                            double* cost_out, int mode, bool with_accept) {
  if (gains != cand) return fail(ILQR_ERR_INVALID, "unsupported rollout variant");
  const int aw = (n_alpha + 3) / 4;  // wavefronts per tile: 4 alphas each
  const int depth = h->ntiles <= h->num_cus ? kDeepPrefetch<M> : 4;  // one block per CU: deep prefetch (see k_rollout)
  return with_bool(gains, [&](auto g) { return with_bool(with_accept, [&](auto acc) { return with_int<kDeepPrefetch<M>, 4>(depth, [&](auto pd) {
    constexpr bool G = decltype(g)::value, ACCEPT = G && decltype(acc)::value;
    hipLaunchKernelGGL((k_rollout<M, G, G, G ? decltype(pd)::value : 4, ACCEPT>), dim3(h->ntiles), dim3(64 * aw), 0, h->stream, v, m, al, n_alpha,
                       cost_out, mode, h->sp, ACCEPT ? h->commit_idx : nullptr);
    HIPCHK(hipGetLastError());
    return 0;
  }); }); });
}
// f(model) for the handle's generic device twin (fp32 handle: the double twin its finite differences are taken in)
template <class F>
static int with_generic_model(ilqr_batch* h, F&& f) {
  if (h->model == ILQR_MODEL_LQ) return h->lq_wide ? f(h->lq_w) : f(h->lq);
#ifdef ILQR_HAVE_USER_MODEL
  if constexpr (kUserGeneric)
    if (h->model == ILQR_MODEL_USER) return f(h->user_g);
#endif
  return fail(ILQR_ERR_UNSUPPORTED, "model %d has no generic device kernels", h->model);
}
// f(model) for the model the handle's generic rollouts integrate: the float twin on an fp32 handle
template <class F>
static int with_rollout_model(ilqr_batch* h, F&& f) {
  if (h->dtype != ILQR_DTYPE_F32) return with_generic_model(h, f);
  if (h->model == ILQR_MODEL_LQ) return f(h->lq_f);
#ifdef ILQR_HAVE_USER_MODEL
  if constexpr (kUserGeneric)
    if (h->model == ILQR_MODEL_USER) return f(h->user_gf);
#endif
  return fail(ILQR_ERR_UNSUPPORTED, "model %d has no fp32 generic device kernels", h->model);
}
// the model with the handle's rows behind it: what the PT and PK instantiations of k_rollout_g / k_derivatives_g / k_evaluate_g take (the
// per-trajectory rows, or the per-knot window while the handle is in knot mode)
template <class M>
static PerTrajectory<M> per_trajectory(const ilqr_batch* h, const M& m) {
  PerTrajectory<M> pm;
  static_cast<M&>(pm) = m;
  pm.traj_params = h->plan.traj_params == ModelRows::per_knot ? h->knot_params : h->traj_params;
  return pm;
}
// f(model argument, PT) for a kernel with PT and PK instantiations: (per_trajectory(h, m), PT_ROWS) while the handle holds per-trajectory
// parameters -- every lane's model copy is then set from its trajectory's row --, (per_trajectory(h, m), PK_ROWS) while it holds per-knot
// rows -- set from row (b, t) before anything is evaluated at knot t --, else (m, ROWS_NONE)
static_assert((int)ModelRows::none == ROWS_NONE && (int)ModelRows::per_trajectory == PT_ROWS && (int)ModelRows::per_knot == PK_ROWS,
              "route.hpp's ModelRows are generic.hpp's template values");
template <class M, class F>
static int with_trajectory_params(const ilqr_batch* h, const M& m, F&& f) {
  if constexpr (has_trajectory_params<M>::value) {
    if (h->plan.traj_params == ModelRows::per_trajectory) return f(per_trajectory(h, m), std::integral_constant<int, PT_ROWS>());
    if (h->plan.traj_params == ModelRows::per_knot) return f(per_trajectory(h, m), std::integral_constant<int, PK_ROWS>());
  }
  return f(m, std::integral_constant<int, ROWS_NONE>());
}
// generic path (generic.hpp): WHAT = RG_INIT / RG_SEARCH / RG_COMMIT.  The LQ model rolls out on the
// matrix cores (k_rollout_lq, one wavefront per trajectory); ILQR_ROUTE_LQ_THREAD_ROLLOUT selects the
// generic thread-per-rollout kernel (same results bit for bit; kept as the cross-check and as the
// template for device models without matrix structure).
template <int WHAT, class M>
static int launch_rollout_g(ilqr_batch* h, const M& m, const AlphaSet& al, double* cost_out, int mode, int write_cost, bool with_accept = false) {
  constexpr bool search = WHAT == RG_SEARCH, commit = WHAT == RG_COMMIT;
  const int md = search ? mode : 0, wc = search ? 0 : commit ? write_cost : 1;  // (the search scores only; the init rollout always writes its cost)
  if constexpr (std::is_same<M, LqModel>::value)
  if (h->plan.rollout != Rollout::generic) {
    const bool keeps = h->plan.rollout == Rollout::lq_accept;  // candidate buffers: the commit of what the next accept chooses is a copy (launch_commit)
    if (search) h->lq_cands_kept = keeps;
    return with_bool(search && with_accept && keeps, [&](auto acc) {
      constexpr bool ACCEPT = search && decltype(acc)::value;
      hipLaunchKernelGGL((k_rollout_lq<WHAT, ACCEPT>), dim3(h->B), dim3(64), 0, h->stream, h->v, m, al, cost_out,
                         (ACCEPT || commit) ? h->commit_idx : nullptr, md, wc, h->sp);
      HIPCHK(hipGetLastError());
      return 0;
    });
  }
  const dim3 grid(search ? (h->B + kSearchTraj - 1) / kSearchTraj : (h->B + 63) / 64);
  return with_trajectory_params(h, m, [&](const auto& pm, auto pt) {
    hipLaunchKernelGGL((k_rollout_g<M, WHAT, decltype(pt)::value>), grid, dim3(64), 0, h->stream, view_of<typename M::real>(h), pm, al, cost_out,
                       commit ? h->commit_idx : nullptr, md, wc, h->sp.fixes);
    HIPCHK(hipGetLastError());
    return 0;
  });
}

// with_accept (tiled models, 11-alpha search): the rollout kernel also does STEP 3/4 for its tile
static int launch_rollout(ilqr_batch* h, bool gains, bool cand, const AlphaSet& al, int n_alpha, double* cost_out, int mode,
                          bool with_accept = false) {
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (int rc = timer_begin(h, ILQR_STAGE_ROLLOUT, &ev)) return rc;
  const int rc = (h->plan.rollout != Rollout::tiled)
      ? with_rollout_model(h, [&](auto& m) {
          if (!gains) return launch_rollout_g<RG_INIT>(h, m, al, cost_out, 0, 1);
          if (n_alpha == NALPHA) return launch_rollout_g<RG_SEARCH>(h, m, al, cost_out, mode, 0, with_accept);
          return launch_rollout_g<RG_COMMIT>(h, m, al, cost_out, 0, 1);  // a single closed-loop rollout written in place (warm start): slot commit_idx of `al`
        })
      : with_model(h, [&](auto& v, auto& m, auto&) { return launch_rollout_t(h, v, m, gains, cand, al, n_alpha, cost_out, mode, with_accept); });
  if (rc) return rc;
  if (cand && h->cands == Cands::grouped) h->cands = Cands::planes;  // (the stage kernels write the alpha planes)
  return timer_end(h, ILQR_STAGE_ROLLOUT, ev);
}

static int refuse_grouped_cands(ilqr_batch* h) {  // k_commit and k_derivatives' fused commit index the candidates as alpha planes
  return h->cands != Cands::grouped ? 0 : fail(ILQR_ERR_STATE, "the candidate buffers hold k_solve_hex's grouped layout: nothing reads them as alpha planes");
}

static AlphaSet line_search_alphas();
static int launch_commit(ilqr_batch* h) {
  if (h->plan.commit == Commit::lq_copy && h->lq_cands_kept) {  // the matrix-core search kept its eleven rollouts: copy the accepted one
    hipLaunchKernelGGL(k_commit_lq, dim3(h->B), dim3(256), 0, h->stream, h->v, h->nx, h->nu, h->commit_idx);
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (h->plan.commit != Commit::tiled)  // no stored candidates otherwise on the generic path: re-run the accepted rollout in place
    return with_rollout_model(h, [&](auto& m) { return launch_rollout_g<RG_COMMIT>(h, m, line_search_alphas(), h->v.cost, 0, 0); });
  if (int rc = refuse_grouped_cands(h)) return rc;
  dim3 grid((h->T + 1 + 15) / 16, h->ntiles), block(256);
  if (int rc = with_model(h, [&](auto& v, auto& m, auto&) {
        hipLaunchKernelGGL((k_commit<std::decay_t<decltype(m)>>), grid, block, 0, h->stream, v, m, h->commit_idx);
        return 0;
      }))
    return rc;
  HIPCHK(hipGetLastError());
  return 0;
}

// copy an accepted-but-not-yet-copied candidate into the nominal trajectory now
static int flush_commit(ilqr_batch* h) {
  if (!h->commit_pending) return 0;
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (int rc = timer_begin(h, ILQR_STAGE_ACCEPT, &ev)) return rc;
  if (int rc = launch_commit(h)) return rc;
  h->commit_pending = false;
  HIPCHK(hipMemsetAsync(h->commit_idx, 0xFF, (size_t)h->Bp * sizeof(int), h->stream));  // all -1
  return timer_end(h, ILQR_STAGE_ACCEPT, ev);
}

// A fresh solve starts: nothing of an earlier one may leak into it -- neither an accepted candidate whose
// copy is still pending (an ilqr_iterate that returned early on an error leaves one), nor the "records hold
// no matrices" state of an exact-derivative LQ sweep (init_traj promises zeroed records, ilqr_core.cpp:39-45).
static int forget_pending(ilqr_batch* h) {
  h->records_partial = false;
  h->lq_fused_stale = false;
  h->lq_caller_records = false;
  h->cands = Cands::none;  // (candidates of an earlier solve are nobody's)
  h->commit_pending = false;
  HIPCHK(hipMemsetAsync(h->commit_idx, 0xFF, (size_t)h->Bp * sizeof(int), h->stream));  // all -1
  return 0;
}
// A fresh trajectory, all of init_traj but x0, u0 and the rollout (ilqr_core.cpp:23-48): zero derivative records and gains, nothing
// pending, lambda / dlambda (the reference's file statics) as for a fresh process
static int fresh_trajectory(ilqr_batch* h) {
  const size_t T = h->T, T1 = h->T + 1;
  if (h->v.D) HIPCHK(hipMemsetAsync(h->v.D, 0, dev_elems(h, T1, rec_of(h)) * elem_size(h), h->stream));
  h->recs = ilqr_batch::REC_ZERO;
  HIPCHK(hipMemsetAsync(h->v.kff, 0, dev_elems(h, T, h->nu) * elem_size(h), h->stream));
  HIPCHK(hipMemsetAsync(h->v.Kfb, 0, dev_elems(h, T, h->nu * h->nx) * elem_size(h), h->stream));
  if (int rc = forget_pending(h)) return rc;
  return launch_per_slot(h, k_reset_state<double>, h->v, h->params.lambda_init, h->params.dlambda_init);
}
// The nominal is about to change under the handle (a shift, a reset of single trajectories): an accepted candidate not yet copied into
// xs / us belongs to the old one and is copied now; the candidates are rollouts of the old one; its records are recomputed when asked for
static int nominal_changes(ilqr_batch* h) {
  if (int rc = flush_commit(h)) return rc;
  h->cands = Cands::none;
  h->lq_cands_kept = false;
  if (!h->aos && h->recs == ilqr_batch::REC_VALID) h->recs = ilqr_batch::REC_STALE;
  return 0;
}
// The nominal's four arrays as k_shift_horizon and k_reset_nominal take them (layout.hpp): nseg segments -- tiles, or trajectories of the
// trajectory-contiguous layout -- of S knots of W contiguous elements, `lanes` trajectories interleaved in a segment
struct NominalArrays {
  struct { void* p; int S, W; } arr[4];  // xs, us, k, K
  int nseg, lanes;
};
static NominalArrays nominal_arrays(const ilqr_batch* h) {
  const int nx = h->nx, nu = h->nu, T = h->T, lanes = h->aos ? 1 : TW;
  return {{{h->v.xs, T + 1, nx * lanes}, {h->v.us, T, nu * lanes}, {h->v.kff, T, nu * lanes}, {h->v.Kfb, T, nu * nx * lanes}},
          h->aos ? h->B : h->ntiles, lanes};
}

// the generic finite-difference sweep (k_derivatives_g): a wavefront per knot, or with t_only >= 0 per trajectory for that knot alone
template <class M>
static int launch_derivatives_g(ilqr_batch* h, const M& m, int force, int t_only) {
  const dim3 grid(t_only < 0 ? h->B * (h->T + 1) : h->B);
  return with_trajectory_params(h, m, [&](const auto& pm, auto pt) { return with_view(h, [&](auto& v) {
    using S = std::remove_pointer_t<decltype(v.D)>;
    if constexpr (std::is_same_v<S, float> && (M::NU > WM)) {  // float records: twins of at most WM controls (ilqr_create lets no fp32 handle have more)
      return fail(ILQR_ERR_UNSUPPORTED, "k_derivatives_g: no fp32 handle has more than %d controls", WM);
    } else {
      hipLaunchKernelGGL((k_derivatives_g<M, S, decltype(pt)::value>), grid, dim3(64), 0, h->stream, v, pm, force, t_only);
      return 0;
    }
  }); });
}
static int launch_derivatives(ilqr_batch* h, int force) {
  const Derivatives route = h->plan.derivatives;
  if (route != Derivatives::tiled)  // the generic sweep has no fused commit: rebuild the accepted rollout first
    if (int rc = flush_commit(h)) return rc;
  if (route == Derivatives::fused_lq) {  // k_backward_w3<.., LQF> forms cx, cu from the knot itself: no sweep, no record array
    h->lq_fused_stale = true;
    h->lq_caller_records = false;
    return 0;
  }
  if (route == Derivatives::tiled && h->commit_pending)
    if (int rc = refuse_grouped_cands(h)) return rc;
  if (int rc = ensure_records(h)) return rc;
  h->recs = ilqr_batch::REC_VALID;
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (int rc = timer_begin(h, ILQR_STAGE_DERIVATIVES, &ev)) return rc;
  dim3 grid((h->T + 1 + 15) / 16, h->ntiles), block(256);
  const int* ci = h->commit_pending ? h->commit_idx : nullptr;
  if (route != Derivatives::tiled) {
    // fp32 handles: the same kernels' float-storage instantiations (float knots widened, double arithmetic, float records)
    int rc = 0;
    if (route == Derivatives::analytic_lq) {
      const int what = (h->route.full_records || h->dtype == ILQR_DTYPE_F32) ? 0 : 1;  // (A/B runs and the bit-identity test; fp32: whole records -- const_rec is double)
      const int chunk = (what == 1) ? 4 * kAnalyticChunk : kAnalyticChunk;
      const int nchunk = (h->T + 1 + chunk - 1) / chunk;
      rc = with_view(h, [&](auto& v) {
        hipLaunchKernelGGL((k_analytic_lq<std::remove_pointer_t<decltype(v.D)>>), dim3(h->B * nchunk), dim3(64), 0, h->stream, v, h->lq, force, what, h->const_rec, chunk);
        return 0;
      });
      h->records_partial = (what == 1);
    } else if (route == Derivatives::lq) {
      // the LQ twin: every perturbed point of the knots t < T evaluated by what moved (k_derivatives_lq), knot T by the generic sweep
      const int nchunk = (h->T + kLqKnotsPerWave - 1) / kLqKnotsPerWave;
      rc = with_view(h, [&](auto& v) {
        hipLaunchKernelGGL((k_derivatives_lq<std::remove_pointer_t<decltype(v.D)>>), dim3(h->B * nchunk), dim3(64), 0, h->stream, v, h->lq, force);
        return launch_derivatives_g(h, h->lq, force, h->T);
      });
    } else {
      rc = with_generic_model(h, [&](auto& m) { return launch_derivatives_g(h, m, force, -1); });
    }
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return timer_end(h, ILQR_STAGE_DERIVATIVES, ev);
  }
  if (int rc = with_model(h, [&](auto& v, auto& m, auto& fdm) {
        hipLaunchKernelGGL((k_derivatives<std::decay_t<decltype(m)>, std::decay_t<decltype(fdm)>>), grid, block, 0, h->stream, v, m, fdm, force, ci);
        return 0;
      }))
    return rc;
  HIPCHK(hipGetLastError());
  // the kernel above performed the copy on the way; commit_idx is rewritten for every trajectory
  // by the next k_accept and only read while commit_pending is set, so it needs no reset here
  h->commit_pending = false;
  return timer_end(h, ILQR_STAGE_DERIVATIVES, ev);
}

// The register-resident backward kernels of the generic layout, one wavefront per trajectory.  k_backward_w2<NT> (fp64 alone: ilqr_create), or
// the k_backward_w3 that `w` describes.  The `if constexpr` below is the list of the k_backward_w3 that exist: FULL only over two row tiles;
// REGV (ILQR_FLAG_REGULARIZE_VXX) on whole, masked records; two control tiles in fp64 and without any of the three.  What it excludes
// route.hpp never asks for (tests/test_route_plan.py), and refusing it here is what keeps it from being compiled.
static int launch_backward_w(ilqr_batch* h, const WaveVariant& w, bool w2, int mode, const double* crec) {
  const dim3 grid(h->B), block(64);
  if (w2)
    return with_int<1, 2>(w.nt, [&](auto nt) {
      hipLaunchKernelGGL(k_backward_w2<decltype(nt)::value>, grid, block, 0, h->stream, h->v, h->nx, h->nu, h->d_umin, h->d_umax, h->sp, mode, crec);
      return 0;
    });
  return with_int<1, 2>(w.nt, [&](auto nt) { return with_int<1, 2>(w.mt, [&](auto mt) { return with_bool(w.full, [&](auto full) {
    return with_bool(w.lqf, [&](auto lqf) { return with_bool(w.regv, [&](auto regv) { return with_bool(w.f32, [&](auto f32) {
      constexpr int NT = decltype(nt)::value, MT = decltype(mt)::value;
      constexpr bool FULL = decltype(full)::value, LQF = decltype(lqf)::value, REGV = decltype(regv)::value, F32 = decltype(f32)::value;
      if constexpr ((FULL && NT != 2) || (REGV && (FULL || LQF)) || (MT == 2 && (FULL || LQF || REGV || F32))) {
        return fail(ILQR_ERR_STATE, "k_backward_w3<%d, %d, %d, %d, %d, %s> is not built", NT, FULL, LQF, REGV, MT, F32 ? "float" : "double");
      } else {
        using S = std::conditional_t<F32, float, double>;
        hipLaunchKernelGGL((k_backward_w3<NT, FULL, LQF, REGV, MT, S>), grid, block, 0, h->stream, view_of<S>(h), h->nx, h->nu, h->d_umin, h->d_umax,
                           h->sp, mode, crec);
        return 0;
      }
    }); }); });
  }); }); });
}

static int launch_backward(ilqr_batch* h, int mode) {
  if (!h->aos)
    if (int rc = materialise_records(h)) return rc;
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (int rc = timer_begin(h, ILQR_STAGE_BACKWARD, &ev)) return rc;
  const Backward route = h->plan.backward;
  if (route != Backward::quad && route != Backward::thread) {
    // the register-resident kernels, two (nx > 16) or more (nx <= 16) wavefronts per SIMD: k_backward_w3, or with ILQR_ROUTE_BACKWARD_W2 the
    // literal-order k_backward_w2 (round 1's LDS kernel k_backward_w, whose bits k_backward_w2 reproduces, was retired in ABI 5)
    const bool fused = h->plan.derivatives == Derivatives::fused_lq && !h->lq_caller_records;  // cx, cu from the knot, the matrices from const_rec: D untouched
    if (!fused)
      if (int rc = ensure_records(h)) return rc;
    const double* crec = (fused || h->records_partial) ? h->const_rec : nullptr;
    if (int rc = launch_backward_w(h, backward_wave_variant(route, h->nx, h->nu, h->dtype, fused), route == Backward::w2, mode, crec)) return rc;
  } else if (int rc = with_model(h, [&](auto& v, auto& m, auto&) {
               using MM = std::decay_t<decltype(m)>;
               if (route == Backward::thread)
                 hipLaunchKernelGGL((k_backward_t<MM>), dim3(h->Bp / 64), dim3(64), 0, h->stream, v, m, h->sp, mode);
               else if constexpr (MM::NX == 4)  // one wavefront = one tile of 16 trajectories x 4 lanes
                 hipLaunchKernelGGL((k_backward_q<MM>), dim3(h->ntiles), dim3(64), 0, h->stream, v, m, h->sp, mode);
               return 0;
             }))
    return rc;
  HIPCHK(hipGetLastError());
  return timer_end(h, ILQR_STAGE_BACKWARD, ev);
}

constexpr int kRingKbTwoBlocks = 60;
static int launch_sweep_backward(ilqr_batch* h, int mode, int force) {
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (int rc = timer_begin(h, ILQR_STAGE_BACKWARD, &ev)) return rc;
  const int* ci = h->commit_pending ? h->commit_idx : nullptr;
  if (int rc = with_model(h, [&](auto& v, auto& m, auto& fdm) {
        using MM = std::decay_t<decltype(m)>;
        using MF = std::decay_t<decltype(fdm)>;
        if constexpr (MM::NX == 4)
          return with_bool(h->plan.sweep == Sweep::one_producer, [&](auto one) {
            constexpr int P = decltype(one)::value ? 1 : kProducers, KB = decltype(one)::value ? kRingKbTwoBlocks : ILQR_RING_KB;
            hipLaunchKernelGGL((k_sweep_backward<MM, P, KB, MF>), dim3(h->ntiles), dim3(64 * (1 + P)), 0, h->stream, v, m, fdm, h->sp, mode, force, ci);
            return 0;
          });
        return 0;
      }))
    return rc;
  HIPCHK(hipGetLastError());
  h->commit_pending = false;  // the producers performed the copy on the way (see launch_derivatives)
  h->recs = ilqr_batch::REC_STALE;  // the records lived in LDS only
  return timer_end(h, ILQR_STAGE_BACKWARD, ev);
}

// selection + lambda schedule + termination; the copy of the accepted candidate is left pending
// (fused into the next derivative sweep, or flushed by flush_commit)
static int launch_accept(ilqr_batch* h) {
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (int rc = timer_begin(h, ILQR_STAGE_ACCEPT, &ev)) return rc;
  if (int rc = launch_per_slot(h, k_accept<double>, h->v, h->sp, h->commit_idx)) return rc;
  h->commit_pending = true;
  return timer_end(h, ILQR_STAGE_ACCEPT, ev);
}

// Whole iterations per tile in one persistent kernel (plan.solve: k_solve_hex / _tile / _wide / _wide2).
static int launch_solve_tiles(ilqr_batch* h, int n_iters) {
  std::pair<hipEvent_t, hipEvent_t> ev;
  HIPCHK(hipMemsetAsync(h->v.n_running, 0, sizeof(int), h->stream));
  if (int rc = timer_begin(h, ILQR_STAGE_SOLVE, &ev)) return rc;
  const AlphaSet al = line_search_alphas();
  const int pending = h->commit_pending ? 1 : 0;
  long long* ticks = h->profile ? h->phase_ticks : nullptr;
  const Solve solve = h->plan.solve;
  const int grid_tiles = (h->active_tiles > 0 && h->active_tiles < h->ntiles) ? h->active_tiles : h->ntiles;  // (the rest hold finished trajectories only)
  if (int rc = with_model(h, [&](auto& v, auto& m, auto& fdm) {
        using MM = std::decay_t<decltype(m)>;
        using MF = std::decay_t<decltype(fdm)>;
        if constexpr (MM::NX != 4) {
          return fail(ILQR_ERR_STATE, "persistent tiles are nx = 4 kernels");
        } else {
          auto solve_with = [&](auto kernel, int blocks, int threads) {
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, h->stream, v, m, fdm, al, h->sp, n_iters, h->sp.fixed_work, h->commit_idx, pending, ticks);
          };
          const int wide_blocks = (grid_tiles + 3) / 4;  // (wide tiles: one per CU while they fit, else two -- or as ILQR_ROUTE_WIDE_ONE/TWO_PER_CU says)
          const bool wide_one = h->route.wide_occ == 1 || (h->route.wide_occ == 0 && wide_blocks <= h->num_cus);
          switch (solve) {
            case Solve::wide: if constexpr (MM::NU == 1) { if (wide_one) solve_with(k_solve_wide<MM, MF, 1>, wide_blocks, 512); else solve_with(k_solve_wide<MM, MF, 2>, wide_blocks, 256); } break;
            case Solve::wide2: if constexpr (MM::NU == 2) solve_with(k_solve_wide2<MM, MF>, wide_blocks, 256); break;
            case Solve::hex: if constexpr (MM::NU == 1) solve_with(k_solve_hex<MM, MF>, grid_tiles, 512); break;
            case Solve::tile1: solve_with(k_solve_tile<MM, MF, 1>, grid_tiles, 256); break;
            case Solve::tile2: solve_with(k_solve_tile<MM, MF, 2>, grid_tiles, 256); break;
            case Solve::none: break;
          }
        }
        return 0;
      }))
    return rc;
  HIPCHK(hipGetLastError());
  h->commit_pending = (solve != Solve::hex);   // the last iteration's accepts (flushed by the caller); k_solve_hex commits every iteration's itself
  if (h->cands != Cands::none)  // (what ilqr_get_candidate finds in the buffers)
    h->cands = (solve == Solve::hex && kHexCandT) ? Cands::grouped : Cands::planes;
  h->recs = ilqr_batch::REC_STALE;
  return timer_end(h, ILQR_STAGE_SOLVE, ev);
}

// launch(&kernel) of a stored-model query (the launch_* below) for the entry point `who`: a launch that was itself refused says which kernel
template <class L>
static int run_launch(const char* who, L&& launch) {
  const char* kernel = "";
  const int rc = launch(&kernel);
  if (rc != ILQR_ERR_HIP) return rc;
  char keep[sizeof(g_err)];
  memcpy(keep, g_err, sizeof(keep));
  return fail(rc, "%s: %s: %.400s", who, kernel, keep);
}
// f(nt, mt, S()) for the instantiation of a stored-model query's wavefront-per-trajectory kernel that a generic handle of these sizes runs
// (value_wave_variant: nt state tiles, mt control tiles, storage type S).  The `if constexpr` is the build list of every such kernel.
template <class F>
static int with_wave_tiles(ilqr_batch* h, const char* kernel_name, F&& f) {
  const WaveVariant w = value_wave_variant(h->nx, h->nu, h->dtype);
  return with_int<1, 2>(w.nt, [&](auto nt) { return with_int<1, 2>(w.mt, [&](auto mt) { return with_bool(w.f32, [&](auto f32) {
    if constexpr (decltype(mt)::value == 2 && decltype(f32)::value) {  // float storage: never with two control tiles (ilqr_create)
      return fail(ILQR_ERR_UNSUPPORTED, "%s: no fp32 handle has more than %d controls", kernel_name, WM);
    } else {
      return f(nt, mt, std::conditional_t<decltype(f32)::value, float, double>());
    }
  }); }); });
}

// The value model of the stored policy (ilqr_get_value / ilqr_copy_value_to_device; value_wave.hpp, value_thread.hpp): picked by the
// handle's layout and sizes alone -- no route bit, no stage timer.  The caller has materialised the records.  Vx [B][nk][nx], Vxx
// [B][nk][nx * nx]: canonical double in device memory, either may be null.
// `name`: the kernel, for the caller's message should the launch itself be refused (route.hpp: value_kernel_name)
static int launch_value(ilqr_batch* h, int t0, int nk, double* Vx, double* Vxx, const char** name) {
  const WaveVariant w = value_wave_variant(h->nx, h->nu, h->dtype);
  *name = value_kernel_name(h->aos, w);
  if (!h->aos) {
    const dim3 grid(h->Bp / 64), block(64);
    if (int rc = with_model(h, [&](auto& v, auto& m, auto&) {
          hipLaunchKernelGGL((k_value_t<std::decay_t<decltype(m)>>), grid, block, 0, h->stream, v, t0, nk, Vx, Vxx);
          return 0;
        }))
      return rc;
  } else if (int rc = with_wave_tiles(h, *name, [&](auto nt, auto mt, auto s) {
               using S = decltype(s);
               hipLaunchKernelGGL((k_value_w<decltype(nt)::value, decltype(mt)::value, S>), dim3(h->B), dim3(64), 0, h->stream, view_of<S>(h), h->nx, h->nu, t0, nk, Vx, Vxx);
               return 0;
             }))
    return rc;
  HIPCHK(hipGetLastError());
  return 0;
}

// The closed-loop covariance of the stored policy (ilqr_get_covariance / ilqr_copy_covariance_to_device; covariance_wave.hpp,
// covariance_thread.hpp): as launch_value, picked by the handle's layout and sizes alone -- no route bit, no stage timer.  The caller
// has materialised the records and checked the window.
static int launch_covariance(ilqr_batch* h, const CovArgs& q, const char** name) {
  const WaveVariant w = value_wave_variant(h->nx, h->nu, h->dtype);
  *name = covariance_kernel_name(h->aos, w);
  if (!h->aos) {
    const dim3 grid(h->Bp / 64), block(64);
    if (int rc = with_model(h, [&](auto& v, auto& m, auto&) {
          hipLaunchKernelGGL((k_covariance_t<std::decay_t<decltype(m)>>), grid, block, 0, h->stream, v, q);
          return 0;
        }))
      return rc;
  } else if (int rc = with_wave_tiles(h, *name, [&](auto nt, auto mt, auto s) {
               using S = decltype(s);
               hipLaunchKernelGGL((k_covariance_w<decltype(nt)::value, decltype(mt)::value, S>), dim3(h->B), dim3(64), 0, h->stream, view_of<S>(h), h->nx, h->nu, q);
               return 0;
             }))
    return rc;
  HIPCHK(hipGetLastError());
  return 0;
}

// The tangent and the adjoint of the stored closed loop (ilqr_get_tangent / ilqr_get_adjoint and their device forms; sensitivity_wave.hpp,
// sensitivity_thread.hpp): as launch_covariance, picked by the handle's layout and sizes alone -- no route bit, no stage timer.  The
// caller has materialised the records, checked the window and that B * n_dirs fits an int.  Generic layout: one wavefront per
// (trajectory, 16 directions); tiled layout: one thread per (trajectory, direction), the direction by block.
template <class Args, class Tiled, class Wave>
static int launch_sensitivity(ilqr_batch* h, const Args& q, const char* kernel_name, Tiled&& tiled, Wave&& wave) {
  if (!h->aos) {
    const dim3 grid((unsigned)(h->Bp / 64) * (unsigned)q.nd), block(64);
    if (int rc = with_model(h, [&](auto& v, auto& m, auto&) {
          tiled(v, m, grid, block);
          return 0;
        }))
      return rc;
  } else if (int rc = with_wave_tiles(h, kernel_name, [&](auto nt, auto mt, auto s) {
               wave(nt, mt, s, dim3((unsigned)h->B * (unsigned)((q.nd + 15) / 16)), dim3(64));
               return 0;
             }))
    return rc;
  HIPCHK(hipGetLastError());
  return 0;
}
static int launch_tangent(ilqr_batch* h, const TangentArgs& q, const char** name) {
  *name = tangent_kernel_name(h->aos, value_wave_variant(h->nx, h->nu, h->dtype));
  return launch_sensitivity(h, q, *name,
      [&](auto& v, auto& m, dim3 grid, dim3 block) { hipLaunchKernelGGL((k_tangent_t<std::decay_t<decltype(m)>>), grid, block, 0, h->stream, v, q); },
      [&](auto nt, auto mt, auto s, dim3 grid, dim3 block) {
        using S = decltype(s);
        hipLaunchKernelGGL((k_tangent_w<decltype(nt)::value, decltype(mt)::value, S>), grid, block, 0, h->stream, view_of<S>(h), h->nx, h->nu, q);
      });
}
static int launch_adjoint(ilqr_batch* h, const AdjointArgs& q, const char** name) {
  *name = adjoint_kernel_name(h->aos, value_wave_variant(h->nx, h->nu, h->dtype));
  return launch_sensitivity(h, q, *name,
      [&](auto& v, auto& m, dim3 grid, dim3 block) { hipLaunchKernelGGL((k_adjoint_t<std::decay_t<decltype(m)>>), grid, block, 0, h->stream, v, q); },
      [&](auto nt, auto mt, auto s, dim3 grid, dim3 block) {
        using S = decltype(s);
        hipLaunchKernelGGL((k_adjoint_w<decltype(nt)::value, decltype(mt)::value, S>), grid, block, 0, h->stream, view_of<S>(h), h->nx, h->nu, q);
      });
}

// The LQ subproblem of the records solved for the caller's linear terms (ilqr_solve_lq / _on_device; lq_solve_wave.hpp, lq_solve_thread.hpp):
// as launch_sensitivity, picked by the handle's layout and sizes alone.  The caller has materialised the records, sized the scratch and
// checked that B * n_dirs fits an int.  Generic layout: the gain sweep, one wavefront per trajectory, then the two direction sweeps, one
// wavefront per (trajectory, 16 directions); tiled layout: one thread per trajectory, then one per (trajectory, direction).
static int launch_lq_solve(ilqr_batch* h, const LqArgs& q, const char** name) {
  const WaveVariant w = value_wave_variant(h->nx, h->nu, h->dtype);
  *name = lq_solve_kernel_name(h->aos, w);
  if (!h->aos) {
    const dim3 block(64), per_traj((unsigned)(h->Bp / 64)), per_dir((unsigned)(h->Bp / 64) * (unsigned)q.nd);
    if (int rc = with_model(h, [&](auto& v, auto& m, auto&) {
          using Mdl = std::decay_t<decltype(m)>;
          hipLaunchKernelGGL((k_lq_gain_t<Mdl>), per_traj, block, 0, h->stream, v, q);
          hipLaunchKernelGGL((k_lq_dir_t<Mdl>), per_dir, block, 0, h->stream, v, q);
          return 0;
        }))
      return rc;
  } else if (int rc = with_wave_tiles(h, *name, [&](auto nt, auto mt, auto s) {
               constexpr int NT = decltype(nt)::value, MT = decltype(mt)::value;
               using S = decltype(s);
               const dim3 block(64), per_traj((unsigned)h->B), per_tile((unsigned)h->B * (unsigned)((q.nd + 15) / 16));
               hipLaunchKernelGGL((k_lq_gain_w<NT, MT, S>), per_traj, block, 0, h->stream, view_of<S>(h), h->nx, h->nu, q);
               hipLaunchKernelGGL((k_lq_back_w<NT, MT, S>), per_tile, block, 0, h->stream, view_of<S>(h), h->nx, h->nu, q);
               hipLaunchKernelGGL((k_lq_fwd_w<NT, MT, S>), per_tile, block, 0, h->stream, view_of<S>(h), h->nx, h->nu, q);
               return 0;
             }))
    return rc;
  HIPCHK(hipGetLastError());
  return 0;
}

// The Kalman filter of the stored linearisation and the covariance of the output-feedback loop (ilqr_get_estimator /
// ilqr_copy_estimator_to_device; estimator_wave.hpp, estimator_thread.hpp): as launch_covariance, picked by the handle's layout and sizes
// alone.  The caller has materialised the records, checked ny and the window and sized the scratch.  Generic layout: the filter sweep by
// (state tiles, output tiles), then -- if Sigma, Su or the expected cost is asked for -- the loop sweep by (state tiles, control tiles),
// one wavefront per trajectory each; tiled layout: one kernel, one thread per trajectory.
static int launch_estimator(ilqr_batch* h, const EstArgs& q, const char** name) {
  const WaveVariant w = value_wave_variant(h->nx, h->nu, h->dtype);
  const int yt = q.ny > 16 ? 2 : 1;
  *name = estimator_kernel_name(h->aos, w.nt, yt);
  if (!h->aos) {
    const dim3 grid(h->Bp / 64), block(64);
    if (int rc = with_model(h, [&](auto& v, auto& m, auto&) {
          hipLaunchKernelGGL((k_estimator_t<std::decay_t<decltype(m)>>), grid, block, 0, h->stream, v, q);
          return 0;
        }))
      return rc;
    HIPCHK(hipGetLastError());
    return 0;
  }
  if (int rc = with_int<1, 2>(w.nt, [&](auto nt) { return with_int<1, 2>(yt, [&](auto ytc) { return with_bool(w.f32, [&](auto f32) {
        constexpr int NT = decltype(nt)::value, YT = decltype(ytc)::value;
        using S = std::conditional_t<decltype(f32)::value, float, double>;
        if constexpr (YT > NT) {  // (ny <= nx: the caller has checked)
          return fail(ILQR_ERR_INVALID, "%s: ny %d beyond nx %d", *name, q.ny, h->nx);
        } else {
          hipLaunchKernelGGL((k_est_filter_w<NT, YT, S>), dim3(h->B), dim3(64), 0, h->stream, view_of<S>(h), h->nx, h->nu, q);
          return 0;
        }
      }); }); }))
    return rc;
  HIPCHK(hipGetLastError());
  if (!est_closed(q)) return 0;
  *name = estimator_loop_kernel_name(w);
  if (int rc = with_wave_tiles(h, *name, [&](auto nt, auto mt, auto s) {
        using S = decltype(s);
        hipLaunchKernelGGL((k_est_loop_w<decltype(nt)::value, decltype(mt)::value, S>), dim3(h->B), dim3(64), 0, h->stream, view_of<S>(h), h->nx, h->nu, q);
        return 0;
      }))
    return rc;
  HIPCHK(hipGetLastError());
  return 0;
}

// The risk-sensitive gains and value of the records' LQ model (ilqr_get_risk_sensitive / ilqr_copy_risk_sensitive_to_device; risk_wave.hpp,
// risk_thread.hpp): as launch_estimator, picked by the handle's layout and sizes alone.  The caller has materialised the records and
// checked nw.  Generic layout: one wavefront per trajectory, by (state tiles, control tiles, noise tiles); tiled layout: one thread per
// trajectory.
static int launch_risk(ilqr_batch* h, const RiskArgs& q, const char** name) {
  const WaveVariant w = value_wave_variant(h->nx, h->nu, h->dtype);
  const int wt = q.nw > 16 ? 2 : 1;
  *name = risk_kernel_name(h->aos, w, wt);
  if (!h->aos) {
    const dim3 grid(h->Bp / 64), block(64);
    if (int rc = with_model(h, [&](auto& v, auto& m, auto&) {
          hipLaunchKernelGGL((k_risk_t<std::decay_t<decltype(m)>>), grid, block, 0, h->stream, v, q);
          return 0;
        }))
      return rc;
  } else if (wt > w.nt) {  // (nw <= nx: the caller has checked)
    return fail(ILQR_ERR_INVALID, "%s: nw %d beyond nx %d", *name, q.nw, h->nx);
  } else if (int rc = with_wave_tiles(h, *name, [&](auto nt, auto mt, auto s) { return with_int<1, 2>(wt, [&](auto wtc) {
               constexpr int NT = decltype(nt)::value, MT = decltype(mt)::value, WT = decltype(wtc)::value;
               using S = decltype(s);
               if constexpr (WT <= NT)  // (more noise tiles than state tiles: refused above, never built)
                 hipLaunchKernelGGL((k_risk_w<NT, MT, WT, S>), dim3(h->B), dim3(64), 0, h->stream, view_of<S>(h), h->nx, h->nu, q);
               return 0;
             }); }))
    return rc;
  HIPCHK(hipGetLastError());
  return 0;
}

// The stored policy applied to caller-given states (ilqr_evaluate_policy / _on_device; evaluate.hpp): picked by the handle's layout alone,
// as launch_value -- no route bit, no stage timer.  One thread per rollout, B * S of them (the caller has checked that they fit an int).
static int launch_evaluate(ilqr_batch* h, const EvalArgs& e, const char** name) {
  const dim3 grid((unsigned)(((size_t)h->B * e.S + 63) / 64)), block(64);
  if (!h->aos)
    return with_model(h, [&](auto& v, auto& m, auto&) {
      *name = evaluate_kernel_name(false, ModelRows::none);
      hipLaunchKernelGGL((k_evaluate_t<std::decay_t<decltype(m)>>), grid, block, 0, h->stream, v, m, e);
      HIPCHK(hipGetLastError());
      return 0;
    });
  return with_rollout_model(h, [&](auto& m) { return with_trajectory_params(h, m, [&](const auto& pm, auto pt) {
    using M = std::decay_t<decltype(m)>;
    *name = evaluate_kernel_name(true, (ModelRows) decltype(pt)::value);
    hipLaunchKernelGGL((k_evaluate_g<M, decltype(pt)::value>), grid, block, 0, h->stream, view_of<typename M::real>(h), pm, e);
    HIPCHK(hipGetLastError());
    return 0;
  }); });
}

// The gradient with respect to the per-trajectory parameters (ilqr_get_param_gradient / _on_device; param_gradient.hpp): the costate
// sweep, then -- when gp is asked for -- the contraction and the reduction of its partials.  The kernels exist only in a build whose twin
// has NTP; the caller has refused every other handle (check_trajectory_params), carved the scratch and checked that the sizes fit an int.
static int launch_param_gradient(ilqr_batch* h, const PgArgs& a, const char** name) {
  *name = param_gradient_kernel_name(h->dtype);
#ifdef ILQR_HAVE_USER_MODEL
  if constexpr (kUserGeneric && kUserNTP > 0) {
    using M = std::decay_t<decltype(h->user_g)>;
    const unsigned ngroup = (unsigned)((a.nd + pg_shape(kUserNTP).dirs - 1) / pg_shape(kUserNTP).dirs);
    if (int rc = with_view(h, [&](auto& v) {
          using S = std::remove_pointer_t<decltype(v.D)>;
          hipLaunchKernelGGL((k_pg_costate<S, M::NX, M::NU>), dim3(h->B), dim3(64), 0, h->stream, v, a.lam);
          if (!a.gp) return 0;
          hipLaunchKernelGGL((k_pg_contract<M, S>), dim3((unsigned)h->B * (unsigned)a.nchunk * ngroup), dim3(64), 0, h->stream, v,
                             per_trajectory(h, h->user_g), a);
          hipLaunchKernelGGL((k_pg_reduce<kUserNTP>), dim3((unsigned)(((size_t)h->B * a.nd * kUserNTP + 255) / 256)), dim3(256), 0, h->stream, h->B, a);
          return 0;
        }))
      return rc;
    HIPCHK(hipGetLastError());
    return 0;
  }
#endif
  return fail(ILQR_ERR_UNSUPPORTED, "%s: this build's user model declares no per-trajectory parameters", *name);
}

static AlphaSet line_search_alphas() {
  AlphaSet a;
  for (int i = 0; i < NALPHA; i++) a.a[i] = kAlphaHost[i];
  return a;
}

static int do_rollout_candidates(ilqr_batch* h, int mode) {
  if (int rc = launch_rollout(h, true, true, line_search_alphas(), NALPHA, h->v.cost_c, mode)) return rc;
  h->cands = Cands::planes;
  return 0;
}

