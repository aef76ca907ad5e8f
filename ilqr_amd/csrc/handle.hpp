// handle.hpp -- the opaque handle behind the C ABI (ilqr_batch: device memory of one batch, its stream, its route choices, its stage
// timers) and the helpers every entry point uses: error plumbing, allocation, host <-> device layout conversion, the record
// array's states.  Included once, by capi.hip.
#pragma once
// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
#define HIPCHK(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(ILQR_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
#define REQUIRE(cond, ...)                              \
  do {                                                  \
    if (!(cond)) return fail(ILQR_ERR_INVALID, __VA_ARGS__); \
  } while (0)

// ------------------------------------------------------------------------------------------
// the handle
// ------------------------------------------------------------------------------------------
struct StageTimer {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;  // (begin, end); an event may end one stage and begin the next
  double ms = 0;
  int launches = 0;
};

enum class Cands { none, planes, grouped };  // what the candidate buffers hold (ilqr_batch::cands)

struct ilqr_batch {
  int model, nx, nu, T, B, Bp, ntiles, device, flags;
  int dtype = ILQR_DTYPE_F64;   // storage and rollout arithmetic (ilqr_desc.dtype)
  double dt;
  ilqr_params params;
  // fp64 handle: its models.  fp32 handle: the double-precision TWINS the finite differences are taken in
  // (kernels.hpp, derivatives_of_knot), built from the float models' own parameter values
  AcrobotModel acrobot;
  DoubleIntegratorModel dint;
  AcrobotModelT<float> acrobot_f;          // fp32 handle: what the rollouts integrate
  DoubleIntegratorModelT<float> dint_f;
  LqModel lq;                   // ILQR_MODEL_LQ: padded matrices on the device (fp32 handle: the float-rounded matrices, for the finite differences and the backward pass)
  LqModelT<float> lq_f;         // ... fp32 handle: the float matrices its rollouts integrate
  LqModelW lq_w;                // ... with 16 < nu <= 32 (lq_wide): B and R padded to 32 columns, the generic kernels only
  bool lq_wide = false;
#ifdef ILQR_HAVE_USER_MODEL
  UserModelT<double> user;      // ILQR_MODEL_USER: the build's user device twin (fp32 handle: the twin the finite differences are taken in)
  GenericModelOf<UserModelT<double>> user_g;  // ... as the generic kernels take it (any NX <= 32, NU <= 16 that is not a tiled nx = 4 shape)
  UserModelT<float> user_f;
  GenericModelOf<UserModelT<float>> user_gf;  // fp32 handle on the generic layout: what k_rollout_g integrates
#endif
  // per-trajectory model parameters (ilqr_set_trajectory_params): canonical double [B][NTP], allocated on first use; plan.traj_params says
  // whether the kernels read them.  Row b is the trajectory in slot b: the generic path never re-packs trajectories (ilqr_generate_trajectory
  // compacts on the persistent routes only) -- whoever brings compaction to this path must move these rows with the trajectories.
  double* traj_params = nullptr;
  // per-knot model parameters (ilqr_set_knot_params): the handle's own window [B][T+1][NTP] of the caller's reference, canonical double,
  // allocated on first use and kept; read while plan.traj_params is per_knot.  knot_stage: a host reference on its way through the gather
  // kernel, [B][n_knots][NTP], allocated by the first host call, kept while the next call's fits (ensure_knot_stage), freed with the handle
  double* knot_params = nullptr;
  double* knot_stage = nullptr;
  size_t knot_stage_elems = 0;
  // single trajectories starting over on the device (reset.hpp; ilqr_reset_trajectories, ilqr_mpc_step_reset): allocated by the first call
  // that needs them (dev_alloc: freed with the handle), nothing per call afterwards
  int* reset_ints = nullptr;         // [3][Bp]: a host mask's copy, the selection of the pass under way, the flags of the last call
  double* reset_us = nullptr;        // the reset controls, in the layout and storage type of us; read while reset_us_set (else: zeros)
  double* reset_us_stage = nullptr;  // canonical [B][T][nu]: a host u0 on its way into that layout (handles that convert)
  bool reset_us_set = false;
  bool reset_flags_valid = false;    // one of the two calls has run: the flags describe it
  // multi-start groups (clone.hpp; ilqr_select_best, ilqr_clone_trajectories, ilqr_clone_best): allocated by the first call that needs them
  int* clone_ints = nullptr;         // [3][Bp]: the map (a host map's copy, or the handle's own best-of-group map), the sources of the call under way, the flags of the last call
  bool clone_flags_valid = false;    // a clone call has run: the flags describe it
  // ilqr_solve_lq's call-sized scratch (lq_solve_wave.hpp: Kd, Mi, P, kd, the failure marks): allocated by the first call, kept while the
  // next call's fits (ensure_lq_scratch), freed with the handle
  double* lq_scratch = nullptr;
  size_t lq_scratch_elems = 0;
  // ilqr_get_estimator's call-sized scratch (estimator_wave.hpp: the failure marks, Pf and N of every knot on the generic layout): as
  // lq_scratch, allocated by the first call, kept while the next call's fits (ensure_est_scratch), freed with the handle
  double* est_scratch = nullptr;
  size_t est_scratch_elems = 0;
  // ilqr_get_risk_sensitive's scratch (risk_wave.hpp: the failure marks, [B]): allocated by the first call (dev_alloc: freed with the handle)
  int* risk_fail = nullptr;
  // ilqr_get_param_gradient's call-sized scratch (param_gradient.hpp: the costate when the caller takes none, the chunks' partials): as
  // lq_scratch, allocated by the first call, kept while the next call's fits (ensure_pg_scratch), freed with the handle
  double* pg_scratch = nullptr;
  size_t pg_scratch_elems = 0;
  // v is the view every entry point addresses arrays through; for an fp32 handle its trajectory pointers hold
  // the addresses of FLOAT arrays (never dereferenced as double: kernels get vf, the same addresses typed float*)
  BatchView v;
  BatchViewT<float> vf;
  SolverParams sp;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int* commit_idx = nullptr;
  long long* phase_ticks = nullptr;  // [ntiles][5] per-tile clocks of k_solve_tile: sweep+backward, rollouts+accept, iterations, shader cycles, wall ticks
  double wall_clock_khz = 100000.0;
  double* staging = nullptr;  // device scratch for canonical <-> tiled conversion and for the host getters' arrays (staging.hpp)
  double* x0_stage = nullptr;  // [B][nx] canonical: a host x0 of ilqr_mpc_step on its way to the device layout (never reallocated, never waited for)
  // LQ model with exact derivatives: the sweep writes one copy of the constant matrices (const_rec) and
  // per knot only cx, cu; records_partial says that D holds no matrices for t < T right now
  double* const_rec = nullptr;   // [2][REC]: the constant blocks of every knot t < T, then knot T's record
  bool records_partial = false;
  // ... on the fused LQ route (plan.derivatives == Derivatives::fused_lq) no sweep runs at all: the backward pass forms cx = cxx x_t, cu = cuu u_t
  // from the knot, and the record array D is allocated only if somebody asks for records (getters, ilqr_set_derivatives)
  bool lq_fused_stale = false;    // fused iterations have run since D was last written: a getter gets the records of the current nominal computed
  bool lq_caller_records = false; // ilqr_set_derivatives replaced the model's blocks: the next backward pass reads D, not the model
  // nx = 4 device models: D (0.75 GB per 4096 acrobot trajectories) is allocated the first time somebody wants
  // records in HBM -- the stage calls, the two-kernel route, the getters.  ilqr_iterate's fused kernel keeps them
  // in LDS (kernels.hpp) and leaves D as it was: recs says what D holds.
  //   REC_ZERO  what init_traj leaves (ilqr_core.cpp:39-45): zeros        REC_VALID  the records of the nominal
  //   REC_STALE iterations have run since: whoever asks gets them computed from the current nominal
  enum { REC_ZERO, REC_VALID, REC_STALE } recs = REC_ZERO;
  size_t staging_elems = 0;
  std::vector<void*> allocs;
  bool initialised = false;  // init_traj / set_trajectory has run
  bool commit_pending = false;  // an accepted candidate is not yet copied into xs/us
  bool lq_cands_kept = false;   // LQ model: the last search rollout (k_rollout_lq<RG_SEARCH>) stored its candidates in v.cand_x / v.cand_u
  // cand_u / cand_x / cost_c hold, slot for slot, the last rollouts of the trajectories now in those slots (none: they belong to nobody --
  // compaction, ilqr_generate_trajectory, moves trajectories without moving their candidates), one alpha plane after the other or in
  // k_solve_hex's grouped layout (rollout.hpp: CANDT).  k_commit and k_derivatives' fused commit read planes only.
  Cands cands = Cands::none;
  bool aos = false;             // host-model / generic handles: trajectory-contiguous layout, wave-per-trajectory backward
  double* d_umin = nullptr;     // [nu] device copies of the limits (generic kernel)
  double* d_umax = nullptr;
  bool profile = false;
  int num_cus = 256;
  // full solves of batches with more tiles than CUs: running trajectories are re-packed into the leading tiles between
  // chunks of iterations (ilqr_generate_trajectory); active_tiles = how many tiles the persistent kernel is launched for
  int active_tiles = 0;
  int* d_perm = nullptr;       // [Bp]
  void* perm_scratch = nullptr;  // as large as the largest per-knot array
  size_t perm_scratch_bytes = 0;
  // The kernels of every stage (route.hpp), fixed at ilqr_create -- a handle never changes kernels between calls, and nothing is read
  // from the environment -- and the ilqr_desc.route knobs the launchers pass on
  RoutePlan plan;
  struct {
    bool full_records = false, no_compaction = false;
    int wide_occ = 0;  // wide tiles per CU: 0 = by the active tile count
  } route;
  StageTimer timers[ILQR_NUM_STAGES];
  std::vector<hipEvent_t> event_pool;
  // inside ilqr_iterate nothing is enqueued between the end of one stage and the begin of the next: the
  // end event serves as the next begin (one event record per kernel boundary instead of two; the
  // records cost ~2.5 us each on the queue)
  bool chain_timers = false;
  hipEvent_t chain_event = nullptr;
};

static int* reset_mask_stage(ilqr_batch* h) { return h->reset_ints; }  // the three rows of reset_ints
static int* reset_sel(ilqr_batch* h) { return h->reset_ints + h->Bp; }
static int* reset_flags(ilqr_batch* h) { return h->reset_ints + 2 * (size_t)h->Bp; }
static int* clone_map(ilqr_batch* h) { return h->clone_ints; }  // the three rows of clone_ints
static int* clone_sel(ilqr_batch* h) { return h->clone_ints + h->Bp; }
static int* clone_flags(ilqr_batch* h) { return h->clone_ints + 2 * (size_t)h->Bp; }
static int rec_of(const ilqr_batch* h) { return rec_size(h->nx, h->nu); }
static size_t elem_size(const ilqr_batch* h) { return h->dtype == ILQR_DTYPE_F32 ? sizeof(float) : sizeof(double); }
// the float view of an fp32 handle: same addresses as v, typed
static void sync_float_view(ilqr_batch* h) {
  const BatchView& v = h->v;
  BatchViewT<float>& f = h->vf;
  f.B = v.B; f.Bp = v.Bp; f.ntiles = v.ntiles; f.T = v.T; f.dt = v.dt;
  f.x0 = (float*)v.x0; f.xs = (float*)v.xs; f.us = (float*)v.us; f.kff = (float*)v.kff; f.Kfb = (float*)v.Kfb;
  f.D = (float*)v.D; f.cand_u = (float*)v.cand_u; f.cand_x = (float*)v.cand_x; f.nch = v.nch;
  f.cost_c = v.cost_c; f.cost = v.cost; f.lambda = v.lambda; f.dlambda = v.dlambda; f.dV = v.dV; f.gnorm = v.gnorm;
  f.status = v.status; f.iters = v.iters; f.flg_change = v.flg_change; f.alpha_idx = v.alpha_idx; f.diverge = v.diverge;
  f.backpass_done = v.backpass_done; f.n_running = v.n_running; f.analytic = v.analytic;
}
// f(real()) with the handle's storage type, float or double: where a handle's dtype picks between two instantiations of the same code
template <class F>
static int with_real(ilqr_batch* h, F&& f) {
  if (h->dtype == ILQR_DTYPE_F32) return f(float());
  return f(double());
}
// the handle's view typed by a storage type, h->v (double) or h->vf (float), and f(view) with the handle's own
template <class R>
static const BatchViewT<R>& view_of(const ilqr_batch* h) {
  if constexpr (std::is_same<R, float>::value) return h->vf; else return h->v;
}
template <class F>
static int with_view(ilqr_batch* h, F&& f) {
  return with_real(h, [&](auto r) { return f(view_of<decltype(r)>(h)); });
}
// f(std::bool_constant<b>()): a launch-time bool as a template argument
template <class F>
static int with_bool(bool b, F&& f) {
  return b ? f(std::true_type()) : f(std::false_type());
}
// f(std::integral_constant<int, I>()) for the I of Is... that i equals: a launch-time int as a template argument
template <int... Is, class F>
static int with_int(int i, F&& f) {
  int rc = 0;
  const bool found = ((i == Is && ((rc = f(std::integral_constant<int, Is>())), true)) || ...);
  return found ? rc : fail(ILQR_ERR_STATE, "no kernel is built for the value %d of a launch-time switch", i);
}
// f(view, model, model the finite differences are taken in) for the handle's device model and arithmetic
template <class F>
static int with_model(ilqr_batch* h, F&& f) {
  if (h->dtype == ILQR_DTYPE_F32) {
    switch (h->model) {
      case ILQR_MODEL_ACROBOT: return f(h->vf, h->acrobot_f, h->acrobot);
      case ILQR_MODEL_DOUBLE_INTEGRATOR: return f(h->vf, h->dint_f, h->dint);
#ifdef ILQR_HAVE_USER_MODEL
      case ILQR_MODEL_USER:
        if constexpr (kUserTiled) return f(h->vf, h->user_f, h->user);
        break;
#endif
      default: break;
    }
  } else {
    switch (h->model) {
      case ILQR_MODEL_ACROBOT: return f(h->v, h->acrobot, h->acrobot);
      case ILQR_MODEL_DOUBLE_INTEGRATOR: return f(h->v, h->dint, h->dint);
#ifdef ILQR_HAVE_USER_MODEL
      case ILQR_MODEL_USER:
        if constexpr (kUserTiled) return f(h->v, h->user, h->user);
        break;
#endif
      default: break;
    }
  }
  return fail(ILQR_ERR_UNSUPPORTED, "model %d has no device kernels of this kind", h->model);
}
// ILQR_MODEL_HOST: the model exists only as host code; nothing but the backward pass runs here
static bool host_model(const ilqr_batch* h) { return h->model == ILQR_MODEL_HOST; }
static int no_device_model();
// elements of a per-knot array with S time slots of E doubles, in this handle's device layout
static size_t dev_elems(const ilqr_batch* h, size_t S, size_t E) {
  return layout_elems(h->aos, h->B, h->ntiles, S, E);
}

template <class T>
static int dev_alloc(ilqr_batch* h, T** p, size_t n) {
  void* q = nullptr;
  HIPCHK(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
  HIPCHK(hipMemsetAsync(q, 0, std::max<size_t>(n, 1) * sizeof(T), h->stream));
  h->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}

// trajectory arrays: n elements of the handle's arithmetic (the pointer keeps the view's nominal double* type)
static int dev_alloc_real(ilqr_batch* h, double** p, size_t n) {
  void* q = nullptr;
  const size_t bytes = std::max<size_t>(n, 1) * elem_size(h);
  HIPCHK(hipMalloc(&q, bytes));
  HIPCHK(hipMemsetAsync(q, 0, bytes, h->stream));
  h->allocs.push_back(q);
  *p = (double*)q;
  return 0;
}

// an LQ model's pointers into a padded buffer [A | B | Q | R | Qf] (A, Q, Qf: GN x GN; B: GN x gm; R: gm x gm) and to the limits
template <class M, class Real>
static void bind_lq(M& m, const Real* pad, size_t gm, const ilqr_batch* h) {
  const size_t nA = (size_t)GN * GN, nB = GN * gm, nR = gm * gm;
  m.nx = h->nx; m.nu = h->nu; m.umin = h->d_umin; m.umax = h->d_umax;
  m.A = pad; m.Bm = pad + nA; m.Q = pad + nA + nB; m.R = pad + 2 * nA + nB; m.Qf = pad + 2 * nA + nB + nR;
}

static int grid_for(size_t n, int block) { return (int)std::min<size_t>((n + block - 1) / block, 65535u * 16u); }

static int no_device_model() {
  return fail(ILQR_ERR_UNSUPPORTED, "host-evaluated model: rollouts and finite differences stay on the host; only the backward pass (ilqr_set_derivatives + ilqr_backward_pass/_step) runs on the device");
}

// stage timing -------------------------------------------------------------------------------
static int timer_event(ilqr_batch* h, hipEvent_t* e) {
  if (!h->event_pool.empty()) {
    *e = h->event_pool.back();
    h->event_pool.pop_back();
    return 0;
  }
  HIPCHK(hipEventCreate(e));
  return 0;
}
static int timer_begin(ilqr_batch* h, int stage, std::pair<hipEvent_t, hipEvent_t>* ev) {
  if (!h->profile) return 0;
  (void)stage;
  if (h->chain_timers && h->chain_event) {
    ev->first = h->chain_event;
  } else {
    if (int rc = timer_event(h, &ev->first)) return rc;
    HIPCHK(hipEventRecord(ev->first, h->stream));
  }
  h->chain_event = nullptr;
  return timer_event(h, &ev->second);
}
static int timer_end(ilqr_batch* h, int stage, const std::pair<hipEvent_t, hipEvent_t>& ev) {
  if (!h->profile) return 0;
  HIPCHK(hipEventRecord(ev.second, h->stream));
  h->timers[stage].pending.push_back(ev);
  h->timers[stage].launches++;
  h->chain_event = h->chain_timers ? ev.second : nullptr;
  return 0;
}
static int timers_drain(ilqr_batch* h) {
  std::vector<hipEvent_t> used;
  for (int s = 0; s < ILQR_NUM_STAGES; s++) {
    StageTimer& t = h->timers[s];
    for (auto& ev : t.pending) {
      float ms = 0;
      HIPCHK(hipEventSynchronize(ev.second));
      HIPCHK(hipEventElapsedTime(&ms, ev.first, ev.second));
      t.ms += ms;
      used.push_back(ev.first);
      used.push_back(ev.second);
    }
    t.pending.clear();
  }
  std::sort(used.begin(), used.end());
  used.erase(std::unique(used.begin(), used.end()), used.end());
  h->event_pool.insert(h->event_pool.end(), used.begin(), used.end());
  h->chain_event = nullptr;
  return 0;
}

// host <-> device helpers -----------------------------------------------------------------------
static int ensure_staging(ilqr_batch* h, size_t elems) {
  if (elems <= h->staging_elems) return 0;
  if (h->staging) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipFree(h->staging));
    h->staging = nullptr;
    h->staging_elems = 0;
  }
  HIPCHK(hipMalloc((void**)&h->staging, elems * sizeof(double)));
  h->staging_elems = elems;
  return 0;
}
static int ensure_lq_scratch(ilqr_batch* h, size_t elems) {
  if (elems <= h->lq_scratch_elems) return 0;
  if (h->lq_scratch) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipFree(h->lq_scratch));
    h->lq_scratch = nullptr;
    h->lq_scratch_elems = 0;
  }
  HIPCHK(hipMalloc((void**)&h->lq_scratch, elems * sizeof(double)));
  h->lq_scratch_elems = elems;
  return 0;
}
static int ensure_est_scratch(ilqr_batch* h, size_t elems) {
  if (elems <= h->est_scratch_elems) return 0;
  if (h->est_scratch) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipFree(h->est_scratch));
    h->est_scratch = nullptr;
    h->est_scratch_elems = 0;
  }
  HIPCHK(hipMalloc((void**)&h->est_scratch, elems * sizeof(double)));
  h->est_scratch_elems = elems;
  return 0;
}
static int ensure_knot_stage(ilqr_batch* h, size_t elems) {
  if (elems <= h->knot_stage_elems) return 0;
  if (h->knot_stage) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipFree(h->knot_stage));
    h->knot_stage = nullptr;
    h->knot_stage_elems = 0;
  }
  HIPCHK(hipMalloc((void**)&h->knot_stage, elems * sizeof(double)));
  h->knot_stage_elems = elems;
  return 0;
}
static int ensure_pg_scratch(ilqr_batch* h, size_t elems) {
  if (elems <= h->pg_scratch_elems) return 0;
  if (h->pg_scratch) {
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipFree(h->pg_scratch));
    h->pg_scratch = nullptr;
    h->pg_scratch_elems = 0;
  }
  HIPCHK(hipMalloc((void**)&h->pg_scratch, elems * sizeof(double)));
  h->pg_scratch_elems = elems;
  return 0;
}
// A host getter's arrays (staging.hpp): room for the plan in the staging buffer, every segment's device pointer, the inputs on their way up ...
static int stage_up(ilqr_batch* h, StagePlan& p) {
  if (int rc = ensure_staging(h, p.total)) return rc;
  p.resolve(h->staging);
  for (int i = 0; i < p.n; i++)
    if (const StageSeg& s = p.seg[i]; s.up && s.host) HIPCHK(hipMemcpyAsync(s.dev, s.host, s.bytes(), hipMemcpyHostToDevice, h->stream));
  return 0;
}
// ... and, after the kernels, the outputs copied out and waited for
static int stage_down(ilqr_batch* h, const StagePlan& p) {
  for (int i = 0; i < p.n; i++)
    if (const StageSeg& s = p.seg[i]; !s.up && s.host) HIPCHK(hipMemcpyAsync(s.host, s.dev, s.bytes(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
static StageDims stage_dims(const ilqr_batch* h) { return {(size_t)h->B, (size_t)h->T, (size_t)h->nx, (size_t)h->nu, (size_t)kUserNTP}; }
// One of the handle's arrays as the conversions take it: S knots of E elements per trajectory, of which the knots [t0, t0 + n) are moved
// (n = 0: all S).  rec: not a plain array but the E elements from offset `off` of every knot's derivative record.
struct DevArray {
  void* p;
  int S, E;
  int t0 = 0, n = 0;
  bool rec = false;
  int off = 0;
};
static int knots(const DevArray& a) { return a.n ? a.n : a.S; }
static DevArray rec_block(const ilqr_batch* h, int off, int E) { return {h->v.D, h->T + 1, E, 0, 0, true, off}; }
// a generic fp64 handle stores a whole array as the canonical array itself: copied, never converted
static bool stored_canonical(const ilqr_batch* h, const DevArray& a) {
  return h->aos && elem_size(h) == sizeof(double) && !a.rec && knots(a) == a.S;
}
// f(index map of `a` in this handle's layout) (layout.hpp)
template <class F>
static int with_map(const ilqr_batch* h, const DevArray& a, F&& f) {
  if (h->aos) return f(AosMap{a.S, a.rec ? rec_of(h) : a.E, a.off, a.t0});
  if (a.rec) return f(TiledRecMap{a.S, rec_of(h), a.off, a.t0});
  return f(TiledMap{a.S, a.E, a.t0});
}
// handle's array -> canonical double [B][n][E] in device memory, and back.  Enqueued on the handle's stream: nothing is waited for,
// the staging buffer is not touched.
static int to_canonical(ilqr_batch* h, const DevArray& a, double* dst) {
  const int n = knots(a);
  const size_t total = (size_t)h->B * n * a.E;
  if (stored_canonical(h, a)) {
    HIPCHK(hipMemcpyAsync(dst, a.p, total * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return 0;
  }
  return with_real(h, [&](auto r) {
    return with_map(h, a, [&](auto map) {
      using real = decltype(r);
      hipLaunchKernelGGL((k_to_canonical<real, decltype(map)>), dim3(grid_for(total, 256)), dim3(256), 0, h->stream, (const real*)a.p, dst, map, h->B, n, a.E);
      HIPCHK(hipGetLastError());
      return 0;
    });
  });
}
static int from_canonical(ilqr_batch* h, const double* src, const DevArray& a) {
  const int n = knots(a);
  if (stored_canonical(h, a)) {
    if (src != a.p) HIPCHK(hipMemcpyAsync(a.p, src, (size_t)h->B * n * a.E * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return 0;
  }
  return with_real(h, [&](auto r) {
    return with_map(h, a, [&](auto map) {
      using real = decltype(r);
      const int groups = h->aos ? h->B : h->ntiles;
      const size_t total = (size_t)groups * n * a.E * map.LANES;
      hipLaunchKernelGGL((k_from_canonical<real, decltype(map)>), dim3(grid_for(total, 256)), dim3(256), 0, h->stream, src, (real*)a.p, map, h->B, groups, n, a.E);
      HIPCHK(hipGetLastError());
      return 0;
    });
  });
}
// canonical host array -> handle's array and back, waited for (the staging buffer is reused by the next call)
static int upload(ilqr_batch* h, const double* src, const DevArray& a) {
  const size_t bytes = (size_t)h->B * knots(a) * a.E * sizeof(double);
  double* dev = (double*)a.p;
  if (!stored_canonical(h, a)) {
    if (int rc = ensure_staging(h, bytes / sizeof(double))) return rc;
    dev = h->staging;
  }
  HIPCHK(hipMemcpyAsync(dev, src, bytes, hipMemcpyHostToDevice, h->stream));
  if (int rc = from_canonical(h, dev, a)) return rc;
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
static int download(ilqr_batch* h, const DevArray& a, double* dst) {
  const size_t bytes = (size_t)h->B * knots(a) * a.E * sizeof(double);
  const double* dev = (const double*)a.p;
  if (!stored_canonical(h, a)) {
    if (int rc = ensure_staging(h, bytes / sizeof(double))) return rc;
    if (int rc = to_canonical(h, a, h->staging)) return rc;
    dev = h->staging;
  }
  HIPCHK(hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
static int launch_derivatives(ilqr_batch* h, int force);
// the record array, allocated (zero-filled) on first use
static int ensure_records(ilqr_batch* h) {
  if (h->v.D) return 0;
  // (generic handles: on first use as well -- 44 GB at configs[4] in fp64, 22 GB in fp32)
  if (int rc = dev_alloc_real(h, &h->v.D, dev_elems(h, h->T + 1, rec_of(h)))) return rc;
  sync_float_view(h);
  return 0;
}
// D as the getters, the stage calls and ilqr_set_derivatives expect it.  LQ handles: fill in the constant
// matrices the partial sweep skipped.  nx = 4 handles: have the sweep compute the records of the current nominal
// trajectory if iterations have run since D was last written.
static int materialise_records(ilqr_batch* h) {
  if (int rc = ensure_records(h)) return rc;
  if (!h->aos) {
    if (h->recs == ilqr_batch::REC_STALE) return launch_derivatives(h, 1);
    return 0;
  }
  // the fused LQ route never wrote D: whole exact records of the current nominal, now (what = 0).  Else a partial sweep's records lack
  // the constant matrices (what = 2; never on an fp32 handle: its sweep writes whole records)
  const bool whole = h->lq_fused_stale;
  if (!whole && !h->records_partial) return 0;
  if (whole) h->lq_fused_stale = h->records_partial = false;
  const int nchunk = (h->T + 1 + kAnalyticChunk - 1) / kAnalyticChunk;
  with_view(h, [&](auto& v) {
    hipLaunchKernelGGL((k_analytic_lq<std::remove_pointer_t<decltype(v.D)>>), dim3(h->B * nchunk), dim3(64), 0, h->stream, v, h->lq, 1, whole ? 0 : 2, h->const_rec, kAnalyticChunk);
    return 0;
  });
  HIPCHK(hipGetLastError());
  return 0;
}
static int upload_rec(ilqr_batch* h, const double* src, int off, int E) {
  if (int rc = materialise_records(h)) return rc;
  h->records_partial = false;  // the caller's blocks replace the model's: every knot reads its own record again
  h->lq_caller_records = true;
  h->recs = ilqr_batch::REC_VALID;

  return upload(h, src, rec_block(h, off, E));
}
// per-trajectory scalar arrays [Bp] on device <-> [B] host
template <class T>
static int scalars_to_host(ilqr_batch* h, const T* dev, T* host) {
  HIPCHK(hipMemcpyAsync(host, dev, (size_t)h->B * sizeof(T), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
template <class T>
static int scalars_to_dev(ilqr_batch* h, const T* host, T* dev) {
  HIPCHK(hipMemcpyAsync(dev, host, (size_t)h->B * sizeof(T), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

