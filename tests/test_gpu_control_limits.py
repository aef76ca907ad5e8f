"""Per-control, asymmetric, pinned and unbounded control limits on every route.

The reference's Model takes any u_min / u_max vectors (include/model.h:17); its box-QP gets [u_min - us, u_max - us]
(src/ilqr_core.cpp:369) and its forward pass does not clamp, so in a real solve box edges sit exactly at 0, boxes exclude 0
and every control has a box of its own.  With one symmetric limit for all controls a kernel that reads u_min[0] for every
control, builds hi from -u_min or swaps two controls' limits leaves the same bits; these tests give every control its own
box and check, on every route:
  (a) every route leaves the bits of the two-kernel route (ILQR_FLAG_UNFUSED) -- kernel names asserted;
  (b) the two-kernel and the default route agree with the oracle built with the same limits (teacher-forced backward passes
      at lambda 1 and 1e-3, walked iterations: tests/parity.py);
  (c) invariants that need no oracle: k[t, j] in [fl(u_min[j] - us[t, j]), fl(u_max[j] - us[t, j])] for the us the pass saw (in the
      precision the kernels form the box in: float for fp32 handles), a pinned control's k exactly its box and its K row 0, and
      with ILQR_FLAG_REFERENCE_FIXES every committed control inside its own limits."""
import numpy as np
import pytest

from tests.util import acrobot_x0, integrator_x0, mat

pytestmark = pytest.mark.gpu
DT = 0.02


def _inf(dtype):
    return np.inf if dtype == "f64" else 1e30


def acrobot_limits(name, dtype):
    return {"asym": ([-0.4], [1.9]), "excludes_0": ([0.15], [1.2]), "unbounded": ([-_inf(dtype)], [_inf(dtype)]),
            "pinned": ([0.3], [0.3])}[name]


INTEGRATOR_LIMITS = {"asym": ([-0.3, -0.9], [0.6, 0.1]), "pinned_0": ([0.0, -0.5], [0.0, 0.5]), "excludes_0": ([0.05, -0.4], [0.4, -0.1])}


def _box(lo, hi, us, dtype):
    """[fl(u_min - us), fl(u_max - us)] as the kernels form it: in float for an fp32 handle (its limits are floats, capi.hip)."""
    if dtype == "f32":
        f = np.float32
        with np.errstate(over="ignore", invalid="ignore"):
            return ((np.asarray(lo, f)[None, None, :] - us.astype(f)).astype(np.float64),
                    (np.asarray(hi, f)[None, None, :] - us.astype(f)).astype(np.float64))
    return np.asarray(lo, float)[None, None, :] - us, np.asarray(hi, float)[None, None, :] - us


class Invariants:
    """(c): collects what a pass's gains owe the box of the trajectory that pass saw."""

    def __init__(self, lo, hi, dtype):
        self.lo, self.hi, self.dtype = np.asarray(lo, float), np.asarray(hi, float), dtype
        self.pinned = self.lo == self.hi
        self.checked = self.pin_free = self.pin_knots = 0

    def gains(self, us, k, K, sel):
        """us: the trajectory the backward pass ran on; k, K its gains; sel: trajectories whose pass completed."""
        sel = np.asarray(sel) & np.all(np.isfinite(k), axis=(1, 2)) & np.all(np.isfinite(us), axis=(1, 2))
        if not sel.any():
            return
        lo, hi = _box(self.lo, self.hi, us[sel], self.dtype)
        ks, Ks = k[sel], K[sel]
        bad = (ks < lo) | (ks > hi)
        assert not bad.any(), ("k outside its own control's box", np.argwhere(bad)[:5], ks[bad][:5], lo[bad][:5], hi[bad][:5])
        self.checked += int(sel.sum())
        for j in np.flatnonzero(self.pinned):
            assert np.array_equal(ks[:, :, j], lo[:, :, j]), ("pinned control's k is not exactly its box", j)
            free = np.any(Ks[:, :, j, :] != 0, axis=2)  # (a knot where this control's gradient is exactly 0 leaves it free)
            self.pin_free += int(free.sum())
            self.pin_knots += free.size

    def committed(self, us, sel):
        """ILQR_FLAG_REFERENCE_FIXES: the stored controls of trajectories that accepted a step lie in their own limits."""
        u = us[np.asarray(sel)]
        lo, hi = (self.lo, self.hi) if self.dtype == "f64" else (self.lo.astype(np.float32), self.hi.astype(np.float32))  # (a float handle's limits)
        assert np.all((u >= lo) & (u <= hi)), "a committed control outside its own limits"

    def done(self, min_checked):
        assert self.checked >= min_checked, (self.checked, min_checked)
        assert self.pin_free <= max(2, self.pin_knots // 100), (self.pin_free, self.pin_knots)


def stepwise(g, n, inv, fixes=False):
    """n calls of iterate(1), each checked against the trajectory read before it (persistent routes: the commit follows the pass)."""
    for _ in range(n):
        _, us = g.trajectory()
        st0 = g.status()[0]
        g.iterate(1)
        st, it, al = g.status()
        k, K = g.gains()
        inv.gains(us, k, K, (st0 == 0) & (st != 3))
        if fixes:
            inv.committed(g.trajectory()[1], al >= 0)


def _state(g):
    from tests.test_gpu_fused_sweep import _state as s
    return s(g)


def _same(a, b, what):
    for n in a:
        assert np.array_equal(a[n], b[n], equal_nan=True), (what, n)


def nx4_routes(model):
    """(name, flags, route, kernel that must run as the solve stage or None); the two-kernel route first."""
    from ilqr_amd import capi
    default = b"k_solve_hex" if model == "acrobot" else b"k_solve_tile"
    wide = (capi.ROUTE_WIDE_TILES | capi.ROUTE_WIDE_ONE_PER_CU, b"k_solve_wide") if model == "acrobot" else (capi.ROUTE_WIDE_TILES, b"k_solve_wide2")
    return [("unfused", capi.FLAG_UNFUSED, 0, None), ("default", 0, 0, default), ("quad_chain", 0, capi.ROUTE_QUAD_CHAIN, b"k_solve_tile"),
            ("two_tiles_per_cu", 0, capi.ROUTE_TWO_TILES_PER_CU, b"k_solve_tile<2>"), ("wide", 0) + wide, ("staged", capi.FLAG_STAGED, 0, b"")]


def _nx4_case(model, limits, dtype):
    if model == "acrobot":
        lo, hi = acrobot_limits(limits, dtype)
        B, T = 37, 61
        x0 = acrobot_x0(B, scale=0.4, seed=17)
        kw = {}
    else:
        lo, hi = INTEGRATOR_LIMITS[limits]
        B, T = 37, 61
        x0 = integrator_x0(B, seed=23)
        kw = dict(goal=[1.0, 0.5, 0.0, 0.0])
    u0 = np.zeros((B, T, len(lo)))  # (outside the box where it excludes 0)
    return lo, hi, x0, u0, kw


NX4_CASES = [("acrobot", n) for n in ("asym", "excludes_0", "unbounded", "pinned")] + [("integrator", n) for n in INTEGRATOR_LIMITS]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model,limits", NX4_CASES)
def test_nx4_routes_equal_the_two_kernel_route(model, limits, dtype):
    """(a) + (c) on every nx = 4 route: iterate(1) four times (each pass's gains against the box of the trajectory it saw), then to
    the end of the solve; every array and scalar bit-identical to ILQR_FLAG_UNFUSED.  ILQR_FLAG_REFERENCE_FIXES (clamped rollouts)
    on the persistent and the two-kernel route likewise, and every committed control in its own limits."""
    from ilqr_amd import BatchILQR, capi
    lo, hi, x0, u0, kw = _nx4_case(model, limits, dtype)
    B, T = u0.shape[:2]
    sv = capi.STAGE_NAMES.index("solve")
    for fixes in (False, True):
        base = capi.FLAG_REFERENCE_FIXES if fixes else 0
        # (with the fixes the persistent route is the 16-trajectory tile, k_solve_tile: route.hpp plan_route)
        routes = nx4_routes(model) if not fixes else [("unfused", capi.FLAG_UNFUSED, 0, None), ("default", 0, 0, b"k_solve_tile"),
                                                      ("staged", capi.FLAG_STAGED, 0, b"")]
        out = []
        for name, fl, route, kernel in routes:
            g = BatchILQR(model, B, T, DT, u_min=lo, u_max=hi, flags=base | fl, route=route, dtype=dtype, params=dict(max_iter=12), **kw)
            if kernel is not None:
                assert g.lib.ilqr_stage_kernel_name(g.h, sv) == kernel, (name, g.lib.ilqr_stage_kernel_name(g.h, sv))
            inv = Invariants(lo, hi, dtype)
            g.init_traj(x0, u0)
            stepwise(g, 4, inv, fixes=fixes)
            inv.done(min_checked=B)
            s = _state(g)
            g.generate_trajectory()
            s.update({"end_" + n: a for n, a in _state(g).items()})
            out.append((name, s))
            g.close()
        for name, s in out[1:]:
            _same(out[0][1], s, (name, "fixes" if fixes else ""))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model,limits", NX4_CASES)
def test_nx4_limits_against_the_oracle(oracle, model, limits, dtype):
    """(b): teacher-forced backward passes of the stage path at lambda 1 and 1e-3 against the oracle with the same per-control
    limits, then iterations of the default route walked against it (both drives), in fp64 and against the float oracle in fp32."""
    from ilqr_amd import BatchILQR
    from tests.parity import check_backward, walk_iterations
    lo, hi, x0, u0, kw = _nx4_case(model, limits, dtype)
    x0, u0 = x0[:24], u0[:24, :48]
    B, T = u0.shape[:2]
    om = oracle.Model(model, goal=kw.get("goal"), u_min=lo, u_max=hi)
    flav = "f64" if dtype == "f64" else "f32"
    with oracle.flavour(flav):
        omt = om.twin(flav)
        xs, us, cost = oracle.batch_rollout(omt, x0, u0, DT)
        do = oracle.batch_derivatives(omt, xs, us, DT)
    xs, us, cost = [np.asarray(a, dtype=np.float64) for a in (xs, us, cost)]
    do = {kk: np.asarray(v, dtype=np.float64) for kk, v in do.items()}
    g = BatchILQR(model, B, T, DT, u_min=lo, u_max=hi, dtype=dtype, **kw)
    inv = Invariants(lo, hi, dtype)
    for lam in (1.0, 1e-3):
        g.set_trajectory(x0=x0, xs=xs, us=us, cost=cost)
        g.set_derivatives(**{kk: (v if kk in ("cx", "cu") else mat(v)) for kk, v in do.items()})
        g.set_gains(k=np.zeros((B, T, om.nu)), K=np.zeros((B, T, om.nu, 4)))
        g.set_lambda(lam, 1.0)
        div = g.backward_pass()
        k, K = g.gains()
        _, us_d = g.trajectory()
        inv.gains(us_d, k, K, div == 0)
        with oracle.flavour(flav):
            ro = oracle.batch_backward(omt, us, do, k_prev=np.zeros((B, T, om.nu)), lam=lam)
        check_backward(oracle, om, us, do, np.zeros((B, T, om.nu)), lam, k, K, g.dV(), div, ro, max_ties=2, max_over10=2, precision=dtype)
    for drive in ("oracle", "gpu"):
        r = walk_iterations(oracle, om, g, x0, u0, DT, 5, drive=drive, precision=dtype)
        ties = r["ties_backward"] + r["ties_search"] + r["ties_stop"]
        assert r["checked"] >= 3 * B, r["checked"]
        if dtype == "f64":
            assert ties <= max(2, r["checked"] // 16) and r["cond_over10"] <= max(2, r["checked"] // 24), r
            assert sum(p["plain"] for p in r["per_iter"]) >= 0.75 * r["checked"], r["per_iter"]
        else:  # the bounds of test_gpu_fp32.test_iterations_teacher_forced (float: ties are no longer rare near an optimum)
            assert ties + r["conditioned_branch"] <= max(4, r["checked"] // 3), r
            assert r["cond_over10"] <= max(2, r["checked"] // 20) and r["unresolved"] <= r["checked"] // 8, r
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# generic path: the LQ model (and host-evaluated models) with a box per control
# ---------------------------------------------------------------------------------------------------------------------------------
def distinct_boxes(m, seed=0):
    """m boxes, all different: asymmetric ones, one pinned, one excluding 0 (above), one with an edge at 0, one excluding 0 (below)."""
    rng = np.random.default_rng(seed)
    lo, hi = -rng.uniform(0.1, 0.6, m), rng.uniform(0.1, 0.6, m)
    special = [(0.2, 0.2), (0.05, 0.45), (0.0, 0.35), (-0.5, -0.08)]
    for j, (a, b) in enumerate(special[: max(0, m - 1)]):
        lo[(3 * j + 1) % m], hi[(3 * j + 1) % m] = a, b
    if m == 1:
        lo[0], hi[0] = -0.15, 0.5
    return lo, hi


LQ_SHAPES = [(32, 16), (17, 9), (6, 2), (31, 1)]


def _lq_case(n, m):
    from tests.test_gpu_lq_end_to_end import dense_mats
    mats = dense_mats(n, m, seed=3 + n + m)
    lo, hi = distinct_boxes(m, seed=n)
    B, T = (12, 30) if n > 16 else (24, 40)
    rng = np.random.default_rng(n * 100 + m)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.3
    return mats, lo, hi, x0, u0


@pytest.mark.parametrize("n,m", LQ_SHAPES)
def test_lq_routes_with_a_box_per_control(oracle, n, m):
    """Rollout routes (k_rollout_lq with its eleven rollouts, ILQR_ROUTE_LQ_RECOMMIT, the generic k_rollout_g) bit-identical with the
    analytic derivatives, with and without ILQR_FLAG_REFERENCE_FIXES (then every committed control in its own limits); k_backward_w3
    (default, with its m = 1 / m = 2 shortcuts) and k_backward_w2 with finite differences: every pass's gains in their own boxes, and
    iterations walked against the oracle with the same limits."""
    from ilqr_amd import BatchILQR, capi
    from tests.parity import walk_iterations
    mats, lo, hi, x0, u0 = _lq_case(n, m)
    B, T = u0.shape[:2]
    rn = lambda g, s: g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index(s))
    for fixes in (0, capi.FLAG_REFERENCE_FIXES):
        out = []
        for route, kernel in ((0, b"k_rollout_lq"), (capi.ROUTE_LQ_RECOMMIT, b"k_rollout_lq"), (capi.ROUTE_LQ_THREAD_ROLLOUT, b"k_rollout_g")):
            g = BatchILQR("lq", B, T, DT, u_min=lo, u_max=hi, lq=mats, flags=capi.FLAG_ANALYTIC_DERIVATIVES | fixes, route=route,
                          params=dict(max_iter=10))
            assert rn(g, "rollout") == kernel
            inv = Invariants(lo, hi, "f64")
            g.init_traj(x0, u0)
            stepwise(g, 3, inv, fixes=bool(fixes))
            inv.done(min_checked=B)
            s = dict(xs=g.trajectory()[0], us=g.trajectory()[1], cost=g.cost(), k=g.gains()[0], K=g.gains()[1], al=g.status()[2])
            g.generate_trajectory()
            s.update(end_us=g.trajectory()[1], end_cost=g.cost(), end_st=g.status()[0])
            out.append(s)
            g.close()
        for s in out[1:]:
            _same(out[0], s, ("lq rollout routes", n, m, fixes))
    om = oracle.Model("lq", lq=mats, u_min=lo, u_max=hi)
    for route, kernel in ((0, b"k_backward_w3"), (capi.ROUTE_BACKWARD_W2, b"k_backward_w2")):
        g = BatchILQR("lq", B, T, DT, u_min=lo, u_max=hi, lq=mats, route=route)
        assert rn(g, "backward") == kernel
        inv = Invariants(lo, hi, "f64")
        g.init_traj(x0, u0)
        stepwise(g, 3, inv)
        inv.done(min_checked=B)
        r = walk_iterations(oracle, om, g, x0, u0, DT, 4, drive="oracle")
        ties = r["ties_backward"] + r["ties_search"] + r["ties_stop"]
        assert r["checked"] >= 3 * B and ties <= max(2, r["checked"] // 10) and r["unresolved"] == 0, r
        assert r["cond_over10"] <= max(2, r["checked"] // 20), r
        g.close()


@pytest.mark.parametrize("n,m", [(32, 16), (6, 2)])
def test_lq_reference_fixes_walked_against_the_fixed_oracle(oracle, n, m):
    """ILQR_FLAG_REFERENCE_FIXES (clamped rollouts, failed factorisations end the box-QP) against the oracle with the same fixes and limits."""
    from ilqr_amd import BatchILQR, capi
    from tests.parity import walk_iterations
    mats, lo, hi, x0, u0 = _lq_case(n, m)
    B, T = u0.shape[:2]
    om = oracle.Model("lq", lq=mats, u_min=lo, u_max=hi)
    g = BatchILQR("lq", B, T, DT, u_min=lo, u_max=hi, lq=mats, flags=capi.FLAG_REFERENCE_FIXES)
    oracle.set_fixes(3)
    try:
        r = walk_iterations(oracle, om, g, x0, u0, DT, 4, drive="gpu")
    finally:
        oracle.set_fixes(0)
    ties = r["ties_backward"] + r["ties_search"] + r["ties_stop"]
    assert r["checked"] >= 3 * B and ties <= max(2, r["checked"] // 10) and r["unresolved"] == 0, r
    _, us = g.trajectory()
    assert np.all((us >= lo) & (us <= hi))
    g.close()


@pytest.mark.parametrize("route", ["w3", "w2"])
def test_host_model_teacher_forced_backward_with_a_box_per_control(oracle, route):
    """A host-evaluated model (n = 7, m = 3; only the backward pass on the device) with three different boxes -- one pinned, one excluding
    0 --: the oracle's records of its own rollout, the device's pass against the oracle's at lambda 1 and 1e-3 (as
    test_gpu_fixes.test_host_model_backward_pass_with_vxx_regularisation), and the gains in their boxes."""
    from ilqr_amd import BatchILQR, capi
    from tests.parity import check_backward
    from tests.test_gpu_lq_end_to_end import dense_mats
    n, m, B, T = 7, 3, 12, 30
    mats = dense_mats(n, m)
    lo, hi = np.array([-0.15, 0.1, 0.25]), np.array([0.4, 0.35, 0.25])
    om = oracle.Model("lq", lq=mats, u_min=lo, u_max=hi)
    rng = np.random.default_rng(9)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.2
    xs, us, cost = oracle.batch_rollout(om, x0, u0, DT)
    do = oracle.batch_derivatives(om, xs, us, DT)
    g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=lo, u_max=hi, route=capi.ROUTE_BACKWARD_W2 if route == "w2" else 0)
    assert g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index("backward")) == {"w2": b"k_backward_w2", "w3": b"k_backward_w3"}[route]
    inv = Invariants(lo, hi, "f64")
    k_prev = rng.normal(size=(B, T, m)) * 0.1
    for lam in (1.0, 1e-3):
        g.set_trajectory(x0=x0, xs=xs, us=us, cost=cost)
        g.set_derivatives(**{kk: (v if kk in ("cx", "cu") else mat(v)) for kk, v in do.items()})
        g.set_gains(k=k_prev, K=np.zeros((B, T, m, n)))
        g.set_lambda(lam, 1.0)
        div = g.backward_pass()
        k, K = g.gains()
        inv.gains(us, k, K, div == 0)
        ro = oracle.batch_backward(om, us, do, k_prev=k_prev, lam=lam)
        check_backward(oracle, om, us, do, k_prev, lam, k, K, g.dV(), div, ro, max_ties=2, max_over10=2)
    inv.done(min_checked=B)
    g.close()
