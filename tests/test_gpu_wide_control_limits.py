"""A box per control on the routes that run 17 to 32 controls, and infinite limits on every wave box-QP.

tests/test_gpu_control_limits.py gives every control its own box up to 16 controls; tests/test_gpu_wide_controls.py runs 17 to 32
controls with one symmetric box for all of them.  Between the two, nothing could tell a kernel that reads control j - 16's limits in
the second control tile (u_min[lane & 15]), builds a tile-2 hi from -u_min, or drops a pinned tile-2 control's zero K row when K is
scattered into tile 2 -- nor a wave box-QP (w_box_qp at 16 or 32 lanes, w3_box_qp_fast) that mishandles an infinite limit, which
only the acrobot's scalar QP had seen.  wide_boxes() places pinned, 0-excluding, 0-edged and infinite boxes in tile 2, none of them
equal or mirrored to its tile-1 partner's; tests/test_oracle_wide_boxes.py shows on the CPU that the oracle's answers on exactly these
problems move far beyond the tolerances below under folded, mirrored or swapped limits.  Checked here:
  (a) host-evaluated models at 17 to 32 controls (k_backward_w3w), teacher-forced against the oracle, with and without infinite limits;
  (b) host-evaluated models at 1 to 16 controls with infinite limits on k_backward_w3, k_backward_w2 and the two-tile route, which must
      also agree with k_backward_w3;
  (c) the wide LQ twin end to end: every pass's gains in their own boxes, iterations walked against the oracle (also with
      ILQR_FLAG_REFERENCE_FIXES, whose clamped rollouts keep every committed control in its own limits), a finished solve;
  (d) the wide example user twin (n = 24, m = 20) likewise.
The invariants and tolerances are those of tests/test_gpu_control_limits.py."""
import numpy as np
import pytest

from tests.util import mat
from tests.test_gpu_control_limits import DT, Invariants, distinct_boxes, stepwise
from tests.test_gpu_lq_end_to_end import dense_mats
from tests.test_gpu_wide_controls import backward_name, stage_kernels, wide_user_lib  # noqa: F401 (wide_user_lib: a fixture)

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------------------------
# the problems (shared with tests/test_oracle_wide_boxes.py, which runs the oracle alone on each of them)
# ---------------------------------------------------------------------------------------------------------------------------------
PINNED = (0.27, 0.27)
ABOVE_0 = (0.06, 0.41)      # excludes 0: the box lies above it
BELOW_0 = (-0.44, -0.07)    # excludes 0: the box lies below it
EDGE_0 = (0.0, 0.33)
PINNED_0 = (0.0, 0.0)       # pinned, both edges at 0
FREE = (-np.inf, np.inf)
UPPER_ONLY = (-np.inf, 0.08)
LOWER_ONLY = (-0.05, np.inf)


def wide_boxes(m, seed=0, unbounded=False):
    """m > 16 boxes, all different.  Lane 16 (the first of tile 2) is pinned away from 0; lane m - 1 is pinned at 0 (an edge at 0 and
    a pinned box; at m = 17 lane 16's box wins).  The other tile-2 lanes take, in this order of priority, the infinite boxes
    (unbounded=True: (-inf, inf), (finite, inf)), the boxes excluding 0 from above and from below and one with an edge at 0; what
    does not fit in tile 2 (m < 24) goes to tile 1, which also holds (-inf, finite) when unbounded.  The rest are random asymmetric.
    Lanes j and j + 16 never get equal or mirrored boxes."""
    assert 16 < m <= 32
    rng = np.random.default_rng(seed)
    lo, hi = -rng.uniform(0.1, 0.6, m), rng.uniform(0.1, 0.6, m)
    tile2 = list(range(17, m - 1))
    order = ([FREE, LOWER_ONLY] if unbounded else []) + [ABOVE_0, BELOW_0, EDGE_0]
    tile1 = [2, 5, 8, 11, 14, 3]
    place = {16: PINNED}
    if m - 1 > 16:
        place[m - 1] = PINNED_0
    if unbounded:
        place[tile1.pop(0)] = UPPER_ONLY
    for box in order:
        place[tile2.pop(0) if tile2 else tile1.pop(0)] = box
    for j, (a, b) in place.items():
        lo[j], hi[j] = a, b
    boxes = list(zip(lo, hi))
    assert len(set(boxes)) == m
    for j in range(16, m):
        assert boxes[j] != boxes[j - 16] and boxes[j] != (-hi[j - 16], -lo[j - 16]), j
    return lo, hi


def infinite_boxes(m):
    """Box sets for m <= 16 with infinite limits: distinct_boxes(m) with one control unbounded on both sides and one on one side (for
    m >= 3 two of them, one per side), on lanes distinct_boxes leaves random.  m <= 2 has room for one replacement: a set per kind."""
    lo, hi = distinct_boxes(m, seed=m)
    if m <= 2:
        out = []
        for box in (FREE, UPPER_ONLY, LOWER_ONLY):
            a, b = lo.copy(), hi.copy()
            a[0], b[0] = box
            out.append((a, b))
        return out
    special = {(3 * j + 1) % m for j in range(min(4, m - 1))}
    spare = [j for j in range(m - 1, -1, -1) if j not in special]
    for box in (FREE, UPPER_ONLY, LOWER_ONLY)[: min(3, len(spare))]:
        j = spare.pop(0)
        lo[j], hi[j] = box
    return [(lo, hi)]


WIDE_HOST_SHAPES = [(32, 32), (24, 20), (5, 17), (16, 31)]   # (5, 17): one lane in tile 2; (16, 31): one padded lane
NARROW_INF_SHAPES = [(32, 16), (17, 9), (7, 3), (6, 2), (31, 1)]
WIDE_LQ_CASES = [(32, 32, True), (24, 20, False)]           # (n, m, unbounded); (24, 20) is also the example user twin
LAMBDAS = (1.0, 1e-3)


def host_problem(oracle, n, m, lo, hi, B=12, T=30):
    """The oracle's rollout and records of an LQ model with these boxes, the gains the box-QPs start from (as
    test_gpu_control_limits.test_host_model_teacher_forced_backward_with_a_box_per_control)."""
    mats = dense_mats(n, m)
    om = oracle.Model("lq", lq=mats, u_min=lo, u_max=hi)
    rng = np.random.default_rng(9 + n + m)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.2
    xs, us, cost = oracle.batch_rollout(om, x0, u0, DT)
    do = oracle.batch_derivatives(om, xs, us, DT)
    k_prev = rng.normal(size=(B, T, m)) * 0.1
    return dict(om=om, x0=x0, xs=xs, us=us, cost=cost, do=do, k_prev=k_prev)


def wide_lq_case(n, m, unbounded):
    """The LQ twin's problem: matrices, boxes, x0, u0 (B, T as the wide tests' sizes allow)."""
    mats = dense_mats(n, m, seed=5)
    lo, hi = wide_boxes(m, seed=n, unbounded=unbounded)
    B, T = 12, 24
    rng = np.random.default_rng(n * 100 + m)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.2
    return mats, lo, hi, x0, u0


# ---------------------------------------------------------------------------------------------------------------------------------
# (a), (b): teacher-forced backward passes
# ---------------------------------------------------------------------------------------------------------------------------------
def _teacher_forced(oracle, p, lo, hi, route, inv):
    """The device's pass on the oracle's records at each lambda, checked against the oracle per knot and against the invariants."""
    from ilqr_amd import BatchILQR
    from tests.parity import check_backward
    om, us, do, k_prev = p["om"], p["us"], p["do"], p["k_prev"]
    B, T, m = us.shape
    n = om.nx
    g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=lo, u_max=hi, route=route)
    name = backward_name(g)
    outs = []
    for lam in LAMBDAS:
        g.set_trajectory(x0=p["x0"], xs=p["xs"], us=us, cost=p["cost"])
        g.set_derivatives(**{kk: (v if kk in ("cx", "cu") else mat(v)) for kk, v in do.items()})
        g.set_gains(k=k_prev, K=np.zeros((B, T, m, n)))
        g.set_lambda(lam, 1.0)
        div = np.asarray(g.backward_pass())
        k, K = g.gains()
        inv.gains(us, k, K, div == 0)
        ro = oracle.batch_backward(om, us, do, k_prev=k_prev, lam=lam)
        check_backward(oracle, om, us, do, k_prev, lam, k, K, g.dV(), div, ro, max_ties=2, max_over10=2)
        outs.append(dict(div=div, k=k, K=K, dV=g.dV(), gnorm=g.gnorm()))
    g.close()
    return name, outs


@pytest.mark.parametrize("unbounded", [False, True])
@pytest.mark.parametrize("n,m", WIDE_HOST_SHAPES)
def test_wide_host_backward_with_a_box_per_control(oracle, n, m, unbounded):
    """(a) k_backward_w3w with wide_boxes at lambda 1 and 1e-3: k, K, dV and the diverge flags per knot against the oracle with the
    same limits; every k inside its own control's box, a pinned control's k exactly its box and its K row 0."""
    lo, hi = wide_boxes(m, seed=n, unbounded=unbounded)
    p = host_problem(oracle, n, m, lo, hi)
    inv = Invariants(lo, hi, "f64")
    name, _ = _teacher_forced(oracle, p, lo, hi, 0, inv)
    assert name == b"k_backward_w3w"
    inv.done(min_checked=2 * len(p["x0"]))


@pytest.mark.parametrize("n,m", NARROW_INF_SHAPES)
def test_infinite_limits_on_every_wave_box_qp(oracle, n, m):
    """(b) infinite limits at m <= 16 through k_backward_w3 (w3_box_qp_fast, the m = 1 / m = 2 shortcuts), k_backward_w2 (w_box_qp at 16
    lanes) and ILQR_ROUTE_TWO_CONTROL_TILES (w_box_qp at 32 lanes), each against the oracle and the invariants as in (a); the two-tile
    route also leaves k_backward_w3's diverge flags and, to 1e-9, its k, K, dV and gradient norm (test_two_control_tiles_against_one)."""
    from ilqr_amd import capi
    for lo, hi in infinite_boxes(m):
        assert np.isinf(lo).any() or np.isinf(hi).any()
        p = host_problem(oracle, n, m, lo, hi)
        runs = {}
        for route, kernel in ((0, b"k_backward_w3"), (capi.ROUTE_BACKWARD_W2, b"k_backward_w2"), (capi.ROUTE_TWO_CONTROL_TILES, b"k_backward_w3w")):
            inv = Invariants(lo, hi, "f64")
            name, runs[route] = _teacher_forced(oracle, p, lo, hi, route, inv)
            assert name == kernel, (name, kernel)
            inv.done(min_checked=2 * len(p["x0"]))
        for one, two in zip(runs[0], runs[capi.ROUTE_TWO_CONTROL_TILES]):
            assert np.array_equal(one["div"], two["div"])
            for key in ("k", "K", "dV", "gnorm"):
                scale = max(1.0, np.abs(one[key]).max())
                assert np.abs(one[key] - two[key]).max() <= 1e-9 * scale, (key, np.abs(one[key] - two[key]).max(), scale)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c), (d): the wide twins end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _walk_bounds(r, B):
    """The bounds of test_gpu_control_limits.test_lq_routes_with_a_box_per_control."""
    ties = r["ties_backward"] + r["ties_search"] + r["ties_stop"]
    assert r["checked"] >= 3 * B and ties <= max(2, r["checked"] // 10) and r["unresolved"] == 0, r
    assert r["cond_over10"] <= max(2, r["checked"] // 20), r


def _walk_fixed(oracle, om, g, x0, u0, B):
    """ILQR_FLAG_REFERENCE_FIXES walked against the oracle with the same fixes (clamped rollouts, failed factorisations end the box-QP)."""
    from tests.parity import walk_iterations
    oracle.set_fixes(3)
    try:
        r = walk_iterations(oracle, om, g, x0, u0, DT, 4, drive="gpu")
    finally:
        oracle.set_fixes(0)
    _walk_bounds(r, B)


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("n,m,unbounded", WIDE_LQ_CASES)
def test_wide_lq_twin_with_a_box_per_control(oracle, n, m, unbounded, analytic):
    """(c) the wide LQ twin (k_backward_w3w, k_rollout_g) with wide_boxes, finite differences or ILQR_FLAG_ANALYTIC_DERIVATIVES: three
    passes' gains in their own boxes; iterations walked against the oracle with the same limits (both drives); with
    ILQR_FLAG_REFERENCE_FIXES (k_rollout_g's clamp, tile 2 included) every committed control in its own limits, walked against the
    oracle with the fixes; a finished solve ends every trajectory with a finite cost not above its start."""
    from ilqr_amd import BatchILQR, capi
    from tests.parity import walk_iterations
    mats, lo, hi, x0, u0 = wide_lq_case(n, m, unbounded)
    B = len(x0)
    om = oracle.Model("lq", lq=mats, u_min=lo, u_max=hi)
    base = capi.FLAG_ANALYTIC_DERIVATIVES if analytic else 0
    for fixes in (0, capi.FLAG_REFERENCE_FIXES):
        g = BatchILQR("lq", B, u0.shape[1], DT, u_min=lo, u_max=hi, lq=mats, flags=base | fixes)
        names = stage_kernels(g)
        assert names[1:] == (b"k_backward_w3w", b"k_rollout_g"), names
        inv = Invariants(lo, hi, "f64")
        g.init_traj(x0, u0)
        stepwise(g, 3, inv, fixes=bool(fixes))
        inv.done(min_checked=B)
        if fixes:
            _walk_fixed(oracle, om, g, x0, u0, B)
            inv.committed(g.trajectory()[1], np.ones(B, dtype=bool))
        else:
            for drive in ("oracle", "gpu"):
                _walk_bounds(walk_iterations(oracle, om, g, x0, u0, DT, 4, drive=drive), B)
        c0 = g.init_traj(x0, u0)
        g.generate_trajectory()
        c = g.cost()
        assert g.count_running() == 0 and np.all(np.isfinite(c)) and np.all(c <= c0 * (1 + 1e-9)), (c, c0)
        if fixes:
            inv.committed(g.trajectory()[1], np.ones(B, dtype=bool))
        g.close()


def test_wide_user_twin_with_a_box_per_control(wide_user_lib, oracle):
    """(d) examples/user_model_linear_wide.hpp (n = 24, m = 20; the user twin's limits are copied per control into its model) with
    wide_boxes(20): iterations walked against the oracle's LQ model with the same matrices and boxes; with ILQR_FLAG_REFERENCE_FIXES
    against the oracle with the fixes, every committed control in its own limits."""
    from ilqr_amd import BatchILQR, capi
    from tests.parity import walk_iterations
    mats, lo, hi, x0, u0 = wide_lq_case(24, 20, False)
    B = len(x0)
    params = np.concatenate([np.ascontiguousarray(a).ravel() for a in mats])
    om = oracle.Model("lq", lq=mats, u_min=lo, u_max=hi)
    for fixes in (0, capi.FLAG_REFERENCE_FIXES):
        g = BatchILQR("user", B, u0.shape[1], DT, u_min=lo, u_max=hi, lib=wide_user_lib, nx=24, nu=20, user_params=params, flags=fixes)
        assert stage_kernels(g) == (b"k_derivatives_g", b"k_backward_w3w", b"k_rollout_g")
        inv = Invariants(lo, hi, "f64")
        g.init_traj(x0, u0)
        stepwise(g, 3, inv, fixes=bool(fixes))
        inv.done(min_checked=B)
        if fixes:
            _walk_fixed(oracle, om, g, x0, u0, B)
            inv.committed(g.trajectory()[1], np.ones(B, dtype=bool))
        else:
            _walk_bounds(walk_iterations(oracle, om, g, x0, u0, DT, 4, drive="gpu"), B)
        g.close()
