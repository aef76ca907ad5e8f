"""17 to 32 controls on the generic path: k_backward_w3w (two 16-column control tiles, the literal box-QP in every step) on
host-evaluated models (ILQR_MODEL_HOST), teacher-forced against the oracle per knot, and ILQR_ROUTE_TWO_CONTROL_TILES, which runs the
same kernel on nu <= 16 problems whose answers k_backward_w3 already pins.  What is not widened is refused by name."""
import numpy as np
import pytest

from tests.util import TOL, mat, relerr, relerr_abs
from tests.parity import check_backward
from tests.parity import first_gain_mismatch_is_knife_edge
from tests.test_gpu_generic_backward import DT, lq_model, run_case
from tests.test_gpu_generic_backward import test_default_kernel_against_the_literal_order_kernel as _literal_order_test
from tests.test_gpu_lq_end_to_end import dense_mats, make, oracle_closed_loop

pytestmark = pytest.mark.gpu


def backward_name(g):
    from ilqr_amd import capi
    return g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index("backward"))


@pytest.mark.parametrize("lam", [1.0, 1e-3])
@pytest.mark.parametrize("n,m", [(32, 32), (32, 24), (24, 20), (17, 17), (8, 32)])
def test_wide_backward_matches_oracle(oracle, n, m, lam):
    """Per-knot gains, dV and diverge flags against the oracle's backward_pass, with part of the controls clamped."""
    om = lq_model(oracle, n, m, lim=0.2)
    frac, g = run_case(oracle, om, B=6, T=12, lam=lam, x_scale=1.0)
    assert backward_name(g) == b"k_backward_w3w"
    assert 0.02 < frac < 0.98, frac  # mixed free / clamped sets: partial K rows, scattered inverses
    g.backward_step()  # the lambda loop and the 32-lane gradient-norm reduction on the same state
    assert np.all(np.isfinite(g.gnorm()))
    g.close()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_wide_non_positive_definite_quu(oracle, where):
    """m = 32, lambda = 0, Quu indefinite with the first, middle or last pivot failing: Eigen's unblocked LLT stops there and the
    partial factor is used (boxqp.cpp:85-88), as test_non_positive_definite_quu pins for m <= 16.  The diverge flags equal the oracle's;
    the gains agree per knot except on the same bounded number of trajectories fp64 cannot pin."""
    om = lq_model(oracle, 32, 32, seed=3, lim=0.5)
    shift = np.zeros(32)
    shift[{"first": 0, "middle": 16, "last": 31}[where]] = -0.35
    frac, g = run_case(oracle, om, B=8, T=10, lam=0.0, u_scale=0.2, cuu_shift=shift, max_unpinned=2)
    ro, div = g.last["ro"], g.last["div"]
    assert np.array_equal(div, ro["diverge"])
    assert g.last["ok"].sum() >= 5, g.last
    g.close()


@pytest.mark.parametrize("lim", [0.05, 0.2])
def test_wide_long_horizon_against_oracle(oracle, lim):
    """T = 200, m = 32, noisy controls of the size of the box: the free set changes along the horizon, so stale factors, scattered
    inverses and partial K rows alternate with whole ones hundreds of times per pass.  Per trajectory the gains agree with the oracle to
    1e-8 per knot, or the first knot where they part is a clamp knife edge (tests/parity.py)."""
    from ilqr_amd import BatchILQR
    n, m = 32, 32
    om = lq_model(oracle, n, m, lim=lim)
    B, T = 8, 200
    rng = np.random.default_rng(11)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = np.clip(rng.normal(size=(B, T, m)) * lim, -1.5 * lim, 1.5 * lim)
    xs, us, cost = oracle.batch_rollout(om, x0, u0, DT)
    dv = oracle.batch_derivatives(om, xs, us, DT)
    k_prev = rng.normal(size=(B, T, m)) * 0.1 * lim
    ro = oracle.batch_backward(om, us, dv, k_prev=k_prev, lam=1e-3)
    g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=om.u_min, u_max=om.u_max)
    g.set_trajectory(x0=x0, xs=xs, us=us, cost=cost)
    g.set_derivatives(**{k: (dv[k] if k in ("cx", "cu") else mat(dv[k])) for k in dv})
    g.set_gains(k=k_prev, K=np.zeros((B, T, m, n)))
    g.set_lambda(1e-3, 1.0)
    div = np.asarray(g.backward_pass())
    k, K = g.gains()
    g.close()
    ko, Ko = np.asarray(ro["k"]), mat(ro["K"])
    assert np.array_equal(div, ro["diverge"]) and np.all(div == 0)
    clamped = (np.abs(K).reshape(B, T, m, n).max(axis=3) == 0)
    changes = (clamped[:, 1:] != clamped[:, :-1]).any(axis=2).mean()
    assert changes > 0.05, changes
    lo_b, hi_b = om.u_min[None, None, :] - us, om.u_max[None, None, :] - us
    for b in range(B):
        if all(np.abs(a[b] - o[b]).max() <= 1e-8 * max(1.0, np.abs(o[b]).max()) for a, o in ((k, ko), (K, Ko))):
            continue
        assert first_gain_mismatch_is_knife_edge(k[b], K[b], ko[b], Ko[b], us[b], lo_b[b], hi_b[b], 1e-8), b


# the case list k_backward_w3 is held to k_backward_w2 on, taken from that test so that the two stay the same list
CROSS_CHECK_CASES = [mk.args[1] for mk in _literal_order_test.pytestmark if mk.name == "parametrize"][0]


@pytest.mark.parametrize("n,m,lim,shift", CROSS_CHECK_CASES)
def test_two_control_tiles_against_one(oracle, n, m, lim, shift):
    """ILQR_ROUTE_TWO_CONTROL_TILES runs k_backward_w3w on the cases test_default_kernel_against_the_literal_order_kernel holds k_backward_w3
    to: equal diverge indices; on the well-conditioned cases k, K, dV and the gradient norm agree to 1e-9 (the two-tile kernel factors every
    box-QP literally where k_backward_w3 refines the previous knot's inverse; both are the inverse to rounding)."""
    from ilqr_amd import BatchILQR, capi
    om = lq_model(oracle, n, m, lim=lim)
    B, T = 9, 14
    rng = np.random.default_rng(5)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.5
    xs, us, cost = oracle.batch_rollout(om, x0, u0, DT)
    dv = oracle.batch_derivatives(om, xs, us, DT)
    if shift is not None:
        s = np.zeros(m)
        s[{"first": 0, "middle": m // 2}[shift]] = -60.0
        dv["cuu"] = dv["cuu"] + np.diag(s)[None, None]
    k_prev = rng.normal(size=(B, T, m)) * 0.1
    outs = []
    for route in (0, capi.ROUTE_TWO_CONTROL_TILES):
        g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=om.u_min, u_max=om.u_max, route=route)
        assert backward_name(g) == {0: b"k_backward_w3", capi.ROUTE_TWO_CONTROL_TILES: b"k_backward_w3w"}[route]
        g.set_trajectory(x0=x0, xs=xs, us=us, cost=cost)
        g.set_derivatives(**{k: (dv[k] if k in ("cx", "cu") else mat(dv[k])) for k in dv})
        g.set_gains(k=k_prev, K=np.zeros((B, T, m, n)))
        g.set_lambda(1e-3 if shift is None else 0.0, 1.0)
        div = g.backward_pass()
        k, K = g.gains()
        outs.append(dict(div=np.asarray(div), k=k, K=K, dV=g.dV(), gnorm=g.gnorm()))
        g.close()
    assert np.array_equal(outs[0]["div"], outs[1]["div"])
    if shift is None:
        for key in ("k", "K", "dV", "gnorm"):
            scale = max(1.0, np.abs(outs[0][key]).max())
            assert np.abs(outs[0][key] - outs[1][key]).max() <= 1e-9 * scale, (key, np.abs(outs[0][key] - outs[1][key]).max(), scale)


def test_wide_control_rejections():
    """nu > 32 is an invalid size; what has not been widened beyond 16 controls says so by name."""
    from ilqr_amd import BatchILQR, capi
    lim = dict(u_min=-np.ones(33), u_max=np.ones(33))
    with pytest.raises(capi.ILQRError, match=r"error -1: .*nu <= 32"):
        BatchILQR("host", 4, 5, DT, nx=8, nu=33, **lim)
    lim = dict(u_min=-np.ones(20), u_max=np.ones(20))
    BatchILQR("lq", 4, 5, DT, lq=dense_mats(8, 20), **lim).close()  # (the LQ twin itself takes 20 controls)
    for kw, what in ((dict(route=capi.ROUTE_BACKWARD_W2), "ILQR_ROUTE_BACKWARD_W2"), (dict(route=capi.ROUTE_LQ_DENSE_FD), "ILQR_ROUTE_LQ_DENSE_FD"),
                     (dict(flags=capi.FLAG_REGULARIZE_VXX), "ILQR_FLAG_REGULARIZE_VXX"), (dict(dtype="f32"), "fp32")):
        with pytest.raises(capi.ILQRError, match=r"error -5: %s supports at most 16 controls \(nu = 20\)" % what):
            BatchILQR("host", 4, 5, DT, nx=8, nu=20, **lim, **kw)
    with pytest.raises(capi.ILQRError, match=r"error -5: ILQR_ROUTE_LQ_DENSE_FD supports at most 16 controls \(nu = 20\)"):
        BatchILQR("lq", 4, 5, DT, lq=dense_mats(8, 20), route=capi.ROUTE_LQ_DENSE_FD, **lim)
    # the cross-check route names one kernel; it does not combine with another backward kernel or with what only k_backward_w3 implements
    lim = dict(u_min=-np.ones(4), u_max=np.ones(4))
    with pytest.raises(capi.ILQRError, match="error -5: ILQR_ROUTE_TWO_CONTROL_TILES and ILQR_ROUTE_BACKWARD_W2"):
        BatchILQR("host", 4, 5, DT, nx=8, nu=4, route=capi.ROUTE_TWO_CONTROL_TILES | capi.ROUTE_BACKWARD_W2, **lim)
    with pytest.raises(capi.ILQRError, match="error -5: ILQR_FLAG_REGULARIZE_VXX is implemented in k_backward_w3"):
        BatchILQR("host", 4, 5, DT, nx=8, nu=4, route=capi.ROUTE_TWO_CONTROL_TILES, flags=capi.FLAG_REGULARIZE_VXX, **lim)


def test_wide_reference_fixes_end_the_qp_on_a_failed_factorisation(oracle):
    """ILQR_FLAG_REFERENCE_FIXES at m = 32: a Cholesky failure on the free subspace ends the box-QP with result -1 (the pass diverges
    there), in w_box_qp's 32-wide instantiation as in the oracle with the same fix."""
    from ilqr_amd import BatchILQR, capi
    n, m, B, T = 16, 32, 8, 10
    om = lq_model(oracle, n, m, seed=3, lim=0.5)
    rng = np.random.default_rng(3)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.2
    xs, us, cost = oracle.batch_rollout(om, x0, u0, DT)
    dv = oracle.batch_derivatives(om, xs, us, DT)
    shift = np.zeros(m)
    shift[20] = -0.35  # an indefinite pivot in the second control tile
    dv["cuu"] = dv["cuu"] + np.diag(shift)[None, None]
    k_prev = rng.normal(size=(B, T, m)) * 0.1
    oracle.set_fixes(2)
    try:
        ro = oracle.batch_backward(om, us, dv, k_prev=k_prev, lam=0.0)
    finally:
        oracle.set_fixes(0)
    ro_plain = oracle.batch_backward(om, us, dv, k_prev=k_prev, lam=0.0)
    g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=om.u_min, u_max=om.u_max, flags=capi.FLAG_REFERENCE_FIXES)
    g.set_trajectory(x0=x0, xs=xs, us=us, cost=cost)
    g.set_derivatives(**{k: (dv[k] if k in ("cx", "cu") else mat(dv[k])) for k in dv})
    g.set_gains(k=k_prev, K=np.zeros((B, T, m, n)))
    g.set_lambda(0.0, 1.0)
    div = np.asarray(g.backward_pass())
    g.close()
    assert np.any(ro["diverge"] != 0) and not np.array_equal(ro["diverge"], ro_plain["diverge"])  # (the fix decides the outcome here)
    assert np.array_equal(div, ro["diverge"])


def stage_kernels(g):
    from ilqr_amd import capi
    return tuple(g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index(s)) for s in ("derivatives", "backward", "rollout"))


@pytest.mark.parametrize("n,m,B,T", [(32, 32, 4, 8), (24, 20, 6, 10)])
def test_wide_lq_stages_match_oracle(oracle, n, m, B, T):
    """The LQ twin with more than 16 controls (LqModelW on the generic kernels), each stage against the oracle on the same inputs:
    the init_traj rollout, the finite-difference records, the backward pass per knot, the 11 line-search rollouts."""
    from oracle.oracle import ALPHAS
    mats = dense_mats(n, m)
    om, g = make(oracle, mats, B, T)
    assert stage_kernels(g) == (b"k_derivatives_g", b"k_backward_w3w", b"k_rollout_g")
    rng = np.random.default_rng(5)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.3
    c0 = g.init_traj(x0, u0)
    xs_o, us_o, c_o = oracle.batch_rollout(om, x0, u0, DT)
    xs, us = g.trajectory()
    assert relerr(xs, xs_o) < 1e-12 and np.array_equal(us, us_o)
    assert np.max(np.abs(c0 - c_o) / np.abs(c_o)) < 1e-12
    g.set_trajectory(x0=x0, xs=xs_o, us=us_o, cost=c_o)
    g.compute_derivatives()
    d = g.derivatives()
    do = oracle.batch_derivatives(om, xs_o, us_o, DT)
    for name in ("fx", "fu", "cx", "cu"):
        ref = do[name] if name in ("cx", "cu") else mat(do[name])
        assert relerr(d[name], ref) < TOL, name
    for name in ("cxx", "cuu", "cxu"):
        assert relerr_abs(d[name][:, :T], mat(do[name])[:, :T], 1e-2) < TOL, name
    assert relerr_abs(d["cxx"][:, T], mat(do["cxx"])[:, T], 1e-2) < TOL
    g.set_derivatives(**{k: (do[k] if k in ("cx", "cu") else mat(do[k])) for k in do})
    k_prev = rng.normal(size=(B, T, m)) * 0.1
    g.set_gains(k=k_prev, K=np.zeros((B, T, m, n)))
    g.set_lambda(1.0, 1.0)
    div = g.backward_pass()
    ro = oracle.batch_backward(om, us_o, do, k_prev=k_prev, lam=1.0)
    k, K = g.gains()
    Ko = mat(ro["K"])
    check_backward(oracle, om, us_o, do, k_prev, 1.0, k, K, g.dV(), div, ro, max_ties=max(1, B // 8), max_over10=max(1, B // 50))
    g.set_gains(k=ro["k"], K=Ko)
    costs = g.rollout_candidates()
    for a in range(len(ALPHAS)):
        _, _, ca = oracle_closed_loop(oracle, om, x0, xs_o, us_o, ro["k"], Ko, ALPHAS[a])
        fin = np.isfinite(ca)
        assert np.max(np.abs(costs[fin, a] - ca[fin]) / np.abs(ca[fin])) < 1e-9, a
    g.close()


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("n,m", [(32, 32), (24, 20)])
def test_wide_lq_free_running_against_oracle(oracle, n, m, analytic):
    """Every iteration of a free-running solve of the wide LQ twin against the oracle (tests/parity.py, device-driven walk), with
    finite differences and with ILQR_FLAG_ANALYTIC_DERIVATIVES; then generate_trajectory() ends every trajectory with a finite cost
    that is not above where it started."""
    from ilqr_amd import capi
    from tests.parity import walk_iterations
    B, T, lim = 10, 16, 0.4
    om, g = make(oracle, dense_mats(n, m, seed=5), B, T, lim=lim, flags=capi.FLAG_ANALYTIC_DERIVATIVES if analytic else 0)
    rng = np.random.default_rng(3)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.1
    r = walk_iterations(oracle, om, g, x0, u0, DT, 4, drive="gpu")
    assert r["checked"] >= 2 * B and len(r["tied"]) <= B // 4, r
    c0 = g.init_traj(x0, u0)
    g.generate_trajectory()
    c = g.cost()
    assert g.count_running() == 0 and np.all(np.isfinite(c)) and np.all(c <= c0 * (1 + 1e-9))
    g.close()


@pytest.fixture(scope="module")
def wide_user_lib():
    from ilqr_amd import _build
    return _build.build_user(_build.USER_WIDE_HEADER, _build.USER_WIDE_LIB)


def test_wide_user_twin(wide_user_lib, oracle):
    """examples/user_model_linear_wide.hpp (n = 24, m = 20, plain loops): every iteration of a free-running solve against the
    oracle's LQ model with the same matrices, and the same problem through the shipped LQ twin (whose sums run in another order:
    agreement to the finite differences' rounding)."""
    from ilqr_amd import BatchILQR
    from tests.parity import walk_iterations
    n, m, B, T, lim = 24, 20, 16, 20, 0.4
    mats = dense_mats(n, m, seed=5)
    params = np.concatenate([np.ascontiguousarray(a).ravel() for a in mats])
    rng = np.random.default_rng(3)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.1
    g = BatchILQR("user", B, T, DT, u_min=-lim, u_max=lim, lib=wide_user_lib, nx=n, nu=m, user_params=params)
    assert stage_kernels(g) == (b"k_derivatives_g", b"k_backward_w3w", b"k_rollout_g")
    om = oracle.Model("lq", lq=mats, u_lim=lim)
    r = walk_iterations(oracle, om, g, x0, u0, DT, 4, drive="gpu")
    assert r["checked"] >= 2 * B and len(r["tied"]) <= B // 8, r
    g.init_traj(x0, u0)
    g.iterate(3)
    c_user, (k_user, _) = g.cost(), g.gains()
    g2 = BatchILQR("lq", B, T, DT, u_min=-lim, u_max=lim, lq=mats)
    g2.init_traj(x0, u0)
    g2.iterate(3)
    ok = np.abs(c_user - g2.cost()) <= 1e-6 * np.abs(c_user)
    assert ok.mean() > 0.9, ok.mean()
    k2, _ = g2.gains()
    assert np.abs(k_user[ok] - k2[ok]).max() <= 1e-6 * max(1.0, np.abs(k2).max())
    g.generate_trajectory()
    assert g.count_running() == 0 and np.all(np.isfinite(g.cost())) and np.all(g.cost() <= c_user * (1 + 1e-9))
    g.close()
    g2.close()
