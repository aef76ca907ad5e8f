"""The fp32 mode on the generic path (ILQR_DTYPE_F32 with the LQ model and with user twins of any size: k_rollout_g, k_derivatives_g,
k_derivatives_lq, k_analytic_lq, k_backward_w3).  The split is DESIGN.md 3.6's: float storage and float rollouts; finite differences,
exact derivatives and the whole backward pass in double on the widened float values, rounded when stored.  So it is checked three ways:
  (1) against an fp64 handle built from the float-rounded model and fed the same float values: the records and gains of the fp32
      handle are the fp64 handle's rounded to float (one float ulp where the double lies on a rounding boundary), dV and diverge equal;
  (2) against the oracle's float twin (flavour "f32"), stage by stage and for whole iterations (tests/parity.py);
  (3) whole solves against the fp64 handle, and the result getters against each other."""
import numpy as np
import pytest

from tests.parity import TOL32, check_backward, walk_iterations
from tests.test_gpu_lq_end_to_end import dense_mats, lq_mats
from tests.util import mat, relerr

pytestmark = pytest.mark.gpu
DT = 0.02
NL = 8
PARAMS = np.array([9.81, 0.1, 2.0, 10.0, 1.0, 0.1, 50.0, 0.0])


@pytest.fixture(scope="module")
def chain_lib():
    from ilqr_amd import _build
    import os
    if not os.path.exists(_build.USER_CHAIN_LIB) and not os.path.exists(_build.HIPCC):
        pytest.skip("the pendulum-chain build is missing and there is no hipcc to make it")
    return _build.build_user(_build.USER_CHAIN_HEADER, _build.USER_CHAIN_LIB)


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """test_whole_solves_and_results copies into torch tensors: torch's device is initialised before this module creates any handle
    (run on its own, a torch initialised after the library had set up the device reported no GPU)."""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def ulps(a, ref):
    """|a - ref| in float ulps of ref (a, ref float-valued)."""
    ref32 = np.asarray(ref, dtype=np.float32)
    return np.max(np.abs(np.asarray(a, dtype=np.float64) - ref32.astype(np.float64)) / np.spacing(np.abs(ref32)).astype(np.float64), initial=0.0)


# (name, model kind, B, T, limit): LQ at configs[4]'s dimensions (k_backward_w3's FULL instantiation), a ragged dense LQ, the chain
CASES = [("lq32x16", "lq", 6, 12, 0.7), ("lq20x5", "lq", 9, 20, 0.7), ("chain", "chain", 10, 30, 1.3)]


def pair(name, kind, B, T, lim, chain_lib, flags=0, route=0):
    """An fp32 handle and the fp64 handle of the same float-rounded model and limits."""
    from ilqr_amd import BatchILQR
    lo, hi = f32(-lim), f32(lim)
    if kind == "lq":
        mats = lq_mats(32, 16) if name == "lq32x16" else dense_mats(20, 5)
        g32 = BatchILQR("lq", B, T, DT, u_min=-lim, u_max=lim, lq=mats, flags=flags, route=route, dtype="f32")
        g64 = BatchILQR("lq", B, T, DT, u_min=lo, u_max=hi, lq=[f32(a) for a in mats], flags=flags, route=route)
    else:
        kw = dict(lib=chain_lib, nx=2 * NL, nu=NL // 2, flags=flags, route=route)
        g32 = BatchILQR("user", B, T, DT, u_min=-lim, u_max=lim, user_params=PARAMS, dtype="f32", **kw)
        g64 = BatchILQR("user", B, T, DT, u_min=lo, u_max=hi, user_params=f32(PARAMS), **kw)
    return g32, g64


def float_state(g, seed):
    rng = np.random.default_rng(seed)
    x0 = f32(rng.uniform(-1, 1, (g.B, g.nx)))
    xs = f32(np.concatenate([x0[:, None], rng.uniform(-1, 1, (g.B, g.T, g.nx))], axis=1))
    us = f32(rng.normal(size=(g.B, g.T, g.nu)) * 0.5)
    k = f32(rng.normal(size=(g.B, g.T, g.nu)) * 0.2)
    return x0, xs, us, k


def feed(gs, x0, xs, us, k):
    for g in gs:
        g.set_trajectory(x0=x0, xs=xs, us=us, cost=np.zeros(g.B))
        g.set_gains(k=k, K=np.zeros((g.B, g.T, g.nu, g.nx)))


def assert_rounded(a32, a64, what):
    assert np.array_equal(a32, f32(a32)), what  # stored as float
    assert ulps(a32, f32(a64)) <= 1.0, (what, ulps(a32, f32(a64)))


def route_flags(kind):
    from ilqr_amd import capi
    out = [(0, 0)]
    if kind == "lq":
        out += [(0, capi.ROUTE_LQ_DENSE_FD), (capi.FLAG_ANALYTIC_DERIVATIVES, 0), (capi.FLAG_ANALYTIC_DERIVATIVES, capi.ROUTE_FULL_RECORDS)]
    return out


@pytest.mark.parametrize("name,kind,B,T,lim", CASES)
def test_records_are_the_fp64_records_rounded(chain_lib, name, kind, B, T, lim):
    """k_derivatives_lq, k_derivatives_g (dense LQ route, knot T, the chain) and k_analytic_lq: the same double arithmetic from the
    widened float knot, one rounding on the way out."""
    for flags, route in route_flags(kind):
        g32, g64 = pair(name, kind, B, T, lim, chain_lib, flags, route)
        x0, xs, us, k = float_state(g32, 3)
        feed((g32, g64), x0, xs, us, k)
        for g in (g32, g64):
            g.compute_derivatives()
        d32, d64 = g32.derivatives(), g64.derivatives()
        for key in ("fx", "fu", "cx", "cu", "cxx", "cxu", "cuu"):
            assert_rounded(d32[key], d64[key], (name, flags, route, key))
        assert np.abs(d32["cxx"]).max() > 0.1
        g32.close()
        g64.close()


@pytest.mark.parametrize("name,kind,B,T,lim", CASES)
def test_gains_are_the_fp64_gains_rounded(chain_lib, name, kind, B, T, lim):
    """k_backward_w3's float-storage instantiations (FULL at 32 x 16, the bounds-checked default, REGV) on float records, and on the
    record-free exact LQ route (LQF: cx, cu formed from the float knot, the matrices from the double const_rec)."""
    from ilqr_amd import capi
    variants = [(0, [1.0, 1e-3]), (capi.FLAG_REGULARIZE_VXX, [1.0, 1e-3])]
    if kind == "lq":
        variants.append((capi.FLAG_ANALYTIC_DERIVATIVES, [1.0, 1e-3]))
    for flags, lams in variants:
        g32, g64 = pair(name, kind, B, T, lim, chain_lib, flags)
        x0, xs, us, k = float_state(g32, 5)
        feed((g32, g64), x0, xs, us, k)
        if not flags & capi.FLAG_ANALYTIC_DERIVATIVES:
            g64.compute_derivatives()  # float-valued records for both: the fp64 handle's rounded
            recs = {kk: f32(v) for kk, v in g64.derivatives().items()}
            for g in (g32, g64):
                g.set_derivatives(**recs)
        else:
            assert g32.lib.ilqr_stage_kernel_name(g32.h, capi.STAGE_NAMES.index("derivatives")) == b""  # (the fused route: no sweep)
        for lam in lams:
            for g in (g32, g64):
                g.set_lambda(lam, 1.0)
                g.set_gains(k=k)
            div32, div64 = g32.backward_pass(), g64.backward_pass()
            (k32, K32), (k64, K64) = g32.gains(), g64.gains()
            what = (name, flags, lam)
            assert_rounded(k32, k64, what)
            assert_rounded(K32, K64, what)
            assert np.array_equal(div32, div64) and np.array_equal(g32.dV(), g64.dV()), what
            assert np.abs(K64).max() > 1e-3, what
        g32.close()
        g64.close()


def oracle_models(oracle, name, kind, lim, chain_lib):
    from ilqr_amd import BatchILQR
    if kind == "lq":
        mats = lq_mats(32, 16) if name == "lq32x16" else dense_mats(20, 5)
        om = oracle.Model("lq", lq=mats, u_lim=lim)
        mk = lambda B, T, **kw: BatchILQR("lq", B, T, DT, u_min=-lim, u_max=lim, lq=mats, dtype="f32", **kw)
    else:
        om = oracle.Model("chain", chain=(NL, PARAMS), u_lim=lim)
        mk = lambda B, T, **kw: BatchILQR("user", B, T, DT, u_min=-lim, u_max=lim, lib=chain_lib, nx=2 * NL, nu=NL // 2, user_params=PARAMS,
                                          dtype="f32", **kw)
    return om, om.twin("f32"), mk


def x0_for(kind, B, seed):
    rng = np.random.default_rng(seed)
    if kind == "chain":
        return f32(np.concatenate([rng.uniform(-1, 1, (B, NL)), rng.uniform(-1, 1, (B, NL)) * 0.5], axis=1))
    return None


@pytest.mark.parametrize("name,kind,B,T,lim", CASES[1:])
def test_against_the_oracle_float_twin(oracle, chain_lib, name, kind, B, T, lim):
    om, om32, mk = oracle_models(oracle, name, kind, lim, chain_lib)
    g = mk(B, T)
    rng = np.random.default_rng(7)
    x0 = x0_for(kind, B, 7) if kind == "chain" else f32(rng.uniform(-1, 1, (B, om.nx)))
    u0 = f32(rng.normal(size=(B, T, om.nu)) * 0.3)
    # rollout (k_rollout_g in float, the cost summed in double)
    cost = g.init_traj(x0, u0)
    xs, us = g.trajectory()
    with oracle.flavour("f32"):
        xs32, us32, c32 = oracle.batch_rollout(om32, x0, u0, DT)
        do = oracle.batch_derivatives(om32, xs32, us32, DT)
    assert np.array_equal(us, u0) and np.array_equal(xs, f32(xs))
    assert relerr(xs, xs32) < TOL32 and np.max(np.abs(cost - c32) / np.abs(c32)) < TOL32
    # teacher-forced backward pass on the float twin's records
    k_prev = f32(rng.normal(size=(B, T, om.nu)) * 0.2)
    for lam in (1.0, 1e-3):
        with oracle.flavour("f32"):
            ro = oracle.batch_backward(om32, us32, do, k_prev=k_prev, lam=lam)
        g.set_trajectory(x0=x0, xs=xs32, us=us32, cost=c32)
        g.set_derivatives(**{kk: (do[kk] if kk in ("cx", "cu") else mat(do[kk])) for kk in do})
        g.set_gains(k=k_prev, K=np.zeros((B, T, om.nu, om.nx)))
        g.set_lambda(lam, 1.0)
        div = g.backward_pass()
        k, K = g.gains()
        r = check_backward(oracle, om, us32, {kk: np.asarray(v, dtype=np.float64) for kk, v in do.items()}, k_prev, lam, k, K, g.dV(), div, ro,
                           max_ties=max(2, B // 8), max_over10=max(1, B // 50), precision="f32")
        print("generic fp32 backward", name, lam, {kk: v for kk, v in r.items() if kk != "good"})
        assert r["good"].sum() > 0
    g.close()
    # whole iterations walked against the float twin (the caps of tests/test_gpu_fp32.py)
    g = mk(B, T)
    r = walk_iterations(oracle, om, g, x0, np.zeros((B, T, om.nu)), DT, 4, precision="f32")
    g.close()
    print("generic fp32 walk", name, r)
    ties = r["ties_backward"] + r["ties_search"] + r["ties_stop"]
    assert r["checked"] >= B * 2
    assert ties + r["conditioned_branch"] <= max(4, r["checked"] // 3), r
    assert r["cond_over10"] <= max(2, r["checked"] // 20), r
    assert r["unresolved"] <= r["checked"] // 8, r


@pytest.mark.parametrize("name,kind,B,T,lim", CASES[1:])
def test_clamped_rollouts_against_the_oracle(oracle, chain_lib, name, kind, B, T, lim):
    """ILQR_FLAG_REFERENCE_FIXES: k_rollout_g's clamp in float, every mode (init, search, the commit rerun)."""
    from ilqr_amd import capi
    om, om32, mk = oracle_models(oracle, name, kind, lim, chain_lib)
    g = mk(B, T, flags=capi.FLAG_REFERENCE_FIXES)
    rng = np.random.default_rng(9)
    x0 = x0_for(kind, B, 9) if kind == "chain" else f32(rng.uniform(-1, 1, (B, om.nx)))
    u0 = f32(rng.normal(size=(B, T, om.nu)) * 2 * lim)
    oracle.set_fixes(3)
    try:
        cost = g.init_traj(x0, u0)
        xs, us = g.trajectory()
        with oracle.flavour("f32"):
            xs32, us32, c32 = oracle.batch_rollout(om32, x0, u0, DT)
        assert np.abs(us).max() <= np.float32(lim) and np.abs(u0).max() > lim
        assert np.array_equal(us, us32) and relerr(xs, xs32) < TOL32 and np.max(np.abs(cost - c32) / np.abs(c32)) < TOL32
        g.iterate(3)
        _, us = g.trajectory()
        assert np.abs(us).max() <= np.float32(lim) and np.all(np.isfinite(g.cost()))
    finally:
        oracle.set_fixes(0)
    g.close()


@pytest.mark.parametrize("name,kind,B,T,lim", [("lq32x16", "lq", 64, 40, 0.7), ("chain", "chain", 48, 40, 1.3)])
def test_whole_solves_and_results(chain_lib, name, kind, B, T, lim):
    import torch
    g32, g64 = pair(name, kind, B, T, lim, chain_lib)
    rng = np.random.default_rng(13)
    x0 = x0_for(kind, B, 13) if kind == "chain" else f32(rng.uniform(-1, 1, (B, g32.nx)))
    u0 = np.zeros((B, T, g32.nu))
    for g in (g32, g64):
        g.init_traj(x0, u0)
        g.generate_trajectory()
        assert g.count_running() == 0
    c32, c64 = g32.cost(), g64.cost()
    assert np.all(np.isfinite(c32))
    rel = np.abs(c32 - c64) / np.abs(c64)
    print("generic fp32 vs fp64 full solves", name, "median %.2e max %.2e" % (np.median(rel), rel.max()))
    assert np.median(rel) < 1e-4 and (rel < 1e-2).mean() > 0.9, rel
    # the getters, the asynchronous results and the device copies agree, and every value is a float
    xs, us = g32.trajectory()
    k, K = g32.gains()
    for a in (xs, us, k, K):
        assert np.array_equal(a, f32(a))
    bufs = g32.result_buffers(pinned=True)
    for a in bufs.values():
        a.fill(np.nan)
    g32.results_async(bufs)
    g32.synchronize()
    assert np.array_equal(bufs["xs"], xs) and np.array_equal(bufs["us"], us) and np.array_equal(bufs["k"], k)
    assert np.array_equal(np.swapaxes(bufs["K"], -1, -2), K) and np.array_equal(bufs["cost"], c32)
    dev = torch.device("cuda", 0)
    t = {n: torch.full(s, float("nan"), dtype=torch.float64, device=dev) for n, s in
         (("xs", xs.shape), ("us", us.shape), ("k", k.shape), ("K", (B, T, g32.nx, g32.nu)))}
    torch.cuda.synchronize()
    g32.copy_trajectory_to_device(t["xs"].data_ptr(), t["us"].data_ptr())
    g32.copy_gains_to_device(t["k"].data_ptr(), t["K"].data_ptr())
    g32.synchronize()
    assert np.array_equal(t["xs"].cpu().numpy(), xs) and np.array_equal(t["us"].cpu().numpy(), us)
    assert np.array_equal(t["k"].cpu().numpy(), k) and np.array_equal(np.swapaxes(t["K"].cpu().numpy(), -1, -2), K)
    g32.close()
    g64.close()


def test_refusals_and_routes():
    from ilqr_amd import BatchILQR, capi
    mats = dense_mats(20, 5)
    lim = dict(u_min=-np.ones(5), u_max=np.ones(5))
    g = BatchILQR("lq", 4, 5, DT, lq=mats, dtype="f32", **lim)
    names = [g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index(s)) for s in ("derivatives", "backward", "rollout")]
    assert names == [b"k_derivatives_lq", b"k_backward_w3", b"k_rollout_g"], names
    g.close()
    for kw, what in ((dict(route=capi.ROUTE_BACKWARD_W2), "ILQR_ROUTE_BACKWARD_W2"), (dict(route=capi.ROUTE_TWO_CONTROL_TILES), "ILQR_ROUTE_TWO_CONTROL_TILES")):
        with pytest.raises(capi.ILQRError, match=r"error -5: fp32 .*%s" % what):
            BatchILQR("lq", 4, 5, DT, lq=mats, dtype="f32", **kw, **lim)
    with pytest.raises(capi.ILQRError, match=r"error -5: fp32 .*ILQR_MODEL_HOST"):
        BatchILQR("host", 4, 5, DT, nx=8, nu=5, dtype="f32", **lim)
