"""Per-trajectory model parameters on the generic wavefront-per-trajectory path (ilqr_set_trajectory_params; the PT instantiations of
k_rollout_g and k_derivatives_g), on the pendulum chain (examples/user_model_pendulum_chain.hpp, NTP = 8).  The CPU side is the existing
twin, one oracle.Model("chain", chain=(NL, params[b])) PER TRAJECTORY, called on batches of one: rollouts and every block of the records,
whole iterations teacher-forced from each trajectory's own twin, full solves, a receding-horizon loop whose targets come from device
memory, the fp32 handle against the float twin, and every refusal."""
import os

import numpy as np
import pytest

from tests.parity import (TOL32, conditioning_verdict, first_gain_mismatch_is_knife_edge, gains_knot_err, load_state)
from tests.test_gpu_user_chain import DT, NL, PARAMS, chain_x0
from tests.util import TOL, mat, relerr

pytestmark = pytest.mark.gpu
NX, NU = 2 * NL, NL // 2


@pytest.fixture(scope="module")
def chain_lib():
    from ilqr_amd import _build
    if not os.path.exists(_build.USER_CHAIN_LIB) and not os.path.exists(_build.HIPCC):
        pytest.skip("the pendulum-chain build is missing and there is no hipcc to make it")
    return _build.build_user(_build.USER_CHAIN_HEADER, _build.USER_CHAIN_LIB)


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """the MPC test copies from torch tensors: torch's device is initialised before this module creates any handle"""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


def draw_params(B, seed):
    """g/l, damping, coupling and the four weights within +-20 % of PARAMS, the target angle uniform in [-1, 1]"""
    rng = np.random.default_rng(seed)
    p = PARAMS[None, :] * (1.0 + rng.uniform(-0.2, 0.2, (B, 8)))
    p[:, 7] = rng.uniform(-1.0, 1.0, B)
    return p


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def handle(chain_lib, B, T, lim, **kw):
    from ilqr_amd import BatchILQR, capi
    g = BatchILQR("user", B, T, DT, u_min=-lim, u_max=lim, lib=chain_lib, nx=NX, nu=NU, user_params=PARAMS, **kw)
    names = {s: g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index(s)) for s in ("derivatives", "backward", "rollout")}
    assert names == {"derivatives": b"k_derivatives_g", "backward": b"k_backward_w3", "rollout": b"k_rollout_g"}, names
    return g


def twins(oracle, params, lim):
    return [oracle.Model("chain", chain=(NL, params[b]), u_lim=lim) for b in range(len(params))]


def each(fn, models, *arrays, **kw):
    """fn(model_b, arrays[b:b+1] ...) per trajectory, the results stacked back into batch arrays (tuples and dicts alike)"""
    outs = [fn(m, *[a[b:b + 1] for a in arrays], **kw) for b, m in enumerate(models)]
    if isinstance(outs[0], dict):
        return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(len(outs[0])))


def check_records(d, do, scale_noise=0.0):
    """the tolerances of test_rollout_and_records_match_the_oracle_twin (scale_noise: what float storage adds, relative)"""
    for key in ("fx", "fu", "cx", "cu"):
        ref = do[key] if key in ("cx", "cu") else mat(do[key])
        assert np.abs(d[key] - ref).max() <= (1e-8 + scale_noise) * max(1.0, np.abs(ref).max()), (key, np.abs(d[key] - ref).max())
    for key in ("cxx", "cxu", "cuu"):
        ref = mat(do[key])
        assert np.abs(d[key] - ref).max() <= (TOL + scale_noise) * max(1.0, np.abs(ref).max()), (key, np.abs(d[key] - ref).max())


def test_rollout_and_records_match_each_trajectorys_twin(oracle, chain_lib):
    B, T, lim = 23, 50, 2.0
    g = handle(chain_lib, B, T, lim)
    params = draw_params(B, 41)
    oms = twins(oracle, params, lim)
    g.set_trajectory_params(params)
    assert np.array_equal(g.trajectory_params(), params)
    x0 = chain_x0(B)
    u0 = np.random.default_rng(1).normal(size=(B, T, NU)) * 0.5
    cost = g.init_traj(x0, u0)
    xs, us = g.trajectory()
    xs_o, us_o, c_o = each(lambda m, a, b: oracle.batch_rollout(m, a, b, DT), oms, x0, u0)
    print("rollout: xs relerr %.2e cost relerr %.2e" % (relerr(xs, xs_o), np.max(np.abs(cost - c_o) / np.abs(c_o))))
    assert relerr(xs, xs_o) < 1e-12 and np.array_equal(us, u0) and np.max(np.abs(cost - c_o) / np.abs(c_o)) < 1e-12
    # ... and NOT the shared model's: the parameters reached the kernel
    xs_s, _, c_s = oracle.batch_rollout(oracle.Model("chain", chain=(NL, PARAMS), u_lim=lim), x0, u0, DT)
    assert np.min(np.abs(cost - c_s) / np.abs(c_s)) > 1e-4
    g.set_trajectory(x0=x0, xs=xs_o, us=us_o, cost=c_o)
    g.compute_derivatives()
    d = g.derivatives()
    do = each(lambda m, a, b: oracle.batch_derivatives(m, a, b, DT), oms, xs_o, us_o)
    check_records(d, do)
    assert np.abs(d["cxx"]).max() > 1.0 and np.abs(d["fx"] - np.eye(NX)[None, None]).max() > 0.01
    # clear: back to the handle-wide model, and the getter says that nothing is set
    g.clear_trajectory_params()
    from ilqr_amd import capi
    with pytest.raises(capi.ILQRError, match=r"error -4: .*no per-trajectory parameters are set"):
        g.trajectory_params()
    cost_c = g.init_traj(x0, u0)
    assert np.max(np.abs(cost_c - c_s) / np.abs(c_s)) < 1e-12
    g.close()


def test_it_is_really_per_trajectory(oracle, chain_lib):
    B, T, lim = 12, 60, 2.0
    g, g_plain = handle(chain_lib, B, T, lim), handle(chain_lib, B, T, lim)
    x0 = np.repeat(chain_x0(1, seed=17), B, axis=0)  # every trajectory the same x0 and u0
    u0 = np.repeat(np.random.default_rng(2).normal(size=(1, T, NU)) * 0.3, B, axis=0)
    params = np.repeat(PARAMS[None], B, axis=0)
    params[:, 7] = np.linspace(-1.0, 1.0, B)  # ... and a target of its own
    oms = twins(oracle, params, lim)
    g.set_trajectory_params(params)
    cost = g.init_traj(x0, u0)
    _, _, c_o = each(lambda m, a, b: oracle.batch_rollout(m, a, b, DT), oms, x0, u0)
    assert np.max(np.abs(cost - c_o) / np.abs(c_o)) < 1e-12
    assert np.unique(np.round(cost, 6)).size == B, cost  # different targets, different costs
    g.iterate(3)
    c3 = g.cost()
    assert np.unique(np.round(c3, 6)).size == B and np.all(c3 <= cost) and np.any(c3 < cost)
    # rows that all equal PARAMS: the results of a handle that never set any
    rows = np.repeat(PARAMS[None], B, axis=0)
    x0r = chain_x0(B, seed=19)
    g.set_trajectory_params(rows)
    res = []
    for h in (g, g_plain):
        c0 = h.init_traj(x0r, u0)
        h.iterate(3)
        xs, us = h.trajectory()
        k, K = h.gains()
        res.append((c0, h.cost(), xs, us, k, K))
    same_bits = all(np.array_equal(a, b) for a, b in zip(*res))
    print("equal rows reproduce the shared-parameter bits:", same_bits)
    for a, b in zip(*res):
        assert relerr(a.reshape(B, -1), b.reshape(B, -1)) < 1e-12
    g.close()
    g_plain.close()


def test_whole_iterations_against_each_trajectorys_twin(oracle, chain_lib):
    """Five iterations, teacher-forced from the twins' state each iteration (walk_iterations(drive="oracle")'s loop with one model per
    trajectory): accepted alpha, status, lambda, gains to TOL per knot, cost to TOL.  Whatever deviates must be PROVEN a clamp tie, a
    line-search tie, an exit tie or fp64 conditioning (the extended-precision twin), and all of those together stay under the cap of
    test_iterations_walked_against_the_oracle_twin.  The seeds were checked on the CPU: twins whose parameters differ in the last bit
    choose the same alphas for every trajectory and iteration."""
    from oracle.oracle import ALPHAS
    B, T, iters = 21, 80, 5
    for lim, seed in ((2.0, 43), (0.5, 44)):
        g = handle(chain_lib, B, T, lim)
        params = draw_params(B, seed)
        oms = twins(oracle, params, lim)
        g.set_trajectory_params(params)
        x0 = chain_x0(B, seed=5)
        u0 = np.zeros((B, T, NU))
        xs, us, cost = each(lambda m, a, b: oracle.batch_rollout(m, a, b, DT), oms, x0, u0)
        st = dict(xs=xs, us=us, k=np.zeros((B, T, NU)), K=np.zeros((B, T, NU, NX)), cost=cost, lam=np.ones(B), dlam=np.ones(B))
        running = np.ones(B, dtype=bool)
        checked = ties = 0
        for it in range(iters):
            if not running.any():
                break
            nx = each(lambda m, *a: oracle.batch_iterate_from(m, *a, DT, n_iters=1), oms, x0, st["xs"], st["us"], st["k"], st["K"], st["cost"], st["lam"], st["dlam"])
            load_state(g, x0, st)
            g.iterate(1)
            gxs, gus = g.trajectory()
            gk, gK = g.gains()
            glam, gdlam = g.lambdas()
            gst, _, gal = g.status()
            gcost = g.cost()
            gst = np.where(gst == 4, 0, gst)
            eg = gains_knot_err(gk, gK, nx["k"], nx["K"], st["us"])
            ec = np.abs(gcost - nx["cost"]) / np.abs(nx["cost"])
            lo, hi = -lim - st["us"], lim - st["us"]
            for b in np.flatnonzero(running):
                checked += 1
                same = gal[b] == nx["alpha"][b] and gst[b] == nx["status"][b] and np.isclose(glam[b], nx["lam"][b], rtol=1e-12, atol=0)
                if same and eg[b] < TOL and ec[b] < TOL:
                    continue
                where = "limit %g iteration %d trajectory %d: alpha %d/%d status %d/%d gain err %.2e cost err %.2e" % (
                    lim, it, b, gal[b], nx["alpha"][b], gst[b], nx["status"][b], eg[b], ec[b])
                print("set aside:", where)
                ties += 1
                if eg[b] >= TOL:
                    if first_gain_mismatch_is_knife_edge(gk[b], gK[b], nx["k"][b], nx["K"][b], st["us"][b], lo[b], hi[b], TOL):
                        continue
                    s = slice(b, b + 1)
                    with oracle.flavour("f80"):
                        r80 = oracle.batch_iterate_from(oms[b].twin("f80"), x0[s], st["xs"][s], st["us"][s], st["k"][s], st["K"][s], st["cost"][s],
                                                        st["lam"][s], st["dlam"][s], DT, n_iters=1)
                    _, _, ok = conditioning_verdict(gk[s], gK[s], nx["k"][s], nx["K"][s], r80["k"], r80["K"], st["us"][s], TOL)
                    assert ok[0], "backward passes differ away from a clamp tie and beyond conditioning -- " + where
                    continue
                if gal[b] != nx["alpha"][b]:  # the earlier-accepted alpha's cost change lies within rounding of zero (z_min = 0)
                    a_lo = min(a for a in (gal[b], nx["alpha"][b]) if a >= 0)
                    s = slice(b, b + 1)
                    cands = [float(oracle.batch_rollout(oms[b], x0[s], st["us"][s] + ALPHAS[a] * nx["k"][s], DT, xs_nom=st["xs"][s], K=nx["K"][s])[2][0])
                             for a in (range(a_lo, len(ALPHAS)) if min(gal[b], nx["alpha"][b]) < 0 else [a_lo])]
                    assert np.any(np.abs(st["cost"][b] - np.array(cands)) <= 1e-9 * abs(st["cost"][b])), "line searches differ away from a tie -- " + where
                    continue
                if gst[b] != nx["status"][b]:
                    dcost = st["cost"][b] - nx["cost"][b]
                    assert abs(dcost - 1e-6) <= 1e-9 * abs(st["cost"][b]) or abs(nx["lam"][b] - 1e11) <= 1e-9 * 1e11, "exits differ away from a tie -- " + where
                    continue
                raise AssertionError("same gains, alpha and status but cost / lambda differ -- " + where)
            running &= nx["status"] == 0
            st = {kk: nx[kk] for kk in ("xs", "us", "k", "K", "cost", "lam", "dlam")}
        print("per-trajectory walk, limit %g: checked %d, set aside %d" % (lim, checked, ties))
        assert checked >= B * 3, checked
        assert ties <= max(2, checked // 10), (ties, checked)
        g.close()


def test_full_solve(oracle, chain_lib):
    """Trajectories finish at different iterations; the final controls re-rolled through each trajectory's own twin reproduce its cost.
    Exits against batch_solve per trajectory in distribution only, with the shares of test_full_solve_in_distribution (this model ends
    its solves in plateaus: that test's docstring)."""
    B, T, lim = 32, 120, 2.0
    g = handle(chain_lib, B, T, lim)
    params = draw_params(B, 47)
    oms = twins(oracle, params, lim)
    g.set_trajectory_params(params)
    x0 = chain_x0(B, seed=8)
    u0 = np.zeros((B, T, NU))
    g.init_traj(x0, u0)
    g.generate_trajectory()
    assert g.count_running() == 0
    st, it, _ = g.status()
    assert np.unique(it).size > 1, it  # (finished at different iterations)
    assert np.array_equal(g.trajectory_params(), params)
    xs, us = g.trajectory()
    xs_o, _, c_o = each(lambda m, a, b: oracle.batch_rollout(m, a, b, DT), oms, x0, us)
    rel = np.abs(g.cost() - c_o) / np.abs(c_o)
    print("full solve: open-loop re-roll cost relerr max %.2e, xs relerr %.2e" % (rel.max(), relerr(xs, xs_o)))
    assert rel.max() < 1e-9
    ro = each(lambda m, a, b: oracle.batch_solve(m, a, b, DT), oms, x0, u0)
    same = (st == ro["status"]) & (it == ro["iters"])
    relc = np.abs(g.cost() - ro["cost"]) / np.abs(ro["cost"])
    print("full solves: same exit %.2f, cost rel err median %.2e max %.2e" % (same.mean(), np.median(relc), relc.max()))
    assert same.mean() >= 0.6, (same.mean(), st, ro["status"], it, ro["iters"])
    assert np.abs(it - ro["iters"]).max() <= 2
    assert np.median(relc) < 1e-6 and (relc < 1e-4).mean() >= 0.9, relc
    g.close()


def test_mpc_with_a_moving_target_from_device_memory(chain_lib):
    """Three receding-horizon steps whose targets are written by torch into a device tensor before each step, handed over as p_device,
    with no host synchronisation between the calls: torch runs on a stream of its own and the handle is given that stream (the stream
    rule of ilqr_amd/batch.py).  The same rows from host arrays with a synchronize() after every call leave the same state."""
    import torch
    B, T, lim = 40, 60, 2.0
    dev = torch.device("cuda", 0)
    x0 = chain_x0(B, seed=23)
    u0 = np.zeros((B, T, NU))
    base = draw_params(B, 53)
    targets = [np.random.default_rng(60 + s).uniform(-1, 1, B) for s in range(3)]
    x_next = [chain_x0(B, seed=70 + s) * 0.8 for s in range(3)]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        g = handle(chain_lib, B, T, lim, stream=stream.cuda_stream)
        g.set_trajectory_params(base)
        g.init_traj(x0, u0)
        g.iterate(2)
        p_dev = torch.tensor(base, dtype=torch.float64, device=dev)
        t_host = [torch.tensor(t, dtype=torch.float64).pin_memory() for t in targets]
        x_dev = [torch.tensor(x, dtype=torch.float64, device=dev) for x in x_next]
        stream.synchronize()
        for s in range(3):  # nothing below waits for the GPU
            p_dev[:, 7].copy_(t_host[s], non_blocking=True)
            g.set_trajectory_params(ptr=p_dev.data_ptr())
            g.mpc_step(x0_ptr=x_dev[s].data_ptr(), shift=1, iters=2)
        g.synchronize()
    ref = handle(chain_lib, B, T, lim)
    ref.set_trajectory_params(base)
    ref.synchronize()
    ref.init_traj(x0, u0)
    ref.iterate(2)
    ref.synchronize()
    for s in range(3):
        rows = base.copy()
        rows[:, 7] = targets[s]
        ref.set_trajectory_params(rows)
        ref.synchronize()
        ref.mpc_step(x0=x_next[s], shift=1, iters=2)
        ref.synchronize()
    last = base.copy()
    last[:, 7] = targets[2]
    assert np.array_equal(g.trajectory_params(), last) and np.array_equal(ref.trajectory_params(), last)
    (xs, us), (xs_r, us_r) = g.trajectory(), ref.trajectory()
    print("mpc from device rows: xs relerr %.2e us relerr %.2e cost relerr %.2e" % (
        relerr(xs, xs_r), relerr(us, us_r), np.max(np.abs(g.cost() - ref.cost()) / np.abs(ref.cost()))))
    assert relerr(xs, xs_r) < 1e-12 and relerr(us, us_r) < 1e-12 and np.max(np.abs(g.cost() - ref.cost()) / np.abs(ref.cost())) < 1e-12
    g.close()
    ref.close()


def test_fp32_handle_against_the_float_twin(oracle, chain_lib):
    """The float rollouts' twin and the double twin of the finite differences both see the FLOAT-rounded rows: rollout and one iteration
    against the oracle's float twin built from each row (tests/test_gpu_generic_fp32.py's tolerances), the records against the double
    twin built from the rows' float values -- and they are, to one float ulp, the records of an fp64 handle given the float-rounded rows."""
    B, T, lim = 10, 30, 1.3
    g32 = handle(chain_lib, B, T, lim, dtype="f32")
    params = draw_params(B, 59)
    params[:, 0] += 1.0 / 3.0 * 1e-3  # (no row is representable in float)
    assert np.all(f32(params) != params)
    g32.set_trajectory_params(params)
    assert np.array_equal(g32.trajectory_params(), params)  # stored as given; rounded where they are used
    oms = twins(oracle, params, lim)
    oms32 = [m.twin("f32") for m in oms]
    rng = np.random.default_rng(7)
    x0 = f32(chain_x0(B, seed=7))
    u0 = f32(rng.normal(size=(B, T, NU)) * 0.3)
    cost = g32.init_traj(x0, u0)
    xs, us = g32.trajectory()
    with oracle.flavour("f32"):
        xs32, us32, c32 = each(lambda m, a, b: oracle.batch_rollout(m, a, b, DT), oms32, x0, u0)
    xs32, c32 = np.asarray(xs32, dtype=np.float64), np.asarray(c32, dtype=np.float64)
    print("fp32 rollout: xs relerr %.2e cost relerr %.2e" % (relerr(xs, xs32), np.max(np.abs(cost - c32) / np.abs(c32))))
    assert np.array_equal(us, u0) and np.array_equal(xs, f32(xs))
    assert relerr(xs, xs32) < TOL32 and np.max(np.abs(cost - c32) / np.abs(c32)) < TOL32
    # records: double finite differences of the model with the rows' float values, from the float knot, stored as float
    g32.compute_derivatives()
    d32 = g32.derivatives()
    oms_r = twins(oracle, f32(params), f32(lim))
    do = each(lambda m, a, b: oracle.batch_derivatives(m, a, b, DT), oms_r, xs, us)
    check_records(d32, do, scale_noise=2.0 ** -23)
    g64 = handle(chain_lib, B, T, f32(lim))
    g64.set_trajectory_params(f32(params))
    g64.set_trajectory(x0=x0, xs=xs, us=us, cost=cost)
    g64.compute_derivatives()
    d64 = g64.derivatives()
    for key in d32:
        ref32 = np.asarray(d64[key], dtype=np.float32)
        err = np.max(np.abs(d32[key] - ref32.astype(np.float64)) / np.spacing(np.abs(ref32)).astype(np.float64))
        assert np.array_equal(d32[key], f32(d32[key])) and err <= 1.0, (key, err)
    g64.close()
    # one iteration from the float twin's state
    st = dict(xs=xs32, us=np.asarray(us32, dtype=np.float64), k=np.zeros((B, T, NU)), K=np.zeros((B, T, NU, NX)), cost=c32, lam=np.ones(B), dlam=np.ones(B))
    with oracle.flavour("f32"):
        nx = each(lambda m, *a: oracle.batch_iterate_from(m, *a, DT, n_iters=1), oms32, x0, st["xs"], st["us"], st["k"], st["K"], st["cost"], st["lam"], st["dlam"])
    nx = {kk: (np.asarray(v, dtype=np.float64) if v.dtype.kind == "f" else v) for kk, v in nx.items()}
    load_state(g32, x0, st)
    g32.iterate(1)
    gk, gK = g32.gains()
    _, _, gal = g32.status()
    same = gal == nx["alpha"]
    eg = gains_knot_err(gk, gK, nx["k"], nx["K"], st["us"])
    ec = np.abs(g32.cost() - nx["cost"]) / np.abs(nx["cost"])
    print("fp32 iteration: same alpha %d/%d, gain err max %.2e, cost err max (same alpha) %.2e" % (same.sum(), B, eg.max(), ec[same].max()))
    # (PRECISIONS["f32"]["gtol"]: the backward pass is double on float records on both sides; beyond it only a proven clamp tie)
    lo, hi = f32(-lim) - st["us"], f32(lim) - st["us"]
    off = [b for b in range(B) if eg[b] >= 1e-5]
    for b in off:
        assert first_gain_mismatch_is_knife_edge(gk[b], gK[b], nx["k"][b], nx["K"][b], st["us"][b], lo[b], hi[b], 1e-5), (b, eg[b])
    ok = same & (eg < 1e-5)
    assert ok.sum() >= B - max(2, B // 8) and np.all(ec[ok] < TOL32), (gal, nx["alpha"], ec, eg)
    g32.close()


def test_refusals(chain_lib):
    from ilqr_amd import BatchILQR, _build, capi
    rows = np.zeros((4, 8))
    # another model
    g = BatchILQR("acrobot", 4, 10, DT)
    for call in (lambda: g.set_trajectory_params(rows), g.trajectory_params, g.clear_trajectory_params):
        with pytest.raises(capi.ILQRError, match=r"error -5: .*ILQR_MODEL_USER"):
            call()
    g.close()
    # the nx = 4 user twin: persistent tiled kernels
    lib4 = _build.build_user(_build.USER_EXAMPLE_HEADER, _build.USER_EXAMPLE_LIB)
    g = BatchILQR("user", 4, 10, DT, u_min=-5.0, u_max=5.0, lib=lib4, nx=4, nu=1)
    assert g.lib.ilqr_trajectory_params_count() == 0
    assert g.lib.ilqr_set_trajectory_params(g.h, rows.ctypes.data_as(capi._dp), None, 8) == -5
    assert b"nx = 4" in g.lib.ilqr_last_error() and b"generic wavefront-per-trajectory" in g.lib.ilqr_last_error()
    g.close()
    # the n = 6 small twin: tiled kernels unless asked onto the generic ones -- and then only its header stands in the way
    lib6 = _build.build_user(_build.USER_EXAMPLE6_HEADER, _build.USER_EXAMPLE6_LIB)
    g = BatchILQR("user", 4, 10, DT, u_min=-1.0, u_max=1.0, lib=lib6, nx=6, nu=2)
    assert g.lib.ilqr_set_trajectory_params(g.h, rows.ctypes.data_as(capi._dp), None, 8) == -5
    assert b"ILQR_ROUTE_WAVE_PER_TRAJECTORY" in g.lib.ilqr_last_error()
    g.close()
    g = BatchILQR("user", 4, 10, DT, u_min=-1.0, u_max=1.0, lib=lib6, nx=6, nu=2, route=capi.ROUTE_WAVE_PER_TRAJECTORY)
    assert g.lib.ilqr_set_trajectory_params(g.h, rows.ctypes.data_as(capi._dp), None, 8) == -5
    msg = g.lib.ilqr_last_error()
    assert b"declares no per-trajectory parameters" in msg and b"ILQR_ROUTE_WAVE_PER_TRAJECTORY" not in msg, msg
    g.close()
    # the chain: a wrong count, both pointers, neither; nothing was set by any of them
    g = handle(chain_lib, 4, 10, 2.0)
    p = rows.ctypes.data_as(capi._dp)
    assert g.lib.ilqr_set_trajectory_params(g.h, p, None, 7) == -1 and b"n = 7" in g.lib.ilqr_last_error() and b"NTP = 8" in g.lib.ilqr_last_error()
    assert g.lib.ilqr_set_trajectory_params(g.h, p, p, 8) == -1 and b"exactly one of p" in g.lib.ilqr_last_error()
    assert g.lib.ilqr_set_trajectory_params(g.h, None, None, 8) == -1 and b"exactly one of p" in g.lib.ilqr_last_error()
    assert g.lib.ilqr_get_trajectory_params(g.h, p, 8) == -4 and b"no per-trajectory parameters are set" in g.lib.ilqr_last_error()
    with pytest.raises(ValueError):
        g.set_trajectory_params(rows, ptr=1)
    with pytest.raises(capi.ILQRError, match=r"error -1: .*n = 5"):
        g.set_trajectory_params(np.zeros((4, 5)))
    g.close()
