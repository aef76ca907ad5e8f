"""Per-knot model parameters on the generic wavefront-per-trajectory path (ilqr_set_knot_params; the PK instantiations of k_rollout_g,
k_derivatives_g and k_evaluate_g), on the pendulum chain (examples/user_model_pendulum_chain.hpp, NTP = 8).  The CPU side is
tests/knot_params.py -- one oracle twin per (trajectory, knot), proven on the CPU by tests/test_knot_params_abi.py --: rollouts and every
block of the records, which row governs which knot, the line search and the commit, equal rows against the per-trajectory handle, a
tracking MPC loop fed from a long device reference with no host synchronisation, policy evaluation, resets, the fp32 handle and every
refusal.  Tolerances are those of tests/test_gpu_traj_params.py: 1e-12 relative for open-loop rollouts and costs, check_records' bounds for
the records, tests.util.TOL for closed-loop per-knot comparisons, tests/test_gpu_generic_fp32.py's (TOL32) for fp32."""
import numpy as np
import pytest

from tests.knot_params import knot_records, knot_rollout, knot_twins, knot_window
from tests.parity import TOL32
from tests.test_gpu_traj_params import check_records, f32, handle
from tests.test_gpu_user_chain import DT, NL, PARAMS, chain_x0
from tests.util import TOL, mat, relerr

pytestmark = pytest.mark.gpu
NX, NU, NTP = 2 * NL, NL // 2, 8


@pytest.fixture(scope="module")
def chain_lib():
    import os
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


def draw_rows(B, n_knots, seed):
    """[B][n_knots][8]: all eight parameters within +-20 % of PARAMS, drawn anew at every knot; the target angle a sinusoid of amplitude 1
    with a phase and a period of each trajectory's own"""
    rng = np.random.default_rng(seed)
    rows = PARAMS[None, None, :] * (1.0 + rng.uniform(-0.2, 0.2, (B, n_knots, 8)))
    phase, period = rng.uniform(0.0, 2.0 * np.pi, (B, 1)), rng.uniform(10.0, 40.0, (B, 1))
    rows[:, :, 7] = np.sin(phase + 2.0 * np.pi * np.arange(n_knots)[None, :] / period)
    return rows


def relcost(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)))


def state(g):
    xs, us = g.trajectory()
    k, K = g.gains()
    return dict(xs=xs, us=us, k=k, K=K, cost=g.cost(), lam=g.lambdas()[0])


# ---- 1. rollout and records against the per-knot twins ---------------------------------------------------------------------------------
def test_rollout_and_records_match_the_per_knot_twins(oracle, chain_lib):
    """B = 67: the init rollout crosses a 64-lane block, the search runs five trajectories per wavefront with a partial last one."""
    B, T, lim = 67, 6, 2.0
    g = handle(chain_lib, B, T, lim)
    rows = draw_rows(B, T + 1, 71)
    tw = knot_twins(oracle, rows, lim)
    g.set_knot_params(rows)
    assert np.array_equal(g.knot_params(), rows)
    x0 = chain_x0(B, seed=31)
    u0 = np.random.default_rng(1).normal(size=(B, T, NU)) * 0.5
    cost = g.init_traj(x0, u0)
    xs, us = g.trajectory()
    xs_o, us_o, c_o = knot_rollout(tw, x0, u0, DT)
    print("rollout: xs relerr %.2e cost relerr %.2e" % (relerr(xs, xs_o), relcost(cost, c_o)))
    assert relerr(xs, xs_o) < 1e-12 and np.array_equal(us, u0) and relcost(cost, c_o) < 1e-12
    g.set_trajectory(x0=x0, xs=xs_o, us=us_o, cost=c_o)
    g.compute_derivatives()
    d = g.derivatives()
    check_records(d, knot_records(tw, xs_o, us_o, DT))
    assert np.abs(d["cxx"]).max() > 1.0 and np.abs(d["fx"] - np.eye(NX)[None, None]).max() > 0.01 and np.abs(d["cx"][:, T]).max() > 0.1
    # the same inputs under per-trajectory rows (row 0 of each trajectory): another problem
    g.set_trajectory_params(rows[:, 0])
    cost_pt = g.init_traj(x0, u0)
    print("against row 0 for every knot: cost differs by at least %.2e relative" % np.min(np.abs(cost_pt - cost) / np.abs(cost)))
    assert np.min(np.abs(cost_pt - cost) / np.abs(cost)) > 1e-4
    # a window of a longer host reference (the handle's scratch grows), bit for bit
    long = draw_rows(B, 2 * T + 5, 72)
    g.set_knot_params(long, k0=2)
    assert np.array_equal(g.knot_params(), knot_window(long, 2, T)) and np.array_equal(g.knot_params(), long[:, 2:T + 3])
    g.set_knot_params(long[:, :4], k0=1)  # ... and of one that ends inside the horizon
    assert np.array_equal(g.knot_params(), knot_window(long[:, :4], 1, T)) and np.all(g.knot_params()[:, 2:] == long[:, 3:4])
    g.close()


# ---- 2. which row governs which knot -----------------------------------------------------------------------------------------------
def test_which_row_governs_which_knot(oracle, chain_lib):
    B, T, lim = 3, 6, 2.0
    g, g2 = handle(chain_lib, B, T, lim), handle(chain_lib, B, T, lim)
    rows = draw_rows(B, T + 1, 73)
    other = draw_rows(B, T + 1, 74)
    x0 = chain_x0(B, seed=32)
    u0 = np.random.default_rng(2).normal(size=(B, T, NU)) * 0.5
    g.set_knot_params(rows)
    cost = g.init_traj(x0, u0)
    xs, us = g.trajectory()
    g.compute_derivatives()
    d = g.derivatives()

    def records_elsewhere(rows2, knot):
        g2.set_knot_params(rows2)
        g2.init_traj(x0, u0)
        g2.set_trajectory(x0=x0, xs=xs, us=us, cost=cost)  # the same knots: only the rows differ
        g2.compute_derivatives()
        d2 = g2.derivatives()
        for t in range(T + 1):
            same = all(np.array_equal(d[key][:, t], d2[key][:, t]) for key in d)
            assert same == (t != knot), (knot, t)

    # row 3 alone: x_0 .. x_3 keep their bits, x_4 on move
    r3 = rows.copy()
    r3[:, 3] = other[:, 3]
    g2.set_knot_params(r3)
    cost3 = g2.init_traj(x0, u0)
    xs3, _ = g2.trajectory()
    assert np.array_equal(xs3[:, :4], xs[:, :4]) and np.all(np.abs(xs3[:, 4:] - xs[:, 4:]).reshape(B, -1).max(axis=1) > 1e-6)
    assert np.all(cost3 != cost)
    records_elsewhere(r3, 3)
    # row T alone: the states keep their bits, the cost moves by the twins' difference in final cost
    rT = rows.copy()
    rT[:, T] = other[:, T]
    g2.set_knot_params(rT)
    costT = g2.init_traj(x0, u0)
    xsT, _ = g2.trajectory()
    assert np.array_equal(xsT, xs)
    fc = lambda r: np.array([oracle.Model("chain", chain=(NL, r[b, T]), u_lim=lim).final_cost(xs[b, T]) for b in range(B)])
    want = fc(rT) - fc(rows)
    print("row T: cost moves by %s, the twins' final costs by %s" % (costT - cost, want))
    # (both costs are the same running sum plus one final cost: their difference is good to the rounding of the totals)
    assert np.all(np.abs(want) > 1e-3) and np.max(np.abs((costT - cost) - want)) <= 1e-12 * np.abs(cost).max()
    records_elsewhere(rT, T)
    g.close()
    g2.close()


# ---- 3. the search and the commit ---------------------------------------------------------------------------------------------------
def test_the_search_and_the_commit_use_the_rows(oracle, chain_lib):
    from oracle.oracle import ALPHAS
    B, T, lim = 12, 20, 2.0
    g = handle(chain_lib, B, T, lim)
    rows = draw_rows(B, T + 1, 75)
    tw = knot_twins(oracle, rows, lim)
    g.set_knot_params(rows)
    x0 = chain_x0(B, seed=33)
    u0 = np.random.default_rng(3).normal(size=(B, T, NU)) * 0.3
    c0 = g.init_traj(x0, u0)
    xs, us = g.trajectory()
    g.compute_derivatives()
    g.backward_pass()
    k, K = g.gains()
    cands = g.rollout_candidates()
    assert cands.shape == (B, len(ALPHAS)) and np.abs(k).max() > 1e-3
    for a, alpha in enumerate(ALPHAS):
        _, _, c_o = knot_rollout(tw, x0, us, DT, xs_nom=xs, k=k, K=K, alpha=alpha)
        assert relcost(cands[:, a], c_o) < TOL, (a, relcost(cands[:, a], c_o))
    assert np.unique(np.round(cands[0], 9)).size == len(ALPHAS)  # (eleven different rollouts)
    # whole iterations: what is committed and costed is a rollout under the rows
    c0 = g.init_traj(x0, u0)
    g.iterate(4)
    xs4, us4 = g.trajectory()
    xs_o, _, c_o = knot_rollout(tw, x0, us4, DT)
    print("after four iterations: cost against the twins' re-roll %.2e, xs %.2e" % (relcost(g.cost(), c_o), relerr(xs4, xs_o)))
    assert relcost(g.cost(), c_o) < 1e-12
    assert np.all(g.cost() <= c0) and np.any(g.cost() < c0)
    g.close()


# ---- 4. equal rows reproduce the per-trajectory handle ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_equal_rows_reproduce_the_per_trajectory_handle(chain_lib, dtype):
    B, T, lim = 12, 20, 2.0
    rows = draw_rows(B, 1, 76)[:, 0]
    x0, x1 = chain_x0(B, seed=34), chain_x0(B, seed=35) * 0.9
    u0 = np.random.default_rng(4).normal(size=(B, T, NU)) * 0.3
    res = []
    for knot in (True, False):
        g = handle(chain_lib, B, T, lim, dtype=dtype)
        if knot:
            g.set_knot_params(np.repeat(rows[:, None], T + 1, axis=1))
        else:
            g.set_trajectory_params(rows)
        c_init = g.init_traj(x0, u0)
        g.iterate(3)
        mid = state(g)
        g.mpc_step(x0=x1, shift=1, iters=2)
        res.append(dict(init=c_init, **{"mid_" + kk: v for kk, v in mid.items()}, **state(g)))
        g.close()
    print("%s: equal knot rows give the per-trajectory handle's bits: %s" % (dtype, all(np.array_equal(res[0][kk], res[1][kk]) for kk in res[0])))
    for kk in res[0]:
        assert relerr(res[0][kk].reshape(B, -1), res[1][kk].reshape(B, -1)) < 1e-12, (kk, relerr(res[0][kk].reshape(B, -1), res[1][kk].reshape(B, -1)))


# ---- 5. tracking MPC from a long device reference, no host synchronisation ---------------------------------------------------------
def test_tracking_mpc_from_a_long_device_reference(chain_lib):
    """Four steps whose windows start at k0 = 1 .. 4 of a reference of T + 3 rows in device memory (the last two run past its end and hold
    the last row), with x0 from device memory and no host synchronisation between the calls: torch runs on a stream of its own and the
    handle is given that stream.  The same windows cut on the host (knot_window) with a synchronize() after every call leave the same state."""
    import torch
    B, T, lim = 9, 20, 2.0
    L = T + 3
    ref_rows = draw_rows(B, L, 77)
    x0 = chain_x0(B, seed=36)
    u0 = np.zeros((B, T, NU))
    x_next = [chain_x0(B, seed=80 + s) * 0.8 for s in range(4)]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        g = handle(chain_lib, B, T, lim, stream=stream.cuda_stream)
        g.set_knot_params(ref_rows, k0=0)
        g.init_traj(x0, u0)
        g.iterate(2)
        ref_dev = torch.tensor(ref_rows, dtype=torch.float64, device="cuda")
        x_dev = [torch.tensor(x, dtype=torch.float64, device="cuda") for x in x_next]
        stream.synchronize()
        for s in range(4):  # nothing below waits for the GPU
            g.set_knot_params(ptr=ref_dev.data_ptr(), n_knots=L, k0=1 + s)
            g.mpc_step(x0_ptr=x_dev[s].data_ptr(), shift=1, iters=2)
        g.synchronize()
    h = handle(chain_lib, B, T, lim)
    h.set_knot_params(knot_window(ref_rows, 0, T))
    h.synchronize()
    h.init_traj(x0, u0)
    h.iterate(2)
    h.synchronize()
    for s in range(4):
        h.set_knot_params(knot_window(ref_rows, 1 + s, T))
        h.synchronize()
        h.mpc_step(x0=x_next[s], shift=1, iters=2)
        h.synchronize()
    last = knot_window(ref_rows, 4, T)
    assert np.all(last[:, -3:] == ref_rows[:, -1:])  # (the window ran past the reference's end)
    assert np.array_equal(g.knot_params(), last) and np.array_equal(h.knot_params(), last)
    (xs, us), (xs_r, us_r) = g.trajectory(), h.trajectory()
    print("tracking from device rows: xs relerr %.2e us relerr %.2e cost relerr %.2e" % (relerr(xs, xs_r), relerr(us, us_r), relcost(g.cost(), h.cost())))
    assert relerr(xs, xs_r) < 1e-12 and relerr(us, us_r) < 1e-12 and relcost(g.cost(), h.cost()) < 1e-12
    g.close()
    h.close()
    del ref_dev, x_dev


# ---- 6. it tracks --------------------------------------------------------------------------------------------------------------------
def test_it_tracks(oracle, chain_lib):
    """The solution found under the knot rows costs less, under the knot rows, than the solution of the same problem with every knot's row
    replaced by the trajectory's mean row (its mean target): the moving target reached the optimiser."""
    B, T, lim = 8, 40, 2.0
    rows = draw_rows(B, T + 1, 78)
    assert np.all(rows[:, :, 7].max(axis=1) - rows[:, :, 7].min(axis=1) > 1.0)  # (the target swings)
    tw = knot_twins(oracle, rows, lim)
    x0 = chain_x0(B, seed=37) * 0.5
    u0 = np.zeros((B, T, NU))
    gk, gm = handle(chain_lib, B, T, lim), handle(chain_lib, B, T, lim)
    gk.set_knot_params(rows)
    gm.set_trajectory_params(rows.mean(axis=1))
    costs = []
    for g in (gk, gm):
        g.init_traj(x0, u0)
        g.iterate(10)
        costs.append(knot_rollout(tw, x0, g.trajectory()[1], DT)[2])
        g.close()
    print("tracking cost under the knot rows: solved with knot rows %s\n                                   solved with the mean row %s" % (costs[0], costs[1]))
    assert np.all(costs[0] < costs[1])


# ---- 7. evaluate_policy under knot rows ----------------------------------------------------------------------------------------------
def test_evaluate_policy_under_knot_rows(oracle, chain_lib):
    B, T, lim, S = 5, 12, 0.5, 3
    g = handle(chain_lib, B, T, lim)
    rows = draw_rows(B, T + 1, 79)
    tw = knot_twins(oracle, rows, lim)
    g.set_knot_params(rows)
    x0 = chain_x0(B, seed=38)
    g.init_traj(x0, np.zeros((B, T, NU)))
    g.iterate(3)
    xs, us = g.trajectory()
    _, K = g.gains()
    rng = np.random.default_rng(6)
    x = xs[:, 3][:, None, :] + 0.3 * rng.normal(size=(B, S, NX))
    for n in (T - 3, 2):
        got = {clamp: g.evaluate_policy(x, t0=3, n=n, clamp=clamp) for clamp in (False, True)}
        for clamp in (False, True):
            for s in range(S):
                xs_o, us_o, c_o = knot_rollout(tw, x[:, s], us, DT, xs_nom=xs, K=K, t0=3, n=n, clamp=(-lim, lim) if clamp else None)
                e = (relcost(got[clamp]["cost"][:, s], c_o), relerr(got[clamp]["x_end"][:, s], xs_o[:, -1]), relerr(got[clamp]["u_first"][:, s], us_o[:, 0]))
                assert max(e) < TOL, (n, clamp, s, e)
        assert not np.array_equal(got[False]["cost"], got[True]["cost"])  # (the clamp bit somewhere)
    # the whole horizon from a new state: the bits the warm start of mpc_step(shift = 0, iters = 0) leaves
    x_new = x0 + 0.05 * rng.normal(size=x0.shape)
    ev = g.evaluate_policy(x_new, t0=0, n=T)
    g.mpc_step(x0=x_new, shift=0, iters=0)
    xs_w, us_w = g.trajectory()
    assert np.array_equal(ev["cost"], g.cost()) and np.array_equal(ev["x_end"], xs_w[:, T]) and np.array_equal(ev["u_first"], us_w[:, 0])
    g.close()


# ---- 8. resets under knot rows ---------------------------------------------------------------------------------------------------------
def test_resets_under_knot_rows(oracle, chain_lib):
    B, T, lim = 6, 12, 2.0
    rows = draw_rows(B, T + 1, 81)
    tw = knot_twins(oracle, rows, lim)
    x0, x_new = chain_x0(B, seed=39), chain_x0(B, seed=40) * 0.9
    u0 = np.random.default_rng(8).normal(size=(B, T, NU)) * 0.3
    u_reset = np.random.default_rng(9).normal(size=(B, T, NU)) * 0.2
    mask = np.array([1, 0, 0, 1, 0, 1], dtype=np.int32)
    gr, gp = handle(chain_lib, B, T, lim), handle(chain_lib, B, T, lim)
    for g in (gr, gp):
        g.set_knot_params(rows)
        g.init_traj(x0, u0)
        g.iterate(2)
    gr.set_reset_controls(u_reset)
    gr.mpc_step(x0=x_new, shift=1, iters=0, reset_mask=mask)
    gp.mpc_step(x0=x_new, shift=1, iters=0)
    (xs, us), (xs_p, us_p) = gr.trajectory(), gp.trajectory()
    sel, rest = mask != 0, mask == 0
    xs_o, _, c_o = knot_rollout(tw, x_new, u_reset, DT)
    print("reset trajectories: xs relerr %.2e cost relerr %.2e" % (relerr(xs[sel], xs_o[sel]), relcost(gr.cost()[sel], c_o[sel])))
    assert np.array_equal(us[sel], u_reset[sel]) and relerr(xs[sel], xs_o[sel]) < 1e-12 and relcost(gr.cost()[sel], c_o[sel]) < 1e-12
    assert np.array_equal(xs[rest], xs_p[rest]) and np.array_equal(us[rest], us_p[rest]) and np.array_equal(gr.cost()[rest], gp.cost()[rest])
    assert not np.array_equal(xs[sel], xs_p[sel])
    gr.close()
    gp.close()


# ---- 9. fp32 against the float twins ---------------------------------------------------------------------------------------------------
def test_fp32_handle_against_the_float_twins(oracle, chain_lib):
    """The float rollouts' twin and the double twin of the finite differences both see the FLOAT-rounded rows: the rollout against the
    oracle's float-flavour per-knot twins, the records against the double twins of the float-rounded rows."""
    B, T, lim = 7, 10, 1.3
    g32 = handle(chain_lib, B, T, lim, dtype="f32")
    rows = draw_rows(B, T + 1, 82)
    rows[:, :, 0] += 1.0 / 3.0 * 1e-3
    assert np.mean(f32(rows) != rows) > 0.99
    g32.set_knot_params(rows)
    assert np.array_equal(g32.knot_params(), rows)  # stored as given; rounded where they are used
    x0 = f32(chain_x0(B, seed=41))
    u0 = f32(np.random.default_rng(10).normal(size=(B, T, NU)) * 0.3)
    cost = g32.init_traj(x0, u0)
    xs, us = g32.trajectory()
    with oracle.flavour("f32"):
        tw32 = knot_twins(oracle, f32(rows), f32(lim))
        xs32, _, c32 = knot_rollout(tw32, x0, u0, DT)
    xs32 = np.asarray(xs32, dtype=np.float64)
    print("fp32 rollout: xs relerr %.2e cost relerr %.2e" % (relerr(xs, xs32), relcost(cost, c32)))
    assert np.array_equal(us, u0) and np.array_equal(xs, f32(xs))
    assert relerr(xs, xs32) < TOL32 and relcost(cost, c32) < TOL32
    g32.compute_derivatives()
    check_records(g32.derivatives(), knot_records(knot_twins(oracle, f32(rows), f32(lim)), xs, us, DT), scale_noise=2.0 ** -23)
    g32.close()


# ---- 10. refusals and modes ------------------------------------------------------------------------------------------------------------
def test_refusals_and_modes(chain_lib):
    """Every refusal that needs a handle (B * (T + 1) * NTP beyond INT_MAX needs a handle of terabytes and is left to the code's reading),
    the getters in the wrong mode, the parameter gradient in knot mode, and the three modes one after the other."""
    from ilqr_amd import BatchILQR, _build, capi
    B, T, lim = 4, 10, 2.0
    ref = np.zeros((B, T + 1, NTP))
    p = ref.ctypes.data_as(capi._dp)
    out = np.zeros((B, T + 1, NTP))
    q = out.ctypes.data_as(capi._dp)
    # another model; the small twin on its tiled kernels: the handles that refuse per-trajectory rows, with the same messages
    g = BatchILQR("acrobot", B, T, DT)
    assert g.lib.ilqr_set_knot_params(g.h, p, None, NTP, T + 1, 0) == -5 and b"ilqr_set_knot_params" in g.lib.ilqr_last_error() and b"ILQR_MODEL_USER" in g.lib.ilqr_last_error()
    assert g.lib.ilqr_get_knot_params(g.h, q, NTP) == -5 and b"ILQR_MODEL_USER" in g.lib.ilqr_last_error()
    assert g.lib.ilqr_set_knot_params(g.h, p, p, NTP, T + 1, 0) == -1 and b"exactly one of p" in g.lib.ilqr_last_error()  # (the argument checks come first)
    assert g.lib.ilqr_set_knot_params(g.h, p, None, NTP, 3, 3) == -1 and b"k0 3 outside" in g.lib.ilqr_last_error()
    g.close()
    lib6 = _build.build_user(_build.USER_EXAMPLE6_HEADER, _build.USER_EXAMPLE6_LIB)
    g = BatchILQR("user", B, T, DT, u_min=-1.0, u_max=1.0, lib=lib6, nx=6, nu=2)
    assert g.lib.ilqr_set_knot_params(g.h, p, None, NTP, T + 1, 0) == -5 and b"ILQR_ROUTE_WAVE_PER_TRAJECTORY" in g.lib.ilqr_last_error()
    g.close()
    # the chain
    g, plain = handle(chain_lib, B, T, lim), handle(chain_lib, B, T, lim)
    lib = g.lib
    assert lib.ilqr_set_knot_params(g.h, p, None, 7, T + 1, 0) == -1 and b"n = 7" in lib.ilqr_last_error() and b"NTP = 8" in lib.ilqr_last_error()
    assert lib.ilqr_set_knot_params(g.h, None, None, NTP, T + 1, 0) == -1 and b"exactly one of p" in lib.ilqr_last_error()
    assert lib.ilqr_set_knot_params(g.h, p, None, NTP, 0, 0) == -1 and b"n_knots 0" in lib.ilqr_last_error()
    assert lib.ilqr_set_knot_params(g.h, p, None, NTP, T + 1, T + 1) == -1 and b"outside [0, n_knots" in lib.ilqr_last_error()
    assert lib.ilqr_get_knot_params(g.h, q, NTP) == -4 and b"no per-knot rows are set" in lib.ilqr_last_error()  # nothing above set anything
    with pytest.raises(ValueError):
        g.set_knot_params(ref, ptr=1)
    with pytest.raises(ValueError):
        g.set_knot_params(ptr=1)  # (a pointer needs n_knots)
    with pytest.raises(capi.ILQRError, match=r"error -1: .*n = 5"):
        g.set_knot_params(np.zeros((B, T + 1, 5)))
    x0 = chain_x0(B, seed=42)
    u0 = np.random.default_rng(11).normal(size=(B, T, NU)) * 0.3
    c_plain = plain.init_traj(x0, u0)
    rows = draw_rows(B, T + 1, 83)
    # knot mode: the per-trajectory getter and the parameter gradient refuse
    g.set_trajectory_params(rows[:, 0])  # (an earlier mode's rows, which nothing below may read)
    c_pt = g.init_traj(x0, u0)
    g.set_knot_params(rows)
    c_pk = g.init_traj(x0, u0)
    assert np.all(c_pk != c_pt) and np.all(c_pt != c_plain)
    with pytest.raises(capi.ILQRError, match=r"error -4: .*per-knot rows are set"):
        g.trajectory_params()
    assert lib.ilqr_get_knot_params(g.h, q, 7) == -1 and b"n = 7" in lib.ilqr_last_error()
    assert lib.ilqr_get_knot_params(g.h, None, NTP) == -1 and b"null array" in lib.ilqr_last_error()
    g.compute_derivatives()
    dxs = np.ones((B, T + 1, NX))
    with pytest.raises(capi.ILQRError, match=r"error -5: .*per-knot rows are set"):
        g.param_gradient(dxs=dxs)
    gp = np.zeros((B, 1, NTP))
    assert lib.ilqr_param_gradient_on_device(g.h, 1, 0, 0.0, dxs.ctypes.data, None, None, gp.ctypes.data, None) == -5  # (refused before the host addresses are touched)
    assert b"per-knot rows are set" in lib.ilqr_last_error()
    # back to one row per trajectory: the knot getter refuses, the rows and the results are the per-trajectory ones
    g.set_trajectory_params(rows[:, 0])
    with pytest.raises(capi.ILQRError, match=r"error -4: .*no per-knot rows are set"):
        g.knot_params()
    assert np.array_equal(g.trajectory_params(), rows[:, 0]) and np.array_equal(g.init_traj(x0, u0), c_pt)
    g.compute_derivatives()
    assert np.all(np.isfinite(g.param_gradient(dxs=dxs)))
    # ... and into knot mode again, then clear: the handle-wide parameters, to the bit, and both getters refuse
    g.set_knot_params(rows)
    assert np.array_equal(g.init_traj(x0, u0), c_pk)
    g.clear_trajectory_params()
    assert np.array_equal(g.init_traj(x0, u0), c_plain)
    g.iterate(2)
    plain.iterate(2)
    for a, b in zip(state(g).values(), state(plain).values()):
        assert np.array_equal(a, b)
    for call in (g.knot_params, g.trajectory_params):
        with pytest.raises(capi.ILQRError, match=r"error -4"):
            call()
    g.close()
    plain.close()
