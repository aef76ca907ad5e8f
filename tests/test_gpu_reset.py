"""Single trajectories start over inside a receding-horizon step, on the device (ilqr_mpc_step_reset, ilqr_reset_trajectories,
ilqr_set_reset_controls, ilqr_get_reset_flags).

- mpc_step with a reset mask equals its host composition (shift, download, overwrite the selected rows, upload, mpc_step(shift=0)) bit for
  bit on every kind of route, with zero reset controls and with reset controls from device memory;
- selecting nobody changes nothing: the step is ilqr_mpc_step's, and the repeated rollout of the non-finite rule is the identity;
- a reset trajectory is a fresh one (init_traj from the new state and the reset controls);
- a trajectory poisoned with NaN recovers under the non-finite rule while the others keep their bits;
- the lambda_max rule; the standalone call against numpy, the flags in device memory, what is refused; no host synchronisation needed."""
import numpy as np
import pytest

from tests.util import TOL, acrobot_x0, integrator_x0, relerr

pytestmark = pytest.mark.gpu
DT = 0.02
B, T = 37, 45  # B: not a multiple of 16 or 64 (partial tiles, padding lanes); T: not a multiple of 8 (tests/test_gpu_mpc.py)
ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5
SEL = np.array([0, 15, 16, 31, 36])  # both sides of a tile boundary, and the last real trajectory of the partial tile
KEYS = ("xs", "us", "k", "K", "cost", "lam", "dlam")
CHAIN_PARAMS = np.array([9.81, 0.1, 2.0, 10.0, 1.0, 0.1, 50.0, 0.0])
ROUTES = {  # tests/test_gpu_mpc.py's table -- name: (problem, extra constructor kwargs, kernel the route must run)
    "acrobot_hex": ("acrobot", dict(), ("solve", "k_solve_hex")),
    "acrobot_quad_chain": ("acrobot", dict(route=256), ("solve", "k_solve_tile")),
    "acrobot_staged": ("acrobot", dict(flags=32), ("backward", "k_sweep_backward")),
    "acrobot_wide": ("acrobot", dict(route=3), ("solve", "k_solve_wide")),
    "acrobot_f32": ("acrobot", dict(dtype="f32"), None),
    "acrobot_fixes": ("acrobot", dict(flags=64), None),
    "integrator": ("integrator", dict(), None),
    "integrator_wide2": ("integrator", dict(route=3), ("solve", "k_solve_wide2")),
    "lq_fd": ("lq", dict(), ("rollout", "k_rollout_lq")),
    "lq_fused": ("lq", dict(flags=16), ("derivatives", "")),
    "lq_f32": ("lq", dict(dtype="f32"), ("rollout", "k_rollout_g")),
    "lq20": ("lq20", dict(), ("backward", "k_backward_w3w")),
    "chain": ("chain", dict(), ("backward", "k_backward_w3")),
}


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """masks, reset controls and x0 live in torch tensors here: torch's device is initialised before this module creates any handle
    (tests/test_gpu_mpc.py)"""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


@pytest.fixture(scope="module")
def chain_lib():
    import os
    from ilqr_amd import _build
    if not os.path.exists(_build.USER_CHAIN_LIB) and not os.path.exists(_build.HIPCC):
        pytest.skip("the pendulum-chain build is missing and there is no hipcc to make it")
    return _build.build_user(_build.USER_CHAIN_HEADER, _build.USER_CHAIN_LIB)


def problem(name, chain_lib=None):
    """(constructor kwargs, x0 [B][nx], nu) of a named handle"""
    from tests.test_gpu_lq_end_to_end import dense_mats
    rng = np.random.default_rng(5)
    if name.startswith("acrobot"):
        return dict(model="acrobot", u_min=-1.5, u_max=1.5), acrobot_x0(B, scale=0.3, seed=4), 1
    if name.startswith("integrator"):
        return dict(model="integrator", goal=[1, .5, 0, 0]), integrator_x0(B), 2
    if name.startswith("lq20"):
        return dict(model="lq", lq=dense_mats(8, 20), u_min=-0.4, u_max=0.4), rng.uniform(-1, 1, (B, 8)), 20
    if name.startswith("lq"):
        return dict(model="lq", lq=dense_mats(6, 3), u_min=-0.4, u_max=0.4), rng.uniform(-1, 1, (B, 6)), 3
    if name.startswith("chain"):
        x0 = np.concatenate([rng.uniform(-1, 1, (B, 8)), rng.uniform(-1, 1, (B, 8)) * 0.5], axis=1)
        return dict(model="user", lib=chain_lib, nx=16, nu=4, u_min=-2.0, u_max=2.0, user_params=CHAIN_PARAMS), x0, 4
    raise KeyError(name)


def make(kw, **extra):
    from ilqr_amd import BatchILQR
    kw = dict(kw, **extra)
    return BatchILQR(kw.pop("model"), B, T, DT, **kw)


def snapshot(g):
    xs, us = g.trajectory()
    k, K = g.gains()
    lam, dlam = g.lambdas()
    return dict(xs=xs, us=us, k=k, K=K, cost=g.cost(), lam=lam, dlam=dlam)


def load(g, s, x0=None):
    """the state `s` (a snapshot) into a handle, through the setters"""
    g.set_trajectory(x0=x0, xs=s["xs"], us=s["us"], cost=s["cost"])
    g.set_gains(k=s["k"], K=s["K"])
    g.set_lambda(s["lam"], s["dlam"])


def assert_same(a, b, keys=KEYS, rows=None, what=None):
    for key in keys:
        x, y = (a[key], b[key]) if rows is None else (a[key][rows], b[key][rows])
        assert np.array_equal(x, y), (key, what)


def np_shift(s, n):
    """include/ilqr_amd.h, ILQR_TAIL_HOLD: knots n later; the tail holds the last knot (xs, us, K) or is zero (k)"""
    out = {key: np.array(v) for key, v in s.items()}
    if n == 0:
        return out
    Tn = s["us"].shape[1]
    out["xs"][:, :Tn + 1 - n] = s["xs"][:, n:]
    out["xs"][:, Tn + 1 - n:] = s["xs"][:, Tn:]
    for key, hold in (("us", True), ("k", False), ("K", True)):
        out[key][:, :Tn - n] = s[key][:, n:]
        out[key][:, Tn - n:] = s[key][:, Tn - 1:] if hold else 0.0
    return out


def np_reset(s, rows, u_reset, lam0=1.0, dlam0=1.0):
    """include/ilqr_amd.h, what a reset is -- the arrays a snapshot holds: us = the reset controls, xs = k = K = 0, lambda and dlambda initial"""
    out = {key: np.array(v) for key, v in s.items()}
    for key in ("xs", "k", "K"):
        out[key][rows] = 0.0
    out["us"][rows] = 0.0 if u_reset is None else u_reset[rows]
    out["lam"][rows] = lam0
    out["dlam"][rows] = dlam0
    return out


def mask_of(rows):
    m = np.zeros(B, dtype=np.int32)
    m[rows] = 1
    return m


def solved(route, chain_lib, seed=17):
    """(kw, extra, x0, nu, snapshot) of the route's handle after init_traj and iterate(4): lambda moved, gains of its own; and the handle"""
    pname, extra, kernel = ROUTES[route]
    kw, x0, nu = problem(pname, chain_lib)
    H = make(kw, **extra)
    if kernel:
        from ilqr_amd import capi
        assert H.lib.ilqr_stage_kernel_name(H.h, capi.STAGE_NAMES.index(kernel[0])).decode() == kernel[1], route
    H.init_traj(x0, 0.1 * np.random.default_rng(seed).standard_normal((B, T, nu)))
    H.iterate(4)
    return kw, extra, x0, nu, snapshot(H), H


# ---- 1. mpc_step(reset_mask) == shift, overwrite the selected rows on the host, upload, mpc_step(shift = 0) --------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_masked_step_equals_the_host_composition(route, chain_lib):
    import torch
    kw, extra, x0, nu, ref, H = solved(route, chain_lib)
    rng = np.random.default_rng(29)
    u_reset = 0.2 * rng.standard_normal((B, T, nu))
    u_dev = torch.from_numpy(u_reset).cuda()
    torch.cuda.synchronize()
    mask = mask_of(SEL)
    for controls in (None, u_reset):
        for n in (0, 3):
            # handles with the budget n: the composition's, and a fresh one for the device call (status and iteration counts compare there)
            Cm, D = make(kw, params=dict(max_iter=n), **extra), make(kw, params=dict(max_iter=n), **extra)
            for g in (H, D):
                g.set_reset_controls(ptr=None if controls is None else u_dev.data_ptr())
            for s in (0, 7):
                x_new = ref["xs"][:, s] + 0.01 * rng.standard_normal(x0.shape)
                what = (route, "zeros" if controls is None else "device controls", n, s)
                # the composition: shift on the device, download, overwrite the selected rows, upload, ilqr_mpc_step(shift = 0)
                load(Cm, ref, x0)
                Cm.shift_horizon(s)
                shifted = snapshot(Cm)
                assert_same(shifted, np_shift(ref, s), what=what)
                load(Cm, np_reset(shifted, SEL, controls))
                Cm.mpc_step(x0=x_new, shift=0, iters=n)
                want, want_st = snapshot(Cm), Cm.status()
                # (a) on the solved handle itself: whatever hidden state it carries must not show
                load(H, ref, x0)
                H.mpc_step(x0=x_new, shift=s, iters=n, reset_mask=mask)
                assert_same(snapshot(H), want, what=what)
                assert np.array_equal(H.reset_flags(), mask), what
                # (b) on the fresh handle with the same budget: status and iteration counts too
                load(D, ref, x0)
                D.mpc_step(x0=x_new, shift=s, iters=n, reset_mask=mask)
                assert_same(snapshot(D), want, what=what)
                for a, b in zip(D.status()[:2], want_st[:2]):
                    assert np.array_equal(a, b), what
            Cm.close()
            D.close()
    H.close()
    del u_dev


# ---- 2. selecting nobody changes nothing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_no_selection_is_the_plain_step(route, chain_lib):
    import torch
    from ilqr_amd import capi
    kw, extra, x0, nu, ref, H = solved(route, chain_lib)
    x_new = ref["xs"][:, 1] + 0.01 * np.random.default_rng(3).standard_normal(x0.shape)
    H.mpc_step(x0=x_new, shift=1, iters=3)
    want = snapshot(H)
    zeros = torch.zeros(B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    xh = np.ascontiguousarray(x_new)
    xp = xh.ctypes.data_as(capi._dp)
    # no mask and no rules (the entry point itself: BatchILQR.mpc_step without reset arguments calls ilqr_mpc_step); an all-zero device
    # mask; the non-finite rule on a finite batch -- the repeated rollout is the identity
    for what, call in (("no mask, no rules", lambda g: g._check(g.lib.ilqr_mpc_step_reset(g.h, xp, None, 1, capi.TAIL_HOLD, 3, None, None, 0))),
                       ("zero device mask", lambda g: g.mpc_step(x0=x_new, shift=1, iters=3, reset_mask_ptr=zeros.data_ptr())),
                       ("non-finite rule, finite batch", lambda g: g.mpc_step(x0=x_new, shift=1, iters=3, reset_nonfinite=True))):
        load(H, ref, x0)
        call(H)
        assert_same(snapshot(H), want, what=(route, what))
        assert np.array_equal(H.reset_flags(), np.zeros(B, dtype=np.int32)), (route, what)
    assert np.all(np.isfinite(want["cost"]))
    H.close()


# ---- 3. a reset trajectory is a fresh one ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["acrobot_hex", "acrobot_f32", "lq_fd", "chain"])
def test_a_reset_trajectory_is_a_fresh_one(route, chain_lib):
    """The selected rows after mpc_step(reset_mask, iters=0) against init_traj(x_new, u_reset) on a second handle: xs, us and cost within
    the project's per-knot tolerance (fp32: tests/parity.py's TOL32, as tests/test_gpu_fp32.py).  Expected difference: 0 -- with K = 0 and
    k = 0 the warm rollout's u = us[t] + 0 alpha + 0 (x - 0) is us[t], and the rest is the same expression sequence.
    The measured maximum is printed."""
    from tests.parity import TOL32
    kw, extra, x0, nu, ref, H = solved(route, chain_lib)
    tol = TOL32 if extra.get("dtype") == "f32" else TOL
    rng = np.random.default_rng(41)
    u_reset = 0.2 * rng.standard_normal((B, T, nu))
    x_new = ref["xs"][:, 1] + 0.01 * rng.standard_normal(x0.shape)
    H.set_reset_controls(u_reset)
    H.mpc_step(x0=x_new, shift=1, iters=0, reset_mask=mask_of(SEL))
    got = snapshot(H)
    F = make(kw, **extra)
    F.init_traj(x_new, u_reset)
    want = snapshot(F)
    errs = dict(xs=relerr(got["xs"][SEL], want["xs"][SEL]), us=relerr(got["us"][SEL], want["us"][SEL]),
                cost=float(np.max(np.abs(got["cost"][SEL] - want["cost"][SEL]) / np.abs(want["cost"][SEL]))))
    print("reset vs fresh", route, errs)
    assert all(e < tol for e in errs.values()), (route, errs)
    assert np.all(got["k"][SEL] == 0) and np.all(got["K"][SEL] == 0) and np.all(got["lam"][SEL] == 1.0) and np.all(got["dlam"][SEL] == 1.0)
    H.close()
    F.close()


# ---- 4. a poisoned trajectory recovers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["acrobot_hex", "acrobot_f32", "lq_fd", "chain"])
def test_nonfinite_trajectories_recover_and_the_others_keep_their_bits(route, chain_lib):
    """NaN in K of two trajectories.  (No call here iterates a non-finite trajectory: NaNs only pass through rollouts, whose loops are straight
    over T.)"""
    kw, extra, x0, nu, ref, H = solved(route, chain_lib)
    bad = np.array([3, 20])
    rest = np.setdiff1d(np.arange(B), bad)
    x_new = ref["xs"][:, 1] + 0.01 * np.random.default_rng(7).standard_normal(x0.shape)
    poisoned = {key: np.array(v) for key, v in ref.items()}
    poisoned["K"][bad] = np.nan
    G = make(kw, **extra)

    def run(state, **step):
        load(G, state, x0)
        G.mpc_step(x0=x_new, shift=1, **step)
        return snapshot(G), G.reset_flags() if any(k.startswith("reset") for k in step) else None

    # the control case: the plain step leaves them non-finite for good, and nobody else notices
    plain0, _ = run(ref, iters=0)
    dead, _ = run(poisoned, iters=0)
    assert not np.any(np.isfinite(dead["cost"][bad])), route
    assert_same(dead, plain0, rows=rest, what=(route, "control case"))
    # the rule: flagged exactly there, every cost finite, the others as if nothing had happened, the two as a masked reset of the same two
    plain3, _ = run(ref, iters=3)
    masked3, _ = run(ref, iters=3, reset_mask=mask_of(bad))
    got, flags = run(poisoned, iters=3, reset_nonfinite=True)
    want_flags = np.zeros(B, dtype=np.int32)
    want_flags[bad] = 2
    assert np.array_equal(flags, want_flags), (route, flags)
    assert np.all(np.isfinite(got["cost"])), route
    assert_same(got, plain3, rows=rest, what=(route, "the other 35"))
    assert_same(got, masked3, rows=bad, what=(route, "the two"))
    G.close()
    H.close()


# ---- 5. the lambda_max rule ----------------------------------------------------------------------------------------------------------------
def test_lambda_max_exits_are_reset():
    """A strict search under a low ceiling (tests/test_gpu_accept_schedule.py's P2) leaves trajectories at status 3.  The initial states
    (acrobot_x0(scale=0.3, seed=4)) and the six iterations were picked with the CPU oracle: oracle.batch_solve under the same tunables
    leaves 15 of the 37 at lambda_max after six iterations (19 running) -- far from both ends of the condition below, which fails the test
    rather than skipping it."""
    P2 = dict(z_min=0.9, lambda_factor=2.5, lambda_max=50.0, max_iter=10)
    kw, x0, nu = problem("acrobot")
    ga, gb = make(kw, params=P2), make(kw, params=P2)
    for g in (ga, gb):
        g.init_traj(x0, np.zeros((B, T, nu)))
        g.iterate(6)
    st = ga.status()[0]
    at_max = st == 3
    assert 1 <= int(at_max.sum()) <= B - 1, np.bincount(st, minlength=5)
    assert np.array_equal(gb.status()[0], st)
    x_new = ga.trajectory()[0][:, 1]
    ga.mpc_step(x0=x_new, shift=1, iters=0, reset_lambda_max=True)
    gb.mpc_step(x0=x_new, shift=1, iters=0)
    assert np.array_equal(ga.reset_flags(), np.where(at_max, 4, 0).astype(np.int32))
    a, b = snapshot(ga), snapshot(gb)
    assert np.all(a["lam"][at_max] == 1.0) and np.all(a["dlam"][at_max] == 1.0)  # (ilqr_default_params: lambda_init = dlambda_init = 1)
    assert np.any(b["lam"][at_max] != 1.0)  # the plain step keeps the lambda that ran into the ceiling
    assert np.all(a["k"][at_max] == 0) and np.all(a["K"][at_max] == 0) and np.all(a["us"][at_max] == 0)
    assert_same(a, b, rows=~at_max, what="iters=0")
    for g in (ga, gb):
        g.iterate(2)
    assert_same(snapshot(ga), snapshot(gb), rows=~at_max, what="two iterations later")
    assert np.all(np.isfinite(snapshot(ga)["cost"]))
    ga.close()
    gb.close()


# ---- 6. the standalone call, the flags in device memory, refusals -----------------------------------------------------------------------
def test_standalone_reset_on_a_host_evaluated_handle_and_refusals():
    import torch
    from ilqr_amd import BatchILQR, capi
    rng = np.random.default_rng(2)
    nx, nu = 5, 3
    hm = BatchILQR("host", B, T, DT, nx=nx, nu=nu, u_min=-1.0, u_max=1.0)
    ip = capi._ip
    m_h = mask_of(SEL)
    m_d = torch.from_numpy(m_h).cuda()
    u_h = np.ascontiguousarray(rng.normal(size=(B, T, nu)))
    u_d = torch.from_numpy(u_h).cuda()
    flags_d = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    x5 = np.ascontiguousarray(rng.normal(size=(B, nx)))
    # before a trajectory exists
    assert hm.lib.ilqr_reset_trajectories(hm.h, m_h.ctypes.data_as(ip), None, 0) == ERR_STATE
    assert np.array_equal(hm.reset_flags(), np.zeros(B, dtype=np.int32))
    state = dict(xs=rng.normal(size=(B, T + 1, nx)), us=rng.normal(size=(B, T, nu)), k=rng.normal(size=(B, T, nu)),
                 K=rng.normal(size=(B, T, nu, nx)), cost=rng.normal(size=B), lam=rng.uniform(1, 9, B), dlam=rng.uniform(1, 2, B))
    state["cost"][[5, 15]] = np.nan   # 15 is masked as well
    state["cost"][9] = np.inf
    state["cost"][10] = -np.inf
    load(hm, state, state["xs"][:, 0])
    # refused, and nothing changed: two mask pointers, unknown rule bits, two control pointers, the step on a host-evaluated model
    assert hm.lib.ilqr_reset_trajectories(hm.h, m_h.ctypes.data_as(ip), m_d.data_ptr(), 0) == ERR_INVALID
    assert hm.lib.ilqr_reset_trajectories(hm.h, None, None, 4) == ERR_INVALID
    assert hm.lib.ilqr_reset_trajectories(hm.h, None, None, -1) == ERR_INVALID
    assert hm.lib.ilqr_set_reset_controls(hm.h, u_h.ctypes.data_as(capi._dp), u_d.data_ptr()) == ERR_INVALID
    assert hm.lib.ilqr_mpc_step_reset(hm.h, x5.ctypes.data_as(capi._dp), None, 1, capi.TAIL_HOLD, 1, None, None, 0) == ERR_UNSUPPORTED
    got = snapshot(hm)
    for key in KEYS:
        assert np.array_equal(got[key], state[key], equal_nan=True), key
    # mask only, zero controls, from a host mask
    hm.reset_trajectories(mask=m_h)
    want = np_reset(state, SEL, None)
    got = snapshot(hm)
    for key in KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    assert np.array_equal(hm.reset_flags(), m_h)
    # device mask + the non-finite rule, reset controls from device memory; the flags in device memory equal the getter's
    load(hm, state, state["xs"][:, 0])
    hm.set_reset_controls(ptr=u_d.data_ptr())
    hm.reset_trajectories(mask_ptr=m_d.data_ptr(), nonfinite=True)
    nonfin = np.array([5, 9, 10, 15])
    want = np_reset(state, np.union1d(SEL, nonfin), u_h)
    got = snapshot(hm)
    for key in KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    want_flags = m_h.copy()
    want_flags[nonfin] |= 2
    assert want_flags[15] == 3
    assert np.array_equal(hm.reset_flags(), want_flags)
    hm.copy_reset_flags_to_device(flags_d.data_ptr())
    hm.synchronize()
    assert np.array_equal(flags_d.cpu().numpy(), want_flags)
    st, it, _ = hm.status()
    assert np.all(st == 0) and np.all(it == 0)
    # rules only; host controls; back to zeros
    load(hm, state, state["xs"][:, 0])
    hm.set_reset_controls(2.0 * u_h)
    hm.reset_trajectories(nonfinite=True)
    want = np_reset(state, nonfin, 2.0 * u_h)
    assert np.array_equal(snapshot(hm)["us"], want["us"]) and np.array_equal(hm.reset_flags(), np.where(np.isin(np.arange(B), nonfin), 2, 0))
    load(hm, state, state["xs"][:, 0])
    hm.set_reset_controls()
    hm.reset_trajectories(mask=m_h)
    assert np.all(snapshot(hm)["us"][SEL] == 0)
    hm.close()
    # a device model: the step's own refusals
    kw, x0, nu1 = problem("acrobot")
    g = make(kw)
    xp = np.ascontiguousarray(x0).ctypes.data_as(capi._dp)
    assert g.lib.ilqr_mpc_step_reset(g.h, xp, None, 1, capi.TAIL_HOLD, 1, m_h.ctypes.data_as(ip), None, 0) == ERR_STATE
    assert g.lib.ilqr_reset_trajectories(g.h, None, None, 3) == ERR_STATE
    g.init_traj(x0, np.zeros((B, T, nu1)))
    g.iterate(1)
    ref = snapshot(g)
    assert g.lib.ilqr_mpc_step_reset(g.h, xp, None, 1, capi.TAIL_HOLD, 1, m_h.ctypes.data_as(ip), m_d.data_ptr(), 0) == ERR_INVALID
    assert g.lib.ilqr_mpc_step_reset(g.h, xp, None, 1, capi.TAIL_HOLD, 1, None, None, 8) == ERR_INVALID
    assert g.lib.ilqr_mpc_step_reset(g.h, xp, None, T, capi.TAIL_HOLD, 1, None, None, 0) == ERR_INVALID
    assert g.lib.ilqr_mpc_step_reset(g.h, None, None, 1, capi.TAIL_HOLD, 1, None, None, 0) == ERR_INVALID
    assert_same(snapshot(g), ref, what="refused calls change nothing")
    g.close()
    del m_d, u_d


# ---- 7. nothing waits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", [("acrobot", "f64"), ("lq", "f32")])
def test_steps_with_masks_from_the_stream_need_no_synchronisation(name, dtype):
    """Three steps whose masks and x0 torch writes on the handle's stream between the calls, with no host synchronisation (the stream rule of
    ilqr_amd/batch.py, as tests/test_gpu_traj_params.py); the same steps from host arrays with a synchronize() after every call leave the
    same state."""
    import torch
    kw, x0, nu = problem(name)
    rng = np.random.default_rng(11)
    u0 = 0.1 * rng.standard_normal((B, T, nu))
    u_reset = 0.05 * rng.standard_normal((B, T, nu))
    x_news = [x0 + 0.02 * (i + 1) * rng.standard_normal(x0.shape) for i in range(3)]
    masks = [(np.arange(B) % 5 == i).astype(np.int32) for i in range(3)]
    stream = torch.cuda.Stream()  # (torch's default stream is the null stream: a handle given stream 0 makes its own)
    with torch.cuda.stream(stream):
        gd = make(kw, dtype=dtype, stream=stream.cuda_stream)
        gd.init_traj(x0, u0)
        gd.iterate(3)
        keep = [torch.from_numpy(u_reset).cuda(non_blocking=True)]
        gd.set_reset_controls(ptr=keep[0].data_ptr())
        lanes = torch.arange(B, device="cuda")
        flags = torch.full((3, B), -1, dtype=torch.int32, device="cuda")
        for i in range(3):
            xd = torch.from_numpy(x_news[i]).cuda(non_blocking=True)
            md = (lanes % 5 == i).to(torch.int32)  # written by a torch kernel on the handle's stream
            keep += [xd, md]
            gd.mpc_step(x0_ptr=xd.data_ptr(), shift=1, iters=2, reset_mask_ptr=md.data_ptr(), reset_nonfinite=True)
            gd.copy_reset_flags_to_device(flags[i].data_ptr())
        stream.synchronize()
        got, got_flags = snapshot(gd), flags.cpu().numpy()
        gd.close()
    gh = make(kw, dtype=dtype)
    gh.init_traj(x0, u0)
    gh.iterate(3)
    gh.set_reset_controls(u_reset)
    gh.synchronize()
    for i in range(3):
        gh.mpc_step(x0=x_news[i], shift=1, iters=2, reset_mask=masks[i], reset_nonfinite=True)
        gh.synchronize()
        assert np.array_equal(gh.reset_flags(), got_flags[i]) and np.array_equal(got_flags[i], masks[i]), i
    assert_same(got, snapshot(gh), what=(name, dtype))
    gh.close()
    del keep
