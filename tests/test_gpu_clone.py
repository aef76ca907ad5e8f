"""Multi-start groups on the device (ilqr_select_best, ilqr_clone_trajectories, ilqr_clone_best, ilqr_get_clone_flags).

- the gather equals numpy's on every kind of route, and a clone is its source from then on;
- the perturbation du: added in double, rounded to the storage type, read for cloned rows only, and the cost stays the source's until the
  next warm rollout;
- select_best against a numpy restatement of its rule (non-finite costs never win, ties go to the lowest index);
- clone_best is select_best + clone_trajectories; the source rule; what is refused; host-evaluated handles.
Every comparison is bit for bit."""
import numpy as np
import pytest

from tests.util import acrobot_x0, integrator_x0

pytestmark = pytest.mark.gpu
DT = 0.02
B, T = 40, 45  # tiles of 16 + 16 + 8: a partial tile and padding lanes; T: not a multiple of 8 (tests/test_gpu_mpc.py)
ERR_INVALID, ERR_STATE = -1, -4
KEYS = ("xs", "us", "k", "K", "cost", "lam", "dlam", "dV", "gnorm", "status", "iters", "alpha_idx")
CHAIN_PARAMS = np.array([9.81, 0.1, 2.0, 10.0, 1.0, 0.1, 50.0, 0.0])
ROUTES = {  # tests/test_gpu_reset.py's table -- name: (problem, extra constructor kwargs, kernel the route must run)
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
# The explicit map: b <- SRC_MAP[b] for the rows named here, identity for the rest.
#   3 <- 9    a source in the same tile                  5 <- 20, 17 <- 2   sources in another tile (20 keeps itself through a -1 entry)
#   37 <- 12  a destination in the partial tile           33 <- 38          source and destination both in the partial tile
#   7, 20, 25: -1 entries                                                    everyone else: an identity entry
CLONED = {3: 9, 5: 20, 17: 2, 37: 12, 33: 38}
MINUS_ONE = (7, 20, 25)


def explicit_map():
    src = np.arange(B, dtype=np.int32)
    for b, s in CLONED.items():
        src[b] = s
    src[list(MINUS_ONE)] = -1
    return src


def effective(src):
    """include/ilqr_amd.h's source rule restated: (the row every trajectory holds afterwards, the flags)"""
    eff, flags = np.arange(B), np.zeros(B, dtype=np.int32)
    for b in range(B):
        s = int(src[b])
        if s < 0 or s == b:
            continue
        if s < B and (src[s] == s or src[s] < 0):
            eff[b], flags[b] = s, 1
        else:
            flags[b] = 2
    return eff, flags


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """maps, du and flags live in torch tensors here: torch's device is initialised before this module creates any handle
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
    """(constructor kwargs, x0 [B][nx], nu) of a named handle: distinct initial states"""
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
    status, iters, alpha_idx = g.status()
    return dict(xs=xs, us=us, k=k, K=K, cost=g.cost(), lam=lam, dlam=dlam, dV=g.dV(), gnorm=g.gnorm(), status=status, iters=iters,
                alpha_idx=alpha_idx)


def assert_rows(got, want, rows_got, rows_want, what, keys=KEYS):
    for key in keys:
        assert np.array_equal(got[key][rows_got], want[key][rows_want]), (key, what)


def solved(route, chain_lib, seed=17):
    """the route's handle after init_traj from distinct states and controls and iterate(4), and (x0, nu)"""
    pname, extra, kernel = ROUTES[route]
    kw, x0, nu = problem(pname, chain_lib)
    H = make(kw, **extra)
    if kernel:
        from ilqr_amd import capi
        assert H.lib.ilqr_stage_kernel_name(H.h, capi.STAGE_NAMES.index(kernel[0])).decode() == kernel[1], route
    H.init_traj(x0, 0.1 * np.random.default_rng(seed).standard_normal((B, T, nu)))
    H.iterate(4)
    return H, x0, nu


def storage(a, f32):
    return a.astype(np.float32).astype(np.float64) if f32 else a


# ---- 1. the gather equals numpy's, every route ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_the_gather_equals_numpy(route, chain_lib):
    H, _, _ = solved(route, chain_lib)
    before = snapshot(H)
    src = explicit_map()
    eff, flags = effective(src)
    assert sorted(np.flatnonzero(flags == 1)) == sorted(CLONED) and not np.any(flags == 2)
    assert not np.array_equal(before["xs"][3], before["xs"][9])  # (distinct trajectories: the gather is visible)
    H.clone_trajectories(src=src)
    after = snapshot(H)
    assert_rows(after, before, np.arange(B), eff, route)
    assert np.array_equal(H.clone_flags(), flags), route
    assert H.lib.ilqr_get_candidate(H.h, 0, None, None) == ERR_STATE, route  # the candidates belong to nobody
    H.close()


# ---- 2. a clone is its source from then on, every route ------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_a_clone_is_its_source_from_then_on(route, chain_lib):
    """Two more iterations after the clone: every getter's row b equals row src[b].  x0, diverge and backpass_done have no getter -- they
    show here (a clone that kept its own x0 rolls out from another state).  flgChange has none either and is 1 in a clone whatever the
    source's: the derivative records stay the slot's, so on the routes whose sweep skips an unchanged trajectory (acrobot_staged, the
    generic ones) a clone of a source whose last search accepted nothing -- most acrobot rows here -- must have them recomputed to stay
    equal.  Rests on a trajectory's bits not depending on its slot (tests/test_gpu_fp32.py: 8 shards equal one handle)."""
    H, _, _ = solved(route, chain_lib)
    src = explicit_map()
    eff, _ = effective(src)
    H.clone_trajectories(src=src)
    H.iterate(2)
    after = snapshot(H)
    assert_rows(after, after, np.arange(B), eff, route)
    H.close()


# ---- 3. the perturbation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["acrobot_hex", "acrobot_f32", "chain"])
def test_du_is_added_to_the_cloned_controls_only(route, chain_lib):
    import torch
    H, x0, nu = solved(route, chain_lib)
    f32 = ROUTES[route][1].get("dtype") == "f32"
    before = snapshot(H)
    src = explicit_map()
    eff, flags = effective(src)
    cloned = np.flatnonzero(flags == 1)
    rest = np.setdiff1d(np.arange(B), cloned)
    du = 0.05 * np.random.default_rng(23).standard_normal((B, T, nu))
    du[rest] = np.nan  # rows of trajectories that are not cloned are not read
    du_d = torch.from_numpy(du).cuda()
    src_d = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    H.clone_trajectories(src_ptr=src_d.data_ptr(), du_ptr=du_d.data_ptr())
    after = snapshot(H)
    assert np.array_equal(after["us"][cloned], storage(before["us"][eff[cloned]] + du[cloned], f32)), route
    assert not np.array_equal(after["us"][cloned], before["us"][eff[cloned]])
    assert_rows(after, before, np.arange(B), eff, route, keys=[k for k in KEYS if k != "us"])  # xs, k, K, cost: the source's
    assert np.array_equal(after["us"][rest], before["us"][rest]), route
    assert np.array_equal(H.clone_flags(), flags), route
    # the next warm rollout costs the perturbed controls
    H.mpc_step(x0=x0, shift=0, iters=0)
    cost = H.cost()
    assert np.all(np.isfinite(cost)), route
    assert np.all(cost[cloned] != cost[eff[cloned]]), route
    H.close()
    del du_d, src_d


# ---- 4. select_best against numpy ------------------------------------------------------------------------------------------------------------
def np_best(c, G):
    """the rule restated: ascending scan with a strict <, finite costs only; a group without one maps everyone to itself"""
    src = np.arange(B, dtype=np.int32)
    for g0 in range(0, B, G):
        best = -1
        for i in range(g0, g0 + G):
            if np.isfinite(c[i]) and (best < 0 or c[i] < c[best]):
                best = i
        if best >= 0:
            src[g0:g0 + G] = best
    return src


@pytest.fixture(scope="module")
def costed_handle():
    kw, x0, nu = problem("acrobot")
    H = make(kw)
    H.init_traj(x0, np.zeros((B, T, nu)))
    yield H
    H.close()


@pytest.mark.parametrize("G", [1, 4, 5, 8, 20, 40])
def test_select_best_against_numpy(G, costed_handle):
    import torch
    H = costed_handle
    base = np.random.default_rng(31).normal(size=B) * 10.0
    plantings = []
    c = base.copy()  # a NaN, a +inf and an exact tie for the minimum inside the first group; a -inf in the second
    c[0] = np.nan
    if G >= 4:
        c[1] = np.inf
        c[G // 2] = c[G - 1] = -100.0
    else:
        c[1] = np.inf
    if B > G:
        c[G + (1 if G > 1 else 2)] = -np.inf
    plantings.append(c)
    c = base.copy()  # the last group: no finite cost at all
    c[B - G:] = np.resize([np.nan, np.inf, -np.inf], G)
    plantings.append(c)
    src_d = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for i, c in enumerate(plantings):
        H.set_trajectory(cost=c)
        want = np_best(c, G)
        if i == 0 and G >= 4:
            assert want[0] == G // 2  # the tie went to the lower index, past the NaN and the inf
        if i == 1:
            assert np.array_equal(want[B - G:], np.arange(B - G, B))
        got = H.select_best(G)
        H.select_best(G, ptr=src_d.data_ptr())
        H.synchronize()
        assert got.dtype == np.int32 and np.array_equal(got, want), (G, i)
        assert np.array_equal(src_d.cpu().numpy(), want), (G, i)
        assert np.array_equal(H.cost(), c, equal_nan=True)  # reads the costs only
    assert np.array_equal(H.clone_flags(), np.zeros(B, dtype=np.int32))  # selecting clones nobody
    del src_d


# ---- 5. clone_best == select_best + clone_trajectories -----------------------------------------------------------------------------------
@pytest.mark.parametrize("route,G", [("acrobot_hex", 4), ("acrobot_hex", 5), ("acrobot_hex", 8), ("acrobot_hex", 20), ("acrobot_hex", 40),
                                     ("lq_f32", 5), ("chain", 20)])
def test_clone_best_is_select_then_clone(route, G, chain_lib):
    """every map, du and flag lives in a torch tensor: no host array in the calls"""
    import torch
    f32 = ROUTES[route][1].get("dtype") == "f32"
    A, _, nu = solved(route, chain_lib)
    C2, _, _ = solved(route, chain_lib)
    before = snapshot(A)
    assert_rows(snapshot(C2), before, np.arange(B), np.arange(B), (route, "two handles, one state"))
    du_d = 0.05 * torch.randn((B, T, nu), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    map_d = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    flags_d = torch.full((2, B), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    A.clone_best(G, du_ptr=du_d.data_ptr())
    A.copy_clone_flags_to_device(flags_d[0].data_ptr())
    C2.select_best(G, ptr=map_d.data_ptr())
    C2.clone_trajectories(src_ptr=map_d.data_ptr(), du_ptr=du_d.data_ptr())
    C2.copy_clone_flags_to_device(flags_d[1].data_ptr())
    A.synchronize()
    C2.synchronize()
    a, c = snapshot(A), snapshot(C2)
    assert_rows(a, c, np.arange(B), np.arange(B), (route, G))
    src, flags, du = map_d.cpu().numpy(), flags_d.cpu().numpy(), du_d.cpu().numpy()
    want = np_best(before["cost"], G)
    assert np.array_equal(src, want), (route, G)
    assert np.array_equal(flags[0], flags[1]) and np.array_equal(flags[0], (want != np.arange(B)).astype(np.int32)), (route, G)
    # every group's rows are its winner's; the controls are the winner's plus the row's own du, the winner's own unperturbed
    assert_rows(a, before, np.arange(B), want, (route, G), keys=[k for k in KEYS if k != "us"])
    losers = want != np.arange(B)
    assert np.array_equal(a["us"][losers], storage(before["us"][want[losers]] + du[losers], f32)), (route, G)
    assert np.array_equal(a["us"][~losers], before["us"][~losers]), (route, G)
    A.close()
    C2.close()
    del du_d, map_d, flags_d


# ---- 6. the source rule -----------------------------------------------------------------------------------------------------------------------
def test_a_source_that_changes_itself_is_refused():
    import torch
    from ilqr_amd import capi
    H, _, _ = solved("acrobot_hex", None)
    before = snapshot(H)
    src = np.arange(B, dtype=np.int32)
    src[1], src[2], src[3], src[5], src[7] = 2, 3, 3, B, -1
    H.clone_trajectories(src=src)
    after = snapshot(H)
    want_rows = np.arange(B)
    want_rows[2] = 3  # 2 is cloned; 1 (its source 2 is a destination) and 5 (no such trajectory) are refused; 7 was not asked
    assert_rows(after, before, np.arange(B), want_rows, "source rule")
    want_flags = np.zeros(B, dtype=np.int32)
    want_flags[2], want_flags[1], want_flags[5] = capi.WAS_CLONED, capi.CLONE_REFUSED, capi.CLONE_REFUSED
    assert np.array_equal(effective(src)[1], want_flags)
    assert np.array_equal(H.clone_flags(), want_flags)
    flags_d = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    H.copy_clone_flags_to_device(flags_d.data_ptr())
    H.synchronize()
    assert np.array_equal(flags_d.cpu().numpy(), want_flags)
    H.close()
    del flags_d


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    import torch
    from ilqr_amd import capi
    ip = capi._ip
    kw, x0, nu = problem("acrobot")
    g = make(kw)
    src = explicit_map()
    sp = src.ctypes.data_as(ip)
    out = np.zeros(B, dtype=np.int32)
    op = out.ctypes.data_as(ip)
    src_d = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    zeros = np.zeros(B, dtype=np.int32)
    # before a trajectory exists
    assert g.lib.ilqr_select_best(g.h, 4, op, None) == ERR_STATE
    assert g.lib.ilqr_clone_trajectories(g.h, sp, None, None) == ERR_STATE
    assert g.lib.ilqr_clone_best(g.h, 4, None) == ERR_STATE
    assert np.array_equal(g.clone_flags(), zeros)
    g.init_traj(x0, 0.1 * np.random.default_rng(1).standard_normal((B, T, nu)))
    g.iterate(1)
    ref = snapshot(g)
    assert g.lib.ilqr_clone_trajectories(g.h, sp, src_d.data_ptr(), None) == ERR_INVALID  # both maps
    assert g.lib.ilqr_clone_trajectories(g.h, None, None, None) == ERR_INVALID            # neither
    assert g.lib.ilqr_select_best(g.h, 4, op, src_d.data_ptr()) == ERR_INVALID
    assert g.lib.ilqr_select_best(g.h, 4, None, None) == ERR_INVALID
    for group in (0, -4, 3):  # 40 % 3 != 0
        assert g.lib.ilqr_select_best(g.h, group, op, None) == ERR_INVALID, group
        assert g.lib.ilqr_clone_best(g.h, group, None) == ERR_INVALID, group
    assert_rows(snapshot(g), ref, np.arange(B), np.arange(B), "refused calls change nothing")
    assert np.array_equal(g.clone_flags(), zeros)
    assert np.array_equal(src_d.cpu().numpy(), src) and not out.any()
    g.iterate(1)  # ... and the handle goes on
    g.close()
    del src_d


# ---- 8. a host-evaluated model ----------------------------------------------------------------------------------------------------------------
def test_clone_on_a_host_evaluated_handle():
    from ilqr_amd import BatchILQR
    rng = np.random.default_rng(2)
    nx, nu = 5, 3
    hm = BatchILQR("host", B, T, DT, nx=nx, nu=nu, u_min=-1.0, u_max=1.0)
    state = dict(xs=rng.normal(size=(B, T + 1, nx)), us=rng.normal(size=(B, T, nu)), k=rng.normal(size=(B, T, nu)),
                 K=rng.normal(size=(B, T, nu, nx)), cost=rng.normal(size=B), lam=rng.uniform(1, 9, B), dlam=rng.uniform(1, 2, B))
    hm.set_trajectory(x0=state["xs"][:, 0], xs=state["xs"], us=state["us"], cost=state["cost"])
    hm.set_gains(k=state["k"], K=state["K"])
    hm.set_lambda(state["lam"], state["dlam"])
    before = snapshot(hm)
    for key, v in state.items():
        assert np.array_equal(before[key], v), key
    src = explicit_map()
    eff, flags = effective(src)
    hm.clone_trajectories(src=src)
    assert_rows(snapshot(hm), before, np.arange(B), eff, "host-evaluated")
    assert np.array_equal(hm.clone_flags(), flags)
    assert np.array_equal(hm.select_best(8), np_best(before["cost"][eff], 8))
    hm.close()
