"""The value model (Vx, Vxx) of the stored policy, per knot, on the device (ilqr_get_value / ilqr_copy_value_to_device; k_value_w on the
generic layout, k_value_t on the tiled one): against a numpy restatement of the header's definition, against the oracle's backward pass,
windows, the device copy, and that asking for it changes nothing a later iteration computes.

Yardstick: value_reference(records, k, K), float64.  Between it and the device (two summation orders of one recursion) the bound is the
project's 1e-9 x max(1, max|.|) (test_default_kernel_against_the_literal_order_kernel); every input is first put through the same
recursion in np.longdouble, which has to agree with float64 within 1e-10 x the same scale -- a factor 10 of headroom -- before the
bound is relied on (against_reference).  Against the oracle: the per-knot 1e-6 of tests/parity.py, on trajectories with diverge == 0."""
import ctypes as C

import numpy as np
import pytest

from tests.util import TOL, acrobot_x0, integrator_x0, mat

pytestmark = pytest.mark.gpu
DT = 0.02
NAMES = ("fx", "fu", "cx", "cu", "cxx", "cxu", "cuu")
GENERIC_SIZES = [(32, 16), (20, 5), (8, 3), (17, 17), (24, 20), (32, 32), (6, 1), (6, 2)]


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """The device-copy case writes into torch tensors: torch's device is initialised before this module creates any handle (a torch
    initialised after the library had set up the device reports no GPU: tests/test_gpu_mpc.py)."""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


def value_reference(d, k, K, dtype=np.float64):
    """The definition of include/ilqr_amd.h (ilqr_get_value).  d: the records as BatchILQR.derivatives() returns them (matrices
    [B][T+1][rows][cols]); k [B][T][m], K [B][T][m][n].  Returns Vx [B][T+1][n], Vxx [B][T+1][n][n]."""
    fx, fu, cx, cu, cxx, cxu, cuu = (np.asarray(d[name], dtype=dtype) for name in NAMES)
    k, K = np.asarray(k, dtype=dtype), np.asarray(K, dtype=dtype)
    B, T1, n = cx.shape
    T = T1 - 1
    tr = lambda M: np.swapaxes(M, -1, -2)
    Vx, Vxx = np.zeros((B, T1, n), dtype=dtype), np.zeros((B, T1, n, n), dtype=dtype)
    Vx[:, T], Vxx[:, T] = cx[:, T], cxx[:, T]
    for t in range(T - 1, -1, -1):
        A, Bm, v, V = fx[:, t], fu[:, t], Vx[:, t + 1][..., None], Vxx[:, t + 1]
        Qx = cx[:, t][..., None] + tr(A) @ v
        Qu = cu[:, t][..., None] + tr(Bm) @ v
        Qxx = cxx[:, t] + tr(A) @ V @ A
        Qux = tr(cxu[:, t]) + tr(Bm) @ V @ A
        Quu = cuu[:, t] + tr(Bm) @ V @ Bm
        Kt, kt = K[:, t], k[:, t][..., None]
        Vx[:, t] = (Qx + tr(Kt) @ Quu @ kt + tr(Kt) @ Qu + tr(Qux) @ kt)[..., 0]
        Vn = Qxx + tr(Kt) @ Quu @ Kt + tr(Kt) @ Qux + tr(Qux) @ Kt
        Vxx[:, t] = 0.5 * (Vn + tr(Vn))
    return Vx, Vxx


def reference_with_headroom(d, k, K):
    """value_reference in float64, after the float64 and np.longdouble recursions have agreed within 1e-10 x max(1, max|.|)."""
    Vx, Vxx = value_reference(d, k, K)
    Lx, Lxx = value_reference(d, k, K, dtype=np.longdouble)
    for a, b, what in ((Vx, Lx, "Vx"), (Vxx, Lxx, "Vxx")):
        scale = max(1.0, float(np.abs(a).max()))
        gap = float(np.abs(a - b).max())
        print("  float64 vs longdouble %s: %.3g (scale %.3g)" % (what, gap, scale))
        assert gap <= 1e-10 * scale, (what, gap, scale)
    return Vx, Vxx


def against_reference(got, d, k, K, t0=0):
    Vx, Vxx = reference_with_headroom(d, k, K)
    for a, b, what in ((got[0], Vx, "Vx"), (got[1], Vxx, "Vxx")):
        b = b[:, t0:t0 + a.shape[1]]
        scale = max(1.0, float(np.abs(b).max()))
        err = float(np.abs(a - b).max())
        print("  device vs reference %s: %.3g (scale %.3g)" % (what, err, scale))
        assert err <= 1e-9 * scale, (what, err, scale)
    return Vx, Vxx


def random_policy(n, m, B=5, T=12, seed=0):
    """Random records (cxx, cuu symmetric), random k, random K with some rows zeroed as clamped controls leave them; sized so that the
    recursion neither grows nor decays over the horizon (fx near the identity, feedback of the order of 1 / sqrt(n))."""
    rng = np.random.default_rng(1000 * n + m + seed)
    sym = lambda M: 0.5 * (M + np.swapaxes(M, -1, -2))
    d = dict(fx=np.eye(n) + 0.1 * rng.normal(size=(B, T + 1, n, n)) / np.sqrt(n), fu=rng.normal(size=(B, T + 1, n, m)) / np.sqrt(n),
             cx=rng.normal(size=(B, T + 1, n)), cu=rng.normal(size=(B, T + 1, m)),
             cxx=sym(rng.normal(size=(B, T + 1, n, n))) / np.sqrt(n) + np.eye(n), cxu=0.3 * rng.normal(size=(B, T + 1, n, m)) / np.sqrt(n),
             cuu=sym(rng.normal(size=(B, T + 1, m, m))) / np.sqrt(m) + np.eye(m))
    k = 0.5 * rng.normal(size=(B, T, m))
    K = 0.5 * rng.normal(size=(B, T, m, n)) / np.sqrt(n)
    K[rng.uniform(size=(B, T, m)) < 0.3] = 0.0
    return d, k, K


def host_handle(n, m, d, k, K, lim=1.0):
    from ilqr_amd import BatchILQR
    B, T = k.shape[0], k.shape[1]
    g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=-lim, u_max=lim)
    g.set_trajectory(x0=np.zeros((B, n)), xs=np.zeros((B, T + 1, n)), us=np.zeros((B, T, m)), cost=np.zeros(B))
    g.set_derivatives(**d)
    g.set_gains(k=k, K=K)
    return g


# ---- 1. generic layout, arbitrary policy ------------------------------------------------------
@pytest.mark.parametrize("n,m", GENERIC_SIZES)
def test_generic_layout_arbitrary_policy(n, m):
    """One and two state tiles, one and two control tiles, ragged edges, the one- and two-control sizes: value() against the definition."""
    d, k, K = random_policy(n, m)
    g = host_handle(n, m, d, k, K)
    got = g.value()
    assert got[0].shape == (5, 13, n) and got[1].shape == (5, 13, n, n)
    against_reference(got, d, k, K)
    assert np.array_equal(got[1][:, :-1], np.swapaxes(got[1][:, :-1], -1, -2))  # every knot t < T is symmetrised, to the bit
    g.close()


def test_knot_T_is_not_symmetrised():
    """Vxx[T] = cxx[T] as stored, and the first step multiplies by it, not by its transpose."""
    n, m = 20, 5
    d, k, K = random_policy(n, m, seed=3)
    d["cxx"][:, -1] += 0.2 * np.random.default_rng(9).normal(size=(5, n, n)) / np.sqrt(n)
    g = host_handle(n, m, d, k, K)
    got = g.value()
    assert np.array_equal(got[1][:, -1], d["cxx"][:, -1]) and np.array_equal(got[0][:, -1], d["cx"][:, -1])
    against_reference(got, d, k, K)
    g.close()


# ---- 2. against the oracle's backward pass ----------------------------------------------------
@pytest.mark.parametrize("n,m", [(32, 16), (24, 20)])
def test_against_the_oracles_backward_pass(oracle, n, m):
    from ilqr_amd import BatchILQR
    from tests.test_gpu_generic_backward import lq_model
    om = lq_model(oracle, n, m, lim=0.5)
    B, T = 8, 12
    rng = np.random.default_rng(3)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.3
    xs, us, cost = oracle.batch_rollout(om, x0, u0, DT)
    dv = oracle.batch_derivatives(om, xs, us, DT)
    k_prev = np.zeros((B, T, m))
    ro = oracle.batch_backward(om, us, dv, k_prev=k_prev, lam=1.0)
    assert (ro["diverge"] != 0).sum() <= B // 8  # (the oracle alone: checkable without a GPU)
    g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=om.u_min, u_max=om.u_max)
    g.set_trajectory(x0=x0, xs=xs, us=us, cost=cost)
    g.set_derivatives(**{kk: (dv[kk] if kk in ("cx", "cu") else mat(dv[kk])) for kk in dv})
    g.set_gains(k=k_prev, K=np.zeros((B, T, m, n)))
    g.set_lambda(1.0, 1.0)
    div = g.backward_pass()
    ok = (div == 0) & (ro["diverge"] == 0)
    assert (~ok).sum() <= B // 8
    Vx, Vxx = g.value(0, 1)
    for b in np.flatnonzero(ok):
        for a, r, what in ((Vx[b, 0], ro["Vx0"][b], "Vx"), (Vxx[b, 0], mat(ro["Vxx0"][b]), "Vxx")):
            err, scale = np.abs(a - r).max(), max(1.0, np.abs(r).max())
            assert err <= TOL * scale, (what, b, err, scale)
    g.close()


# ---- 3. nx = 4, every knot --------------------------------------------------------------------
def nx4_handle(model, dtype, B=20, T=30, **kw):
    from ilqr_amd import BatchILQR
    lim = 1.5 if model == "acrobot" else 0.5
    g = BatchILQR(model, B, T, DT, u_min=-lim, u_max=lim, dtype=dtype, **kw)
    x0 = acrobot_x0(B, scale=0.3, seed=5) if model == "acrobot" else integrator_x0(B, seed=5)
    u0 = np.random.default_rng(2).normal(size=(B, T, g.nu)) * 0.2
    return g, x0, u0, lim


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model", ["acrobot", "double_integrator"])
def test_nx4_every_knot(oracle, model, dtype):
    """B = 20 is no multiple of the 16-trajectory tile.  fp64: every knot against the oracle's members; fp32: against the definition on
    the handle's own (float-valued) records and gains."""
    B, T = 20, 30
    g, x0, u0, lim = nx4_handle(model, dtype, B, T)
    g.init_traj(x0, u0)
    g.compute_derivatives()
    div = g.backward_pass()
    Vx, Vxx = g.value()
    if dtype == "f32":
        against_reference((Vx, Vxx), g.derivatives(), *g.gains())
    else:
        om = oracle.Model(model, u_lim=lim)
        left_out = 0
        for b in range(B):
            s = oracle.Solver(om, T, DT)
            s.init_traj(x0[b], u0[b])
            s.compute_derivatives()
            if s.backward_pass() != 0 or div[b] != 0:
                left_out += 1
                continue
            for a, r, what in ((Vx[b], s.vecs("Vx"), "Vx"), (Vxx[b], s.mat("Vxx"), "Vxx")):
                for t in range(T + 1):  # per knot
                    err, scale = np.abs(a[t] - r[t]).max(), max(1.0, np.abs(r[t]).max())
                    assert err <= TOL * scale, (what, b, t, err, scale)
        assert left_out <= B // 8, left_out
    g.close()


# ---- 4. persistent routes ---------------------------------------------------------------------
def test_persistent_route_and_the_handle_is_left_alone():
    g, x0, u0, _ = nx4_handle("acrobot", "f64")
    twin = g.clone()
    for h in (g, twin):
        h.init_traj(x0, u0)
        h.iterate(3)
    got = g.value()
    against_reference(got, g.derivatives(), *g.gains())
    for h in (g, twin):
        h.iterate(2)
    assert np.array_equal(g.trajectory()[0], twin.trajectory()[0]) and np.array_equal(g.trajectory()[1], twin.trajectory()[1])
    assert np.array_equal(g.gains()[0], twin.gains()[0]) and np.array_equal(g.gains()[1], twin.gains()[1])
    assert np.array_equal(g.cost(), twin.cost())
    g.close()
    twin.close()


# ---- 5. windows -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generic_handle():
    d, k, K = random_policy(20, 5, seed=1)
    g = host_handle(20, 5, d, k, K)
    yield g
    g.close()


@pytest.fixture(scope="module")
def tiled_handle():
    g, x0, u0, _ = nx4_handle("double_integrator", "f64")
    g.init_traj(x0, u0)
    g.compute_derivatives()
    g.backward_pass()
    yield g
    g.close()


@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_windows_are_slices_of_the_full_result(generic_handle, tiled_handle, which):
    g = generic_handle if which == "generic" else tiled_handle
    T = g.T
    Vx, Vxx = g.value()
    assert np.abs(Vxx).max() > 0
    for t0, n in ((0, 1), (T, 1), (3, 4), (0, T + 1)):
        wx, wxx = g.value(t0, n)
        assert np.array_equal(wx, Vx[:, t0:t0 + n]) and np.array_equal(wxx, Vxx[:, t0:t0 + n]), (t0, n)
    # one output at a time
    dp = C.POINTER(C.c_double)
    only_x, only_xx = np.zeros((g.B, 4, g.nx)), np.zeros((g.B, 4, g.nx * g.nx))
    assert g.lib.ilqr_get_value(g.h, 3, 4, only_x.ctypes.data_as(dp), None) == 0 and np.array_equal(only_x, Vx[:, 3:7])
    assert g.lib.ilqr_get_value(g.h, 3, 4, None, only_xx.ctypes.data_as(dp)) == 0
    assert np.array_equal(only_xx.reshape(g.B, 4, g.nx, g.nx), np.swapaxes(Vxx[:, 3:7], -1, -2))
    # refusals
    for t0, n in ((-1, 1), (0, 0), (T + 1, 1), (3, T), (0, T + 2), (T, 2), (2, -1)):
        assert g.lib.ilqr_get_value(g.h, t0, n, only_x.ctypes.data_as(dp), only_xx.ctypes.data_as(dp)) == -1, (t0, n)
        assert g.lib.ilqr_copy_value_to_device(g.h, t0, n, only_x.ctypes.data, only_xx.ctypes.data) == -1, (t0, n)
    assert g.lib.ilqr_get_value(g.h, 0, 1, None, None) == -1 and b"both null" in g.lib.ilqr_last_error()
    assert g.lib.ilqr_copy_value_to_device(g.h, 0, 1, None, None) == -1


def test_fresh_handle_is_a_state_error():
    from ilqr_amd import BatchILQR
    dp = C.POINTER(C.c_double)
    for g in (BatchILQR("acrobot", 4, 10, DT), BatchILQR("host", 4, 10, DT, nx=6, nu=2, u_min=-1.0, u_max=1.0)):
        vx, vxx = np.zeros((4, 1, g.nx)), np.zeros((4, 1, g.nx * g.nx))
        assert g.lib.ilqr_get_value(g.h, 0, 1, vx.ctypes.data_as(dp), vxx.ctypes.data_as(dp)) == -4
        assert g.lib.ilqr_copy_value_to_device(g.h, 0, 1, vx.ctypes.data, vxx.ctypes.data) == -4
        g.close()


# ---- 6. device copy ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_copy_to_device_equals_the_getter(generic_handle, tiled_handle, which):
    import torch
    g = generic_handle if which == "generic" else tiled_handle
    t0, n = 2, 5
    Vx, Vxx = g.value(t0, n)
    dvx = torch.full((g.B, n, g.nx), -7.0, dtype=torch.float64, device="cuda")
    dvxx = torch.full((g.B, n, g.nx * g.nx), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # (the fills ran on torch's stream, the copy runs on the handle's)
    g.copy_value_to_device(t0, n, Vx_ptr=dvx.data_ptr(), Vxx_ptr=dvxx.data_ptr())
    g.synchronize()
    assert np.array_equal(dvx.cpu().numpy(), Vx)
    assert np.array_equal(dvxx.cpu().numpy().reshape(g.B, n, g.nx, g.nx), np.swapaxes(Vxx, -1, -2))
    # one output only: the other buffer is not touched
    dvx.fill_(-7.0)
    torch.cuda.synchronize()
    g.copy_value_to_device(t0, n, Vxx_ptr=dvxx.data_ptr())
    g.synchronize()
    assert float(dvx.min()) == -7.0 == float(dvx.max())


# ---- 7. the record-free LQ route and a user twin -----------------------------------------------
def test_record_free_lq_route(oracle):
    """LQ model with exact derivatives on the default route: no record array exists until somebody asks; the value model is that of the
    records the getter returns."""
    from ilqr_amd import BatchILQR, capi
    n, m, B, T = 20, 5, 6, 12
    rng = np.random.default_rng(7)
    A = -np.eye(n) + 0.1 * rng.normal(size=(n, n)) / np.sqrt(n)
    Bm = rng.normal(size=(n, m)) / np.sqrt(n)
    g = BatchILQR("lq", B, T, DT, lq=(A, Bm, np.eye(n), 0.1 * np.eye(m), np.eye(n)), u_min=-0.5, u_max=0.5, flags=capi.FLAG_ANALYTIC_DERIVATIVES)
    assert g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index("derivatives")) == b""  # (the fused route: no sweep kernel)
    twin = g.clone()
    x0, u0 = rng.uniform(-1, 1, (B, n)), rng.normal(size=(B, T, m)) * 0.3
    for h in (g, twin):
        h.init_traj(x0, u0)
        h.iterate(2)
    got = g.value()
    against_reference(got, g.derivatives(), *g.gains())
    for h in (g, twin):
        h.iterate(2)
    assert np.array_equal(g.trajectory()[1], twin.trajectory()[1]) and np.array_equal(g.gains()[1], twin.gains()[1]) and np.array_equal(g.cost(), twin.cost())
    g.close()
    twin.close()


@pytest.fixture(scope="module")
def chain_lib():
    import os
    from ilqr_amd import _build
    if not os.path.exists(_build.USER_CHAIN_LIB) and not os.path.exists(_build.HIPCC):
        pytest.skip("the pendulum-chain build is missing and there is no hipcc to make it")
    return _build.build_user(_build.USER_CHAIN_HEADER, _build.USER_CHAIN_LIB)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_user_twin(chain_lib, dtype):
    from ilqr_amd import BatchILQR
    from tests.test_gpu_user_chain import NL, PARAMS, chain_x0
    B, T = 6, 10
    g = BatchILQR("user", B, T, DT, u_min=-2.0, u_max=2.0, lib=chain_lib, nx=2 * NL, nu=NL // 2, user_params=PARAMS, dtype=dtype)
    g.init_traj(chain_x0(B, seed=4), np.zeros((B, T, NL // 2)))
    g.iterate(2)
    got = g.value()
    against_reference(got, g.derivatives(), *g.gains())
    g.close()


# ---- 8. every request through the staging buffer -----------------------------------------------
from tests import getter_vs_device as gd  # noqa: E402


@pytest.mark.parametrize("case", gd.CASES)
@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_getter_equals_the_device_form_request_by_request(which, case):
    """ilqr_get_value against ilqr_copy_value_to_device, bit for bit: both outputs; Vxx alone; Vxx alone, both, Vxx alone on one handle."""
    args = lambda g: [gd.Arg("Vx", "out", (gd.B * gd.NK * g.nx,)), gd.Arg("Vxx", "out", (gd.B * gd.NK * g.nx * g.nx,))]
    gd.check(lambda: gd.handle(which), case, "ilqr_get_value", "ilqr_copy_value_to_device", (gd.T0, gd.NK), args)
