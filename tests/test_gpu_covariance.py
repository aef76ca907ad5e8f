"""The closed-loop state covariance, control covariance and expected noise cost of the stored policy on the device (ilqr_get_covariance /
ilqr_copy_covariance_to_device; k_covariance_w on the generic layout, k_covariance_t on the tiled one): against a numpy restatement of
the header's definition, against the value kernel through the identity J = 1/2 <Vxx[0], Sigma0> + 1/2 sum_t <Vxx[t+1], W>, against the
device model itself through ilqr_evaluate_policy, windows, the device copy, and that asking for it changes nothing a later iteration
computes.

Yardstick: cov_reference(records, K, Sigma0, W), float64.  Between it and the device (two summation orders of one recursion) the bound is
the project's 1e-9 x max(1, max|.|); every input is first put through the same recursion in np.longdouble, which has to agree with
float64 within 1e-10 x the same scale -- a factor 10 of headroom -- before the bound is relied on (reference_with_headroom)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_gpu_value import GENERIC_SIZES, NAMES, host_handle, nx4_handle, random_policy
from tests.util import TOL

pytestmark = pytest.mark.gpu
DT = 0.02
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """The device-copy case uses torch tensors: torch's device is initialised before this module creates any handle (a torch initialised
    after the library had set up the device reports no GPU: tests/test_gpu_mpc.py)."""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


def cov_reference(d, K, Sigma0, W, dtype=np.float64):
    """The definition of include/ilqr_amd.h (ilqr_get_covariance).  d: the records as BatchILQR.derivatives() returns them (matrices
    [B][T+1][rows][cols]); K [B][T][m][n]; Sigma0, W [B][n][n] or None (zero).  Returns Sigma [B][T+1][n][n], Su [B][T][m][m], J [B]."""
    fx, fu, cx, cu, cxx, cxu, cuu = (np.asarray(d[name], dtype=dtype) for name in NAMES)
    K = np.asarray(K, dtype=dtype)
    B, T1, n = cx.shape
    T, m = T1 - 1, K.shape[2]
    tr = lambda M: np.swapaxes(M, -1, -2)
    sym = lambda M: (M + tr(M)) / 2
    dot = lambda X, Y: (X * Y).sum(axis=(-1, -2))
    Sigma, Su, J = np.zeros((B, T1, n, n), dtype=dtype), np.zeros((B, T, m, m), dtype=dtype), np.zeros(B, dtype=dtype)
    Wm = np.zeros((B, n, n), dtype=dtype) if W is None else np.asarray(W, dtype=dtype)
    if Sigma0 is not None:
        Sigma[:, 0] = np.asarray(Sigma0, dtype=dtype)
    for t in range(T):
        S, Kt = Sigma[:, t], K[:, t]
        A = fx[:, t] + fu[:, t] @ Kt
        Z = S @ tr(Kt)
        Su[:, t] = sym(Kt @ Z)
        J += (dot(cxx[:, t], S) + dot(cuu[:, t], Su[:, t]) + 2 * dot(cxu[:, t], Z)) / 2
        Sigma[:, t + 1] = sym(A @ S @ tr(A) + Wm)
    J += dot(cxx[:, T], Sigma[:, T]) / 2
    return Sigma, Su, J


def noise_inputs(n, B=5, seed=0):
    """Sigma0 = L L' with L ~ N(0, 1/n); W = L L' with L ~ 0.1 N(0, 1/n): [B][n][n] each."""
    rng = np.random.default_rng(7000 + 10 * n + seed)
    L0 = rng.normal(size=(B, n, n)) / np.sqrt(n)
    Lw = 0.1 * rng.normal(size=(B, n, n)) / np.sqrt(n)
    return L0 @ np.swapaxes(L0, -1, -2), Lw @ np.swapaxes(Lw, -1, -2)


def scale_of(a):
    return max(1.0, float(np.abs(a).max()))


def reference_with_headroom(d, K, Sigma0, W):
    """cov_reference in float64, after the float64 and np.longdouble recursions have agreed within 1e-10 x max(1, max|.|)."""
    ref = cov_reference(d, K, Sigma0, W)
    lng = cov_reference(d, K, Sigma0, W, dtype=np.longdouble)
    for a, b, what in zip(ref, lng, ("Sigma", "Su", "J")):
        gap = float(np.abs(a - b).max())
        print("  float64 vs longdouble %s: %.3g (scale %.3g)" % (what, gap, scale_of(a)))
        assert gap <= 1e-10 * scale_of(a), (what, gap, scale_of(a))
    return ref


def against_reference(got, ref, bound=1e-9):
    """got, ref: (Sigma, Su, J), any member of got may be None; windows are the caller's business."""
    for a, b, what in zip(got, ref, ("Sigma", "Su", "J")):
        if a is None:
            continue
        assert a.shape == b.shape, (what, a.shape, b.shape)
        err = float(np.abs(a - b).max())
        print("  device vs reference %s: %.3g (scale %.3g)" % (what, err, scale_of(b)))
        assert err <= bound * scale_of(b), (what, err, scale_of(b))


@functools.lru_cache(maxsize=None)
def generic_case(n, m, seed=0):
    """(d, k, K, Sigma0, W, reference): computed once per size, shared, never written to."""
    d, k, K = random_policy(n, m, seed=seed)
    S0, W = noise_inputs(n, seed=seed)
    return d, k, K, S0, W, reference_with_headroom(d, K, S0, W)


def everything(g, S0, W):
    """(Sigma of every knot 0..T, Su of every knot 0..T-1, J): two calls, since a window with Su ends before knot T."""
    Sg = g.covariance(S0, W)
    Sg_T, Su, J = g.covariance(S0, W, Su=True, expected_cost=True)
    assert Sg.shape[1] == g.T + 1 and Sg_T.shape[1] == g.T and np.array_equal(Sg_T, Sg[:, :-1])
    return Sg, Su, J


# ---- 1. generic layout -------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", GENERIC_SIZES)
def test_generic_layout(n, m):
    """One and two state tiles, one and two control tiles, ragged edges, the one- and two-control sizes."""
    d, k, K, S0, W, ref = generic_case(n, m)
    g = host_handle(n, m, d, k, K)
    Sg, Su, J = everything(g, S0, W)
    assert Sg.shape == (5, 13, n, n) and Su.shape == (5, 12, m, m) and J.shape == (5,)
    against_reference((Sg, Su, J), ref)
    assert np.array_equal(Sg[:, 0], S0)  # as given, to the bit
    assert np.array_equal(Sg[:, 1:], np.swapaxes(Sg[:, 1:], -1, -2)) and np.array_equal(Su, np.swapaxes(Su, -1, -2))  # symmetric to the bit
    g.close()


def test_sigma0_is_taken_as_given():
    """Sigma[0] is not symmetrised, and the first step multiplies by it, not by its transpose."""
    n, m = 20, 5
    d, k, K, S0, W, _ = generic_case(n, m)
    S0 = S0 + 0.2 * np.random.default_rng(9).normal(size=S0.shape) / np.sqrt(n)
    g = host_handle(n, m, d, k, K)
    got = everything(g, S0, W)
    assert np.array_equal(got[0][:, 0], S0)
    against_reference(got, reference_with_headroom(d, K, S0, W))
    g.close()


# ---- 2. windows and NULLs ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def generic_handle():
    d, k, K, S0, W, _ = generic_case(20, 5, seed=1)
    g = host_handle(20, 5, d, k, K)
    yield g, S0, W
    g.close()


@pytest.fixture(scope="module")
def tiled_handle():
    g, x0, u0, _ = nx4_handle("double_integrator", "f64")
    g.init_traj(x0, u0)
    g.compute_derivatives()
    g.backward_pass()
    yield (g,) + noise_inputs(4, B=g.B)
    g.close()


@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_windows_and_nulls(generic_handle, tiled_handle, which):
    g, S0, W = generic_handle if which == "generic" else tiled_handle
    T, n, m, B = g.T, g.nx, g.nu, g.B
    Sg, Su, J = everything(g, S0, W)
    assert np.abs(Su).max() > 0 and np.abs(J).max() > 0
    for t0, nk in ((3, 4), (0, 1), (T, 1), (T - 1, 1)):
        assert np.array_equal(g.covariance(S0, W, t0, nk), Sg[:, t0:t0 + nk]), (t0, nk)
    w_s, w_u = g.covariance(S0, W, 3, 4, Su=True)
    assert np.array_equal(w_s, Sg[:, 3:7]) and np.array_equal(w_u, Su[:, 3:7])
    # one output at a time (raw calls: the numpy method always asks for Sigma)
    s0c, wc = g._cov_input(S0), g._cov_input(W)
    p = lambda a: a.ctypes.data_as(dp)
    only_j, only_u = np.zeros(B), np.zeros((B, 4, m, m))
    assert g.lib.ilqr_get_covariance(g.h, 0, 1, p(s0c), p(wc), None, None, p(only_j)) == 0 and np.array_equal(only_j, J)
    assert g.lib.ilqr_get_covariance(g.h, 3, 4, p(s0c), p(wc), None, p(only_u), None) == 0
    assert np.array_equal(np.swapaxes(only_u, -1, -2), Su[:, 3:7])
    # NULL inputs
    z = g.covariance(None, W)
    assert np.array_equal(z[:, 0], np.zeros((B, n, n))) and np.abs(z[:, 1]).max() > 0
    for a, b in zip(g.covariance(S0, None, Su=True, expected_cost=True), g.covariance(S0, np.zeros((n, n)), Su=True, expected_cost=True)):
        assert np.array_equal(a, b)
    # refusals
    buf_s, buf_u = np.zeros((B, T + 1, n * n)), np.zeros((B, T + 1, m * m))
    for t0, nk in ((-1, 1), (0, 0), (T + 1, 1), (3, T), (0, T + 2), (T, 2), (2, -1)):
        assert g.lib.ilqr_get_covariance(g.h, t0, nk, None, None, p(buf_s), None, p(only_j)) == -1, (t0, nk)
        assert g.lib.ilqr_copy_covariance_to_device(g.h, t0, nk, None, None, buf_s.ctypes.data, None, None) == -1, (t0, nk)
    for t0, nk in ((0, T + 1), (T, 1), (T - 2, 3)):  # Su with knot T in the window
        assert g.lib.ilqr_get_covariance(g.h, t0, nk, None, None, p(buf_s), p(buf_u), None) == -1, (t0, nk)
        assert b"knot T" in g.lib.ilqr_last_error()
        assert g.lib.ilqr_copy_covariance_to_device(g.h, t0, nk, None, None, None, buf_u.ctypes.data, None) == -1, (t0, nk)
    assert g.lib.ilqr_get_covariance(g.h, 0, 1, p(s0c), p(wc), None, None, None) == -1 and b"all null" in g.lib.ilqr_last_error()
    assert g.lib.ilqr_copy_covariance_to_device(g.h, 0, 1, None, None, None, None, None) == -1


def test_fresh_handle_is_a_state_error():
    from ilqr_amd import BatchILQR
    for g in (BatchILQR("acrobot", 4, 10, DT), BatchILQR("host", 4, 10, DT, nx=6, nu=2, u_min=-1.0, u_max=1.0)):
        s = np.zeros((4, 1, g.nx * g.nx))
        assert g.lib.ilqr_get_covariance(g.h, 0, 1, None, None, s.ctypes.data_as(dp), None, None) == -4
        assert g.lib.ilqr_copy_covariance_to_device(g.h, 0, 1, None, None, s.ctypes.data, None, None) == -4
        g.close()


# ---- 3. against the existing value kernel ------------------------------------------------------
@pytest.mark.parametrize("n,m", [(20, 5), (32, 32)])
def test_expected_cost_against_the_value_kernel(n, m):
    """J = 1/2 <Vxx[0], Sigma0> + 1/2 sum_t <Vxx[t+1], W> with Vxx from ilqr_get_value on the same handle: two independent kernels."""
    d, k, K, S0, W, _ = generic_case(n, m)
    g = host_handle(n, m, d, k, K)
    _, _, J = g.covariance(S0, W, Su=True, expected_cost=True)
    _, Vxx = g.value()
    dot = lambda X, Y: (X * Y).sum(axis=(-1, -2))
    want = 0.5 * dot(Vxx[:, 0], S0) + 0.5 * sum(dot(Vxx[:, t + 1], W) for t in range(g.T))
    err = float(np.abs(J - want).max())
    print("  covariance kernel vs value kernel J: %.3g (scale %.3g)" % (err, scale_of(want)))
    assert err <= 1e-9 * scale_of(want), (err, scale_of(want))
    g.close()


# ---- 4. nx = 4 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model", ["acrobot", "double_integrator"])
def test_nx4(model, dtype):
    """B = 20 is no multiple of the 16-trajectory tile; the recursion is double in both dtypes, so one bound."""
    g, x0, u0, _ = nx4_handle(model, dtype, B=20, T=30)
    g.init_traj(x0, u0)
    g.iterate(3)
    g.compute_derivatives()
    S0, W = noise_inputs(4, B=20)
    got = everything(g, S0, W)
    against_reference(got, reference_with_headroom(g.derivatives(), g.gains()[1], S0, W))
    assert np.array_equal(got[0][:, 1:], np.swapaxes(got[0][:, 1:], -1, -2))
    g.close()


# ---- 5. against the device model itself --------------------------------------------------------
def test_against_the_device_model():
    """An LQ model is linear and nothing clamps, so the closed loop maps x0 + e_i to x_end + Phi e_i exactly: Phi, column by column, from
    ilqr_evaluate_policy on n + 1 samples; with W = 0, Sigma[T] = Phi Sigma0 Phi'."""
    from ilqr_amd import BatchILQR, capi
    n, m, B, T = 6, 2, 5, 12
    rng = np.random.default_rng(11)
    A = -np.eye(n) + 0.1 * rng.normal(size=(n, n)) / np.sqrt(n)
    Bm = rng.normal(size=(n, m)) / np.sqrt(n)
    g = BatchILQR("lq", B, T, DT, lq=(A, Bm, np.eye(n), 0.1 * np.eye(m), np.eye(n)), u_min=-1e3, u_max=1e3, flags=capi.FLAG_ANALYTIC_DERIVATIVES)
    x0, u0 = rng.uniform(-1, 1, (B, n)), rng.normal(size=(B, T, m)) * 0.3
    g.init_traj(x0, u0)
    g.iterate(2)
    assert np.abs(g.trajectory()[1]).max() < 1e2 and np.abs(g.gains()[1]).max() > 0  # nothing near the limits; a feedback exists
    samples = x0[:, None, :] + np.concatenate([np.zeros((1, n)), np.eye(n)])[None]
    x_end = g.evaluate_policy(samples, 0, T)["x_end"]
    Phi = np.swapaxes(x_end[:, 1:] - x_end[:, :1], -1, -2)  # column i: the image of e_i
    S0, _ = noise_inputs(n, B=B)
    Sg = g.covariance(S0, None, T, 1)[:, 0]
    want = Phi @ S0 @ np.swapaxes(Phi, -1, -2)
    err = float(np.abs(Sg - want).max())
    print("  Sigma[T] vs Phi Sigma0 Phi': %.3g (scale %.3g)" % (err, scale_of(want)))
    assert err <= TOL * scale_of(want), (err, scale_of(want))
    g.close()


# ---- 6. fp32 generic ---------------------------------------------------------------------------
def test_fp32_generic():
    """Float records and gains are widened, the recursion is double: the definition on the handle's float-valued records and gains."""
    from ilqr_amd import BatchILQR
    from tests.test_gpu_lq_end_to_end import lq_mats
    n, m, B, T = 20, 5, 6, 12
    g = BatchILQR("lq", B, T, DT, lq=lq_mats(n, m), u_min=-0.5, u_max=0.5, dtype="f32")
    rng = np.random.default_rng(5)
    g.init_traj(rng.uniform(-1, 1, (B, n)), rng.normal(size=(B, T, m)) * 0.3)
    g.iterate(2)
    S0, W = noise_inputs(n, B=B)
    got = everything(g, S0, W)
    against_reference(got, reference_with_headroom(g.derivatives(), g.gains()[1], S0, W))
    g.close()


# ---- 7. device variant -------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_copy_to_device_equals_the_getter(generic_handle, tiled_handle, which):
    import torch
    g, S0, W = generic_handle if which == "generic" else tiled_handle
    t0, nk, B, n, m = 2, 5, g.B, g.nx, g.nu
    Sg, Su, J = g.covariance(S0, W, t0, nk, Su=True, expected_cost=True)
    d_s0, d_w = torch.from_numpy(g._cov_input(S0)).cuda(), torch.from_numpy(g._cov_input(W)).cuda()
    d_s = torch.full((B, nk, n * n), -7.0, dtype=torch.float64, device="cuda")
    d_u = torch.full((B, nk, m * m), -7.0, dtype=torch.float64, device="cuda")
    d_j = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # (the copies and fills ran on torch's stream, the call runs on the handle's)
    g.copy_covariance_to_device(t0, nk, d_s0.data_ptr(), d_w.data_ptr(), d_s.data_ptr(), d_u.data_ptr(), d_j.data_ptr())
    g.synchronize()
    assert np.array_equal(d_s.cpu().numpy().reshape(B, nk, n, n), np.swapaxes(Sg, -1, -2))
    assert np.array_equal(d_u.cpu().numpy().reshape(B, nk, m, m), np.swapaxes(Su, -1, -2))
    assert np.array_equal(d_j.cpu().numpy(), J)
    # one output only: the other buffers are not touched
    d_s.fill_(-7.0)
    d_u.fill_(-7.0)
    torch.cuda.synchronize()
    g.copy_covariance_to_device(t0, nk, d_s0.data_ptr(), d_w.data_ptr(), expected_cost_ptr=d_j.data_ptr())
    g.synchronize()
    assert float(d_s.min()) == -7.0 == float(d_s.max()) and float(d_u.min()) == -7.0 == float(d_u.max())
    assert np.array_equal(d_j.cpu().numpy(), J)


# ---- 8. read-only ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiled", "generic"])
def test_the_handle_is_left_alone(which):
    from ilqr_amd import BatchILQR, capi
    if which == "tiled":
        g, x0, u0, _ = nx4_handle("acrobot", "f64")
    else:
        from tests.test_gpu_lq_end_to_end import lq_mats
        n, m, B, T = 20, 5, 6, 12
        g = BatchILQR("lq", B, T, DT, lq=lq_mats(n, m), u_min=-0.5, u_max=0.5, flags=capi.FLAG_ANALYTIC_DERIVATIVES)
        rng = np.random.default_rng(7)
        x0, u0 = rng.uniform(-1, 1, (B, n)), rng.normal(size=(B, T, m)) * 0.3
    twin = g.clone()
    for h in (g, twin):
        h.init_traj(x0, u0)
        h.iterate(2)
    S0, W = noise_inputs(g.nx, B=g.B)
    got = everything(g, S0, W)
    against_reference(got, reference_with_headroom(g.derivatives(), g.gains()[1], S0, W))
    for h in (g, twin):
        h.iterate(3)
    for a, b in zip(g.trajectory() + g.gains() + (g.cost(),) + g.lambdas(), twin.trajectory() + twin.gains() + (twin.cost(),) + twin.lambdas()):
        assert np.array_equal(a, b)
    g.close()
    twin.close()


# ---- every request through the staging buffer ---------------------------------------------------
from tests import getter_vs_device as gd  # noqa: E402


@pytest.mark.parametrize("case", gd.CASES)
@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_getter_equals_the_device_form_request_by_request(which, case):
    """ilqr_get_covariance against ilqr_copy_covariance_to_device, bit for bit: every pointer; expected_cost alone with Sigma0 and W null;
    that, every pointer, that again on one handle."""

    def args(g):
        rng, n, m = np.random.default_rng(3), g.nx, g.nu
        return [gd.Arg("Sigma0", "in", gd.spd(rng, n)), gd.Arg("W", "in", gd.spd(rng, n, 0.01)), gd.Arg("Sigma", "out", (gd.B * gd.NK * n * n,)),
                gd.Arg("Su", "out", (gd.B * gd.NK * m * m,)), gd.Arg("expected_cost", "out", (gd.B,))]
    gd.check(lambda: gd.handle(which), case, "ilqr_get_covariance", "ilqr_copy_covariance_to_device", (gd.T0, gd.NK), args)
