"""The tangent and the adjoint of the stored closed loop on the device (ilqr_get_tangent / ilqr_get_adjoint and their device forms;
k_tangent_w / k_adjoint_w on the generic layout, k_tangent_t / k_adjoint_t on the tiled one): against a numpy restatement of the header's
definition, column independence to the bit, the transpose identity between the two kernels, against the value and covariance kernels,
against the device model itself through ilqr_evaluate_policy, windows, NULLs and refusals, the device copies, that asking changes nothing
a later iteration computes, and C++ callers of the facade.

Yardstick: tangent_reference / adjoint_reference(records, K, the caller's vectors), float64.  Between it and the device (two summation
orders of one recursion) the bound is the project's 1e-9 x max(1, max|.|); every input is first put through the same recursion in
np.longdouble, which has to agree with float64 within 1e-10 x the same scale -- a factor 10 of headroom -- before the bound is relied on
(with_headroom)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_value import GENERIC_SIZES, host_handle, nx4_handle, random_policy
from tests.util import TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.02
dp = C.POINTER(C.c_double)
DIRECTION_COUNTS = (1, 16, 17, 33)


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """The device-copy case uses torch tensors: torch's device is initialised before this module creates any handle (a torch initialised
    after the library had set up the device reports no GPU: tests/test_gpu_mpc.py)."""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


# ---- the yardstick -----------------------------------------------------------------------------
def tangent_reference(d, K, dx0=None, dv=None, dtype=np.float64):
    """The definition of include/ilqr_amd.h (ilqr_get_tangent).  d: the records as BatchILQR.derivatives() returns them (matrices
    [B][T+1][rows][cols]); K [B][T][m][n]; dx0 [B][S][n], dv [B][T][S][m] or None (zero).  Returns dxs [B][T+1][S][n], dus [B][T][S][m]."""
    fx, fu, K = np.asarray(d["fx"], dtype=dtype), np.asarray(d["fu"], dtype=dtype), np.asarray(K, dtype=dtype)
    B, T, m, n = K.shape
    S = (dx0 if dx0 is not None else dv).shape[-2]
    tr = lambda M: np.swapaxes(M, -1, -2)
    dxs, dus = np.zeros((B, T + 1, S, n), dtype=dtype), np.zeros((B, T, S, m), dtype=dtype)
    if dx0 is not None:
        dxs[:, 0] = np.asarray(dx0, dtype=dtype)
    for t in range(T):
        dus[:, t] = dxs[:, t] @ tr(K[:, t])  # rows are directions: (K dx)' = dx' K'
        if dv is not None:
            dus[:, t] += np.asarray(dv[:, t], dtype=dtype)
        dxs[:, t + 1] = dxs[:, t] @ tr(fx[:, t]) + dus[:, t] @ tr(fu[:, t])
    return dxs, dus


def adjoint_reference(d, K, gx=None, gu=None, dtype=np.float64):
    """The definition of include/ilqr_amd.h (ilqr_get_adjoint) for cotangents over the whole horizon (a window: zeros outside it).
    gx [B][T+1][S][n], gu [B][T][S][m] or None (zero).  Returns a [B][T+1][S][n] (g_x0 = a[:, 0]) and g_v = w [B][T][S][m]."""
    fx, fu, K = np.asarray(d["fx"], dtype=dtype), np.asarray(d["fu"], dtype=dtype), np.asarray(K, dtype=dtype)
    B, T, m, n = K.shape
    S = (gx if gx is not None else gu).shape[-2]
    a, w = np.zeros((B, T + 1, S, n), dtype=dtype), np.zeros((B, T, S, m), dtype=dtype)
    if gx is not None:
        a[:, T] = np.asarray(gx[:, T], dtype=dtype)
    for t in range(T - 1, -1, -1):
        w[:, t] = a[:, t + 1] @ fu[:, t]  # (fu'a)' = a' fu
        if gu is not None:
            w[:, t] += np.asarray(gu[:, t], dtype=dtype)
        a[:, t] = a[:, t + 1] @ fx[:, t] + w[:, t] @ K[:, t]
        if gx is not None:
            a[:, t] += np.asarray(gx[:, t], dtype=dtype)
    return a, w


def scale_of(a):
    return max(1.0, float(np.abs(a).max()))


def with_headroom(reference, d, K, first, second):
    """reference(...) in float64, after the float64 and np.longdouble recursions have agreed within 1e-10 x max(1, max|.|)."""
    ref = reference(d, K, first, second)
    lng = reference(d, K, first, second, dtype=np.longdouble)
    for a, b in zip(ref, lng):
        gap = float(np.abs(a - b).max())
        print("  float64 vs longdouble %s: %.3g (scale %.3g)" % (reference.__name__, gap, scale_of(a)))
        assert gap <= 1e-10 * scale_of(a), (reference.__name__, gap, scale_of(a))
    return ref


def close(got, want, what, bound=1e-9):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max())
    print("  device vs reference %s: %.3g (scale %.3g)" % (what, err, scale_of(want)))
    assert err <= bound * scale_of(want), (what, err, scale_of(want))


def directions(n, m, S, B=5, T=12, seed=0):
    """(dx0 [B][S][n], dv [B][T][S][m], gx [B][T+1][S][n], gu [B][T][S][m]): standard normal, dv a tenth of that (a perturbation of the controls)."""
    rng = np.random.default_rng(9000 + 100 * n + m + 7 * S + seed)
    return rng.normal(size=(B, S, n)), 0.1 * rng.normal(size=(B, T, S, m)), rng.normal(size=(B, T + 1, S, n)), rng.normal(size=(B, T, S, m))


def identity_directions(n, B=5):
    return np.ascontiguousarray(np.broadcast_to(np.eye(n), (B, n, n)))


def check_both_calls(g, d, K, S, seed=0):
    """Tangent and adjoint of S random directions on the handle g against the yardstick on (d, K)."""
    B, T, n, m = g.B, g.T, g.nx, g.nu
    dx0, dv, gx, gu = directions(n, m, S, B, T, seed)
    dxs, dus = g.tangent(dx0, dv)
    assert dxs.shape == (B, T + 1, S, n) and dus.shape == (B, T, S, m)
    for got, want, what in zip((dxs, dus), with_headroom(tangent_reference, d, K, dx0, dv), ("dxs", "dus")):
        close(got, want, "%s, %d directions" % (what, S))
    assert np.array_equal(dxs[:, 0], dx0)  # as given, to the bit
    g_x0, g_v = g.adjoint(gx, gu)
    assert g_x0.shape == (B, S, n) and g_v.shape == (B, T, S, m)
    a, w = with_headroom(adjoint_reference, d, K, gx, gu)
    close(g_x0, a[:, 0], "g_x0, %d directions" % S)
    close(g_v, w, "g_v, %d directions" % S)


# ---- raw calls: one output at a time, buffers of the caller's -----------------------------------
def p(a):
    return None if a is None else a.ctypes.data_as(dp)


def raw_tangent(g, t0, nk, S, dx0, dv, dxs=True, dus=True, fill=0.0):
    nku = max(min(t0 + nk, g.T) - t0, 0)
    o_x = np.full((g.B, nk, S, g.nx), fill) if dxs else None
    o_u = np.full((g.B, nku, S, g.nu), fill) if dus else None
    rc = g.lib.ilqr_get_tangent(g.h, t0, nk, S, p(dx0), p(dv), p(o_x), p(o_u))
    return rc, o_x, o_u


def raw_adjoint(g, t0, nk, S, gx, gu, g_x0=True, g_v=True, fill=0.0):
    o_x = np.full((g.B, S, g.nx), fill) if g_x0 else None
    o_v = np.full((g.B, g.T, S, g.nu), fill) if g_v else None
    rc = g.lib.ilqr_get_adjoint(g.h, t0, nk, S, p(gx), p(gu), p(o_x), p(o_v))
    return rc, o_x, o_v


# ---- 1. generic layout -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def generic_policy(n, m, seed=0):
    """(d, k, K): computed once per size, shared, never written to."""
    return random_policy(n, m, seed=seed)


@pytest.mark.parametrize("n,m", GENERIC_SIZES)
def test_generic_layout(n, m):
    """One and two state tiles, one and two control tiles, ragged edges, the one- and two-control sizes; one direction, a full tile of
    them, a tile and one, two tiles and one."""
    d, k, K = generic_policy(n, m)
    g = host_handle(n, m, d, k, K)
    B, T = g.B, g.T
    # the transition matrices: dx0 = I
    Phi, KPhi = g.transition_matrices()
    assert Phi.shape == (B, T + 1, n, n) and KPhi.shape == (B, T, m, n)
    ref_x, ref_u = with_headroom(tangent_reference, d, K, identity_directions(n), None)
    close(Phi, np.swapaxes(ref_x, -1, -2), "Phi")
    close(KPhi, np.swapaxes(ref_u, -1, -2), "K Phi")
    assert np.array_equal(Phi[:, 0], identity_directions(n))
    for S in DIRECTION_COUNTS:
        check_both_calls(g, d, K, S)
    # g_v after a window that ends before T: exact zeros, whatever the buffer held
    S, t0, nk = 17, 2, 4
    _, _, gx, gu = directions(n, m, S)
    rc, _, g_v = raw_adjoint(g, t0, nk, S, np.ascontiguousarray(gx[:, t0:t0 + nk]), np.ascontiguousarray(gu[:, t0:t0 + nk]), fill=-7.0)
    assert rc == 0
    assert np.array_equal(g_v[:, t0 + nk:], np.zeros((B, T - t0 - nk, S, m))) and np.abs(g_v[:, :t0 + nk]).min() > 0
    pad_x, pad_u = np.zeros_like(gx), np.zeros_like(gu)
    pad_x[:, t0:t0 + nk], pad_u[:, t0:t0 + nk] = gx[:, t0:t0 + nk], gu[:, t0:t0 + nk]
    close(g_v, with_headroom(adjoint_reference, d, K, pad_x, pad_u)[1], "g_v of a window")
    g.close()


# ---- 2. column independence, bit for bit -------------------------------------------------------
def tiled_policy_handle(model="double_integrator", dtype="f64", B=20, T=30):
    g, x0, u0, _ = nx4_handle(model, dtype, B=B, T=T)
    g.init_traj(x0, u0)
    g.iterate(3)
    g.compute_derivatives()
    return g


@pytest.mark.parametrize("which", ["20x5", "32x32", "nx4"])
def test_a_column_depends_on_its_own_column_only(which):
    """Column 20 of a 33-direction call and column 3 of a 5-direction call equal the same direction computed alone, to the bit."""
    if which == "nx4":
        g = tiled_policy_handle()
    else:
        n, m = (20, 5) if which == "20x5" else (32, 32)
        g = host_handle(n, m, *generic_policy(n, m))
    for S, col in ((33, 20), (5, 3)):
        dx0, dv, gx, gu = directions(g.nx, g.nu, S, g.B, g.T)
        one = lambda a: np.ascontiguousarray(a[..., col:col + 1, :])
        dxs, dus = g.tangent(dx0, dv)
        dxs1, dus1 = g.tangent(one(dx0), one(dv))
        assert np.array_equal(dxs[:, :, col], dxs1[:, :, 0]) and np.array_equal(dus[:, :, col], dus1[:, :, 0]), (S, col)
        g_x0, g_v = g.adjoint(gx, gu)
        g_x01, g_v1 = g.adjoint(one(gx), one(gu))
        assert np.array_equal(g_x0[:, col], g_x01[:, 0]) and np.array_equal(g_v[:, :, col], g_v1[:, :, 0]), (S, col)
        assert np.abs(dxs1).max() > 0 and np.abs(g_v1).max() > 0
    g.close()


# ---- 3. the two kernels are each other's transposes --------------------------------------------
@pytest.mark.parametrize("which", ["20x5", "17x17", "32x32", "nx4"])
def test_transpose_identity_on_the_device(which):
    """sum_t <gx, dx> + sum_t <gu, du> = <g_x0, dx0> + sum_t <g_v, dv>, per trajectory and direction: k_tangent against k_adjoint."""
    if which == "nx4":
        g = tiled_policy_handle()
    else:
        n, m = {"20x5": (20, 5), "17x17": (17, 17), "32x32": (32, 32)}[which]
        g = host_handle(n, m, *generic_policy(n, m))
    dx0, dv, gx, gu = directions(g.nx, g.nu, 3, g.B, g.T)
    dxs, dus = g.tangent(dx0, dv)
    g_x0, g_v = g.adjoint(gx, gu)
    lhs = (gx * dxs).sum(axis=(1, 3)) + (gu * dus).sum(axis=(1, 3))
    rhs = (g_x0 * dx0).sum(axis=2) + (g_v * dv).sum(axis=(1, 3))
    err = float(np.abs(lhs - rhs).max())
    print("  <g, J d> vs <J'g, d>: %.3g (scale %.3g)" % (err, scale_of(lhs)))
    assert np.abs(lhs).max() > 0.1 and err <= 1e-9 * scale_of(lhs), (err, scale_of(lhs))
    g.close()


# ---- 4. against the existing kernels on the same handle ----------------------------------------
@pytest.mark.parametrize("n,m", [(20, 5), (32, 32)])
def test_against_the_value_and_covariance_kernels(n, m):
    """With k = 0 the adjoint of (cx, cu) is Vx of ilqr_get_value; with W = 0, Phi[T] Sigma0 Phi[T]' is Sigma[T] of ilqr_get_covariance."""
    from tests.test_gpu_covariance import noise_inputs
    d, k, K = generic_policy(n, m)
    g = host_handle(n, m, d, np.zeros_like(k), K)
    g_x0, _ = g.adjoint(d["cx"], np.ascontiguousarray(d["cu"][:, :-1]))  # (one direction: [B][T+1][nx], [B][T][nu])
    Vx, _ = g.value(0, 1)
    err = float(np.abs(g_x0 - Vx[:, 0]).max())
    print("  adjoint kernel vs value kernel Vx[0]: %.3g (scale %.3g)" % (err, scale_of(Vx)))
    assert g_x0.shape == (g.B, n) and err <= 1e-9 * scale_of(Vx), (err, scale_of(Vx))
    S0, _ = noise_inputs(n)
    Phi_T = g.transition_matrices(g.T, 1)[0][:, 0]
    want = g.covariance(S0, None, g.T, 1)[:, 0]
    got = Phi_T @ S0 @ np.swapaxes(Phi_T, -1, -2)
    err = float(np.abs(got - want).max())
    print("  Phi Sigma0 Phi' vs covariance kernel Sigma[T]: %.3g (scale %.3g)" % (err, scale_of(want)))
    assert err <= 1e-9 * scale_of(want), (err, scale_of(want))
    g.close()


# ---- 5. against the device model itself --------------------------------------------------------
def test_against_the_device_model():
    """An LQ model is linear and nothing clamps, so the closed loop maps x0 + e_i to x_end + Phi e_i exactly: Phi[T], column by column,
    from ilqr_evaluate_policy on n + 1 samples, and K[0] from its u_first over one knot."""
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
    Phi_T = np.swapaxes(x_end[:, 1:] - x_end[:, :1], -1, -2)  # column i: the image of e_i
    u_first = g.evaluate_policy(samples, 0, 1)["u_first"]
    K0 = np.swapaxes(u_first[:, 1:] - u_first[:, :1], -1, -2)
    Phi, KPhi = g.transition_matrices()
    for got, want, what in ((Phi[:, T], Phi_T, "Phi[T]"), (KPhi[:, 0], K0, "K[0]")):
        err = float(np.abs(got - want).max())
        print("  tangent vs the device model %s: %.3g (scale %.3g)" % (what, err, scale_of(want)))
        assert err <= TOL * scale_of(want), (what, err, scale_of(want))
    g.close()


# ---- 6. nx = 4 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model", ["acrobot", "double_integrator"])
def test_nx4(model, dtype):
    """B = 20 is no multiple of the 16-trajectory tile; the recursion is double in both dtypes, so one bound."""
    g = tiled_policy_handle(model, dtype)
    d, K = g.derivatives(), g.gains()[1]
    Phi, KPhi = g.transition_matrices()
    ref_x, ref_u = with_headroom(tangent_reference, d, K, identity_directions(4, g.B), None)
    close(Phi, np.swapaxes(ref_x, -1, -2), "Phi")
    close(KPhi, np.swapaxes(ref_u, -1, -2), "K Phi")
    for S in (1, 5):
        check_both_calls(g, d, K, S)
    g.close()


# ---- 7. fp32 generic ---------------------------------------------------------------------------
def test_fp32_generic():
    """Float records and gains are widened, the recursion is double: the definition on the handle's float-valued records and gains."""
    from ilqr_amd import BatchILQR
    from tests.test_gpu_lq_end_to_end import lq_mats
    n, m, B, T = 20, 5, 6, 12
    g = BatchILQR("lq", B, T, DT, lq=lq_mats(n, m), u_min=-0.5, u_max=0.5, dtype="f32")
    rng = np.random.default_rng(5)
    g.init_traj(rng.uniform(-1, 1, (B, n)), rng.normal(size=(B, T, m)) * 0.3)
    g.iterate(2)
    d, K = g.derivatives(), g.gains()[1]
    for S in (1, 17):
        check_both_calls(g, d, K, S)
    g.close()


# ---- 8. windows, NULLs, refusals ---------------------------------------------------------------
@pytest.fixture(scope="module")
def generic_handle():
    g = host_handle(20, 5, *generic_policy(20, 5, seed=1))
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
def test_windows_and_nulls(generic_handle, tiled_handle, which):
    g = generic_handle if which == "generic" else tiled_handle
    T, n, m, B, S = g.T, g.nx, g.nu, g.B, 3
    dx0, dv, gx, gu = directions(n, m, S, B, T)
    dxs, dus = g.tangent(dx0, dv)
    g_x0, g_v = g.adjoint(gx, gu)
    assert np.abs(dus).max() > 0 and np.abs(g_v).max() > 0
    cut = lambda a, t0, nk: np.ascontiguousarray(a[:, t0:t0 + nk])
    for t0, nk in ((3, 4), (0, 1), (T, 1), (T - 1, 2)):
        # the tangent's window is a slice of the full call
        w_x, w_u = g.tangent(dx0, dv, t0, nk)
        assert np.array_equal(w_x, dxs[:, t0:t0 + nk]) and np.array_equal(w_u, dus[:, t0:t0 + nk]), (t0, nk)
        # the adjoint's window is the full call with zeros outside it
        pad_x, pad_u = np.zeros_like(gx), np.zeros_like(gu)
        pad_x[:, t0:t0 + nk], pad_u[:, t0:t0 + nk] = gx[:, t0:t0 + nk], gu[:, t0:t0 + nk]
        full = g.adjoint(pad_x, pad_u)
        win = g.adjoint(cut(gx, t0, nk), cut(gu, t0, nk) if t0 < T else None, t0, nk)
        assert np.array_equal(win[0], full[0]) and np.array_equal(win[1], full[1]), (t0, nk)
        assert np.array_equal(win[1][:, t0 + nk:], np.zeros((B, max(T - t0 - nk, 0), S, m)))
    # each single output equals the paired call's
    t0, nk = 3, 4
    rc, o_x, o_u = raw_tangent(g, t0, nk, S, dx0, dv)
    assert rc == 0 and np.array_equal(o_x, dxs[:, 3:7]) and np.array_equal(o_u, dus[:, 3:7])
    assert np.array_equal(raw_tangent(g, t0, nk, S, dx0, dv, dus=False)[1], o_x) and np.array_equal(raw_tangent(g, t0, nk, S, dx0, dv, dxs=False)[2], o_u)
    rc, a_x, a_v = raw_adjoint(g, t0, nk, S, cut(gx, t0, nk), cut(gu, t0, nk))
    assert rc == 0 and np.abs(a_x).max() > 0
    assert np.array_equal(raw_adjoint(g, t0, nk, S, cut(gx, t0, nk), cut(gu, t0, nk), g_v=False)[1], a_x)
    assert np.array_equal(raw_adjoint(g, t0, nk, S, cut(gx, t0, nk), cut(gu, t0, nk), g_x0=False)[2], a_v)
    # NULL inputs are zeros
    for a, b in zip(g.tangent(dx0, None), g.tangent(dx0, np.zeros_like(dv))):
        assert np.array_equal(a, b)
    for a, b in zip(g.tangent(None, dv), g.tangent(np.zeros_like(dx0), dv)):
        assert np.array_equal(a, b) and np.abs(a).max() > 0
    for a, b in zip(g.adjoint(gx, None), g.adjoint(gx, np.zeros_like(gu))):
        assert np.array_equal(a, b)
    for a, b in zip(g.adjoint(None, gu), g.adjoint(np.zeros_like(gx), gu)):
        assert np.array_equal(a, b) and np.abs(a).max() > 0
    # one direction without the direction axis
    f_x, f_u = g.tangent(dx0[:, 1], dv[:, :, 1])
    assert f_x.shape == (B, T + 1, n) and np.array_equal(f_x, dxs[:, :, 1]) and np.array_equal(f_u, dus[:, :, 1])
    f_0, f_v = g.adjoint(gx[:, :, 1], gu[:, :, 1])
    assert f_0.shape == (B, n) and np.array_equal(f_0, g_x0[:, 1]) and np.array_equal(f_v, g_v[:, :, 1])
    # refusals: -1, nothing enqueued, the output buffers untouched
    buf_x, buf_u = np.full((B, T + 1, S, n), -7.0), np.full((B, T, S, m), -7.0)
    calls = (g.lib.ilqr_get_tangent, g.lib.ilqr_get_adjoint)
    dev_calls = (g.lib.ilqr_copy_tangent_to_device, g.lib.ilqr_copy_adjoint_to_device)
    for t0, nk in ((-1, 1), (0, 0), (T + 1, 1), (3, T), (0, T + 2), (T, 2), (2, -1)):  # bad windows
        for call in calls:
            assert call(g.h, t0, nk, S, p(buf_x), p(buf_u), p(buf_x), p(buf_u)) == -1, (t0, nk)
            assert b"window" in g.lib.ilqr_last_error()
        for call in dev_calls:
            assert call(g.h, t0, nk, S, buf_x.ctypes.data, buf_u.ctypes.data, buf_x.ctypes.data, buf_u.ctypes.data) == -1, (t0, nk)
    for S_bad in (0, -3, 2 ** 31 - 1):  # no direction; sizes beyond an int
        for call in calls:
            assert call(g.h, 0, 1, S_bad, p(buf_x), p(buf_u), p(buf_x), p(buf_u)) == -1, S_bad
        for call in dev_calls:
            assert call(g.h, 0, 1, S_bad, buf_x.ctypes.data, buf_u.ctypes.data, buf_x.ctypes.data, buf_u.ctypes.data) == -1, S_bad
    for call in calls:  # both inputs NULL; both outputs NULL
        assert call(g.h, 0, 2, S, None, None, p(buf_x), p(buf_u)) == -1 and b"both null" in g.lib.ilqr_last_error()
        assert call(g.h, 0, 2, S, p(buf_x), p(buf_u), None, None) == -1 and b"both null" in g.lib.ilqr_last_error()
    for call in dev_calls:
        assert call(g.h, 0, 2, S, None, None, buf_x.ctypes.data, buf_u.ctypes.data) == -1
        assert call(g.h, 0, 2, S, buf_x.ctypes.data, buf_u.ctypes.data, None, None) == -1
    # the control-sized array of the window when the window is knot T alone: dus (an output), gu (an input)
    assert g.lib.ilqr_get_tangent(g.h, T, 1, S, p(buf_x), None, p(buf_x), p(buf_u)) == -1 and b"knot T" in g.lib.ilqr_last_error()
    assert b"has no control" in g.lib.ilqr_last_error()
    assert g.lib.ilqr_copy_tangent_to_device(g.h, T, 1, S, buf_x.ctypes.data, None, None, buf_u.ctypes.data) == -1
    assert g.lib.ilqr_get_adjoint(g.h, T, 1, S, p(buf_x), p(buf_u), p(buf_x), None) == -1 and b"has no control" in g.lib.ilqr_last_error()
    assert g.lib.ilqr_copy_adjoint_to_device(g.h, T, 1, S, None, buf_u.ctypes.data, buf_x.ctypes.data, None) == -1
    g.synchronize()
    assert buf_x.min() == -7.0 == buf_x.max() and buf_u.min() == -7.0 == buf_u.max()


def test_fresh_handle_is_a_state_error():
    from ilqr_amd import BatchILQR
    for g in (BatchILQR("acrobot", 4, 10, DT), BatchILQR("host", 4, 10, DT, nx=6, nu=2, u_min=-1.0, u_max=1.0)):
        x, u = np.zeros((4, 11, 1, g.nx)), np.zeros((4, 10, 1, g.nu))
        assert g.lib.ilqr_get_tangent(g.h, 0, 1, 1, p(x), None, p(x), None) == -4
        assert g.lib.ilqr_copy_tangent_to_device(g.h, 0, 1, 1, x.ctypes.data, None, x.ctypes.data, None) == -4
        assert g.lib.ilqr_get_adjoint(g.h, 0, 1, 1, p(x), None, p(x), p(u)) == -4
        assert g.lib.ilqr_copy_adjoint_to_device(g.h, 0, 1, 1, x.ctypes.data, None, x.ctypes.data, None) == -4
        g.close()


# ---- 9. device variants ------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_copy_to_device_equals_the_getter(generic_handle, tiled_handle, which):
    import torch
    g = generic_handle if which == "generic" else tiled_handle
    t0, nk, S, B, n, m, T = 2, 5, 17, g.B, g.nx, g.nu, g.T
    dx0, dv, gx, gu = directions(n, m, S, B, T)
    gx, gu = np.ascontiguousarray(gx[:, t0:t0 + nk]), np.ascontiguousarray(gu[:, t0:t0 + nk])
    dxs, dus = g.tangent(dx0, dv, t0, nk)
    g_x0, g_v = g.adjoint(gx, gu, t0, nk)
    dev = lambda a: torch.from_numpy(a).cuda()
    fresh = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    d_dx0, d_dv, d_gx, d_gu = dev(dx0), dev(dv), dev(gx), dev(gu)
    d_dxs, d_dus, d_gx0, d_gv = fresh(B, nk, S, n), fresh(B, nk, S, m), fresh(B, S, n), fresh(B, T, S, m)
    torch.cuda.synchronize()  # (the copies and fills ran on torch's stream, the calls run on the handle's)
    g.copy_tangent_to_device(t0, nk, S, d_dx0.data_ptr(), d_dv.data_ptr(), d_dxs.data_ptr(), d_dus.data_ptr())
    g.copy_adjoint_to_device(t0, nk, S, d_gx.data_ptr(), d_gu.data_ptr(), d_gx0.data_ptr(), d_gv.data_ptr())
    g.synchronize()
    for got, want in ((d_dxs, dxs), (d_dus, dus), (d_gx0, g_x0), (d_gv, g_v)):
        assert np.array_equal(got.cpu().numpy(), want)
    # one output only: the other buffer is not touched
    for t in (d_dxs, d_dus, d_gx0, d_gv):
        t.fill_(-7.0)
    torch.cuda.synchronize()
    g.copy_tangent_to_device(t0, nk, S, d_dx0.data_ptr(), d_dv.data_ptr(), dus_ptr=d_dus.data_ptr())
    g.copy_adjoint_to_device(t0, nk, S, d_gx.data_ptr(), d_gu.data_ptr(), g_x0_ptr=d_gx0.data_ptr())
    g.synchronize()
    assert float(d_dxs.min()) == -7.0 == float(d_dxs.max()) and float(d_gv.min()) == -7.0 == float(d_gv.max())
    assert np.array_equal(d_dus.cpu().numpy(), dus) and np.array_equal(d_gx0.cpu().numpy(), g_x0)


# ---- 10. read-only -----------------------------------------------------------------------------
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
    check_both_calls(g, g.derivatives(), g.gains()[1], 5)
    for h in (g, twin):
        h.iterate(3)
    for a, b in zip(g.trajectory() + g.gains() + (g.cost(),) + g.lambdas(), twin.trajectory() + twin.gains() + (twin.cost(),) + twin.lambdas()):
        assert np.array_equal(a, b)
    g.close()
    twin.close()


# ---- 11. C++ callers of the facade -------------------------------------------------------------
CALLER = r'''
#include "ilqr_amd.hpp"
#include <cmath>
#include <cstdio>
int main() {
  using namespace ilqr_amd;
  const int T = 20, S = 3;
  VectorXd goal(4);
  goal(0) = 1.0; goal(1) = 0.5; goal(2) = 0.0; goal(3) = 0.0;
  iLQR s(new DoubleIntegrator(goal), 0.02);
  s.verbose = false;
  VectorXd x0(4);
  x0(0) = 0.2; x0(1) = -0.1; x0(2) = 0.0; x0(3) = 0.1;
  VectorXd u(2);
  u(0) = 0.0; u(1) = 0.0;
  VecOfVecXd u0(T, u);
  s.init_traj(x0, u0);
  s.generate_trajectory();
  // Phi: dx0 = I
  MatrixXd I4(4, 4);
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) I4(i, j) = i == j ? 1.0 : 0.0;
  VecOfMatXd Phi, KPhi;
  s.tangent(I4, VecOfMatXd(), Phi, &KPhi);
  if ((int)Phi.size() != T + 1 || (int)KPhi.size() != T || Phi[0].rows() != 4 || Phi[0].cols() != 4 || KPhi[0].rows() != 2 || KPhi[0].cols() != 4) return 1;
  double first = 0;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) first = std::fmax(first, std::fabs(Phi[0](i, j) - I4(i, j)));
  // S directions with perturbed controls; the adjoint of some cotangents; the transpose identity
  MatrixXd dx0(4, S);
  VecOfMatXd dv(T), gx(T + 1), gu(T);
  for (int c = 0; c < S; c++)
    for (int i = 0; i < 4; i++) dx0(i, c) = 0.3 * std::sin(1.0 + i + 4 * c);
  for (int t = 0; t <= T; t++) {
    gx[t] = MatrixXd(4, S);
    for (int c = 0; c < S; c++)
      for (int i = 0; i < 4; i++) gx[t](i, c) = std::cos(0.7 * t + i - c);
    if (t == T) break;
    dv[t] = MatrixXd(2, S);
    gu[t] = MatrixXd(2, S);
    for (int c = 0; c < S; c++)
      for (int j = 0; j < 2; j++) { dv[t](j, c) = 0.1 * std::sin(0.3 * t + j + c); gu[t](j, c) = std::sin(0.5 * t - j + 2 * c); }
  }
  VecOfMatXd dxs, dus, g_v;
  MatrixXd g_x0;
  s.tangent(dx0, dv, dxs, &dus);
  s.adjoint(gx, gu, g_x0, &g_v);
  if ((int)dxs.size() != T + 1 || (int)dus.size() != T || (int)g_v.size() != T || g_x0.rows() != 4 || g_x0.cols() != S) return 1;
  double gap = 0, big = 0;
  for (int c = 0; c < S; c++) {
    double lhs = 0, rhs = 0;
    for (int i = 0; i < 4; i++) rhs += g_x0(i, c) * dx0(i, c);
    for (int t = 0; t <= T; t++)
      for (int i = 0; i < 4; i++) lhs += gx[t](i, c) * dxs[t](i, c);
    for (int t = 0; t < T; t++)
      for (int j = 0; j < 2; j++) { lhs += gu[t](j, c) * dus[t](j, c); rhs += g_v[t](j, c) * dv[t](j, c); }
    gap = std::fmax(gap, std::fabs(lhs - rhs));
    big = std::fmax(big, std::fabs(lhs));
  }
  // a window is a slice
  VecOfMatXd Win, WinU;
  s.tangent(dx0, dv, Win, &WinU, 3, 2);
  double win = 0;
  for (int c = 0; c < S; c++) {
    for (int i = 0; i < 4; i++) win = std::fmax(win, std::fabs(Win[1](i, c) - dxs[4](i, c)));
    for (int j = 0; j < 2; j++) win = std::fmax(win, std::fabs(WinU[0](j, c) - dus[3](j, c)));
  }
  std::printf("first %g identity gap %g of %g window %g\n", first, gap, big, win);
  return (first == 0 && big > 0.1 && gap <= 1e-9 * std::fmax(1.0, big) && win == 0 && Win.size() == 2 && WinU.size() == 2) ? 0 : 2;
}
'''

BATCH_CALLER = r'''
#include "ilqr_amd.hpp"
#include <cmath>
#include <cstdio>
int main() {
  using namespace ilqr_amd;
  const int B = 3, T = 15, S = 4;
  VectorXd goal(4);
  goal(0) = 1.0; goal(1) = 0.5; goal(2) = 0.0; goal(3) = 0.0;
  BatchILQR b(std::make_shared<DoubleIntegrator>(goal), B, T, 0.02);
  std::vector<double> x0((size_t)B * 4), u0((size_t)B * T * 2, 0.0);
  for (size_t i = 0; i < x0.size(); i++) x0[i] = 0.1 * (double)(i % 5) - 0.2;
  b.init_traj(x0, u0);
  b.iterate(2);
  // dx0 = I per trajectory: [B][S = 4][nx]
  std::vector<double> dx0((size_t)B * S * 4, 0.0), dv((size_t)B * T * S * 2), gx((size_t)B * (T + 1) * S * 4), gu((size_t)B * T * S * 2);
  for (int t = 0; t < B; t++)
    for (int i = 0; i < 4; i++) dx0[((size_t)t * S + i) * 4 + i] = 1.0;
  for (size_t i = 0; i < dv.size(); i++) dv[i] = 0.1 * std::sin(0.37 * (double)i);
  for (size_t i = 0; i < gx.size(); i++) gx[i] = std::cos(0.11 * (double)i);
  for (size_t i = 0; i < gu.size(); i++) gu[i] = std::sin(0.23 * (double)i + 1.0);
  std::vector<double> Phi, dxs, dus, g_x0, g_v, Win, WinU, OnlyX;
  b.tangent(S, &dx0, nullptr, &Phi, nullptr);
  if (Phi.size() != (size_t)B * (T + 1) * S * 4) return 1;
  double first = 0;
  for (int t = 0; t < B; t++)
    for (int e = 0; e < S * 4; e++) first = std::fmax(first, std::fabs(Phi[(size_t)t * (T + 1) * S * 4 + e] - dx0[(size_t)t * S * 4 + e]));
  b.tangent(S, &dx0, &dv, &dxs, &dus);
  b.adjoint(S, &gx, &gu, &g_x0, &g_v);
  if (dxs.size() != (size_t)B * (T + 1) * S * 4 || dus.size() != (size_t)B * T * S * 2 || g_x0.size() != (size_t)B * S * 4 || g_v.size() != dv.size()) return 1;
  double lhs = 0, rhs = 0;  // (summed over trajectories and directions: one number)
  for (size_t i = 0; i < gx.size(); i++) lhs += gx[i] * dxs[i];
  for (size_t i = 0; i < gu.size(); i++) lhs += gu[i] * dus[i];
  for (size_t i = 0; i < dx0.size(); i++) rhs += g_x0[i] * dx0[i];
  for (size_t i = 0; i < dv.size(); i++) rhs += g_v[i] * dv[i];
  b.tangent(S, &dx0, &dv, &Win, &WinU, 3, 4);
  b.tangent(S, &dx0, &dv, &OnlyX, nullptr, 3, 4);
  double win = 0;
  for (int t = 0; t < B; t++)
    for (int k = 0; k < 4; k++) {
      for (int e = 0; e < S * 4; e++) {
        const double v = dxs[((size_t)t * (T + 1) + 3 + k) * S * 4 + e];
        win = std::fmax(win, std::fabs(Win[((size_t)t * 4 + k) * S * 4 + e] - v));
        win = std::fmax(win, std::fabs(OnlyX[((size_t)t * 4 + k) * S * 4 + e] - v));
      }
      for (int e = 0; e < S * 2; e++) win = std::fmax(win, std::fabs(WinU[((size_t)t * 4 + k) * S * 2 + e] - dus[((size_t)t * T + 3 + k) * S * 2 + e]));
    }
  std::printf("first %g identity %g vs %g window %g\n", first, lhs, rhs, win);
  return (first == 0 && std::fabs(lhs) > 0.1 && std::fabs(lhs - rhs) <= 1e-9 * std::fmax(1.0, std::fabs(lhs)) && win == 0) ? 0 : 2;
}
'''


@pytest.mark.parametrize("which", ["iLQR", "BatchILQR"])
def test_facade_sensitivity_members(tmp_path, which):
    """C++ callers of the facade's tangent() / adjoint(): the single-problem iLQR (one nx x n_dirs matrix per knot) and BatchILQR's plain
    vectors; Phi[0] = I, a window is a slice, the transpose identity holds to 1e-9."""
    from ilqr_amd import _build
    _build.build()
    src = tmp_path / "sensitivity_caller.cpp"
    src.write_text(CALLER if which == "iLQR" else BATCH_CALLER)
    exe = str(tmp_path / "sensitivity_caller")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-DILQR_AMD_NO_EIGEN", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + os.path.join(ROOT, "ilqr_amd", "lib"), "-lilqr_amd", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "ilqr_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- every request through the staging buffer ---------------------------------------------------
from tests import getter_vs_device as gd  # noqa: E402


@pytest.mark.parametrize("case", gd.CASES)
@pytest.mark.parametrize("call", ["tangent", "adjoint"])
@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_getter_equals_the_device_form_request_by_request(which, call, case):
    """ilqr_get_tangent / ilqr_get_adjoint against their device forms, bit for bit: every pointer; the last input and the last output
    alone (a call without inputs is refused); that, every pointer, that again on one handle."""

    def args(g):
        rng, per_x, per_u = np.random.default_rng(3), gd.B * gd.ND * g.nx, gd.B * gd.ND * g.nu
        x_one, u_all, x_win, u_win = per_x, per_u * gd.T, per_x * gd.NK, per_u * (min(gd.T0 + gd.NK, gd.T) - gd.T0)
        if call == "tangent":
            return [gd.Arg("dx0", "in", rng.normal(size=x_one)), gd.Arg("dv", "in", rng.normal(size=u_all)), gd.Arg("dxs", "out", (x_win,)), gd.Arg("dus", "out", (u_win,))]
        return [gd.Arg("gx", "in", rng.normal(size=x_win)), gd.Arg("gu", "in", rng.normal(size=u_win)), gd.Arg("g_x0", "out", (x_one,)), gd.Arg("g_v", "out", (u_all,))]
    gd.check(lambda: gd.handle(which), case, "ilqr_get_%s" % call, "ilqr_copy_%s_to_device" % call, (gd.T0, gd.NK, gd.ND), args, needs_input=True)
