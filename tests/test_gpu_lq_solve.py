"""ilqr_solve_lq / ilqr_solve_lq_on_device on the device (k_lq_gain_w, k_lq_back_w, k_lq_fwd_w on the generic layout; k_lq_gain_t, k_lq_dir_t
on the tiled one): against a numpy restatement of the header's definition, the KKT residuals of the device's own outputs, column
independence to the bit, against the solver's own backward pass, a Quu that is not positive definite, NULLs and refusals, the device
form, that asking changes nothing a later iteration computes, and a C++ caller of the facade.

Yardstick: lq_reference(records, K, dx0, gx, gu, mu, hold), float64.  Between it and the device the bound is the project's
1e-9 x max(1, max|.|); every input is first put through the same recursion in np.longdouble, which has to agree with float64 within
1e-10 x the same scale -- a factor 10 of headroom -- before the bound is relied on (with_headroom).  tests/test_lq_solve_abi.py checks the
yardstick itself against a dense KKT solve on the CPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_value import GENERIC_SIZES, host_handle, nx4_handle
from tests.util import TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.02
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int)
DIRECTION_COUNTS = (1, 16, 17, 33)
NX4_MU = 1.0  # (the yardstick on the nx = 4 handles' own records reports info == 0 everywhere at this value: test_nx4 requires it)


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """The device-form case uses torch tensors: torch's device is initialised before this module creates any handle."""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


# ---- the yardstick -----------------------------------------------------------------------------
def cholesky_lower(A):
    """Lower Cholesky in index order, any dtype: (L, 0), or (None, 1) at a pivot that is <= 0 or not finite."""
    m = A.shape[0]
    L = np.zeros_like(A)
    for j in range(m):
        piv = A[j, j] - L[j, :j] @ L[j, :j]
        if not (piv > 0) or not np.isfinite(piv):
            return None, 1
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, 0


def cholesky_solve(L, R):
    """(L L')^-1 R, any dtype."""
    m = L.shape[0]
    Y = np.array(R, dtype=L.dtype)
    for i in range(m):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    for i in range(m - 1, -1, -1):
        Y[i] = (Y[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y


def held_rows(K, hold):
    """[B][T][m] bool: row e of K[t] is exactly zero (with the flag)."""
    return (np.asarray(K) == 0).all(axis=-1) if hold else np.zeros(np.asarray(K).shape[:-1], dtype=bool)


def lq_reference(d, K, dx0=None, gx=None, gu=None, mu=0.0, hold=True, dtype=np.float64):
    """The definition of include/ilqr_amd.h (ilqr_solve_lq).  d: the records as BatchILQR.derivatives() returns them (matrices
    [B][T+1][rows][cols]); K [B][T][m][n]; dx0 [B][S][n], gx [B][T+1][S][n], gu [B][T][S][m] or None (zero).
    Returns dxs [B][T+1][S][n], dus [B][T][S][m], dlam [B][T+1][S][n], info [B]."""
    fx, fu, cxx, cxu, cuu = (np.asarray(d[k], dtype=dtype) for k in ("fx", "fu", "cxx", "cxu", "cuu"))
    B, T, m, n = np.asarray(K).shape
    S = next(a for a in (dx0, gx, gu) if a is not None).shape[-2]
    held = held_rows(K, hold)
    mu = dtype(mu)
    half = dtype(0.5)
    dxs, dus, dlam = np.zeros((B, T + 1, S, n), dtype=dtype), np.zeros((B, T, S, m), dtype=dtype), np.zeros((B, T + 1, S, n), dtype=dtype)
    info = np.zeros(B, dtype=np.int32)
    for b in range(B):
        P = [None] * (T + 1)
        Kd, Ls = [None] * T, [None] * T
        P[T] = cxx[b, T]
        for t in range(T - 1, -1, -1):
            A, Bm = fx[b, t], fu[b, t]
            Qxx = cxx[b, t] + A.T @ P[t + 1] @ A
            Qux = cxu[b, t].T + Bm.T @ P[t + 1] @ A
            Quu = cuu[b, t] + Bm.T @ P[t + 1] @ Bm + mu * np.eye(m, dtype=dtype)
            F = np.flatnonzero(~held[b, t])
            Kd[t] = np.zeros((m, n), dtype=dtype)
            if len(F):
                Ls[t], bad = cholesky_lower(Quu[np.ix_(F, F)])
                if bad:
                    info[b] = t + 1
                    break
                Kd[t][F] = -cholesky_solve(Ls[t], Qux[F])
            Pn = Qxx + Qux.T @ Kd[t]
            P[t] = half * (Pn + Pn.T)
        if info[b]:
            dxs[b], dus[b], dlam[b] = np.nan, np.nan, np.nan
            continue
        # directions are rows: (M x)' = x' M'
        v = [None] * (T + 1)
        kd = [None] * T
        v[T] = np.asarray(gx[b, T], dtype=dtype) if gx is not None else np.zeros((S, n), dtype=dtype)
        for t in range(T - 1, -1, -1):
            w = v[t + 1] @ fu[b, t]
            if gu is not None:
                w = w + np.asarray(gu[b, t], dtype=dtype)
            F = np.flatnonzero(~held[b, t])
            kd[t] = np.zeros((S, m), dtype=dtype)
            if len(F):
                kd[t][:, F] = -cholesky_solve(Ls[t], w[:, F].T).T
            v[t] = v[t + 1] @ fx[b, t] + w @ Kd[t]
            if gx is not None:
                v[t] = v[t] + np.asarray(gx[b, t], dtype=dtype)
        x = np.asarray(dx0[b], dtype=dtype) if dx0 is not None else np.zeros((S, n), dtype=dtype)
        for t in range(T + 1):
            dxs[b, t] = x
            dlam[b, t] = x @ P[t].T + v[t]
            if t == T:
                break
            dus[b, t] = x @ Kd[t].T + kd[t]
            x = x @ fx[b, t].T + dus[b, t] @ fu[b, t].T
    return dxs, dus, dlam, info


def scale_of(a):
    return max(1.0, float(np.abs(a).max()))


def with_headroom(d, K, dx0, gx, gu, mu, hold):
    """lq_reference(...) in float64, after the float64 and np.longdouble recursions have agreed within 1e-10 x max(1, max|.|)."""
    ref = lq_reference(d, K, dx0, gx, gu, mu, hold)
    lng = lq_reference(d, K, dx0, gx, gu, mu, hold, dtype=np.longdouble)
    assert np.array_equal(ref[3], lng[3])
    ok = ref[3] == 0
    for a, b, what in zip(ref[:3], lng[:3], ("dxs", "dus", "dlam")):
        gap = float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0
        print("  float64 vs longdouble %s: %.3g (scale %.3g)" % (what, gap, scale_of(a[ok]) if ok.any() else 1.0))
        assert not ok.any() or gap <= 1e-10 * scale_of(a[ok]), (what, gap)
    return ref


def close(got, want, what, bound=1e-9):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got - want).max())
    print("  device vs reference %s: %.3g (scale %.3g)" % (what, err, scale_of(want)))
    assert err <= bound * scale_of(want), (what, err, scale_of(want))


@functools.lru_cache(maxsize=None)
def convex_policy(n, m, B=5, T=12, seed=0):
    """(d, k, K): convex records [cxx cxu; cxu' cuu] = 0.5 I + G G', G ~ N(0, 1) / sqrt(n + m) per knot; fx, fu, K as random_policy makes
    them (30 % of K's rows zeroed).  Computed once per size, shared, never written to."""
    rng = np.random.default_rng(7000 * n + m + seed)
    G = rng.normal(size=(B, T + 1, n + m, n + m)) / np.sqrt(n + m)
    H = 0.5 * np.eye(n + m) + G @ np.swapaxes(G, -1, -2)
    d = dict(fx=np.eye(n) + 0.1 * rng.normal(size=(B, T + 1, n, n)) / np.sqrt(n), fu=rng.normal(size=(B, T + 1, n, m)) / np.sqrt(n),
             cx=rng.normal(size=(B, T + 1, n)), cu=rng.normal(size=(B, T + 1, m)),
             cxx=np.ascontiguousarray(H[..., :n, :n]), cxu=np.ascontiguousarray(H[..., :n, n:]), cuu=np.ascontiguousarray(H[..., n:, n:]))
    k = 0.5 * rng.normal(size=(B, T, m))
    K = 0.5 * rng.normal(size=(B, T, m, n)) / np.sqrt(n)
    K[rng.uniform(size=(B, T, m)) < 0.3] = 0.0
    return d, k, K


def directions(n, m, S, B=5, T=12, seed=0):
    """(dx0 [B][S][n], gx [B][T+1][S][n], gu [B][T][S][m]): standard normal."""
    rng = np.random.default_rng(9500 + 100 * n + m + 7 * S + seed)
    return rng.normal(size=(B, S, n)), rng.normal(size=(B, T + 1, S, n)), rng.normal(size=(B, T, S, m))


def check_call(g, d, K, S, mu, hold, dx0, gx, gu, what=""):
    """One call on the handle against the yardstick; returns the device's outputs."""
    ref = with_headroom(d, K, dx0, gx, gu, mu, hold)
    dxs, dus, dlam, info = g.lq_solve(gx=gx, gu=gu, dx0=dx0, mu=mu, hold_clamped=hold, dlam=True)
    assert info.dtype == np.int32 and np.array_equal(info, ref[3]) and not info.any(), (info, ref[3])
    for got, want, name in zip((dxs, dus, dlam), ref[:3], ("dxs", "dus", "dlam")):
        close(got, want, "%s %s, %d directions" % (name, what, S))
    held = held_rows(K, hold)
    assert np.array_equal(dus[held[:, :, None, :].repeat(S, axis=2)], np.zeros(int(held.sum()) * S))  # held controls: exact zeros
    assert np.array_equal(dxs[:, 0], dx0 if dx0 is not None else np.zeros_like(dxs[:, 0]))           # as given, to the bit
    return dxs, dus, dlam


# ---- 1. generic layout -------------------------------------------------------------------------
@pytest.mark.parametrize("mu,hold", [(0.0, True), (0.7, False)])
@pytest.mark.parametrize("n,m", GENERIC_SIZES)
def test_generic_layout(n, m, mu, hold):
    d, k, K = convex_policy(n, m)
    g = host_handle(n, m, d, k, K)
    for S in DIRECTION_COUNTS:
        dx0, gx, gu = directions(n, m, S)
        check_call(g, d, K, S, mu, hold, dx0, gx, gu)
    S = 3
    dx0, gx, gu = directions(n, m, S)
    check_call(g, d, K, S, mu, hold, None, gx, gu, "(dx0 NULL)")
    check_call(g, d, K, S, mu, hold, dx0, None, gu, "(gx NULL)")
    check_call(g, d, K, S, mu, hold, dx0, gx, None, "(gu NULL)")
    g.close()


# ---- 2. KKT residuals of the device's own outputs ----------------------------------------------
@pytest.mark.parametrize("n,m", [(20, 5), (32, 32), (6, 2)])
def test_kkt_residuals_of_the_outputs(n, m):
    """No recursion trusted: the dynamics, the multipliers' recursion and stationarity on the free controls, from the outputs alone."""
    d, k, K = convex_policy(n, m)
    g = host_handle(n, m, d, k, K)
    B, T, S = g.B, g.T, 17
    tr = lambda M: np.swapaxes(M, -1, -2)
    for mu, hold in ((0.0, True), (0.7, False)):
        dx0, gx, gu = directions(n, m, S)
        dxs, dus, dlam, info = g.lq_solve(gx=gx, gu=gu, dx0=dx0, mu=mu, hold_clamped=hold, dlam=True)
        assert not info.any()
        fx, fu, cxx, cxu, cuu = (d[kk][:, :T] for kk in ("fx", "fu", "cxx", "cxu", "cuu"))
        x, u = dxs[:, :T], dus
        dyn = dxs[:, 1:] - (x @ tr(fx) + u @ tr(fu))
        lam = dlam[:, :T] - (gx[:, :T] + x @ tr(cxx) + u @ tr(cxu) + dlam[:, 1:] @ fx)
        lamT = dlam[:, T] - (gx[:, T] + dxs[:, T] @ tr(d["cxx"][:, T]))
        stat = u @ tr(cuu + mu * np.eye(m)) + x @ cxu + gu + dlam[:, 1:] @ fu
        stat[held_rows(K, hold)[:, :, None, :].repeat(S, axis=2)] = 0.0  # (free rows only)
        for r, ref, what in ((dyn, dxs, "dynamics"), (lam, dlam, "dlam recursion"), (lamT, dlam, "dlam[T]"), (stat, dlam, "stationarity")):
            err = float(np.abs(r).max())
            print("  KKT residual %s: %.3g (scale %.3g)" % (what, err, scale_of(ref)))
            assert err <= 1e-9 * scale_of(ref), (what, err)
    g.close()


# ---- 3. nx = 4 ---------------------------------------------------------------------------------
def tiled_policy_handle(model="double_integrator", dtype="f64", B=20, T=30):
    g, x0, u0, _ = nx4_handle(model, dtype, B=B, T=T)
    g.init_traj(x0, u0)
    g.iterate(3)
    g.compute_derivatives()
    return g


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model", ["acrobot", "double_integrator"])
def test_nx4(model, dtype):
    """B = 20 is no multiple of the 16-trajectory tile; the recursion is double in both dtypes, so one bound.  mu = NX4_MU keeps the
    acrobot's finite-difference cuu from deciding the outcome: the yardstick reports info == 0 on every trajectory."""
    g = tiled_policy_handle(model, dtype)
    d, K = g.derivatives(), g.gains()[1]
    for S, hold in ((1, True), (5, False)):
        dx0, gx, gu = directions(4, g.nu, S, g.B, g.T)
        ref = with_headroom(d, K, dx0, gx, gu, NX4_MU, hold)
        assert not ref[3].any(), ref[3]
        check_call(g, d, K, S, NX4_MU, hold, dx0, gx, gu)
    g.close()


def test_fp32_generic():
    """Float records and gains are widened, the recursion is double: the definition on the handle's float-valued records and gains (the
    LQ model's cxx, cuu are positive definite: mu = 0)."""
    from ilqr_amd import BatchILQR
    from tests.test_gpu_lq_end_to_end import lq_mats
    n, m, B, T = 20, 5, 6, 12
    g = BatchILQR("lq", B, T, DT, lq=lq_mats(n, m), u_min=-0.5, u_max=0.5, dtype="f32")
    rng = np.random.default_rng(5)
    g.init_traj(rng.uniform(-1, 1, (B, n)), rng.normal(size=(B, T, m)) * 0.3)
    g.iterate(2)
    d, K = g.derivatives(), g.gains()[1]
    for S, hold in ((1, True), (17, False)):
        dx0, gx, gu = directions(n, m, S, B, T)
        check_call(g, d, K, S, 0.0, hold, dx0, gx, gu)
    g.close()


# ---- 4. column independence, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("which", ["20x5", "32x32", "nx4"])
def test_a_column_depends_on_its_own_column_only(which):
    """Column 20 of a 33-direction call and column 3 of a 5-direction call equal the same direction computed alone, to the bit."""
    if which == "nx4":
        g, mu = tiled_policy_handle(), NX4_MU
    else:
        n, m = (20, 5) if which == "20x5" else (32, 32)
        g, mu = host_handle(n, m, *convex_policy(n, m)), 0.0
    for S, col in ((33, 20), (5, 3)):
        dx0, gx, gu = directions(g.nx, g.nu, S, g.B, g.T)
        one = lambda a: np.ascontiguousarray(a[..., col:col + 1, :])
        many = g.lq_solve(gx=gx, gu=gu, dx0=dx0, mu=mu, dlam=True)
        alone = g.lq_solve(gx=one(gx), gu=one(gu), dx0=one(dx0), mu=mu, dlam=True)
        assert not many[3].any() and not alone[3].any()
        for a, b in zip(many[:3], alone[:3]):
            assert np.array_equal(a[:, :, col], b[:, :, 0]) and np.abs(b).max() > 0, (S, col)
    g.close()


# ---- 5. against the solver's own backward pass -------------------------------------------------
@pytest.mark.parametrize("n,m", [(32, 16), (24, 20)])
def test_against_the_solvers_backward_pass(oracle, n, m):
    """An LQ-model host handle with limits so wide that nothing clamps, lambda = 0: the backward pass's k, K are the LQ solution, so
    lq_solve(gx = cx, gu = cu).dus is the tangent of dv = k, and lq_solve(dx0 = I).dus is K Phi."""
    from ilqr_amd import BatchILQR
    from tests.test_gpu_generic_backward import lq_model
    from tests.util import mat
    om = lq_model(oracle, n, m, lim=1e3)
    B, T = 8, 12
    rng = np.random.default_rng(3)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.3
    xs, us, cost = oracle.batch_rollout(om, x0, u0, DT)
    dv = oracle.batch_derivatives(om, xs, us, DT)
    k_prev = np.zeros((B, T, m))
    ro = oracle.batch_backward(om, us, dv, k_prev=k_prev, lam=0.0)
    assert (ro["diverge"] != 0).sum() <= B // 8  # (the oracle alone: checkable without a GPU)
    g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=om.u_min, u_max=om.u_max)
    g.set_trajectory(x0=x0, xs=xs, us=us, cost=cost)
    g.set_derivatives(**{kk: (dv[kk] if kk in ("cx", "cu") else mat(dv[kk])) for kk in dv})
    g.set_gains(k=k_prev, K=np.zeros((B, T, m, n)))
    g.set_lambda(0.0, 1.0)
    div = g.backward_pass()
    ok = div == 0
    assert ok.sum() >= B - B // 8
    k, K = g.gains()
    assert np.abs(K).min(axis=-1).max() > 0 and (np.abs(K).max(axis=-1) > 0)[ok].all()  # nothing clamped
    d = g.derivatives()
    dus, info = g.lq_solve(gx=d["cx"], gu=np.ascontiguousarray(d["cu"][:, :-1]), mu=0.0, hold_clamped=False)[1:]
    want = g.tangent(dv=k)[1]
    assert not info[ok].any()
    err = float(np.abs(dus[ok] - want[ok]).max())
    print("  lq_solve(cx, cu).dus vs tangent(dv = k): %.3g (scale %.3g)" % (err, scale_of(want[ok])))
    assert err <= TOL * scale_of(want[ok]), (err, scale_of(want[ok]))
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(n), (B, n, n)))
    dus, info = g.lq_solve(dx0=eye, mu=0.0, hold_clamped=False)[1:]
    KPhi = g.transition_matrices()[1]
    err = float(np.abs(np.swapaxes(dus, -1, -2)[ok] - KPhi[ok]).max())
    print("  lq_solve(dx0 = I).dus vs K Phi: %.3g (scale %.3g)" % (err, scale_of(KPhi[ok])))
    assert err <= TOL * scale_of(KPhi[ok]), (err, scale_of(KPhi[ok]))
    g.close()


# ---- 6. not positive definite ------------------------------------------------------------------
def indefinite_case(n, m):
    """(sound records, the same with cuu[2, 7] = -1e3 I, K with every control of that knot free, K with every control of it held)."""
    d, k, K = convex_policy(n, m) if n != 4 else convex_policy(n, m, B=5, T=12)
    bad = {kk: np.array(vv) for kk, vv in d.items()}
    bad["cuu"][2, 7] = -1e3 * np.eye(m)
    K_free, K_held = np.array(K), np.array(K)
    K_free[2, 7] = 0.25
    K_held[2, 7] = 0.0
    return d, bad, k, K_free, K_held


@pytest.mark.parametrize("n,m", [(20, 5), (32, 32), (4, 1), (4, 2)])
def test_not_positive_definite(n, m):
    d, bad, k, K_free, K_held = indefinite_case(n, m)
    S = 3
    dx0, gx, gu = directions(n, m, S)
    assert np.array_equal(lq_reference(bad, K_free, dx0, gx, gu)[3], [0, 0, 8, 0, 0])  # (the yardstick says the same)
    if n == 4:
        from ilqr_amd import BatchILQR
        g = BatchILQR("double_integrator", 5, 12, DT, u_min=-1.0, u_max=1.0) if m == 2 else BatchILQR("acrobot", 5, 12, DT, u_min=-1.0, u_max=1.0)
        assert g.nu == m
        g.init_traj(np.zeros((5, 4)), np.zeros((5, 12, m)))
        setup = lambda recs, K: (g.set_derivatives(**recs), g.set_gains(k=k, K=K))
    else:
        g = host_handle(n, m, d, k, K_free)
        setup = lambda recs, K: (g.set_derivatives(**recs), g.set_gains(k=k, K=K))
    setup(d, K_free)
    sound = g.lq_solve(gx=gx, gu=gu, dx0=dx0, dlam=True)
    assert not sound[3].any()
    setup(bad, K_free)
    got = g.lq_solve(gx=gx, gu=gu, dx0=dx0, dlam=True)
    assert np.array_equal(got[3], [0, 0, 8, 0, 0]), got[3]
    others = [0, 1, 3, 4]
    for a, b in zip(got[:3], sound[:3]):
        assert np.isnan(a[2]).all() and np.array_equal(a[others], b[others])
    setup(bad, K_held)
    held = g.lq_solve(gx=gx, gu=gu, dx0=dx0, dlam=True)
    assert not held[3].any() and all(np.isfinite(a).all() for a in held[:3])
    ref = lq_reference(bad, K_held, dx0, gx, gu)
    for a, b, what in zip(held[:3], ref[:3], ("dxs", "dus", "dlam")):
        close(a, b, what + " with the bad knot held")
    g.close()


# ---- 7. refusals and edge cases ----------------------------------------------------------------
def p(a):
    return None if a is None else a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def generic_handle():
    g = host_handle(20, 5, *convex_policy(20, 5, seed=1))
    yield g
    g.close()


@pytest.fixture(scope="module")
def tiled_handle():
    g = tiled_policy_handle()
    yield g
    g.close()


@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_refusals_and_null_info(generic_handle, tiled_handle, which):
    g = generic_handle if which == "generic" else tiled_handle
    B, T, n, m, S = g.B, g.T, g.nx, g.nu, 3
    dx0, gx, gu = directions(n, m, S, B, T)
    mu = 0.0 if which == "generic" else NX4_MU
    dxs, dus, dlam, info = g.lq_solve(gx=gx, gu=gu, dx0=dx0, mu=mu, dlam=True)
    assert not info.any()
    # info = NULL works; each single output equals the full call's
    o_x, o_u, o_l = np.zeros_like(dxs), np.zeros_like(dus), np.zeros_like(dlam)
    assert g.lib.ilqr_solve_lq(g.h, S, 1, mu, p(dx0), p(gx), p(gu), p(o_x), p(o_u), p(o_l), None) == 0
    assert np.array_equal(o_x, dxs) and np.array_equal(o_u, dus) and np.array_equal(o_l, dlam)
    for keep in range(3):
        outs = [np.full_like(a, -7.0) if i == keep else None for i, a in enumerate((dxs, dus, dlam))]
        assert g.lib.ilqr_solve_lq(g.h, S, 1, mu, p(dx0), p(gx), p(gu), p(outs[0]), p(outs[1]), p(outs[2]), None) == 0
        assert np.array_equal(outs[keep], (dxs, dus, dlam)[keep]), keep
    # one direction without the direction axis
    f = g.lq_solve(gx=gx[:, :, 1], gu=gu[:, :, 1], dx0=dx0[:, 1], mu=mu, dlam=True)
    assert f[0].shape == (B, T + 1, n) and all(np.array_equal(a, b[:, :, 1]) for a, b in zip(f[:3], (dxs, dus, dlam)))
    # refusals: -1, nothing enqueued, the output buffers untouched
    bx, bu = np.full((B, T + 1, S, n), -7.0), np.full((B, T, S, m), -7.0)
    bi = np.full(B, -7, dtype=np.int32)
    host = lambda S_=S, flags=1, mu_=0.0, ins=(bx, bx, bu), outs=(bx, bu, bx): g.lib.ilqr_solve_lq(
        g.h, S_, flags, mu_, p(ins[0]), p(ins[1]), p(ins[2]), p(outs[0]), p(outs[1]), p(outs[2]), bi.ctypes.data_as(ip))
    q = lambda a: None if a is None else a.ctypes.data
    dev = lambda S_=S, flags=1, mu_=0.0, ins=(bx, bx, bu), outs=(bx, bu, bx): g.lib.ilqr_solve_lq_on_device(
        g.h, S_, flags, mu_, q(ins[0]), q(ins[1]), q(ins[2]), q(outs[0]), q(outs[1]), q(outs[2]), bi.ctypes.data)
    none3 = (None, None, None)
    for call in (host, dev):
        for S_bad in (0, -3, 2 ** 31 - 1):
            assert call(S_=S_bad) == -1, S_bad
        assert b"INT_MAX" in g.lib.ilqr_last_error() or b"fit an int" in g.lib.ilqr_last_error()
        for flags in (2, 3, -1, 1 << 20):
            assert call(flags=flags) == -1 and b"flag" in g.lib.ilqr_last_error(), flags
        for mu_bad in (-1e-300, -1.0, np.inf, -np.inf, np.nan):
            assert call(mu_=mu_bad) == -1 and b"mu" in g.lib.ilqr_last_error(), mu_bad
        assert call(ins=none3) == -1 and b"all null" in g.lib.ilqr_last_error()
        assert call(outs=none3) == -1 and b"all null" in g.lib.ilqr_last_error()
    assert g.lib.ilqr_solve_lq(None, S, 1, 0.0, p(bx), None, None, p(bx), None, None, None) == -1 and b"null handle" in g.lib.ilqr_last_error()
    assert g.lib.ilqr_solve_lq_on_device(None, S, 1, 0.0, q(bx), None, None, q(bx), None, None, None) == -1
    g.synchronize()
    assert bx.min() == -7.0 == bx.max() and bu.min() == -7.0 == bu.max() and bi.min() == -7 == bi.max()


def test_fresh_handle_is_a_state_error():
    from ilqr_amd import BatchILQR
    for g in (BatchILQR("acrobot", 4, 10, DT), BatchILQR("host", 4, 10, DT, nx=6, nu=2, u_min=-1.0, u_max=1.0)):
        x = np.zeros((4, 11, 1, g.nx))
        assert g.lib.ilqr_solve_lq(g.h, 1, 1, 0.0, None, p(x), None, p(x), None, None, None) == -4
        assert g.lib.ilqr_solve_lq_on_device(g.h, 1, 1, 0.0, None, x.ctypes.data, None, x.ctypes.data, None, None, None) == -4
        g.close()


# ---- 8. the device form ------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_device_form_equals_the_getter(generic_handle, tiled_handle, which):
    import torch
    g = generic_handle if which == "generic" else tiled_handle
    S, B, n, m, T = 17, g.B, g.nx, g.nu, g.T
    mu = 0.3 if which == "generic" else NX4_MU
    dx0, gx, gu = directions(n, m, S, B, T)
    dxs, dus, dlam, info = g.lq_solve(gx=gx, gu=gu, dx0=dx0, mu=mu, dlam=True)
    dev = lambda a: torch.from_numpy(a).cuda()
    fresh = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    d_dx0, d_gx, d_gu = dev(dx0), dev(gx), dev(gu)
    d_dxs, d_dus, d_dlam = fresh(B, T + 1, S, n), fresh(B, T, S, m), fresh(B, T + 1, S, n)
    d_info = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (the copies and fills ran on torch's stream, the call runs on the handle's)
    g.copy_lq_solve_to_device(S, mu, True, d_dx0.data_ptr(), d_gx.data_ptr(), d_gu.data_ptr(), d_dxs.data_ptr(), d_dus.data_ptr(), d_dlam.data_ptr(),
                              d_info.data_ptr())
    g.synchronize()
    for got, want in ((d_dxs, dxs), (d_dus, dus), (d_dlam, dlam), (d_info, info)):
        assert np.array_equal(got.cpu().numpy(), want)
    # dxs alone (kd rests in the handle's scratch): the other buffers are not touched
    for t in (d_dxs, d_dus, d_dlam):
        t.fill_(-7.0)
    torch.cuda.synchronize()
    g.copy_lq_solve_to_device(S, mu, True, d_dx0.data_ptr(), d_gx.data_ptr(), d_gu.data_ptr(), dxs_ptr=d_dxs.data_ptr())
    g.synchronize()
    assert np.array_equal(d_dxs.cpu().numpy(), dxs)
    assert float(d_dus.min()) == -7.0 == float(d_dus.max()) and float(d_dlam.min()) == -7.0 == float(d_dlam.max())


# ---- 9. read-only ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiled", "generic"])
def test_the_handle_is_left_alone(which):
    from ilqr_amd import BatchILQR, capi
    if which == "tiled":
        g, x0, u0, _ = nx4_handle("acrobot", "f64")  # (ilqr_iterate: the persistent route)
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
    dx0, gx, gu = directions(g.nx, g.nu, 5, g.B, g.T)
    out = g.lq_solve(gx=gx, gu=gu, dx0=dx0, mu=NX4_MU, dlam=True)
    assert np.isfinite(out[0][out[3] == 0]).all() and (out[3] == 0).any()
    for h in (g, twin):
        h.iterate(2)
    for a, b in zip(g.trajectory() + g.gains() + (g.cost(),) + g.lambdas(), twin.trajectory() + twin.gains() + (twin.cost(),) + twin.lambdas()):
        assert np.array_equal(a, b)
    g.close()
    twin.close()


# ---- 10. a C++ caller of the facade ------------------------------------------------------------
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
  std::vector<double> dx0((size_t)B * S * 4), gx((size_t)B * (T + 1) * S * 4), gu((size_t)B * T * S * 2);
  for (size_t i = 0; i < dx0.size(); i++) dx0[i] = 0.3 * std::sin(1.0 + 0.7 * (double)i);
  for (size_t i = 0; i < gx.size(); i++) gx[i] = std::cos(0.11 * (double)i);
  for (size_t i = 0; i < gu.size(); i++) gu[i] = std::sin(0.23 * (double)i + 1.0);
  std::vector<double> dxs, dus, dlam;
  std::vector<int> info = b.lq_solve(S, &dx0, &gx, &gu, &dxs, &dus, &dlam, 1.0, true);
  if (dxs.size() != gx.size() || dus.size() != gu.size() || dlam.size() != gx.size() || (int)info.size() != B) return 1;
  FILE* f = std::fopen("lq_solve_out.bin", "wb");
  if (!f) return 1;
  std::fwrite(dx0.data(), sizeof(double), dx0.size(), f);
  std::fwrite(gx.data(), sizeof(double), gx.size(), f);
  std::fwrite(gu.data(), sizeof(double), gu.size(), f);
  std::fwrite(dxs.data(), sizeof(double), dxs.size(), f);
  std::fwrite(dus.data(), sizeof(double), dus.size(), f);
  std::fwrite(dlam.data(), sizeof(double), dlam.size(), f);
  std::fclose(f);
  int bad = 0;
  for (int i = 0; i < B; i++) bad += info[i] != 0;
  double first = 0;
  for (int t = 0; t < B; t++)
    for (int e = 0; e < S * 4; e++) first = std::fmax(first, std::fabs(dxs[(size_t)t * (T + 1) * S * 4 + e] - dx0[(size_t)t * S * 4 + e]));
  std::printf("info nonzero %d first %g\n", bad, first);
  return (bad == 0 && first == 0) ? 0 : 2;
}
'''


def test_facade_caller_gets_the_python_answer(tmp_path):
    """BatchILQR::lq_solve of the C++ facade on a double integrator: the same handle set up from Python gives the same answer."""
    from ilqr_amd import BatchILQR, _build
    _build.build()
    src = tmp_path / "lq_solve_caller.cpp"
    src.write_text(BATCH_CALLER)
    exe = str(tmp_path / "lq_solve_caller")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-DILQR_AMD_NO_EIGEN", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + os.path.join(ROOT, "ilqr_amd", "lib"), "-lilqr_amd", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "ilqr_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    B, T, S = 3, 15, 4
    raw = np.fromfile(str(tmp_path / "lq_solve_out.bin"))
    sizes = [B * S * 4, B * (T + 1) * S * 4, B * T * S * 2, B * (T + 1) * S * 4, B * T * S * 2, B * (T + 1) * S * 4]
    parts = np.split(raw, np.cumsum(sizes)[:-1])
    dx0, gx, gu = parts[0].reshape(B, S, 4), parts[1].reshape(B, T + 1, S, 4), parts[2].reshape(B, T, S, 2)
    g = BatchILQR("double_integrator", B, T, 0.02, goal=np.array([1.0, 0.5, 0.0, 0.0]))
    x0 = (0.1 * (np.arange(B * 4) % 5) - 0.2).reshape(B, 4)
    g.init_traj(x0, np.zeros((B, T, 2)))
    g.iterate(2)
    want = g.lq_solve(gx=gx, gu=gu, dx0=dx0, mu=1.0, hold_clamped=True, dlam=True)
    assert not want[3].any()
    for got, ref, what in zip(parts[3:], want[:3], ("dxs", "dus", "dlam")):
        close(got.reshape(ref.shape), ref, what + " of the C++ caller", bound=1e-12)
    g.close()


# ---- every request through the staging buffer ---------------------------------------------------
from tests import getter_vs_device as gd  # noqa: E402


@pytest.mark.parametrize("case", gd.CASES)
@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_getter_equals_the_device_form_request_by_request(which, case):
    """ilqr_solve_lq against ilqr_solve_lq_on_device, bit for bit: every pointer; gu in, dlam and info out (a call without inputs is
    refused, and so is info alone); that, every pointer, that again on one handle."""

    def args(g):
        rng, per_x, per_u = np.random.default_rng(3), gd.B * gd.ND * g.nx, gd.B * gd.ND * g.nu
        return [gd.Arg("dx0", "in", rng.normal(size=per_x)), gd.Arg("gx", "in", rng.normal(size=per_x * (gd.T + 1))), gd.Arg("gu", "in", rng.normal(size=per_u * gd.T)),
                gd.Arg("dxs", "out", (per_x * (gd.T + 1),)), gd.Arg("dus", "out", (per_u * gd.T,)), gd.Arg("dlam", "out", (per_x * (gd.T + 1),)),
                gd.Arg("info", "info", (gd.B,))]
    gd.check(lambda: gd.handle(which), case, "ilqr_solve_lq", "ilqr_solve_lq_on_device", (gd.ND, 0, 0.0), args, needs_input=True)
