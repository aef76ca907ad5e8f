"""ilqr_get_risk_sensitive / ilqr_copy_risk_sensitive_to_device on the device (k_risk_w on the generic layout, k_risk_t on the tiled one):
against a numpy restatement of the header's definition, the bit rules, mu, cross-checks against ilqr_get_value, ilqr_get_covariance and
ilqr_solve_lq at theta = 0, both failure signs, NULLs and refusals, the device form, and that asking changes nothing a later iteration
computes.

Yardstick: risk_reference(records, stored K, C, theta, mu, hold), float64, a hand-written Cholesky and substitution so that it also runs in
np.longdouble.  Between it and the device the bound is the project's 1e-9 x max(1, max|.|) for two summation orders of one recursion; the
noise scale of every case is chosen by choose_noise so that float64 and np.longdouble agree within 1e-10 x the same scale -- a factor 10
of headroom -- and no pivot is near zero.  tests/test_risk_abi.py checks the yardstick itself against things written independently of it.
The refusal of B * (T + 1) * nx * nx beyond INT_MAX is not exercised here: a handle of that size does not fit a test."""
import ctypes as C_
import functools

import numpy as np
import pytest

from tests.test_gpu_lq_solve import NX4_MU, close, convex_policy, held_rows, scale_of, tiled_policy_handle
from tests.test_gpu_value import GENERIC_SIZES, host_handle, nx4_handle

pytestmark = pytest.mark.gpu
DT = 0.02
dp = C_.POINTER(C_.c_double)
ip = C_.POINTER(C_.c_int)
OUTPUTS = ("K", "k", "Vx", "Vxx", "risk_cost")
NOISE_SCALES = tuple(0.1 / 2 ** i for i in range(10))  # 0.1, 0.05, 0.025, 0.0125 and on down (the acrobot's terminal cost is stiff)
PIVOT_FLOOR_M, PIVOT_FLOOR_QUU = 0.2, 0.05
THETAS = (0.5, -0.5, 0.0)
GENERIC_CASES = [(n, m, nw) for n, m in GENERIC_SIZES for nw in sorted({1, min(n, 17), n})] + [(32, 16, 5), (32, 16, 16), (20, 5, 5), (20, 5, 16)]


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """The device-form case uses torch tensors: torch's device is initialised before this module creates any handle."""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


# ---- the yardstick -----------------------------------------------------------------------------
def chol_lower(A):
    """Lower Cholesky in index order, any dtype: (L, pivots met, failed?).  A pivot <= 0 or not finite ends it (that pivot is the last)."""
    m = A.shape[0]
    L = np.zeros_like(A)
    pivots = []
    for j in range(m):
        piv = A[j, j] - L[j, :j] @ L[j, :j]
        pivots.append(piv)
        if not (piv > 0) or not np.isfinite(piv):
            return None, pivots, True
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L, pivots, False


def forward_subst(L, R):
    """L^-1 R, any dtype."""
    Y = np.array(R, dtype=L.dtype)
    for i in range(L.shape[0]):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def backward_subst(L, R):
    """L'^-1 R, any dtype."""
    Y = np.array(R, dtype=L.dtype)
    for i in range(L.shape[0] - 1, -1, -1):
        Y[i] = (Y[i] - L[i + 1:, i] @ Y[i + 1:]) / L[i, i]
    return Y


def risk_reference(d, K_stored, C, theta, mu=0.0, hold=False, dtype=np.float64):
    """The definition of include/ilqr_amd.h (ilqr_get_risk_sensitive).  d: the records as BatchILQR.derivatives() returns them (matrices
    [B][T+1][rows][cols]); K_stored [B][T][m][n] (read for the held set alone); C [B][n][nw].  Returns a dict: K [B][T][m][n], k [B][T][m],
    Vx [B][T+1][n], Vxx [B][T+1][n][n], risk_cost [B], info int32 [B]; and, for the tests' preconditions, pivots_M and pivots_Quu: per
    trajectory the pivots met, in the order met (a failing pivot is the last)."""
    fx, fu, cx, cu, cxx, cxu, cuu = (np.asarray(d[name], dtype=dtype) for name in ("fx", "fu", "cx", "cu", "cxx", "cxu", "cuu"))
    C = np.asarray(C, dtype=dtype)
    B, T, m, n = np.asarray(K_stored).shape
    nw = C.shape[-1]
    held = held_rows(K_stored, hold)
    theta, mu, half = dtype(theta), dtype(mu), dtype(0.5)
    out = dict(K=np.zeros((B, T, m, n), dtype=dtype), k=np.zeros((B, T, m), dtype=dtype), Vx=np.zeros((B, T + 1, n), dtype=dtype),
               Vxx=np.zeros((B, T + 1, n, n), dtype=dtype), risk_cost=np.zeros(B, dtype=dtype), info=np.zeros(B, dtype=np.int32),
               pivots_M=[[] for _ in range(B)], pivots_Quu=[[] for _ in range(B)])
    for b in range(B):
        P, v, s = cxx[b, T], cx[b, T], dtype(0)
        out["Vxx"][b, T], out["Vx"][b, T] = P, v
        for t in range(T - 1, -1, -1):
            G = P @ C[b]
            CtG = C[b].T @ G
            M = np.eye(nw, dtype=dtype) - theta * (half * (CtG + CtG.T))
            R, pivots, bad = chol_lower(M)
            out["pivots_M"][b] += pivots
            if bad:
                out["info"][b] = -(t + 1)
                break
            Y = forward_subst(R, G.T)
            y = forward_subst(R, C[b].T @ v)
            Pt = P + theta * (Y.T @ Y)
            vt = v + theta * (Y.T @ y)
            if theta != 0:
                st = s + theta / 2 * (y @ y) - np.log(np.diag(R)).sum() / theta
            else:
                st = s + half * np.trace(CtG)
            A, Bm = fx[b, t], fu[b, t]
            Qx, Qu = cx[b, t] + A.T @ vt, cu[b, t] + Bm.T @ vt
            Qxx = cxx[b, t] + A.T @ Pt @ A
            Qux = cxu[b, t].T + Bm.T @ Pt @ A
            Quu = cuu[b, t] + Bm.T @ Pt @ Bm + mu * np.eye(m, dtype=dtype)
            F = np.flatnonzero(~held[b, t])
            Kt, kt = np.zeros((m, n), dtype=dtype), np.zeros(m, dtype=dtype)
            if len(F):
                L, pivots, bad = chol_lower(Quu[np.ix_(F, F)])
                out["pivots_Quu"][b] += pivots
                if bad:
                    out["info"][b] = t + 1
                    break
                Kt[F] = -backward_subst(L, forward_subst(L, Qux[F]))
                kt[F] = -backward_subst(L, forward_subst(L, Qu[F]))
            Pn = Qxx + Qux.T @ Kt
            P, v, s = half * (Pn + Pn.T), Qx + Kt.T @ Qu, st + half * (Qu @ kt)
            out["K"][b, t], out["k"][b, t], out["Vxx"][b, t], out["Vx"][b, t] = Kt, kt, P, v
        out["risk_cost"][b] = s
        if out["info"][b]:
            for name in OUTPUTS:
                out[name][b] = np.nan
    return out


def noise(n, nw, B, scale=1.0):
    """C [B][n][nw] = scale N(0, 1) / sqrt(n), seeded per size."""
    return scale * np.random.default_rng(8800 + 100 * n + nw).normal(size=(B, n, nw)) / np.sqrt(n)


def qualifies(d, K, C, theta, mu, hold):
    """The float64 yardstick at this C if it has its headroom, else None: float64 and np.longdouble within 1e-10 x max(1, max|.|) on every
    output, no pivot of M below 0.2, none of Quu_FF below 0.05 (and so no failure)."""
    ref = risk_reference(d, K, C, theta, mu, hold)
    low_M = min(min(p) for p in ref["pivots_M"])
    low_Quu = min([min(p) for p in ref["pivots_Quu"] if len(p)], default=np.inf)
    print("  scale of C %.3g: info %s, least pivot of M %.3g, of Quu_FF %.3g" % (float(np.abs(C).max()), ref["info"].tolist(), low_M, low_Quu))
    if ref["info"].any() or low_M < PIVOT_FLOOR_M or low_Quu < PIVOT_FLOOR_QUU:
        return None
    lng = risk_reference(d, K, C, theta, mu, hold, dtype=np.longdouble)
    if lng["info"].any():
        return None
    for name in OUTPUTS:
        gap = float(np.abs(ref[name] - lng[name]).max())
        print("  float64 vs longdouble %s: %.3g (scale %.3g)" % (name, gap, scale_of(ref[name])))
        if gap > 1e-10 * scale_of(ref[name]):
            return None
    return ref


def choose_noise(d, K, n, nw, theta, mu, hold):
    """(s, C, yardstick): the first noise scale s of NOISE_SCALES at which the yardstick has its headroom (qualifies).  theta = 0 takes the
    scale of theta = 0.5."""
    B = np.asarray(K).shape[0]
    for s in NOISE_SCALES:
        C = noise(n, nw, B, s)
        ref = qualifies(d, K, C, theta if theta != 0 else 0.5, mu, hold)
        if ref is not None:
            return s, C, (ref if theta != 0 else risk_reference(d, K, C, 0.0, mu, hold))
    raise AssertionError("no noise scale of %s qualifies for n = %d, nw = %d, theta = %g, hold = %s" % (NOISE_SCALES, n, nw, theta, hold))


@functools.lru_cache(maxsize=None)
def generic_case(n, m, nw, theta, mu=0.0, hold=False):
    """(s, C, yardstick) on convex_policy(n, m).  Computed once per case, shared, never written to."""
    d, _, K = convex_policy(n, m)
    return choose_noise(d, K, n, nw, theta, mu, hold)


def ask(g, C, theta, mu=0.0, hold=False):
    return g.risk_sensitive(C, theta, mu=mu, hold_clamped=hold, K=True, k=True, Vx=True, Vxx=True, risk_cost=True, info=True)


def check_call(g, d, K_stored, C, ref, theta, mu, hold, what=""):
    """One call on the handle against the yardstick, and the bit rules; returns the device's outputs."""
    B, T, m, n = np.asarray(K_stored).shape
    got = ask(g, C, theta, mu, hold)
    assert got["info"].dtype == np.int32 and not got["info"].any() and not ref["info"].any(), (got["info"], ref["info"])
    assert got["K"].shape == (B, T, m, n) and got["Vxx"].shape == (B, T + 1, n, n)
    for name in OUTPUTS:
        close(got[name], ref[name], "%s %s theta %g hold %s" % (name, what, theta, hold))
    assert np.array_equal(got["Vxx"][:, :T], np.swapaxes(got["Vxx"][:, :T], -1, -2))  # symmetric to the bit
    assert np.array_equal(got["Vxx"][:, T], np.asarray(d["cxx"])[:, T]) and np.array_equal(got["Vx"][:, T], np.asarray(d["cx"])[:, T])
    held = held_rows(K_stored, hold)
    assert np.array_equal(got["K"][held], np.zeros((int(held.sum()), n))) and np.array_equal(got["k"][held], np.zeros(int(held.sum())))
    return got


# ---- 1. generic layout -------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,nw", GENERIC_CASES)
def test_generic_layout(n, m, nw):
    d, k, K = convex_policy(n, m)
    g = host_handle(n, m, d, k, K)
    for hold in (False, True):
        for theta in THETAS:
            s, C, ref = generic_case(n, m, nw, theta, 0.0, hold)
            check_call(g, d, K, C, ref, theta, 0.0, hold, "s %g" % s)
    g.close()


# ---- 2. mu -------------------------------------------------------------------------------------
def test_mu():
    n, m, nw, mu = 20, 5, 5, 0.3
    d, k, K = convex_policy(n, m)
    g = host_handle(n, m, d, k, K)
    for hold in (False, True):
        s, C, ref = generic_case(n, m, nw, 0.5, mu, hold)
        got = check_call(g, d, K, C, ref, 0.5, mu, hold, "mu %g" % mu)
        assert np.abs(got["K"] - generic_case(n, m, nw, 0.5, 0.0, hold)[2]["K"]).max() > 1e-4  # (mu is not ignored)
    g.close()


# ---- 3. against the existing kernels at theta = 0 ----------------------------------------------
@pytest.mark.parametrize("n,m,nw", [(20, 5, 5), (24, 20, 17)])
def test_against_value_covariance_and_lq_solve(n, m, nw):
    d, k, K = convex_policy(n, m)
    B, T = k.shape[:2]
    C = noise(n, nw, B, 0.1)
    W = C @ np.swapaxes(C, -1, -2)
    g = host_handle(n, m, d, k, K)
    got = ask(g, C, 0.0)
    assert not got["info"].any()
    # ilqr_solve_lq(dx0 = I): dlam[0] = P[0] dx0 (directions are rows: P[0]' = P[0])
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(n), (B, n, n)))
    dlam, info = g.lq_solve(dx0=eye, mu=0.0, hold_clamped=False, dlam=True)[2:]
    assert not info.any()
    close(dlam[:, 0], got["Vxx"][:, 0], "solve_lq(dx0 = I).dlam[0] vs Vxx[0]")
    # the value of the optimal policy is the Riccati solution
    g.set_gains(k=got["k"], K=got["K"])
    Vx, Vxx = g.value()
    close(Vx, got["Vx"], "ilqr_get_value's Vx of the installed gains")
    close(Vxx, got["Vxx"], "ilqr_get_value's Vxx of the installed gains")
    g.close()
    # records without linear terms: risk_cost is the expected noise cost of the installed gains
    flat = dict(d, cx=np.zeros_like(d["cx"]), cu=np.zeros_like(d["cu"]))
    g = host_handle(n, m, flat, k, K)
    got = ask(g, C, 0.0)
    assert not got["info"].any() and np.abs(got["k"]).max() == 0.0
    g.set_gains(k=got["k"], K=got["K"])
    J = g.covariance(W=W, expected_cost=True)[1]
    close(got["risk_cost"], J, "risk_cost vs ilqr_get_covariance's expected cost")
    assert np.abs(J).min() > 1e-3
    g.close()


# ---- 4. nx = 4 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model", ["acrobot", "double_integrator"])
def test_nx4(model, dtype):
    """B = 20 is no multiple of the 16-trajectory tile; the recursion is double in both dtypes, so one bound.  mu = NX4_MU keeps the
    acrobot's finite-difference cuu from deciding the outcome; the noise scale is chosen on the handle's own records."""
    g = tiled_policy_handle(model, dtype)
    d, K = g.derivatives(), g.gains()[1]
    for nw in (1, 2, 4):
        for hold in (False, True):
            for theta in THETAS:
                s, C, ref = choose_noise(d, K, 4, nw, theta, NX4_MU, hold)
                check_call(g, d, K, C, ref, theta, NX4_MU, hold, "nw %d s %g" % (nw, s))
    g.close()


# ---- 5. fp32 generic ---------------------------------------------------------------------------
def test_fp32_generic():
    """Float records and gains are widened, the recursion is double: the definition on the handle's float-valued records."""
    from ilqr_amd import BatchILQR
    from tests.test_gpu_lq_end_to_end import lq_mats
    n, m, B, T = 20, 5, 6, 12
    g = BatchILQR("lq", B, T, DT, lq=lq_mats(n, m), u_min=-0.5, u_max=0.5, dtype="f32")
    rng = np.random.default_rng(5)
    g.init_traj(rng.uniform(-1, 1, (B, n)), rng.normal(size=(B, T, m)) * 0.3)
    g.iterate(2)
    d, K = g.derivatives(), g.gains()[1]
    for nw, hold in ((5, True), (17, False)):
        for theta in THETAS:
            s, C, ref = choose_noise(d, K, n, nw, theta, 0.0, hold)
            check_call(g, d, K, C, ref, theta, 0.0, hold, "nw %d s %g" % (nw, s))
    g.close()


# ---- 6. failures -------------------------------------------------------------------------------
def one(d, K, C, b):
    """Trajectory b alone, as the yardstick takes it."""
    return {name: np.asarray(a)[b:b + 1] for name, a in d.items()}, np.asarray(K)[b:b + 1], C[b:b + 1]


def breakdown_inputs(d, K, C, theta, mu):
    """C with trajectory 1 scaled until the yardstick breaks down at the first step (info = -T) and trajectory 3 scaled, by a search, until
    it breaks down at a knot <= T - 3 with every earlier pivot above 1e-6 and the failing one below -1e-6."""
    T = np.asarray(K).shape[1]
    bad = np.array(C)
    f = 1.0
    while risk_reference(*one(d, K, f * C, 1), theta, mu)["info"][0] != -T:
        f *= 2.0
        assert f < 1e6
    bad[1] = f * C[1]
    f = 1.0
    for _ in range(400):
        f *= 1.03
        r = risk_reference(*one(d, K, f * C, 3), theta, mu)
        piv = r["pivots_M"][0]
        if r["info"][0] < 0 and -r["info"][0] - 1 <= T - 3 and piv[-1] < -1e-6 and min(piv[:-1]) > 1e-6:
            bad[3] = f * C[3]
            return bad
    raise AssertionError("no scale of C[3] breaks down at a knot <= T - 3 with clear pivots")


@pytest.mark.parametrize("n,m,nw", [(20, 5, 5), (32, 32, 17), (4, 1, 2), (4, 2, 4)])
def test_failures(n, m, nw):
    theta, mu, T = 0.5, 0.0, 12
    d, k, K = convex_policy(n, m)
    K = np.where(np.abs(K).sum(axis=-1, keepdims=True) == 0, 0.25, K)  # every control free
    C = noise(n, nw, 5, 0.05)
    bad_d = {name: np.array(a) for name, a in d.items()}
    bad_d["cuu"][2, 7] = -1e3 * np.eye(m)
    bad_C = breakdown_inputs(d, K, C, theta, mu)
    want = risk_reference(bad_d, K, bad_C, theta, mu)
    assert want["info"][1] == -T and want["info"][2] == 8 and -(T - 2) <= want["info"][3] < 0 and not want["info"][[0, 4]].any(), want["info"]
    piv = want["pivots_M"][3]
    assert piv[-1] < -1e-6 and min(piv[:-1]) > 1e-6  # (the test's own precondition)
    if n == 4:
        from ilqr_amd import BatchILQR
        g = BatchILQR("double_integrator" if m == 2 else "acrobot", 5, T, DT, u_min=-1.0, u_max=1.0)
        assert g.nu == m
        g.init_traj(np.zeros((5, 4)), np.zeros((5, T, m)))
        g.set_derivatives(**d)
        g.set_gains(k=k, K=K)
    else:
        g = host_handle(n, m, d, k, K)
    sound = ask(g, C, theta, mu)
    assert not sound["info"].any()
    g.set_derivatives(**bad_d)
    got = ask(g, bad_C, theta, mu)
    assert np.array_equal(got["info"], want["info"]), (got["info"], want["info"])
    for name in OUTPUTS:
        assert np.isnan(got[name][[1, 2, 3]]).all() and np.array_equal(got[name][[0, 4]], sound[name][[0, 4]]), name
    g.close()


# ---- 7. NULLs and refusals ---------------------------------------------------------------------
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


def handle_case(g, which):
    """(nw, theta, mu, C canonical [B][n*nw], C) for the two module handles, with ILQR_LQ_HOLD_CLAMPED: the noise scale by choose_noise."""
    nw, theta, mu = (5, 0.5, 0.0) if which == "generic" else (2, 0.5, NX4_MU)
    C = choose_noise(g.derivatives(), g.gains()[1], g.nx, nw, theta, mu, True)[1]
    return nw, theta, mu, np.ascontiguousarray(np.swapaxes(C, -1, -2)), C


def buffers(g, fill=-7.0):
    B, T, n, m = g.B, g.T, g.nx, g.nu
    return [np.full(shape, fill) for shape in ((B, T, n, m), (B, T, m), (B, T + 1, n), (B, T + 1, n, n), (B,))]


@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_nulls_and_refusals(generic_handle, tiled_handle, which):
    g = generic_handle if which == "generic" else tiled_handle
    lib, B, n = g.lib, g.B, g.nx
    nw, theta, mu, Cc, C = handle_case(g, which)
    full = buffers(g)
    info = np.full(B, -7, dtype=np.int32)
    assert lib.ilqr_get_risk_sensitive(g.h, nw, theta, 1, mu, p(Cc), *[p(a) for a in full], info.ctypes.data_as(ip)) == 0
    assert not info.any() and all(np.isfinite(a).all() for a in full)
    api = ask(g, C, theta, mu, True)
    assert np.array_equal(np.swapaxes(full[0], -1, -2), api["K"]) and np.array_equal(full[4], api["risk_cost"])
    # one output at a time (info NULL): the bits of the full call
    for keep in range(5):
        outs = [np.full_like(a, -7.0) if i == keep else None for i, a in enumerate(full)]
        assert lib.ilqr_get_risk_sensitive(g.h, nw, theta, 1, mu, p(Cc), *[p(a) for a in outs], None) == 0
        assert np.array_equal(outs[keep], full[keep]), OUTPUTS[keep]
    # refusals: -1 with the word for it, nothing enqueued, the output buffers untouched
    bufs = buffers(g)
    bi = np.full(B, -7, dtype=np.int32)
    q = lambda a: None if a is None else a.ctypes.data
    host = lambda nw_=nw, theta_=theta, flags=1, mu_=mu, C__=Cc, outs=bufs: lib.ilqr_get_risk_sensitive(
        g.h, nw_, theta_, flags, mu_, p(C__), *[p(a) for a in outs], bi.ctypes.data_as(ip))
    dev = lambda nw_=nw, theta_=theta, flags=1, mu_=mu, C__=Cc, outs=bufs: lib.ilqr_copy_risk_sensitive_to_device(
        g.h, nw_, theta_, flags, mu_, q(C__), *[q(a) for a in outs], bi.ctypes.data)
    for call in (host, dev):
        for nw_bad in (0, -1, n + 1, 2 ** 31 - 1):
            assert call(nw_=nw_bad) == -1 and b"nw" in lib.ilqr_last_error(), nw_bad
        assert call(C__=None) == -1 and b"C is required" in lib.ilqr_last_error()
        for flags in (2, 3, -1, 1 << 20):
            assert call(flags=flags) == -1 and b"flag" in lib.ilqr_last_error(), flags
        for mu_bad in (-1e-300, -1.0, np.inf, -np.inf, np.nan):
            assert call(mu_=mu_bad) == -1 and b"mu" in lib.ilqr_last_error(), mu_bad
        for theta_bad in (np.inf, -np.inf, np.nan):
            assert call(theta_=theta_bad) == -1 and b"theta" in lib.ilqr_last_error(), theta_bad
        assert call(outs=[None] * 5) == -1 and b"all null" in lib.ilqr_last_error()
    assert lib.ilqr_get_risk_sensitive(None, nw, theta, 1, mu, p(Cc), *[p(a) for a in bufs], None) == -1 and b"null handle" in lib.ilqr_last_error()
    assert lib.ilqr_copy_risk_sensitive_to_device(None, nw, theta, 1, mu, q(Cc), *[q(a) for a in bufs], None) == -1
    assert b"null handle" in lib.ilqr_last_error()
    g.synchronize()
    assert all(a.min() == -7.0 == a.max() for a in bufs) and bi.min() == -7 == bi.max()
    # the handle answers as before
    again = buffers(g)
    assert lib.ilqr_get_risk_sensitive(g.h, nw, theta, 1, mu, p(Cc), *[p(a) for a in again], None) == 0
    assert all(np.array_equal(a, b) for a, b in zip(again, full))


def test_fresh_handle_is_a_state_error():
    from ilqr_amd import BatchILQR
    for g in (BatchILQR("acrobot", 4, 10, DT), BatchILQR("host", 4, 10, DT, nx=6, nu=2, u_min=-1.0, u_max=1.0)):
        Cc, K = np.zeros((4, g.nx)), np.zeros((4, 10, g.nx, g.nu))
        assert g.lib.ilqr_get_risk_sensitive(g.h, 1, 0.5, 0, 0.0, p(Cc), p(K), None, None, None, None, None) == -4
        assert g.lib.ilqr_copy_risk_sensitive_to_device(g.h, 1, 0.5, 0, 0.0, Cc.ctypes.data, K.ctypes.data, None, None, None, None, None) == -4
        g.close()


# ---- 8. the device form ------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_device_form_equals_the_getter(generic_handle, tiled_handle, which):
    import torch
    g = generic_handle if which == "generic" else tiled_handle
    B, T, n, m = g.B, g.T, g.nx, g.nu
    nw, theta, mu, Cc, C = handle_case(g, which)
    full = buffers(g)
    info = np.zeros(B, dtype=np.int32)
    assert g.lib.ilqr_get_risk_sensitive(g.h, nw, theta, 1, mu, p(Cc), *[p(a) for a in full], info.ctypes.data_as(ip)) == 0
    d_C = torch.from_numpy(Cc).cuda()
    d_out = [torch.full(a.shape, -7.0, dtype=torch.float64, device="cuda") for a in full]
    d_info = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (the copies and fills ran on torch's stream, the call runs on the handle's)
    g.copy_risk_sensitive_to_device(nw, theta, d_C.data_ptr(), mu=mu, hold_clamped=True, K_ptr=d_out[0].data_ptr(), k_ptr=d_out[1].data_ptr(),
                                    Vx_ptr=d_out[2].data_ptr(), Vxx_ptr=d_out[3].data_ptr(), risk_cost_ptr=d_out[4].data_ptr(),
                                    info_ptr=d_info.data_ptr())
    g.synchronize()
    for got, want in zip(d_out + [d_info], full + [info]):
        assert np.array_equal(got.cpu().numpy(), want)
    # K and risk_cost alone: the other buffers are not touched
    for t in d_out:
        t.fill_(-7.0)
    torch.cuda.synchronize()
    g.copy_risk_sensitive_to_device(nw, theta, d_C.data_ptr(), mu=mu, hold_clamped=True, K_ptr=d_out[0].data_ptr(), risk_cost_ptr=d_out[4].data_ptr())
    g.synchronize()
    assert np.array_equal(d_out[0].cpu().numpy(), full[0]) and np.array_equal(d_out[4].cpu().numpy(), full[4])
    assert all(float(d_out[i].min()) == -7.0 == float(d_out[i].max()) for i in (1, 2, 3))


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
    C = choose_noise(g.derivatives(), g.gains()[1], g.nx, 2, 0.5, NX4_MU, True)[1]
    out = ask(g, C, 0.5, NX4_MU, True)
    assert not out["info"].any() and np.isfinite(out["K"]).all()
    for h in (g, twin):
        h.iterate(2)
    for a, b in zip(g.trajectory() + g.gains() + (g.cost(),) + g.lambdas(), twin.trajectory() + twin.gains() + (twin.cost(),) + twin.lambdas()):
        assert np.array_equal(a, b)
    g.close()
    twin.close()


# ---- 10. every request through the staging buffer -----------------------------------------------
from tests import getter_vs_device as gd  # noqa: E402


@pytest.mark.parametrize("case", gd.CASES)
@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_getter_equals_the_device_form_request_by_request(which, case):
    """ilqr_get_risk_sensitive against ilqr_copy_risk_sensitive_to_device, bit for bit: every pointer; C in (required), risk_cost and info
    out (info alone is refused); that, every pointer, that again on one handle."""
    nw = 2

    def args(g):
        n, m = g.nx, g.nu
        return [gd.Arg("C", "req", 0.05 * np.random.default_rng(3).normal(size=(gd.B, n, nw))), gd.Arg("K", "out", (gd.B * gd.T * m * n,)),
                gd.Arg("k", "out", (gd.B * gd.T * m,)), gd.Arg("Vx", "out", (gd.B * (gd.T + 1) * n,)), gd.Arg("Vxx", "out", (gd.B * (gd.T + 1) * n * n,)),
                gd.Arg("risk_cost", "out", (gd.B,)), gd.Arg("info", "info", (gd.B,))]
    gd.check(lambda: gd.handle(which), case, "ilqr_get_risk_sensitive", "ilqr_copy_risk_sensitive_to_device", (nw, 0.1, 0, 1.0), args)
