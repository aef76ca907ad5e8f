"""The Kalman filter of the stored linearisation and the covariance of the output-feedback loop on the device (ilqr_get_estimator /
ilqr_copy_estimator_to_device; k_est_filter_w and k_est_loop_w on the generic layout, k_estimator_t on the tiled one): against a numpy
restatement of the header's definition, against the covariance kernel (no feedback: the open-loop covariance whatever the filter does),
windows and NULLs, failed factorisations, the device copy, and that asking for it changes nothing a later iteration computes.

Yardstick: estimator_reference(records, K, H, P0, W, V), float64, with a hand-written Cholesky and substitution so that it also runs in
np.longdouble.  Between it and the device (two summation orders of one recursion) the bound is the project's 1e-9 x max(1, max|.|); every
input is first put through the same recursion in np.longdouble, which has to agree with float64 within 1e-10 x the same scale -- a factor
10 of headroom -- and its smallest Cholesky pivot has to stay above 0.05 before the bound is relied on (reference_with_headroom)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.test_gpu_value import GENERIC_SIZES, NAMES, host_handle, nx4_handle, random_policy

pytestmark = pytest.mark.gpu
DT = 0.02
dp = C.POINTER(C.c_double)
OUTPUTS = ("Pp", "Pf", "L", "Sigma", "Su", "expected_cost")
PIVOT_FLOOR = 0.05


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """The device-copy case uses torch tensors: torch's device is initialised before this module creates any handle (a torch initialised
    after the library had set up the device reports no GPU: tests/test_gpu_mpc.py)."""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


def tr(M):
    return np.swapaxes(M, -1, -2)


def sym(M):
    return (M + tr(M)) / 2


def cholesky_lower(S):
    """S [B][q][q] = R R', R lower, in index order, in S's dtype.  Returns (R, pivots [B][q]); a pivot <= 0 or not finite poisons its
    trajectory with NaN (the caller reads the pivots)."""
    B, q, _ = S.shape
    R = np.zeros_like(S)
    piv = np.zeros(S.shape[:2], dtype=S.dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(q):
            s = S[:, j, j] - (R[:, j, :j] * R[:, j, :j]).sum(axis=-1)
            piv[:, j] = s
            s = np.where(s > 0, s, np.nan)
            R[:, j, j] = np.sqrt(s)
            for i in range(j + 1, q):
                R[:, i, j] = (S[:, i, j] - (R[:, i, :j] * R[:, j, :j]).sum(axis=-1)) / R[:, j, j]
    return R, piv


def solve_with_factor(R, X):
    """(R R')^-1 X by forward and back substitution; R [B][q][q] lower, X [B][q][c]."""
    q = R.shape[1]
    Yv = np.zeros_like(X)
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(q):
            Yv[:, r] = (X[:, r] - (R[:, r, :r, None] * Yv[:, :r]).sum(axis=1)) / R[:, r, r, None]
        Z = np.zeros_like(X)
        for r in range(q - 1, -1, -1):
            Z[:, r] = (Yv[:, r] - (R[:, r + 1:, r, None] * Z[:, r + 1:]).sum(axis=1)) / R[:, r, r, None]
    return Z


def estimator_reference(d, K, H, P0, W, V, dtype=np.float64):
    """The definition of include/ilqr_amd.h (ilqr_get_estimator).  d: the records as BatchILQR.derivatives() returns them (matrices
    [B][T+1][rows][cols]); K [B][T][m][n]; H [B][ny][n]; V [B][ny][ny]; P0, W [B][n][n] or None (zero).  Returns a dict: Pp, Pf, Sigma
    [B][T+1][n][n], L [B][T+1][n][ny], Su [B][T][m][m], expected_cost [B], info int [B] (0, or the knot of the first pivot <= 0 or not
    finite + 1: that trajectory's outputs are NaN) and pivots [B][T+1][ny] (NaN after a failure)."""
    fx, fu, cx, cu, cxx, cxu, cuu = (np.asarray(d[name], dtype=dtype) for name in NAMES)
    K, H, V = (np.asarray(a, dtype=dtype) for a in (K, H, V))
    B, T1, n = cx.shape
    T, m, ny = T1 - 1, K.shape[2], H.shape[1]
    dot = lambda X, Y: (X * Y).sum(axis=(-1, -2))
    zeros = lambda *shape: np.zeros(shape, dtype=dtype)
    Pp, Pf, Sigma, L, Su, J = zeros(B, T1, n, n), zeros(B, T1, n, n), zeros(B, T1, n, n), zeros(B, T1, n, ny), zeros(B, T, m, m), zeros(B)
    pivots = np.full((B, T1, ny), np.nan, dtype=dtype)
    info = np.zeros(B, dtype=np.int32)
    Wm = zeros(B, n, n) if W is None else np.asarray(W, dtype=dtype)
    P = zeros(B, n, n) if P0 is None else np.array(P0, dtype=dtype)
    eye = np.eye(n, dtype=dtype)
    Xh = A = None
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T1):
            Pp[:, t] = P
            S = sym(H @ P @ tr(H) + V)
            R, piv = cholesky_lower(S)
            bad = ~(np.isfinite(piv) & (piv > 0)).all(axis=-1)
            pivots[info == 0, t] = piv[info == 0]
            info = np.where((info == 0) & bad, t + 1, info).astype(np.int32)
            Lk = tr(solve_with_factor(R, tr(P @ tr(H))))  # L = Pp H' S^-1, as L' = S^-1 (Pp H')'
            L[:, t] = Lk
            G = eye - Lk @ H
            Pf[:, t] = sym(G @ P @ tr(G) + Lk @ V @ tr(Lk))
            N = sym(Lk @ S @ tr(Lk))
            Xh = sym(N) if t == 0 else sym(A @ Xh @ tr(A) + N)
            Sigma[:, t] = Xh + Pf[:, t]
            J += dot(cxx[:, t], Sigma[:, t]) / 2
            if t < T:
                Kt = K[:, t]
                Z = Xh @ tr(Kt)
                Su[:, t] = sym(Kt @ Z)
                J += (dot(cuu[:, t], Su[:, t]) + 2 * dot(cxu[:, t], Z)) / 2
                A = fx[:, t] + fu[:, t] @ Kt
                P = sym(fx[:, t] @ Pf[:, t] @ tr(fx[:, t]) + Wm)
    out = dict(Pp=Pp, Pf=Pf, L=L, Sigma=Sigma, Su=Su, expected_cost=J)
    for a in out.values():
        a[info != 0] = np.nan
    out.update(info=info, pivots=pivots)
    return out


def estimator_inputs(n, ny, B=5, seed=0):
    """H ~ N(0, 1/n) [B][ny][n]; P0 = a a', a ~ N(0, 1/n); W = a a', a ~ 0.1 N(0, 1/n); V = 0.1 (a a' + I), a ~ N(0, 1/ny)."""
    rng = np.random.default_rng(9000 + 100 * n + ny + seed)
    H = rng.normal(size=(B, ny, n)) / np.sqrt(n)
    a0 = rng.normal(size=(B, n, n)) / np.sqrt(n)
    aw = 0.1 * rng.normal(size=(B, n, n)) / np.sqrt(n)
    av = rng.normal(size=(B, ny, ny)) / np.sqrt(ny)
    return H, a0 @ tr(a0), aw @ tr(aw), 0.1 * (av @ tr(av) + np.eye(ny))


def scale_of(a):
    return max(1.0, float(np.nanmax(np.abs(a))))


def reference_with_headroom(d, K, H, P0, W, V):
    """estimator_reference in float64, after the float64 and np.longdouble recursions have agreed within 1e-10 x max(1, max|.|) and no
    Cholesky pivot has come below PIVOT_FLOOR."""
    ref = estimator_reference(d, K, H, P0, W, V)
    lng = estimator_reference(d, K, H, P0, W, V, dtype=np.longdouble)
    assert not ref["info"].any() and not lng["info"].any()
    floor = float(ref["pivots"].min())
    print("  smallest Cholesky pivot of the reference: %.3g" % floor)
    assert floor > PIVOT_FLOOR, floor
    for what in OUTPUTS:
        gap = float(np.abs(ref[what] - lng[what]).max())
        print("  float64 vs longdouble %s: %.3g (scale %.3g)" % (what, gap, scale_of(ref[what])))
        assert gap <= 1e-10 * scale_of(ref[what]), (what, gap, scale_of(ref[what]))
    return ref


def against_reference(got, ref, bound=1e-9):
    """got: a dict of full-horizon outputs; every member it has is held to the reference."""
    for what in OUTPUTS:
        if what not in got:
            continue
        a, b = got[what], ref[what]
        assert a.shape == b.shape, (what, a.shape, b.shape)
        err = float(np.abs(a - b).max())
        print("  device vs reference %s: %.3g (scale %.3g)" % (what, err, scale_of(b)))
        assert err <= bound * scale_of(b), (what, err, scale_of(b))


def everything(g, H, P0, W, V):
    """Every output over every knot it has: two calls, since a window with Su ends before knot T."""
    out = g.estimator(H, P0, W, V, Pp=True, Sigma=True, info=True)
    more = g.estimator(H, P0, W, V, Pf=False, L=False, Sigma=True, Su=True, expected_cost=True, info=True)
    assert out["Sigma"].shape[1] == g.T + 1 and more["Su"].shape[1] == g.T
    assert np.array_equal(more["Sigma"], out["Sigma"][:, :-1], equal_nan=True) and np.array_equal(more["info"], out["info"])
    out.update(Su=more["Su"], expected_cost=more["expected_cost"])
    return out


def check_the_bit_rules(got, P0):
    assert np.array_equal(got["Pp"][:, 0], P0)  # as given, to the bit
    for what, a in (("Pp", got["Pp"][:, 1:]), ("Pf", got["Pf"]), ("Sigma", got["Sigma"]), ("Su", got["Su"])):
        assert np.array_equal(a, tr(a)), what  # symmetric to the bit


@functools.lru_cache(maxsize=None)
def generic_case(n, m, ny, seed=0):
    """(d, k, K, H, P0, W, V, reference): computed once per size, shared, never written to."""
    d, k, K = random_policy(n, m, seed=seed)
    H, P0, W, V = estimator_inputs(n, ny, seed=seed)
    return d, k, K, H, P0, W, V, reference_with_headroom(d, K, H, P0, W, V)


def generic_cases():
    cases = []
    for n, m in GENERIC_SIZES:
        nys = {1, min(n, 17), n}
        if (n, m) in ((32, 16), (20, 5)):
            nys |= {5, 16}
        cases += [(n, m, ny) for ny in sorted(nys)]
    return cases


# ---- 1. generic layout (9: ILQR_MODEL_HOST with nu = 32 is the (32, 32) size) -------------------
@pytest.mark.parametrize("n,m,ny", generic_cases())
def test_generic_layout(n, m, ny):
    """One and two tiles of each of n, m and ny, ragged edges."""
    d, k, K, H, P0, W, V, ref = generic_case(n, m, ny)
    g = host_handle(n, m, d, k, K)
    got = everything(g, H, P0, W, V)
    assert got["L"].shape == (5, 13, n, ny) and got["Su"].shape == (5, 12, m, m) and got["expected_cost"].shape == (5,)
    assert not got["info"].any()
    against_reference(got, ref)
    check_the_bit_rules(got, P0)
    g.close()


def test_host_model_with_32_controls_is_covered():
    assert (32, 32, 32) in generic_cases() and (32, 32, 1) in generic_cases()


# ---- 2. P0 is taken as given -------------------------------------------------------------------
def test_p0_is_taken_as_given():
    """Pp[0] is not symmetrised, and the first products use P0, not its transpose."""
    n, m, ny = 20, 5, 5
    d, k, K, H, P0, W, V, _ = generic_case(n, m, ny)
    P0 = P0 + 0.2 * np.random.default_rng(9).normal(size=P0.shape) / np.sqrt(n)
    assert np.abs(P0 - tr(P0)).max() > 1e-2
    g = host_handle(n, m, d, k, K)
    got = everything(g, H, P0, W, V)
    assert np.array_equal(got["Pp"][:, 0], P0)
    ref = reference_with_headroom(d, K, H, P0, W, V)
    against_reference(got, ref)
    assert np.abs(estimator_reference(d, K, H, tr(P0), W, V)["L"] - ref["L"]).max() > 1e-3  # (the transpose would show)
    g.close()


# ---- 3. the filter ignores K -------------------------------------------------------------------
def test_the_filter_ignores_the_gains():
    n, m, ny = 20, 5, 17
    d, k, K, H, P0, W, V, _ = generic_case(n, m, ny)
    K2 = random_policy(n, m, seed=3)[2]
    assert np.abs(K2 - K).max() > 1e-2
    g, g2 = host_handle(n, m, d, k, K), host_handle(n, m, d, k, K2)
    a, b = everything(g, H, P0, W, V), everything(g2, H, P0, W, V)
    for what in ("Pp", "Pf", "L"):
        assert np.array_equal(a[what], b[what]), what
    assert np.abs(a["Sigma"] - b["Sigma"]).max() > 1e-6  # (and the loop does not)
    g.close()
    g2.close()


# ---- 4. against the existing covariance kernel -------------------------------------------------
@pytest.mark.parametrize("n,m", [(20, 5), (32, 32)])
def test_no_feedback_is_the_open_loop_covariance(n, m):
    """With K = 0 the true state's covariance is the open-loop one, whatever the filter does: Sigma[t] against ilqr_get_covariance
    (Sigma0 = P0, W) of the same handle, two independent kernels."""
    d, k, K, H, P0, W, V, _ = generic_case(n, m, min(n, 17))
    g = host_handle(n, m, d, k, np.zeros_like(K))
    Sg = g.estimator(H, P0, W, V, Pf=False, L=False, Sigma=True)["Sigma"]
    want = g.covariance(P0, W)
    err = float(np.abs(Sg - want).max())
    print("  estimator vs covariance kernel Sigma: %.3g (scale %.3g)" % (err, scale_of(want)))
    assert Sg.shape == want.shape and err <= 1e-9 * scale_of(want), (err, scale_of(want))
    g.close()


# ---- 5. windows and NULLs ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def generic_handle():
    d, k, K, H, P0, W, V, _ = generic_case(20, 5, 5, seed=1)
    g = host_handle(20, 5, d, k, K)
    yield g, H, P0, W, V
    g.close()


@pytest.fixture(scope="module")
def tiled_handle():
    g, x0, u0, _ = nx4_handle("double_integrator", "f64")
    g.init_traj(x0, u0)
    g.compute_derivatives()
    g.backward_pass()
    yield (g,) + estimator_inputs(4, 2, B=g.B)
    g.close()


@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_windows_and_nulls(generic_handle, tiled_handle, which):
    g, H, P0, W, V = generic_handle if which == "generic" else tiled_handle
    T, n, m, B, ny = g.T, g.nx, g.nu, g.B, H.shape[1]
    full = everything(g, H, P0, W, V)
    assert np.abs(full["Su"]).max() > 0 and np.abs(full["expected_cost"]).max() > 0 and not full["info"].any()
    for t0, nk in ((0, 1), (T, 1), (3, 4)):
        w = g.estimator(H, P0, W, V, t0=t0, n_knots=nk, Pp=True, Sigma=True)
        for what in ("Pp", "Pf", "L", "Sigma"):
            assert np.array_equal(w[what], full[what][:, t0:t0 + nk]), (what, t0, nk)
    w = g.estimator(H, P0, W, V, t0=3, n_knots=4, Pp=True, Sigma=True, Su=True)
    for what in ("Pp", "Pf", "L", "Sigma", "Su"):
        assert np.array_equal(w[what], full[what][:, 3:7]), what
    # one output at a time, and the expected cost alone
    none = dict(Pf=False, L=False)
    for what in ("Pp", "Pf", "L", "Sigma", "Su"):
        for t0, nk in ((0, T), (2, 5)):
            one = g.estimator(H, P0, W, V, t0=t0, n_knots=nk, **dict(none, **{what: True}))
            assert list(one) == [what] and np.array_equal(one[what], full[what][:, t0:t0 + nk]), (what, t0, nk)
    only_j = g.estimator(H, P0, W, V, t0=0, n_knots=1, expected_cost=True, **none)
    assert list(only_j) == ["expected_cost"] and np.array_equal(only_j["expected_cost"], full["expected_cost"])
    # NULL inputs are zeros
    a, b = g.estimator(H, None, None, V, Pp=True, Sigma=True), g.estimator(H, np.zeros((n, n)), np.zeros((n, n)), V, Pp=True, Sigma=True)
    for what in a:
        assert np.array_equal(a[what], b[what]), what
    # refusals, each before anything is enqueued
    p = lambda x: None if x is None else x.ctypes.data_as(dp)
    raw = lambda x: None if x is None else x.ctypes.data  # (host addresses: a refused call reads none of them)
    Hc, Vc = g._mat_input(H, ny, n), g._mat_input(V, ny, ny)
    buf_s, buf_u = np.zeros((B, T + 1, n * n)), np.zeros((B, T + 1, m * m))
    get, copy = g.lib.ilqr_get_estimator, g.lib.ilqr_copy_estimator_to_device

    def refused(word, t0, nk, ny_, Hx, Vx, Pf, Su, J):
        for code in (get(g.h, t0, nk, ny_, p(Hx), None, None, p(Vx), None, p(Pf), None, None, p(Su), p(J), None),
                     copy(g.h, t0, nk, ny_, raw(Hx), None, None, raw(Vx), None, raw(Pf), None, None, raw(Su), raw(J), None)):
            assert code == -1 and word in g.lib.ilqr_last_error(), (word, t0, nk, ny_, g.lib.ilqr_last_error())

    for t0, nk in ((-1, 1), (0, 0), (T + 1, 1), (3, T), (0, T + 2), (T, 2), (2, -1)):
        refused(b"window", t0, nk, ny, Hc, Vc, buf_s, None, None)
    for t0, nk in ((0, T + 1), (T, 1), (T - 2, 3)):  # Su with knot T in the window
        refused(b"knot T", t0, nk, ny, Hc, Vc, buf_s, buf_u, None)
    for bad_ny in (0, -1, n + 1):
        refused(b"ny", 0, 1, bad_ny, Hc, Vc, buf_s, None, None)
    refused(b"required", 0, 1, ny, None, Vc, buf_s, None, None)
    refused(b"required", 0, 1, ny, Hc, None, buf_s, None, None)
    refused(b"all null", 0, 1, ny, Hc, Vc, None, None, None)
    assert get(None, 0, 1, ny, p(Hc), None, None, p(Vc), None, p(buf_s), None, None, None, None, None) == -1
    # ... and none of them has disturbed the handle's answer
    assert np.array_equal(g.estimator(H, P0, W, V)["L"], full["L"])


def test_fresh_handle_is_a_state_error():
    from ilqr_amd import BatchILQR
    for g in (BatchILQR("acrobot", 4, 10, DT), BatchILQR("host", 4, 10, DT, nx=6, nu=2, u_min=-1.0, u_max=1.0)):
        s, Hc, Vc = np.zeros((4, 1, g.nx * g.nx)), np.zeros((4, g.nx)), np.ones((4, 1))
        assert g.lib.ilqr_get_estimator(g.h, 0, 1, 1, Hc.ctypes.data_as(dp), None, None, Vc.ctypes.data_as(dp), None, s.ctypes.data_as(dp), None, None, None,
                                        None, None) == -4
        assert g.lib.ilqr_copy_estimator_to_device(g.h, 0, 1, 1, Hc.ctypes.data, None, None, Vc.ctypes.data, None, s.ctypes.data, None, None, None, None,
                                                   None) == -4
        g.close()


# ---- 6. failure --------------------------------------------------------------------------------
def late_failure_V(d, K, H, P0, W, V, b):
    """A V for trajectory b with which the REFERENCE's first non-positive pivot falls at a knot >= 2, clearly: every earlier pivot above
    1e-6, the failing one below -1e-6 (found on the CPU; the caller asserts it)."""
    one = lambda a: None if a is None else a[b:b + 1]
    db = {name: d[name][b:b + 1] for name in NAMES}
    ny = H.shape[1]
    for c in np.geomspace(3.0, 1e-6, 600):  # (the first failing knot moves later as c shrinks)
        Vb = -c * np.eye(ny)[None]
        r = estimator_reference(db, K[b:b + 1], one(H), one(P0), one(W), Vb)
        t = int(r["info"][0]) - 1
        if t < 2:
            continue
        piv = r["pivots"][0]
        ok = piv[:t].min() > 1e-6 and np.nanmin(piv[t]) < -1e-6 and np.all(piv[t][:int(np.nanargmin(piv[t]))] > 1e-6)
        if ok:
            return Vb[0], t + 1
    return None, 0


@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_failed_trajectories(generic_handle, tiled_handle, which):
    g, H, P0, W, V = generic_handle if which == "generic" else tiled_handle
    B, ny = g.B, H.shape[1]
    d, K = g.derivatives(), g.gains()[1]
    good = everything(g, H, P0, W, V)
    Vbad = V.copy()
    Vbad[1] = -10.0 * np.eye(ny)
    Vbad[3], want3 = late_failure_V(d, K, H, P0, W, V, 3)
    assert want3 >= 3, "precondition: no V found whose first non-positive pivot falls at a knot >= 2"
    ref = estimator_reference(d, K, H, P0, W, Vbad)
    assert ref["info"][1] == 1 and ref["info"][3] == want3 and not np.delete(ref["info"], (1, 3)).any()  # the test's own precondition
    got = everything(g, H, P0, W, Vbad)
    assert np.array_equal(got["info"], ref["info"]), (got["info"], ref["info"])
    keep = np.delete(np.arange(B), (1, 3))
    for what in OUTPUTS:
        assert np.isnan(got[what][[1, 3]]).all(), what
        assert np.array_equal(got[what][keep], good[what][keep]), what
    # a window of a failed trajectory is NaN throughout, knots before the failure included
    w = g.estimator(H, P0, W, Vbad, t0=0, n_knots=want3, Pp=True, Sigma=True, info=True)
    assert all(np.isnan(w[what][3]).all() for what in ("Pp", "Pf", "L", "Sigma")) and w["info"][3] == want3
    # ... and a recursion that ends before the failing knot does not meet it
    w = g.estimator(H, P0, W, Vbad, t0=0, n_knots=want3 - 1, Pp=True, Sigma=True, info=True)
    assert all(np.isfinite(w[what][3]).all() for what in ("Pp", "Pf", "L", "Sigma")) and w["info"][3] == 0 and w["info"][1] == 1


# ---- 7. nx = 4 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model", ["acrobot", "double_integrator"])
def test_nx4(model, dtype):
    """B = 20 is no multiple of the 16-trajectory tile; the recursion is double in both dtypes, so one bound."""
    g, x0, u0, _ = nx4_handle(model, dtype, B=20, T=30)
    g.init_traj(x0, u0)
    g.iterate(3)
    g.compute_derivatives()
    d, K = g.derivatives(), g.gains()[1]
    for ny in (1, 2, 4):
        H, P0, W, V = estimator_inputs(4, ny, B=20)
        got = everything(g, H, P0, W, V)
        assert not got["info"].any()
        against_reference(got, reference_with_headroom(d, K, H, P0, W, V))
        check_the_bit_rules(got, P0)
    g.close()


# ---- 8. fp32 generic ---------------------------------------------------------------------------
def test_fp32_generic():
    """Float records and gains are widened, the recursion is double: the definition on the handle's float-valued records and gains."""
    from ilqr_amd import BatchILQR
    from tests.test_gpu_lq_end_to_end import lq_mats
    n, m, B, T, ny = 20, 5, 6, 12, 7
    g = BatchILQR("lq", B, T, DT, lq=lq_mats(n, m), u_min=-0.5, u_max=0.5, dtype="f32")
    rng = np.random.default_rng(5)
    g.init_traj(rng.uniform(-1, 1, (B, n)), rng.normal(size=(B, T, m)) * 0.3)
    g.iterate(2)
    H, P0, W, V = estimator_inputs(n, ny, B=B)
    got = everything(g, H, P0, W, V)
    against_reference(got, reference_with_headroom(g.derivatives(), g.gains()[1], H, P0, W, V))
    check_the_bit_rules(got, P0)
    g.close()


# ---- 10. device variant ------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["generic", "tiled"])
def test_copy_to_device_equals_the_getter(generic_handle, tiled_handle, which):
    import torch
    g, H, P0, W, V = generic_handle if which == "generic" else tiled_handle
    t0, nk, B, n, m, ny = 2, 5, g.B, g.nx, g.nu, H.shape[1]
    want = g.estimator(H, P0, W, V, t0=t0, n_knots=nk, Pp=True, Sigma=True, Su=True, expected_cost=True, info=True)
    dev = lambda a: torch.from_numpy(a).cuda()
    d_h, d_v, d_p0, d_w = dev(g._mat_input(H, ny, n)), dev(g._mat_input(V, ny, ny)), dev(g._cov_input(P0)), dev(g._cov_input(W))
    full = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device="cuda")
    o = dict(Pp=full(B, nk, n, n), Pf=full(B, nk, n, n), L=full(B, nk, ny, n), Sigma=full(B, nk, n, n), Su=full(B, nk, m, m), expected_cost=full(B))
    d_info = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (the copies and fills ran on torch's stream, the call runs on the handle's)
    g.copy_estimator_to_device(t0, nk, ny, d_h.data_ptr(), d_v.data_ptr(), d_p0.data_ptr(), d_w.data_ptr(), o["Pp"].data_ptr(), o["Pf"].data_ptr(),
                               o["L"].data_ptr(), o["Sigma"].data_ptr(), o["Su"].data_ptr(), o["expected_cost"].data_ptr(), d_info.data_ptr())
    g.synchronize()
    for what in OUTPUTS:
        a = o[what].cpu().numpy()
        assert np.array_equal(a if what == "expected_cost" else tr(a), want[what]), what
    assert np.array_equal(d_info.cpu().numpy(), want["info"])
    # the filter alone: the other buffers are not touched
    for what in ("Sigma", "Su", "expected_cost"):
        o[what].fill_(-7.0)
    o["L"].fill_(-7.0)
    torch.cuda.synchronize()
    g.copy_estimator_to_device(t0, nk, ny, d_h.data_ptr(), d_v.data_ptr(), d_p0.data_ptr(), d_w.data_ptr(), L_ptr=o["L"].data_ptr())
    g.synchronize()
    for what in ("Sigma", "Su", "expected_cost"):
        assert float(o[what].min()) == -7.0 == float(o[what].max()), what
    assert np.array_equal(tr(o["L"].cpu().numpy()), want["L"])


# ---- 11. read-only -----------------------------------------------------------------------------
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
    H, P0, W, V = estimator_inputs(g.nx, 2, B=g.B)
    got = everything(g, H, P0, W, V)
    against_reference(got, reference_with_headroom(g.derivatives(), g.gains()[1], H, P0, W, V))
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
    """ilqr_get_estimator against ilqr_copy_estimator_to_device, bit for bit: every pointer; H and V in (required), P0 and W null,
    expected_cost and info out (info alone is refused); that, every pointer, that again on one handle."""
    ny = 2

    def args(g):
        rng, n, m, nn = np.random.default_rng(3), g.nx, g.nu, gd.B * g.nx * g.nx
        return [gd.Arg("H", "req", rng.normal(size=(gd.B, ny, n))), gd.Arg("P0", "in", gd.spd(rng, n)), gd.Arg("W", "in", gd.spd(rng, n, 0.01)),
                gd.Arg("V", "req", gd.spd(rng, ny, 0.1)), gd.Arg("Pp", "out", (nn * gd.NK,)), gd.Arg("Pf", "out", (nn * gd.NK,)),
                gd.Arg("L", "out", (gd.B * gd.NK * n * ny,)), gd.Arg("Sigma", "out", (nn * gd.NK,)), gd.Arg("Su", "out", (gd.B * gd.NK * m * m,)),
                gd.Arg("expected_cost", "out", (gd.B,)), gd.Arg("info", "info", (gd.B,))]
    gd.check(lambda: gd.handle(which), case, "ilqr_get_estimator", "ilqr_copy_estimator_to_device", (gd.T0, gd.NK, ny), args)
