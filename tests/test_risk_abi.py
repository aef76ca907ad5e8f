"""CPU-side checks of the risk-sensitive entry points (ilqr_get_risk_sensitive, ilqr_copy_risk_sensitive_to_device): declared, exported,
bound, refusing a null handle without a device -- and the yardstick of tests/test_gpu_risk.py itself, against things written independently
of it: the dense saddle point of the disturbance game, the risk-adjusted value matrix inv(inv(P) - theta C C'), a scalar problem by hand
with both failure signs, tests/test_gpu_lq_solve.py's lq_reference at theta = 0, and that every input matters; then the headroom of the
GPU tests' inputs (float64 against np.longdouble, pivots away from zero) and that the facade's members compile."""
import ctypes as C_
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RISK_SYMBOLS = ("ilqr_get_risk_sensitive", "ilqr_copy_risk_sensitive_to_device")


def test_header_library_and_ctypes_table_carry_the_calls():
    from ilqr_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_amd.h")).read(), flags=re.S)
    lib = capi.load()
    for name in RISK_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*ilqr_batch\s*\*\s*h\s*,\s*int\s+nw\s*,\s*double\s+theta\s*,\s*int\s+flags\s*,\s*double\s+mu\s*," % name, src), name
        assert hasattr(lib, name) and name in capi.SYMBOLS
        # handle; nw, theta, flags, mu; C; K, k, Vx, Vxx, risk_cost; info
        assert len(capi.SYMBOLS[name][1]) == 12 and capi.SYMBOLS[name][1][1:5] == [C_.c_int, C_.c_double, C_.c_int, C_.c_double]
    dp, ip = C_.POINTER(C_.c_double), C_.POINTER(C_.c_int)
    assert capi.SYMBOLS["ilqr_get_risk_sensitive"][1][5:] == [dp] * 6 + [ip]
    assert capi.SYMBOLS["ilqr_copy_risk_sensitive_to_device"][1][5:] == [C_.c_void_p] * 7
    names = lambda fn: [w.split()[-1].lstrip("*") for w in re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % fn, src).group(1).split(",")]
    assert names("ilqr_get_risk_sensitive") == ["h", "nw", "theta", "flags", "mu", "C", "K", "k", "Vx", "Vxx", "risk_cost", "info"]
    assert names("ilqr_copy_risk_sensitive_to_device") == ["h", "nw", "theta", "flags", "mu", "C_device", "K_device", "k_device", "Vx_device",
                                                           "Vxx_device", "risk_cost_device", "info_device"]
    assert lib.ilqr_abi_version() == 6  # additive: the ABI number and ilqr_desc stay


def test_null_handle_is_refused():
    """ILQR_ERR_INVALID before anything else is looked at (the other refusals need a handle, hence a device: tests/test_gpu_risk.py)."""
    from ilqr_amd import capi
    lib = capi.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C_.POINTER(C_.c_double))
    assert lib.ilqr_get_risk_sensitive(None, 1, 0.5, 0, 0.0, p, p, p, None, None, None, None) == -1 and b"null handle" in lib.ilqr_last_error()
    assert lib.ilqr_copy_risk_sensitive_to_device(None, 1, 0.5, 0, 0.0, buf.ctypes.data, buf.ctypes.data, None, None, None, None, None) == -1
    assert b"null handle" in lib.ilqr_last_error()


def convex_records(n, m, T, seed, B=1):
    """Records with [cxx cxu; cxu' cuu] = 0.5 I + G G' per knot, as tests/test_gpu_lq_solve.py's convex_policy makes them."""
    rng = np.random.default_rng(seed)
    G = rng.normal(size=(B, T + 1, n + m, n + m)) / np.sqrt(n + m)
    H = 0.5 * np.eye(n + m) + G @ np.swapaxes(G, -1, -2)
    return dict(fx=np.eye(n) + 0.2 * rng.normal(size=(B, T + 1, n, n)), fu=rng.normal(size=(B, T + 1, n, m)) / np.sqrt(n),
                cx=rng.normal(size=(B, T + 1, n)), cu=rng.normal(size=(B, T + 1, m)),
                cxx=np.ascontiguousarray(H[..., :n, :n]), cxu=np.ascontiguousarray(H[..., :n, n:]), cuu=np.ascontiguousarray(H[..., n:, n:]))


def test_yardstick_is_the_saddle_point_of_the_game():
    """(a) The quadratic in (du[0..T-1], xi[0..T-1]) got by rolling the LQ model out from dx0, with -|xi|^2 / (2 theta) per knot, solved
    densely for its stationary point; the yardstick's gains rolled out under that worst-case xi give the same controls."""
    from tests.test_gpu_risk import risk_reference
    n, m, nw, T, theta = 3, 2, 2, 3, 0.4
    d = convex_records(n, m, T, seed=11)
    rng = np.random.default_rng(12)
    C, dx0 = 0.2 * rng.normal(size=(1, n, nw)), rng.normal(size=n)
    ref = risk_reference(d, np.ones((1, T, m, n)), C, theta)
    assert not ref["info"].any()
    nz = T * (m + nw)
    Eu = lambda t: np.eye(nz)[t * m:(t + 1) * m]
    Ex = lambda t: np.eye(nz)[T * m + t * nw:T * m + (t + 1) * nw]
    a, S = dx0, np.zeros((n, nz))
    g, H = np.zeros(nz), np.zeros((nz, nz))
    for t in range(T + 1):
        cxx, cx = d["cxx"][0, t], d["cx"][0, t]
        g += S.T @ cx + S.T @ cxx @ a
        H += S.T @ cxx @ S
        if t == T:
            break
        cxu, cuu, cu = d["cxu"][0, t], d["cuu"][0, t], d["cu"][0, t]
        g += Eu(t).T @ cu + Eu(t).T @ cxu.T @ a
        H += S.T @ cxu @ Eu(t) + Eu(t).T @ cxu.T @ S + Eu(t).T @ cuu @ Eu(t) - Ex(t).T @ Ex(t) / theta
        a, S = d["fx"][0, t] @ a, d["fx"][0, t] @ S + d["fu"][0, t] @ Eu(t) + C[0] @ Ex(t)
    z = np.linalg.solve(0.5 * (H + H.T), -g)
    x, worst = dx0, 0.0
    for t in range(T):
        u = ref["K"][0, t] @ x + ref["k"][0, t]
        worst = max(worst, float(np.abs(u - Eu(t) @ z).max()))
        x = d["fx"][0, t] @ x + d["fu"][0, t] @ u + C[0] @ (Ex(t) @ z)
    print("  feedback controls under the worst-case disturbance vs the dense saddle point: %.3g" % worst)
    assert worst <= 1e-12 and np.abs(z).max() > 1e-2


def test_yardstick_risk_adjusted_value_matrix():
    """(b) Pt = inv(inv(P) - theta C C') for a full-rank C: with fx = I, fu = 0, cxx[0] = 0 and cxu = 0 the step returns Vxx[0] = Pt."""
    from tests.test_gpu_risk import risk_reference
    n, theta = 5, 0.4
    rng = np.random.default_rng(21)
    G = rng.normal(size=(n, n)) / np.sqrt(n)
    P = 0.5 * np.eye(n) + G @ G.T
    C = 0.5 * rng.normal(size=(1, n, n)) / np.sqrt(n)
    d = dict(fx=np.broadcast_to(np.eye(n), (1, 2, n, n)), fu=np.zeros((1, 2, n, 1)), cx=np.zeros((1, 2, n)), cu=np.zeros((1, 2, 1)),
             cxx=np.stack([np.zeros((n, n)), P])[None], cxu=np.zeros((1, 2, n, 1)), cuu=np.ones((1, 2, 1, 1)))
    for th in (theta, -theta):
        ref = risk_reference(d, np.ones((1, 1, 1, n)), C, th)
        want = np.linalg.inv(np.linalg.inv(P) - th * C[0] @ C[0].T)
        gap = float(np.abs(ref["Vxx"][0, 0] - want).max())
        print("  Pt vs inv(inv(P) - theta C C'), theta %g: %.3g" % (th, gap))
        assert not ref["info"].any() and gap <= 1e-12 and np.abs(want - P).max() > 1e-2


def scalar_records(fx, fu, cx, cu, cxx, cxu, cuu, cxT, cxxT):
    d = {name: np.zeros((1, 2, 1, 1)) for name in ("fx", "fu", "cxx", "cxu", "cuu")}
    d.update(cx=np.zeros((1, 2, 1)), cu=np.zeros((1, 2, 1)))
    for name, val in (("fx", fx), ("fu", fu), ("cxx", cxx), ("cxu", cxu), ("cuu", cuu)):
        d[name][0, 0, 0, 0] = val
    d["cx"][0, 0, 0], d["cu"][0, 0, 0], d["cx"][0, 1, 0], d["cxx"][0, 1, 0, 0] = cx, cu, cxT, cxxT
    return d


def test_yardstick_on_a_scalar_problem():
    """(c) n = m = nw = 1, T = 1, by hand: every output, both failure signs."""
    from tests.test_gpu_risk import risk_reference
    fx, fu, cx, cu, cxx, cxu, cuu, cxT, cxxT, c, theta, mu = 0.9, 0.5, 0.3, -0.2, 2.0, 0.1, 1.5, 0.7, 3.0, 0.4, 0.5, 0.25
    d = scalar_records(fx, fu, cx, cu, cxx, cxu, cuu, cxT, cxxT)
    one = np.ones((1, 1, 1, 1))
    r = risk_reference(d, one, c * one[0], theta, mu)
    M = 1 - theta * c * c * cxxT
    Pt = cxxT + theta * (cxxT * c) ** 2 / M
    vt = cxT + theta * cxxT * c * c * cxT / M
    st = theta / 2 * (c * cxT) ** 2 / M - np.log(np.sqrt(M)) / theta
    Qx, Qu, Qxx, Qux, Quu = cx + fx * vt, cu + fu * vt, cxx + fx * Pt * fx, cxu + fu * Pt * fx, cuu + fu * Pt * fu + mu
    K, k = -Qux / Quu, -Qu / Quu
    near = lambda x, y: abs(x - y) < 1e-14
    assert r["info"][0] == 0 and near(r["K"][0, 0, 0, 0], K) and near(r["k"][0, 0, 0], k)
    assert near(r["Vxx"][0, 0, 0, 0], Qxx + Qux * K) and near(r["Vx"][0, 0, 0], Qx + K * Qu) and near(r["risk_cost"][0], st + 0.5 * Qu * k)
    assert r["Vxx"][0, 1, 0, 0] == cxxT and r["Vx"][0, 1, 0] == cxT
    # theta = 0 exactly: the trace term
    r0 = risk_reference(d, one, c * one[0], 0.0, mu)
    Qu0, Quu0 = cu + fu * cxT, cuu + fu * cxxT * fu + mu
    assert near(r0["risk_cost"][0], 0.5 * c * c * cxxT - 0.5 * Qu0 * Qu0 / Quu0)
    # breakdown: theta c^2 P >= 1; and a Quu that is not positive
    bad = risk_reference(d, one, 1.0 * one[0], theta, mu)
    assert bad["info"][0] == -1 and all(np.isnan(bad[name]).all() for name in ("K", "k", "Vx", "Vxx", "risk_cost"))
    bad = risk_reference(scalar_records(fx, fu, cx, cu, cxx, cxu, -2.0, cxT, cxxT), one, c * one[0], theta, 0.0)
    assert bad["info"][0] == 1 and all(np.isnan(bad[name]).all() for name in ("K", "k", "Vx", "Vxx", "risk_cost"))


@pytest.mark.parametrize("hold", [False, True])
def test_yardstick_at_theta_zero_is_lq_reference(hold):
    """(d) dx0 = I gives dus[0] = K[0] and dlam[0] = P[0]; gx = cx, gu = cu gives dlam[0] = v[0]."""
    from tests.test_gpu_lq_solve import convex_policy, lq_reference
    from tests.test_gpu_risk import noise, risk_reference
    n, m, nw, mu = 6, 2, 3, 0.2
    d, _, K = convex_policy(n, m)
    B, T = K.shape[:2]
    ref = risk_reference(d, K, noise(n, nw, B, 0.1), 0.0, mu, hold)
    eye = np.broadcast_to(np.eye(n), (B, n, n))
    _, dus, dlam, info = lq_reference(d, K, dx0=eye, mu=mu, hold=hold)
    assert not info.any() and not ref["info"].any()
    tr = lambda a: np.swapaxes(a, -1, -2)
    lin = lq_reference(d, K, gx=d["cx"][:, :, None], gu=d["cu"][:, :T, None], mu=mu, hold=hold)[2]
    for got, want, what in ((ref["K"][:, 0], tr(dus[:, 0]), "K[0]"), (ref["Vxx"][:, 0], tr(dlam[:, 0]), "Vxx[0]"), (ref["Vx"][:, 0], lin[:, 0, 0], "Vx[0]")):
        gap, scale = float(np.abs(got - want).max()), max(1.0, float(np.abs(want).max()))
        print("  theta = 0 vs lq_reference, %s: %.3g (scale %.3g)" % (what, gap, scale))
        assert gap <= 1e-12 * scale, (what, gap)


def test_every_input_moves_the_gains():
    """(e) C, theta, mu and the hold flag each move the gains by more than 1e-4."""
    from tests.test_gpu_lq_solve import convex_policy
    from tests.test_gpu_risk import noise, risk_reference
    n, m, nw = 8, 3, 4
    d, _, K = convex_policy(n, m)
    C = noise(n, nw, K.shape[0], 0.1)
    base = dict(C=C, theta=0.5, mu=0.0, hold=False)
    ref = risk_reference(d, K, **base)
    assert not ref["info"].any()
    for change in (dict(C=2 * C), dict(theta=-0.5), dict(theta=0.0), dict(mu=0.5), dict(hold=True)):
        other = risk_reference(d, K, **dict(base, **change))
        assert not other["info"].any()
        for name in ("K", "k"):
            assert np.abs(other[name] - ref[name]).max() > 1e-4, (list(change), name)


def test_the_yardstick_has_its_headroom():
    """On the GPU tests' inputs (convex_policy, theta = +-0.5, with and without held controls): some noise scale of the list qualifies --
    float64 and np.longdouble within 1e-10 x scale on every output, no pivot of M below 0.2, none of Quu_FF below 0.05 -- and at that
    scale the gains still differ from theta = 0's by more than 1e-4."""
    from tests.test_gpu_lq_solve import convex_policy
    from tests.test_gpu_risk import GENERIC_CASES, generic_case, risk_reference
    least = np.inf
    for n, m, nw in GENERIC_CASES:
        d, _, K = convex_policy(n, m)
        for hold in (False, True):
            for theta in (0.5, -0.5):
                s, C, ref = generic_case(n, m, nw, theta, 0.0, hold)  # (raises if no scale qualifies)
                effect = float(np.abs(ref["K"] - risk_reference(d, K, C, 0.0, 0.0, hold)["K"]).max())
                print("  n %d m %d nw %d theta %g hold %s: s = %g, effect on K %.3g" % (n, m, nw, theta, hold, s, effect))
                assert effect > 1e-4, (n, m, nw, theta, hold, s, effect)
                least = min(least, effect)
    print("  smallest effect on K: %.3g" % least)


def test_facade_risk_caller_compiles(tmp_path):
    """The facade's members compile without a device: a translation unit that only names them."""
    src = tmp_path / "risk_names.cpp"
    src.write_text(r'''
#include "ilqr_amd.hpp"
void f(ilqr_amd::BatchILQR& b, void* dev) {
  std::vector<double> C, K, k, Vx, Vxx, J; std::vector<int> info;
  b.risk_sensitive(2, 0.5, C, &K, &k);
  b.risk_sensitive(2, -0.5, C, nullptr, nullptr, &Vx, &Vxx, &J, &info, ILQR_LQ_HOLD_CLAMPED, 0.1);
  b.copy_risk_sensitive_to_device(2, 0.5, 0, 0.0, dev, dev, dev, nullptr, nullptr, nullptr, dev);
}
''')
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-DILQR_AMD_NO_EIGEN", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "risk_names.o")])
