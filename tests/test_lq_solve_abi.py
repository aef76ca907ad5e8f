"""CPU-side checks of ilqr_solve_lq / ilqr_solve_lq_on_device: declared, exported, bound, refusing a null handle without a device -- and
the yardstick of tests/test_gpu_lq_solve.py itself: on every size of its cases the float64 recursion agrees with np.longdouble within
1e-10 x max(1, max|.|), a factor 10 inside the bound the device is held to, and with a dense KKT solve of the same problem (an
independent method: one np.linalg.solve of the whole optimality system, multipliers included) within 1e-12 x scale; the problems are
well conditioned, nothing decays or blows up, every input matters; a scalar problem by hand; the solution operator is symmetric."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQ_SYMBOLS = ("ilqr_solve_lq", "ilqr_solve_lq_on_device")
SIZES = [(32, 16), (20, 5), (8, 3), (17, 17), (24, 20), (32, 32), (6, 1), (6, 2), (4, 1), (4, 2)]


def test_header_library_and_ctypes_table_carry_the_calls():
    from ilqr_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_amd.h")).read(), flags=re.S)
    lib = capi.load()
    for name in LQ_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*ilqr_batch\s*\*\s*h\s*,\s*int\s+n_dirs\s*,\s*int\s+flags\s*,\s*double\s+mu\s*," % name, src), name
        assert hasattr(lib, name) and name in capi.SYMBOLS
        assert len(capi.SYMBOLS[name][1]) == 11 and capi.SYMBOLS[name][1][1:4] == [C.c_int, C.c_int, C.c_double]
    assert re.search(r"\bILQR_LQ_HOLD_CLAMPED\s*=\s*1\b", src) and capi.LQ_HOLD_CLAMPED == 1
    assert lib.ilqr_abi_version() == 6  # additive: the ABI number and ilqr_desc stay


def test_null_handle_is_refused():
    from ilqr_amd import capi
    lib = capi.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ilqr_solve_lq(None, 1, 0, 0.0, p, p, p, p, p, p, None) == -1 and b"null handle" in lib.ilqr_last_error()
    assert lib.ilqr_solve_lq_on_device(None, 1, 0, 0.0, buf.ctypes.data, None, None, buf.ctypes.data, None, None, None) == -1
    assert b"null handle" in lib.ilqr_last_error()


def kkt_solve(d, K, b, dx0, gx, gu, mu, hold):
    """Trajectory b's optimality system, solved whole: unknowns (dx[0..T], du[0..T-1], dlam[0..T], the held controls' multipliers).
    Lagrangian: cost + sum_t dlam[t+1]'(fx dx[t] + fu du[t] - dx[t+1]) + dlam[0]'(dx0 - dx[0]).  Returns (dxs, dus, dlam, condition)."""
    from tests.test_gpu_lq_solve import held_rows
    B, T, m, n = K.shape
    S = dx0.shape[1]
    held = held_rows(K, hold)[b]
    ox, ou = lambda t: t * n, lambda t: (T + 1) * n + t * m
    nz = (T + 1) * n + T * m
    ol = lambda t: nz + t * n
    hidx = [(t, e) for t in range(T) for e in range(m) if held[t, e]]
    N = nz + (T + 1) * n + len(hidx)
    M, rhs = np.zeros((N, N)), np.zeros((N, S))
    for t in range(T + 1):
        X = slice(ox(t), ox(t) + n)
        M[X, X] = d["cxx"][b, t]
        rhs[X] = -gx[b, t].T
        M[X, ol(t):ol(t) + n] -= np.eye(n)  # -dlam[t]
        M[ol(t):ol(t) + n, X] -= np.eye(n)
        if t == T:
            break
        U = slice(ou(t), ou(t) + m)
        M[U, U] = d["cuu"][b, t] + mu * np.eye(m)
        M[X, U], M[U, X] = d["cxu"][b, t], d["cxu"][b, t].T
        rhs[U] = -gu[b, t].T
        Ln = slice(ol(t + 1), ol(t + 1) + n)
        M[X, Ln] += d["fx"][b, t].T
        M[Ln, X] += d["fx"][b, t]
        M[U, Ln] += d["fu"][b, t].T
        M[Ln, U] += d["fu"][b, t]
    rhs[ol(0):ol(0) + n] = -dx0[b].T
    for i, (t, e) in enumerate(hidx):
        r = nz + (T + 1) * n + i
        M[r, ou(t) + e] = M[ou(t) + e, r] = 1.0
    z = np.linalg.solve(M, rhs)
    dxs = z[:(T + 1) * n].reshape(T + 1, n, S).transpose(0, 2, 1)
    dus = z[(T + 1) * n:nz].reshape(T, m, S).transpose(0, 2, 1)
    dlam = z[nz:nz + (T + 1) * n].reshape(T + 1, n, S).transpose(0, 2, 1)
    return dxs, dus, dlam, np.linalg.cond(M)


@pytest.mark.parametrize("n,m", SIZES)
def test_the_yardstick_earns_its_use(n, m):
    from tests.test_gpu_lq_solve import convex_policy, directions, lq_reference, scale_of, with_headroom
    d, k, K = convex_policy(n, m)
    dx0, gx, gu = directions(n, m, 3)
    for mu, hold in ((0.0, True), (0.7, False)):
        dxs, dus, dlam, info = with_headroom(d, K, dx0, gx, gu, mu, hold)  # (asserts the 1e-10 agreement with np.longdouble)
        assert not info.any()
        for b in range(K.shape[0]):
            kx, ku, kl, cond = kkt_solve(d, K, b, dx0, gx, gu, mu, hold)
            assert cond <= 1e4, cond
            for got, want, what in ((dxs[b], kx, "dxs"), (dus[b], ku, "dus"), (dlam[b], kl, "dlam")):
                err = float(np.abs(got - want).max())
                assert err <= 1e-12 * scale_of(want), (what, b, err, scale_of(want))
        # neither decayed nor blown up
        assert 0.5 <= np.abs(dxs).max() < 30 and 0.5 <= np.abs(dus).max() < 30 and 1.0 <= np.abs(dlam).max() < 300
        assert np.abs(dxs[:, -1]).max() > 0.05 and np.abs(dlam[:, 0]).max() > 0.5
    # every input matters
    base = lq_reference(d, K, dx0, gx, gu, 0.0, True)
    for other in (lq_reference(d, K, None, gx, gu, 0.0, True), lq_reference(d, K, dx0, None, gu, 0.0, True), lq_reference(d, K, dx0, gx, None, 0.0, True),
                  lq_reference(d, K, dx0, gx, gu, 0.7, True), lq_reference(d, K, dx0, gx, gu, 0.0, False)):
        assert np.abs(other[1] - base[1]).max() > 1e-3 and np.abs(other[0] - base[0]).max() > 1e-3


def test_yardstick_on_a_scalar_problem():
    """n = m = 1, T = 2, by hand."""
    from tests.test_gpu_lq_solve import lq_reference
    fx, fu, cxx, cxu, cuu = (0.9, 1.1), (0.5, -0.4), (1.2, 0.8, 1.5), (0.1, -0.2), (0.7, 0.9)
    d = {kk: np.zeros((1, 3, 1, 1)) for kk in ("fx", "fu", "cxx", "cxu", "cuu")}
    for t in range(3):
        d["cxx"][0, t, 0, 0] = cxx[t]
        if t < 2:
            d["fx"][0, t, 0, 0], d["fu"][0, t, 0, 0], d["cxu"][0, t, 0, 0], d["cuu"][0, t, 0, 0] = fx[t], fu[t], cxu[t], cuu[t]
    K = np.ones((1, 2, 1, 1))
    x0, gx, gu, mu = 0.8, (0.3, -1.2, 2.0), (0.6, -0.1), 0.25
    dxs, dus, dlam, info = lq_reference(d, K, np.array([[[x0]]]), np.array(gx).reshape(1, 3, 1, 1), np.array(gu).reshape(1, 2, 1, 1), mu, True)
    P2, v2 = cxx[2], gx[2]
    quu1 = cuu[1] + fu[1] * P2 * fu[1] + mu
    qux1 = cxu[1] + fu[1] * P2 * fx[1]
    Kd1 = -qux1 / quu1
    P1 = cxx[1] + fx[1] * P2 * fx[1] + qux1 * Kd1
    w1 = gu[1] + fu[1] * v2
    kd1 = -w1 / quu1
    v1 = gx[1] + fx[1] * v2 + Kd1 * w1
    quu0 = cuu[0] + fu[0] * P1 * fu[0] + mu
    qux0 = cxu[0] + fu[0] * P1 * fx[0]
    Kd0 = -qux0 / quu0
    P0 = cxx[0] + fx[0] * P1 * fx[0] + qux0 * Kd0
    w0 = gu[0] + fu[0] * v1
    kd0 = -w0 / quu0
    v0 = gx[0] + fx[0] * v1 + Kd0 * w0
    u0 = Kd0 * x0 + kd0
    x1 = fx[0] * x0 + fu[0] * u0
    u1 = Kd1 * x1 + kd1
    x2 = fx[1] * x1 + fu[1] * u1
    assert not info.any() and dxs[0, 0, 0, 0] == x0
    assert np.allclose(dxs[0, 1:, 0, 0], (x1, x2), rtol=0, atol=1e-14) and np.allclose(dus[0, :, 0, 0], (u0, u1), rtol=0, atol=1e-14)
    assert np.allclose(dlam[0, :, 0, 0], (P0 * x0 + v0, P1 * x1 + v1, P2 * x2 + v2), rtol=0, atol=1e-14)
    # the multipliers' own recursion
    assert abs(dlam[0, 1, 0, 0] - (gx[1] + cxx[1] * x1 + cxu[1] * u1 + fx[1] * dlam[0, 2, 0, 0])) < 1e-14
    # held (K row zero): du = 0 and the state runs open loop; an indefinite Quu only fails where it is free
    dxs, dus, _, info = lq_reference(d, np.zeros_like(K), np.array([[[x0]]]), None, None, mu, True)
    assert not info.any() and np.array_equal(dus, np.zeros_like(dus)) and np.allclose(dxs[0, :, 0, 0], (x0, fx[0] * x0, fx[1] * fx[0] * x0), rtol=0, atol=1e-15)
    d["cuu"][0, 1, 0, 0] = -50.0
    assert lq_reference(d, K, np.array([[[x0]]]), None, None, mu, True)[3][0] == 2
    assert lq_reference(d, np.zeros_like(K), np.array([[[x0]]]), None, None, mu, True)[3][0] == 0


@pytest.mark.parametrize("n,m", SIZES)
def test_the_solution_operator_is_symmetric(n, m):
    """With dx0 = 0 the map g -> S g = (dxs, dus) is minus the inverse of the reduced Hessian: <g2, S g1> = <g1, S g2>."""
    from tests.test_gpu_lq_solve import convex_policy, directions, lq_reference, scale_of
    d, k, K = convex_policy(n, m)
    _, gx1, gu1 = directions(n, m, 3, seed=1)
    _, gx2, gu2 = directions(n, m, 3, seed=2)
    for mu, hold in ((0.0, True), (0.7, False)):
        x1, u1 = lq_reference(d, K, None, gx1, gu1, mu, hold)[:2]
        x2, u2 = lq_reference(d, K, None, gx2, gu2, mu, hold)[:2]
        lhs = (gx2 * x1).sum(axis=(1, 3)) + (gu2 * u1).sum(axis=(1, 3))
        rhs = (gx1 * x2).sum(axis=(1, 3)) + (gu1 * u2).sum(axis=(1, 3))
        assert np.abs(lhs).max() > 0.1 and np.abs(lhs - rhs).max() <= 1e-12 * scale_of(lhs), np.abs(lhs - rhs).max()


def test_facade_lq_solve_caller_compiles(tmp_path):
    """The facade's members compile without a device: a translation unit that only names them."""
    src = tmp_path / "lq_solve_names.cpp"
    src.write_text(r'''
#include "ilqr_amd.hpp"
void f(ilqr_amd::iLQR& s, ilqr_amd::BatchILQR& b, void* dev) {
  ilqr_amd::MatrixXd dx0(4, 3); ilqr_amd::VecOfMatXd gx, gu, dxs, dus, dlam;
  int i = s.lq_solve(gx, gu, dx0, dxs, dus); i += s.lq_solve(gx, gu, dx0, dxs, dus, &dlam, 0.5, false);
  std::vector<double> a, c, d, e, g, l;
  std::vector<int> info = b.lq_solve(3, &a, &c, &d, &e, &g); info = b.lq_solve(3, nullptr, &c, nullptr, &e, nullptr, &l, 1.0, false);
  b.solve_lq_on_device(3, ILQR_LQ_HOLD_CLAMPED, 0.0, dev, nullptr, nullptr, dev, nullptr, nullptr, nullptr);
  (void)i;
}
''')
    for extra in (["-DILQR_AMD_NO_EIGEN"], []):  # (without the macro: Eigen's types where Eigen is installed, the stand-ins elsewhere)
        subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall"] + extra + ["-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "lq_solve_names.o")])
