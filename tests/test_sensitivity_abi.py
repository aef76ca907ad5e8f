"""CPU-side checks of the tangent and adjoint entry points (ilqr_get_tangent, ilqr_copy_tangent_to_device, ilqr_get_adjoint,
ilqr_copy_adjoint_to_device): declared, exported, bound, refusing a null handle without a device -- and the yardstick of
tests/test_gpu_sensitivity.py itself: on every input of its generic and nx = 4 cases the float64 recursion agrees with np.longdouble
within 1e-10 x max(1, max|.|), a factor 10 inside the bound the device is held to; the inputs neither blow up nor decay over the horizon;
every input matters; and the two recursions are each other's transposes, the adjoint is the value model's Vx, the tangent squares to the
covariance."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENS_SYMBOLS = ("ilqr_get_tangent", "ilqr_copy_tangent_to_device", "ilqr_get_adjoint", "ilqr_copy_adjoint_to_device")
SIZES = [(32, 16), (20, 5), (8, 3), (17, 17), (24, 20), (32, 32), (6, 1), (6, 2), (4, 1), (4, 2)]


def test_header_library_and_ctypes_table_carry_the_calls():
    from ilqr_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_amd.h")).read(), flags=re.S)
    lib = capi.load()
    for name in SENS_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*ilqr_batch\s*\*\s*h\s*,\s*int\s+t0\s*,\s*int\s+n_knots\s*,\s*int\s+n_dirs\s*," % name, src), name
        assert hasattr(lib, name) and name in capi.SYMBOLS
        assert len(capi.SYMBOLS[name][1]) == 8 and capi.SYMBOLS[name][1][1:4] == [C.c_int, C.c_int, C.c_int]
    assert lib.ilqr_abi_version() == 6  # additive: the ABI number and ilqr_desc stay


def test_null_handle_is_refused():
    from ilqr_amd import capi
    lib = capi.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    for name in ("ilqr_get_tangent", "ilqr_get_adjoint"):
        assert getattr(lib, name)(None, 0, 1, 1, p, p, p, None) == -1 and b"null handle" in lib.ilqr_last_error()
    for name in ("ilqr_copy_tangent_to_device", "ilqr_copy_adjoint_to_device"):
        assert getattr(lib, name)(None, 0, 1, 1, buf.ctypes.data, None, buf.ctypes.data, None) == -1 and b"null handle" in lib.ilqr_last_error()


def yardstick_inputs(n, m, B=5, T=12):
    """The inputs of the headroom check: dx0 = I with random dv (1 % of a unit of control in every direction, as the du of a clone or
    exploration noise is: Phi itself reaches 2.9 at these sizes); three directions of standard-normal gx, gu."""
    from tests.test_gpu_sensitivity import identity_directions
    rng = np.random.default_rng(4000 + 10 * n + m)
    return identity_directions(n, B), 0.01 * rng.normal(size=(B, T, n, m)), rng.normal(size=(B, T + 1, 3, n)), rng.normal(size=(B, T, 3, m))


@pytest.mark.parametrize("n,m", SIZES)
def test_the_yardstick_has_its_headroom(n, m):
    from tests.test_gpu_sensitivity import adjoint_reference, generic_policy, tangent_reference, with_headroom
    d, k, K = generic_policy(n, m)
    dx0, dv, gx, gu = yardstick_inputs(n, m)
    dxs, dus = with_headroom(tangent_reference, d, K, dx0, dv)  # (asserts the 1e-10 agreement with np.longdouble)
    a, w = with_headroom(adjoint_reference, d, K, gx, gu)
    # neither blown up nor decayed over the horizon
    assert 1.0 <= np.abs(dxs).max() < 3.0, np.abs(dxs).max()
    assert np.abs(dxs[:, -1]).max() > 0.1 and 1.0 < np.abs(a).max() < 30.0, (np.abs(dxs[:, -1]).max(), np.abs(a).max())
    # pure functions of (records, K) and the caller's vectors: each of them matters
    zK = np.zeros_like(K)
    assert np.abs(tangent_reference(d, zK, dx0, dv)[0] - dxs).max() > 1e-3 and np.abs(adjoint_reference(d, zK, gx, gu)[0] - a).max() > 1e-3
    assert np.abs(tangent_reference(d, K, None, dv)[0] - dxs).max() > 1e-3 and np.abs(tangent_reference(d, K, dx0, None)[0] - dxs).max() > 1e-3
    assert np.abs(adjoint_reference(d, K, None, gu)[0] - a).max() > 1e-3 and np.abs(adjoint_reference(d, K, gx, None)[0] - a).max() > 1e-3
    assert np.abs(adjoint_reference(d, K, gx, None)[1] - w).max() > 1e-3


def test_yardstick_on_a_scalar_problem():
    """n = m = 1, T = 2, by hand."""
    from tests.test_gpu_sensitivity import adjoint_reference, tangent_reference
    fx, fu, K = (0.9, 1.1), (0.5, -0.4), (-0.7, 0.3)
    d = dict(fx=np.zeros((1, 3, 1, 1)), fu=np.zeros((1, 3, 1, 1)))
    Km = np.zeros((1, 2, 1, 1))
    for t in range(2):
        d["fx"][0, t, 0, 0], d["fu"][0, t, 0, 0], Km[0, t, 0, 0] = fx[t], fu[t], K[t]
    x0, v = 0.8, (0.25, -0.5)
    dxs, dus = tangent_reference(d, Km, np.array([[[x0]]]), np.array([[[[v[0]]], [[v[1]]]]]))
    u0 = K[0] * x0 + v[0]
    x1 = fx[0] * x0 + fu[0] * u0
    u1 = K[1] * x1 + v[1]
    x2 = fx[1] * x1 + fu[1] * u1
    assert dxs[0, 0, 0, 0] == x0 and np.allclose(dxs[0, 1:, 0, 0], (x1, x2), rtol=0, atol=1e-15) and np.allclose(dus[0, :, 0, 0], (u0, u1), rtol=0, atol=1e-15)
    gx, gu = (0.3, -1.2, 2.0), (0.6, -0.1)
    a, w = adjoint_reference(d, Km, np.array(gx).reshape(1, 3, 1, 1), np.array(gu).reshape(1, 2, 1, 1))
    a2 = gx[2]
    w1 = gu[1] + fu[1] * a2
    a1 = gx[1] + fx[1] * a2 + K[1] * w1
    w0 = gu[0] + fu[0] * a1
    a0 = gx[0] + fx[0] * a1 + K[0] * w0
    assert a[0, 2, 0, 0] == a2 and np.allclose(a[0, :2, 0, 0], (a0, a1), rtol=0, atol=1e-15) and np.allclose(w[0, :, 0, 0], (w0, w1), rtol=0, atol=1e-15)
    # and the two are transposes of each other
    assert abs((gx[0] * x0 + gx[1] * x1 + gx[2] * x2 + gu[0] * u0 + gu[1] * u1) - (a0 * x0 + w0 * v[0] + w1 * v[1])) < 1e-15


@pytest.mark.parametrize("n,m", SIZES)
def test_three_identities_hold_on_the_yardstick(n, m):
    """(a) the transpose identity; (b) with k = 0 the adjoint of (cx, cu) is the value model's Vx at every knot; (c) with W = 0 and a
    symmetric Sigma0, Phi[t] Sigma0 Phi[t]' is the covariance at every knot: each to 1e-12 x scale."""
    from tests.test_gpu_covariance import cov_reference, noise_inputs
    from tests.test_gpu_sensitivity import adjoint_reference, directions, generic_policy, identity_directions, scale_of, tangent_reference
    from tests.test_gpu_value import value_reference
    d, k, K = generic_policy(n, m)
    tr = lambda M: np.swapaxes(M, -1, -2)
    # (a)
    dx0, dv, gx, gu = directions(n, m, 3)
    dxs, dus = tangent_reference(d, K, dx0, dv)
    a, w = adjoint_reference(d, K, gx, gu)
    lhs = (gx * dxs).sum(axis=(1, 3)) + (gu * dus).sum(axis=(1, 3))
    rhs = (a[:, 0] * dx0).sum(axis=2) + (w * dv).sum(axis=(1, 3))
    assert np.abs(lhs).max() > 0.1 and np.abs(lhs - rhs).max() <= 1e-12 * scale_of(lhs), np.abs(lhs - rhs).max()
    # (b)
    a, _ = adjoint_reference(d, K, d["cx"][:, :, None, :], d["cu"][:, :-1, None, :])
    Vx, _ = value_reference(d, np.zeros_like(k), K)
    assert np.abs(a[:, :, 0] - Vx).max() <= 1e-12 * scale_of(Vx), np.abs(a[:, :, 0] - Vx).max()
    # (c)
    S0, _ = noise_inputs(n)
    Phi = tr(tangent_reference(d, K, identity_directions(n), None)[0])
    Sigma, _, _ = cov_reference(d, K, S0, None)
    assert np.abs(Phi @ S0[:, None] @ tr(Phi) - Sigma).max() <= 1e-12 * scale_of(Sigma), np.abs(Phi @ S0[:, None] @ tr(Phi) - Sigma).max()


def test_facade_sensitivity_caller_compiles(tmp_path):
    """The facade's members compile without a device: a translation unit that only names them."""
    src = tmp_path / "sensitivity_names.cpp"
    src.write_text(r'''
#include "ilqr_amd.hpp"
void f(ilqr_amd::iLQR& s, ilqr_amd::BatchILQR& b, void* dev) {
  ilqr_amd::MatrixXd dx0(4, 3), g_x0; ilqr_amd::VecOfMatXd dv, dxs, dus, gx, gu, g_v;
  s.tangent(dx0, dv, dxs); s.tangent(dx0, dv, dxs, &dus); s.tangent(dx0, dv, dxs, &dus, 2, 3);
  s.adjoint(gx, gu, g_x0); s.adjoint(gx, gu, g_x0, &g_v); s.adjoint(gx, gu, g_x0, &g_v, 2, 3);
  std::vector<double> a, c, d, e;
  b.tangent(3, &a, &c, &d, &e); b.tangent(3, &a, nullptr, &d, nullptr, 2, 3);
  b.adjoint(3, &a, &c, &d, &e); b.adjoint(3, nullptr, &c, &d, nullptr, 2, 3);
  b.copy_tangent_to_device(0, 1, 3, dev, nullptr, dev, nullptr);
  b.copy_adjoint_to_device(0, 1, 3, dev, nullptr, dev, nullptr);
}
''')
    for extra in (["-DILQR_AMD_NO_EIGEN"], []):  # (without the macro: Eigen's types where Eigen is installed, the stand-ins elsewhere)
        subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall"] + extra + ["-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "sensitivity_names.o")])
