"""CPU-side checks of the estimator entry points (ilqr_get_estimator, ilqr_copy_estimator_to_device): declared, exported, bound,
refusing a null handle without a device -- and the yardstick of tests/test_gpu_estimator.py itself: the two n x n recursions of the
definition (Sigma = Xh + Pf) agree with an independently written joint recursion on z = [x - xs; xhat_prior - xs] (2n x 2n), the
float64 recursion agrees with np.longdouble on the GPU tests' inputs, and a scalar problem by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EST_SYMBOLS = ("ilqr_get_estimator", "ilqr_copy_estimator_to_device")


def test_header_library_and_ctypes_table_carry_the_calls():
    from ilqr_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_amd.h")).read(), flags=re.S)
    lib = capi.load()
    for name in EST_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*ilqr_batch\s*\*\s*h\s*,\s*int\s+t0\s*,\s*int\s+n_knots\s*,\s*int\s+ny\s*," % name, src), name
        assert hasattr(lib, name) and name in capi.SYMBOLS
        # handle, window, ny; H, P0, W, V; Pp, Pf, L, Sigma, Su, expected_cost; info
        assert len(capi.SYMBOLS[name][1]) == 15 and capi.SYMBOLS[name][1][1:4] == [C.c_int, C.c_int, C.c_int]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert capi.SYMBOLS["ilqr_get_estimator"][1][4:] == [dp] * 10 + [ip]
    assert capi.SYMBOLS["ilqr_copy_estimator_to_device"][1][4:] == [C.c_void_p] * 11
    decl = re.search(r"int\s+ilqr_get_estimator\s*\(([^;]*)\)\s*;", src).group(1)
    assert [w.split()[-1].lstrip("*") for w in decl.split(",")] == ["h", "t0", "n_knots", "ny", "H", "P0", "W", "V", "Pp", "Pf", "L", "Sigma", "Su",
                                                                    "expected_cost", "info"]
    assert lib.ilqr_abi_version() == 6  # additive: the ABI number and ilqr_desc stay


def test_null_handle_is_refused():
    """ILQR_ERR_INVALID before anything else is looked at (the other refusals need a handle, hence a device: tests/test_gpu_estimator.py)."""
    from ilqr_amd import capi
    lib = capi.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ilqr_get_estimator(None, 0, 1, 1, p, p, p, p, p, p, p, None, None, None, None) == -1 and b"null handle" in lib.ilqr_last_error()
    assert lib.ilqr_copy_estimator_to_device(None, 0, 1, 1, buf.ctypes.data, None, None, buf.ctypes.data, None, buf.ctypes.data, None, None, None, None,
                                             None) == -1
    assert b"null handle" in lib.ilqr_last_error()


def joint_recursion(d, K, H, P0, W, V, L):
    """The loop u = us + K (xhat - xs) written out on z = [dx; xp], dx = x - xs and xp the estimate BEFORE the knot's measurement, with the
    gains L given: xf = xp + L (H dx + v - H xp) = F z + L v, F = [L H, I - L H]; dx+ = fx dx + fu K xf + w; xp+ = (fx + fu K) xf.
    Nothing here uses the orthogonality of the optimal filter's error.  Returns Sigma = cov(dx), Su = cov(K xf), J."""
    from tests.test_gpu_estimator import NAMES, tr
    fx, fu, cx, cu, cxx, cxu, cuu = (np.asarray(d[name]) for name in NAMES)
    B, T1, n = cx.shape
    T, m = T1 - 1, K.shape[2]
    dot = lambda X, Y: (X * Y).sum(axis=(-1, -2))
    C2 = np.zeros((B, 2 * n, 2 * n))
    C2[:, :n, :n] = P0
    Sigma, Su, J = np.zeros((B, T1, n, n)), np.zeros((B, T, m, m)), np.zeros(B)
    for t in range(T1):
        F = np.concatenate([L[:, t] @ H, np.eye(n) - L[:, t] @ H], axis=2)  # [B][n][2n]
        Sigma[:, t] = C2[:, :n, :n]
        J += dot(cxx[:, t], Sigma[:, t]) / 2
        if t == T:
            break
        Kt = K[:, t]
        cov_xf = F @ C2 @ tr(F) + L[:, t] @ V @ tr(L[:, t])
        Su[:, t] = Kt @ cov_xf @ tr(Kt)
        E_dx_du = C2[:, :n] @ tr(F) @ tr(Kt)  # E[dx du'] (v is independent of dx)
        J += dot(cuu[:, t], Su[:, t]) / 2 + dot(cxu[:, t], E_dx_du)
        A = fx[:, t] + fu[:, t] @ Kt
        M = np.concatenate([np.concatenate([fx[:, t], np.zeros((B, n, n))], axis=2) + fu[:, t] @ Kt @ F, A @ F], axis=1)  # z+ = M z + Bv v + [w; 0]
        Bv = np.concatenate([fu[:, t] @ Kt @ L[:, t], A @ L[:, t]], axis=1)
        C2 = M @ C2 @ tr(M) + Bv @ V @ tr(Bv)
        C2[:, :n, :n] += W
    return Sigma, Su, J


@pytest.mark.parametrize("n,m,ny", [(4, 1, 2), (17, 3, 5), (32, 16, 32)])
def test_the_definition_is_the_joint_covariance(n, m, ny):
    """Sigma, Su and J of the two n x n recursions against the 2n x 2n joint recursion (with the reference's L[t])."""
    from tests.test_gpu_estimator import estimator_inputs, estimator_reference, random_policy
    d, _, K = random_policy(n, m, B=2, T=7)
    H, P0, W, V = estimator_inputs(n, ny, B=2)
    ref = estimator_reference(d, K, H, P0, W, V)
    assert not ref["info"].any()
    for a, b, what in zip(joint_recursion(d, K, H, P0, W, V, ref["L"]), (ref["Sigma"], ref["Su"], ref["expected_cost"]), ("Sigma", "Su", "J")):
        gap, scale = float(np.abs(a - b).max()), max(1.0, float(np.abs(b).max()))
        print("  two n x n recursions vs the joint recursion, %s: %.3g (scale %.3g)" % (what, gap, scale))
        assert gap <= 1e-12 * scale, (what, gap, scale)
    # each input matters, and the gains matter to the loop alone
    other = estimator_reference(d, np.zeros_like(K), H, P0, W, V)
    assert np.array_equal(other["L"], ref["L"]) and np.array_equal(other["Pf"], ref["Pf"]) and np.abs(other["Sigma"] - ref["Sigma"]).max() > 1e-4
    for change in (dict(P0=None), dict(W=None), dict(V=2 * V), dict(H=-0.5 * H)):
        args = dict(H=H, P0=P0, W=W, V=V)
        args.update(change)
        assert np.abs(estimator_reference(d, K, **args)["Pf"] - ref["Pf"]).max() > 1e-4, list(change)


@pytest.mark.parametrize("n,m,ny", [(32, 16, 1), (32, 16, 17), (20, 5, 5), (8, 3, 8), (17, 17, 17), (6, 1, 6), (4, 2, 4)])
def test_the_yardstick_has_its_headroom(n, m, ny):
    """On the GPU tests' inputs: float64 and np.longdouble within 1e-10 x scale, every pivot above the floor (asserted inside), and the
    filter does what a filter does -- the measurement never adds uncertainty, and Sigma = Xh + Pf is at least Pf."""
    from tests.test_gpu_estimator import generic_case
    ref = generic_case(n, m, ny)[-1]
    eig = np.linalg.eigvalsh
    assert eig(ref["Pp"] - ref["Pf"]).min() > -1e-12 and eig(ref["Sigma"] - ref["Pf"]).min() > -1e-12 and eig(ref["Pf"]).min() > -1e-12
    assert 1e-3 < np.abs(ref["Sigma"]).max() < 100.0 and np.abs(ref["Su"]).max() > 1e-4 and np.all(np.isfinite(ref["expected_cost"]))


def test_yardstick_on_a_scalar_problem():
    """n = m = ny = 1, T = 1, by hand."""
    from tests.test_gpu_estimator import estimator_reference
    fx, fu, cxx, cxu, cuu, K, p0, w, v, h, cxxT = 0.9, 0.5, 2.0, 0.1, 1.5, -0.7, 0.8, 0.05, 0.3, 1.2, 3.0
    d = {name: np.zeros((1, 2, 1, 1)) for name in ("fx", "fu", "cxx", "cxu", "cuu")}
    d.update(cx=np.zeros((1, 2, 1)), cu=np.zeros((1, 2, 1)))
    for name, val in (("fx", fx), ("fu", fu), ("cxx", cxx), ("cxu", cxu), ("cuu", cuu)):
        d[name][0, 0, 0, 0] = val
    d["cxx"][0, 1, 0, 0] = cxxT
    one = lambda x: np.array([[[x]]])
    r = estimator_reference(d, np.array([[[[K]]]]), one(h), one(p0), one(w), one(v))
    s0 = h * p0 * h + v
    l0 = p0 * h / s0
    pf0 = p0 - l0 * h * p0  # (the Joseph form of the optimal gain)
    xh0 = l0 * s0 * l0
    pp1 = fx * pf0 * fx + w
    s1 = h * pp1 * h + v
    l1 = pp1 * h / s1
    pf1 = pp1 - l1 * h * pp1
    a = fx + fu * K
    xh1 = a * xh0 * a + l1 * s1 * l1
    near = lambda x, y: abs(x - y) < 1e-14
    assert r["Pp"][0, 0, 0, 0] == p0 and near(r["L"][0, 0, 0, 0], l0) and near(r["Pf"][0, 0, 0, 0], pf0) and near(r["Pp"][0, 1, 0, 0], pp1)
    assert near(r["L"][0, 1, 0, 0], l1) and near(r["Pf"][0, 1, 0, 0], pf1) and near(r["Sigma"][0, 0, 0, 0], xh0 + pf0)
    assert near(r["Sigma"][0, 1, 0, 0], xh1 + pf1) and near(r["Su"][0, 0, 0, 0], K * K * xh0)
    assert near(r["expected_cost"][0], 0.5 * (cxx * (xh0 + pf0) + cuu * K * K * xh0 + 2 * cxu * xh0 * K) + 0.5 * cxxT * (xh1 + pf1))
    # a pivot that is not positive ends the trajectory at that knot
    bad = estimator_reference(d, np.array([[[[K]]]]), one(h), one(p0), one(w), one(-2.0))
    assert bad["info"][0] == 1 and np.isnan(bad["Pf"]).all() and np.isnan(bad["expected_cost"]).all()


def test_facade_estimator_caller_compiles(tmp_path):
    """The facade's members compile without a device: a translation unit that only names them."""
    src = tmp_path / "estimator_names.cpp"
    src.write_text(r'''
#include "ilqr_amd.hpp"
void f(ilqr_amd::BatchILQR& b, void* dev) {
  std::vector<double> H, P0, W, V, Pp, Pf, L, Sg, Su, J; std::vector<int> info;
  b.estimator(2, H, &P0, &W, V, &Pp, &Pf, &L);
  b.estimator(2, H, nullptr, nullptr, V, nullptr, nullptr, nullptr, &Sg, &Su, &J, &info, 1, 3);
  b.copy_estimator_to_device(0, 1, 2, dev, nullptr, nullptr, dev, nullptr, dev, dev, nullptr, nullptr, nullptr, dev);
}
''')
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-DILQR_AMD_NO_EIGEN", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "estimator_names.o")])
