"""CPU-side checks of the parameter-gradient entry points (ilqr_get_param_gradient, ilqr_param_gradient_on_device): declared, exported,
bound, every argument refusal that needs no handle, the null handle -- and the yardstick of tests/test_gpu_param_gradient.py itself
(pg_reference, costate) against things written independently of it: the parameters whose derivative is known in closed form (the damping,
the control weight, the final scale) and, on the oracle's own solves with linear dynamics, central differences over whole re-solves."""
import ctypes as C_
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ilqr_get_param_gradient", "ilqr_param_gradient_on_device")


def test_header_library_and_ctypes_table_carry_the_calls():
    from ilqr_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_amd.h")).read(), flags=re.S)
    lib = capi.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*ilqr_batch\s*\*\s*h\s*,\s*int\s+n_dirs\s*,\s*int\s+flags\s*,\s*double\s+eps_p\s*," % name, src), name
        assert hasattr(lib, name) and name in capi.SYMBOLS
        # handle; n_dirs, flags, eps_p; dxs, dus, dlam; gp, lam
        assert len(capi.SYMBOLS[name][1]) == 9 and capi.SYMBOLS[name][1][1:4] == [C_.c_int, C_.c_int, C_.c_double]
    assert capi.SYMBOLS["ilqr_get_param_gradient"][1][4:] == [C_.POINTER(C_.c_double)] * 5
    assert capi.SYMBOLS["ilqr_param_gradient_on_device"][1][4:] == [C_.c_void_p] * 5
    names = lambda fn: [w.split()[-1].lstrip("*") for w in re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % fn, src).group(1).split(",")]
    assert names("ilqr_get_param_gradient") == ["h", "n_dirs", "flags", "eps_p", "dxs", "dus", "dlam", "gp", "lam"]
    assert names("ilqr_param_gradient_on_device") == ["h", "n_dirs", "flags", "eps_p", "dxs_device", "dus_device", "dlam_device", "gp_device", "lam_device"]
    assert re.search(r"\benum\s+ilqr_param_gradient_flags\b", src)
    assert lib.ilqr_abi_version() == 6  # additive: the ABI number and ilqr_desc stay


def test_argument_refusals_and_the_null_handle():
    """ILQR_ERR_INVALID with its message for every argument check (they need no handle and come first), then for the null handle; the
    refusals that need a handle, hence a device: tests/test_gpu_param_gradient.py."""
    from ilqr_amd import capi
    lib = capi.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C_.POINTER(C_.c_double))
    cases = (((0, 0, 0.0, p, p, p, p, p), b"n_dirs 0 must be >= 1"), ((1, 2, 0.0, p, p, p, p, p), b"unknown flag bits 0x2"),
             ((1, 0, -1.0, p, p, p, p, p), b"eps_p -1 must be finite and >= 0"), ((1, 0, float("nan"), p, p, p, p, p), b"must be finite and >= 0"),
             ((1, 0, float("inf"), p, p, p, p, p), b"must be finite and >= 0"), ((1, 0, 0.0, None, None, None, p, p), b"dxs, dus and dlam are all null"),
             ((1, 0, 0.0, p, None, None, None, None), b"gp and lam are both null"), ((1, 0, 1e-3, p, None, None, p, None), b"null handle"))
    for args, msg in cases:
        assert lib.ilqr_get_param_gradient(None, *args) == -1 and msg in lib.ilqr_last_error(), (args[:3], lib.ilqr_last_error())
        assert b"ilqr_get_param_gradient" in lib.ilqr_last_error() or msg == b"null handle"
        dev = [None if a is None else buf.ctypes.data for a in args[3:]]
        assert lib.ilqr_param_gradient_on_device(None, *args[:3], *dev) == -1 and msg in lib.ilqr_last_error(), (args[:3], lib.ilqr_last_error())


def chain_nominal(oracle, rows, T, dt, seed):
    from tests.test_gpu_param_gradient import NU, costate
    from tests.test_gpu_user_chain import NL, chain_x0
    from tests.util import mat
    B = len(rows)
    rng = np.random.default_rng(seed)
    x0, u0 = chain_x0(B, seed=seed), rng.normal(size=(B, T, NU)) * 0.5
    xs, us, d = [], [], []
    for b in range(B):
        m = oracle.Model("chain", chain=(NL, rows[b]), u_lim=2.0)
        x, u, _ = oracle.batch_rollout(m, x0[b:b + 1], u0[b:b + 1], dt)
        xs.append(x), us.append(u), d.append(oracle.batch_derivatives(m, x, u, dt))
    d = {k: np.concatenate([np.asarray(r[k], dtype=np.float64) for r in d]) for k in d[0]}
    d = {k: (mat(a) if a.ndim == 4 else a) for k, a in d.items()}
    return np.concatenate(xs), np.concatenate(us), d, costate(d)


def test_yardstick_against_closed_forms(oracle):
    """Three parameters of the chain enter linearly, so their column of gp is known without any stencil: the damping (F_omega carries
    -dt damp omega: A_t and B_t both, signs included), the control weight (cost carries wu |u|^2 / 2) and the final scale (knot T alone)."""
    from tests.test_gpu_param_gradient import NTP, draw_params, pg_reference, stencil_case
    from tests.test_gpu_user_chain import DT, NL
    B, T, S = 2, 7, 3
    rows = draw_params(B, 61)
    xs, us, d, lam = chain_nominal(oracle, rows, T, DT, 7)
    dxs, dus, dlam = stencil_case(B, T, S, 23)
    gp, bound = pg_reference(oracle, rows, 2.0, DT, xs, us, lam, dxs, dus, dlam)
    assert gp.shape == (B, S, NTP) and np.all(bound > 0)
    damp = -DT * (np.einsum("bti,btsi->bs", lam[:, 1:, NL:], dxs[:, :T, :, NL:]) + np.einsum("btsi,bti->bs", dlam[:, 1:, :, NL:], xs[:, :T, NL:]))
    wu = np.einsum("bti,btsi->bs", us, dus)
    wf = np.einsum("bi,bsi->bs", d["cx"][:, T], dxs[:, T]) / rows[:, 6:7]  # cx[T] = grad final_cost = wf grad state_cost (central differences)
    # damp, wu: the stencil is exact (linear), what is left is its rounding, about u |Psi| n / (4 eps h) per knot; wf: cx[T]'s own truncation
    for j, want, tol in ((1, damp, 1e-6), (5, wu, 1e-6), (6, wf, 1e-5)):
        gap = np.abs(gp[:, :, j] - want).max() / np.abs(want).max()
        print("  gp[:, :, %d] against its closed form: %.3g relative (bound %.3g)" % (j, gap, bound[:, :, j].max() / np.abs(want).max()))
        assert gap <= tol and np.abs(want).max() > 1e-3, (j, gap)


def test_yardstick_end_to_end_with_linear_dynamics(oracle):
    """The GPU end-to-end test with the oracle in the device's place: 33 solves of the chain at g/l = 0, the yardsticks of ilqr_solve_lq and
    of this call, and central differences over the re-solves under the GPU test's own requirement."""
    from tests.test_gpu_lq_solve import lq_reference
    from tests.test_gpu_param_gradient import NTP, NU, NX, costate, pg_reference
    from tests.test_gpu_user_chain import NL
    from tests.util import mat
    T, dt, lim = 20, 0.02, 50.0
    p0 = np.array([0.0, 0.1, 2.0, 10.0, 1.0, 0.1, 50.0, 0.3])
    delta = 1e-3 * np.maximum(1.0, np.abs(p0))
    rows = [p0]
    for j in range(NTP):
        for step in (delta[j], -delta[j], delta[j] / 2, -delta[j] / 2):
            rows.append(p0.copy())
            rows[-1][j] += step
    rng = np.random.default_rng(0)
    x0 = np.concatenate([rng.uniform(-1, 1, (1, NL)), rng.uniform(-1, 1, (1, NL)) * 0.5], axis=1)
    u0 = 0.3 * rng.normal(size=(1, T, NU))
    w, v = rng.normal(size=(T + 1, NX)), rng.normal(size=(T, NU))
    oracle.set_params(tol_fun=1e-14, tol_grad=1e-12)
    try:
        sols = [oracle.batch_solve(oracle.Model("chain", chain=(NL, r), u_lim=lim), x0, u0, dt, max_iters=400) for r in rows]
    finally:
        oracle.set_params()
    L = np.array([float(np.sum(w * s["xs"][0]) + np.sum(v * s["us"][0])) for s in sols])
    xs, us = np.asarray(sols[0]["xs"], dtype=np.float64), np.asarray(sols[0]["us"], dtype=np.float64)
    assert np.abs(us).max() < lim
    d = oracle.batch_derivatives(oracle.Model("chain", chain=(NL, p0), u_lim=lim), xs, us, dt)
    d = {k: (mat(np.asarray(a, dtype=np.float64)) if a.ndim == 4 else np.asarray(a, dtype=np.float64)) for k, a in d.items()}
    lam = costate(d)
    station = np.abs(d["cu"][0, :T] + np.einsum("trc,tr->tc", d["fu"][0, :T], lam[0, 1:])).max()
    dxs, dus, dlam, info = lq_reference(d, np.ones((1, T, NU, NX)), gx=w[None, :, None], gu=v[None, :, None], hold=False)
    assert not info.any() and station <= 1e-6, station
    gp, _ = pg_reference(oracle, p0[None], lim, dt, xs, us, lam, dxs, dus, dlam)
    fd1 = np.array([(L[1 + 4 * j] - L[2 + 4 * j]) / (2 * delta[j]) for j in range(NTP)])
    fd2 = np.array([(L[3 + 4 * j] - L[4 + 4 * j]) / delta[j] for j in range(NTP)])
    lhs, rhs = np.abs(gp[0, 0] - fd2), 10 * np.abs(fd1 - fd2) + 1e-4 * np.maximum(1.0, np.abs(fd2))
    print("  stationarity %.2e; worst |gp - fd| / allowed %.3f; worst relative %.2e" % (station, (lhs / rhs).max(), (lhs / np.maximum(1.0, np.abs(fd2))).max()))
    assert np.all(lhs <= rhs), (gp[0, 0], fd2, fd1)


def test_facade_param_gradient_caller_compiles(tmp_path):
    """The facade's members compile without a device: a translation unit that only names them."""
    src = tmp_path / "pg_names.cpp"
    src.write_text(r'''
#include "ilqr_amd.hpp"
void f(ilqr_amd::BatchILQR& b, void* dev) {
  std::vector<double> dxs, dus, dlam, lam;
  std::vector<double> gp = b.param_gradient(2, &dxs, &dus, &dlam);
  gp = b.param_gradient(1, nullptr, nullptr, &dlam, &lam, 1e-4);
  b.param_gradient_on_device(2, ILQR_PARAM_GRADIENT_NO_FLAGS, 0.0, dev, dev, nullptr, dev, nullptr);
}
''')
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-DILQR_AMD_NO_EIGEN", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "pg_names.o")])
