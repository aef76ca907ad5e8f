"""CPU-side checks of per-knot model parameters (ilqr_set_knot_params, ilqr_get_knot_params): declared, bound, carried by BatchILQR and the
facade; the refusals that need no handle, in the order the header states, then the null handle; the window's clamp at the reference's
end; and the CPU reference of tests/test_gpu_knot_params.py itself (tests/knot_params.py) proven against the oracle's own batch functions:
with every knot's row equal to the trajectory's row it must reproduce oracle.batch_rollout and oracle.batch_derivatives."""
import ctypes as C_
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_ctypes_table_and_wrappers_carry_the_calls():
    from ilqr_amd import BatchILQR, capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_amd.h")).read(), flags=re.S)
    names = lambda fn: [w.split()[-1].lstrip("*") for w in re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % fn, src).group(1).split(",")]
    assert names("ilqr_set_knot_params") == ["h", "p", "p_device", "n", "n_knots", "k0"]
    assert names("ilqr_get_knot_params") == ["h", "p", "n"]
    dp = C_.POINTER(C_.c_double)
    assert capi.SYMBOLS["ilqr_set_knot_params"][1][1:] == [dp, C_.c_void_p, C_.c_int, C_.c_int, C_.c_int]
    assert capi.SYMBOLS["ilqr_get_knot_params"][1][1:] == [dp, C_.c_int]
    lib = capi.load()
    assert hasattr(lib, "ilqr_set_knot_params") and hasattr(lib, "ilqr_get_knot_params")
    assert callable(BatchILQR.set_knot_params) and callable(BatchILQR.knot_params)
    assert lib.ilqr_abi_version() == 6  # additive: the ABI number and ilqr_desc stay


def test_handle_free_refusals_come_first_and_in_order():
    """ILQR_ERR_INVALID for not exactly one pointer, n_knots < 1, k0 outside [0, n_knots) -- in that order, each winning over the ones
    behind it --, and only then the null handle."""
    from ilqr_amd import capi
    lib = capi.load()
    buf = np.zeros(64)
    p, d = buf.ctypes.data_as(C_.POINTER(C_.c_double)), buf.ctypes.data
    #        p     p_device  n  n_knots  k0
    cases = (((None, None, 8, 0, -1), b"exactly one of p (host) and p_device"),
             ((p, d, 8, 0, -1), b"exactly one of p (host) and p_device"),
             ((p, None, 8, 0, -1), b"n_knots 0 must be >= 1"),
             ((None, d, 8, -3, 0), b"n_knots -3 must be >= 1"),
             ((p, None, 8, 4, -1), b"k0 -1 outside [0, n_knots = 4)"),
             ((p, None, 8, 4, 4), b"k0 4 outside [0, n_knots = 4)"),
             ((p, None, 8, 4, 3), b"null handle"),
             ((None, d, 5, 1, 0), b"null handle"))
    for args, msg in cases:
        assert lib.ilqr_set_knot_params(None, *args) == -1 and msg in lib.ilqr_last_error(), (args[2:], lib.ilqr_last_error())
        assert b"ilqr_set_knot_params" in lib.ilqr_last_error() or msg == b"null handle"
    assert lib.ilqr_get_knot_params(None, p, 8) == -1 and b"null handle" in lib.ilqr_last_error()


def test_the_window_clamps_at_the_references_end():
    from tests.knot_params import knot_window
    B, L, n, T = 2, 5, 3, 6
    ref = np.arange(B * L * n, dtype=np.float64).reshape(B, L, n)
    w = knot_window(ref, 0, T)
    assert w.shape == (B, T + 1, n) and np.array_equal(w[:, :L], ref) and np.all(w[:, L:] == ref[:, -1:])
    w = knot_window(ref, 3, T)
    assert np.array_equal(w[:, :2], ref[:, 3:]) and np.all(w[:, 2:] == ref[:, -1:])
    w = knot_window(ref, L - 1, T)  # the last row alone: all rows equal
    assert np.all(w == ref[:, -1:])
    long = np.arange(B * 20 * n, dtype=np.float64).reshape(B, 20, n)
    assert np.array_equal(knot_window(long, 4, T), long[:, 4:4 + T + 1])  # a reference that does not end inside the horizon: a plain slice


def test_the_cpu_reference_reproduces_the_oracle_when_all_rows_are_equal(oracle):
    """knot_rollout against oracle.batch_rollout (1e-14 relative; open loop, and closed loop around a nominal with gains), knot_records
    against oracle.batch_derivatives (exactly): the pendulum chain, B = 3, T = 6, one row per trajectory repeated over the knots."""
    from tests.knot_params import knot_records, knot_rollout, knot_twins
    from tests.test_gpu_user_chain import DT, NL, PARAMS, chain_x0
    from tests.util import relerr
    B, T, lim = 3, 6, 2.0
    NX, NU = 2 * NL, NL // 2
    rng = np.random.default_rng(5)
    rows = PARAMS[None, :] * (1.0 + rng.uniform(-0.2, 0.2, (B, 8)))
    rows[:, 7] = rng.uniform(-1.0, 1.0, B)
    tw = knot_twins(oracle, np.repeat(rows[:, None], T + 1, axis=1), lim)
    oms = [oracle.Model("chain", chain=(NL, rows[b]), u_lim=lim) for b in range(B)]
    x0, u0 = chain_x0(B, seed=11), rng.normal(size=(B, T, NU)) * 0.5
    ref = [oracle.batch_rollout(oms[b], x0[b:b + 1], u0[b:b + 1], DT) for b in range(B)]
    xs_o, us_o, c_o = (np.concatenate([r[i] for r in ref]) for i in range(3))
    xs, us, c = knot_rollout(tw, x0, u0, DT)
    print("open loop: xs %.2e cost %.2e" % (relerr(xs, xs_o), np.max(np.abs(c - c_o) / np.abs(c_o))))
    assert relerr(xs, xs_o) < 1e-14 and np.array_equal(us, u0) and np.max(np.abs(c - c_o) / np.abs(c_o)) < 1e-14
    # closed loop: the nominal above, random gains, another start
    K = rng.normal(size=(B, T, NU, NX)) * 0.2
    x1 = x0 + 0.05 * rng.normal(size=x0.shape)
    ref = [oracle.batch_rollout(oms[b], x1[b:b + 1], u0[b:b + 1], DT, xs_nom=xs_o[b:b + 1], K=K[b:b + 1]) for b in range(B)]
    xs_c, us_c, c_c = (np.concatenate([r[i] for r in ref]) for i in range(3))
    xs2, us2, c2 = knot_rollout(tw, x1, u0, DT, xs_nom=xs_o, K=K)
    print("closed loop: xs %.2e us %.2e cost %.2e" % (relerr(xs2, xs_c), relerr(us2, us_c), np.max(np.abs(c2 - c_c) / np.abs(c_c))))
    assert relerr(xs2, xs_c) < 1e-14 and relerr(us2, us_c) < 1e-14 and np.max(np.abs(c2 - c_c) / np.abs(c_c)) < 1e-14
    assert relerr(us2, u0) > 1e-3  # (the feedback did something)
    # a window of the same rollout: knots 2 .. 4 from the state at knot 2, no final cost
    xs3, us3, c3 = knot_rollout(tw, xs2[:, 2], u0, DT, xs_nom=xs_o, K=K, t0=2, n=3)
    assert np.array_equal(xs3, xs2[:, 2:6]) and np.array_equal(us3, us2[:, 2:5]) and np.all(c3 < c2)
    # records
    d = knot_records(tw, xs_o, us_o, DT)
    for b in range(B):
        do = oracle.batch_derivatives(oms[b], xs_o[b:b + 1], us_o[b:b + 1], DT)
        for key in do:
            assert d[key].shape[1:] == do[key].shape[1:] and np.array_equal(d[key][b], do[key][0]), (b, key)
    assert np.abs(d["cxx"]).max() > 1.0 and np.abs(d["cx"][:, T]).max() > 0.0


def test_facade_knot_params_caller_compiles(tmp_path):
    """The facade's members compile without a device: a translation unit that only names them."""
    src = tmp_path / "knot_names.cpp"
    src.write_text(r'''
#include "ilqr_amd.hpp"
void f(ilqr_amd::BatchILQR& b, const void* dev) {
  std::vector<double> ref;
  b.set_knot_params(ref, 12, 3);
  b.set_knot_params(dev, 400);
  std::vector<double> w = b.knot_params();
}
''')
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-DILQR_AMD_NO_EIGEN", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "knot_names.o")])
