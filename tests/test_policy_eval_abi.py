"""CPU-side checks of the policy-evaluation entry points (ilqr_evaluate_policy, ilqr_evaluate_policy_on_device): declared, exported,
bound, refusing a null handle without a device, the facade's members -- and the yardstick of tests/test_gpu_policy_eval.py itself:
policy_reference() in float64 agrees with the same call in the oracle's f80 flavour within 1e-10 on every fp64 handle kind, with and
without the clamp (a factor 10 inside the bound the device is held to); the clamp case is not vacuous; windows compose on the oracle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_gpu_policy_eval import (B, DT, KINDS64, T, WINDOWS, draw_samples, initial_controls, kind_problem, oracle_model, policy_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_SYMBOLS = ("ilqr_evaluate_policy", "ilqr_evaluate_policy_on_device")
HEADROOM = 1e-10


def test_header_library_and_ctypes_table_carry_the_calls():
    from ilqr_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_amd.h")).read(), flags=re.S)
    lib = capi.load()
    for name in EVAL_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*ilqr_batch\s*\*\s*h\s*,\s*int\s+t0\s*,\s*int\s+n_knots\s*,\s*int\s+n_samples\s*,\s*int\s+flags\s*," % name, src), name
        assert hasattr(lib, name) and name in capi.SYMBOLS
        assert capi.SYMBOLS[name][1][1:5] == [C.c_int] * 4 and len(capi.SYMBOLS[name][1]) == 9
    assert re.search(r"\bILQR_EVAL_CLAMP\s*=\s*1\b", src) and capi.EVAL_CLAMP == 1
    assert lib.ilqr_abi_version() == 6  # additive: the ABI number and ilqr_desc stay


def test_null_handle_is_refused():
    from ilqr_amd import capi
    lib = capi.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ilqr_evaluate_policy(None, 0, 1, 1, 0, p, p, p, p) == -1 and b"null handle" in lib.ilqr_last_error()
    assert lib.ilqr_evaluate_policy_on_device(None, 0, 1, 1, 0, buf.ctypes.data, buf.ctypes.data, None, None) == -1
    assert b"null handle" in lib.ilqr_last_error()


def test_facade_policy_caller_compiles(tmp_path):
    """The facade's members compile without a device: a translation unit that only names them."""
    src = tmp_path / "policy_names.cpp"
    src.write_text(r'''
#include "ilqr_amd.hpp"
void f(ilqr_amd::iLQR& s, ilqr_amd::BatchILQR& b, void* dev, const ilqr_amd::VectorXd& x) {
  ilqr_amd::VectorXd u = s.feedback_control(3, x);
  std::vector<double> xs, cost, x_end, u_first;
  b.evaluate_policy(xs, 4, &cost, &x_end, &u_first);
  b.evaluate_policy(xs, 1, nullptr, nullptr, &u_first, 2, 1, ILQR_EVAL_CLAMP);
  b.evaluate_policy_on_device(0, 1, 4, dev, nullptr, dev, nullptr);
  b.evaluate_policy_on_device(0, 1, 4, dev, dev, dev, dev, ILQR_EVAL_CLAMP);
}
''')
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-DILQR_AMD_NO_EIGEN", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "policy_names.o")])


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_policies(oracle):
    """per fp64 kind: the oracle's model and the policy of init_traj + three iterations, solved by the oracle itself (no device here)"""
    cache = {}

    def get(kind):
        if kind not in cache:
            _, x0, nu = kind_problem(kind)
            om = oracle_model(oracle, kind)
            r = oracle.batch_solve(om, x0, initial_controls(nu), DT, max_iters=3)
            cache[kind] = (om, r["xs"], r["us"], r["K"])
        return cache[kind]
    return get


def rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    d = np.abs(a - b).reshape(a.shape[0], -1).max(axis=1)
    s = np.abs(b).reshape(b.shape[0], -1).max(axis=1)
    return float(np.max(d / np.maximum(s, 1e-300)))


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("kind", KINDS64)
def test_the_yardstick_has_its_headroom(oracle, cpu_policies, kind, clamp):
    om, xs, us, K = cpu_policies(kind)
    worst = 0.0
    try:
        oracle.set_fixes(1 if clamp else 0)
        with oracle.flavour("f80"):
            om80 = om.twin("f80")
        for S, t0, n in [(S, t0, n) for S in (1, 3) for t0, n in WINDOWS] + [(70, 0, T), (70, 7, T - 7), (70, 7, 1)]:
            x = draw_samples(xs, t0, S)
            got = policy_reference(oracle, om, xs, us, K, x, t0, n)
            with oracle.flavour("f80"):
                want = policy_reference(oracle, om80, xs, us, K, x, t0, n)
            assert np.all(np.isfinite(got[0]))
            for key, a, b in zip(("cost", "x_end"), got, want):
                err = rel(a, b)
                worst = max(worst, err)
                assert err < HEADROOM, (kind, clamp, S, t0, n, key, err)
    finally:
        oracle.set_fixes(0)
    print("%s clamp=%d: f64 against f80 %.2e" % (kind, clamp, worst))


def test_the_clamp_case_is_not_vacuous(oracle, cpu_policies):
    om, xs, us, K = cpu_policies("acrobot_f64")
    x = draw_samples(xs, 0, 3)
    free = policy_reference(oracle, om, xs, us, K, x, 0, T)[0]
    try:
        oracle.set_fixes(1)
        clamped = policy_reference(oracle, om, xs, us, K, x, 0, T)[0]
    finally:
        oracle.set_fixes(0)
    share = float(np.mean(free != clamped))
    print("the clamp changes the cost of %.0f %% of the rollouts" % (100 * share))
    assert share >= 0.5


@pytest.mark.parametrize("kind", KINDS64)
def test_windows_compose_on_the_oracle(oracle, cpu_policies, kind):
    """a full rollout's tail equals the window rollout started from its own xs[t0], bit for bit on x_end"""
    om, xs, us, K = cpu_policies(kind)
    x = draw_samples(xs, 0, 3)
    xs_full, _, _ = oracle.batch_rollout(om, x.reshape(B * 3, -1), np.repeat(us, 3, axis=0), DT, xs_nom=np.repeat(xs, 3, axis=0), K=np.repeat(K, 3, axis=0))
    whole = policy_reference(oracle, om, xs, us, K, x, 0, T)
    assert np.array_equal(whole[1].reshape(B * 3, -1), xs_full[:, T])
    for t0 in (7, T - 1):
        tail = policy_reference(oracle, om, xs, us, K, xs_full[:, t0].reshape(B, 3, -1), t0, T - t0)
        assert np.array_equal(tail[1], whole[1]), (kind, t0)
