"""Receding-horizon steps on the device (ABI 6: ilqr_shift_horizon, ilqr_mpc_step, ilqr_copy_controls_to_device).

- the in-place shift of every layout and storage type equals the numpy shift of include/ilqr_amd.h's table, bit for bit;
- mpc_step equals its host composition (shift on the host, set_trajectory + set_gains + set_lambda, warm start with max_iter = n) bit for
  bit, on a handle that has just solved and on a fresh one, on every kind of route;
- a device x0 gives the bits of a host x0, the control window equals a slice of the getter;
- the new nominal is the oracle's closed-loop rollout around the shifted nominal, step after step;
- what is refused, and the C++ facade's loop."""
import os
import subprocess

import numpy as np
import pytest

from tests.util import TOL, acrobot_x0, integrator_x0, relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.02
B, T = 37, 45  # B: not a multiple of 16 or 64 (partial tiles, padding lanes); T: not a multiple of 8
ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5


def np_shift(xs, us, k, K, s, tail):
    """include/ilqr_amd.h, enum ilqr_tail: knots s later; the tail holds the last knot (xs always, us / K under hold) or is zero."""
    Tn = us.shape[1]
    xs2, us2, k2, K2 = (np.zeros_like(a) for a in (xs, us, k, K))
    xs2[:, :Tn + 1 - s] = xs[:, s:]
    xs2[:, Tn + 1 - s:] = xs[:, Tn:]
    for src, dst, hold in ((us, us2, tail == "hold"), (k, k2, False), (K, K2, tail == "hold")):
        dst[:, :Tn - s] = src[:, s:]
        if hold:
            dst[:, Tn - s:] = src[:, Tn - 1:]
    return xs2, us2, k2, K2


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """x0 and control windows live in torch tensors here: torch's device is initialised before this module creates any handle (a torch
    initialised after the library had set up the device reports no GPU: tests/test_gpu_generic_fp32.py)."""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


@pytest.fixture(scope="module")
def chain_lib():
    from ilqr_amd import _build
    if not os.path.exists(_build.USER_CHAIN_LIB) and not os.path.exists(_build.HIPCC):
        pytest.skip("the pendulum-chain build is missing and there is no hipcc to make it")
    return _build.build_user(_build.USER_CHAIN_HEADER, _build.USER_CHAIN_LIB)


def lq_mats(n, m):
    from tests.test_gpu_lq_end_to_end import dense_mats
    return dense_mats(n, m)


CHAIN_PARAMS = np.array([9.81, 0.1, 2.0, 10.0, 1.0, 0.1, 50.0, 0.0])


def problem(name, chain_lib=None):
    """(constructor kwargs, x0 [B][nx], nu) of a named handle"""
    rng = np.random.default_rng(5)
    if name.startswith("acrobot"):
        return dict(model="acrobot", u_min=-1.5, u_max=1.5), acrobot_x0(B, scale=0.3, seed=4), 1
    if name.startswith("integrator"):
        return dict(model="integrator", goal=[1, .5, 0, 0]), integrator_x0(B), 2
    if name.startswith("lq20"):
        return dict(model="lq", lq=lq_mats(8, 20), u_min=-0.4, u_max=0.4), rng.uniform(-1, 1, (B, 8)), 20
    if name.startswith("lq"):
        return dict(model="lq", lq=lq_mats(6, 3), u_min=-0.4, u_max=0.4), rng.uniform(-1, 1, (B, 6)), 3
    if name.startswith("chain"):
        x0 = np.concatenate([rng.uniform(-1, 1, (B, 8)), rng.uniform(-1, 1, (B, 8)) * 0.5], axis=1)
        return dict(model="user", lib=chain_lib, nx=16, nu=4, u_min=-2.0, u_max=2.0, user_params=CHAIN_PARAMS), x0, 4
    raise KeyError(name)


def make(kw, **extra):
    from ilqr_amd import BatchILQR
    kw = dict(kw, **extra)
    return BatchILQR(kw.pop("model"), B, T, DT, **kw)


def snapshot(g):
    xs, us = g.trajectory()
    k, K = g.gains()
    lam, dlam = g.lambdas()
    return dict(xs=xs, us=us, k=k, K=K, cost=g.cost(), lam=lam, dlam=dlam)


def assert_same(a, b, keys):
    for key in keys:
        assert np.array_equal(a[key], b[key]), key


# ---- 1. the shift, per layout and storage type ------------------------------------------------------------------------------------------
SHIFT_HANDLES = ["acrobot_f64", "acrobot_f32", "integrator", "lq_f64", "lq_f32", "lq20", "host", "chain"]


@pytest.mark.parametrize("name", SHIFT_HANDLES)
def test_shift_matches_numpy_bit_for_bit(name, chain_lib):
    from ilqr_amd import BatchILQR
    rng = np.random.default_rng(9)
    if name == "host":  # host-evaluated model: the nominal comes from the caller
        nx, nu = 5, 3
        g = BatchILQR("host", B, T, DT, nx=nx, nu=nu, u_min=-1.0, u_max=1.0)
        ref = dict(xs=rng.normal(size=(B, T + 1, nx)), us=rng.normal(size=(B, T, nu)), k=rng.normal(size=(B, T, nu)),
                   K=rng.normal(size=(B, T, nu, nx)), cost=rng.normal(size=B))
        ref["x0"] = ref["xs"][:, 0]
    else:
        kw, x0, nu = problem(name, chain_lib)
        g = make(kw, dtype="f32" if name.endswith("f32") else "f64")
        g.init_traj(x0, 0.1 * rng.standard_normal((B, T, nu)))
        g.iterate(3)
        ref = snapshot(g)
        ref["x0"] = x0
    for s in (0, 1, 5, T - 1):
        for tail in ("hold", "zero"):
            g.set_trajectory(x0=ref["x0"], xs=ref["xs"], us=ref["us"], cost=ref["cost"])
            g.set_gains(k=ref["k"], K=ref["K"])
            lam0 = g.lambdas()
            g.shift_horizon(s, tail)
            got = snapshot(g)
            xs2, us2, k2, K2 = np_shift(ref["xs"], ref["us"], ref["k"], ref["K"], s, tail)
            for key, want in (("xs", xs2), ("us", us2), ("k", k2), ("K", K2)):
                assert np.array_equal(got[key], want), (key, s, tail)
            assert np.array_equal(got["cost"], ref["cost"]) and np.array_equal(got["lam"], lam0[0]) and np.array_equal(got["dlam"], lam0[1])
    g.close()


def test_shift_leaves_status_and_forgets_the_candidates():
    from ilqr_amd import capi
    kw, x0, nu = problem("acrobot")
    g = make(kw)
    g.init_traj(x0, np.zeros((B, T, nu)))
    g.iterate(2)
    g.candidate(0)  # the last line search's rollouts are there ...
    st = g.status()
    g.shift_horizon(3)
    for a, b in zip(st, g.status()):
        assert np.array_equal(a, b)
    with pytest.raises(capi.ILQRError, match="-4"):  # ... and belong to the old horizon afterwards
        g.candidate(0)
    g.close()


# ---- 2. mpc_step == shift on the host + warm start with max_iter = n ------------------------------------------------------------------
ROUTES = {  # name: (problem, extra constructor kwargs, kernel the route must run)
    "acrobot_hex": ("acrobot", dict(), ("solve", "k_solve_hex")),
    "acrobot_quad_chain": ("acrobot", dict(route=256), ("solve", "k_solve_tile")),
    "acrobot_staged": ("acrobot", dict(flags=32), ("backward", "k_sweep_backward")),
    "acrobot_wide": ("acrobot", dict(route=3), ("solve", "k_solve_wide")),
    "acrobot_f32": ("acrobot", dict(dtype="f32"), None),
    "acrobot_fixes": ("acrobot", dict(flags=64), None),
    "integrator": ("integrator", dict(), None),
    "integrator_wide2": ("integrator", dict(route=3), ("solve", "k_solve_wide2")),
    "lq_fd": ("lq", dict(), ("rollout", "k_rollout_lq")),
    "lq_fused": ("lq", dict(flags=16), ("derivatives", "")),
    "lq_f32": ("lq", dict(dtype="f32"), ("rollout", "k_rollout_g")),
    "lq20": ("lq20", dict(), ("backward", "k_backward_w3w")),
    "chain": ("chain", dict(), ("backward", "k_backward_w3")),
}


def _route_kernel(g, stage):
    from ilqr_amd import capi
    return g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index(stage)).decode()


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_mpc_step_equals_the_host_composition(route, chain_lib):
    pname, extra, kernel = ROUTES[route]
    kw, x0, nu = problem(pname, chain_lib)
    rng = np.random.default_rng(17)
    u0 = 0.1 * rng.standard_normal((B, T, nu))
    for n in (0, 3):
        for s in (0, 1, 7):
            H = make(kw, **extra)
            if kernel:
                assert _route_kernel(H, kernel[0]) == kernel[1], route
            H.init_traj(x0, u0)
            H.iterate(4)  # a solved handle: lambda moved, candidates and records of its own
            ref = snapshot(H)
            xs2, us2, k2, K2 = np_shift(ref["xs"], ref["us"], ref["k"], ref["K"], s, "hold")
            x_new = ref["xs"][:, s] + 0.01 * rng.standard_normal(x0.shape)
            # the composition: host shift, upload, ilqr_warm_start on a handle with max_iter = n
            Cm = make(kw, params=dict(max_iter=n), **extra)
            Cm.set_trajectory(xs=xs2, us=us2, cost=ref["cost"])
            Cm.set_gains(k=k2, K=K2)
            Cm.set_lambda(ref["lam"], ref["dlam"])
            Cm.generate_trajectory(x_new)
            want, want_st = snapshot(Cm), Cm.status()
            # (a) on the solved handle itself: whatever hidden state it carries must not show
            H.mpc_step(x0=x_new, shift=s, iters=n)
            assert_same(snapshot(H), want, ("xs", "us", "k", "K", "cost", "lam", "dlam"))
            # (b) on a fresh handle with the same budget: status and iteration counts too
            D = make(kw, params=dict(max_iter=n), **extra)
            D.set_trajectory(x0=x0, xs=ref["xs"], us=ref["us"], cost=ref["cost"])
            D.set_gains(k=ref["k"], K=ref["K"])
            D.set_lambda(ref["lam"], ref["dlam"])
            D.mpc_step(x0=x_new, shift=s, iters=n)
            assert_same(snapshot(D), want, ("xs", "us", "k", "K", "cost", "lam", "dlam"))
            for a, b in zip(D.status()[:2], want_st[:2]):
                assert np.array_equal(a, b), (route, n, s)
            if n == 0:
                assert np.array_equal(D.status()[1], np.zeros(B, dtype=np.int32))
            for g in (H, Cm, D):
                g.close()


# ---- 3. device x0, control window ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["acrobot_f64", "acrobot_f32", "lq_f64", "lq_f32"])
def test_device_x0_and_control_window(name):
    import torch
    kw, x0, nu = problem(name)
    dtype = "f32" if name.endswith("f32") else "f64"
    stream = torch.cuda.Stream()  # (torch's default stream is the null stream: a handle given stream 0 makes its own)
    with torch.cuda.stream(stream):
        _device_x0_and_control_window(kw, x0, nu, dtype, stream)


def _device_x0_and_control_window(kw, x0, nu, dtype, stream):
    import torch
    assert torch.cuda.current_stream().cuda_stream == stream.cuda_stream != 0
    rng = np.random.default_rng(23)
    u0 = 0.1 * rng.standard_normal((B, T, nu))
    gh, gd = make(kw, dtype=dtype), make(kw, dtype=dtype, stream=stream.cuda_stream)
    for g in (gh, gd):
        g.init_traj(x0, u0)
        g.iterate(3)
    for step in range(3):
        x_new = gh.trajectory()[0][:, 1] + 0.01 * rng.standard_normal(x0.shape)
        gh.mpc_step(x0=x_new, shift=1, iters=2)
        xd = torch.from_numpy(x_new).cuda(non_blocking=True)  # on the current stream, which is the handle's: ordered without a synchronisation
        gd.mpc_step(x0_ptr=xd.data_ptr(), shift=1, iters=2)
        win = torch.full((B, 4, nu), np.nan, dtype=torch.float64, device="cuda")
        gd.copy_controls_to_device(step, 4, win.data_ptr())
        stream.synchronize()
        del xd
        a, b = snapshot(gh), snapshot(gd)
        assert_same(a, b, ("xs", "us", "k", "K", "cost", "lam", "dlam"))
        assert np.array_equal(win.cpu().numpy(), b["us"][:, step:step + 4])
    last = torch.full((B, 1, nu), np.nan, dtype=torch.float64, device="cuda")
    gd.copy_controls_to_device(T - 1, 1, last.data_ptr())
    stream.synchronize()
    assert np.array_equal(last.cpu().numpy(), gd.trajectory()[1][:, T - 1:])
    gh.close()
    gd.close()


# ---- 4. the oracle: the new nominal is the closed-loop rollout around the shifted one ---------------------------------------------------
@pytest.mark.parametrize("model", ["integrator", "acrobot", "lq"])
@pytest.mark.parametrize("s,tail", [(1, "hold"), (4, "zero")])
def test_receding_steps_follow_the_oracle(oracle, model, s, tail):
    kw, x0, nu = problem(model)
    om = {"integrator": lambda: oracle.Model("integrator", goal=[1, .5, 0, 0]),
          "acrobot": lambda: oracle.Model("acrobot", u_lim=1.5),
          "lq": lambda: oracle.Model("lq", lq=kw["lq"], u_lim=0.4)}[model]()
    rng = np.random.default_rng(31)
    g = make(kw)
    g.init_traj(x0, np.zeros((B, T, nu)))
    g.iterate(4)
    for step in range(4):
        ref = snapshot(g)
        xs2, us2, k2, K2 = np_shift(ref["xs"], ref["us"], ref["k"], ref["K"], s, tail)
        x_new = ref["xs"][:, s] + 0.02 * rng.standard_normal(x0.shape)
        g.mpc_step(x0=x_new, shift=s, iters=0, tail=tail)
        xs_w, us_w = g.trajectory()
        xs_o, us_o, c_o = oracle.batch_rollout(om, x_new, us2, DT, xs_nom=xs2, K=K2)
        assert np.array_equal(xs_w[:, 0], x_new)
        assert relerr(xs_w, xs_o) < TOL and relerr(us_w, us_o) < TOL, step
        assert np.max(np.abs(g.cost() - c_o) / np.abs(c_o)) < TOL
        assert np.array_equal(g.gains()[0], k2)  # a warm start rolls out, it does not touch the gains
        g.iterate(2)  # new gains around the new nominal for the next step
    g.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_and_call_order_are_refused():
    import torch
    from ilqr_amd import BatchILQR, capi
    kw, x0, nu = problem("acrobot")
    g = make(kw)
    lib, h = g.lib, g.h
    xh = np.ascontiguousarray(x0)
    xp = xh.ctypes.data_as(capi._dp)
    xd = torch.from_numpy(xh).cuda()
    win = torch.zeros((B, T, nu), dtype=torch.float64, device="cuda")
    HOLD = capi.TAIL_HOLD
    # before any trajectory
    assert lib.ilqr_shift_horizon(h, 1, HOLD) == ERR_STATE
    assert lib.ilqr_mpc_step(h, xp, None, 1, HOLD, 1) == ERR_STATE
    assert lib.ilqr_copy_controls_to_device(h, 0, 1, win.data_ptr()) == ERR_STATE
    g.init_traj(x0, np.zeros((B, T, nu)))
    g.iterate(1)
    ref = snapshot(g)
    for shift, tail in ((-1, HOLD), (T, HOLD), (T + 5, HOLD), (1, 2), (1, -1)):
        assert lib.ilqr_shift_horizon(h, shift, tail) == ERR_INVALID, (shift, tail)
        assert lib.ilqr_mpc_step(h, xp, None, shift, tail, 1) == ERR_INVALID, (shift, tail)
    assert lib.ilqr_mpc_step(h, xp, None, 1, HOLD, -1) == ERR_INVALID
    assert lib.ilqr_mpc_step(h, xp, xd.data_ptr(), 1, HOLD, 1) == ERR_INVALID  # both
    assert lib.ilqr_mpc_step(h, None, None, 1, HOLD, 1) == ERR_INVALID           # neither
    for t0, n in ((-1, 1), (0, 0), (0, T + 1), (T - 2, 3), (T, 1)):
        assert lib.ilqr_copy_controls_to_device(h, t0, n, win.data_ptr()) == ERR_INVALID, (t0, n)
    assert lib.ilqr_copy_controls_to_device(h, 0, T, None) == ERR_INVALID
    assert_same(snapshot(g), ref, ("xs", "us", "k", "K", "cost", "lam", "dlam"))  # nothing refused changed anything
    assert lib.ilqr_copy_controls_to_device(h, 0, T, win.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(win.cpu().numpy(), ref["us"])
    g.close()
    hm = BatchILQR("host", B, T, DT, nx=5, nu=3, u_min=-1.0, u_max=1.0)
    rng = np.random.default_rng(2)
    hm.set_trajectory(x0=rng.normal(size=(B, 5)), xs=rng.normal(size=(B, T + 1, 5)), us=rng.normal(size=(B, T, 3)))
    x5 = np.ascontiguousarray(rng.normal(size=(B, 5)))
    assert hm.lib.ilqr_mpc_step(hm.h, x5.ctypes.data_as(capi._dp), None, 1, HOLD, 1) == ERR_UNSUPPORTED
    hm.shift_horizon(1)  # the shift itself serves host-evaluated models
    hm.close()


# ---- 6. the C++ facade ----------------------------------------------------------------------------------------------------------------
CPP = r'''
#include "ilqr_amd.hpp"
#include <hip/hip_runtime_api.h>
#include <cmath>
#include <cstdio>
using namespace ilqr_amd;
class HostOnly : public Model {  // no device twin: the host-model engine
 public:
  HostOnly() { x_dims = 2; u_dims = 1; u_min = VectorXd(1); u_max = VectorXd(1); u_min(0) = -1; u_max(0) = 1; }
  VectorXd dynamics(const VectorXd& x, const VectorXd& u) override { VectorXd d(2); d(0) = x(1); d(1) = u(0); return d; }
  double cost(const VectorXd& x, const VectorXd& u) override { return x(0) * x(0) + x(1) * x(1) + u(0) * u(0); }
  double final_cost(const VectorXd& x) override { return 10 * (x(0) * x(0) + x(1) * x(1)); }
};
int main() {
  const int B = 8, T = 60, n = 4, m = 2;
  VectorXd goal(4); goal(0) = 1; goal(1) = 0.5; goal(2) = 0; goal(3) = 0;
  BatchILQR eng(std::make_shared<DoubleIntegrator>(goal), B, T, 0.05);
  std::vector<double> x0(B * n), u0((size_t)B * T * m, 0.0);
  for (int b = 0; b < B; b++) for (int i = 0; i < n; i++) x0[b * n + i] = (i < 2 ? goal(i) - 0.3 - 0.02 * b * (i + 1) : 0.0);
  eng.init_traj(x0, u0);
  eng.iterate(10);
  auto dist = [&](const std::vector<double>& x) {
    double d = 0;
    for (int b = 0; b < B; b++) for (int i = 0; i < 2; i++) d = std::max(d, std::fabs(x[b * n + i] - goal(i)));
    return d;
  };
  const double d0 = dist(x0);
  double* x_dev = nullptr; double* u_dev = nullptr;
  if (hipMalloc((void**)&x_dev, sizeof(double) * B * n) != hipSuccess || hipMalloc((void**)&u_dev, sizeof(double) * B * m) != hipSuccess) return 3;
  std::vector<double> x = x0;
  for (int step = 0; step < 10; step++) {
    const std::vector<double> xs = eng.states();
    for (int b = 0; b < B; b++) for (int i = 0; i < n; i++) x[b * n + i] = xs[((size_t)b * (T + 1) + 1) * n + i];  // the prediction xs[1]
    if (step % 2 == 0) {
      eng.mpc_step(x, 1, 3);
    } else {
      if (hipMemcpy(x_dev, x.data(), sizeof(double) * B * n, hipMemcpyHostToDevice) != hipSuccess) return 3;
      eng.mpc_step((const void*)x_dev, 1, 3, ILQR_TAIL_HOLD);
    }
    eng.copy_controls_to_device(0, 1, u_dev);
    eng.synchronize();
    std::vector<double> u(B * m);
    if (hipMemcpy(u.data(), u_dev, sizeof(double) * B * m, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    const std::vector<double> us = eng.controls();
    for (int b = 0; b < B; b++) for (int j = 0; j < m; j++) if (u[b * m + j] != us[(size_t)b * T * m + j]) return 4;
  }
  const double d1 = dist(x);
  printf("goal_distance %.6f %.6f\n", d0, d1);
  if (!(d1 < d0)) return 5;  // 10 control periods of 0.05 s toward the goal
  BatchILQR host(std::make_shared<HostOnly>(), 2, 10, 0.02);
  std::vector<double> hx(4, 0.5), hu(20, 0.0);
  host.init_traj(hx, hu);
  bool threw = false;
  try { host.mpc_step(hx, 1, 1); } catch (const std::logic_error&) { threw = true; }
  if (!threw) return 6;
  threw = false;
  try { host.shift_horizon(1); } catch (const std::logic_error&) { threw = true; }
  if (!threw) return 7;
  hipFree(x_dev); hipFree(u_dev);
  printf("ok\n");
  return 0;
}
'''


def test_cpp_facade_receding_loop(tmp_path):
    from ilqr_amd import _build
    _build.build()
    src, exe = tmp_path / "mpc.cpp", str(tmp_path / "mpc")
    src.write_text(CPP)
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-DILQR_AMD_NO_EIGEN", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", str(src), "-o", exe,
                           "-L" + os.path.join(ROOT, "ilqr_amd", "lib"), "-lilqr_amd", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "ilqr_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "ok" in r.stdout
