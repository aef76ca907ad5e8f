"""Every way an array crosses the C ABI, on every storage a handle has (tiled or trajectory-contiguous, fp64 or fp32), with a ragged batch:
the arrays are canonical double [B][S][E] outside and an index map plus a cast away from the handle's own layout, so with values a
float holds exactly

- set_trajectory / set_gains / set_derivatives followed by the getters return the bits that went in;
- ilqr_get_results_async and ilqr_copy_trajectory_to_device / ilqr_copy_gains_to_device equal the getters;
- ilqr_copy_controls_to_device(t0, n) equals us[:, t0 : t0 + n];
- ilqr_mpc_step(shift = 0, n_iters = 0) leaves the same nominal for a host x0 as for the same x0 in device memory (device models only:
  a host-evaluated model has no MPC step)."""
import numpy as np
import pytest

from tests.test_gpu_lq_end_to_end import dense_mats

pytestmark = pytest.mark.gpu
DT = 0.02
B, T = 19, 9  # B: one full tile and a partial one; T + 1 = 10 knots
HANDLES = ["acrobot_f64", "acrobot_f32", "lq_f64", "lq_f32", "host"]
RECORD_BLOCKS = ("fx", "fu", "cx", "cu", "cxx", "cxu", "cuu")


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """torch's device is initialised before this module creates any handle (tests/test_gpu_mpc.py)"""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


def make(name, stream=None):
    from ilqr_amd import BatchILQR
    dtype = "f32" if name.endswith("f32") else "f64"
    if name.startswith("acrobot"):
        return BatchILQR("acrobot", B, T, DT, u_min=-1.5, u_max=1.5, dtype=dtype, stream=stream)
    if name.startswith("lq"):
        return BatchILQR("lq", B, T, DT, lq=dense_mats(6, 3), u_min=-0.4, u_max=0.4, dtype=dtype, stream=stream)
    return BatchILQR("host", B, T, DT, nx=6, nu=3, u_min=-1.0, u_max=1.0, stream=stream)


def exact(rng, *shape):
    """multiples of 1/64 in (-8, 8): float holds them exactly, and no two neighbours of an array are likely to be equal"""
    return rng.integers(-511, 512, size=shape).astype(np.float64) / 64.0


def arrays(g, seed):
    rng = np.random.default_rng(seed)
    n, m = g.nx, g.nu
    a = dict(x0=exact(rng, B, n), xs=exact(rng, B, T + 1, n), us=exact(rng, B, T, m), cost=exact(rng, B), k=exact(rng, B, T, m),
             K=exact(rng, B, T, m, n))
    d = dict(fx=exact(rng, B, T + 1, n, n), fu=exact(rng, B, T + 1, n, m), cx=exact(rng, B, T + 1, n), cu=exact(rng, B, T + 1, m),
             cxx=exact(rng, B, T + 1, n, n), cxu=exact(rng, B, T + 1, n, m), cuu=exact(rng, B, T + 1, m, m))
    return a, d


def on_device(shape):
    import torch
    return torch.full(shape, np.nan, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("name", HANDLES)
def test_setters_getters_and_device_copies_return_the_same_bits(name):
    import torch
    stream = torch.cuda.Stream()  # the handle runs on torch's current stream: its copies into torch tensors are ordered by the stream
    with torch.cuda.stream(stream):
        g = make(name, stream=stream.cuda_stream)
        n, m = g.nx, g.nu
        a, d = arrays(g, 3)
        g.set_trajectory(x0=a["x0"], xs=a["xs"], us=a["us"], cost=a["cost"])
        g.set_gains(k=a["k"], K=a["K"])
        g.set_derivatives(**d)
        # the getters
        xs, us = g.trajectory()
        k, K = g.gains()
        assert np.array_equal(xs, a["xs"]) and np.array_equal(us, a["us"])
        assert np.array_equal(k, a["k"]) and np.array_equal(K, a["K"])
        got = g.derivatives()
        for key in RECORD_BLOCKS:
            assert np.array_equal(got[key], d[key]), key
        # one block replaced: the others stay
        cxu2 = exact(np.random.default_rng(4), B, T + 1, n, m)
        g.set_derivatives(cxu=cxu2)
        got = g.derivatives()
        for key in RECORD_BLOCKS:
            assert np.array_equal(got[key], cxu2 if key == "cxu" else d[key]), key
        # every array in one call, nothing waited for in between
        for pinned in (False, True):
            bufs = g.result_buffers(pinned=pinned)
            for v in bufs.values():
                v[...] = np.nan
            g.results_async(bufs)
            g.synchronize()
            assert np.array_equal(bufs["xs"], xs) and np.array_equal(bufs["us"], us) and np.array_equal(bufs["k"], k)
            assert np.array_equal(np.swapaxes(bufs["K"], -1, -2), K) and np.array_equal(bufs["cost"], a["cost"])
        # a subset of the arrays: each still lands in its own buffer
        bufs = g.result_buffers(pinned=False, K=False)
        g.results_async(dict(us=bufs["us"]))
        g.synchronize()
        assert np.array_equal(bufs["us"], us) and not bufs["xs"].any()
        # canonical arrays in device memory
        xs_d, us_d, k_d, K_d = on_device((B, T + 1, n)), on_device((B, T, m)), on_device((B, T, m)), on_device((B, T, n, m))
        g.copy_trajectory_to_device(xs_d.data_ptr(), us_d.data_ptr())
        g.copy_gains_to_device(k_d.data_ptr(), K_d.data_ptr())
        stream.synchronize()
        assert np.array_equal(xs_d.cpu().numpy(), xs) and np.array_equal(us_d.cpu().numpy(), us)
        assert np.array_equal(k_d.cpu().numpy(), k) and np.array_equal(np.swapaxes(K_d.cpu().numpy(), -1, -2), K)
        # control windows: the first knot, the last, one strictly inside, all
        for t0, nk in ((0, 1), (T - 1, 1), (2, 4), (3, T - 3), (0, T)):
            win = on_device((B, nk, m))
            g.copy_controls_to_device(t0, nk, win.data_ptr())
            stream.synchronize()
            assert np.array_equal(win.cpu().numpy(), us[:, t0:t0 + nk]), (t0, nk)
        # x0 alone: xs[:, 0] is not touched by it, and a second set_trajectory replaces what the first left
        a2, _ = arrays(g, 5)
        g.set_trajectory(x0=a2["x0"])
        assert np.array_equal(g.trajectory()[0], a["xs"])
        g.set_trajectory(xs=a2["xs"], us=a2["us"])
        xs, us = g.trajectory()
        assert np.array_equal(xs, a2["xs"]) and np.array_equal(us, a2["us"])
        g.close()


@pytest.mark.parametrize("name", HANDLES[:4])
def test_mpc_step_x0_from_host_and_from_device_memory(name):
    import torch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        gh, gd = make(name), make(name, stream=stream.cuda_stream)
        rng = np.random.default_rng(7)
        x0, u0 = exact(rng, B, gh.nx) / 16.0, exact(rng, B, T, gh.nu) / 64.0
        for g in (gh, gd):
            g.init_traj(x0, u0)
            g.iterate(2)
        x_new = x0 + exact(rng, B, gh.nx) / 256.0
        gh.mpc_step(x0=x_new, shift=0, iters=0)
        xd = torch.from_numpy(x_new).cuda(non_blocking=True)
        gd.mpc_step(x0_ptr=xd.data_ptr(), shift=0, iters=0)
        stream.synchronize()
        (xs_h, us_h), (xs_d, us_d) = gh.trajectory(), gd.trajectory()
        assert np.isfinite(xs_h).all() and np.isfinite(us_h).all()
        assert np.array_equal(xs_h[:, 0], x_new)  # (exactly representable in float: an fp32 handle holds it too)
        assert np.array_equal(xs_h, xs_d) and np.array_equal(us_h, us_d)
        assert np.array_equal(gh.cost(), gd.cost())
        for p, q in zip(gh.gains(), gd.gains()):
            assert np.array_equal(p, q)
        # ... and a second step from host memory on the handle that took device memory before, and the other way round
        x_new2 = x_new + exact(rng, B, gh.nx) / 256.0
        xd2 = torch.from_numpy(x_new2).cuda(non_blocking=True)
        gd.mpc_step(x0=x_new2, shift=0, iters=0)
        stream.synchronize()
        gh.mpc_step(x0_ptr=xd2.data_ptr(), shift=0, iters=0)
        (xs_h, us_h), (xs_d, us_d) = gh.trajectory(), gd.trajectory()
        assert np.array_equal(xs_h[:, 0], x_new2)
        assert np.array_equal(xs_h, xs_d) and np.array_equal(us_h, us_d) and np.array_equal(gh.cost(), gd.cost())
        gh.close()
        gd.close()
