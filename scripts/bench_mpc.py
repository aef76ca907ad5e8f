"""Receding-horizon steps on the headline problem (acrobot, T = 499, B = 4096, limits +-1.5, fp64): the device loop of ilqr_mpc_step against
the same loop done the host way.

  python scripts/bench_mpc.py [--steps 50] [--out profiles/mpc_step_bench.txt]

1. 20 iterations solve the first horizon.  Then `--steps` receding steps with shift = 1 for each budget n_iters in {0, 1, 3}: the next x0
   is xs[1] of the current nominal plus noise, made by torch on the handle's stream (the stream rule of INTEGRATION.md), and
   ilqr_mpc_step runs between two HIP events.  Reported: the GPU time of the step (events) and the host wall time of the call itself.
2. The shift alone (ilqr_shift_horizon, k_shift_horizon) between events, next to a hipMemcpyAsync device-to-device copy of the same bytes
   (xs, us, k, K: 164 MB) on the same stream -- under `rocprofv3 --kernel-trace --stats` both show up in the kernel table as well.
3. The same steps the host way: ilqr_get_results_async into page-locked buffers, the shift in numpy, set_trajectory / set_gains, and
   ilqr_warm_start on a handle with max_iter = n_iters.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, DT, LIM = 4096, 499, 0.02, 1.5


def x0_batch():
    rng = np.random.default_rng(1234)
    return rng.uniform(-1, 1, size=(B, 4)) * np.array([np.pi, np.pi, 1.0, 1.0])


def np_shift(xs, us, k, K, s):  # include/ilqr_amd.h, ILQR_TAIL_HOLD (K in the ABI's memory layout [B][T][nx][nu])
    for a, hold in ((xs, True), (us, True), (k, False), (K, True)):
        n = a.shape[1]
        a[:, :n - s] = a[:, s:].copy()
        a[:, n - s:] = a[:, n - 1:n] if hold else 0.0


def med(v):
    return statistics.median(v) if v else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--host-steps", type=int, default=None, help="steps of the host-way loop (default: --steps)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    stream = torch.cuda.Stream()  # the handles' stream and torch's (its default stream is the null stream: a handle given 0 makes its own)
    with torch.cuda.stream(stream):
        run(args, torch, stream)


def run(args, torch, stream):
    from ilqr_amd import BatchILQR
    sp = stream.cuda_stream
    assert sp and torch.cuda.current_stream().cuda_stream == sp
    hip = C.CDLL("libamdhip64.so.7")  # (the runtime torch has loaded)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    gen = torch.Generator(device="cuda").manual_seed(7)
    lines, rec = [], {"problem": dict(model="acrobot", B=B, T=T, u_lim=LIM, dtype="f64", shift=1, steps=args.steps)}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        return e

    dev = torch.cuda.get_device_properties(0)
    say("bench_mpc: %s, acrobot T=%d B=%d limits +-%.1f fp64, shift 1, %d steps per budget" % (dev.name, T, B, LIM, args.steps))
    x0 = x0_batch()
    u0 = np.zeros((B, T, 1))
    xs_buf = torch.empty((B, T + 1, 4), dtype=torch.float64, device="cuda")

    # ---- 1. the device loop ----
    rec["device"] = {}
    for n in (0, 1, 3):
        g = BatchILQR("acrobot", B, T, DT, u_min=-LIM, u_max=LIM, stream=sp)
        g.init_traj(x0, u0)
        g.iterate(20)
        g.synchronize()
        gpu_ms, call_us = [], []
        for step in range(args.steps + 2):  # (two warm-up steps)
            g.copy_trajectory_to_device(xs_buf.data_ptr(), None)
            x_new = (xs_buf[:, 1] + 1e-3 * torch.randn((B, 4), dtype=torch.float64, device="cuda", generator=gen)).contiguous()
            e0 = ev()
            t0 = time.perf_counter()
            g.mpc_step(x0_ptr=x_new.data_ptr(), shift=1, iters=n)
            t1 = time.perf_counter()
            e1 = ev()
            e1.synchronize()
            if step >= 2:
                gpu_ms.append(e0.elapsed_time(e1))
                call_us.append((t1 - t0) * 1e6)
        st = g.status()[0]
        rec["device"][n] = dict(gpu_ms_median=med(gpu_ms), gpu_ms_min=min(gpu_ms), gpu_ms_max=max(gpu_ms),
                                call_us_median=med(call_us), call_us_max=max(call_us), running_after=int((st == 0).sum()))
        say("device  n_iters=%d: mpc_step GPU %.3f ms median (%.3f .. %.3f), host call %.1f us median (max %.1f) = %.1f %% of the GPU time; "
            "%d of %d trajectories still running" % (n, med(gpu_ms), min(gpu_ms), max(gpu_ms), med(call_us), max(call_us),
                                                     100.0 * med(call_us) / 1e3 / med(gpu_ms), rec["device"][n]["running_after"], B))
        g.close()

    # ---- 2. the shift kernel against a device-to-device copy of the same bytes ----
    g = BatchILQR("acrobot", B, T, DT, u_min=-LIM, u_max=LIM, stream=sp)
    g.init_traj(x0, u0)
    g.iterate(5)
    nbytes = B * ((T + 1) * 4 + T + T + T * 4) * 8
    src = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    shift_ms, copy_ms = [], []
    for rep in range(12):
        e0 = ev()
        g.shift_horizon(1)
        e1 = ev()
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, C.c_void_p(sp))  # hipMemcpyDeviceToDevice
        assert rc == 0, rc
        e2 = ev()
        e2.synchronize()
        if rep >= 2:
            shift_ms.append(e0.elapsed_time(e1))
            copy_ms.append(e1.elapsed_time(e2))
    rec["shift"] = dict(bytes=nbytes, shift_ms_median=med(shift_ms), copy_ms_median=med(copy_ms), ratio=med(shift_ms) / med(copy_ms))
    say("shift   %.1f MB (xs, us, k, K): ilqr_shift_horizon %.1f us median (%.1f .. %.1f), hipMemcpyAsync D2D of the same bytes %.1f us "
        "(%.1f .. %.1f): ratio %.2f; shift moves %.2f TB/s (read + write)" % (
            nbytes / 1e6, 1e3 * med(shift_ms), 1e3 * min(shift_ms), 1e3 * max(shift_ms), 1e3 * med(copy_ms), 1e3 * min(copy_ms),
            1e3 * max(copy_ms), med(shift_ms) / med(copy_ms), 2 * nbytes / (med(shift_ms) * 1e-3) / 1e12))
    for n in (0, 1, 3):
        share = med(shift_ms) / rec["device"][n]["gpu_ms_median"]
        say("        the shift is %.1f %% of an mpc_step with n_iters=%d" % (100 * share, n))
    g.close()
    del src, dst

    # ---- 3. the host way ----
    rec["host"] = {}
    hsteps = args.host_steps if args.host_steps is not None else args.steps
    for n in (0, 1, 3):
        g = BatchILQR("acrobot", B, T, DT, u_min=-LIM, u_max=LIM, params=dict(max_iter=n))
        g.init_traj(x0, u0)
        g.iterate(20)
        bufs = g.result_buffers(pinned=True, K=True)
        rng = np.random.default_rng(8)
        wall_ms = []
        for step in range(hsteps + 2):
            t0 = time.perf_counter()
            g.results_async(bufs)
            g.synchronize()
            xs, us, k, K = bufs["xs"], bufs["us"], bufs["k"], bufs["K"]
            x_new = xs[:, 1] + 1e-3 * rng.standard_normal((B, 4))
            np_shift(xs, us, k, K, 1)
            g.set_trajectory(xs=xs, us=us)
            g.lib.ilqr_set_gains(g.h, k.ctypes.data_as(C.POINTER(C.c_double)), K.ctypes.data_as(C.POINTER(C.c_double)))  # (memory layout)
            g.generate_trajectory(x_new)  # ilqr_warm_start: returns when its iterations are done
            t1 = time.perf_counter()
            if step >= 2:
                wall_ms.append((t1 - t0) * 1e3)
        rec["host"][n] = dict(wall_ms_median=med(wall_ms), wall_ms_min=min(wall_ms), wall_ms_max=max(wall_ms))
        say("host    n_iters=%d: results_async + numpy shift + set_trajectory/set_gains + warm_start %.2f ms median per step (%.2f .. %.2f); "
            "device loop %.3f ms: %.1f x" % (n, med(wall_ms), min(wall_ms), max(wall_ms), rec["device"][n]["gpu_ms_median"],
                                            med(wall_ms) / rec["device"][n]["gpu_ms_median"]))
        g.close()
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
