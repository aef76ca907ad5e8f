"""What a multi-start step costs, on the headline problem (acrobot, T = 499, B = 4096, limits +-1.5, fp64, shift 1, one iteration per step).

  python scripts/bench_mpc_clone.py [--steps 30] [--host-reps 3] [--out profiles/mpc_clone_bench.txt]

For the group sizes 2, 4 and 16 (B = environments x plans, a group = the plans of one environment):
  (a) step          ilqr_mpc_step alone
  (b) step+clone    ilqr_mpc_step, then ilqr_clone_best(group, du): the best plan of every group over the others, plus noise
      clone         ilqr_clone_best(group, du) alone, between two events of its own (k_select_best, k_select_clone, k_clone_nominal)
  (c) host          the composition without the call: every getter, the gather in numpy, every setter (host clock, synchronised;
                    status, iteration counts, flgChange and dV have no setter: the composition is not even a faithful copy)
  (d) d2d copy      a plain device-to-device copy of the bytes the clone writes -- (group - 1) / group of x0, xs, us, k, K --: the yardstick
                    for the gather kernel
As scripts/bench_mpc_reset.py: the next x0 is xs[1] of the handle's nominal plus noise, made by torch on the handle's stream, the calls run
between two HIP events, and (a) and (b) take their steps in turn on handles of their own.  Reported: median (min .. max) per step, and
(b) - (a) and `clone` against (d).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, DT, LIM = 4096, 499, 0.02, 1.5
GROUPS = (2, 4, 16)
NX, NU = 4, 1
TRAJ_BYTES = 8 * (NX + (T + 1) * NX + T * NU + T * NU + T * NU * NX)  # x0, xs, us, k, K of one trajectory, fp64


def x0_batch():
    rng = np.random.default_rng(1234)
    return rng.uniform(-1, 1, size=(B, 4)) * np.array([np.pi, np.pi, 1.0, 1.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    stream = torch.cuda.Stream()  # the handles' stream and torch's (its default stream is the null stream: a handle given 0 makes its own)
    with torch.cuda.stream(stream):
        run(args, torch, stream)


def host_clone(g, group):
    """the composition: getters, numpy gather by the best-of-group map, setters (what has a setter)"""
    xs, us = g.trajectory()
    k, K = g.gains()
    cost = g.cost()
    lam, dlam = g.lambdas()
    c = np.where(np.isfinite(cost), cost, np.inf).reshape(-1, group)
    src = (np.arange(B) // group) * group + np.repeat(np.argmin(c, axis=1), group)
    g.set_trajectory(x0=xs[src, 0], xs=xs[src], us=us[src], cost=cost[src])
    g.set_gains(k=k[src], K=K[src])
    g.set_lambda(lam[src], dlam[src])
    g.synchronize()


def run(args, torch, stream):
    from ilqr_amd import BatchILQR
    sp = stream.cuda_stream
    assert sp and torch.cuda.current_stream().cuda_stream == sp
    gen = torch.Generator(device="cuda").manual_seed(7)
    lines, rec = [], {"problem": dict(model="acrobot", B=B, T=T, u_lim=LIM, dtype="f64", shift=1, n_iters=1, steps=args.steps), "groups": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        return e

    def stats(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v))

    def fmt(s):
        return "%.3f ms median (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])

    say("bench_mpc_clone: %s, acrobot T=%d B=%d limits +-%.1f fp64, shift 1, 1 iteration per step, %d steps per row"
        % (torch.cuda.get_device_properties(0).name, T, B, LIM, args.steps))
    x0, u0 = x0_batch(), np.zeros((B, T, 1))
    xs_buf = torch.empty((B, T + 1, 4), dtype=torch.float64, device="cuda")
    for group in GROUPS:
        hs = {}
        for case in ("step", "step+clone"):
            g = BatchILQR("acrobot", B, T, DT, u_min=-LIM, u_max=LIM, stream=sp)
            g.init_traj(x0, u0)
            g.iterate(20)
            g.synchronize()
            hs[case] = g
        ms = {"step": [], "step+clone": [], "clone": []}
        n_cloned = 0
        flags = torch.zeros(B, dtype=torch.int32, device="cuda")
        for step in range(args.steps + 2):  # (two warm-up steps)
            du = 1e-2 * torch.randn((B, T, NU), dtype=torch.float64, device="cuda", generator=gen)
            for case in ("step", "step+clone"):
                g = hs[case]
                g.copy_trajectory_to_device(xs_buf.data_ptr(), None)
                x_new = (xs_buf[:, 1] + 1e-3 * torch.randn((B, 4), dtype=torch.float64, device="cuda", generator=gen)).contiguous()
                e0 = ev()
                g.mpc_step(x0_ptr=x_new.data_ptr(), shift=1, iters=1)
                e1 = ev()
                if case == "step+clone":
                    g.clone_best(group, du_ptr=du.data_ptr())
                e2 = ev()
                e2.synchronize()
                if step >= 2:
                    ms[case].append(e0.elapsed_time(e2))
                    if case == "step+clone":
                        ms["clone"].append(e1.elapsed_time(e2))
                        g.copy_clone_flags_to_device(flags.data_ptr())
                        n_cloned += int((flags == 1).sum().item())
        # (d) the bytes the clone writes, copied once device to device
        nbytes = (B - B // group) * TRAJ_BYTES
        a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        d2d = []
        for i in range(args.steps + 2):
            e0 = ev()
            b.copy_(a)
            e1 = ev()
            e1.synchronize()
            if i >= 2:
                d2d.append(e0.elapsed_time(e1))
        del a, b
        # (c) the host composition, on the handle that cloned (one warm-up repeat)
        host = []
        for i in range(args.host_reps + 1):
            stream.synchronize()
            t0 = time.perf_counter()
            host_clone(hs["step+clone"], group)
            if i >= 1:
                host.append(1e3 * (time.perf_counter() - t0))
        r = dict(step=stats(ms["step"]), step_clone=stats(ms["step+clone"]), clone=stats(ms["clone"]), d2d=stats(d2d), host=stats(host),
                 cloned_per_step=n_cloned / args.steps, clone_bytes=nbytes)
        r["b_minus_a"] = r["step_clone"]["median"] - r["step"]["median"]
        rec["groups"][group] = r
        say("group=%-2d (a) step        GPU %s" % (group, fmt(r["step"])))
        say("group=%-2d (b) step+clone  GPU %s   (b)-(a) %+.3f ms   %.0f cloned per step" % (group, fmt(r["step_clone"]), r["b_minus_a"], r["cloned_per_step"]))
        say("group=%-2d     clone alone GPU %s" % (group, fmt(r["clone"])))
        say("group=%-2d (d) d2d copy    GPU %s   %.1f MB written (%.0f GB/s read+write)"
            % (group, fmt(r["d2d"]), nbytes / 1e6, 2 * nbytes / 1e6 / r["d2d"]["median"]))
        say("group=%-2d (c) host        wall %s" % (group, fmt(r["host"])))
        for g in hs.values():
            g.close()
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
