"""What resets inside a receding-horizon step cost, on the headline problem (acrobot, T = 499, B = 4096, limits +-1.5, fp64, shift 1).

  python scripts/bench_mpc_reset.py [--steps 50] [--out profiles/mpc_reset_bench.txt]

Four ways to take the same step, each on a handle of its own that solved the first horizon with 20 iterations, for the budgets n_iters = 0
and 3:
  plain      ilqr_mpc_step                                      (the call as it was)
  no-select  ilqr_mpc_step_reset, no mask, no rules             (k_select_reset + k_reset_nominal find nobody)
  mask 1 %   ilqr_mpc_step_reset, a device mask over 1 % of B   (another 1 % every step, written by torch on the handle's stream)
  nonfinite  ilqr_mpc_step_reset, ILQR_RESET_NONFINITE          (one more selection, rollout and commit)
As scripts/bench_mpc.py: the next x0 is xs[1] of the handle's nominal plus noise, made by torch on the handle's stream, and the call runs
between two HIP events.  The four take their steps in turn, step by step, so that whatever else the machine does meets all of them alike;
reported: median (min .. max) of the GPU time per step, and each row's difference to `plain` against plain's own spread.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, DT, LIM = 4096, 499, 0.02, 1.5
CASES = ("plain", "no-select", "mask 1 %", "nonfinite")


def x0_batch():
    rng = np.random.default_rng(1234)
    return rng.uniform(-1, 1, size=(B, 4)) * np.array([np.pi, np.pi, 1.0, 1.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    stream = torch.cuda.Stream()  # the handles' stream and torch's (its default stream is the null stream: a handle given 0 makes its own)
    with torch.cuda.stream(stream):
        run(args, torch, stream)


def run(args, torch, stream):
    from ilqr_amd import BatchILQR, capi
    sp = stream.cuda_stream
    assert sp and torch.cuda.current_stream().cuda_stream == sp
    gen = torch.Generator(device="cuda").manual_seed(7)
    lines, rec = [], {"problem": dict(model="acrobot", B=B, T=T, u_lim=LIM, dtype="f64", shift=1, steps=args.steps), "gpu_ms": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        return e

    say("bench_mpc_reset: %s, acrobot T=%d B=%d limits +-%.1f fp64, shift 1, %d steps per row, the four rows of a budget step in turn"
        % (torch.cuda.get_device_properties(0).name, T, B, LIM, args.steps))
    x0, u0 = x0_batch(), np.zeros((B, T, 1))
    xs_buf = torch.empty((B, T + 1, 4), dtype=torch.float64, device="cuda")
    lanes = torch.arange(B, device="cuda")
    n_sel = max(1, B // 100)
    for n in (0, 3):
        hs = {}
        for case in CASES:
            g = BatchILQR("acrobot", B, T, DT, u_min=-LIM, u_max=LIM, stream=sp)
            g.init_traj(x0, u0)
            g.iterate(20)
            g.synchronize()
            hs[case] = g
        ms = {case: [] for case in CASES}
        n_reset = {case: 0 for case in CASES}
        flags = torch.zeros(B, dtype=torch.int32, device="cuda")
        for step in range(args.steps + 2):  # (two warm-up steps)
            mask = (((lanes * 7 + step * n_sel) % B) < n_sel).to(torch.int32)  # 1 % of the batch, spread over the tiles, moving every step
            for case in CASES:
                g = hs[case]
                g.copy_trajectory_to_device(xs_buf.data_ptr(), None)
                x_new = (xs_buf[:, 1] + 1e-3 * torch.randn((B, 4), dtype=torch.float64, device="cuda", generator=gen)).contiguous()
                xp = x_new.data_ptr()
                e0 = ev()
                if case == "plain":
                    g.mpc_step(x0_ptr=xp, shift=1, iters=n)
                elif case == "no-select":
                    g._check(g.lib.ilqr_mpc_step_reset(g.h, None, xp, 1, capi.TAIL_HOLD, n, None, None, 0))
                elif case == "mask 1 %":
                    g.mpc_step(x0_ptr=xp, shift=1, iters=n, reset_mask_ptr=mask.data_ptr())
                else:
                    g.mpc_step(x0_ptr=xp, shift=1, iters=n, reset_nonfinite=True)
                e1 = ev()
                e1.synchronize()
                if step >= 2:
                    ms[case].append(e0.elapsed_time(e1))
                    if case != "plain":
                        g.copy_reset_flags_to_device(flags.data_ptr())
                        n_reset[case] += int((flags != 0).sum().item())
        base = statistics.median(ms["plain"])
        spread = max(ms["plain"]) - min(ms["plain"])
        rec["gpu_ms"][n] = {}
        for case in CASES:
            v = ms[case]
            med = statistics.median(v)
            rec["gpu_ms"][n][case] = dict(median=med, min=min(v), max=max(v), resets_per_step=n_reset[case] / args.steps)
            say("n_iters=%d  %-9s  GPU %.3f ms median (%.3f .. %.3f)  %+.3f ms to plain (plain's own min..max spread %.3f ms)  %.1f resets per step"
                % (n, case, med, min(v), max(v), med - base, spread, n_reset[case] / args.steps))
        for g in hs.values():
            g.close()
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
