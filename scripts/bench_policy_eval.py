"""What applying the stored feedback policy to caller-given states costs (ilqr_evaluate_policy_on_device; k_evaluate_t / k_evaluate_g).

  python scripts/bench_policy_eval.py [--reps 30] [--small] [--out profiles/policy_eval_bench.txt]

Two problems: the headline acrobot (T = 499, B = 4096, limits +-1.5, fp64, the policy of 20 iterations: k_evaluate_t) and the pendulum-chain
twin (n = 16, m = 4, T = 200, B = 4096, fp64, the policy of 3 iterations: k_evaluate_g).  Per problem, every call between two HIP events
on the handle's stream, median (min .. max) of --reps timings after 3 warm-up calls, the rows of a comparison taking their calls in turn:

  full horizon   evaluate(t0 = 0, n = T, S = 64): B * 64 rollouts, against the same handle's ilqr_rollout_candidates (11 * B rollouts of the
                 search kernel, k_rollout / k_rollout_g), both as time per rollout-knot.  The same arithmetic per knot; the search stores a
                 candidate per step, the evaluation stores nothing and shares a trajectory's nominal fetch among its lanes.
  lookup         evaluate(n = 1, S = 1), the control for a measured state, against what a caller does without it: ilqr_copy_gains_to_device
                 (K) + ilqr_copy_trajectory_to_device (xs, us) of the same handle.
  plant step     evaluate(n = shift = 1, S = 1) alone, and followed by ilqr_mpc_step(x0_device = x_end, shift 1, 1 iteration): the plant
                 step's share of a receding-horizon step.
--small: B = 256 and short horizons, to try the script out."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, NALPHA, S_FULL = 0.02, 11, 64
CHAIN_PARAMS = np.array([9.81, 0.1, 2.0, 10.0, 1.0, 0.1, 50.0, 0.0])


def problems(small):
    from ilqr_amd import _build
    B = 256 if small else 4096
    rng = np.random.default_rng(1234)
    yield dict(name="acrobot", B=B, T=99 if small else 499, iters=20, kernel="k_evaluate_t",
               ctor=dict(model="acrobot", u_min=-1.5, u_max=1.5), x0=rng.uniform(-1, 1, size=(B, 4)) * np.array([np.pi, np.pi, 1.0, 1.0]), nu=1)
    lib = _build.build_user(_build.USER_CHAIN_HEADER, _build.USER_CHAIN_LIB)
    x0 = np.concatenate([rng.uniform(-1, 1, (B, 8)), rng.uniform(-1, 1, (B, 8)) * 0.5], axis=1)
    yield dict(name="chain", B=B, T=40 if small else 200, iters=3, kernel="k_evaluate_g",
               ctor=dict(model="user", lib=lib, nx=16, nu=4, u_min=-2.0, u_max=2.0, user_params=CHAIN_PARAMS), x0=x0, nu=4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 20, "median of at least 20"
    import torch
    torch.cuda.init()
    stream = torch.cuda.Stream()  # the handles' stream and torch's (its default stream is the null stream: a handle given 0 makes its own)
    with torch.cuda.stream(stream):
        run(args, torch, stream)


def run(args, torch, stream):
    from ilqr_amd import BatchILQR
    sp = stream.cuda_stream
    assert sp and torch.cuda.current_stream().cuda_stream == sp
    lines, rec = [], {"reps": args.reps, "problems": {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def in_turn(rows):
        """rows: name -> callable; every row takes a call per round, 3 warm-up rounds, then --reps timed ones: name -> list of ms"""
        ms = {name: [] for name in rows}
        for rep in range(args.reps + 3):
            for name, fn in rows.items():
                t = timed(fn)
                if rep >= 3:
                    ms[name].append(t)
        return ms

    def stat(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v))

    say("bench_policy_eval: %s, fp64, %d timings per row after 3 warm-up calls, the rows of a comparison in turn" % (torch.cuda.get_device_properties(0).name, args.reps))
    gen = torch.Generator(device="cuda").manual_seed(7)
    for p in problems(args.small):
        B, T, nu = p["B"], p["T"], p["nu"]
        ctor = dict(p["ctor"])
        g = BatchILQR(ctor.pop("model"), B, T, DT, stream=sp, **ctor)
        nx = g.nx
        g.init_traj(p["x0"], np.zeros((B, T, nu)))
        g.iterate(p["iters"])
        g.synchronize()
        out = rec["problems"][p["name"]] = dict(B=B, T=T, nx=nx, nu=nu, kernel=p["kernel"])
        say("%s: nx=%d nu=%d T=%d B=%d, the policy of %d iterations (%s)" % (p["name"], nx, nu, T, B, p["iters"], p["kernel"]))
        f64 = dict(dtype=torch.float64, device="cuda")
        xs = torch.empty((B, T + 1, nx), **f64)
        us = torch.empty((B, T, nu), **f64)
        K = torch.empty((B, T, nx * nu), **f64)
        g.copy_trajectory_to_device(xs.data_ptr(), None)
        # ---- full horizon, S = 64, against the search rollout ----
        x = (xs[:, 0][:, None, :] + 0.05 * torch.randn((B, S_FULL, nx), generator=gen, **f64)).contiguous()
        cost = torch.empty((B, S_FULL), **f64)
        x_end = torch.empty((B, S_FULL, nx), **f64)
        u_first = torch.empty((B, S_FULL, nu), **f64)
        ms = in_turn({"evaluate": lambda: g.evaluate_policy_on_device(0, T, S_FULL, x.data_ptr(), cost.data_ptr(), x_end.data_ptr(), u_first.data_ptr()),
                      "search": lambda: g._check(g.lib.ilqr_rollout_candidates(g.h, None))})
        finite = float(torch.isfinite(cost).double().mean().item())  # (an overflowing rollout costs what a finite one costs: no branch in the step)
        assert finite > 0.5, finite
        knots = {"evaluate": B * S_FULL * T, "search": NALPHA * B * T}
        out["full_horizon"] = {}
        for name in ("evaluate", "search"):
            s = stat(ms[name])
            ps = {k: 1e9 * v / knots[name] for k, v in s.items()}  # ms -> ps per rollout-knot
            out["full_horizon"][name] = dict(ms=s, rollouts=knots[name] // T, ps_per_rollout_knot=ps)
            say("  full horizon  %-8s %7d rollouts  GPU %8.3f ms median (%.3f .. %.3f)  %7.2f ps per rollout-knot (%.2f .. %.2f)"
                % (name, knots[name] // T, s["median"], s["min"], s["max"], ps["median"], ps["min"], ps["max"]))
        e, r = out["full_horizon"]["evaluate"]["ps_per_rollout_knot"], out["full_horizon"]["search"]["ps_per_rollout_knot"]
        out["full_horizon"]["finite_share"] = finite
        say("  full horizon  %.2f %% of the evaluated rollouts stay finite" % (100 * finite))
        say("  full horizon  evaluate / search per rollout-knot: %.2f (the search's own min .. max spread: %.2f .. %.2f of its median)"
            % (e["median"] / r["median"], r["min"] / r["median"], r["max"] / r["median"]))
        # ---- the lookup: n = 1, S = 1 against copying the policy out ----
        x1 = (xs[:, 0] + 0.05 * torch.randn((B, nx), generator=gen, **f64)).contiguous()
        u1 = torch.empty((B, 1, nu), **f64)
        xe1 = torch.empty((B, 1, nx), **f64)

        def copy_out():
            g.copy_gains_to_device(None, K.data_ptr())
            g.copy_trajectory_to_device(xs.data_ptr(), us.data_ptr())
        ms = in_turn({"evaluate n=1 S=1": lambda: g.evaluate_policy_on_device(0, 1, 1, x1.data_ptr(), None, None, u1.data_ptr()),
                      "copy K, xs, us out": copy_out})
        out["lookup"] = {name: stat(v) for name, v in ms.items()}
        mb = (K.numel() + xs.numel() + us.numel()) * 8 / 1e6
        for name, v in ms.items():
            s = stat(v)
            say("  lookup        %-20s GPU %8.4f ms median (%.4f .. %.4f)%s" % (name, s["median"], s["min"], s["max"], "  %.0f MB written" % mb if "copy" in name else ""))
        # ---- the plant step's share of a receding-horizon step (last: the steps move the horizon) ----
        def plant():
            g.evaluate_policy_on_device(0, 1, 1, x1.data_ptr(), None, xe1.data_ptr(), None)

        def plant_and_step():
            plant()
            g.mpc_step(x0_ptr=xe1.data_ptr(), shift=1, iters=1)
            x1.copy_(xe1[:, 0])  # the next measured state: where the model says the plant went
        ms = in_turn({"plant step alone": plant, "plant step + mpc_step(1)": plant_and_step})
        out["plant_step"] = {name: stat(v) for name, v in ms.items()}
        for name, v in ms.items():
            s = stat(v)
            say("  plant step    %-24s GPU %8.4f ms median (%.4f .. %.4f)" % (name, s["median"], s["min"], s["max"]))
        a, b = out["plant_step"]["plant step alone"]["median"], out["plant_step"]["plant step + mpc_step(1)"]["median"]
        say("  plant step    share of the receding-horizon step: %.2f %%" % (100 * a / b))
        g.close()
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
