"""What ilqr_param_gradient_on_device costs (k_pg_costate, k_pg_contract, k_pg_reduce) beside the same handle's finite-difference sweep
(ilqr_compute_derivatives: k_derivatives_g), which evaluates the same model point by point: 40 Euler maps and 880 cost evaluations per
knot there, 6 * NTP = 48 evaluations (cost and Euler map each) per knot and direction here.

  python scripts/bench_param_gradient.py [--reps 30] [--small] [--out profiles/param_gradient_bench.txt]

The pendulum chain (examples/user_model_pendulum_chain.hpp, nx = 16, nu = 4, NTP = 8) at B = 4096, T = 200, fp64, per-trajectory rows
within +-20 % of the defaults, the nominal of 3 iterations; n_dirs in {1, 4}.  Every call between two HIP events on the handle's stream,
median (min .. max) of --reps timings after 3 warm-up calls (the first of which allocates the scratch), the rows taking their calls in turn:

  derivatives       ilqr_compute_derivatives: the whole sweep, every knot
  param_gradient S  dxs, dus, dlam of S directions to gp (the costate in scratch)
  ... S with lam    the same, the costate written to the caller's array
No pass/fail threshold.  --small: B = 256, T = 40, to try the script out."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 0.02
NL, NX, NU, NTP = 8, 16, 4, 8
PARAMS = np.array([9.81, 0.1, 2.0, 10.0, 1.0, 0.1, 50.0, 0.0])
DIRS = (1, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 20, "median of at least 20"
    import torch
    torch.cuda.init()
    stream = torch.cuda.Stream()  # the handle's stream and torch's (its default stream is the null stream: a handle given 0 makes its own)
    with torch.cuda.stream(stream):
        run(args, torch, stream)


def run(args, torch, stream):
    from ilqr_amd import BatchILQR, _build
    lib = _build.build_user(_build.USER_CHAIN_HEADER, _build.USER_CHAIN_LIB)
    sp = stream.cuda_stream
    assert sp and torch.cuda.current_stream().cuda_stream == sp
    lines = []

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

    B, T = (256, 40) if args.small else (4096, 200)
    rng = np.random.default_rng(1234)
    g = BatchILQR("user", B, T, DT, u_min=-2.0, u_max=2.0, lib=lib, nx=NX, nu=NU, user_params=PARAMS, stream=sp)
    rows_p = PARAMS[None, :] * (1.0 + rng.uniform(-0.2, 0.2, (B, NTP)))
    rows_p[:, 7] = rng.uniform(-1.0, 1.0, B)
    g.set_trajectory_params(rows_p)
    g.init_traj(np.concatenate([rng.uniform(-1, 1, (B, NL)), rng.uniform(-1, 1, (B, NL)) * 0.5], axis=1), np.zeros((B, T, NU)))
    g.iterate(3)
    g.compute_derivatives()
    g.synchronize()
    f64 = dict(dtype=torch.float64, device="cuda")
    Smax = max(DIRS)  # the caller's arrays, sized for the most directions (a smaller S uses a prefix)
    dxs, dlam = torch.randn((B * (T + 1) * Smax * NX,), **f64), torch.randn((B * (T + 1) * Smax * NX,), **f64)
    dus = torch.randn((B * T * Smax * NU,), **f64)
    gp, lam = torch.empty((B * Smax * NTP,), **f64), torch.empty((B * (T + 1) * NX,), **f64)
    rows = {"derivatives": g.compute_derivatives}
    for S in DIRS:
        rows["param_gradient %d" % S] = lambda S=S: g.param_gradient_on_device(S, dxs, dus, dlam, gp=gp)
        rows["param_gradient %d with lam" % S] = lambda S=S: g.param_gradient_on_device(S, dxs, dus, dlam, gp=gp, lam=lam)
    ms = {name: [] for name in rows}
    for rep in range(args.reps + 3):
        for name, fn in rows.items():
            t = timed(fn)
            if rep >= 3:
                ms[name].append(t)
    assert bool(torch.isfinite(gp).all())
    say("bench_param_gradient: %s, fp64, %d timings per row after 3 warm-up calls, the rows in turn" % (torch.cuda.get_device_properties(0).name, args.reps))
    say("pendulum chain: nx=%d nu=%d NTP=%d T=%d B=%d, the nominal of 3 iterations, derivatives stage kernel %s" % (
        NX, NU, NTP, T, B, g.lib.ilqr_stage_kernel_name(g.h, 0).decode()))
    rec = dict(reps=args.reps, B=B, T=T, rows={})
    base = statistics.median(ms["derivatives"])
    for name, v in ms.items():
        s = dict(median=statistics.median(v), min=min(v), max=max(v))
        rec["rows"][name] = s
        say("  %-28s GPU %9.4f ms median (%.4f .. %.4f)  %8.2f ns per trajectory-knot  %5.2f x derivatives" %
            (name, s["median"], s["min"], s["max"], 1e6 * s["median"] / (B * (T + 1)), s["median"] / base))
    g.close()
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
