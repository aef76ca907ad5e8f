"""What per-knot model parameters cost (ilqr_set_knot_params: the PK instantiations of k_rollout_g / k_derivatives_g, k_gather_knot_params)
beside the same handle with no rows and with per-trajectory rows.

  python scripts/bench_knot_params.py [--rounds 6] [--iters 5] [--small] [--parent-lib OTHER.so] [--out profiles/knot_params_bench.txt]

The pendulum chain (examples/user_model_pendulum_chain.hpp, nx = 16, nu = 4, NTP = 8) at B = 4096, T = 200, fp64, ILQR_FLAG_FIXED_WORK (every
iteration does the whole work for every trajectory).  Three modes on ONE handle, taking their turns round after round so that they see the
same clocks: no rows (the shared parameters), per-trajectory rows within +-20 % of the defaults, and knot rows that repeat each
trajectory's row at every knot -- the same problem as the per-trajectory mode, so the same work, through the PK instantiations.  A turn:
the mode set, init_traj, one warm-up iteration, then --iters iterations between two synchronisations on the host clock, the stage times
from ilqr_profile_read (HIP events round every stage).  Reported per mode: the median (min .. max) over the rounds of the time per
iteration and of every stage's time per launch, then knot rows minus per-trajectory rows per stage, beside the per-trajectory rows' own
spread.
--parent-lib: another build of the twin's library (the parent commit's: it has no knot rows) takes turns of the two modes it has in the
same rounds -- the yardstick for "the kernels of those two modes did not change".
The gather: ilqr_set_knot_params from a device reference of n_knots = 2 T rows between two HIP events on the handle's stream, k0 moving,
median of 20 after 3 warm-up calls; and from a host reference of the same size (one host-to-device copy, then the same gather).
No pass/fail threshold.  --small: B = 256, T = 40, to try the script out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT, LIM = 0.02, 2.0
NL, NX, NU, NTP = 8, 16, 4, 8
PARAMS = np.array([9.81, 0.1, 2.0, 10.0, 1.0, 0.1, 50.0, 0.0])
STAGES = ("derivatives", "backward", "rollout", "accept")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    stream = torch.cuda.Stream()  # the handle's stream and torch's (its default stream is the null stream: a handle given 0 makes its own)
    with torch.cuda.stream(stream):
        run(args, torch, stream)


def run(args, torch, stream):
    from ilqr_amd import BatchILQR, _build, capi
    lib = _build.build_user(_build.USER_CHAIN_HEADER, _build.USER_CHAIN_LIB)
    sp = stream.cuda_stream
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B, T = (256, 40) if args.small else (4096, 200)
    rng = np.random.default_rng(1234)
    x0 = np.concatenate([rng.uniform(-1, 1, (B, NL)), rng.uniform(-1, 1, (B, NL)) * 0.5], axis=1)
    u0 = np.zeros((B, T, NU))
    rows = PARAMS[None, :] * (1.0 + rng.uniform(-0.2, 0.2, (B, NTP)))
    rows[:, 7] = rng.uniform(-1.0, 1.0, B)
    knot_rows = np.ascontiguousarray(np.repeat(rows[:, None], T + 1, axis=1))

    def make(path):
        return BatchILQR("user", B, T, DT, u_min=-LIM, u_max=LIM, lib=path, nx=NX, nu=NU, user_params=PARAMS, flags=capi.FLAG_FIXED_WORK,
                         params=dict(max_iter=args.iters + 3), stream=sp)

    builds = {"this": make(lib)}
    if args.parent_lib:  # a build from before the knot rows exports two symbols fewer: bound here with the ones it has
        import ctypes
        older = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name, (res, argtypes) in capi.SYMBOLS.items():
            fn = getattr(older, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, argtypes
        capi._libs[os.path.abspath(args.parent_lib)] = older
        builds["parent"] = make(args.parent_lib)
    setters = {"none": lambda g: g.clear_trajectory_params(), "traj": lambda g: g.set_trajectory_params(rows), "knot": lambda g: g.set_knot_params(knot_rows)}
    turns = [(b, m) for m in ("none", "traj", "knot") for b in builds if m != "knot" or hasattr(builds[b].lib, "ilqr_set_knot_params")]
    got = {turn: dict(iter_ms=[], cost=None, **{s: [] for s in STAGES}) for turn in turns}
    for rnd in range(args.rounds + 1):  # (round 0 warms every mode of every build up and is dropped)
        for turn in turns:
            g = builds[turn[0]]
            setters[turn[1]](g)
            g.init_traj(x0, u0)
            g.iterate(1)
            g.profile(True)
            g.profile_reset()
            g.synchronize()
            t0 = time.perf_counter()
            g.iterate(args.iters)
            g.synchronize()
            dt = time.perf_counter() - t0
            p = g.profile_read()
            g.profile(False)
            if rnd == 0:
                continue
            got[turn]["iter_ms"].append(dt / args.iters * 1e3)
            got[turn]["cost"] = float(g.cost().mean())
            for s in STAGES:
                ms, n = p[s]
                got[turn][s].append(ms / n if n else 0.0)
    g = builds["this"]
    say("bench_knot_params: %s, fp64, fixed work, %d rounds of %d iterations per mode after a warm-up round, the modes in turn" % (
        torch.cuda.get_device_properties(0).name, args.rounds, args.iters))
    say("pendulum chain: nx=%d nu=%d NTP=%d T=%d B=%d; stage kernels %s; per-knot window %.1f MB" % (
        NX, NU, NTP, T, B, ", ".join(g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index(s)).decode() for s in STAGES[:3]), knot_rows.nbytes / 1e6))
    med = lambda v: statistics.median(v)
    fmt = lambda v: "%8.3f (%.3f .. %.3f)" % (med(v), min(v), max(v))
    rec = dict(B=B, T=T, rounds=args.rounds, iters=args.iters, modes={})
    say("%-14s %-28s %s" % ("build, rows", "ms per iteration", "  ".join("%-28s" % (s + " ms per launch") for s in STAGES)))
    for turn in turns:
        r = got[turn]
        say("%-14s %-28s %s   mean cost %.6g" % ("%s, %s" % turn, fmt(r["iter_ms"]), "  ".join("%-28s" % fmt(r[s]) for s in STAGES), r["cost"]))
        rec["modes"]["%s/%s" % turn] = {k: (dict(median=med(v), min=min(v), max=max(v)) if isinstance(v, list) else v) for k, v in r.items()}
    if ("this", "knot") in got:
        pt, pk = got[("this", "traj")], got[("this", "knot")]
        say("knot rows minus per-trajectory rows (medians; in brackets the per-trajectory rows' own max - min over the rounds):")
        for key in ("iter_ms",) + STAGES:
            say("  %-12s %+8.3f ms  %+6.2f %%   [spread %.3f ms]" % (key, med(pk[key]) - med(pt[key]), 100.0 * (med(pk[key]) / med(pt[key]) - 1.0) if med(pt[key]) else 0.0,
                                                                 max(pt[key]) - min(pt[key])))
    if "parent" in builds:
        say("this build minus the parent's (medians; in brackets the parent's own max - min over the rounds):")
        for m in ("none", "traj"):
            a, b = got[("this", m)], got[("parent", m)]
            for key in ("iter_ms", "derivatives", "rollout"):
                say("  %-5s %-12s %+8.3f ms  %+6.2f %%   [spread %.3f ms]" % (m, key, med(a[key]) - med(b[key]), 100.0 * (med(a[key]) / med(b[key]) - 1.0), max(b[key]) - min(b[key])))
        builds["parent"].close()

    # the gather on its own
    L = 2 * T
    ref = PARAMS[None, None, :] * (1.0 + rng.uniform(-0.2, 0.2, (B, L, NTP)))
    ref_dev = torch.tensor(ref, dtype=torch.float64, device="cuda")
    stream.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    dev_ms = [timed(lambda i=i: g.set_knot_params(ptr=ref_dev.data_ptr(), n_knots=L, k0=i % L)) for i in range(23)][3:]
    want = ref[:, np.minimum(22 % L + np.arange(T + 1), L - 1)]  # (the last call: i = 22)
    assert np.array_equal(g.knot_params(), want)
    host_ms = [timed(lambda i=i: g.set_knot_params(ref, k0=i % L)) for i in range(23)][3:]
    say("gather, n_knots = 2 T = %d (window %.1f MB written, the reference %.1f MB): from device memory %.4f ms median (%.4f .. %.4f) = %.2f TB/s read + write of the window;"
        % (L, knot_rows.nbytes / 1e6, ref.nbytes / 1e6, med(dev_ms), min(dev_ms), max(dev_ms), 2 * knot_rows.nbytes / (med(dev_ms) * 1e-3) / 1e12))
    say("        from a pageable host array (copy of the whole reference, then the gather) %.3f ms median (%.3f .. %.3f)" % (med(host_ms), min(host_ms), max(host_ms)))
    rec["gather"] = dict(n_knots=L, device_ms=dict(median=med(dev_ms), min=min(dev_ms), max=max(dev_ms)), host_ms=dict(median=med(host_ms), min=min(host_ms), max=max(host_ms)))
    g.close()
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
