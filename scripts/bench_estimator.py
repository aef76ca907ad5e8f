"""What ilqr_copy_estimator_to_device costs (k_estimator_t / k_est_filter_w, k_est_loop_w) beside one ilqr_copy_covariance_to_device and
one ilqr_backward_pass of the same handle, which do comparable algebra: one sweep of n x n products over the same records.

  python scripts/bench_estimator.py [--reps 30] [--small] [--out profiles/estimator_bench.txt]

Two problems: the LQ model (n = 32, m = 16, T = 200, B = 8192, fp64, exact derivatives, the policy of 3 iterations) at ny = 8 and 32 outputs
and the headline acrobot (T = 499, B = 4096, limits +-1.5, fp64, the policy of 20 iterations) at ny = 2.  Per problem, every call between
two HIP events on the handle's stream, median (min .. max) of --reps timings after 3 warm-up calls (the first of which materialises the
records and allocates the scratch), the rows taking their calls in turn:

  backward pass       ilqr_backward_pass: the solver's own Riccati sweep with its box-QP
  covariance          Sigma0, W to the expected cost alone (the whole horizon, nothing per knot written)
  filter ny           H, P0, W, V to L of every knot (the filter sweep alone; the gains are what a controller needs)
  filter+loop ny      the same plus the expected cost: the filter sweep leaves Pf, N per knot in handle scratch, the loop sweep reads them
No pass/fail threshold.  --small: B = 256 and short horizons, to try the script out."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = 0.02


def problems(small):
    from bench import lq_mats
    from ilqr_amd import capi
    rng = np.random.default_rng(1234)
    B = 256 if small else 8192
    yield dict(name="lq 32x16", B=B, T=40 if small else 200, iters=3, nu=16, nys=(8, 32),
               ctor=dict(model="lq", lq=lq_mats(32, 16), u_min=-1.0, u_max=1.0, flags=capi.FLAG_ANALYTIC_DERIVATIVES), x0=rng.uniform(-1, 1, size=(B, 32)))
    B = 256 if small else 4096
    yield dict(name="acrobot", B=B, T=99 if small else 499, iters=20, nu=1, nys=(2,), ctor=dict(model="acrobot", u_min=-1.5, u_max=1.5),
               x0=rng.uniform(-1, 1, size=(B, 4)) * np.array([np.pi, np.pi, 1.0, 1.0]))


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

    say("bench_estimator: %s, fp64, %d timings per row after 3 warm-up calls, the rows in turn" % (torch.cuda.get_device_properties(0).name, args.reps))
    for p in problems(args.small):
        B, T, nu = p["B"], p["T"], p["nu"]
        ctor = dict(p["ctor"])
        g = BatchILQR(ctor.pop("model"), B, T, DT, stream=sp, **ctor)
        n = g.nx
        g.init_traj(p["x0"], np.zeros((B, T, nu)))
        g.iterate(p["iters"])
        g.compute_derivatives()
        g.synchronize()
        f64 = dict(dtype=torch.float64, device="cuda")
        eye = lambda q, s: (s * torch.eye(q, **f64)).repeat(B, 1, 1).contiguous()
        P0, W = eye(n, 0.5), eye(n, 0.01)
        J = torch.empty((B,), **f64)
        info = torch.zeros((B,), dtype=torch.int32, device="cuda")
        rows = {"backward pass": lambda: g._check(g.lib.ilqr_backward_pass(g.h, None)),
                "covariance": lambda: g.copy_covariance_to_device(0, 1, P0.data_ptr(), W.data_ptr(), expected_cost_ptr=J.data_ptr())}
        keep = []
        for ny in p["nys"]:
            H = (torch.randn((B, n, ny), **f64) / n ** 0.5).contiguous()  # memory: column-major ny x nx
            V = eye(ny, 0.1)
            L = torch.empty((B, T + 1, ny, n), **f64)
            keep += [H, V, L]
            rows["filter %d" % ny] = lambda ny=ny, H=H, V=V, L=L: g.copy_estimator_to_device(0, T + 1, ny, H.data_ptr(), V.data_ptr(), P0.data_ptr(), W.data_ptr(),
                                                                                             L_ptr=L.data_ptr(), info_ptr=info.data_ptr())
            rows["filter+loop %d" % ny] = lambda ny=ny, H=H, V=V, L=L: g.copy_estimator_to_device(0, T + 1, ny, H.data_ptr(), V.data_ptr(), P0.data_ptr(),
                                                                                                  W.data_ptr(), L_ptr=L.data_ptr(),
                                                                                                  expected_cost_ptr=J.data_ptr(), info_ptr=info.data_ptr())
        ms = {name: [] for name in rows}
        for rep in range(args.reps + 3):
            for name, fn in rows.items():
                t = timed(fn)
                if rep >= 3:
                    ms[name].append(t)
        failed = int((info != 0).sum())
        say("%s: nx=%d nu=%d T=%d B=%d, the policy of %d iterations; trajectories the last call reported as failed: %d" % (p["name"], n, nu, T, B, p["iters"], failed))
        out = rec["problems"][p["name"]] = dict(B=B, T=T, nx=n, nu=nu, failed=failed, rows={})
        for name, v in ms.items():
            s = dict(median=statistics.median(v), min=min(v), max=max(v))
            out["rows"][name] = s
            say("  %-18s GPU %9.4f ms median (%.4f .. %.4f)  %8.2f ps per trajectory-knot  %5.2f x backward pass" %
                (name, s["median"], s["min"], s["max"], 1e9 * s["median"] / (B * T), s["median"] / statistics.median(ms["backward pass"])))
        g.close()
        del rows, keep, P0, W, J
        torch.cuda.empty_cache()
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
