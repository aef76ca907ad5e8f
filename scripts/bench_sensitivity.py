"""What the tangent and the adjoint of the stored closed loop cost (ilqr_copy_tangent_to_device / ilqr_copy_adjoint_to_device; k_tangent_t,
k_adjoint_t / k_tangent_w, k_adjoint_w) beside the covariance and the value model of the same handle (ilqr_copy_covariance_to_device,
ilqr_copy_value_to_device), which stream a superset of the same records.

  python scripts/bench_sensitivity.py [--reps 30] [--small] [--out profiles/sensitivity_bench.txt]

Two problems: the headline acrobot (T = 499, B = 4096, limits +-1.5, fp64, the policy of 20 iterations) and configs[4] (the LQ model,
n = 32, m = 16, T = 200, B = 8192, fp64, exact derivatives, the policy of 3 iterations).  Per problem, every call between two HIP events
on the handle's stream, median (min .. max) of --reps timings after 3 warm-up calls (the first of which materialises the records), the
rows taking their calls in turn:

  value           Vx[0], Vxx[0]: the whole backward recursion, one knot written
  covariance      Sigma[T] and the expected cost: the whole forward recursion, one knot written
  tangent S       S directions of dx0 to dxs[T]: the whole forward recursion, one knot written (the record stream alone)
  tangent S all   dx0 and dv of the whole horizon to every dxs[t] and dus[t] (the caller's arrays included)
  adjoint S       S cotangents gx[T] to g_x0: the whole backward recursion, one knot read and one written
  adjoint S all   gx and gu of the whole horizon to g_x0 and every g_v[t]
for S = 1, 16 and nx.  No pass/fail threshold.  --small: B = 256 and short horizons, to try the script out."""
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
    B = 256 if small else 4096
    yield dict(name="acrobot", B=B, T=99 if small else 499, iters=20, nu=1, ctor=dict(model="acrobot", u_min=-1.5, u_max=1.5),
               x0=rng.uniform(-1, 1, size=(B, 4)) * np.array([np.pi, np.pi, 1.0, 1.0]))
    B = 256 if small else 8192
    yield dict(name="configs[4]", B=B, T=40 if small else 200, iters=3, nu=16,
               ctor=dict(model="lq", lq=lq_mats(32, 16), u_min=-1.0, u_max=1.0, flags=capi.FLAG_ANALYTIC_DERIVATIVES), x0=rng.uniform(-1, 1, size=(B, 32)))


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

    say("bench_sensitivity: %s, fp64, %d timings per row after 3 warm-up calls, the rows in turn" % (torch.cuda.get_device_properties(0).name, args.reps))
    for p in problems(args.small):
        B, T, nu = p["B"], p["T"], p["nu"]
        ctor = dict(p["ctor"])
        g = BatchILQR(ctor.pop("model"), B, T, DT, stream=sp, **ctor)
        n = g.nx
        g.init_traj(p["x0"], np.zeros((B, T, nu)))
        g.iterate(p["iters"])
        g.synchronize()
        f64 = dict(dtype=torch.float64, device="cuda")
        S0 = (0.1 * torch.eye(n, **f64)).repeat(B, 1, 1).contiguous()
        W = (0.001 * torch.eye(n, **f64)).repeat(B, 1, 1).contiguous()
        Vx, Vxx = torch.empty((B, 1, n), **f64), torch.empty((B, 1, n * n), **f64)
        Sg, J = torch.empty((B, 1, n * n), **f64), torch.empty((B,), **f64)
        rows = {"value": lambda: g.copy_value_to_device(0, 1, Vx.data_ptr(), Vxx.data_ptr()),
                "covariance": lambda: g.copy_covariance_to_device(T, 1, S0.data_ptr(), W.data_ptr(), Sg.data_ptr(), None, J.data_ptr())}
        # the caller's arrays, sized for the most directions and shared by every S (a smaller S uses a prefix): one state-sized pair for one
        # knot; over the horizon one state-sized array (dxs out, then gx in: finite whatever the tangent left) and two control-sized ones
        # (dv / gu in, random; dus / g_v out)
        Smax = max(16, n)
        x_one, x_out = torch.randn((B * Smax * n,), **f64), torch.empty((B * Smax * n,), **f64)
        x_all = torch.randn((B * (T + 1) * Smax * n,), **f64)
        u_in, u_all = 0.1 * torch.randn((B * T * Smax * nu,), **f64), torch.empty((B * T * Smax * nu,), **f64)
        for S in sorted({1, 16, n}):
            rows["tangent %d" % S] = lambda S=S: g.copy_tangent_to_device(T, 1, S, x_one.data_ptr(), None, x_out.data_ptr(), None)
            rows["tangent %d all" % S] = lambda S=S: g.copy_tangent_to_device(0, T + 1, S, x_one.data_ptr(), u_in.data_ptr(), x_all.data_ptr(), u_all.data_ptr())
            rows["adjoint %d" % S] = lambda S=S: g.copy_adjoint_to_device(T, 1, S, x_one.data_ptr(), None, x_out.data_ptr(), None)
            rows["adjoint %d all" % S] = lambda S=S: g.copy_adjoint_to_device(0, T + 1, S, x_all.data_ptr(), u_in.data_ptr(), x_out.data_ptr(), u_all.data_ptr())
        ms = {name: [] for name in rows}
        for rep in range(args.reps + 3):
            for name, fn in rows.items():
                t = timed(fn)
                if rep >= 3:
                    ms[name].append(t)
        assert bool(torch.isfinite(J).all()) and bool(torch.isfinite(x_out).all()) and bool(torch.isfinite(u_all).all())
        say("%s: nx=%d nu=%d T=%d B=%d, the policy of %d iterations" % (p["name"], n, nu, T, B, p["iters"]))
        out = rec["problems"][p["name"]] = dict(B=B, T=T, nx=n, nu=nu, rows={})
        for name, v in ms.items():
            s = dict(median=statistics.median(v), min=min(v), max=max(v))
            out["rows"][name] = s
            say("  %-16s GPU %9.4f ms median (%.4f .. %.4f)  %8.2f ps per trajectory-knot  %5.2f x covariance" %
                (name, s["median"], s["min"], s["max"], 1e9 * s["median"] / (B * T), s["median"] / statistics.median(ms["covariance"])))
        g.close()
        del rows, x_one, x_out, x_all, u_in, u_all
        torch.cuda.empty_cache()
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
