"""What ilqr_copy_risk_sensitive_to_device costs (k_risk_w / k_risk_t) beside one ilqr_solve_lq_on_device(n_dirs = 1) of the same handle,
whose gain sweep does the same Riccati step without the noise adjustment.

  python scripts/bench_risk.py [--reps 30] [--small] [--out profiles/risk_bench.txt]

Two problems: the LQ model (n = 32, m = 16, T = 200, B = 8192, fp64, exact derivatives, the policy of 3 iterations) at nw = 1, 16 and 32
noise directions and the headline acrobot (T = 499, B = 4096, limits +-1.5, fp64, the policy of 20 iterations, mu = 1) at nw = 2.  Per
problem, every call between two HIP events on the handle's stream, median (min .. max) of --reps timings after 3 warm-up calls (the first
of which materialises the records and allocates the scratch), the rows taking their calls in turn:

  lq_solve 1          ilqr_solve_lq_on_device, one direction, gx and gu to dus (the gain sweep and the two direction sweeps)
  risk nw             C to K and k of every knot, theta = 0.5, ILQR_LQ_HOLD_CLAMPED
  risk nw +Vxx        the same plus Vxx of every knot
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
THETA = 0.5


def problems(small):
    from bench import lq_mats
    from ilqr_amd import capi
    rng = np.random.default_rng(1234)
    B = 256 if small else 8192
    yield dict(name="lq 32x16", B=B, T=40 if small else 200, iters=3, nu=16, nws=(1, 16, 32), mu=0.0, noise=0.005,
               ctor=dict(model="lq", lq=lq_mats(32, 16), u_min=-1.0, u_max=1.0, flags=capi.FLAG_ANALYTIC_DERIVATIVES), x0=rng.uniform(-1, 1, size=(B, 32)))
    B = 256 if small else 4096
    yield dict(name="acrobot", B=B, T=99 if small else 499, iters=20, nu=1, nws=(2,), mu=1.0, noise=1e-5, ctor=dict(model="acrobot", u_min=-1.5, u_max=1.5),
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
    lines, rec = [], {"reps": args.reps, "theta": THETA, "problems": {}}

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

    say("bench_risk: %s, fp64, theta = %g, %d timings per row after 3 warm-up calls, the rows in turn" %
        (torch.cuda.get_device_properties(0).name, THETA, args.reps))
    for p in problems(args.small):
        B, T, nu, mu = p["B"], p["T"], p["nu"], p["mu"]
        ctor = dict(p["ctor"])
        g = BatchILQR(ctor.pop("model"), B, T, DT, stream=sp, **ctor)
        n = g.nx
        g.init_traj(p["x0"], np.zeros((B, T, nu)))
        g.iterate(p["iters"])
        g.compute_derivatives()
        g.synchronize()
        f64 = dict(dtype=torch.float64, device="cuda")
        gx, gu = torch.randn((B, T + 1, 1, n), **f64), torch.randn((B, T, 1, nu), **f64)
        dus = torch.empty((B, T, 1, nu), **f64)
        K, k, Vxx = torch.empty((B, T, n, nu), **f64), torch.empty((B, T, nu), **f64), torch.empty((B, T + 1, n, n), **f64)
        info = {nw: torch.zeros((B,), dtype=torch.int32, device="cuda") for nw in p["nws"]}
        info_lq = torch.zeros((B,), dtype=torch.int32, device="cuda")
        rows = {"lq_solve 1": lambda: g.copy_lq_solve_to_device(1, mu, True, gx_ptr=gx.data_ptr(), gu_ptr=gu.data_ptr(), dus_ptr=dus.data_ptr(),
                                                                info_ptr=info_lq.data_ptr())}
        keep = []
        for nw in p["nws"]:
            C = (p["noise"] * torch.randn((B, nw, n), **f64) / n ** 0.5).contiguous()  # memory: column-major nx x nw
            keep.append(C)
            rows["risk %d" % nw] = lambda nw=nw, C=C: g.copy_risk_sensitive_to_device(nw, THETA, C.data_ptr(), mu=mu, hold_clamped=True, K_ptr=K.data_ptr(),
                                                                                     k_ptr=k.data_ptr(), info_ptr=info[nw].data_ptr())
            rows["risk %d +Vxx" % nw] = lambda nw=nw, C=C: g.copy_risk_sensitive_to_device(nw, THETA, C.data_ptr(), mu=mu, hold_clamped=True,
                                                                                          K_ptr=K.data_ptr(), k_ptr=k.data_ptr(), Vxx_ptr=Vxx.data_ptr(),
                                                                                          info_ptr=info[nw].data_ptr())
        ms = {name: [] for name in rows}
        for rep in range(args.reps + 3):
            for name, fn in rows.items():
                t = timed(fn)
                if rep >= 3:
                    ms[name].append(t)
        failed = {nw: dict(breakdown=int((info[nw] < 0).sum()), quu=int((info[nw] > 0).sum())) for nw in p["nws"]}
        say("%s: nx=%d nu=%d T=%d B=%d mu=%g, noise scale %g, the policy of %d iterations; trajectories the last calls reported as failed: "
            "lq_solve %d, risk by nw %s" % (p["name"], n, nu, T, B, mu, p["noise"], p["iters"], int((info_lq != 0).sum()), failed))
        out = rec["problems"][p["name"]] = dict(B=B, T=T, nx=n, nu=nu, failed=failed, rows={})
        base = statistics.median(ms["lq_solve 1"])
        for name, v in ms.items():
            s = dict(median=statistics.median(v), min=min(v), max=max(v), ratio=statistics.median(v) / base)
            out["rows"][name] = s
            say("  %-14s GPU %9.4f ms median (%.4f .. %.4f)  %8.2f ps per trajectory-knot  %5.2f x lq_solve" %
                (name, s["median"], s["min"], s["max"], 1e9 * s["median"] / (B * T), s["ratio"]))
        g.close()
        del rows, keep, gx, gu, dus, K, k, Vxx
        torch.cuda.empty_cache()
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
