"""What ilqr_solve_lq_on_device costs (k_lq_gain_t, k_lq_dir_t / k_lq_gain_w, k_lq_back_w, k_lq_fwd_w) beside one ilqr_backward_pass, one
ilqr_copy_tangent_to_device and one ilqr_copy_adjoint_to_device of the same handle, which together do comparable algebra: a Riccati sweep
over the same records, a backward and a forward sweep over the caller's directions.

  python scripts/bench_lq_solve.py [--reps 30] [--small] [--out profiles/lq_solve_bench.txt]

Two problems: the headline acrobot (T = 499, B = 4096, limits +-1.5, fp64, the policy of 20 iterations) at 1, 4 and 16 directions and the LQ
model (n = 32, m = 16, T = 200, B = 8192, fp64, exact derivatives, the policy of 3 iterations) at 1 and 16 directions.  Per problem, every
call between two HIP events on the handle's stream, median (min .. max) of --reps timings after 3 warm-up calls (the first of which
materialises the records and allocates the scratch), the rows taking their calls in turn:

  backward pass     ilqr_backward_pass: the solver's own Riccati sweep with its box-QP (it rewrites k, K: the held set of later calls)
  tangent S all     dx0 and dv of the whole horizon to every dxs[t] and dus[t]
  adjoint S all     gx and gu of the whole horizon to g_x0 and every g_v[t]
  lq_solve S        dx0, gx, gu to dxs, dus (mu = 1 on the acrobot, whose finite-difference cuu is not definite everywhere; else 0;
                    ILQR_LQ_HOLD_CLAMPED)
  lq_solve S dlam   the same with dlam: P[t] is stored and read back, one more state-sized array goes out
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
    B = 256 if small else 4096
    yield dict(name="acrobot", B=B, T=99 if small else 499, iters=20, nu=1, dirs=(1, 4, 16), mu=1.0, ctor=dict(model="acrobot", u_min=-1.5, u_max=1.5),
               x0=rng.uniform(-1, 1, size=(B, 4)) * np.array([np.pi, np.pi, 1.0, 1.0]))
    B = 256 if small else 8192
    yield dict(name="lq 32x16", B=B, T=40 if small else 200, iters=3, nu=16, dirs=(1, 16), mu=0.0,
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

    say("bench_lq_solve: %s, fp64, %d timings per row after 3 warm-up calls, the rows in turn" % (torch.cuda.get_device_properties(0).name, args.reps))
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
        # the caller's arrays, sized for the most directions and shared by every S (a smaller S uses a prefix)
        Smax = max(p["dirs"])
        x0_in, x0_out = torch.randn((B * Smax * n,), **f64), torch.empty((B * Smax * n,), **f64)
        gx_in = torch.randn((B * (T + 1) * Smax * n,), **f64)
        gu_in = torch.randn((B * T * Smax * nu,), **f64)
        dxs, dlam = torch.empty((B * (T + 1) * Smax * n,), **f64), torch.empty((B * (T + 1) * Smax * n,), **f64)
        dus = torch.empty((B * T * Smax * nu,), **f64)
        info = torch.zeros((B,), dtype=torch.int32, device="cuda")
        rows = {"backward pass": lambda: g._check(g.lib.ilqr_backward_pass(g.h, None))}
        for S in p["dirs"]:
            rows["tangent %d all" % S] = lambda S=S: g.copy_tangent_to_device(0, T + 1, S, x0_in.data_ptr(), gu_in.data_ptr(), dxs.data_ptr(), dus.data_ptr())
            rows["adjoint %d all" % S] = lambda S=S: g.copy_adjoint_to_device(0, T + 1, S, gx_in.data_ptr(), gu_in.data_ptr(), x0_out.data_ptr(), dus.data_ptr())
            rows["lq_solve %d" % S] = lambda S=S: g.copy_lq_solve_to_device(S, mu, True, x0_in.data_ptr(), gx_in.data_ptr(), gu_in.data_ptr(), dxs.data_ptr(),
                                                                           dus.data_ptr(), None, info.data_ptr())
            rows["lq_solve %d dlam" % S] = lambda S=S: g.copy_lq_solve_to_device(S, mu, True, x0_in.data_ptr(), gx_in.data_ptr(), gu_in.data_ptr(),
                                                                                dxs.data_ptr(), dus.data_ptr(), dlam.data_ptr(), info.data_ptr())
        ms = {name: [] for name in rows}
        for rep in range(args.reps + 3):
            for name, fn in rows.items():
                t = timed(fn)
                if rep >= 3:
                    ms[name].append(t)
        failed = int((info != 0).sum())
        say("%s: nx=%d nu=%d T=%d B=%d, the policy of %d iterations, mu = %g; trajectories the last lq_solve reported as not positive definite: %d" %
            (p["name"], n, nu, T, B, p["iters"], mu, failed))
        out = rec["problems"][p["name"]] = dict(B=B, T=T, nx=n, nu=nu, mu=mu, not_positive_definite=failed, rows={})
        for name, v in ms.items():
            s = dict(median=statistics.median(v), min=min(v), max=max(v))
            out["rows"][name] = s
            say("  %-18s GPU %9.4f ms median (%.4f .. %.4f)  %8.2f ps per trajectory-knot  %5.2f x backward pass" %
                (name, s["median"], s["min"], s["max"], 1e9 * s["median"] / (B * T), s["median"] / statistics.median(ms["backward pass"])))
        g.close()
        del rows, x0_in, x0_out, gx_in, gu_in, dxs, dus, dlam
        torch.cuda.empty_cache()
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n" + json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
