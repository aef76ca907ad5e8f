"""The CPU reference of per-knot model parameters (ilqr_set_knot_params), shared by tests/test_knot_params_abi.py -- which proves it on the
CPU against the oracle's own batch functions -- and tests/test_gpu_knot_params.py.  One oracle twin PER (trajectory, knot); a rollout is
stepped through the twins' point functions (cost / integrate / final_cost), knot t under twin t, the final cost under twin T; a record is
the oracle's own finite-difference sweep on a two-knot slice under the twin of the knot it describes.  No test in this file."""
import numpy as np

from tests.test_gpu_user_chain import NL


def knot_window(p, k0, T):
    """The gather of ilqr_set_knot_params in numpy: row t of the window is row min(k0 + t, n_knots - 1) of p [B][n_knots][NTP]."""
    p = np.asarray(p)
    n_knots = p.shape[1]
    assert 0 <= k0 < n_knots
    return np.ascontiguousarray(p[:, np.minimum(k0 + np.arange(T + 1), n_knots - 1)])


def knot_twins(oracle, rows, lim):
    """rows [B][T+1][8] -> twins[b][t], one oracle pendulum chain per (trajectory, knot), in the oracle's current flavour."""
    return [[oracle.Model("chain", chain=(NL, rows[b, t]), u_lim=lim) for t in range(rows.shape[1])] for b in range(rows.shape[0])]


def knot_rollout(twins, x0, u, dt, xs_nom=None, k=None, K=None, alpha=0.0, clamp=None, t0=0, n=None):
    """orc_forward_pass with knot t evaluated under twins[b][t]: from x0 [B][nx] at knot t0 through n knots (default: to the horizon's end),
    u_t = u[b, t] + alpha k[b, t] + K[b, t] (x_t - xs_nom[b, t]) (K [B][T][nu][nx]; each sum over the state index ascending from zero, as the
    oracle and the kernels form it), clamped to clamp = (lo, hi) when given.  The cost is summed in ascending knot order in double and
    takes twin T's final cost when the rollout reaches knot T.  Returns xs [B][n+1][nx], us [B][n][nu], cost [B]; knots and arithmetic in
    the precision of the twins' flavour."""
    B, T = len(twins), len(twins[0]) - 1
    n = T - t0 if n is None else n
    rt = np.float32 if twins[0][0].flavour == "f32" else np.longdouble if twins[0][0].flavour == "f80" else np.float64
    x0, u = np.asarray(x0, dtype=rt), np.asarray(u, dtype=rt)
    nx, nu = x0.shape[1], u.shape[2]
    xs, us, cost = np.zeros((B, n + 1, nx), dtype=rt), np.zeros((B, n, nu), dtype=rt), np.zeros(B)
    for b in range(B):
        x, total = x0[b].copy(), 0.0
        for i in range(n):
            t = t0 + i
            m = twins[b][t]
            ut = u[b, t].copy()
            if k is not None:
                ut = ut + np.asarray(k[b, t], dtype=rt) * rt(alpha)
            if K is not None:
                d = x - np.asarray(xs_nom[b, t], dtype=rt)
                Kt = np.asarray(K[b, t], dtype=rt)
                acc = np.zeros(nu, dtype=rt)
                for j in range(nx):
                    acc = acc + Kt[:, j] * d[j]
                ut = ut + acc
            if clamp is not None:
                ut = np.minimum(np.maximum(ut, np.asarray(clamp[0], dtype=rt)), np.asarray(clamp[1], dtype=rt))
            xs[b, i], us[b, i] = x, ut
            total += float(m.cost(x, ut))
            x = m.integrate(x, ut, dt)
        xs[b, n] = x
        if t0 + n == T:
            total += float(twins[b][T].final_cost(x))
        cost[b] = total
    return xs, us, cost


def knot_records(twins, xs, us, dt):
    """The derivative records under per-knot twins, in oracle.batch_derivatives' memory layout [B][T+1][col][row]: a running knot t is
    record 0 of the two-knot slice (xs[t : t + 2], us[t : t + 1]) under twin t; knot T is record 1 of the last slice under twin T."""
    from oracle import oracle
    B, T = len(twins), len(twins[0]) - 1
    out = None
    for b in range(B):
        for t in range(T + 1):
            s = min(t, T - 1)
            d = oracle.batch_derivatives(twins[b][t], xs[b:b + 1, s:s + 2], us[b:b + 1, s:s + 1], dt)
            if out is None:
                out = {key: np.zeros((B, T + 1) + a.shape[2:], dtype=a.dtype) for key, a in d.items()}
            for key, a in d.items():
                out[key][b, t] = a[0, t - s]
    return out
