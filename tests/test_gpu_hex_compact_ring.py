"""k_solve_hex keeps a COMPACT record per knot in its LDS rings for a model whose running cost ignores the state (the acrobot:
state_free_running_cost, csrc/models.hpp): fx, fu, cu, cuu, the control and its weight, and one number Z = c - c in place of the
24 entries of cx, cxx and cxu, which are all that number times a constant; knot T's cx and cxx travel beside the ring.  The
two-kernel route (ILQR_FLAG_UNFUSED) still writes and reads the full Rec<4,1> in HBM.  Both must leave the same state TO THE BIT
-- compared as raw bit patterns, so that a sign of zero counts: fp64 and fp32, finite differences and the model's exact
derivatives, a ragged batch, one tile and the flagship's 4096, horizons on and off the producers' 16-knot rounds, narrow and
wide limits, iteration by iteration and through the rest of the solve (where the lambda retries and the slow box-QP exits are)."""
import numpy as np
import pytest

from tests.util import acrobot_x0

pytestmark = pytest.mark.gpu
DT = 0.02
RETRIES = {}  # case -> (trajectory, iteration) pairs in which STEP 2 retried, summed over the module (reported by the last test)


def bits(a, dtype):
    """the raw bit pattern of a float array the getters hand out as float64 (a float handle's values widen and narrow exactly)"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    return a.view(np.uint64) if dtype == "f64" else a.astype(np.float32).view(np.uint32)


def scalars(g):
    st, it, al = g.status()
    lam, dlam = g.lambdas()
    dV = g.dV()
    return dict(cost=g.cost(), dV0=dV[:, 0].copy(), dV1=dV[:, 1].copy(), lam=lam, dlam=dlam, st=st, it=it, al=al)


def arrays(g):
    xs, us = g.trajectory()
    k, K = g.gains()
    return dict(xs=xs, us=us, k=k, K=K)


def assert_same_bits(a, b, dtype, what):
    assert a.keys() == b.keys()
    for n in a:
        # lambda, dlambda and dV are doubles in a float handle too
        dt = "f64" if n in ("lam", "dlam", "dV0", "dV1") or n.endswith(("_lam", "_dlam", "_dV0", "_dV1")) else dtype
        x, y = bits(a[n], dt), bits(b[n], dt)
        if not np.array_equal(x, y):
            bad = np.argwhere(x != y)
            raise AssertionError("%s: %s differs in %d of %d entries, first at %s: %r / %r" % (what, n, len(bad), x.size, bad[0], a[n][tuple(bad[0])], b[n][tuple(bad[0])]))


def count_retries(before, after):
    """An accepted search divides lambda by at least lambda_factor; lambda not below its old value after an accepted search means the
    backward pass raised it first: STEP 2 retried (ilqr_core.cpp:136-150)."""
    run = before["st"] == 0
    return int(np.sum(run & (after["al"] >= 0) & (before["lam"] > 0) & (after["lam"] >= before["lam"])))


def run_case(B, T, lim, dtype, analytic, n_step, finish):
    from ilqr_amd import BatchILQR, capi
    x0 = acrobot_x0(B, scale=0.6, seed=100 + T)
    if dtype == "f32":
        x0 = x0.astype(np.float32).astype(np.float64)
    u0 = np.zeros((B, T, 1))
    base = capi.FLAG_ANALYTIC_DERIVATIVES if analytic else 0
    sv = capi.STAGE_NAMES.index("solve")
    out, retries = [], 0
    for fl in (0, capi.FLAG_UNFUSED):
        g = BatchILQR("acrobot", B, T, DT, u_min=-lim, u_max=lim, flags=base | fl, dtype=dtype, params=dict(max_iter=40))
        if fl == 0:
            assert g.lib.ilqr_stage_kernel_name(g.h, sv) == b"k_solve_hex"
        g.init_traj(x0, u0)
        s = {}
        prev = scalars(g)
        for i in range(n_step):
            g.iterate(1)
            cur = scalars(g)
            if fl == 0:
                retries += count_retries(prev, cur)
            s.update({"%d_%s" % (i, n): a for n, a in cur.items()})
            prev = cur
            if i == 1 or i == n_step - 1:
                s.update({"%d_%s" % (i, n): a for n, a in arrays(g).items()})
        if finish:
            g.generate_trajectory()
            s.update({"end_" + n: a for n, a in scalars(g).items()})
            s.update({"end_" + n: a for n, a in arrays(g).items()})
        out.append(s)
        g.close()
    what = "B=%d T=%d lim=%g %s %s" % (B, T, lim, dtype, "analytic" if analytic else "fd")
    assert_same_bits(out[0], out[1], dtype, what)
    RETRIES[what] = retries
    return out[0]


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("lim", [1.5, 5.0])
@pytest.mark.parametrize("T", [17, 100, 499])
@pytest.mark.parametrize("B", [37, 16])
def test_compact_ring_equals_the_two_kernel_route(B, T, lim, dtype, analytic):
    """a ragged batch (two whole tiles and a sub-tile of one trajectory with a lane to spare) and one tile: twelve iterations one by one,
    then the rest of the solve"""
    s = run_case(B, T, lim, dtype, analytic, n_step=12, finish=True)
    assert np.all(np.isfinite(s["end_cost"]))


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("lim", [1.5, 5.0])
@pytest.mark.parametrize("T", [17, 100, 499])
def test_compact_ring_equals_the_two_kernel_route_at_the_flagship_batch(T, lim, dtype, analytic):
    """B = 4096: a tile on every CU, every ring in use at once; four iterations one by one"""
    run_case(4096, T, lim, dtype, analytic, n_step=4, finish=False)


def test_lambda_retries_were_among_the_cases():
    """(runs last: reports in how many (trajectory, iteration) pairs of the cases above the backward pass retried with a larger lambda)"""
    print("\nSTEP 2 retries per case:", {k: v for k, v in RETRIES.items() if v})
    if not RETRIES:  # (selected on its own)
        run_case(37, 100, 1.5, "f64", False, n_step=12, finish=True)
    assert sum(RETRIES.values()) > 0, "no case reached a lambda retry"
