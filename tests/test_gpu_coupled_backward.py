"""Every stage backward kernel on records whose state-control block cxu is dense and as large as cxx and cuu (tests/coupled.py),
teacher-forced against the oracle's backward pass with the same per-control limits, at lambda 1 and 1e-3.

Every backward kernel starts Qux from cxu'; both shipped nx = 4 models and the LQ twin have cxu = 0, so until these tests a wrong stride,
a missing transpose, a dropped term or a wrong sign in any of those reads left the suite green.  tests/test_coupled_inputs.py proves on
the CPU that the reference itself needs none of the allowances of tests/parity.py on these inputs and that the gains move by >= 25 % per
knot on every trajectory under either mistake: a kernel that misses the project's tolerances here is wrong.

  k_backward_q, k_backward_t   acrobot (nu = 1) and double-integrator (nu = 2) handles, fp64 and fp32 (float records, the float twin)
  k_backward_w3, k_backward_w2 host handles at (32,16), (17,9), (6,2), (31,1), (3,1); the two against each other at 1e-9
  two control tiles            ILQR_ROUTE_TWO_CONTROL_TILES at (12,16), (32,16) against one tile; nu > 16 at (20,17), (24,20), (32,32)
  ILQR_FLAG_REGULARIZE_VXX     k_backward_w3<.., REGV> at (32,16), (6,2); k_backward_q / k_backward_t on both nx = 4 handles
Worst per-knot error of the gains against the oracle over every case, measured on an MI355X (each test prints its own): k_backward_q and
k_backward_t 2.8e-14 (REGV 5.1e-14), in fp32 0 -- the bits of the float twin; k_backward_w3 1.4e-13 (REGV 4.4e-14), k_backward_w2
1.1e-13; two control tiles 1.9e-15 with ONE trajectory a proven clamp tie: (20,17), seed 1, lambda 1e-3, trajectory 7, knot 7, control 1.
There both sides find the same k to 1e-16, 3.4e-5 inside the box-QP's 1e-4 band of the upper bound; the oracle leaves the control free,
the kernel clamps it (K row 0): at a converged free control the gradient is zero to rounding, and its sign is what boxqp.cpp:65-71 asks.
No other pass used a tie or the conditioning allowance."""
import numpy as np
import pytest

from tests import coupled
from tests.coupled import B, T, LAMBDAS, SEEDS
from tests.parity import check_backward, gains_knot_err

pytestmark = pytest.mark.gpu
DT = 0.02
NX4 = {1: "acrobot", 2: "double_integrator"}


def _name(g):
    from ilqr_amd import capi
    return g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index("backward"))


def run(oracle, g, n, m, seed, dtype="f64", kernel=None, fixes=0):
    """Both lambdas of one (handle, shape, seed): records in, the round trip of cxu to the bit, the pass, the gains in their boxes, and
    check_backward at the project's tolerance with max_ties = max_over10 = 2.  Returns {lam: device outputs}."""
    from tests.test_gpu_control_limits import Invariants
    f32 = dtype == "f32"
    rec, lo, hi, us, k_prev = coupled.case(n, m, seed, f32=f32)
    om = coupled.box_model(oracle, n, m, lo, hi)
    if kernel is not None:
        assert _name(g) == kernel, _name(g)
    inv = Invariants(lo, hi, dtype)
    out = {}
    for lam in LAMBDAS:
        g.set_trajectory(x0=np.zeros((B, n)), xs=np.zeros((B, T + 1, n)), us=us, cost=np.ones(B))
        g.set_derivatives(**rec)
        g.set_gains(k=k_prev, K=np.zeros((B, T, m, n)))
        g.set_lambda(lam, 1.0)
        back = g.derivatives()
        assert np.array_equal(back["cxu"], rec["cxu"]) and np.abs(back["cxu"]).min() > 0
        div = g.backward_pass()
        k, K = g.gains()
        dV = g.dV()
        inv.gains(us, k, K, div == 0)
        oracle.set_fixes(fixes)
        try:
            ro = coupled.oracle_backward(oracle, om, us, rec, k_prev, lam, "f32" if f32 else "f64")
            r = check_backward(oracle, om, us, coupled.memory_layout(rec), k_prev, lam, k, K, dV, div, ro, max_ties=2, max_over10=2, precision=dtype)
        finally:
            oracle.set_fixes(0)
        e = gains_knot_err(k, K, ro["k"], ro["Km"], us)
        print("coupled backward %s %s (%d,%d) seed %d lambda %g%s: worst per-knot error %.2e, median %.2e, ties %d, conditioned %d, clamped %.2f" % (
            _name(g).decode(), dtype, n, m, seed, lam, " REGV" if fixes else "", e.max(), np.median(e), r["ties"], r["conditioned"], coupled.clamped_share(K)))
        assert np.all(div == 0) and r["good"].sum() >= B - 2
        out[lam] = dict(k=k, K=K, dV=dV, gnorm=g.gnorm(), div=div, ro=ro)
    inv.done(min_checked=B)
    return out


def _nx4(m, dtype, thread, lo, hi, flags=0):
    from ilqr_amd import BatchILQR, capi
    kw = dict(goal=[1.0, 0.5, 0.0, 0.0]) if m == 2 else {}
    # (UNFUSED: an nx = 4 handle then names the stage call's own kernel)
    return BatchILQR(NX4[m], B, T, DT, u_min=lo, u_max=hi, dtype=dtype, flags=flags | capi.FLAG_UNFUSED | (capi.FLAG_BACKWARD_THREAD_PER_TRAJ if thread else 0), **kw)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kernel", ["k_backward_q", "k_backward_t"])
@pytest.mark.parametrize("m", [1, 2])
def test_nx4_stage_kernels(oracle, m, kernel, dtype, seed):
    """cxu is a 4-vector at nu = 1 -- no transpose to get wrong -- and a 4 x 2 block at nu = 2."""
    lo, hi = coupled.case(4, m, seed, f32=dtype == "f32")[1:3]
    g = _nx4(m, dtype, kernel == "k_backward_t", lo, hi)
    run(oracle, g, 4, m, seed, dtype=dtype, kernel=kernel.encode())
    g.close()


def _close(a, b, what):
    """the bound of test_default_kernel_against_the_literal_order_kernel: 1e-9 max(1, max|.|) on k, K, dV, gnorm, equal div"""
    for lam in LAMBDAS:
        assert np.array_equal(a[lam]["div"], b[lam]["div"])
        for key in ("k", "K", "dV", "gnorm"):
            scale = max(1.0, np.abs(a[lam][key]).max())
            d = np.abs(a[lam][key] - b[lam][key]).max()
            assert d <= 1e-9 * scale, (what, lam, key, d, scale)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", coupled.HOST_SHAPES)
def test_wave_kernels(oracle, n, m, seed):
    """k_backward_w3 (with its m = 1 and m = 2 shortcuts, one and two state tiles, masked and full records) and the literal-order
    k_backward_w2, each against the oracle and the two against each other."""
    from ilqr_amd import BatchILQR, capi
    lo, hi = coupled.case(n, m, seed)[1:3]
    outs = []
    for route, kernel in ((0, b"k_backward_w3"), (capi.ROUTE_BACKWARD_W2, b"k_backward_w2")):
        g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=lo, u_max=hi, route=route)
        outs.append(run(oracle, g, n, m, seed, kernel=kernel))
        g.close()
    _close(outs[0], outs[1], "w3 against w2")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", coupled.TWO_TILE_SHAPES)
def test_two_control_tiles_by_route_bit(oracle, n, m, seed):
    """ILQR_ROUTE_TWO_CONTROL_TILES: m = 16 through the two-tile kernel (second tile empty) against the oracle and the one-tile result."""
    from ilqr_amd import BatchILQR, capi
    lo, hi = coupled.case(n, m, seed)[1:3]
    outs = []
    for route, kernel in ((0, b"k_backward_w3"), (capi.ROUTE_TWO_CONTROL_TILES, b"k_backward_w3w")):
        g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=lo, u_max=hi, route=route)
        outs.append(run(oracle, g, n, m, seed, kernel=kernel))
        g.close()
    _close(outs[0], outs[1], "two tiles against one")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", coupled.WIDE_SHAPES)
def test_more_than_16_controls(oracle, n, m, seed):
    """nu > 16: cxu spans both control tiles, the second one partly (17, 20) or wholly (32) filled."""
    from ilqr_amd import BatchILQR
    lo, hi = coupled.case(n, m, seed)[1:3]
    g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=lo, u_max=hi)
    run(oracle, g, n, m, seed, kernel=b"k_backward_w3w")
    g.close()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m,kernel", [(32, 16, "k_backward_w3"), (6, 2, "k_backward_w3"), (4, 1, "k_backward_q"), (4, 2, "k_backward_q"),
                                        (4, 1, "k_backward_t"), (4, 2, "k_backward_t")])
def test_vxx_regularisation(oracle, n, m, kernel, seed):
    """ILQR_FLAG_REGULARIZE_VXX: Qux_reg = cxu' + fu'(Vxx' + lambda I) fx, the value update on the unregularised Qux -- against the oracle
    under set_fixes(4), and it IS another regularisation: the result differs from the oracle's with lambda I on Quu."""
    from ilqr_amd import BatchILQR, capi
    rec, lo, hi, us, k_prev = coupled.case(n, m, seed)
    if n == 4:
        g = _nx4(m, "f64", kernel == "k_backward_t", lo, hi, flags=capi.FLAG_REGULARIZE_VXX)
    else:
        g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=lo, u_max=hi, flags=capi.FLAG_REGULARIZE_VXX)
    out = run(oracle, g, n, m, seed, kernel=kernel.encode(), fixes=4)
    g.close()
    om = coupled.box_model(oracle, n, m, lo, hi)
    for lam in LAMBDAS:
        r0 = coupled.oracle_backward(oracle, om, us, rec, k_prev, lam)
        ro = out[lam]["ro"]
        moved = max(np.abs(r0["Km"] - ro["Km"]).max(), np.abs(r0["k"] - ro["k"]).max())
        assert moved > 100 * 1e-6 * max(np.abs(ro["Km"]).max(), np.abs(ro["k"]).max()), (lam, moved)  # (far beyond the tolerance the device met)
        assert np.abs(out[lam]["K"] - r0["Km"]).max() > 50 * 1e-6 * np.abs(ro["Km"]).max()
