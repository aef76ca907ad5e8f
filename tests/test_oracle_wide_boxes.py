"""The problems of tests/test_gpu_wide_control_limits.py would expose a kernel that gets a control's limits wrong (CPU, the oracle alone).

A kernel that reads control j - 16's limits for control j >= 16 (folded), forms the box as [-u_max, -u_min] (mirrored) or exchanges the
two control tiles' limits (swapped) computes the oracle's backward pass under those limits instead.  On every problem the GPU tests
use -- same shapes, seeds, boxes, records, starting gains and lambdas -- the oracle's gains under each mutant must differ from its
gains under the true limits by far more than the per-knot tolerance of tests/parity.py's check_backward on most trajectories (more
than check_backward's knife-edge and conditioning allowances could excuse), and every special box (pinned, excluding 0, an edge at 0,
one-sided) must be active on a real share of knots, so that it decides something there."""
import numpy as np
import pytest

from tests.parity import TOL, gains_knot_err
from tests.util import mat
from tests.test_gpu_control_limits import DT
from tests.test_gpu_wide_control_limits import (ABOVE_0, BELOW_0, EDGE_0, LAMBDAS, LOWER_ONLY, NARROW_INF_SHAPES, PINNED, PINNED_0,
                                                UPPER_ONLY, WIDE_HOST_SHAPES, WIDE_LQ_CASES, host_problem, infinite_boxes, wide_boxes,
                                                wide_lq_case)

SPECIAL = (PINNED, ABOVE_0, BELOW_0, EDGE_0, PINNED_0, UPPER_ONLY, LOWER_ONLY)
MARGIN = 100 * TOL      # a mutant's gains must be this far off per knot ...
MOST = 0.75             # ... on at least this share of the trajectories
MIN_ACTIVE = 0.1        # share of knots on which each special box's k sits on one of its edges


def mutants(lo, hi):
    """name -> (lo, hi) a wrong kernel would in effect use; only those that differ from the true limits."""
    m = len(lo)
    out = {"mirrored": (-hi, -lo)}
    if m > 16:
        w = m - 16
        f_lo, f_hi = lo.copy(), hi.copy()
        f_lo[16:], f_hi[16:] = lo[:w], hi[:w]
        out["folded"] = (f_lo, f_hi)
        s_lo, s_hi = f_lo.copy(), f_hi.copy()
        s_lo[:w], s_hi[:w] = lo[16:], hi[16:]
        out["swapped"] = (s_lo, s_hi)
    return {k: v for k, v in out.items() if not (np.array_equal(v[0], lo) and np.array_equal(v[1], hi))}


def check_problem(oracle, om, us, do, k_prev, lam, lo, hi, special_lanes):
    ro = oracle.batch_backward(om, us, do, k_prev=k_prev, lam=lam)
    k, K = ro["k"], mat(ro["K"])
    assert np.all(ro["diverge"] == 0)
    seen = mutants(lo, hi)
    for name, (a, b) in seen.items():
        rm = oracle.batch_backward(oracle.Model("lq", lq=om.lq_arg, u_min=a, u_max=b), us, do, k_prev=k_prev, lam=lam)
        off = gains_knot_err(rm["k"], mat(rm["K"]), k, K, us) > MARGIN
        assert off.mean() >= MOST, (name, lam, off.mean())
    L, H = lo[None, None, :] - us, hi[None, None, :] - us
    active = ((k == L) | (k == H)).mean(axis=(0, 1))
    for j in special_lanes:
        if lo[j] == hi[j]:
            assert active[j] == 1.0, (j, active[j])
        assert active[j] >= MIN_ACTIVE, (j, (lo[j], hi[j]), active[j])
    return seen


@pytest.mark.parametrize("unbounded", [False, True])
@pytest.mark.parametrize("n,m", WIDE_HOST_SHAPES)
def test_wide_host_problems_expose_wrong_limits(oracle, n, m, unbounded):
    """test_wide_host_backward_with_a_box_per_control's problems: folded, mirrored and swapped limits all move the gains; the special
    boxes of tile 2 are active."""
    lo, hi = wide_boxes(m, seed=n, unbounded=unbounded)
    tile2 = [j for j in range(16, m) if (lo[j], hi[j]) in SPECIAL]
    assert 16 in tile2 and (m == 17 or m - 1 in tile2)
    p = host_problem(oracle, n, m, lo, hi)
    for lam in LAMBDAS:
        seen = check_problem(oracle, p["om"], p["us"], p["do"], p["k_prev"], lam, lo, hi, tile2)
        assert set(seen) == {"mirrored", "folded", "swapped"}


@pytest.mark.parametrize("n,m", NARROW_INF_SHAPES)
def test_infinite_limit_problems_expose_wrong_limits(oracle, n, m):
    """test_infinite_limits_on_every_wave_box_qp's problems: mirrored limits move the gains wherever they are not the true ones (a
    lone (-inf, inf) box is its own mirror); the one-sided boxes are active."""
    mirrored = 0
    for lo, hi in infinite_boxes(m):
        one_sided = [j for j in range(m) if (lo[j], hi[j]) in (UPPER_ONLY, LOWER_ONLY)]
        p = host_problem(oracle, n, m, lo, hi)
        for lam in LAMBDAS:
            mirrored += "mirrored" in check_problem(oracle, p["om"], p["us"], p["do"], p["k_prev"], lam, lo, hi, one_sided)
    assert mirrored >= 2 * (len(infinite_boxes(m)) - (m == 1))


@pytest.mark.parametrize("n,m,unbounded", WIDE_LQ_CASES)
def test_wide_lq_problems_expose_wrong_limits(oracle, n, m, unbounded):
    """The first backward pass of test_wide_lq_twin_with_a_box_per_control's and (n = 24, m = 20) test_wide_user_twin_with_a_box_per_control's
    walks (the oracle's rollout of u0, gains 0, lambda 1): folded, mirrored and swapped limits all move the gains; the special boxes of
    tile 2 are active."""
    mats, lo, hi, x0, u0 = wide_lq_case(n, m, unbounded)
    om = oracle.Model("lq", lq=mats, u_min=lo, u_max=hi)
    xs, us, cost = oracle.batch_rollout(om, x0, u0, DT)
    do = oracle.batch_derivatives(om, xs, us, DT)
    tile2 = [j for j in range(16, m) if (lo[j], hi[j]) in SPECIAL]
    seen = check_problem(oracle, om, us, do, np.zeros_like(us), 1.0, lo, hi, tile2)
    assert set(seen) == {"mirrored", "folded", "swapped"}


def test_wide_boxes_keep_the_tiles_apart():
    """Every placement wide_boxes promises, at every m the GPU tests use."""
    for m in sorted({m for _, m in WIDE_HOST_SHAPES} | {m for _, m, _ in WIDE_LQ_CASES}):
        for unbounded in (False, True):
            lo, hi = wide_boxes(m, seed=m, unbounded=unbounded)
            boxes = list(zip(lo, hi))
            assert len(set(boxes)) == m
            assert lo[16] == hi[16] != 0 and lo[m - 1] == hi[m - 1]
            for j in range(16, m):
                assert boxes[j] != boxes[j - 16] and boxes[j] != (-hi[j - 16], -lo[j - 16])
            if m >= 20:
                assert 0.0 in (lo[m - 1], hi[m - 1])
            if m >= 24:
                tile2 = boxes[16:]
                assert ABOVE_0 in tile2 and BELOW_0 in tile2
            if unbounded:
                assert UPPER_ONLY in boxes[:16]
                if m >= 20:
                    assert (-np.inf, np.inf) in boxes[16:] and LOWER_ONLY in boxes[16:]
