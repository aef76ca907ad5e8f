"""The parity harness and per-control limits (no GPU): an oracle model's twin in another arithmetic flavour keeps the
limits it was given, whatever the kind and however they were set; and a pinned control (u_min == u_max) never lets
the walk excuse a gain mismatch as a box-QP clamp tie."""
import numpy as np
import pytest

from tests.parity import first_gain_mismatch_is_knife_edge


def _models(oracle):
    from tests.test_gpu_lq_end_to_end import dense_mats
    chain = (8, np.array([9.81, 0.1, 2.0, 10.0, 1.0, 0.1, 50.0, 0.0]))
    return {
        "acrobot": (dict(), [-0.3], [0.9]),
        "integrator": (dict(goal=[1.0, 0.5, 0.0, 0.0]), [-0.3, -0.9], [0.6, 0.1]),
        "lq": (dict(lq=dense_mats(5, 3, seed=2), u_lim=1.0), [-0.3, 0.15, 0.2], [0.9, 0.7, 0.2]),
        "chain": (dict(chain=chain, u_lim=2.0), [-0.3, 0.0, -1.1, 0.05], [0.9, 0.0, 0.3, 0.4]),
    }


@pytest.mark.parametrize("how", ["set_limits", "constructor"])
@pytest.mark.parametrize("kind", ["acrobot", "integrator", "lq", "chain"])
def test_twin_keeps_per_control_limits(oracle, kind, how):
    """f64 -> f32 / f80 / f64 twins, and back from a float model: every control keeps its own asymmetric box (rounded to the
    twin's precision), whether the limits came with the constructor or from set_limits afterwards."""
    kw, lo, hi = _models(oracle)[kind]
    lo, hi = np.array(lo), np.array(hi)
    if how == "set_limits":
        om = oracle.Model(kind, **kw)
        om.set_limits(lo, hi)
    else:
        om = oracle.Model(kind, **dict(kw, u_lim=None), u_min=lo, u_max=hi)
    assert np.array_equal(om.u_min, lo) and np.array_equal(om.u_max, hi)
    rounded = dict(f32=lambda v: v.astype(np.float32).astype(np.float64), f64=lambda v: v, f80=lambda v: v)
    for name in ("f32", "f80", "f64"):
        tw = om.twin(name)
        assert tw.flavour == name and tw.nu == len(lo)
        assert np.array_equal(tw.u_min, rounded[name](lo)), (name, tw.u_min, lo)
        assert np.array_equal(tw.u_max, rounded[name](hi)), (name, tw.u_max, hi)
        back = tw.twin("f64")  # (a twin of a twin: what the walks build from an f32 model)
        assert np.array_equal(back.u_min, rounded[name](lo)) and np.array_equal(back.u_max, rounded[name](hi))


def test_twin_box_reaches_the_solver(oracle):
    """The twin's limits are the ones its backward pass clamps to: an acrobot boxed to [0.15, 1.2] started at u = 0
    (outside the box) gets k in [0.15 - u, 1.2 - u] in every flavour, and the first step lands inside the box."""
    om = oracle.Model("acrobot")
    om.set_limits(0.15, 1.2)
    B, T, dt = 3, 30, 0.02
    x0 = np.array([[0.3, -0.2, 0.1, 0.0], [-1.0, 0.5, 0.0, 0.2], [2.0, 0.1, -0.3, 0.1]])
    u0 = np.zeros((B, T, 1))
    for name in ("f64", "f32", "f80"):
        with oracle.flavour(name):
            tw = om.twin(name)
            xs, us, _ = oracle.batch_rollout(tw, x0, u0, dt)
            d = oracle.batch_derivatives(tw, xs, us, dt)
            r = oracle.batch_backward(tw, us, d)
        k = np.asarray(r["k"], dtype=np.float64)
        assert np.all(r["diverge"] == 0)
        assert np.all(k >= 0.15 - 1e-6) and np.all(k <= 1.2 + 1e-6), (name, k.min(), k.max())


def _pinned_case(T=12, n=4):
    """One trajectory with m = 2: control 0 pinned at u = 0.3 (its k sits exactly on its zero-width box), control 1 free in
    [-1, 1] with k well inside."""
    rng = np.random.default_rng(5)
    us = np.stack([np.full(T, 0.3), rng.uniform(-0.3, 0.3, T)], axis=1)
    lo = np.array([0.3, -1.0])[None, :] - us
    hi = np.array([0.3, 1.0])[None, :] - us
    ko = np.stack([lo[:, 0], rng.uniform(-0.2, 0.2, T)], axis=1)
    Ko = np.zeros((T, 2, n))
    Ko[:, 1, :] = rng.normal(size=(T, n))
    return us, lo, hi, ko, Ko


def test_pinned_control_does_not_excuse_a_gain_mismatch():
    us, lo, hi, ko, Ko = _pinned_case()
    k, K = ko.copy(), Ko.copy()
    k[7, 1] += 5e-5  # a gain mismatch of the size the band admits, on the FREE control, far from both of its bounds
    assert not first_gain_mismatch_is_knife_edge(k, K, ko, Ko, us, lo, hi)
    K2 = Ko.copy()
    K2[4, 1, 2] *= 1 + 1e-4  # a feedback-gain mismatch only
    assert not first_gain_mismatch_is_knife_edge(ko, K2, ko, Ko, us, lo, hi)


def test_genuine_clamp_tie_next_to_a_pinned_control_is_still_a_tie():
    """The stricter band still recognises a real knife edge: control 1 inside the 1e-4 band of its upper bound on one side."""
    us, lo, hi, ko, Ko = _pinned_case()
    ko[7, 1] = hi[7, 1] - 5e-5
    k = ko.copy()
    k[7, 1] = hi[7, 1]
    K = Ko.copy()
    K[7, 1, :] = 0.0  # clamped on this side: its feedback row is zero
    assert first_gain_mismatch_is_knife_edge(k, K, ko, Ko, us, lo, hi)
