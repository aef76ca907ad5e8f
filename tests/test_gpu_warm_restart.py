"""What a restart of the outer loop keeps and what it starts over, asserted directly on the handle's state.

- ilqr_warm_start (generate_trajectory(x0)) keeps every trajectory's lambda / dlambda bit for bit and restarts status, iteration count,
  alpha index, dV and gnorm -- on the tiled and the generic layout, fp64 and fp32;
- ilqr_reset_state(h, 1) does the same on a host-evaluated handle that has an accepted iteration behind it;
- ilqr_reset_state(h, 0) leaves the handle's own lambda_init / dlambda_init and zero gains.

B = 5, T = 8: a partial tile, padding up to 64 slots, one checkpoint chunk boundary."""
import numpy as np
import pytest

from tests.util import acrobot_x0, integrator_x0, mat

pytestmark = pytest.mark.gpu
DT = 0.02
B, T = 5, 8
LAM = 0.5 + np.arange(B)      # per trajectory, none the default 1
DLAM = 1.6 ** np.arange(B) * 1.25


def lq_mats(n, m):
    from tests.test_gpu_lq_end_to_end import dense_mats
    return dense_mats(n, m)


def problem(name):
    """(constructor kwargs, x0 [B][nx], nu)"""
    if name.startswith("acrobot"):
        return dict(model="acrobot", u_min=-1.5, u_max=1.5, dtype=name[-3:]), acrobot_x0(B, scale=0.3, seed=4), 1
    if name == "integrator":
        return dict(model="integrator", goal=[1, .5, 0, 0]), integrator_x0(B), 2
    return dict(model="lq", lq=lq_mats(6, 3), u_min=-0.4, u_max=0.4), np.random.default_rng(5).uniform(-1, 1, (B, 6)), 3


def make(kw, **extra):
    from ilqr_amd import BatchILQR
    kw = dict(kw, **extra)
    return BatchILQR(kw.pop("model"), B, T, DT, **kw)


def assert_restarted(g):
    st, it, al = g.status()
    assert np.array_equal(st, np.zeros(B, dtype=np.int32)) and np.array_equal(it, np.zeros(B, dtype=np.int32))
    assert np.array_equal(al, np.full(B, -1, dtype=np.int32))
    assert np.array_equal(g.dV(), np.zeros((B, 2))) and np.array_equal(g.gnorm(), np.zeros(B))


@pytest.mark.parametrize("name", ["acrobot_f64", "acrobot_f32", "integrator", "lq"])
def test_warm_start_keeps_lambda(name):
    kw, x0, nu = problem(name)
    src = make(kw)
    src.init_traj(x0, 0.1 * np.random.default_rng(9).standard_normal((B, T, nu)))
    src.iterate(2)
    xs, us = src.trajectory()
    k, K = src.gains()
    g = make(kw, params=dict(max_iter=0))
    g.set_trajectory(x0=x0, xs=xs, us=us, cost=src.cost())
    g.set_gains(k=k, K=K)
    g.iterate(1)  # a run state that is not a fresh handle's: one iteration counted, max_iter reached
    st, it, _ = g.status()
    assert np.all(st != 0) and np.all(it == 1) and np.any(g.dV() != 0)
    xs, us = g.trajectory()
    g.set_lambda(LAM, DLAM)
    g.generate_trajectory(x0 + 1e-3)
    lam, dlam = g.lambdas()
    assert np.array_equal(lam, LAM) and np.array_equal(dlam, DLAM)
    assert_restarted(g)
    assert np.all(np.isfinite(g.cost())) and not np.array_equal(g.trajectory()[0], xs)  # the warm rollout ran
    src.close()
    g.close()


def test_warm_reset_on_a_host_evaluated_handle(oracle):
    from ilqr_amd import BatchILQR
    n, m = 3, 2
    om = oracle.Model("lq", lq=lq_mats(n, m), u_lim=1.0)
    g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=-1.0, u_max=1.0, params=dict(max_iter=1))
    rng = np.random.default_rng(3)
    x0 = rng.uniform(-1, 1, (B, n))
    xs, us, cost = oracle.batch_rollout(om, x0, rng.normal(size=(B, T, m)) * 0.2, DT)
    do = oracle.batch_derivatives(om, xs, us, DT)
    g.set_trajectory(x0=x0, xs=xs, us=us, cost=cost)
    g.reset_state(False)
    g.set_derivatives(**{key: (v if key in ("cx", "cu") else mat(v)) for key, v in do.items()})
    g.backward_step()
    g.accept_candidates(np.repeat(cost[:, None] + 1.0, 11, axis=1))  # a failed search: one iteration counted, max_iter reached
    st, it, _ = g.status()
    assert np.all(st != 0) and np.all(it == 1) and np.any(g.dV() != 0)
    g.set_lambda(LAM, DLAM)
    g.reset_state(warm=True)
    lam, dlam = g.lambdas()
    assert np.array_equal(lam, LAM) and np.array_equal(dlam, DLAM)
    assert_restarted(g)
    g.close()


@pytest.mark.parametrize("name", ["acrobot_f64", "lq"])
def test_cold_reset_starts_from_the_handles_own_lambda(name):
    kw, x0, nu = problem(name)
    g = make(kw, params=dict(lambda_init=3.0, dlambda_init=2.0))
    g.init_traj(x0, np.zeros((B, T, nu)))
    g.iterate(2)
    assert np.any(g.gains()[1] != 0)
    g.set_lambda(LAM, DLAM)
    g.reset_state(warm=False)
    lam, dlam = g.lambdas()
    assert np.array_equal(lam, np.full(B, 3.0)) and np.array_equal(dlam, np.full(B, 2.0))
    k, K = g.gains()
    assert np.array_equal(k, np.zeros_like(k)) and np.array_equal(K, np.zeros_like(K))
    assert_restarted(g)
    g.close()
