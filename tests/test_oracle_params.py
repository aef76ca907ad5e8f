"""oracle.set_params reaches every arithmetic flavour of the oracle -- the f64 reference twin, the f32 twin of the product's fp32 mode
and the f80 yardstick -- those loaded before the call and those loaded after it, as set_fixes does.  A flavour left on the default
tunables would walk an fp32 handle, or judge a conditioning verdict, under another schedule than the one the test set."""
import numpy as np
import pytest

DT = 0.02
# a strict search and a low ceiling: z_min = 0.9 rejects most steps, lambda_factor = 3 climbs to lambda_max = 50 within a few
# iterations (status 3); the defaults run the same acrobot problem to max_iters
STRICT = dict(tol_fun=1e-4, tol_grad=1e-9, lambda_factor=3.0, lambda_max=50.0, lambda_min=1e-3, z_min=0.9)


def _solve(oracle, name, om64, x0, u0, max_iters):
    with oracle.flavour(name):
        om = om64.twin(name) if name != "f64" else om64
        s = oracle.Solver(om, u0.shape[0], DT)
        st, log = s.generate_trajectory(x0, u0, max_iters=max_iters, log=True)
        return dict(status=st, iters=s.iters, lam=float(s.lam), dlam=float(s.dlam), cost=np.asarray(log, dtype=np.float64))


def test_set_params_reaches_every_flavour(oracle):
    assert oracle.get_params() == oracle.DEFAULT_PARAMS
    T, max_iters = 60, 12
    om = oracle.Model("acrobot", u_lim=1.5)
    x0 = np.array([0.81, -0.63, 0.18, -0.09])
    u0 = np.zeros((T, 1))
    default = _solve(oracle, "f64", om, x0, u0, max_iters)
    with oracle.flavour("f32"):
        oracle.lib()  # loaded BEFORE set_params
    oracle.forget("f80")  # (and f80 bound after it: lib() applies the remembered tunables when it binds a flavour)
    try:
        oracle.set_params(**STRICT)
        assert oracle.get_params() == STRICT
        got = {name: _solve(oracle, name, om, x0, u0, max_iters) for name in ("f64", "f32", "f80")}
    finally:
        oracle.set_params()
    print("default", default, "\nstrict", got)
    assert default["status"] == 0 and default["iters"] == max_iters  # (the default schedule never reaches lambda_max = 1e11)
    ref = got["f64"]
    assert ref["status"] == 3 and ref["lam"] > STRICT["lambda_max"] and ref["iters"] < max_iters, ref
    for name in ("f32", "f80"):
        r = got[name]
        assert (r["status"], r["iters"]) == (ref["status"], ref["iters"]), (name, r, ref)
        # the schedule is pure products of lambda_factor: f32 keeps it in double (bit for bit), f80 in extended precision
        assert r["lam"] == pytest.approx(ref["lam"], rel=1e-15) and r["dlam"] == pytest.approx(ref["dlam"], rel=1e-15), (name, r, ref)
        assert np.allclose(r["cost"], ref["cost"], rtol=1e-4), (name, r["cost"], ref["cost"])
    # the defaults are back in every flavour
    assert oracle.get_params() == oracle.DEFAULT_PARAMS
    for name in ("f64", "f32", "f80"):
        assert _solve(oracle, name, om, x0, u0, max_iters)["status"] == 0
