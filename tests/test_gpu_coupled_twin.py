"""Device twins whose running cost couples state and control, 0.5 x'Qx + 0.5 u'Ru + x'N u: the finite-difference kernels must PRODUCE
cxu = N (derivatives.hpp, generic.hpp), and the persistent routes -- the fused sweeps, k_solve_tile, k_solve_hex's ring record, the wide
tiles -- must carry it from their sweep to their backward pass, where no stage call can put it (tests/test_gpu_coupled_backward.py
covers the stage kernels).  Both shipped nx = 4 models have cxu = 0.

  tests/native/user_model_coupled4.hpp (nx = 4; nu = 1 and, _nu2, nu = 2): every nx = 4 route bit-identical to ILQR_FLAG_UNFUSED in fp64
      and fp32; the records' cxu against N; iterations of the default and the two-kernel route walked against the oracle's
      Model("lq", ..., cross=N)
  examples/user_model_linear6.hpp with its optional N (nx = 6, nu = 2): both of its routes likewise, and its analytic_record
Parameters: tests/coupled.py (the cost is convex: tests/test_coupled_inputs.py)."""
import numpy as np
import pytest

from tests import coupled

pytestmark = pytest.mark.gpu
DT = 0.02


@pytest.fixture(scope="module")
def coupled4_libs():
    from ilqr_amd import _build
    return {1: _build.build_user(_build.USER_COUPLED4_HEADER, _build.USER_COUPLED4_LIB),
            2: _build.build_user(_build.USER_COUPLED4_NU2_HEADER, _build.USER_COUPLED4_NU2_LIB)}


@pytest.fixture(scope="module")
def user6_lib():
    from ilqr_amd import _build
    return _build.build_user(_build.USER_EXAMPLE6_HEADER, _build.USER_EXAMPLE6_LIB)


def _problem(n, m, Bt, Tt):
    from tests.test_gpu_control_limits import distinct_boxes
    mats, N = coupled.coupled_mats(n, m, coupled.TWIN_SEED[n, m])
    lo, hi = distinct_boxes(m)
    x0, u0 = coupled.twin_start(n, m, Bt, Tt, coupled.TWIN_SEED[n, m])
    return mats, N, lo, hi, x0, u0


def _cxu_is_N(g, N, Tt):
    """the sweep's cxu[t < T] against N at the second differences' bound (tests/test_gpu_user_model.py) -- and N is not ~0"""
    g.compute_derivatives()
    cxu = g.derivatives()["cxu"]
    err = np.abs(cxu[:, :Tt] - N).max()
    print("coupled twin (%d,%d): |cxu - N| max %.2e, |cxu| max %.3f" % (N.shape + (err, np.abs(cxu).max())))
    assert err <= 1e-6 * max(1.0, np.abs(N).max()), err
    assert np.abs(cxu).max() > 0.05
    return cxu


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nu", [1, 2])
def test_coupled4_routes_equal_the_two_kernel_route(coupled4_libs, nu, dtype):
    """Every nx = 4 route (kernel names asserted; nu = 1 runs k_solve_hex by default, with the full ring record a user twin keeps): four
    calls of iterate(1), each pass's gains in the box of the trajectory it saw, then the solve to its end -- every array and scalar
    bit-identical to ILQR_FLAG_UNFUSED, the records (cxu among them) included."""
    from ilqr_amd import BatchILQR, capi
    from tests.test_gpu_control_limits import Invariants, _same, _state, nx4_routes, stepwise
    Bt, Tt = 83, 40
    mats, N, lo, hi, x0, u0 = _problem(4, nu, Bt, Tt)
    sv = capi.STAGE_NAMES.index("solve")
    out = []
    for name, fl, route, kernel in nx4_routes("acrobot" if nu == 1 else "integrator"):
        g = BatchILQR("user", Bt, Tt, DT, u_min=lo, u_max=hi, flags=fl, route=route, dtype=dtype, params=dict(max_iter=12), lib=coupled4_libs[nu],
                      nx=4, nu=nu, user_params=coupled.twin_params(mats, N))
        if kernel is not None:
            assert g.lib.ilqr_stage_kernel_name(g.h, sv) == kernel, (name, g.lib.ilqr_stage_kernel_name(g.h, sv))
        inv = Invariants(lo, hi, dtype)
        g.init_traj(x0, u0)
        stepwise(g, 4, inv)
        inv.done(min_checked=Bt)
        s = _state(g)
        g.generate_trajectory()
        s.update({"end_" + n: a for n, a in _state(g).items()})
        out.append((name, s))
        g.close()
    cxu = out[0][1]["d_cxu"]
    # what the routes carried is N (a float handle: differences taken in double from float knots and float parameters, stored as float)
    assert np.abs(cxu[:, :Tt] - N).max() <= 1e-6 * max(1.0, np.abs(N).max()) + (2 * 2.0 ** -24 * np.abs(N).max() if dtype == "f32" else 0.0)
    for name, s in out[1:]:
        _same(out[0][1], s, (name, nu, dtype))


@pytest.mark.parametrize("nu", [1, 2])
def test_coupled4_against_the_oracle(coupled4_libs, oracle, nu):
    """The sweep's cxu is N; five iterations of the default route and of the two-kernel route walked against the oracle's LQ model with
    the same cross term and limits, both drives (tests/parity.py); one walk of the fp32 mode against the float twin."""
    from ilqr_amd import BatchILQR, capi
    from tests.parity import walk_iterations
    Bt, Tt = 24, 40
    mats, N, lo, hi, x0, u0 = _problem(4, nu, Bt, Tt)
    om = oracle.Model("lq", lq=mats, cross=N, u_min=lo, u_max=hi)
    kw = dict(u_min=lo, u_max=hi, lib=coupled4_libs[nu], nx=4, nu=nu, user_params=coupled.twin_params(mats, N))
    for flags in (0, capi.FLAG_UNFUSED):
        g = BatchILQR("user", Bt, Tt, DT, flags=flags, **kw)
        g.init_traj(x0, u0)
        _cxu_is_N(g, N, Tt)
        for drive in ("oracle", "gpu"):
            r = walk_iterations(oracle, om, g, x0, u0, DT, 5, drive=drive)
            print("coupled twin (4,%d) flags %d drive %s:" % (nu, flags, drive), {kk: v for kk, v in r.items() if kk not in ("per_iter", "tied")})
            assert r["checked"] >= 3 * Bt and len(r["tied"]) <= Bt // 8, r
        g.close()
    g = BatchILQR("user", Bt, Tt, DT, dtype="f32", **kw)
    r = walk_iterations(oracle, om, g, x0, u0, DT, 5, drive="gpu", precision="f32")
    print("coupled twin (4,%d) f32:" % nu, {kk: v for kk, v in r.items() if kk not in ("per_iter", "tied")})
    ties = r["ties_backward"] + r["ties_search"] + r["ties_stop"]
    assert r["checked"] >= 3 * Bt, r["checked"]
    assert ties + r["conditioned_branch"] <= max(4, r["checked"] // 3), r  # (the bounds of test_nx4_limits_against_the_oracle in float)
    assert r["cond_over10"] <= max(2, r["checked"] // 20) and r["unresolved"] <= r["checked"] // 8, r
    g.close()


@pytest.mark.parametrize("route", ["thread", "wave"])
def test_linear6_with_a_cross_term(user6_lib, oracle, route):
    """examples/user_model_linear6.hpp with its optional N on both of its routes (k_derivatives / k_backward_t / k_rollout and
    k_derivatives_g / k_backward_w3 / k_rollout_g): the finite differences' cxu against N, every finite-difference block against the
    twin's own analytic_record (the bounds of test_generic_user_model_analytic_record; its cxu IS N, knot T stays 0), and four iterations
    walked against the oracle's coupled model."""
    from ilqr_amd import BatchILQR, capi
    from tests.parity import walk_iterations
    from tests.test_gpu_user_model import _kernels6, _route6
    n, m, Bt, Tt = 6, 2, 21, 40
    mats, N, lo, hi, x0, u0 = _problem(n, m, Bt, Tt)
    params = np.concatenate([coupled.twin_params(mats), [0.0], N.ravel()])  # (A, B, Q, R, Qf, wb = 0, N)
    recs = {}
    for name, fl in (("fd", 0), ("exact", capi.FLAG_ANALYTIC_DERIVATIVES)):
        g = BatchILQR("user", Bt, Tt, DT, u_min=lo, u_max=hi, lib=user6_lib, nx=n, nu=m, user_params=params, flags=fl, route=_route6(route))
        _kernels6(g, route)
        assert g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index("backward")) == (b"k_backward_t" if route == "thread" else b"k_backward_w3")
        g.init_traj(x0, u0)
        if name == "fd":
            _cxu_is_N(g, N, Tt)
        else:
            g.compute_derivatives()
        recs[name] = g.derivatives()
        if name == "fd":
            om = oracle.Model("lq", lq=mats, cross=N, u_min=lo, u_max=hi)
            r = walk_iterations(oracle, om, g, x0, u0, DT, 4, drive="gpu")
            print("coupled twin (6,2) %s:" % route, {kk: v for kk, v in r.items() if kk not in ("per_iter", "tied")})
            assert r["checked"] >= 2 * Bt and len(r["tied"]) <= Bt // 8, r
        g.close()
    fd, ex = recs["fd"], recs["exact"]
    assert np.array_equal(ex["cxu"][:, :Tt], np.broadcast_to(N, (Bt, Tt, n, m))) and np.all(ex["cxu"][:, Tt] == 0) and np.all(fd["cxu"][:, Tt] == 0)
    for key in ("fx", "fu", "cx", "cu"):
        assert np.abs(fd[key] - ex[key]).max() <= 1e-8 * max(1.0, np.abs(ex[key]).max()), key
    for key in ("cxx", "cuu"):
        assert np.abs(fd[key] - ex[key]).max() <= 1e-6 * max(1.0, np.abs(ex[key]).max()), key
    assert np.abs(fd["cxu"][:, :Tt] - ex["cxu"][:, :Tt]).max() <= 1e-6
