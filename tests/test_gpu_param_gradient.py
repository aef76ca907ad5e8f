"""The gradient of a caller's loss with respect to the per-trajectory model parameters (ilqr_get_param_gradient /
ilqr_param_gradient_on_device; k_pg_costate, k_pg_contract, k_pg_reduce) on the pendulum chain (examples/user_model_pendulum_chain.hpp,
NTP = 8).  The yardstick is the definition of include/ilqr_amd.h evaluated in numpy with one oracle.Model("chain", ...) per perturbed row
(pg_reference); tests/test_param_gradient_abi.py checks the yardstick itself on the CPU.  Then the whole chain compute_derivatives ->
lq_solve -> param_gradient against central differences over whole re-solves where the records' LQ model is exact (linear dynamics), the
bit-for-bit promises, the fp32 handle and every refusal that needs a handle."""
import os

import numpy as np
import pytest

from tests.test_gpu_user_chain import DT, NL, PARAMS, chain_x0

pytestmark = pytest.mark.gpu
NX, NU, NTP = 2 * NL, NL // 2, 8
EPS = 1e-3  # the records' own step
U = 2.0 ** -53


@pytest.fixture(scope="module")
def chain_lib():
    from ilqr_amd import _build
    if not os.path.exists(_build.USER_CHAIN_LIB) and not os.path.exists(_build.HIPCC):
        pytest.skip("the pendulum-chain build is missing and there is no hipcc to make it")
    return _build.build_user(_build.USER_CHAIN_HEADER, _build.USER_CHAIN_LIB)


@pytest.fixture(scope="module", autouse=True)
def torch_device_first():
    """test_bits hands torch tensors over: torch's device is initialised before this module creates any handle"""
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()


def draw_params(B, seed):
    """as tests/test_gpu_traj_params.py: the first seven within +-20 % of PARAMS, the target angle uniform in [-1, 1]"""
    rng = np.random.default_rng(seed)
    p = PARAMS[None, :] * (1.0 + rng.uniform(-0.2, 0.2, (B, 8)))
    p[:, 7] = rng.uniform(-1.0, 1.0, B)
    return p


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def handle(chain_lib, B, T, lim, **kw):
    from ilqr_amd import BatchILQR
    return BatchILQR("user", B, T, DT, u_min=-lim, u_max=lim, lib=chain_lib, nx=NX, nu=NU, user_params=PARAMS, **kw)


def costate(d):
    """lam[T] = cx[T], lam[t] = cx[t] + fx[t]' lam[t+1] on records as BatchILQR.derivatives() returns them (fx [B][T+1][row][col])"""
    lam = np.zeros_like(d["cx"])
    T = lam.shape[1] - 1
    lam[:, T] = d["cx"][:, T]
    for t in range(T - 1, -1, -1):
        lam[:, t] = d["cx"][:, t] + np.einsum("brc,br->bc", d["fx"][:, t], lam[:, t + 1])
    return lam


def pg_reference(oracle, params, lim, dt, xs, us, lam, dxs, dus, dlam, eps_p=1e-3):
    """The definition of include/ilqr_amd.h (ilqr_get_param_gradient), term by term: one oracle twin per perturbed row, Model.cost /
    final_cost / integrate.  dxs, dlam [B][T+1][S][nx], dus [B][T][S][nu].  Returns (gp [B][S][NTP], bound [B][S][NTP]): the bound is the
    forward rounding bound 32 u sum_t [4 max|Psi| n_t / (4 eps h) + 2 |dlam[t+1]|_1 max|F| / (2 h)] from the reference's own intermediates."""
    B, T = us.shape[:2]
    S = dxs.shape[2]
    gp, bound = np.zeros((B, S, NTP)), np.zeros((B, S, NTP))
    for b in range(B):
        for j in range(NTP):
            h = eps_p * max(1.0, abs(params[b, j]))
            rows = [params[b].copy(), params[b].copy()]
            rows[0][j] = params[b, j] + h
            rows[1][j] = params[b, j] - h
            Mp, Mm = (oracle.Model("chain", chain=(NL, r), u_lim=lim) for r in rows)
            for s in range(S):
                total = scale = 0.0
                for t in range(T + 1):
                    last = t == T
                    x, u = xs[b, t], (None if last else us[b, t])
                    dx, du = dxs[b, t, s], (np.zeros(NU) if last else dus[b, t, s])
                    n = float(np.sqrt(np.dot(dx, dx) + np.dot(du, du)))
                    if n > 0.0:
                        def psi(M, sigma):
                            step = sigma * (EPS / n)
                            if last:
                                return float(M.final_cost(x + step * dx))
                            return float(M.cost(x + step * dx, u + step * du)) + float(np.dot(lam[b, t + 1], M.integrate(x + step * dx, u + step * du, dt)))
                        v = [psi(Mp, 1.0), psi(Mp, -1.0), psi(Mm, 1.0), psi(Mm, -1.0)]
                        total += (v[0] - v[1] - v[2] + v[3]) * n / (4 * EPS * h)
                        scale += 4 * max(abs(a) for a in v) * n / (4 * EPS * h)
                    if not last:
                        Fp, Fm = Mp.integrate(x, u, dt), Mm.integrate(x, u, dt)
                        total += float(np.dot(dlam[b, t + 1, s], Fp - Fm)) / (2 * h)
                        scale += 2 * float(np.abs(dlam[b, t + 1, s]).sum()) * max(float(np.abs(Fp).max()), float(np.abs(Fm).max())) / (2 * h)
                gp[b, s, j] = total
                bound[b, s, j] = 32 * U * scale
    return gp, bound


def stencil_case(B, T, S, seed):
    """Random dxs, dus, dlam with: direction 1 all zero in dxs, dus at two knots (the n = 0 branch), direction 2 with dxs = dus = 0
    everywhere (only B_t), one trajectory with dxs[T] = 0."""
    rng = np.random.default_rng(seed)
    dxs, dus, dlam = rng.normal(size=(B, T + 1, S, NX)), rng.normal(size=(B, T, S, NU)), rng.normal(size=(B, T + 1, S, NX))
    dxs[:, 2, 1], dus[:, 2, 1], dxs[:, 5, 1], dus[:, 5, 1] = 0.0, 0.0, 0.0, 0.0
    dxs[:, :, 2], dus[:, :, 2] = 0.0, 0.0
    dxs[1, T] = 0.0
    return dxs, dus, dlam


def nominal(g, B, T, seed, rows):
    g.set_trajectory_params(rows)
    rng = np.random.default_rng(seed)
    g.init_traj(f32(chain_x0(B, seed=seed)), f32(rng.normal(size=(B, T, NU)) * 0.5))
    g.compute_derivatives()
    return g.trajectory()


def check_against_reference(oracle, g, rows, lim, dxs, dus, dlam, what):
    """lam against the numpy recursion on the device's own records, gp against pg_reference with the device's lam, under its bound"""
    gp, lam = g.param_gradient(dxs, dus, dlam, want_lam=True)
    xs, us = g.trajectory()
    lam_ref = costate(g.derivatives())
    err = np.abs(lam - lam_ref).max() / np.abs(lam_ref).max()
    print("%s: lam relerr %.2e" % (what, err))
    assert err <= 1e-12
    ref, bound = pg_reference(oracle, rows, lim, DT, xs, us, lam, dxs, dus, dlam)
    ratio = np.abs(gp - ref) / bound
    print("%s: worst |gp - ref| / bound %.3f (max |gp| %.3g, max relative error %.2e)" % (
        what, ratio.max(), np.abs(ref).max(), (np.abs(gp - ref) / np.maximum(np.abs(ref), 1e-300)).max()))
    assert np.all(np.isfinite(gp)) and ratio.max() <= 1.0, ratio
    return gp, lam, ref, bound


def test_stencil_against_the_oracle_twin(oracle, chain_lib):
    """Worst observed / bound ratio on the MI355X: see DESIGN.md 3.21."""
    B, T, S, lim = 3, 7, 3, 2.0
    g = handle(chain_lib, B, T, lim)
    rows = draw_params(B, 41)
    xs, us = nominal(g, B, T, 3, rows)
    dxs, dus, dlam = stencil_case(B, T, S, 11)
    gp, lam, ref, bound = check_against_reference(oracle, g, rows, lim, dxs, dus, dlam, "fp64 stencil")
    # ... and NOT what the handle-wide PARAMS would give: the rows reached the kernel
    shared, _ = pg_reference(oracle, np.repeat(PARAMS[None], B, axis=0), lim, DT, xs, us, lam, dxs, dus, dlam)
    for b in range(B):
        gap = np.abs(gp[b] - shared[b]).max()
        assert gap > 1e-3 * np.abs(gp[b]).max() and gap > 10 * bound[b].max(), (b, gap)
    # one input alone, the others NULL: the same terms as zeros in their place
    zx, zu, zl = np.zeros_like(dxs), np.zeros_like(dus), np.zeros_like(dlam)
    assert np.array_equal(g.param_gradient(dxs, dus, None), g.param_gradient(dxs, dus, zl))
    assert np.array_equal(g.param_gradient(None, None, dlam), g.param_gradient(zx, zu, dlam))
    g.close()


def test_end_to_end_with_linear_dynamics(chain_lib):
    """g/l = 0 makes the chain linear in (x, u), so the records' LQ model is the problem's own: compute_derivatives -> lq_solve(gx = w, gu
    = v) -> param_gradient on trajectory 0 against central differences of L = sum w.xs + sum v.us over 32 whole re-solves under p0 +- delta_j
    e_j and p0 +- (delta_j / 2) e_j, within 10 x the two steps' disagreement plus 1e-4 relative.  One handle, B = 33."""
    T, dt, lim = 20, 0.02, 50.0
    p0 = np.array([0.0, 0.1, 2.0, 10.0, 1.0, 0.1, 50.0, 0.3])
    delta = 1e-3 * np.maximum(1.0, np.abs(p0))
    rows = [p0]
    for j in range(NTP):
        for step in (delta[j], -delta[j], delta[j] / 2, -delta[j] / 2):
            r = p0.copy()
            r[j] += step
            rows.append(r)
    rows = np.array(rows)
    B = len(rows)
    assert B == 33
    rng = np.random.default_rng(0)
    x0 = np.concatenate([rng.uniform(-1, 1, (1, NL)), rng.uniform(-1, 1, (1, NL)) * 0.5], axis=1)  # (as chain_x0 draws it)
    u0 = 0.3 * rng.normal(size=(T, NU))
    w, v = rng.normal(size=(T + 1, NX)), rng.normal(size=(T, NU))
    from ilqr_amd import BatchILQR
    g = BatchILQR("user", B, T, dt, u_min=-lim, u_max=lim, lib=chain_lib, nx=NX, nu=NU, user_params=p0,
                  params=dict(tol_fun=1e-14, tol_grad=1e-12, max_iter=400))
    g.set_trajectory_params(rows)
    g.init_traj(np.repeat(x0, B, axis=0), np.repeat(u0[None], B, axis=0))
    g.generate_trajectory()
    xs, us = g.trajectory()
    print("end to end: iterations %s, status %s, max |u| %.3g" % (g.status()[1][:3], g.status()[0][:3], np.abs(us).max()))
    assert np.abs(us).max() < lim  # no control clamps
    g.compute_derivatives()
    gx, gu = np.repeat(w[None], B, axis=0), np.repeat(v[None], B, axis=0)
    dxs, dus, dlam, info = g.lq_solve(gx=gx, gu=gu, dlam=True)
    assert not info.any()
    gp, lam = g.param_gradient(dxs, dus, dlam, want_lam=True)
    d = g.derivatives()
    station = np.abs(d["cu"][0, :T] + np.einsum("trc,tr->tc", d["fu"][0, :T], lam[0, 1:])).max()
    print("end to end: max_t |cu + fu' lam| = %.3g" % station)
    assert station <= 1e-6  # the solve reached the stationary point the formula assumes
    L = np.einsum("ti,bti->b", w, xs) + np.einsum("ti,bti->b", v, us)
    fd1 = np.array([(L[1 + 4 * j] - L[2 + 4 * j]) / (2 * delta[j]) for j in range(NTP)])
    fd2 = np.array([(L[3 + 4 * j] - L[4 + 4 * j]) / delta[j] for j in range(NTP)])
    lhs = np.abs(gp[0] - fd2)
    rhs = 10 * np.abs(fd1 - fd2) + 1e-4 * np.maximum(1.0, np.abs(fd2))
    for j in range(NTP):
        print("  p[%d]: gp %+.8e  fd(delta/2) %+.8e  fd(delta) %+.8e  |gp - fd| %.2e  allowed %.2e" % (j, gp[0, j], fd2[j], fd1[j], lhs[j], rhs[j]))
    assert np.all(lhs <= rhs), (lhs, rhs)
    assert np.abs(fd2).max() > 1e-2  # (a gradient worth the name)
    g.close()


def test_bits(chain_lib):
    import torch
    B, T, S, lim = 3, 7, 3, 2.0
    g, twin = handle(chain_lib, B, T, lim), handle(chain_lib, B, T, lim)
    rows = draw_params(B, 43)
    for h in (g, twin):
        nominal(h, B, T, 5, rows)
    dxs, dus, dlam = stencil_case(B, T, S, 13)
    gp, lam = g.param_gradient(dxs, dus, dlam, want_lam=True)
    gp2, lam2 = g.param_gradient(dxs, dus, dlam, want_lam=True)
    assert np.array_equal(gp, gp2) and np.array_equal(lam, lam2) and np.all(np.isfinite(gp))
    assert np.array_equal(g.param_gradient(dxs, dus, dlam), gp)  # (lam in scratch: the same gp)
    for s in range(S):  # a column depends on its own column only
        one = g.param_gradient(dxs[:, :, s], dus[:, :, s], dlam[:, :, s])
        assert np.array_equal(one, gp[:, s]), s
    # device memory in, device memory out
    dev = torch.device("cuda", 0)
    t_in = [torch.tensor(a, dtype=torch.float64, device=dev) for a in (dxs, dus, dlam)]
    t_gp, t_lam = torch.zeros((B, S, NTP), dtype=torch.float64, device=dev), torch.zeros((B, T + 1, NX), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    g.param_gradient_on_device(S, t_in[0], t_in[1], t_in[2].data_ptr(), gp=t_gp, lam=t_lam)
    g.synchronize()
    assert np.array_equal(t_gp.cpu().numpy(), gp) and np.array_equal(t_lam.cpu().numpy(), lam)
    # read-only: two further iterations are those of a twin that never asked
    for h in (g, twin):
        h.iterate(1)
        h.iterate(1)
    for a, b in zip(g.trajectory() + g.gains() + (g.cost(),) + g.lambdas(), twin.trajectory() + twin.gains() + (twin.cost(),) + twin.lambdas()):
        assert np.array_equal(a, b)
    g.close()
    twin.close()


def test_fp32_handle(oracle, chain_lib):
    """All arithmetic double on the float-rounded rows and the widened stored trajectory: the same reference under the same bound."""
    B, T, S, lim = 3, 7, 3, 2.0
    g = handle(chain_lib, B, T, lim, dtype="f32")
    rows = draw_params(B, 47)
    rows[:, 0] += 1.0 / 3.0 * 1e-3  # (no row is representable in float)
    assert np.all(f32(rows) != rows)
    xs, us = nominal(g, B, T, 9, rows)
    assert np.array_equal(xs, f32(xs)) and np.array_equal(us, f32(us))
    dxs, dus, dlam = stencil_case(B, T, S, 17)
    check_against_reference(oracle, g, f32(rows), f32(lim), dxs, dus, dlam, "fp32 handle")
    g.close()


def test_refusals_on_the_device(chain_lib):
    from ilqr_amd import BatchILQR, capi
    B, T, S, lim = 3, 7, 2, 2.0
    g = handle(chain_lib, B, T, lim)
    rows = draw_params(B, 53)
    dxs, dus, dlam = stencil_case(B, T, 3, 19)
    dxs, dus, dlam = (np.ascontiguousarray(a[:, :, :S]) for a in (dxs, dus, dlam))
    gp_buf, lam_buf = np.zeros((B, S, NTP)), np.zeros((B, T + 1, NX))
    p = lambda a: a.ctypes.data_as(capi._dp) if a is not None else None
    call = lambda n_dirs=S, flags=0, eps_p=0.0, i=(dxs, dus, dlam), o=(gp_buf, lam_buf): g.lib.ilqr_get_param_gradient(
        g.h, n_dirs, flags, eps_p, p(i[0]), p(i[1]), p(i[2]), p(o[0]), p(o[1]))
    err = g.lib.ilqr_last_error
    # before ilqr_init_traj, and before any rows are set
    assert call() == -4 and b"before ilqr_init_traj" in err()
    g.init_traj(chain_x0(B), np.zeros((B, T, NU)))
    g.compute_derivatives()
    assert call() == -4 and b"no per-trajectory parameters are set" in err()
    g.set_trajectory_params(rows)
    g.compute_derivatives()
    assert call() == 0
    gp0, lam0 = gp_buf.copy(), lam_buf.copy()
    assert np.all(np.isfinite(gp0)) and np.abs(gp0).max() > 0

    def still_the_same():
        gp_buf[:], lam_buf[:] = 0.0, 0.0
        assert call() == 0 and np.array_equal(gp_buf, gp0) and np.array_equal(lam_buf, lam0)

    for kw, msg in ((dict(n_dirs=0), b"n_dirs 0 must be >= 1"), (dict(flags=1), b"unknown flag bits 0x1"), (dict(eps_p=-1.0), b"eps_p -1 must be finite"),
                    (dict(eps_p=float("nan")), b"must be finite and >= 0"), (dict(eps_p=float("inf")), b"must be finite and >= 0"),
                    (dict(i=(None, None, None)), b"dxs, dus and dlam are all null"), (dict(o=(None, None)), b"gp and lam are both null")):
        assert call(**kw) == -1 and msg in err(), (kw, err())
        still_the_same()
    assert g.lib.ilqr_param_gradient_on_device(g.h, 0, 0, 0.0, None, None, None, None, None) == -1 and b"ilqr_param_gradient_on_device: n_dirs" in err()
    g.clear_trajectory_params()
    assert call() == -4 and b"no per-trajectory parameters are set" in err()
    g.set_trajectory_params(rows)
    still_the_same()
    g.close()
    # the default library: no user model
    g = BatchILQR("acrobot", 4, 10, DT)
    g.init_traj(np.zeros((4, 4)), np.zeros((4, 10, 1)))
    z = np.zeros((4, 11, 1, 4))
    with pytest.raises(capi.ILQRError, match=r"error -5: .*ILQR_MODEL_USER"):
        g.param_gradient(dxs=z)
    g.close()


# ---- every request through the staging buffer ---------------------------------------------------
from tests import getter_vs_device as gd  # noqa: E402


@pytest.mark.parametrize("case", gd.CASES)
def test_getter_equals_the_device_form_request_by_request(chain_lib, case):
    """ilqr_get_param_gradient against ilqr_param_gradient_on_device, bit for bit, on the build whose twin has NTP: every pointer; dlam in
    and lam out alone (a call without inputs is refused); that, every pointer, that again on one handle."""

    def make():
        g = handle(chain_lib, gd.B, gd.T, 2.0)
        nominal(g, gd.B, gd.T, 3, draw_params(gd.B, 41))
        return g

    def args(g):
        rng, per_x, per_u = np.random.default_rng(3), gd.B * gd.ND * NX, gd.B * gd.ND * NU
        return [gd.Arg("dxs", "in", rng.normal(size=per_x * (gd.T + 1))), gd.Arg("dus", "in", rng.normal(size=per_u * gd.T)),
                gd.Arg("dlam", "in", rng.normal(size=per_x * (gd.T + 1))), gd.Arg("gp", "out", (gd.B * gd.ND * NTP,)), gd.Arg("lam", "out", (gd.B * (gd.T + 1) * NX,))]
    gd.check(make, case, "ilqr_get_param_gradient", "ilqr_param_gradient_on_device", (gd.ND, 0, 0.0), args, needs_input=True)
