"""What the GPU tests of coupled costs (tests/test_gpu_coupled_backward.py, tests/test_gpu_coupled_twin.py) assume about their inputs,
proven on the CPU: for every (shape, seed, lambda) they use
  1. the fp64 oracle completes every trajectory and agrees with its own x87 yardstick to 1e-9 per knot -- three decades inside the
     project's 1e-6, so none of the tie / conditioning allowances of tests/parity.py is needed by the REFERENCE on these inputs;
  2. the free set is mixed: between 5 % and 90 % of the rows of K are clamped;
  3. with an unbounded box the oracle's gains are those of a Riccati recursion written here in numpy long doubles, independent of
     the oracle (Qux = cxu' + fu'Vxx fx, K = -(Quu + lambda I)^-1 Qux, the value update with the unregularised Quu): the first check
     that the oracle's own cxu path is right;
  4. the gains depend on cxu: with cxu = 0, or with the n x m block read with the strides of an m x n one (m >= 2), they move by at
     least 1 % per knot on EVERY trajectory -- a kernel that made either mistake could not pass.
And the oracle's LQ model with a cost term x'N u (Model("lq", ..., cross=N)): its finite-difference cxu is N."""
import numpy as np
import pytest

from tests import coupled
from tests.coupled import B, T, LAMBDAS, SEEDS
from tests.parity import gains_knot_err
from tests.util import mat


def _agreement(oracle, n, m, seed, lam, f32=False):
    rec, lo, hi, us, k_prev = coupled.case(n, m, seed, f32=f32)
    om = coupled.box_model(oracle, n, m, lo, hi)
    twin, yard = ("f32", "f64") if f32 else ("f64", "f80")
    r = coupled.oracle_backward(oracle, om, us, rec, k_prev, lam, twin)
    y = coupled.oracle_backward(oracle, om, us, rec, k_prev, lam, yard)
    return r, y, gains_knot_err(r["k"], r["Km"], y["k"], y["Km"], us)


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", coupled.ALL_SHAPES)
def test_reference_needs_no_allowance_and_the_free_set_is_mixed(oracle, n, m, seed, lam):
    r, y, e = _agreement(oracle, n, m, seed, lam)
    share = coupled.clamped_share(r["Km"])
    print("coupled inputs (%d,%d) seed %d lambda %g: f64 vs f80 per knot %.2e, clamped share %.2f" % (n, m, seed, lam, e.max(), share))
    assert np.all(r["diverge"] == 0) and np.all(y["diverge"] == 0)
    assert e.max() <= 1e-9, e
    assert 0.05 <= share <= 0.9, share


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", coupled.NX4_SHAPES)
def test_float_records_float_twin_against_fp64(oracle, n, m, seed, lam):
    """The fp32 cases: records rounded to float, the float twin (float records, limits and stored gains, the recursion in double) against
    the fp64 oracle on the same numbers.  What separates them is the rounding of the limits and of the stored gains to float, 2^-24 each:
    1e-6 per knot is a decade inside the fp32 tolerance of the GPU test (1e-5)."""
    r, y, e = _agreement(oracle, n, m, seed, lam, f32=True)
    print("coupled inputs (%d,%d) seed %d lambda %g: f32 twin vs f64 per knot %.2e" % (n, m, seed, lam, e.max()))
    assert np.all(r["diverge"] == 0) and np.all(y["diverge"] == 0)
    assert e.max() <= 1e-6, e
    assert 0.05 <= coupled.clamped_share(r["Km"]) <= 0.9


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", coupled.REGV_SHAPES)
def test_reference_needs_no_allowance_with_vxx_regularisation(oracle, n, m, seed, lam):
    """The same proof for the passes ILQR_FLAG_REGULARIZE_VXX is compared with (oracle.set_fixes(4): lambda on Vxx').  There lambda = 1e-3
    regularises by 1e-3 fu'fu ~ 1e-5, next to nothing, and ONE pass of the 16 -- (32,16), seed 2, lambda 1e-3, trajectory 6 -- has the
    fp64 oracle and its yardstick on the two sides of a box-QP clamp tie (a control within the 1e-4 band of its bound: tests/parity.py).
    The family is fixed, so it stays, stated: every other trajectory agrees to 1e-9, and a trajectory that does not is a PROVEN tie, at
    most one per pass -- the GPU test allows two (max_ties = 2), so a kernel on either side of this tie still has one to spare."""
    from tests.parity import first_gain_mismatch_is_knife_edge
    oracle.set_fixes(4)
    try:
        r, y, e = _agreement(oracle, n, m, seed, lam)
    finally:
        oracle.set_fixes(0)
    rec, lo, hi, us, k_prev = coupled.case(n, m, seed)
    off = np.flatnonzero(e > 1e-9)
    print("coupled inputs (%d,%d) seed %d lambda %g, lambda on Vxx: f64 vs f80 per knot %.2e without the %d tied" % (
        n, m, seed, lam, np.delete(e, off).max(), len(off)))
    assert np.all(r["diverge"] == 0) and np.all(y["diverge"] == 0)
    assert len(off) <= (1 if (n, m, seed, lam) == (32, 16, 2, 1e-3) else 0), e
    for b in off:
        assert first_gain_mismatch_is_knife_edge(r["k"][b], r["Km"][b], y["k"][b], y["Km"][b], us[b], lo[None] - us[b], hi[None] - us[b], 1e-9), b
    assert 0.05 <= coupled.clamped_share(r["Km"]) <= 0.9


def _solve_spd(M, R):
    """M^-1 R for batches of symmetric positive definite M [b][m][m], R [b][m][c], in the arrays' own precision (np.linalg has no
    long double): Cholesky, then the two triangular solves."""
    m = M.shape[-1]
    L = np.zeros_like(M)
    for j in range(m):
        d = M[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
        assert np.all(d > 0)
        L[:, j, j] = np.sqrt(d)
        for i in range(j + 1, m):
            L[:, i, j] = (M[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)) / L[:, j, j]
    Y = np.zeros_like(R)
    for i in range(m):
        Y[:, i] = (R[:, i] - np.einsum("bl,blc->bc", L[:, i, :i], Y[:, :i])) / L[:, i, i][:, None]
    X = np.zeros_like(R)
    for i in range(m - 1, -1, -1):
        X[:, i] = (Y[:, i] - np.einsum("bl,blc->bc", L[:, i + 1:, i], X[:, i + 1:])) / L[:, i, i][:, None]
    return X


def riccati_longdouble(rec, lam):
    """The unconstrained backward recursion of src/ilqr_core.cpp:350-401 on math-layout records, in np.longdouble."""
    ld = np.longdouble
    fx, fu, cx, cu, cxx, cxu, cuu = [np.asarray(rec[k], dtype=ld) for k in ("fx", "fu", "cx", "cu", "cxx", "cxu", "cuu")]
    nb, t1, n, m = fu.shape
    Tn = t1 - 1
    tr = lambda a: np.swapaxes(a, -1, -2)
    Vx, Vxx = cx[:, Tn], cxx[:, Tn]
    k, K = np.zeros((nb, Tn, m), ld), np.zeros((nb, Tn, m, n), ld)
    for i in range(Tn - 1, -1, -1):
        A, Bu = fx[:, i], fu[:, i]
        Qx = cx[:, i] + np.einsum("bji,bj->bi", A, Vx)
        Qu = cu[:, i] + np.einsum("bji,bj->bi", Bu, Vx)
        Qxx = cxx[:, i] + tr(A) @ Vxx @ A
        Qux = tr(cxu[:, i]) + tr(Bu) @ Vxx @ A
        Quu = cuu[:, i] + tr(Bu) @ Vxx @ Bu
        sol = _solve_spd(Quu + ld(lam) * np.eye(m, dtype=ld), np.concatenate([Qu[:, :, None], Qux], axis=2))
        ki, Ki = -sol[:, :, 0], -sol[:, :, 1:]
        Vx = Qx + np.einsum("bai,bac,bc->bi", Ki, Quu, ki) + np.einsum("bai,ba->bi", Ki, Qu) + np.einsum("bai,ba->bi", Qux, ki)
        Vxx = Qxx + tr(Ki) @ Quu @ Ki + tr(Ki) @ Qux + tr(Qux) @ Ki
        Vxx = ld(0.5) * (Vxx + tr(Vxx))
        k[:, i], K[:, i] = ki, Ki
    return k, K


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", coupled.ALL_SHAPES)
def test_unbounded_oracle_is_the_plain_riccati_recursion(oracle, n, m, seed, lam):
    rec, lo, hi, us, k_prev = coupled.case(n, m, seed)
    om = coupled.box_model(oracle, n, m, np.full(m, -np.inf), np.full(m, np.inf))
    r = coupled.oracle_backward(oracle, om, us, rec, k_prev, lam)
    k, K = riccati_longdouble(rec, lam)
    e = gains_knot_err(r["k"], r["Km"], k, K, us)
    print("coupled inputs (%d,%d) seed %d lambda %g: unbounded oracle vs numpy long-double Riccati per knot %.2e" % (n, m, seed, lam, e.max()))
    assert np.all(r["diverge"] == 0) and e.max() <= 1e-9, e


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,m", coupled.ALL_SHAPES)
def test_gains_depend_on_cxu_and_on_its_strides(oracle, n, m, seed, lam):
    rec, lo, hi, us, k_prev = coupled.case(n, m, seed)
    om = coupled.box_model(oracle, n, m, lo, hi)
    r = coupled.oracle_backward(oracle, om, us, rec, k_prev, lam)
    wrong = {"cxu = 0": np.zeros_like(rec["cxu"])}
    if m >= 2:
        wrong["strides of an m x n block"] = coupled.mis_strided(rec["cxu"])
    for what, cxu in wrong.items():
        w = coupled.oracle_backward(oracle, om, us, dict(rec, cxu=cxu), k_prev, lam)
        moved = gains_knot_err(w["k"], w["Km"], r["k"], r["Km"], us)
        print("coupled inputs (%d,%d) seed %d lambda %g: %s moves the gains by %.2f per knot at least" % (n, m, seed, lam, what, moved.min()))
        assert moved.min() >= 1e-2, (what, moved)


# ---------------------------------------------------------------------------------------------------------------------------------
# the coupled LQ twin's parameters, and the oracle model it is walked against
# ---------------------------------------------------------------------------------------------------------------------------------
TWINS = [(n, m, coupled.TWIN_SEED[n, m]) for n, m in ((4, 1), (4, 2), (6, 2))]


@pytest.mark.parametrize("n,m,seed", TWINS)
def test_twin_cost_is_convex(n, m, seed):
    mats, N = coupled.coupled_mats(n, m, seed)
    ev = np.linalg.eigvalsh(coupled.cost_hessian(mats, N))
    print("coupled twin (%d,%d): least eigenvalue of [[Q, N], [N', R]] %.3f, |N| max %.3f" % (n, m, ev.min(), np.abs(N).max()))
    assert ev.min() >= 0.05 and np.abs(N).max() > 0.05


@pytest.mark.parametrize("n,m,seed", TWINS)
def test_oracle_lq_model_with_a_cross_term(oracle, n, m, seed):
    """batch_derivatives of Model("lq", ..., cross=N): cxu[t < T] is N to the second differences' rounding (the bound of
    tests/test_gpu_user_model.py: 1e-6 max(1, |N|max)), knot T stays 0; without N the records are plain lq's to the bit; the float
    twin carries N too."""
    mats, N = coupled.coupled_mats(n, m, seed)
    x0, u0 = coupled.twin_start(n, m, 5, 12, seed)
    om, plain = oracle.Model("lq", lq=mats, cross=N, u_lim=0.5), oracle.Model("lq", lq=mats, u_lim=0.5)
    xs, us, cost = oracle.batch_rollout(om, x0, u0, 0.02)
    xp, _, cp = oracle.batch_rollout(plain, x0, u0, 0.02)
    run = np.einsum("bti,ij,btj->b", xs[:, :12], N, us)
    assert np.array_equal(xs, xp) and np.allclose(cost - cp, run, rtol=1e-12, atol=1e-13)
    d = oracle.batch_derivatives(om, xs, us, 0.02)
    bound = 1e-6 * max(1.0, np.abs(N).max())
    assert np.abs(mat(d["cxu"])[:, :12] - N).max() <= bound and np.all(d["cxu"][:, 12] == 0)
    # the other blocks: cx and cu gain N u and N'x
    dp = oracle.batch_derivatives(plain, xs, us, 0.02)
    assert np.abs(d["cx"][:, :12] - dp["cx"][:, :12] - us @ N.T).max() <= 1e-8
    assert np.abs(d["cu"][:, :12] - dp["cu"][:, :12] - xs[:, :12] @ N).max() <= 1e-8
    for kk in ("fx", "fu", "cxx", "cuu"):
        assert np.abs(d[kk] - dp[kk]).max() <= bound, kk
    none = oracle.Model("lq", lq=mats, cross=None, u_lim=0.5)
    dn = oracle.batch_derivatives(none, xs, us, 0.02)
    for kk in dn:
        assert np.array_equal(dn[kk], dp[kk]), kk
    with oracle.flavour("f32"):
        d32 = oracle.batch_derivatives(om.twin("f32"), xs, us, 0.02)
    # (float records of double differences: the bound above and the rounding of N and of the record to float)
    assert np.abs(mat(np.asarray(d32["cxu"], dtype=np.float64))[:, :12] - N).max() <= bound + 2 * 2.0 ** -24 * np.abs(N).max()
