"""Derivative records with a dense state-control block (cxu != 0) for the backward kernels, and the coupled LQ twin's parameters
(test infrastructure; tests/test_coupled_inputs.py proves on the CPU what the GPU tests assume about them).

Both shipped nx = 4 models have a cost without a state-control term and the LQ twin hard-codes cxu = 0, so the records every other
test hands a backward kernel carry cxu = 0 or finite-difference noise.  coupled_records draws the whole cost Hessian
[cxx cxu; cxu' cuu] = 0.5 I + G G' of one positive definite matrix per knot: cxu is as large as cxx and cuu, all its entries differ,
and for nu >= 2 it is not symmetric in any way a transposed or mis-strided read could survive.

The family is FIXED (seeds 1 and 2, fu scaled by 0.2): with fu ~ N(0, 1) / sqrt(n) and boxes, the fp64 oracle parts from its own x87
yardstick on box-QP knife edges at m >= 16 and lambda = 1e-3, which no kernel can be held to.  On this family it does not
(test_coupled_inputs.py), so a kernel that misses the project's tolerances here is wrong."""
import numpy as np

from tests.util import mat

B, T = 9, 14
SEEDS = (1, 2)
LAMBDAS = (1.0, 1e-3)
NX4_SHAPES = [(4, 1), (4, 2)]                         # k_backward_q, k_backward_t (acrobot and double-integrator handles)
HOST_SHAPES = [(32, 16), (17, 9), (6, 2), (31, 1), (3, 1)]   # k_backward_w3 and k_backward_w2
TWO_TILE_SHAPES = [(12, 16), (32, 16)]                # ILQR_ROUTE_TWO_CONTROL_TILES against one tile
WIDE_SHAPES = [(20, 17), (24, 20), (32, 32)]          # nu > 16: two control tiles natively
REGV_SHAPES = [(32, 16), (6, 2), (4, 1), (4, 2)]      # ILQR_FLAG_REGULARIZE_VXX
ALL_SHAPES = NX4_SHAPES + HOST_SHAPES + [(12, 16)] + WIDE_SHAPES
MATRICES = ("fx", "fu", "cxx", "cxu", "cuu")


def coupled_records(n, m, B, T, seed):
    rng = np.random.default_rng(1000 * seed + 100 * n + m)
    G = rng.normal(size=(B, T + 1, n + m, n + m)) / np.sqrt(n + m)
    H = 0.5 * np.eye(n + m) + G @ np.swapaxes(G, -1, -2)        # [cxx cxu; cxu' cuu], positive definite
    return dict(fx=np.eye(n) + 0.1 * rng.normal(size=(B, T + 1, n, n)) / np.sqrt(n),
                fu=0.2 * rng.normal(size=(B, T + 1, n, m)) / np.sqrt(n),
                cx=rng.normal(size=(B, T + 1, n)), cu=rng.normal(size=(B, T + 1, m)),
                cxx=H[..., :n, :n].copy(), cxu=H[..., :n, n:].copy(), cuu=H[..., n:, n:].copy())


def coupled_case(m, B, T, seed):
    rng = np.random.default_rng(seed)
    lo, hi = -rng.uniform(0.1, 0.6, m), rng.uniform(0.1, 0.6, m)
    return lo, hi, rng.uniform(-0.05, 0.05, (B, T, m)), rng.normal(size=(B, T, m)) * 0.1   # lo, hi, us, k_prev


def case(n, m, seed, f32=False):
    """(records in math layout [row][col], lo, hi, us, k_prev) of one shape and seed; f32: every array rounded to float first, so that
    a float handle and the float oracle are given the same numbers."""
    rec = coupled_records(n, m, B, T, seed)
    lo, hi, us, k_prev = coupled_case(m, B, T, seed)
    if f32:
        r = lambda a: np.asarray(a, np.float32).astype(np.float64)
        rec, lo, hi, us, k_prev = {k: r(v) for k, v in rec.items()}, r(lo), r(hi), r(us), r(k_prev)
    return rec, lo, hi, us, k_prev


def memory_layout(rec):
    """math layout -> the oracle's (column-major matrices: [..., col, row])"""
    return {k: np.ascontiguousarray(mat(v) if k in MATRICES else v) for k, v in rec.items()}


def box_model(oracle, n, m, lo, hi):
    """An oracle model of these dimensions and limits; batch_backward reads nothing else of it."""
    z = np.zeros
    return oracle.Model("lq", lq=(z((n, n)), z((n, m)), z((n, n)), z((m, m)), z((n, n))), u_min=lo, u_max=hi)


def oracle_backward(oracle, om, us, rec, k_prev, lam, flav="f64"):
    """oracle.batch_backward on math-layout records in one arithmetic flavour; everything back as float64, K as [B][T][nu][nx]."""
    with oracle.flavour(flav):
        omt = om if om.flavour == flav else om.twin(flav)
        r = oracle.batch_backward(omt, us, memory_layout(rec), k_prev=k_prev, lam=lam)
    r = {k: (np.asarray(v, dtype=np.float64) if v.dtype.kind == "f" else v) for k, v in r.items()}
    r["Km"] = mat(r["K"])
    return r


def mis_strided(cxu):
    """What a kernel would see that read the n x m block with the strides of an m x n one."""
    b, t, n, m = cxu.shape
    return np.ascontiguousarray(cxu.reshape(b, t, m, n).swapaxes(-1, -2))


def clamped_share(K):
    """share of the rows of K [B][T][nu][nx] that are exactly zero (a clamped control: ilqr_core.cpp:373-385)"""
    return float((np.abs(K).max(axis=-1) == 0).mean())


# ---------------------------------------------------------------------------------------------------------------------------------
# the coupled LQ twin: xdot = A x + B u, cost 0.5 x'Qx + 0.5 u'Ru + x'N u, final cost 0.5 x'Qf x
# ---------------------------------------------------------------------------------------------------------------------------------
# the seed of each twin's matrices: the first at which [[Q, N], [N', R]] is positive definite by the margin test_coupled_inputs.py asks
# for (dense_mats' R is 0.2 (I + ...), of the size of N'N: most seeds give a cost that is not convex)
TWIN_SEED = {(4, 1): 4, (4, 2): 4, (6, 2): 12}


def cross_term(n, m, seed):
    """N = 0.3 normal / sqrt(n), every entry different from every other (and from its negative)."""
    N = 0.3 * np.random.default_rng(7000 + 100 * seed + 10 * n + m).normal(size=(n, m)) / np.sqrt(n)
    assert len(np.unique(np.abs(N).round(6))) == N.size
    return N


def coupled_mats(n, m, seed):
    """(A, B, Q, R, Qf), N with [[Q, N], [N', R]] positive definite: least eigenvalue >= 0.05."""
    from tests.test_gpu_lq_end_to_end import dense_mats
    mats = dense_mats(n, m, seed)
    N = cross_term(n, m, seed)
    return mats, N


def cost_hessian(mats, N):
    Q, R = np.asarray(mats[2]), np.asarray(mats[3])
    return np.block([[0.5 * (Q + Q.T), N], [N.T, 0.5 * (R + R.T)]])


def twin_params(mats, N=None):
    """user_params of the coupled twins: A, B, Q, R, Qf, N row-major"""
    return np.concatenate([np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (tuple(mats) + (() if N is None else (N,)))])


def twin_start(n, m, Bt, Tt, seed):
    rng = np.random.default_rng(900 + seed)
    return rng.uniform(-1, 1, (Bt, n)), rng.normal(size=(Bt, Tt, m)) * 0.1
