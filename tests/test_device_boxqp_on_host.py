"""The product's device box-QP sources (ilqr_amd/csrc/boxqp.hpp are __host__ __device__) compiled
for the HOST and checked against the oracle on a machine without a GPU: the generic projected-Newton
solver for m = 1..4, the scalar solver used for the acrobot, and its straight-line fast path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "devfn_host.hip")
SO = os.path.join(HERE, "native", "libdevfn_host.so")
HIPCC = "/opt/rocm/bin/hipcc"
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def dev():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    hdr = os.path.join(os.path.dirname(HERE), "ilqr_amd", "csrc", "boxqp.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-o", SO, SRC])
    lib = C.CDLL(SO)
    for f in (lib.devfn_box_qp_scalar, lib.devfn_box_qp_scalar_fast):
        f.argtypes = [C.c_double] * 5 + [dp, ip, dp]
    return lib


def _generic(lib, Q, c, x0, lo, hi):
    m = len(c)
    q = np.ascontiguousarray(np.asarray(Q, float).T).ravel()
    c, x0, lo, hi = [np.ascontiguousarray(v, dtype=float) for v in (c, x0, lo, hi)]
    x = np.zeros(m)
    vf = np.zeros(m, dtype=np.int32)
    R = np.zeros(m * m)
    nf = C.c_int(0)
    r = lib.devfn_box_qp(m, q.ctypes.data_as(dp), c.ctypes.data_as(dp), x0.ctypes.data_as(dp), lo.ctypes.data_as(dp),
                         hi.ctypes.data_as(dp), x.ctypes.data_as(dp), vf.ctypes.data_as(ip), R.ctypes.data_as(dp), C.byref(nf))
    return r, x, vf


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_generic_device_boxqp(oracle, dev, m):
    rng = np.random.default_rng(40 + m)
    n_tie = 0
    N = 3000
    for t in range(N):
        A = rng.normal(size=(m, m))
        Q = A @ A.T + (0.05 if t % 5 else -0.3) * np.eye(m)
        c = rng.normal(size=m) * 2
        x0 = rng.normal(size=m)
        lo = -rng.uniform(0.05, 1.5, size=m)
        hi = rng.uniform(0.05, 1.5, size=m)
        ro = oracle.boxqp(Q, c, x0, lo, hi)
        r, x, vf = _generic(dev, Q, c, x0, lo, hi)
        same = (r == ro["result"] and np.array_equal(vf, ro["v_free"]) and np.allclose(x, ro["x_opt"], rtol=1e-9, atol=1e-12))
        if not same:  # rounding-level ties (FMA contraction in the host build of the device code)
            assert r >= 1 and ro["result"] >= 1
            n_tie += 1
    assert n_tie <= N // 200, n_tie


def _qp2(lib, Q, c, x0, lo, hi, detect=0):
    q = np.ascontiguousarray(np.asarray(Q, float).T).ravel()
    c, x0, lo, hi = [np.ascontiguousarray(v, dtype=float) for v in (c, x0, lo, hi)]
    x, vf, mi, nf = np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(3), C.c_int(0)
    r = lib.devfn_box_qp2(q.ctypes.data_as(dp), c.ctypes.data_as(dp), x0.ctypes.data_as(dp), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp),
                          x.ctypes.data_as(dp), vf.ctypes.data_as(ip), mi.ctypes.data_as(dp), C.byref(nf), detect)
    return r, x, vf, mi, nf.value


def test_scalarised_m2_solver(oracle, dev):
    """box_qp2 (the double integrator's box-QP: free-set cases instead of rank-matched selects, adjugate instead of
    Cholesky + two triangular inverses) against the oracle AND the generic device solver: same result code, free set and
    x; positive definite, indefinite (Eigen's unchecked partial factor) and tiny-limit cases; warm starts on the bounds."""
    rng = np.random.default_rng(77)
    n_tie = n_indef = 0
    N = 12000
    for t in range(N):
        A = rng.normal(size=(2, 2))
        Q = A @ A.T + (0.05 if t % 5 else -0.4) * np.eye(2)
        if t % 11 == 0:
            Q = 0.5 * (Q + Q.T) + np.array([[0, 1e-13], [0, 0]])  # not exactly symmetric, as Quu is not
        c = rng.normal(size=2) * 2
        lo = -rng.uniform(0.05, 1.5, size=2)
        hi = rng.uniform(0.05, 1.5, size=2)
        x0 = rng.normal(size=2)
        if t % 3 == 1:
            x0 = np.where(rng.uniform(size=2) < 0.5, lo, hi)
        ro = oracle.boxqp(Q, c, x0, lo, hi)
        r, x, vf, mi, nf = _qp2(dev, Q, c, x0, lo, hi)
        rg, xg, vfg = _generic(dev, Q, c, x0, lo, hi)
        n_indef += int(np.linalg.eigvalsh(0.5 * (Q + Q.T)).min() <= 0)
        for rr, xx, vv in ((ro["result"], ro["x_opt"], ro["v_free"]), (rg, xg, vfg)):
            same = (r == rr or {int(r), int(rr)} == {2, 4}) and np.array_equal(vf, vv) and np.allclose(x, xx, rtol=1e-9, atol=1e-12)
            if not same:  # rounding-level ties: clamp membership / stall test decided by the last bits
                assert r >= 1 and rr >= 1, (t, r, rr)
                n_tie += 1
        if vf.sum() == 2 and r in (4, 5) and np.linalg.eigvalsh(0.5 * (Q + Q.T)).min() > 1e-3:
            Mi = np.array([[mi[0], mi[1]], [mi[1], mi[2]]])
            Ql = np.array([[Q[0, 0], Q[1, 0]], [Q[1, 0], Q[1, 1]]])  # (the factorisation reads the lower triangle)
            assert nf == 2 and np.allclose(Mi @ Ql, np.eye(2), atol=1e-9)
    assert n_indef > N // 10 and n_tie <= N // 150, (n_tie, n_indef)
    # opt-in fix: an indefinite free block ends the QP with -1
    r, *_ = _qp2(dev, [[-1.0, 0.0], [0.0, 2.0]], [0.3, 0.2], [0.0, 0.0], [-1, -1], [1, 1], detect=1)
    assert r == -1


def test_m2_straight_line_part_equals_the_loop(dev):
    """box_qp2 = iteration 0 with the unit step + iteration 1 up to its gradient test, written straight-line, and
    box_qp2_loop for everything else.  Whatever the straight-line part answers must be what the loop leaves: result code,
    x, free set, the compact inverse and its size -- to the last bit on x and Minv up to fused-multiply-add placement
    (1e-15), over positive definite, indefinite, clamped-start and (opt-in) failed-factorisation cases."""
    rng = np.random.default_rng(2024)
    N = 30000
    n_fast_exit = {}
    for t in range(N):
        A = rng.normal(size=(2, 2))
        Q = A @ A.T + (0.05 if t % 5 else -0.4) * np.eye(2)
        if t % 7 == 0:
            Q = Q * 10.0 ** rng.uniform(-3, 6)
        c = rng.normal(size=2) * 2 * (np.abs(Q).max() if t % 7 == 0 else 1.0)
        lo = -rng.uniform(0.05, 1.5, size=2)
        hi = rng.uniform(0.05, 1.5, size=2)
        x0 = rng.normal(size=2)
        if t % 3 == 1:
            x0 = np.where(rng.uniform(size=2) < 0.5, lo, hi)
        detect = int(t % 13 == 0)
        a = _qp2(dev, Q, c, x0, lo, hi, detect)
        q = np.ascontiguousarray(np.asarray(Q, float).T).ravel()
        x, vf, mi, nf = np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(3), C.c_int(0)
        r = dev.devfn_box_qp2_loop(q.ctypes.data_as(dp), c.ctypes.data_as(dp), x0.ctypes.data_as(dp), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp),
                                   x.ctypes.data_as(dp), vf.ctypes.data_as(ip), mi.ctypes.data_as(dp), C.byref(nf), detect)
        assert a[0] == r, (t, a[0], r)
        assert np.array_equal(a[2], vf) and a[4] == nf.value, t
        assert np.allclose(a[1], x, rtol=1e-15, atol=0) and np.allclose(a[3], mi, rtol=1e-14, atol=0), (t, a[1], x, a[3], mi)
        n_fast_exit[r] = n_fast_exit.get(r, 0) + 1
    assert {2, 4, 5, 6} <= set(n_fast_exit) and -1 in n_fast_exit, n_fast_exit


@pytest.mark.parametrize("m", [2])
def test_scalarised_m2_solver_reproduces_the_reference_vectors(dev, m):
    """tests/golden/ref_pieces.npz qp2_*: inputs and outputs of the REAL src/boxqp.cpp (scripts/make_golden.py)."""
    d = np.load(os.path.join(HERE, "golden", "ref_pieces.npz"))
    n = len(d["qp2_result"])
    ties = 0
    for i in range(n):
        r, x, vf, mi, nf = _qp2(dev, d["qp2_Q"][i], d["qp2_c"][i], d["qp2_x0"][i], d["qp2_lo"][i], d["qp2_hi"][i])
        if r != d["qp2_result"][i]:
            assert {int(r), int(d["qp2_result"][i])} == {2, 4}  # converged-point tie
            ties += 1
        assert np.array_equal(vf, d["qp2_v_free"][i]), i
        assert np.allclose(x, d["qp2_x_opt"][i], rtol=1e-10, atol=1e-13), i
    assert n >= 200 and ties <= n // 20


def test_scalar_solver_and_fast_path(oracle, dev):
    rng = np.random.default_rng(3)
    n_slow = n_tie = 0
    N = 20000
    for t in range(N):
        Q = rng.uniform(0.01, 5) if t % 7 else rng.uniform(-2, 0.01)
        c = rng.normal() * 2
        lo, hi = -rng.uniform(0.01, 2), rng.uniform(0.01, 2)
        x0 = (rng.normal(), lo, hi)[t % 3]
        ro = oracle.boxqp([[Q]], [c], [x0], [lo], [hi])
        for fn in (dev.devfn_box_qp_scalar, dev.devfn_box_qp_scalar_fast):
            x, fr, mv = C.c_double(), C.c_int(), C.c_double()
            r = fn(Q, c, x0, lo, hi, C.byref(x), C.byref(fr), C.byref(mv))
            assert r >= 0  # (the fast path continues by itself when a QP needs a third iteration)
            ok = fr.value == ro["v_free"][0] and abs(x.value - ro["x_opt"][0]) <= 1e-12 * max(1, abs(x.value))
            code_ok = r == ro["result"] or (Q <= 0 and {r, ro["result"]} == {2, 4})
            if not (ok and code_ok):
                n_tie += 1  # clamp membership decided by a rounding-noise gradient (boxqp.h:61-64)
            assert (Q > 0) == (abs(mv.value - 1.0 / Q) <= 1e-15 * abs(1.0 / Q)) or Q <= 0
    assert n_tie <= 4


def test_float_instantiation_against_the_fp32_oracle(oracle, dev):
    """The box-QP sources instantiated for float (the product's fp32 mode, BASELINE configs[3]) against the
    oracle's float build (liboracle_ilqr_f32.so): same results up to float rounding; the float-noise ties
    (clamp membership / stall exit decided by the last bit) are counted."""
    fp = C.POINTER(C.c_float)
    for f in (dev.devfn_box_qp_scalar_f32, dev.devfn_box_qp_scalar_fast_f32):
        f.argtypes = [C.c_float] * 5 + [fp, ip, fp]
    rng = np.random.default_rng(8)
    n_tie, N = 0, 6000
    with oracle.flavour("f32"):
        for t in range(N):
            m = 1 + t % 4
            A = rng.normal(size=(m, m))
            Q = (A @ A.T + 0.2 * np.eye(m)).astype(np.float32)
            c = (rng.normal(size=m) * 2).astype(np.float32)
            x0 = rng.normal(size=m).astype(np.float32)
            lo = (-rng.uniform(0.05, 1.5, size=m)).astype(np.float32)
            hi = rng.uniform(0.05, 1.5, size=m).astype(np.float32)
            ro = oracle.boxqp(Q, c, x0, lo, hi)
            q = np.ascontiguousarray(Q.T).ravel()
            x = np.zeros(m, dtype=np.float32)
            vf = np.zeros(m, dtype=np.int32)
            r = dev.devfn_box_qp_f32(m, q.ctypes.data_as(fp), c.ctypes.data_as(fp), x0.ctypes.data_as(fp), lo.ctypes.data_as(fp),
                                     hi.ctypes.data_as(fp), x.ctypes.data_as(fp), vf.ctypes.data_as(ip))
            same = np.array_equal(vf, ro["v_free"]) and np.allclose(x, ro["x_opt"], rtol=2e-4, atol=2e-5)
            if not same or (r != ro["result"] and {int(r), int(ro["result"])} != {2, 4}):
                assert r >= 1 and ro["result"] >= 1
                n_tie += 1
            if m == 2:
                x2, vf2 = np.zeros(2, dtype=np.float32), np.zeros(2, dtype=np.int32)
                r2 = dev.devfn_box_qp2_f32(q.ctypes.data_as(fp), c.ctypes.data_as(fp), x0.ctypes.data_as(fp), lo.ctypes.data_as(fp),
                                           hi.ctypes.data_as(fp), x2.ctypes.data_as(fp), vf2.ctypes.data_as(ip))
                assert r2 >= 1
                if not (np.array_equal(vf2, ro["v_free"]) and np.allclose(x2, ro["x_opt"], rtol=2e-4, atol=2e-5)):
                    n_tie += 1
            if m == 1:
                for fn in (dev.devfn_box_qp_scalar_f32, dev.devfn_box_qp_scalar_fast_f32):
                    xs, fr, mv = C.c_float(), C.c_int(), C.c_float()
                    rs = fn(float(Q[0, 0]), float(c[0]), float(x0[0]), float(lo[0]), float(hi[0]), C.byref(xs), C.byref(fr), C.byref(mv))
                    assert rs >= 0
                    if fr.value != ro["v_free"][0] or abs(xs.value - ro["x_opt"][0]) > 2e-5 + 2e-4 * abs(xs.value):
                        n_tie += 1
    assert n_tie <= N // 100, n_tie


def test_gradient_norm_test_without_the_square_root(dev):
    """boxqp.cpp:93-97 tests sqrt(|g|^2) < 1e-8; the device code tests |g|^2 < y* (the smallest value whose correctly
    rounded root is >= 1e-8).  Equivalent for every input: checked on the 4001 doubles / floats around the threshold,
    on random magnitudes, and on 0 / denormals / inf / nan."""
    dev.devfn_grad_norm_below_min.argtypes = [C.c_double]
    dev.devfn_grad_norm_below_min_f32.argtypes = [C.c_float]
    t = np.float64(1e-8)
    y = t * t
    cases = [0.0, 5e-324, 1e-300, 1e-20, 1e-12, 1.0, 1e300, np.inf, np.nan]
    v = y
    for _ in range(2000):
        v = np.nextafter(v, 0)
    for _ in range(4001):
        cases.append(float(v))
        v = np.nextafter(v, 1)
    cases += list(10.0 ** np.random.default_rng(0).uniform(-40, 5, 2000))
    for gn2 in cases:
        assert bool(dev.devfn_grad_norm_below_min(gn2)) == bool(np.sqrt(np.float64(gn2)) < t), gn2
    t32 = np.float32(1e-8)
    v = np.float32(t32 * t32)
    cases32 = [np.float32(0), np.float32(1e-45), np.float32(1e-30), np.float32(1.0), np.float32(np.inf), np.float32(np.nan)]
    for _ in range(2000):
        v = np.nextafter(v, np.float32(0))
    for _ in range(4001):
        cases32.append(v)
        v = np.nextafter(v, np.float32(1))
    for gn2 in cases32:
        assert bool(dev.devfn_grad_norm_below_min_f32(float(gn2))) == bool(np.sqrt(np.float32(gn2)) < t32), gn2


def test_finish_predicates_equal_the_result_code(dev):
    """qp1_finish_ok (boxqp.hpp: what the kernels call -- success and "goes on" as predicates) against qp1_finish (the
    reference's result code 4 / 5 / 6 / 2 / -1): same x, free flag, minv; goes_on <=> code == "goes on"; ok <=> code >= 1.
    Positive definite, indefinite (with and without the opt-in detection), warm starts on the bounds."""
    dev.devfn_qp1_finish_flavours_agree.argtypes = [C.c_double] * 5 + [C.c_int]
    rng = np.random.default_rng(17)
    n_goes_on = 0
    for t in range(40000):
        Q = rng.uniform(0.01, 5) if t % 7 else rng.uniform(-2, 0.01)
        c = rng.normal() * 2
        lo, hi = -rng.uniform(0.01, 2), rng.uniform(0.01, 2)
        x0 = (rng.normal(), lo, hi)[t % 3]
        for det in (0, 1):
            r = dev.devfn_qp1_finish_flavours_agree(Q, c, x0, lo, hi, det)
            assert r == 0, (r, Q, c, x0, lo, hi, det)


# ---------------------------------------------------------------------------------------------------------------------------------
# Boxes a real solve hands the box-QP (the box is [u_min - u, u_max - u], src/ilqr_core.cpp:369, and the forward pass does not clamp):
# an edge exactly 0 (u sits on a limit), boxes that exclude 0 (feedback or the caller's u0 put u outside its limits), pinned
# controls (lo == hi), unbounded controls (+-inf) and huge finite ones (+-1e300); and warm starts outside the box.
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = ("excludes_0_above", "excludes_0_below", "edge_at_0", "pinned", "infinite", "huge", "x0_outside")


def _box(rng, shape, m):
    a, b = rng.uniform(0.05, 1.2, size=m), rng.uniform(0.05, 1.5, size=m)
    if shape == "excludes_0_above":
        lo, hi = a, a + b
    elif shape == "excludes_0_below":
        lo, hi = -a - b, -a
    elif shape == "edge_at_0":
        up = rng.uniform(size=m) < 0.5
        lo, hi = np.where(up, 0.0, -a), np.where(up, b, 0.0)
    elif shape == "pinned":
        v = np.where(rng.uniform(size=m) < 0.3, 0.0, rng.uniform(-1, 1, size=m))
        lo, hi = v, v.copy()
    elif shape == "infinite":
        lo, hi = np.full(m, -np.inf), np.full(m, np.inf)
    elif shape == "huge":
        lo, hi = np.full(m, -1e300), np.full(m, 1e300)
    else:
        lo, hi = -a, b
    if shape not in ("x0_outside",) and m > 1 and rng.uniform() < 0.5:  # half the problems mix this shape with ordinary boxes
        keep = rng.uniform(size=m) < 0.5
        lo, hi = np.where(keep, lo, -a), np.where(keep, hi, b)
    return lo, hi


def _x0(rng, shape, lo, hi):
    m = len(lo)
    if shape == "x0_outside":
        side = rng.uniform(size=m) < 0.5
        return np.where(side, lo - rng.uniform(0.01, 2, size=m), hi + rng.uniform(0.01, 2, size=m))
    x0 = rng.normal(size=m)
    pick = rng.uniform(size=m)
    fin = np.isfinite(lo) & (np.abs(lo) < 1e100)
    return np.where((pick < 0.25) & fin, lo, np.where((pick < 0.5) & fin, hi, x0))


def _problems(seed, m, N, indefinite_every=5):
    """N problems of dimension m, cycling through SHAPES; every `indefinite_every`-th Q indefinite (Eigen's unchecked factor)."""
    rng = np.random.default_rng(seed)
    for t in range(N):
        shape = SHAPES[t % len(SHAPES)]
        A = rng.normal(size=(m, m))
        Q = A @ A.T + (-0.3 if indefinite_every and t % indefinite_every == 0 else 0.05) * np.eye(m)
        c = rng.normal(size=m) * 2
        lo, hi = _box(rng, shape, m)
        yield t, shape, Q, c, _x0(rng, shape, lo, hi), lo, hi


def _same_x(x, xo, rtol, atol):
    return np.allclose(x, xo, rtol=rtol, atol=atol, equal_nan=True)


def _in_box(x, lo, hi):
    return bool(np.all((x >= lo) & (x <= hi)))


def _kkt_residual(Q, c, x, lo, hi):
    """Projected gradient of 1/2 x'Qx + c'x at x in extended precision: | x - clip(x - g, lo, hi) | per component, scaled by |g| + 1."""
    L = np.longdouble
    Ql, cl, xl = np.asarray(Q, dtype=L), np.asarray(c, dtype=L), np.asarray(x, dtype=L)
    g = Ql @ xl + cl
    pg = np.abs(xl - np.clip(xl - g, np.asarray(lo, dtype=L), np.asarray(hi, dtype=L)))
    return float((pg / (np.abs(g) + 1)).max())


KKT_TOL = 1e-7  # (result 5: the free gradient is below 1e-8; result 6: every clamped x sits exactly on its bound)


def _check_invariants(Q, x, r, lo, hi, c, what):
    if r >= 1 and np.all(lo <= hi):
        assert _in_box(x, lo, hi), (what, x, lo, hi)
    if r in (5, 6) and np.linalg.eigvalsh(0.5 * (Q + Q.T)).min() > 1e-2:
        res = _kkt_residual(Q, c, x, lo, hi)
        assert res <= KKT_TOL, (what, r, res, x, lo, hi)
        return 1
    return 0


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_generic_solver_on_solve_shaped_boxes(oracle, dev, m):
    """box_qp<m> on every box shape against the oracle: same result code, free set and x (1e-9), rounding ties counted with
    the budget of test_generic_device_boxqp; x in its box and, for a clearly positive definite Q, KKT at exits 5 / 6."""
    N, n_tie, n_kkt, seen = 2100, 0, 0, set()
    for t, shape, Q, c, x0, lo, hi in _problems(140 + m, m, N):
        ro = oracle.boxqp(Q, c, x0, lo, hi)
        r, x, vf = _generic(dev, Q, c, x0, lo, hi)
        same = r == ro["result"] and np.array_equal(vf, ro["v_free"]) and _same_x(x, ro["x_opt"], 1e-9, 1e-12)
        if not same:
            assert r >= 1 and ro["result"] >= 1, (t, shape, r, ro["result"])
            n_tie += 1
        n_kkt += _check_invariants(Q, x, r, lo, hi, c, (t, shape))
        seen.add((shape, int(r)))
    assert n_tie <= N // 200, n_tie
    assert n_kkt > N // 3, n_kkt
    assert {s for s, _ in seen} == set(SHAPES)


def test_m2_solver_on_solve_shaped_boxes(oracle, dev):
    """box_qp2 (the double integrator's solver) on every box shape against the oracle and the generic solver."""
    N, n_tie, n_kkt = 7000, 0, 0
    for t, shape, Q, c, x0, lo, hi in _problems(240, 2, N):
        ro = oracle.boxqp(Q, c, x0, lo, hi)
        r, x, vf, mi, nf = _qp2(dev, Q, c, x0, lo, hi)
        rg, xg, vfg = _generic(dev, Q, c, x0, lo, hi)
        for rr, xx, vv in ((ro["result"], ro["x_opt"], ro["v_free"]), (rg, xg, vfg)):
            same = (r == rr or {int(r), int(rr)} == {2, 4}) and np.array_equal(vf, vv) and _same_x(x, xx, 1e-9, 1e-12)
            if not same:
                assert r >= 1 and rr >= 1, (t, shape, r, rr)
                n_tie += 1
        n_kkt += _check_invariants(Q, x, r, lo, hi, c, (t, shape))
    assert n_tie <= N // 150, n_tie
    assert n_kkt > N // 3, n_kkt


def test_scalar_solvers_on_solve_shaped_boxes(oracle, dev):
    """box_qp_scalar and its straight-line fast path (the acrobot's solver) on every box shape against the oracle."""
    N, n_tie, n_kkt = 7000, 0, 0
    for t, shape, Q, c, x0, lo, hi in _problems(340, 1, N, indefinite_every=7):
        ro = oracle.boxqp(Q, c, x0, lo, hi)
        q = float(Q[0, 0])
        for fn in (dev.devfn_box_qp_scalar, dev.devfn_box_qp_scalar_fast):
            x, fr, mv = C.c_double(), C.c_int(), C.c_double()
            r = fn(q, float(c[0]), float(x0[0]), float(lo[0]), float(hi[0]), C.byref(x), C.byref(fr), C.byref(mv))
            assert r >= 0
            xo = ro["x_opt"][0]
            ok = fr.value == ro["v_free"][0] and (x.value == xo or abs(x.value - xo) <= 1e-12 * max(1, abs(x.value)))
            code_ok = r == ro["result"] or (q <= 0 and {r, ro["result"]} == {2, 4})
            if not (ok and code_ok):
                assert r >= 1 and ro["result"] >= 1, (t, shape, r, ro["result"])
                n_tie += 1
            n_kkt += _check_invariants(Q, np.array([x.value]), r, lo, hi, c, (t, shape))
    assert n_tie <= 4, n_tie
    assert n_kkt > N // 2, n_kkt


def test_float_solvers_on_solve_shaped_boxes(oracle, dev):
    """The float instantiations (box_qp<1..4>, box_qp2, the scalar solver and its fast path) on every box shape (+-1e300 becomes
    +-inf in float, as a float handle's limits do) against the oracle's float build, with the tie budget of
    test_float_instantiation_against_the_fp32_oracle; x in its box whatever the shape.  One more kind of tie is counted apart:
    same x and free set, but exit 5 (free gradient below 1e-8: in float that means exactly zero) on one side and 2 (no
    improvement) on the other -- an unclamped minimum, common in unbounded boxes, where FMA contraction decides whether
    Q x + c rounds to exactly 0."""
    fp = C.POINTER(C.c_float)
    for f in (dev.devfn_box_qp_scalar_f32, dev.devfn_box_qp_scalar_fast_f32):
        f.argtypes = [C.c_float] * 5 + [fp, ip, fp]
    N, n_tie, n_exit_tie = 0, 0, 0
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    with oracle.flavour("f32"):
        for m in (1, 2, 3, 4):
            for t, shape, Q, c, x0, lo, hi in _problems(440 + m, m, 1400, indefinite_every=0):
                N += 1
                with np.errstate(over="ignore"):
                    Q, c, x0, lo, hi = f32(Q + 0.15 * np.eye(m)), f32(c), f32(x0), f32(lo), f32(hi)
                ro = oracle.boxqp(Q, c, x0, lo, hi)
                q = np.ascontiguousarray(Q.T).ravel()
                x = np.zeros(m, dtype=np.float32)
                vf = np.zeros(m, dtype=np.int32)
                ptr = lambda a: a.ctypes.data_as(fp)
                r = dev.devfn_box_qp_f32(m, ptr(q), ptr(c), ptr(x0), ptr(lo), ptr(hi), ptr(x), vf.ctypes.data_as(ip))
                outs = [(r, x, vf)]
                if m == 2:
                    x2, vf2 = np.zeros(2, dtype=np.float32), np.zeros(2, dtype=np.int32)
                    r2 = dev.devfn_box_qp2_f32(ptr(q), ptr(c), ptr(x0), ptr(lo), ptr(hi), ptr(x2), vf2.ctypes.data_as(ip))
                    outs.append((r2, x2, vf2))
                if m == 1:
                    for fn in (dev.devfn_box_qp_scalar_f32, dev.devfn_box_qp_scalar_fast_f32):
                        xs, fr, mv = C.c_float(), C.c_int(), C.c_float()
                        rs = fn(float(Q[0, 0]), float(c[0]), float(x0[0]), float(lo[0]), float(hi[0]), C.byref(xs), C.byref(fr), C.byref(mv))
                        outs.append((rs, np.array([xs.value], dtype=np.float32), np.array([fr.value], dtype=np.int32)))
                for rr, xx, vv in outs:
                    assert rr >= 1, (m, t, shape, rr)
                    assert _in_box(xx, lo, hi), (m, t, shape, xx, lo, hi)
                    same = np.array_equal(vv, ro["v_free"]) and _same_x(xx, ro["x_opt"], 2e-4, 2e-5)
                    if same and {int(rr), int(ro["result"])} == {2, 5}:
                        n_exit_tie += 1
                    elif not same or (rr != ro["result"] and {int(rr), int(ro["result"])} != {2, 4}):
                        assert ro["result"] >= 1, (m, t, shape, ro["result"])
                        n_tie += 1
    assert n_tie <= N // 100, (n_tie, N)
    assert n_exit_tie <= N // 10, (n_exit_tie, N)
