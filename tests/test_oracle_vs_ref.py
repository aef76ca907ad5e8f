"""The oracle against the REAL reference code (oracle/_ref/libref_ilqr.so = the reference's
src/boxqp.cpp, finite_diff.h and model headers compiled where they lie).  The shim can only be
built where the reference sources are, so its answers to every case below are also recorded in
tests/golden/ref_answers.npz (scripts/make_golden.py): where the shim is built the tests ask it and
require the recording to hold the same bits; everywhere else they compare the oracle with the recording."""
import hashlib
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_answers.npz")


def _inputs_digest(cases):
    h = hashlib.sha256()
    for case in cases:
        for a in case:
            h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def pack(name, cases, answers):
    """One test's cases and the reference's answers (one dict of scalars / arrays per case) as flat npz entries: per field the
    values of all cases end to end (float64) and each case's shape (-1 = no such dimension); the digest of the inputs."""
    out = {name + ".inputs_sha256": _inputs_digest(cases)}
    for f in answers[0]:
        vals = [np.asarray(a[f], dtype=np.float64) for a in answers]
        out["%s.%s.data" % (name, f)] = np.concatenate([v.ravel() for v in vals])
        out["%s.%s.shape" % (name, f)] = np.array([list(v.shape) + [-1] * (2 - v.ndim) for v in vals], dtype=np.int8)
    return out


def unpack(d, name):
    fields = sorted({k.split(".")[1] for k in d.files if k.startswith(name + ".") and k.endswith(".data")})
    per = {}
    for f in fields:
        shapes = [tuple(s for s in row if s >= 0) for row in d["%s.%s.shape" % (name, f)]]
        ends = np.cumsum([int(np.prod(s)) for s in shapes])
        data = d["%s.%s.data" % (name, f)]
        per[f] = [data[e - int(np.prod(s)):e].reshape(s) for s, e in zip(shapes, ends)]
        per[f] = [v.item() if v.ndim == 0 else v for v in per[f]]  # (scalars as Python numbers)
    return [{f: per[f][i] for f in fields} for i in range(len(per[fields[0]]))]


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def reference(O, name, cases, ask):
    """The reference's answers to `cases` (ask(*case) -> dict): the recording, which must be of these very inputs, and which
    must equal the shim's answers bit for bit where the shim is built."""
    d = np.load(GOLDEN)
    assert np.array_equal(d[name + ".inputs_sha256"], _inputs_digest(cases)), \
        "%s: the cases drawn here are not the ones recorded (re-record with scripts/make_golden.py)" % name
    rec = unpack(d, name)
    assert len(rec) == len(cases)
    if O.ref_available():
        for case, r in zip(cases, rec):
            live = ask(*case)
            assert set(live) == set(r) and all(_same_bits(live[f], r[f]) for f in r), name
    return rec


# ---- the cases (seeded) and what is asked of the reference about each ----

def boxqp_small_cases(m):
    rng = np.random.default_rng(10 + m)
    cases = []
    for trial in range(4000):
        A = rng.normal(size=(m, m))
        Q = A @ A.T + (0.05 if trial % 4 else -0.3) * np.eye(m)
        c = rng.normal(size=m) * 2
        x0 = rng.normal(size=m)
        lo = -rng.uniform(0.05, 1.5, size=m)
        hi = rng.uniform(0.05, 1.5, size=m)
        cases.append((Q, c, x0, lo, hi))
    return cases


def boxqp_random_pd_cases():
    rng = np.random.default_rng(0)
    cases = []
    for trial in range(6000):
        m = int(rng.integers(1, 7))
        A = rng.normal(size=(m, m))
        Q = A @ A.T + 0.05 * np.eye(m)
        c = rng.normal(size=m) * 2
        x0 = rng.normal(size=m)
        lo = -rng.uniform(0.05, 1.5, size=m)
        hi = rng.uniform(0.05, 1.5, size=m)
        cases.append((Q, c, x0, lo, hi))
    return cases


def line_search_cases():
    rng = np.random.default_rng(1)
    cases = []
    for _ in range(3000):
        m = int(rng.integers(1, 6))
        A = rng.normal(size=(m, m))
        Q = A @ A.T + 0.1 * np.eye(m)
        c, x0, d = rng.normal(size=m), rng.normal(size=m), rng.normal(size=m)
        lo, hi = -rng.uniform(0.1, 2, size=m), rng.uniform(0.1, 2, size=m)
        cases.append((x0, d, Q, c, lo, hi))
    return cases


MODELS = [(0, "acrobot", None), (1, "integrator", [1, .5, 0, 0])]
FD_NAMES = ("fx", "fu", "cx", "cu", "cxx", "cuu")


def model_cases(nu):
    rng = np.random.default_rng(2)
    cases = []
    for _ in range(200):
        x = rng.uniform(-1, 1, 4) * np.array([np.pi, np.pi, 3, 3])
        u = rng.uniform(-5, 5, nu)
        cases.append((x, u))
    return cases


def ask_boxqp(O):
    def ask(Q, c, x0, lo, hi):
        r = O.ref_boxqp(Q, c, x0, lo, hi)
        a = {k: r[k] for k in ("result", "x_opt", "v_free", "R_free")}
        # R_free only where the oracle has a factor, the one place the tests compare it: where nothing was factorised in the call,
        # the reference hands back what its free-set matrix last held -- uninitialised memory at result 6
        if not O.boxqp(Q, c, x0, lo, hi)["R_free"].size:
            a["R_free"] = np.zeros((0, 0))
        return a
    return ask


def ask_line_search(O):
    def ask(x0, d, Q, c, lo, hi):
        r = O.ref_line_search(x0, d, Q, c, lo, hi)
        return dict(failed=r["failed"], n_steps=r["n_steps"], x_opt=r["x_opt"], v_opt=r["v_opt"],
                    quad_cost=O.ref_quad_cost(Q, c, x0), clamp=O.ref_clamp(x0, lo, hi))
    return ask


def ask_model(O, mid, goal, dt=0.02):
    def ask(x, u):
        dx, x1, c, f = O.ref_model_eval(mid, goal, x, u, dt)
        a = dict(dx=dx, x1=x1, c=c, f=f)
        for is_final in (0, 1):
            r = O.ref_fd_knot(mid, goal, x, u, dt, is_final)
            for kname in FD_NAMES:
                a["fd%d_%s" % (is_final, kname)] = r[kname]
        return a
    return ask


def record(O):
    """Every test's recording (scripts/make_golden.py writes it, with the shim built)."""
    out = {}
    for name, cases, ask in ([("boxqp_small_m%d" % m, boxqp_small_cases(m), ask_boxqp(O)) for m in (1, 2)] +
                             [("boxqp_random_pd", boxqp_random_pd_cases(), ask_boxqp(O)),
                              ("line_search", line_search_cases(), ask_line_search(O))] +
                             [("model_" + name, model_cases(1 if mid == 0 else 2), ask_model(O, mid, goal)) for mid, name, goal in MODELS]):
        out.update(pack(name, cases, [ask(*c) for c in cases]))
    return out


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


def test_ref_kats(O):
    """test/test_finite_diff.cpp:13-32 on the reference's own operators (a check of the shim itself: only where it is built)."""
    if not O.ref_available():
        pytest.skip("reference shim not built (no reference sources here)")
    assert abs(O.ref().ref_fd_scalar_negquad(-1.0) - 2) < 1e-6
    import ctypes as C
    out = np.zeros(2)
    x = np.array([1.0, 1.0])
    O.ref().ref_fd_grad_quadvec(x.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)))
    assert np.allclose(out, [2, 10], atol=1e-6)


@pytest.mark.parametrize("m", [1, 2])
def test_boxqp_exact_small(O, m):
    """m = 1, 2 (the shipped models' control dimensions): identical result code, free set and
    solution on every case, PD or not."""
    cases = boxqp_small_cases(m)
    for (Q, c, x0, lo, hi), b in zip(cases, reference(O, "boxqp_small_m%d" % m, cases, ask_boxqp(O))):
        a = O.boxqp(Q, c, x0, lo, hi)
        if m == 2 and a["result"] != b["result"]:
            # 2 <-> 4 at a converged point is a rounding-level tie (see test below)
            assert {a["result"], b["result"]} == {2, 4}
        else:
            assert a["result"] == b["result"]
        assert np.array_equal(a["v_free"], b["v_free"])
        assert np.allclose(a["x_opt"], b["x_opt"], rtol=1e-10, atol=1e-13, equal_nan=True)
        if a["R_free"].size:
            assert np.allclose(a["R_free"], b["R_free"], rtol=1e-12, atol=1e-14, equal_nan=True)


def test_boxqp_random_pd(O):
    """Positive-definite Q, m up to 6.  The oracle forms R^-1 R^-T by a triangular solve where
    the reference uses two PartialPivLU inverses: identical up to rounding,
    so >= 99.8 % of cases must agree on code, free set and x; the rest are knife-edge ties."""
    cases = boxqp_random_pd_cases()
    n_ok = n = 0
    for (Q, c, x0, lo, hi), b in zip(cases, reference(O, "boxqp_random_pd", cases, ask_boxqp(O))):
        a = O.boxqp(Q, c, x0, lo, hi)
        n += 1
        same = (a["result"] == b["result"] and np.array_equal(a["v_free"], b["v_free"]) and
                np.allclose(a["x_opt"], b["x_opt"], rtol=1e-9, atol=1e-12))
        n_ok += same
        assert a["result"] >= 1 and b["result"] >= 1
    assert n_ok >= 0.998 * n, (n_ok, n)


def test_line_search_and_helpers(O):
    cases = line_search_cases()
    for (x0, d, Q, c, lo, hi), b in zip(cases, reference(O, "line_search", cases, ask_line_search(O))):
        a = O.line_search(x0, d, Q, c, lo, hi)
        assert a["failed"] == b["failed"] and a["n_steps"] == b["n_steps"]
        assert np.allclose(a["x_opt"], b["x_opt"], rtol=1e-12, equal_nan=True)
        assert np.isclose(a["v_opt"], b["v_opt"], rtol=1e-12, equal_nan=True)
        assert np.isclose(O.quad_cost(Q, c, x0), b["quad_cost"], rtol=1e-13, atol=1e-13)
        assert np.array_equal(O.clamp_to_limits(x0, lo, hi), b["clamp"])


@pytest.mark.parametrize("mid,name,goal", MODELS)
def test_models_and_fd_bit_exact(O, mid, name, goal):
    """dynamics / Euler step / cost / final_cost and every finite-difference array of a knot
    point equal the reference's BIT FOR BIT (same operation order, same libm, no FMA)."""
    m = O.Model(name, goal=goal)
    dt = 0.02
    cases = model_cases(m.nu)
    for (x, u), r in zip(cases, reference(O, "model_" + name, cases, ask_model(O, mid, goal, dt))):
        assert np.array_equal(r["dx"], m.dynamics(x, u))
        assert np.array_equal(r["x1"], m.integrate(x, u, dt))
        assert r["c"] == m.cost(x, u) and r["f"] == m.final_cost(x)
        d = O.batch_derivatives(m, np.stack([x, x])[None], u[None, None], dt)
        for is_final in (0, 1):
            for kname in FD_NAMES:
                if is_final and kname in ("fx", "fu"):
                    continue
                assert np.array_equal(d[kname][0, is_final], r["fd%d_%s" % (is_final, kname)]), (kname, is_final)
