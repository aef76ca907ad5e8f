"""STEP 3/4 of the outer loop (src/ilqr_core.cpp:184-282) -- which line-search candidate is accepted, how lambda and dlambda move, which
exit ends a trajectory, the iteration count -- and STEP 2's retry loop (:136-159), under tunables (ilqr_params) other than the reference's.

Part 1, the decision table: ilqr_accept_candidates on host-evaluated handles against `ref_accept`, a plain statement of STEP 3/4 in
double with one rounding per operation (no fused multiply-add), bit for bit.  Rows are built on purpose for every branch: which alpha
wins, the sgn branch (expected <= 0), z exactly at z_min and one double above, rows where a contracted `dV0 + alpha dV1` decides the
other way, non-finite costs, the cost exit at tol_fun, lambda at its floor and its ceiling, max_iter, finished trajectories, fixed work,
and an abandoned backward pass.
Part 2, STEP 2 against the oracle: a pass that diverges until lambda is large enough, per trajectory, on the host path's backward
kernels; the schedule the oracle's passes imply, lambda and dlambda bit for bit, and the abandoned pass past lambda_max."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests.util import mat

pytestmark = pytest.mark.gpu
DT = 0.02
ALPHAS = (1.0000, 0.5012, 0.2512, 0.1259, 0.0631, 0.0316, 0.0158, 0.0079, 0.0040, 0.0020, 0.0010)  # include/ilqr.h:24
INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------------------------------------------------------------------------
# the plain reference of STEP 3/4
# ------------------------------------------------------------------------------------------------------------------------------------
def expected_of(alpha, dV0, dV1):
    """:200, rounded after every operation (Python floats: IEEE double, no contraction)"""
    return -alpha * (dV0 + alpha * dV1)


def expected_fused(alpha, dV0, dV1):
    """the same with dV0 + alpha * dV1 rounded once, as a fused multiply-add gives it (exact sum by Fraction, one rounding)"""
    return -alpha * float(Fraction(dV0) + Fraction(alpha) * Fraction(dV1))


def sgn(x):
    return float(int(0.0 < x) - int(x < 0.0))


def z_of(dcost, e):
    return dcost / e if e > 0 else sgn(dcost)


def ref_accept(p, s, cost_c, fixed_work=False):
    """One STEP 3/4 for one trajectory.  s: dict(status, iters, alpha, lam, dlam, cost, dV0, dV1, done) -> (new state, accepted index).
    A finished trajectory is left as it is (accepted -1)."""
    if s["status"] != 0:
        return dict(s), -1
    s = dict(s)
    lam, dlam, cost_s = s["lam"], s["dlam"], s["cost"]
    fwd, acc, new_cost, dcost = False, -1, 0.0, 0.0
    if s["done"]:
        for a, alpha in enumerate(ALPHAS):  # first z > z_min in alpha order
            new_cost = cost_c[a]
            dcost = cost_s - new_cost
            if z_of(dcost, expected_of(alpha, s["dV0"], s["dV1"])) > p["z_min"]:
                fwd, acc = True, a
                break
    status, f = 0, p["lambda_factor"]
    if fwd:
        dlam = min(dlam / f, 1 / f)
        lam = lam * dlam * (1.0 if lam > p["lambda_min"] else 0.0)
        s["cost"] = new_cost
        if not fixed_work and dcost < p["tol_fun"]:
            status = 2
    else:
        dlam = max(dlam * f, f)
        lam = max(lam * dlam, p["lambda_min"])
        if not fixed_work and lam > p["lambda_max"]:
            status = 3
    s["iters"] += 1
    if status == 0 and not fixed_work and s["iters"] >= p["max_iter"]:
        status = 4
    s.update(status=status, lam=lam, dlam=dlam, alpha=acc)
    return s, acc


def passing(p, s, cost_c):
    return [z_of(s["cost"] - c, expected_of(al, s["dV0"], s["dV1"])) > p["z_min"] for al, c in zip(ALPHAS, cost_c)]


def stretch(x, k):
    """x moved k doubles up (k > 0) or down"""
    for _ in range(abs(k)):
        x = math.nextafter(x, INF if k > 0 else -INF)
    return x


def same_bits(a, b):
    """float arrays equal bit for bit (any NaN equals any NaN)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))


# ------------------------------------------------------------------------------------------------------------------------------------
# host-evaluated handles
# ------------------------------------------------------------------------------------------------------------------------------------
BASE = dict(max_iter=100, tol_fun=1e-4, tol_grad=1e-6, lambda_init=1.0, dlambda_init=1.0, lambda_factor=2.5, lambda_max=1e4,
            lambda_min=1e-3, z_min=0.0)


def host_setup(oracle, n, m, B, T, params, flags=0, lim=1.0, seed=3):
    """a host handle and the records of an LQ twin's rollout (memory layout, as oracle.batch_derivatives gives them)"""
    from ilqr_amd import BatchILQR
    from tests.test_gpu_lq_end_to_end import dense_mats
    om = oracle.Model("lq", lq=dense_mats(n, m), u_lim=lim)
    g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=-lim, u_max=lim, params=params, flags=flags)
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-1, 1, (B, n))
    u0 = rng.normal(size=(B, T, m)) * 0.2 * lim
    xs, us, cost = oracle.batch_rollout(om, x0, u0, DT)
    do = oracle.batch_derivatives(om, xs, us, DT)
    return om, g, dict(x0=x0, xs=xs, us=us, cost=cost, do=do)


def stage(g, d, cost_s, lam, dlam, us=None):
    """set_trajectory, reset_state(0), set_derivatives, set_gains (k = 0, K = 0), set_lambda, backward_step"""
    B, T = g.B, g.T
    g.set_trajectory(x0=d["x0"], xs=d["xs"], us=d["us"] if us is None else us, cost=cost_s)
    g.reset_state(False)
    g.set_derivatives(**{k: (v if k in ("cx", "cu") else mat(v)) for k, v in d["do"].items()})
    g.set_gains(k=np.zeros((B, T, g.nu)), K=np.zeros((B, T, g.nu, g.nx)))
    g.set_lambda(lam, dlam)
    g.backward_step()


def read_state(g, p):
    st, it, al = g.status()
    lam, dlam = g.lambdas()
    cost, dV = g.cost(), g.dV()
    # the retry loop leaves only by a completed pass or by lambda > lambda_max (the abandoned pass: no search)
    return [dict(status=int(st[b]), iters=int(it[b]), alpha=int(al[b]), lam=float(lam[b]), dlam=float(dlam[b]), cost=float(cost[b]),
                 dV0=float(dV[b, 0]), dV1=float(dV[b, 1]), done=not (lam[b] > p["lambda_max"])) for b in range(g.B)]


def accept_and_compare(g, p, states, cost_c, fixed_work=False, what=""):
    """one ilqr_accept_candidates against ref_accept; returns the reference's new states"""
    acc = g.accept_candidates(cost_c)
    new, ref_acc = zip(*[ref_accept(p, s, [float(v) for v in c], fixed_work) for s, c in zip(states, cost_c)])
    st, it, al = g.status()
    lam, dlam = g.lambdas()
    cost = g.cost()
    r = {k: np.array([s[k] for s in new]) for k in ("status", "iters", "alpha", "lam", "dlam", "cost")}
    bad = [b for b in range(g.B) if not (acc[b] == ref_acc[b] and st[b] == r["status"][b] and it[b] == r["iters"][b] and al[b] == r["alpha"][b]
                                          and same_bits(lam[b], r["lam"][b]) and same_bits(dlam[b], r["dlam"][b]) and same_bits(cost[b], r["cost"][b]))]
    report = ["b=%d device (acc %d st %d it %d lam %r dlam %r cost %r) reference (acc %d st %d it %d lam %r dlam %r cost %r) dV %r cost_s %r"
              % (b, acc[b], st[b], it[b], lam[b], dlam[b], cost[b], ref_acc[b], r["status"][b], r["iters"][b], r["lam"][b], r["dlam"][b],
                 r["cost"][b], (states[b]["dV0"], states[b]["dV1"]), states[b]["cost"]) for b in bad]
    assert not bad, "%s: %d rows differ from the plain STEP 3/4\n%s" % (what, len(bad), "\n".join(report[:12]))
    assert np.array_equal(acc, np.array(ref_acc)) and np.array_equal(st, r["status"]) and np.array_equal(it, r["iters"])
    assert np.array_equal(al, r["alpha"]) and same_bits(lam, r["lam"]) and same_bits(dlam, r["dlam"]) and same_bits(cost, r["cost"])
    assert g.count_running() == int(np.sum(st == 0))
    return list(new)


def lambda_landing_on(target, f, above):
    """lambda (dlambda = 1, a failed search: dlambda' = f) whose lambda * f rounds to target exactly, or to a double above it"""
    lam = target / f
    for k in range(-64, 65):
        x = stretch(lam, k)
        y = x * f
        if (y == target) if not above else (y > target and y <= stretch(target, 4)):
            return x
    raise AssertionError("no lambda lands on %r" % target)


# ------------------------------------------------------------------------------------------------------------------------------------
# Part 1: the decision table
# ------------------------------------------------------------------------------------------------------------------------------------
TALLY_KEYS = ("accept", "reject_all", "first_of_several", "only_alpha10", "sgn_e0_pos", "sgn_e0_zero", "sgn_e0_neg", "sgn_eneg_pos",
              "sgn_eneg_zero", "sgn_eneg_neg", "z_eq_zmin", "z_next_above", "contraction", "nan", "pinf", "minf", "nan_accepted",
              "tolfun_equal", "tolfun_below", "floor_to_zero", "floor_above", "zero_to_floor", "ceiling_exact", "ceiling_above",
              "status1", "status2", "status3", "status4", "abandoned", "finished_skipped", "fixed_work")


def _tally():
    return {k: 0 for k in TALLY_KEYS}


@pytest.fixture(scope="module")
def tally():
    """rows per branch over the whole module, reported at its end (each test asserts the branches of its own rows)"""
    t = _tally()
    yield t
    print("\naccept decision table, rows per branch:", t)


@pytest.mark.parametrize("zmin", [0.0, 0.3, -0.5])
@pytest.mark.parametrize("n,m", [(3, 2), (6, 3), (20, 17)])
def test_accept_decision_table(oracle, tally, n, m, zmin):
    B, T = 64, 20
    p = dict(BASE, z_min=zmin)
    om, g, d = host_setup(oracle, n, m, B, T, p)
    lmin, lmax, f, tol = p["lambda_min"], p["lambda_max"], p["lambda_factor"], p["tol_fun"]
    # rows fixed before the pass: zero first-order records (k = 0, dV = 0: expected == 0), a box that excludes 0 with the gradient
    # pointing out of it (expected < 0), and the lambdas of the floor / ceiling rows
    E0 = list(range(0, 9))          # expected == 0: dcost +, 0, - ; cost exit at tol_fun; NaN; gradient-norm exit
    ENEG = list(range(9, 12))       # expected < 0: dcost +, 0, -
    LAM = list(range(12, 17))       # lambda at lambda_min, one double above; 0; landing on lambda_max, above it
    us = d["us"].copy()
    do = {k: v.copy() for k, v in d["do"].items()}
    for b in E0:
        do["cx"][b] = 0.0
        do["cu"][b] = 0.0
    for b in ENEG:
        us[b] = -2.0   # below u_min = -1: every du >= 1
        do["cu"][b] += 5.0
    for b in range(17, 25):  # larger first-order records: an expected of 1 or more, which z = 5e-324 (the double above z_min = 0) needs
        do["cx"][b] *= 30.0
        do["cu"][b] *= 30.0
    d = dict(d, us=us, do=do)
    lam0 = np.ones(B)
    dlam0 = np.ones(B)
    lam0[8] = 1e-6  # E0 row 8: gnorm = 0 and lambda < 1e-5: status 1 in backward_step
    lam0[12], lam0[13], lam0[14] = lmin, stretch(lmin, 1), 0.0
    lam0[15], lam0[16] = lambda_landing_on(lmax, f, False), lambda_landing_on(lmax, f, True)
    cost_s = d["cost"].copy()
    cost_s[3:5] = 0.0  # (the cost-exit rows: dcost = 0 - new_cost exactly)
    stage(g, d, cost_s, lam0, dlam0, us=us)
    states = read_state(g, p)
    assert states[8]["status"] == 1 and all(s["status"] == 0 for b, s in enumerate(states) if b != 8)
    assert all(s["done"] for s in states)
    E = [[expected_of(al, s["dV0"], s["dV1"]) for al in ALPHAS] for s in states]
    for b in E0:
        assert states[b]["dV0"] == 0.0 and states[b]["dV1"] == 0.0
    assert all(all(e < 0 for e in E[b]) for b in ENEG), [E[b] for b in ENEG]
    rows = {}
    cost_c = np.zeros((B, 11))

    def reject_cost(b, a):  # a cost no z_min here accepts: dcost = -(|expected| + 1)
        return states[b]["cost"] + abs(E[b][a]) + 1.0

    def pass_cost(b, a):    # z = 1 (expected > 0) or sgn = +1
        return states[b]["cost"] - (E[b][a] if E[b][a] > 0 else 1.0)

    def row(b, kind, costs):
        rows[b] = kind
        cost_c[b] = costs

    for b, dc in zip(E0[:3] + ENEG, (1.0, 0.0, -1.0) * 2):
        row(b, ("sgn_e0_" if b in E0 else "sgn_eneg_") + {1.0: "pos", 0.0: "zero", -1.0: "neg"}[dc], [states[b]["cost"] - dc] * 11)
    c = states[3]["cost"]
    row(3, "tolfun_equal", [c - tol] * 11)
    row(4, "tolfun_below", [c - math.nextafter(tol, 0.0)] * 11)
    assert c - (c - tol) == tol and c - (c - math.nextafter(tol, 0.0)) == math.nextafter(tol, 0.0)
    row(5, "nan", [NAN] + [pass_cost(5, a) for a in range(1, 11)])   # expected == 0: sgn(NaN) = 0 -- accepted when z_min < 0
    row(6, "pinf", [INF] + [pass_cost(6, a) for a in range(1, 11)])
    row(7, "minf", [-INF] + [pass_cost(7, a) for a in range(1, 11)])
    row(8, "finished_skipped", [states[8]["cost"] - 1.0] * 11)
    for b in (12, 13):
        row(b, "floor_to_zero" if b == 12 else "floor_above", [pass_cost(b, a) for a in range(11)])
    for b in (14, 15, 16):
        row(b, {14: "zero_to_floor", 15: "ceiling_exact", 16: "ceiling_above"}[b], [reject_cost(b, a) for a in range(11)])
    # the rest: natural records, rows chosen from the pass's own dV
    free = [b for b in range(17, B) if all(e > 0 for e in E[b])]
    assert len(free) >= 40, "expected > 0 at every alpha on most natural rows"
    take = iter(free)
    b = next(take)
    row(b, "first_of_several", [pass_cost(b, a) for a in range(11)])
    b = next(take)
    row(b, "only_alpha10", [reject_cost(b, a) for a in range(10)] + [pass_cost(b, 10)])
    b = next(take)
    row(b, "reject_all", [reject_cost(b, a) for a in range(11)])
    for a_mid, val in ((5, NAN), (5, INF), (5, -INF)):
        b = next(take)
        row(b, {INF: "pinf", -INF: "minf"}.get(val, "nan"), [reject_cost(b, a) for a in range(a_mid)] + [val] + [pass_cost(b, a) for a in range(a_mid + 1, 11)])
    # z exactly z_min (rejected: the test is strict) and the next double above it (accepted), cost_s = 0 so that dcost = -new_cost exactly
    n_eq = n_above = n_contr = 0
    rest = list(take)
    for b in rest:
        if n_eq >= 3 and n_above >= 3:
            break
        want = "z_eq_zmin" if n_eq <= n_above else "z_next_above"
        # (z_min = 0: dcost / expected = 5e-324 needs expected >= 2/3 -- dcost is a whole number of 5e-324 -- so the largest expected)
        a = (b * 7) % 11 if zmin != 0 else int(np.argmax(E[b]))
        e = E[b][a]
        if want == "z_eq_zmin" and zmin == 0:
            hit = 0.0  # (z = 0 exactly: dcost = 0)
        else:
            t0 = zmin * e if zmin != 0 else e * 5e-324
            target = zmin if want == "z_eq_zmin" else math.nextafter(zmin, INF)
            hit = next((x for x in (stretch(t0, k) for k in range(-40, 41)) if x / e == target), None)
        if hit is not None:
            states[b]["cost"] = 0.0
            row(b, want, [INF] * a + [-hit] + [INF] * (10 - a))
            n_eq, n_above = n_eq + (want == "z_eq_zmin"), n_above + (want == "z_next_above")
    # the contraction rows: the twice-rounded expected and the fused one on opposite sides of z_min (cost_s = 0 again)
    for b in rest:
        if b in rows or n_contr >= 12:
            continue
        for a in range(11):
            er, ef = E[b][a], expected_fused(ALPHAS[a], states[b]["dV0"], states[b]["dV1"])
            if zmin == 0 or er == ef or er <= 0 or ef <= 0:
                continue
            hit = None
            for k in range(-24, 25):
                dcost = stretch(zmin * er, k)
                if (dcost / er > zmin) != (dcost / ef > zmin):
                    hit = dcost
                    break
            if hit is not None:
                states[b]["cost"] = 0.0
                row(b, "contraction", [INF] * a + [-hit] + [pass_cost(b, a2) for a2 in range(a + 1, 11)])
                n_contr += 1
                break
    for b in range(B):
        if b not in rows:  # natural candidates: the acceptance the reference gives them
            row(b, "natural", [states[b]["cost"] - E[b][a] * (0.1 + 0.1 * ((a + b) % 13)) for a in range(11)])
    cost_s = np.array([s["cost"] for s in states])
    g.set_trajectory(cost=cost_s)  # (only the scalars of the contraction / threshold rows changed; records, gains, dV stay)
    states = [dict(s, cost=float(c)) for s, c in zip(states, cost_s)]
    new = accept_and_compare(g, p, states, cost_c, what="n=%d m=%d z_min=%g" % (n, m, zmin))
    # the branches this handle's rows reached (by the reference's own account): every one of them must have been reached here
    t = _tally()
    for b in range(B):
        s0, s1, kind = states[b], new[b], rows[b]
        if s0["status"] != 0:
            t["finished_skipped"] += kind == "finished_skipped"
            t["status1"] += 1
            continue
        acc = s1["alpha"] >= 0
        t["accept" if acc else "reject_all"] += 1
        if s1["status"] in (2, 3):
            t["status%d" % s1["status"]] += 1
        if kind in ("first_of_several",) and acc and s1["alpha"] == 0 and sum(passing(p, s0, cost_c[b])) >= 2:
            t[kind] += 1
        elif kind == "only_alpha10" and s1["alpha"] == 10:
            t[kind] += 1
        elif kind.startswith("sgn_") or kind in ("z_eq_zmin", "z_next_above", "contraction", "pinf", "minf"):
            t[kind] += 1
            assert kind != "z_eq_zmin" or not acc
            assert kind != "z_next_above" or acc
        elif kind == "nan":
            t["nan"] += 1
            t["nan_accepted"] += acc and math.isnan(s1["cost"])
        elif kind == "tolfun_equal" and acc and s1["status"] == 0:
            t[kind] += 1
        elif kind == "tolfun_below" and s1["status"] == 2:
            t[kind] += 1
        elif kind == "floor_to_zero" and acc and s1["lam"] == 0.0:
            t[kind] += 1
        elif kind == "floor_above" and acc and s1["lam"] > 0.0:
            t[kind] += 1
        elif kind == "zero_to_floor" and not acc and s1["lam"] == lmin:
            t[kind] += 1
        elif kind == "ceiling_exact" and s1["lam"] == lmax and s1["status"] == 0:
            t[kind] += 1
        elif kind == "ceiling_above" and s1["status"] == 3:
            t[kind] += 1
    for k, v in t.items():
        tally[k] += v
    need = [k for k in TALLY_KEYS if k not in ("contraction", "status4", "abandoned", "fixed_work") and (k != "nan_accepted" or zmin < 0)]
    missing = [k for k in need if t[k] == 0]
    print("n=%d m=%d z_min=%g rows per branch:" % (n, m, zmin), t)
    assert not missing, "branches no row reached: %s (%s)" % (missing, t)
    g.close()


def test_accept_repeated_calls_max_iter_and_finished(oracle, tally):
    """max_iter = 3: status 4 arrives with the third accept; status 2 takes priority over 4; finished trajectories stay as they are."""
    B, T = 16, 12
    p = dict(BASE, max_iter=3, z_min=0.3)
    om, g, d = host_setup(oracle, 3, 2, B, T, p, seed=8)
    do = {k: v.copy() for k, v in d["do"].items()}
    for b in range(B):
        if b % 4 in (1, 2):  # zero first-order records: expected == 0, every dcost > 0 is accepted (sgn = 1 > z_min)
            do["cx"][b] = 0.0
            do["cu"][b] = 0.0
    stage(g, dict(d, do=do), d["cost"].copy(), np.ones(B), np.ones(B))
    states = read_state(g, p)
    assert all(s["status"] == 0 and s["done"] for s in states)
    E = [[expected_of(al, s["dV0"], s["dV1"]) for al in ALPHAS] for s in states]
    assert all(all(e > 0 for e in E[b]) for b in range(0, B, 4))
    tol = p["tol_fun"]
    for call in range(3):
        cost_c = np.zeros((B, 11))
        for b in range(B):
            c = states[b]["cost"]
            kind = b % 4
            if kind == 0:    # big steps every call: running, running, max_iter
                cost_c[b] = [c - 10 * e for e in E[b]]
            elif kind == 1:  # steps of 1, 1, then one below tol_fun: on the third call status 2 wins over 4
                cost_c[b] = [c - (1.0 if call < 2 else 0.5 * tol)] * 11
            elif kind == 2:  # converges on the first call, then is left alone
                cost_c[b] = [c - (0.5 * tol if call == 0 else 1.0)] * 11
            else:            # no step ever: lambda climbs (1 -> 2.5 -> 15.6 -> 156)
                cost_c[b] = [c + abs(e) + 1 for e in E[b]]
        states = accept_and_compare(g, p, states, cost_c, what="call %d" % (call + 1))
        st = np.array([s["status"] for s in states])
        if call < 2:
            assert np.all(st[0::4] == 0) and np.all(st[1::4] == 0) and np.all(st[3::4] == 0)
    assert np.all(np.array([s["status"] for s in states])[1::4] == 2) and all(s["iters"] == 3 for s in states[1::4])
    st = np.array([s["status"] for s in states])
    it = np.array([s["iters"] for s in states])
    assert np.all(st[0::4] == 4) and np.all(it[0::4] == 3)
    tally["status4"] += int(np.sum(st == 4))
    assert np.all(st[2::4] == 2) and np.all(it[2::4] == 1)  # finished on call 1, skipped by calls 2 and 3
    tally["finished_skipped"] += len(st[2::4])
    tally["status2"] += int(np.sum(st == 2))
    g.close()


def test_accept_fixed_work(oracle, tally):
    """ILQR_FLAG_FIXED_WORK: no exit fires -- not tol_fun, not lambda_max, not max_iter -- and every call still counts an iteration."""
    from ilqr_amd import capi
    B, T = 12, 10
    p = dict(BASE, max_iter=2, z_min=-0.5, lambda_max=20.0)
    om, g, d = host_setup(oracle, 6, 3, B, T, p, flags=capi.FLAG_FIXED_WORK, seed=9)
    stage(g, d, d["cost"].copy(), np.full(B, 3.0), np.ones(B))
    states = read_state(g, p)
    for call in range(4):
        cost_c = np.array([[s["cost"] - 1e-9] * 11 if b % 2 == 0 else [s["cost"] + abs(s["dV0"]) + 1.0] * 11 for b, s in enumerate(states)])
        states = accept_and_compare(g, p, states, cost_c, fixed_work=True, what="fixed work, call %d" % (call + 1))
    assert all(s["status"] == 0 and s["iters"] == 4 for s in states)
    assert all(s["lam"] > p["lambda_max"] for s in states[1::2])  # past the ceiling, still running
    tally["fixed_work"] += B
    g.close()


def test_accept_after_an_abandoned_pass(oracle, tally):
    """ILQR_FLAG_REFERENCE_FIXES, cuu made indefinite at one knot and a small lambda_max: the retry loop gives up (backpass_done = 0) and the
    accept takes the no-step branch (status 3, no alpha, cost unchanged) although every candidate would pass."""
    from ilqr_amd import capi
    B, T = 16, 15
    p = dict(BASE, lambda_max=10.0, z_min=0.3)
    om, g, d = host_setup(oracle, 6, 3, B, T, p, flags=capi.FLAG_REFERENCE_FIXES, lim=50.0, seed=10)
    do = {k: v.copy() for k, v in d["do"].items()}
    for b in range(0, B, 2):
        do["cuu"][b, 5 + b % 7] -= 50.0 * np.eye(3)
    d = dict(d, do=do)
    stage(g, d, d["cost"].copy(), np.ones(B), np.ones(B))
    states = read_state(g, p)
    assert not any(s["done"] for s in states[0::2]) and all(s["done"] for s in states[1::2])
    cost_c = np.array([[s["cost"] - 1e3] * 11 for s in states])
    new = accept_and_compare(g, p, states, cost_c, what="abandoned pass")
    assert all(s["status"] == 3 and s["alpha"] == -1 and s["cost"] == s0["cost"] for s, s0 in zip(new[0::2], states[0::2]))
    assert all(s["alpha"] == 0 for s in new[1::2])
    tally["abandoned"] += B // 2
    tally["status3"] += B // 2
    g.close()


def contraction_hit(states, b, zmin):
    """(alpha index, dcost) where z computed from the twice-rounded expected and from the fused one fall on opposite sides of z_min"""
    s = states[b]
    for a in range(1, 11):  # (alpha = 1: the product is exact, both agree)
        er, ef = expected_of(ALPHAS[a], s["dV0"], s["dV1"]), expected_fused(ALPHAS[a], s["dV0"], s["dV1"])
        if er == ef or er <= 0 or ef <= 0:
            continue
        for k in range(-24, 25):
            dcost = stretch(zmin * er, k)
            if (dcost / er > zmin) != (dcost / ef > zmin):
                return a, dcost
    return None


@pytest.mark.parametrize("zmin", [0.3, -0.5])
@pytest.mark.parametrize("n,m", [(3, 2), (6, 3)])
def test_accept_contraction_rows(oracle, tally, n, m, zmin):
    """A rounding of dV0 + alpha dV1 that a contraction would skip is rare (a few per cent of (trajectory, alpha) pairs), so this test
    looks for such pairs in every trajectory of four passes (four lambdas: four sets of dV) and asserts it found a handful."""
    B, T = 64, 20
    p = dict(BASE, z_min=zmin)
    om, g, d = host_setup(oracle, n, m, B, T, p, seed=17)
    found = 0
    for lam in (1.0, 0.37, 2.9, 0.11):
        stage(g, d, d["cost"].copy(), np.full(B, lam), np.ones(B))
        states = read_state(g, p)
        cost_c = np.zeros((B, 11))
        hits = []
        for b in range(B):
            E = [expected_of(al, states[b]["dV0"], states[b]["dV1"]) for al in ALPHAS]
            h = contraction_hit(states, b, zmin)
            if h is None:
                cost_c[b] = [states[b]["cost"] - e * 0.5 for e in E]
                continue
            a, dcost = h
            states[b]["cost"] = 0.0  # (dcost = 0 - new_cost exactly)
            cost_c[b] = [INF] * a + [-dcost] + [-(e if e > 0 else 1.0) for e in E[a + 1:]]
            hits.append(b)
        g.set_trajectory(cost=np.array([s["cost"] for s in states]))
        accept_and_compare(g, p, states, cost_c, what="contraction rows, n=%d m=%d z_min=%g lambda=%g" % (n, m, zmin, lam))
        found += len(hits)
    print("contraction rows n=%d m=%d z_min=%g: %d" % (n, m, zmin, found))
    tally["contraction"] += found
    assert found >= 5, found
    g.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# Part 2: STEP 2's retry loop against the oracle, the abandoned pass included
# ------------------------------------------------------------------------------------------------------------------------------------
def oracle_step2(oracle, om, us, do, k0, lam0, dlam0, p):
    """The retry loop of :136-150 per trajectory, each pass the oracle's (batch_backward at that trajectory's lambda, warm-started from
    the gains the previous attempt left), and the gradient norm of :153 (ilqr_core.cpp:405-412) of the gains it leaves -- not its exit
    test (the callers keep lambda >= 1e-5 or gnorm >= tol_grad).  K is carried like k: an attempt that diverges at knot i has written
    the knots above i only, so after an abandoned pass the knots at and below its divergence knot hold what earlier attempts left
    (zeros where none reached, as the caller's set_gains).  In the flavour of `om` (the float twin for an fp32 handle)."""
    B = us.shape[0]
    lam, dlam = np.array(lam0, dtype=np.float64), np.array(dlam0, dtype=np.float64)
    k = np.array(k0, dtype=np.float64)
    out = dict(k=np.zeros_like(k), K=None, dV=np.zeros((B, 2)), div=np.zeros(B, dtype=np.int32), done=np.zeros(B, bool), tries=np.zeros(B, int))
    K = np.zeros((B,) + (us.shape[1], om.nx, om.nu))
    todo = np.ones(B, bool)
    while todo.any():
        sel = np.nonzero(todo)[0]
        with oracle.flavour(om.flavour):
            r = oracle.batch_backward(om, us[sel], {kk: v[sel] for kk, v in do.items()}, k_prev=k[sel], lam=lam[sel])
        r = {kk: (np.asarray(v, dtype=np.float64) if v.dtype.kind == "f" else v) for kk, v in r.items()}
        for i, b in enumerate(sel):
            dv = r["diverge"][i]
            k[b], out["dV"][b], out["div"][b] = r["k"][i], r["dV"][i], dv
            K[b, dv + 1 if dv else 0:] = r["K"][i, dv + 1 if dv else 0:]
            out["tries"][b] += 1
            if r["diverge"][i] == 0:
                out["done"][b], todo[b] = True, False
                continue
            dlam[b] = max(dlam[b] * p["lambda_factor"], p["lambda_factor"])
            lam[b] = max(lam[b] * dlam[b], p["lambda_min"])
            if lam[b] > p["lambda_max"]:
                todo[b] = False
    out.update(k=k, K=K, lam=lam, dlam=dlam)
    out["gnorm"] = np.mean(np.max(np.abs(k) / (np.abs(us) + 1), axis=2), axis=1)
    return out


STEP2_CASES = [  # (name, n, m, route, kernel of the stage, dtype)
    ("host", 6, 3, 0, "k_backward_w3", "f64"),
    ("host", 6, 3, "ROUTE_BACKWARD_W2", "k_backward_w2", "f64"),
    ("host", 6, 3, "ROUTE_TWO_CONTROL_TILES", "k_backward_w3w", "f64"),
    ("host", 24, 20, 0, "k_backward_w3w", "f64"),
    ("acrobot", 4, 1, 0, "k_backward_q", "f64"),
    ("acrobot", 4, 1, "thread", "k_backward_t", "f64"),
    ("integrator", 4, 2, 0, "k_backward_q", "f64"),
    ("integrator", 4, 2, "thread", "k_backward_t", "f64"),
    # fp32 (float records, Riccati step and box-QP; lambda, dV and the gradient norm in double) against the float twin
    ("acrobot", 4, 1, 0, "k_backward_q", "f32"),
    ("acrobot", 4, 1, "thread", "k_backward_t", "f32"),
    ("integrator", 4, 2, 0, "k_backward_q", "f32"),
    ("integrator", 4, 2, "thread", "k_backward_t", "f32"),
]


@pytest.fixture
def fixed_oracle(oracle):
    oracle.set_fixes(3)
    yield oracle
    oracle.set_fixes(0)


@pytest.mark.parametrize("lambda_factor", [1.6, 3.0])
@pytest.mark.parametrize("name,n,m,route,kernel,dtype", STEP2_CASES)
def test_step2_retry_schedule_matches_the_oracle(fixed_oracle, tally, name, n, m, route, kernel, dtype, lambda_factor):
    """ILQR_FLAG_REFERENCE_FIXES (a failed factorisation is a divergence), cuu shifted down by a different amount per trajectory at one
    knot: every trajectory diverges until its own lambda covers the shift; lambda_max low enough that the larger shifts run out of retries
    (the abandoned pass: partial dV, the gains of the last attempt above its divergence knot and the earlier ones below, no search)."""
    from ilqr_amd import BatchILQR, capi
    from tests.util import acrobot_x0, integrator_x0
    oracle = fixed_oracle
    B, T = 24, 30
    p = dict(BASE, lambda_factor=lambda_factor, lambda_max=60.0, lambda_min=1e-3, z_min=0.0)
    flags = capi.FLAG_REFERENCE_FIXES
    rng = np.random.default_rng(31)
    if name == "host":
        from tests.test_gpu_lq_end_to_end import dense_mats
        lim = 50.0
        om = oracle.Model("lq", lq=dense_mats(n, m), u_lim=lim)
        g = BatchILQR("host", B, T, DT, nx=n, nu=m, u_min=-lim, u_max=lim, params=p, flags=flags,
                      route=0 if route == 0 else getattr(capi, route))
        x0 = rng.uniform(-1, 1, (B, n))
    else:
        lim = 50.0
        goal = [1.0, 0.5, 0.0, 0.0]
        om = oracle.Model(name, u_lim=lim) if name == "acrobot" else oracle.Model(name, goal=goal, u_lim=lim)
        kw = dict(goal=goal) if name == "integrator" else {}
        g = BatchILQR(name, B, T, DT, u_min=-lim, u_max=lim, params=p, dtype=dtype, **kw,
                      flags=flags | capi.FLAG_UNFUSED | (capi.FLAG_BACKWARD_THREAD_PER_TRAJ if route == "thread" else 0))
        x0 = acrobot_x0(B, scale=0.5) if name == "acrobot" else integrator_x0(B)
    # (UNFUSED: an nx = 4 handle then names the stage call's own kernel, which backward_step runs either way)
    assert g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index("backward")) == kernel.encode()
    u0 = rng.normal(size=(B, T, m)) * 0.2
    xs, us, cost = oracle.batch_rollout(om, x0, u0, DT)
    do = oracle.batch_derivatives(om, xs, us, DT)
    # the shift: eigenvalues of Quu at that knot pushed below zero by 0 .. ~300, so that the lambda that covers it lies anywhere from
    # the first try to far past lambda_max = 60; trajectories 0, 1 keep their records (no retry)
    bad_t = rng.integers(2, T - 2, size=B)
    shift = np.concatenate([[0.0, 0.0], np.exp(rng.uniform(np.log(0.5), np.log(300.0), size=B - 2))])
    for b in range(B):
        do["cuu"][b, bad_t[b]] -= shift[b] * np.eye(m)
    k0 = rng.normal(size=(B, T, m)) * 0.05
    lam0 = np.where(np.arange(B) % 3 == 0, 0.0, 1.0)
    dlam0 = np.ones(B)
    # (an fp32 handle rounds the records, controls and warm start to float as it stores them; the float twin is given the same)
    ro = oracle_step2(oracle, om if dtype == "f64" else om.twin("f32"), us, do, k0, lam0, dlam0, p)
    g.set_trajectory(x0=x0, xs=xs, us=us, cost=cost)
    g.reset_state(False)
    g.set_derivatives(**{k: (v if k in ("cx", "cu") else mat(v)) for k, v in do.items()})
    g.set_gains(k=k0, K=np.zeros((B, T, m, n)))
    g.set_lambda(lam0, dlam0)
    g.backward_step()
    lam, dlam = g.lambdas()
    print("%s %s %s f=%g: tries %s, abandoned %d" % (name, kernel, dtype, lambda_factor, ro["tries"].tolist(), int(np.sum(~ro["done"]))))
    assert same_bits(lam, ro["lam"]) and same_bits(dlam, ro["dlam"]), (lam, ro["lam"], dlam, ro["dlam"])
    assert np.sum(ro["tries"] > 1) >= 4 and np.sum(~ro["done"]) >= 2 and np.sum(ro["done"] & (ro["tries"] > 1)) >= 2, ro["tries"]
    k, K = g.gains()
    dV, gn = g.dV(), g.gnorm()
    tol = 1e-7 if dtype == "f64" else 1e-5
    for b in range(B):
        sk = max(np.abs(ro["k"][b]).max(), 1e-12)
        assert np.abs(k[b] - ro["k"][b]).max() <= tol * sk, (b, ro["done"][b], np.abs(k[b] - ro["k"][b]).max(), sk)
        # K over the whole horizon: after an abandoned pass, the last attempt's gains above its divergence knot and the earlier
        # attempts' (or set_gains' zeros) at and below it
        Ko = mat(ro["K"][b])
        assert np.abs(K[b] - Ko).max() <= tol * max(np.abs(Ko).max(), 1e-12), (b, ro["done"][b], ro["div"][b])
        assert abs(dV[b, 0] - ro["dV"][b, 0]) <= tol * max(abs(ro["dV"][b, 0]), 1e-12) + 1e-300, (b, dV[b], ro["dV"][b])
        assert abs(dV[b, 1] - ro["dV"][b, 1]) <= tol * max(abs(ro["dV"][b, 1]), 1e-12) + 1e-300, (b, dV[b], ro["dV"][b])
        assert abs(gn[b] - ro["gnorm"][b]) <= tol * max(ro["gnorm"][b], 1e-12), (b, gn[b], ro["gnorm"][b])
    st, it, _ = g.status()
    assert np.all(st == 0)
    # STEP 3/4 after it: the abandoned passes take the no-step branch (status 3) although every candidate would pass
    if name == "host":
        states = read_state(g, p)
        assert [s["done"] for s in states] == ro["done"].tolist()
        new = accept_and_compare(g, p, states, np.array([[s["cost"] - 1e3] * 11 for s in states]), what="after STEP 2")
        assert all((s["status"] == 3 and s["alpha"] == -1) == (not dn) for s, dn in zip(new, ro["done"]))
    tally["abandoned"] += int(np.sum(~ro["done"]))
    g.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# Part 3: whole iterations on the routes under three parameter sets
# ------------------------------------------------------------------------------------------------------------------------------------
# P1 a fast schedule; P2 a strict search under a low ceiling (LAMBDA_MAX exits); P3 a negative z_min under fixed work (steps that raise
# the cost are accepted, no exit fires)
PSETS = {
    "P1": (dict(lambda_init=10.0, dlambda_init=2.0, lambda_factor=3.0, lambda_min=1e-3, z_min=0.3, tol_fun=1e-3, max_iter=9), False),
    "P2": (dict(z_min=0.9, lambda_factor=2.5, lambda_max=50.0, max_iter=10), False),
    "P3": (dict(z_min=-0.5, max_iter=8), True),
}


@pytest.fixture
def params_oracle(oracle):
    """the oracle under a parameter set (tunables of the handle's ilqr_params that the oracle has: set_params), defaults restored after"""
    def use(prm):
        oracle.set_params(**{k: v for k, v in prm.items() if k in oracle.PARAM_NAMES})
        return oracle
    try:
        yield use
    finally:
        oracle.set_params()
        oracle.set_fixes(0)


def _nx4(model, B, T):
    from tests.util import acrobot_x0, integrator_x0
    if model == "acrobot":
        return 1.5, acrobot_x0(B, scale=0.5, seed=41), {}
    return 0.5, integrator_x0(B, seed=43), dict(goal=[1.0, 0.5, 0.0, 0.0])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model", ["acrobot", "integrator"])
@pytest.mark.parametrize("pset", list(PSETS))
def test_nx4_routes_under_non_default_params_equal_the_two_kernel_route(model, dtype, pset):
    """Every nx = 4 route (k_solve_hex, k_solve_tile<1/2>, k_solve_wide / wide2, staged) and the opt-in fixes' routes under P1, P2, P3:
    three stepwise iterations, then the rest of the solve; every array, status, iteration count and lambda bit-identical to
    ILQR_FLAG_UNFUSED (its stage kernels k_backward_q and k_accept)."""
    from ilqr_amd import BatchILQR, capi
    from tests.test_gpu_control_limits import _same, _state, nx4_routes
    prm, fixed = PSETS[pset]
    B, T = 37, 61
    lim, x0, kw = _nx4(model, B, T)
    u0 = np.zeros((B, T, 1 if model == "acrobot" else 2))
    sv = capi.STAGE_NAMES.index("solve")
    reached = set()
    for fixes in (False, True):
        base = (capi.FLAG_REFERENCE_FIXES if fixes else 0) | (capi.FLAG_FIXED_WORK if fixed else 0)
        routes = nx4_routes(model) if not fixes else [("unfused", capi.FLAG_UNFUSED, 0, None), ("default", 0, 0, b"k_solve_tile"),
                                                      ("staged", capi.FLAG_STAGED, 0, b"")]
        out = []
        for name, fl, route, kernel in routes:
            g = BatchILQR(model, B, T, DT, u_min=-lim, u_max=lim, flags=base | fl, route=route, dtype=dtype, params=prm, **kw)
            if kernel is not None:
                assert g.lib.ilqr_stage_kernel_name(g.h, sv) == kernel, (name, g.lib.ilqr_stage_kernel_name(g.h, sv))
            g.init_traj(x0, u0)
            lam0, dlam0 = g.lambdas()
            assert np.all(lam0 == prm.get("lambda_init", 1.0)) and np.all(dlam0 == prm.get("dlambda_init", 1.0))
            s = {}
            for i in range(3):
                g.iterate(1)
                s.update({"%d_%s" % (i, n): a for n, a in _state(g).items()})
            g.generate_trajectory()
            s.update({"end_" + n: a for n, a in _state(g).items()})
            out.append((name, s))
            g.close()
        for name, s in out[1:]:
            _same(out[0][1], s, (pset, name, "fixes" if fixes else ""))
        reached |= set(out[0][1]["end_st"].tolist())
        if fixed:  # (no exit; generate_trajectory adds max_iter iterations to the three stepwise ones)
            assert np.all(out[0][1]["end_st"] == 0) and np.all(out[0][1]["end_it"] == 3 + prm["max_iter"])
    print(pset, model, dtype, "end statuses", sorted(reached))
    if pset == "P2" and model == "acrobot":
        assert 3 in reached, reached  # the low ceiling is reached on the routes (the integrator's steps pass even z_min = 0.9)
    if pset == "P1":
        assert reached - {0, 4}, reached  # an exit before max_iter


@pytest.mark.parametrize("drive", ["oracle", "gpu"])
@pytest.mark.parametrize("model", ["acrobot", "integrator"])
@pytest.mark.parametrize("pset", list(PSETS))
def test_nx4_walk_under_non_default_params(params_oracle, model, pset, drive):
    """the persistent route under P1, P2, P3 walked iteration by iteration against the oracle with the same tunables"""
    from ilqr_amd import BatchILQR
    from tests.parity import walk_iterations
    prm, fixed = PSETS[pset]
    oracle = params_oracle(prm)
    B, T = 24, 60
    lim, x0, kw = _nx4(model, B, T)
    from ilqr_amd import capi
    om = oracle.Model(model, u_lim=lim, **kw)
    g = BatchILQR(model, B, T, DT, u_min=-lim, u_max=lim, params=prm, flags=capi.FLAG_FIXED_WORK if fixed else 0, **kw)
    r = walk_iterations(oracle, om, g, x0, np.zeros((B, T, om.nu)), DT, prm["max_iter"], fixed_work=fixed, params=prm, drive=drive)
    g.close()
    print("walk", pset, model, drive, {k: v for k, v in r.items() if k not in ("tied", "per_iter")})
    assert r["checked"] >= 2 * B and len(r["tied"]) <= max(2, r["checked"] // 10), r


GENERIC_ROUTES = [("default", 6, 3, 0, "f64"), ("ROUTE_LQ_THREAD_ROLLOUT", 6, 3, 0, "f64"), ("ROUTE_LQ_RECOMMIT", 6, 3, 0, "f64"),
                  ("ROUTE_BACKWARD_W2", 6, 3, 0, "f64"), ("ROUTE_TWO_CONTROL_TILES", 6, 3, 0, "f64"), ("default", 24, 20, 0, "f64"),
                  ("default", 6, 3, 0, "f32")]


@pytest.mark.parametrize("pset", ["P1", "P2"])
@pytest.mark.parametrize("route,n,m,flags,dtype", GENERIC_ROUTES)
def test_generic_routes_walk_under_non_default_params(params_oracle, route, n, m, flags, dtype, pset):
    """the LQ twin on the generic path's routes (k_rollout_lq accepting on the default route, k_accept after the thread-per-rollout
    search or the re-committed one; k_backward_w3, w2, w3w; more than 16 controls; fp32) walked against the oracle under P1 and P2"""
    from ilqr_amd import BatchILQR, capi
    from tests.parity import walk_iterations
    from tests.test_gpu_lq_end_to_end import dense_mats
    prm, _ = PSETS[pset]
    oracle = params_oracle(prm)
    B, T, lim = 24, 30, 0.3
    mats = dense_mats(n, m)
    om = oracle.Model("lq", lq=mats, u_lim=lim)
    g = BatchILQR("lq", B, T, DT, u_min=-lim, u_max=lim, lq=mats, params=prm, flags=flags, dtype=dtype,
                  route=0 if route == "default" else getattr(capi, route))
    x0 = np.random.default_rng(51).uniform(-1, 1, (B, n))
    r = walk_iterations(oracle, om, g, x0, np.zeros((B, T, m)), DT, prm["max_iter"], params=prm, precision=dtype)
    g.close()
    print("generic walk", pset, route, n, m, dtype, {k: v for k, v in r.items() if k not in ("tied", "per_iter")})
    assert r["checked"] >= 2 * B
    if dtype == "f64":
        assert len(r["tied"]) <= max(2, r["checked"] // 10), r
    else:  # (the caps of tests/test_gpu_generic_fp32.py: float gains meet clamp knife edges more often)
        assert r["ties_backward"] + r["ties_search"] + r["ties_stop"] + r["conditioned_branch"] <= max(4, r["checked"] // 3), r
        assert r["cond_over10"] <= max(2, r["checked"] // 20) and r["unresolved"] <= r["checked"] // 8, r


@pytest.mark.parametrize("pset", ["P1", "P2"])
def test_retries_inside_whole_iterations(params_oracle, pset):
    """An LQ twin whose R has one negative eigenvalue, with the fixes: lambda moves through retries on its own inside whole iterations;
    walked on k_backward_w3, w2 and w3w with a lambda_max that some trajectories reach"""
    from ilqr_amd import BatchILQR, capi
    from tests.parity import walk_iterations
    from tests.test_gpu_lq_end_to_end import dense_mats
    prm, _ = PSETS[pset]
    prm = dict(prm, lambda_max=30.0)
    oracle = params_oracle(prm)
    oracle.set_fixes(3)
    n, m, B, T, lim = 6, 3, 24, 30, 5.0
    A, Bm, Q, R, Qf = dense_mats(n, m)
    w, V = np.linalg.eigh(R)
    R = V @ np.diag(np.concatenate([[-0.05], w[1:]])) @ V.T
    mats = (A, Bm, Q, R, Qf)
    om = oracle.Model("lq", lq=mats, u_lim=lim)
    x0 = np.random.default_rng(53).uniform(-1, 1, (B, n))
    for route in (0, capi.ROUTE_BACKWARD_W2, capi.ROUTE_TWO_CONTROL_TILES):
        g = BatchILQR("lq", B, T, DT, u_min=-lim, u_max=lim, lq=mats, params=prm, flags=capi.FLAG_REFERENCE_FIXES, route=route)
        g.init_traj(x0, np.zeros((B, T, m)))
        g.compute_derivatives()
        g.set_lambda(0.0, 1.0)
        assert np.any(g.backward_pass() > 0)  # (Quu indefinite: whenever lambda falls low enough, STEP 2 has to retry)
        r = walk_iterations(oracle, om, g, x0, np.zeros((B, T, m)), DT, prm["max_iter"], params=prm)
        g.init_traj(x0, np.zeros((B, T, m)))
        g.generate_trajectory()
        st, _, _ = g.status()
        lam, _ = g.lambdas()
        g.close()
        print("retries", pset, route, "statuses", np.bincount(st, minlength=5), "lambda", lam.min(), lam.max(),
              {k: v for k, v in r.items() if k not in ("tied", "per_iter")})
        assert r["checked"] >= 2 * B and len(r["tied"]) <= max(2, r["checked"] // 10), r
