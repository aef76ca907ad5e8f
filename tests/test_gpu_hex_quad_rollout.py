"""k_solve_hex rolls out one QUAD per SIMD: the chain wavefront of pair s carries the four trajectories of its sub-tile under all eleven
alphas (lane = 4 alpha + q, csrc/quad_lanes.hpp) and fetches the quad's forty nominal rows of a step itself; the accepted candidates
are committed in descending chunk order, two tasks' loads at a time.  Every rollout is the expression sequence it always was, so the
kernel must leave, TO THE BIT, what the quad-chain route (ILQR_ROUTE_QUAD_CHAIN: k_solve_tile, sixteen trajectories x four alphas per
wavefront) and the staged route (ILQR_FLAG_UNFUSED: one kernel per stage) leave: trajectory, gains, cost, lambda, status, accepted alpha
and every candidate of every alpha -- compared as raw bit patterns.

Shapes, the smallest that reach each edge: T = 1 and 7 are shorter than the prefetch depth (8), 7 and 9 no multiple of the control group
(4) or the checkpoint spacing (8), 1..9 a single producer round, 33 shorter than the ring's lead, 67 several rounds; B = 1 a lone
trajectory, 3 a ragged quad, 17 a tile with three empty pairs, 37 a ragged last tile.  iterate(3) then iterate(2) crosses a launch
boundary with accepts pending.  After every launch the nominal trajectory must be the accepted candidates, re-read through the getter:
the commit is complete when the kernel ends, on every path."""
import numpy as np
import pytest

from tests.util import acrobot_x0

pytestmark = pytest.mark.gpu
DT = 0.02
LIM = 1.5
NALPHA = 11
DRIVES = {"1": (1,), "3+2": (3, 2), "4": (4,)}
ACCEPTED = {}  # case -> accepted line searches found at its launch ends, over the three routes (checked by the last test)


def bits(a, dtype):
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    return a.view(np.uint64) if dtype == "f64" else a.astype(np.float32).view(np.uint32)


def state(g, candidates=True):
    xs, us = g.trajectory()
    k, K = g.gains()
    st, it, al = g.status()
    lam, dlam = g.lambdas()
    s = dict(xs=xs, us=us, k=k, K=K, cost=g.cost(), lam=lam, dlam=dlam, st=st, it=it, al=al)
    if candidates:
        for a in range(NALPHA):
            s["cand%d_xs" % a], s["cand%d_us" % a] = g.candidate(a)
    return s


def assert_same_bits(a, b, dtype, what):
    assert a.keys() == b.keys()
    for n in a:
        dt = "f64" if n in ("lam", "dlam") else dtype  # lambda and dlambda are doubles in a float handle too
        x, y = bits(a[n], dt), bits(b[n], dt)
        if not np.array_equal(x, y):
            bad = np.argwhere(x != y)
            raise AssertionError("%s: %s differs in %d of %d entries, first at %s: %r / %r"
                                 % (what, n, len(bad), x.size, bad[0], a[n][tuple(bad[0])], b[n][tuple(bad[0])]))


def assert_committed(s, dtype, what):
    """the nominal trajectory of every trajectory that accepted a candidate IS that candidate"""
    al = s["al"]
    for a in np.unique(al[al >= 0]):
        sel = al == a
        for n in ("xs", "us"):
            assert np.array_equal(bits(s[n][sel], dtype), bits(s["cand%d_%s" % (a, n)][sel], dtype)), (what, "alpha %d" % a, n)


def routes():
    from ilqr_amd import capi
    return (("hex", 0, 0, b"k_solve_hex"), ("quad_chain", 0, capi.ROUTE_QUAD_CHAIN, b"k_solve_tile"), ("staged", capi.FLAG_UNFUSED, 0, None))


def make(B, T, dtype, flags, route, kernel, max_iter=40):
    from ilqr_amd import BatchILQR, capi
    g = BatchILQR("acrobot", B, T, DT, u_min=-LIM, u_max=LIM, flags=flags, route=route, dtype=dtype, params=dict(max_iter=max_iter))
    if kernel is not None:
        assert g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index("solve")) == kernel
    return g


def start(B, T, dtype):
    x0 = acrobot_x0(B, scale=0.6, seed=300 + T)
    if dtype == "f32":
        x0 = x0.astype(np.float32).astype(np.float64)
    return x0, np.zeros((B, T, 1))


@pytest.mark.parametrize("drive", list(DRIVES))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 3, 17, 37])
@pytest.mark.parametrize("T", [1, 7, 9, 33, 67])
def test_quad_rollouts_leave_the_bits_of_the_other_routes(T, B, dtype, drive):
    x0, u0 = start(B, T, dtype)
    out = {}
    accepted = 0
    for name, flags, route, kernel in routes():
        g = make(B, T, dtype, flags, route, kernel)
        g.init_traj(x0, u0)
        launches = []
        for n in DRIVES[drive]:
            g.iterate(n)
            launches.append(state(g))
        g.close()
        out[name] = launches
        for i, s in enumerate(launches):  # the commit is complete at the end of every launch, on every route
            assert_committed(s, dtype, "%s T=%d B=%d %s launch %d" % (name, T, B, dtype, i))
            accepted += int((s["al"] >= 0).sum())
    for other in ("quad_chain", "staged"):
        for i, (a, b) in enumerate(zip(out["hex"], out[other])):
            assert_same_bits(a, b, dtype, "hex / %s T=%d B=%d %s drive %s launch %d" % (other, T, B, dtype, drive, i))
    ACCEPTED["T=%d B=%d %s %s" % (T, B, dtype, drive)] = accepted


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_trajectories_of_one_quad_finish_at_different_iterations(dtype):
    """a full solve without ILQR_FLAG_FIXED_WORK: trajectories leave their loops one by one, a quad's lanes of a finished trajectory
    compute along and store nothing, a quad with nobody left skips its rollout and still meets every barrier"""
    B, T = 37, 33
    x0, u0 = start(B, T, dtype)
    out = {}
    for name, flags, route, kernel in routes()[:2]:
        g = make(B, T, dtype, flags, route, kernel, max_iter=200)
        g.init_traj(x0, u0)
        g.generate_trajectory()
        out[name] = state(g, candidates=False)
        g.close()
    assert_same_bits(out["hex"], out["quad_chain"], dtype, "full solve %s" % dtype)
    it = out["hex"]["it"]
    assert np.all(out["hex"]["st"] != 0)
    quads = [it[q:q + 4] for q in range(0, B - B % 4, 4)]
    assert any(len(set(q.tolist())) > 1 for q in quads), "no quad whose trajectories finished at different iterations"


def test_commits_were_among_the_cases():
    """(runs last) the launch ends of the cases above must have had accepted candidates to commit -- after a first iteration and later,
    across the launch boundary, on every horizon and batch"""
    if not ACCEPTED:  # (selected on its own)
        test_quad_rollouts_leave_the_bits_of_the_other_routes(33, 37, "f64", "3+2")
    with_work = [c for c, n in ACCEPTED.items() if n > 0]
    print("\ncases with accepts at a launch end: %d of %d" % (len(with_work), len(ACCEPTED)))
    assert len(with_work) * 2 > len(ACCEPTED), sorted(set(ACCEPTED) - set(with_work))
