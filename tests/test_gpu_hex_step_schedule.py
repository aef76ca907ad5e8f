"""k_solve_hex's chain takes the knots of a pass in groups of four ring slots (csrc/backward_hex.hpp: HexGate, kHexSlotPhases): its step
loop is unrolled by four, a knot's slot is the group's plus an immediate, the ring's bookkeeping and the published index move once per
group, and the compact ring has 44 slots; the step's nine matrix instructions are issued in three places of the step instead of one.
None of this changes an expression, so the kernel must leave, TO THE BIT, what the quad-chain route (ILQR_ROUTE_QUAD_CHAIN:
k_solve_tile) and the staged route (ILQR_FLAG_STAGED: one kernel per stage) leave after 8 iterations: xs, us, k, K, cost, lambda,
status and iteration counts, compared as raw bit patterns, plain and with ILQR_FLAG_FIXED_WORK, in fp64 and fp32 handles.

Shapes, for where the groups can go wrong: T = 3 is shorter than the unroll; T = 46 and 93 make the compact ring (44 slots) wrap once
and twice, and T + 1 = 47 and 94 leave remainders of 3 and 2 knots behind the last whole group; T = 130 makes the full ring of 24 slots
(the user twin of the acrobot: no state_free_running_cost, so full records) wrap five times.  B = 1 is one lane of one chain, 5 a
partial quad, 16 a full tile, 21 a second, partial tile.  Limits +-1.5 and +-5 are the bench's; +-0.02 clamps nearly every control,
which is where the box-QP leaves early and where the Armijo search goes beyond k = 16.

A lambda retry restarts a pass with the running index in the middle of the ring.  No public parameter forces one in this kernel: its
box-QP does not test Quu + lambda for definiteness (that is the opt-in ILQR_FLAG_REFERENCE_FIXES, which takes another route), so a pass
is abandoned only when a box-QP's own line search fails, and neither a large nor a small lambda_init, nor lambda set to 0 or below
-(cuu + 50) through set_lambda, made the stand-alone backward stage report a diverged knot on any shape tried (T = 46 .. 499, B = 21 and 48,
three limits, up to 60 iterations).  So the last test takes the state named for that case instead: 25 fixed-work iterations into the
solve of tests/test_gpu_parity.py's late-solve setup (B = 48, T = 499, limits +-1.5: lambda at 0 for most trajectories, controls on the
bounds, search directions that are rounding noise), and walks 8 iterations from there one at a time.  It reports how many first passes
the stand-alone backward stage sees abandoned there (none, when this was written): the restart itself is exercised by
scripts/soak_hex.py's whole solves and, for the ring's bounds, by the abandoned passes of tests/test_hex_ring_bounds.py."""
import numpy as np
import pytest

from tests.util import acrobot_x0

pytestmark = pytest.mark.gpu
DT = 0.02
ITERS = 8
LIMITS = (1.5, 5.0, 0.02)
USER_PARAMS = [3.1415, 0, 0, 0, 20, 20]  # the shipped acrobot's goal and weights (tests/test_gpu_user_model.py)


@pytest.fixture(scope="module")
def user_lib():
    from ilqr_amd import _build
    return _build.build_user(_build.USER_EXAMPLE_HEADER, _build.USER_EXAMPLE_LIB)


def bits(a, dtype):
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    return a.view(np.uint64) if dtype == "f64" else a.astype(np.float32).view(np.uint32)


def state(g):
    xs, us = g.trajectory()
    k, K = g.gains()
    st, it, al = g.status()
    lam, dlam = g.lambdas()
    return dict(xs=xs, us=us, k=k, K=K, cost=g.cost(), lam=lam, dlam=dlam, st=st, it=it)


def assert_same_bits(a, b, dtype, what):
    assert a.keys() == b.keys()
    for n in a:
        dt = "f64" if n in ("lam", "dlam") else dtype  # lambda and dlambda are doubles in a float handle too
        x, y = bits(a[n], dt), bits(b[n], dt)
        if not np.array_equal(x, y):
            bad = np.argwhere(x != y)
            raise AssertionError("%s: %s differs in %d of %d entries, first at %s: %r / %r"
                                 % (what, n, len(bad), x.size, bad[0], a[n][tuple(bad[0])], b[n][tuple(bad[0])]))


def routes():
    from ilqr_amd import capi
    return (("hex", 0, 0, b"k_solve_hex"), ("quad_chain", 0, capi.ROUTE_QUAD_CHAIN, b"k_solve_tile"), ("staged", capi.FLAG_STAGED, 0, None))


def make(model, B, T, lim, dtype, flags, route, kernel, lib=None):
    from ilqr_amd import BatchILQR, capi
    kw = dict(model="acrobot") if model == "acrobot" else dict(model="user", lib=lib, nx=4, nu=1, user_params=USER_PARAMS)
    g = BatchILQR(B=B, T=T, dt=DT, u_min=-lim, u_max=lim, flags=flags, route=route, dtype=dtype, params=dict(max_iter=40), **kw)
    if kernel is not None:
        assert g.lib.ilqr_stage_kernel_name(g.h, capi.STAGE_NAMES.index("solve")) == kernel
    return g


def start(B, T, dtype, scale=0.6):
    x0 = acrobot_x0(B, scale=scale, seed=500 + T)
    if dtype == "f32":
        x0 = x0.astype(np.float32).astype(np.float64)
    return x0, np.zeros((B, T, 1))


def compare_routes(model, B, T, lim, dtype, fixed, lib=None):
    from ilqr_amd import capi
    x0, u0 = start(B, T, dtype)
    out = {}
    for name, flags, route, kernel in routes():
        g = make(model, B, T, lim, dtype, flags | (capi.FLAG_FIXED_WORK if fixed else 0), route, kernel, lib)
        g.init_traj(x0, u0)
        g.iterate(ITERS)
        out[name] = state(g)
        g.close()
    what = "%s T=%d B=%d lim=%g %s %s" % (model, T, B, lim, dtype, "fixed work" if fixed else "plain")
    for other in ("quad_chain", "staged"):
        assert_same_bits(out["hex"], out[other], dtype, "hex / %s %s" % (other, what))
    return out["hex"]


@pytest.mark.parametrize("fixed", [False, True], ids=["plain", "fixed_work"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 5, 16, 21])
@pytest.mark.parametrize("T", [3, 46, 93, 130])
def test_compact_ring_in_groups_of_four_leaves_the_bits_of_the_other_routes(T, B, dtype, fixed):
    """the built-in acrobot: compact slots, a ring of 44"""
    for lim in LIMITS:
        s = compare_routes("acrobot", B, T, lim, dtype, fixed)
        if fixed:
            assert np.all(s["it"] == ITERS)


@pytest.mark.parametrize("fixed", [False, True], ids=["plain", "fixed_work"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 5, 16, 21])
@pytest.mark.parametrize("T", [3, 46, 93, 130])
def test_full_ring_in_groups_of_four_leaves_the_bits_of_the_other_routes(user_lib, T, B, dtype, fixed):
    """the user twin of the acrobot: full records, a ring of 24 (T = 130: five wraps)"""
    for lim in LIMITS:
        compare_routes("user", B, T, lim, dtype, fixed, lib=user_lib)


def abandoned_knots(probe, g, x0):
    """Where the FIRST backward pass of g's next iteration gives up, per trajectory (0: it runs through): g's state copied into a
    second handle, whose stand-alone backward stage (one pass at the current lambda, no retry) reports the knot it diverged at."""
    xs, us = g.trajectory()
    k, K = g.gains()
    lam, dlam = g.lambdas()
    probe.set_trajectory(x0=x0, xs=xs, us=us, cost=g.cost())
    probe.set_gains(k=k, K=K)
    probe.set_lambda(lam, dlam)
    probe.compute_derivatives()
    return probe.backward_pass()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model", ["acrobot", "user"])
def test_late_in_a_solve_leaves_the_bits_of_the_other_routes(user_lib, model, dtype):
    """The late-solve state of tests/test_gpu_parity.py (B = 48, T = 499, limits +-1.5, 25 fixed-work iterations in), then 8 iterations
    one by one: bit for bit on the three routes after every one of them.  Before each, the state goes through the stand-alone backward
    stage of a second handle, which names the knots at which a first pass would be abandoned (printed; see the module's docstring)."""
    from ilqr_amd import capi
    B, T, lim = 48, 499, 1.5
    x0 = acrobot_x0(B)
    if dtype == "f32":
        x0 = x0.astype(np.float32).astype(np.float64)
    u0 = np.zeros((B, T, 1))
    out, knots = {}, []
    for name, flags, route, kernel in routes():
        g = make(model, B, T, lim, dtype, flags | capi.FLAG_FIXED_WORK, route, kernel, user_lib)
        probe = make(model, B, T, lim, dtype, capi.FLAG_STAGED, 0, None, user_lib) if name == "hex" else None
        g.init_traj(x0, u0)
        g.iterate(25)
        steps = []
        for _ in range(ITERS):
            if probe is not None:
                div = abandoned_knots(probe, g, x0)
                knots += [int(i) for i in div[div > 0]]
            g.iterate(1)
            steps.append(state(g))
        out[name] = steps
        assert np.all(steps[-1]["it"] == 25 + ITERS)
        g.close()
        if probe is not None:
            probe.close()
    print("\n%s %s: first passes abandoned at knots %s (%s knots into the pass); lambda == 0 for %d of %d trajectories"
          % (model, dtype, knots, [T - i for i in knots], int((out["hex"][0]["lam"] == 0).sum()), B))
    for other in ("quad_chain", "staged"):
        for i, (a, b) in enumerate(zip(out["hex"], out[other])):
            assert_same_bits(a, b, dtype, "hex / %s iteration %d, %s %s" % (other, 25 + i, model, dtype))
