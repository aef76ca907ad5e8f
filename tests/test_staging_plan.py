"""The staging plans (ilqr_amd/csrc/staging.hpp) compiled for the HOST: where every host getter of the stored-model queries puts each of
its arrays in the handle's staging buffer, for every subset of its optional pointers, against the layout written out here by hand from
the getters as they stood before they shared a plan (offset chains, one per getter).  tests/native/staging_host.cpp calls the very
functions capi.hip's getters call, so a slip in a declaration shows here, on a machine without a GPU."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "staging_host.cpp")
SO = os.path.join(HERE, "native", "libstaging_host.so")
HIPCC = "/opt/rocm/bin/hipcc"

B, T, NTP = 3, 5, 3
SHAPES = [(6, 3), (4, 1)]  # a generic handle's and a tiled handle's
ND, NY, NW, NS, T0, NK = 2, 2, 2, 2, 1, 3
UP, DOWN = 1, 0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    deps = [SRC, os.path.join(ROOT, "ilqr_amd", "csrc", "staging.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([HIPCC, "-x", "c++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, SRC])
    return C.CDLL(SO)


# ---- the layout before the plan: per getter, its pointers in staging order as (elements, direction, is the int array `info`) ----
def value(nx, nu):
    return [(B * NK * nx, DOWN, False), (B * NK * nx * nx, DOWN, False)], []


def covariance(nx, nu):
    nn = B * nx * nx
    return [(nn, UP, False), (nn, UP, False), (nn * NK, DOWN, False), (B * NK * nu * nu, DOWN, False), (B, DOWN, False)], []


def _sens(nx, nu):
    per_x, per_u = B * ND * nx, B * ND * nu
    return per_x, per_u * T, per_x * NK, per_u * (min(T0 + NK, T) - T0)  # x_one, u_all, x_win, u_win


def tangent(nx, nu):
    x_one, u_all, x_win, u_win = _sens(nx, nu)
    return [(x_one, UP, False), (u_all, UP, False), (x_win, DOWN, False), (u_win, DOWN, False)], []


def adjoint(nx, nu):
    x_one, u_all, x_win, u_win = _sens(nx, nu)
    return [(x_win, UP, False), (u_win, UP, False), (x_one, DOWN, False), (u_all, DOWN, False)], []


def lq_solve(nx, nu):
    per_x, per_u = B * ND * nx, B * ND * nu
    return [(per_x, UP, False), (per_x * (T + 1), UP, False), (per_u * T, UP, False), (per_x * (T + 1), DOWN, False), (per_u * T, DOWN, False),
            (per_x * (T + 1), DOWN, False), (B, DOWN, True)], []


def estimator(nx, nu):
    nn = B * nx * nx
    return [(B * NY * nx, UP, False), (nn, UP, False), (nn, UP, False), (B * NY * NY, UP, False), (nn * NK, DOWN, False), (nn * NK, DOWN, False),
            (B * NK * nx * NY, DOWN, False), (nn * NK, DOWN, False), (B * NK * nu * nu, DOWN, False), (B, DOWN, False), (B, DOWN, True)], [0, 3]  # H, V


def risk(nx, nu):
    return [(B * nx * NW, UP, False), (B * T * nu * nx, DOWN, False), (B * T * nu, DOWN, False), (B * (T + 1) * nx, DOWN, False),
            (B * (T + 1) * nx * nx, DOWN, False), (B, DOWN, False), (B, DOWN, True)], [0]  # C


def evaluate(nx, nu):
    R = B * NS
    return [(R * nx, UP, False), (R, DOWN, False), (R * nx, DOWN, False), (R * nu, DOWN, False)], [0]  # x


def param_gradient(nx, nu):
    per_x, per_u = B * ND * nx, B * ND * nu
    return [(per_x * (T + 1), UP, False), (per_u * T, UP, False), (per_x * (T + 1), UP, False), (B * ND * NTP, DOWN, False), (B * (T + 1) * nx, DOWN, False)], []


GETTERS = [value, covariance, tangent, adjoint, lq_solve, estimator, risk, evaluate, param_gradient]


def expected(arrays, given):
    """The prefix sum every getter wrote out by hand: a null pointer takes no room; info's B ints take (B + 1) / 2 doubles and copy
    B * sizeof(int) bytes.  Per pointer: (offset in doubles, room in doubles, bytes copied, direction, int array, device byte offset or -1)."""
    at, segs = 0, []
    for (n, direction, ints), g in zip(arrays, given):
        room = 0 if not g else (n + 1) // 2 if ints else n
        nbytes = 0 if not g else n * (4 if ints else 8)
        segs.append((at, room, nbytes, direction, int(ints), 8 * at if g else -1))
        at += room
    return segs, at


@pytest.mark.parametrize("nx,nu", SHAPES)
@pytest.mark.parametrize("getter", GETTERS, ids=lambda g: g.__name__)
def test_every_null_pattern_has_the_layout_the_getter_wrote_by_hand(lib, getter, nx, nu):
    arrays, required = getter(nx, nu)
    assert len(arrays) <= lib.stage_max_segments()
    fn = getattr(lib, "stage_%s_plan" % getter.__name__)
    fn.argtypes = [C.POINTER(C.c_size_t)] + [C.c_size_t] * 6 + [C.c_uint, C.POINTER(C.c_longlong)]
    fn.restype = None
    dims = (C.c_size_t * 5)(B, T, nx, nu, NTP)
    optional = [i for i in range(len(arrays)) if i not in required]
    for pattern in itertools.product([False, True], repeat=len(optional)):
        given = [True] * len(arrays)
        for i, g in zip(optional, pattern):
            given[i] = g
        out = (C.c_longlong * (2 + 6 * 11))()
        fn(dims, T0, NK, ND, NY, NW, NS, sum(1 << i for i, g in enumerate(given) if g), out)
        want, total = expected(arrays, given)
        got = [tuple(out[2 + 6 * i: 8 + 6 * i]) for i in range(out[0])]
        assert (out[0], out[1], got) == (len(arrays), total, want), given
        # what the layout must guarantee whatever the formulas: null -> no room and a null device pointer; the rest disjoint, inside the
        # buffer, 8-byte aligned (offsets are counted in whole doubles)
        spans = []
        for (off, room, nbytes, _, ints, dev), g in zip(got, given):
            if not g:
                assert (room, nbytes, dev) == (0, 0, -1)
                continue
            assert dev == 8 * off and dev % 8 == 0 and 0 < nbytes <= 8 * room and 8 * (off + room) <= 8 * out[1]
            spans.append((dev, dev + 8 * room))
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), given
        assert sum(b - a for a, b in spans) == 8 * out[1]
