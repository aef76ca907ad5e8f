"""The lane maps of k_solve_hex's quad rollouts (ilqr_amd/csrc/quad_lanes.hpp) compiled for the HOST.  The wavefront of pair s rolls
out the four trajectories 4 s + q under the eleven alphas on lanes 4 alpha + q, and lanes 4 row + q pass the quad's nominal rows of a
step (u, k, K[4], xs[4]: ten per trajectory) from memory through the wavefront's LDS:

  * lanes 0..43 are a bijection onto the 44 (alpha, trajectory) pairs, the four pairs' wavefronts together onto the tile's 176;
  * the fetching lanes cover the 40 (row, trajectory) pairs, each once on lanes 0..39; a lane beyond them repeats a pair another lane
    has, address and slot alike;
  * the LDS elements a wavefront writes are exactly the elements its rollout lanes read;
  * an unclamped prefetch PD steps ahead reads the element the arrays' own index map names while it is inside the horizon, and beyond
    it stays inside what ilqr_create allocates (the layout plus rollout_fetch_slack_elems), for T = 1, 7, 8, 9 and the last tile."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "quad_lanes_host.hip")
SO = os.path.join(HERE, "native", "libquad_lanes_host.so")
HIPCC = "/opt/rocm/bin/hipcc"
TW, NALPHA, NX, NU = 16, 11, 4, 1
ip = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "ilqr_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in ("quad_lanes.hpp", "rollout.hpp", "layout.hpp", "common.hpp", "boxqp.hpp", "models.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, SRC])
    lib = C.CDLL(SO)
    lib.quad_fetch_elem.restype = C.c_longlong
    lib.quad_tidx.restype = C.c_longlong
    lib.quad_alloc_elems.restype = C.c_longlong
    return lib


def ints(n=64):
    return (C.c_int * n)()


def test_rollout_lanes_are_a_bijection_onto_alpha_x_trajectory(lib):
    n = lib.quad_rollout_lane_count()
    assert n == 4 * NALPHA == 44
    tile = []
    for s in range(4):
        alpha, l = ints(), ints()
        lib.quad_rollout_map(s, alpha, l)
        mine = [(alpha[j], l[j]) for j in range(n)]
        assert sorted(mine) == [(a, 4 * s + q) for a in range(NALPHA) for q in range(4)]
        assert all(alpha[j] >= NALPHA for j in range(n, 64))  # the lanes behind have no alpha: they sit the rollout out
        tile += mine
    assert sorted(tile) == [(a, l) for a in range(NALPHA) for l in range(TW)]


def test_fetch_lanes_are_a_bijection_onto_row_x_trajectory(lib):
    rows = lib.quad_row_count(NX, NU)
    assert rows == 10
    n = lib.quad_rollout_lane_count()
    for s in range(4):
        row, l, slot = ints(), ints(), ints()
        lib.quad_fetch_map(s, rows, row, l, slot)
        own = [(row[j], l[j]) for j in range(4 * rows)]
        assert sorted(own) == [(r, 4 * s + q) for r in range(rows) for q in range(4)]
        assert len(set(slot[j] for j in range(4 * rows))) == 4 * rows  # one LDS element each
        for j in range(4 * rows, n):  # a repeat of a pair that has its owner: same trajectory as the lane rolls out, same slot
            k = own.index((row[j], l[j]))
            assert slot[j] == slot[k] and l[j] == 4 * s + j % 4


def test_a_wavefront_writes_exactly_the_lds_elements_its_lanes_read(lib):
    rows = lib.quad_row_count(NX, NU)
    n = lib.quad_rollout_lane_count()
    assert rows % 2 == 0
    for s in range(4):
        row, l, slot = ints(), ints(), ints()
        lib.quad_fetch_map(s, rows, row, l, slot)
        written = {slot[j]: (row[j], l[j]) for j in range(n)}
        alpha, lt = ints(), ints()
        lib.quad_rollout_map(s, alpha, lt)
        read = set()
        for j in range(n):
            sl = ints(rows)
            lib.quad_read_slots(s, j, rows // 2, sl)
            for r in range(rows):  # element r of what the lane reads is row r of the trajectory the lane rolls out
                assert written[sl[r]] == (r, lt[j])
            read |= set(sl)
        assert read == set(written)
        assert max(read) < 4 * ((rows + 3) // 4) * TW  # inside the wavefront's share of LDS (k_solve_hex: kShareReals)


@pytest.mark.parametrize("T", [1, 7, 8, 9])
def test_the_prefetch_reads_the_right_rows_and_stays_inside_the_slack(lib, T):
    rows = lib.quad_row_count(NX, NU)
    PD = lib.quad_prefetch_depth()
    assert PD == 8
    ntiles = 8
    dims = {0: (T, NU, 0), 1: (T, NU, 0), 2: (T, NU * NX, 0), 3: (T + 1, NX, 0)}  # array -> knots, elements per knot
    alloc = {a: lib.quad_alloc_elems(ntiles, S, E, NX, NU) for a, (S, E, _) in dims.items()}
    first_row = {0: 0, 1: NU, 2: 2 * NU, 3: 2 * NU + NU * NX}
    furthest = dict.fromkeys(dims, 0)
    for tile in (0, ntiles - 1):
        for s in range(4):
            row, l, slot = ints(), ints(), ints()
            lib.quad_fetch_map(s, rows, row, l, slot)
            for j in range(lib.quad_rollout_lane_count()):
                arr = C.c_int()
                for tt in range(T + PD):  # the ring is filled with steps 0 .. PD - 1, step s_ refills with s_ + PD, s_ <= T - 1
                    e = lib.quad_fetch_elem(NX, NU, T, tile, s, j, tt, C.byref(arr))
                    S, E, _ = dims[arr.value]
                    if tt < S:
                        assert e == lib.quad_tidx(tile, tt, row[j] - first_row[arr.value], l[j], S, E)
                    assert 0 <= e < alloc[arr.value]
                    furthest[arr.value] = max(furthest[arr.value], e)
    # (the bound is not idle: the gains' last fetch of the last tile ends on the allocation's last element)
    assert furthest[2] == alloc[2] - 1
