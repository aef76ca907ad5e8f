"""The index maps of ilqr_amd/csrc/layout.hpp compiled for the HOST: where element (b, s, e) of a canonical [B][n][E] array lives in a
handle's array, for each of the three device layouts, against a numpy statement of the layout written from the comments in common.hpp:

    tiled plain array      [tile][S][E][16]
    tiled record block     [tile][T+1][REC/2][16][2], element e of a record at pair e >> 1, slot e & 1
    trajectory-contiguous  [b][S][stride]

Every map must equal that statement, be injective, and stay inside what the handle allocates for the array (dev_elems /
ensure_records = layout_elems), for ragged batches, knot windows and every block of the derivative records."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "layout_host.hip")
SO = os.path.join(HERE, "native", "liblayout_host.so")
HIPCC = "/opt/rocm/bin/hipcc"
TW = 16
BATCHES = [1, 15, 16, 17, 19, 130]
KNOTS = [1, 2, 9]
RECORD_DIMS = [(4, 1), (4, 2), (6, 3), (32, 16)]
llp, ip = C.POINTER(C.c_longlong), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "ilqr_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in ("layout.hpp", "common.hpp", "boxqp.hpp", "models.hpp")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, SRC])
    lib = C.CDLL(SO)
    lib.layout_tiled.argtypes = [C.c_int] * 5 + [llp]
    lib.layout_tiled_rec.argtypes = [C.c_int] * 7 + [llp]
    lib.layout_aos.argtypes = [C.c_int] * 7 + [llp]
    lib.layout_alloc_elems.argtypes = [C.c_int] * 5
    lib.layout_alloc_elems.restype = C.c_longlong
    lib.layout_rec_offsets.argtypes = [C.c_int, C.c_int, ip, ip]
    return lib


def ntiles_of(B):
    """ilqr_create: the batch padded to whole 64-trajectory groups, in tiles of 16"""
    return (B + 63) // 64 * 4


def windows(S):
    """(t0, n): all knots, the first, the last, and -- where S has room -- a window strictly inside [0, S)"""
    w = {(0, S), (0, 1), (S - 1, 1)}
    if S >= 3:
        w |= {(1, 1), (2, S - 4)} if S >= 7 else {(1, 1)}
    return sorted(w)


def call(fn, B, n, E, *args):
    out = np.full((B, n, E), -1, dtype=np.int64)
    fn(*args, out.ctypes.data_as(llp))
    return out


def check(got, want, alloc):
    assert np.array_equal(got, want)
    assert len(np.unique(got)) == got.size  # injective
    assert got.min() >= 0 and got.max() < alloc


def record_blocks(nx, nu):
    """common.hpp, struct Rec: blocks stored in the order fx, fu, cx, cxx, cxu, cu, cuu (the two odd-sized ones last); (offset, length)
    of each in the ABI's order fx, fu, cx, cu, cxx, cxu, cuu"""
    sizes = dict(fx=nx * nx, fu=nx * nu, cx=nx, cxx=nx * nx, cxu=nx * nu, cu=nu, cuu=nu * nu)
    at, o = {}, 0
    for name in ("fx", "fu", "cx", "cxx", "cxu", "cu", "cuu"):
        at[name] = o
        o += sizes[name]
    return [(at[k], sizes[k]) for k in ("fx", "fu", "cx", "cu", "cxx", "cxu", "cuu")], o


@pytest.mark.parametrize("B", BATCHES)
def test_tiled_plain_array(lib, B):
    nt = ntiles_of(B)
    for S in KNOTS:
        for E in (1, 4, 6):
            alloc = lib.layout_alloc_elems(0, B, nt, S, E)
            dev = np.arange(nt * S * E * TW, dtype=np.int64).reshape(nt, S, E, TW)  # [tile][S][E][16]
            assert alloc == dev.size
            canon = dev.transpose(0, 3, 1, 2).reshape(nt * TW, S, E)  # b = tile * 16 + lane
            for t0, n in windows(S):
                check(call(lib.layout_tiled, B, n, E, B, S, E, t0, n), canon[:B, t0:t0 + n], alloc)


@pytest.mark.parametrize("nx,nu", RECORD_DIMS)
def test_record_offsets(lib, nx, nu):
    off, ln = (C.c_int * 7)(), (C.c_int * 7)()
    blocks, rec = record_blocks(nx, nu)
    assert lib.layout_rec_offsets(nx, nu, off, ln) == rec and rec % 2 == 0
    assert list(zip(off, ln)) == blocks
    covered = sorted(e for o, n in blocks for e in range(o, o + n))
    assert covered == list(range(rec))  # the seven blocks tile the record


@pytest.mark.parametrize("nx,nu", RECORD_DIMS)
@pytest.mark.parametrize("B", BATCHES)
def test_tiled_record_blocks(lib, B, nx, nu):
    nt = ntiles_of(B)
    blocks, rec = record_blocks(nx, nu)
    for S in KNOTS:
        alloc = lib.layout_alloc_elems(0, B, nt, S, rec)
        dev = np.arange(nt * S * rec * TW, dtype=np.int64).reshape(nt, S, rec // 2, TW, 2)  # [tile][T+1][REC/2][16][2]
        assert alloc == dev.size
        canon = dev.transpose(0, 3, 1, 2, 4).reshape(nt * TW, S, rec)  # element e = 2 * pair + slot
        seen = []
        for off, E in blocks:
            for t0, n in windows(S):
                got = call(lib.layout_tiled_rec, B, n, E, B, S, rec, off, E, t0, n)
                check(got, canon[:B, t0:t0 + n, off:off + E], alloc)
                if (t0, n) == (0, S):
                    seen.append(got.ravel())
        assert len(np.unique(np.concatenate(seen))) == B * S * rec  # no two blocks share an element


@pytest.mark.parametrize("B", BATCHES)
def test_trajectory_contiguous(lib, B):
    for S in KNOTS:
        # plain arrays: stride = E, off = 0 -- the canonical array itself
        for E in (1, 4, 6):
            alloc = lib.layout_alloc_elems(1, B, ntiles_of(B), S, E)
            dev = np.arange(B * S * E, dtype=np.int64).reshape(B, S, E)  # [b][S][E]
            assert alloc == dev.size
            for t0, n in windows(S):
                check(call(lib.layout_aos, B, n, E, B, S, E, 0, E, t0, n), dev[:, t0:t0 + n], alloc)
        # record blocks: stride = REC
        for nx, nu in RECORD_DIMS:
            blocks, rec = record_blocks(nx, nu)
            alloc = lib.layout_alloc_elems(1, B, ntiles_of(B), S, rec)
            dev = np.arange(B * S * rec, dtype=np.int64).reshape(B, S, rec)  # [b][S][stride]
            assert alloc == dev.size
            for off, E in blocks:
                for t0, n in windows(S):
                    check(call(lib.layout_aos, B, n, E, B, S, rec, off, E, t0, n), dev[:, t0:t0 + n, off:off + E], alloc)
