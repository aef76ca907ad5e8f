"""The claim the compact ring record of k_solve_hex rests on (csrc/models.hpp: state_free_running_cost), checked on the CPU with the
product's own finite-difference code compiled for the host: the acrobot's running cost does not read the state, so every entry of
cx, cxx and cxu that derivatives_of_knot computes for a full record of a knot t < T is the same value as the record's one number
Z = c - c, bit for bit: +0.0 for a finite cost, NaN for an overflowing one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "state_free_cost_host.hip")
SO = os.path.join(HERE, "native", "libstate_free_cost_host.so")
HIPCC = "/opt/rocm/bin/hipcc"
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def dev():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    csrc = os.path.join(os.path.dirname(HERE), "ilqr_amd", "csrc")
    newest = max([os.path.getmtime(SRC)] + [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc)])
    if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
        subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-o", SO, SRC])
    lib = C.CDLL(SO)
    lib.devfn_acrobot_dropped_entries.argtypes = [dp, C.c_double, dp]
    lib.devfn_acrobot_dropped_entries.restype = None
    lib.devfn_acrobot_dropped_entries_f32.argtypes = [C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float)]
    lib.devfn_acrobot_dropped_entries_f32.restype = None
    return lib


def _entries(lib, x, u):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.full(25, 7.0)
    lib.devfn_acrobot_dropped_entries(x.ctypes.data_as(dp), float(u), out.ctypes.data_as(dp))
    return out


STATES = [np.zeros(4), np.array([3.1415, 0.0, 0.0, 0.0]), np.array([-2.5, 1.25, 7.0, -11.0]), np.array([1e-310, -5e-324, 1e8, -1e-8])]


@pytest.mark.parametrize("u", [0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, 1.5, -1.5, 1e150, -1e150])
def test_dropped_entries_of_a_finite_cost_are_c_minus_c(dev, u):
    for x in STATES:
        out = _entries(dev, x, u)
        z = out[24:25].view(np.uint64)[0]
        assert z == 0, (u, x, out[24])  # +0.0
        assert np.array_equal(out[:24].view(np.uint64), np.full(24, z, dtype=np.uint64)), (u, x, out)


@pytest.mark.parametrize("u", [1e200, -1e200, float("inf"), float("nan")])
def test_dropped_entries_of_a_non_finite_cost_are_nan_like_c_minus_c(dev, u):
    for x in STATES:
        out = _entries(dev, x, u)
        assert np.isnan(out[24]) and np.all(np.isnan(out[:24])), (u, x, out)


def _entries_f32(lib, x, u):
    fp = C.POINTER(C.c_float)
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.full(25, 7.0, dtype=np.float32)
    lib.devfn_acrobot_dropped_entries_f32(x.ctypes.data_as(fp), float(np.float32(u)), out.ctypes.data_as(fp))
    return out


@pytest.mark.parametrize("u", [0.0, -0.0, 1e-45, -1e-45, 1e-40, 1.5, -1.5, 1e15, -1e15])
def test_float_instantiation_finite(dev, u):
    for x in STATES:
        out = _entries_f32(dev, x, u)
        assert np.array_equal(out.view(np.uint32), np.zeros(25, dtype=np.uint32)), (u, x, out)  # every entry and c - c: +0.0


@pytest.mark.parametrize("u", [1e25, float("inf"), float("nan")])
def test_float_instantiation_non_finite(dev, u):
    for x in STATES:
        assert np.all(np.isnan(_entries_f32(dev, x, u))), (u, x)
