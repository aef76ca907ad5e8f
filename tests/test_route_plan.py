"""The route plan (ilqr_amd/csrc/route.hpp) compiled for the HOST: which kernel every stage of a handle runs -- the names
ilqr_stage_kernel_name reports, bench.py labels its record with and the GPU tests assert -- for the descriptors those tests create,
checked on a machine without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

from ilqr_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "route_host.cpp")
SO = os.path.join(HERE, "native", "libroute_host.so")
HIPCC = "/opt/rocm/bin/hipcc"
ACROBOT, INTEGRATOR, LQ, HOST, USER = capi.MODEL_ACROBOT, capi.MODEL_DOUBLE_INTEGRATOR, capi.MODEL_LQ, capi.MODEL_HOST, capi.MODEL_USER
# the example user twins' traits (models.hpp: kUserTiled, kUserSmall)
USER_ACROBOT, USER_LINEAR6, USER_CHAIN, USER_WIDE = (True, False), (True, True), (False, False), (False, False)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    deps = [SRC, os.path.join(ROOT, "ilqr_amd", "csrc", "route.hpp"), os.path.join(ROOT, "include", "ilqr_amd.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([HIPCC, "-x", "c++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", SO, SRC])
    lib = C.CDLL(SO)
    lib.route_kernel_names.argtypes = [C.c_int] * 10 + [C.POINTER(C.c_char_p)]
    lib.route_default_names.argtypes = [C.POINTER(C.c_char_p)]
    lib.route_wave_variants.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int)]
    lib.route_wave_variants.restype = C.c_char_p
    return lib


def names(lib, model, nx, nu, B, flags=0, route=0, cus=256, user=(False, False), cands=-1):
    """Stage -> kernel name of a handle of B trajectories (ntiles as ilqr_create counts them) on a device of `cus` CUs."""
    out = (C.c_char_p * capi.NUM_STAGES)()
    ntiles = (B + 63) // 64 * 4
    lib.route_kernel_names(model, nx, nu, flags, route, ntiles, cus, user[0], user[1], cands, out)
    return dict(zip(capi.STAGE_NAMES, out))


def test_a_null_handle_reports_the_defaults(lib):
    out = (C.c_char_p * capi.NUM_STAGES)()
    lib.route_default_names(out)
    assert list(out) == [b"k_derivatives", b"k_backward_t", b"k_rollout", b"k_accept", b""]


def test_the_fused_kernels(lib):
    """tests/test_gpu_fused_sweep.py::test_stage_kernel_name_reports_the_fused_kernel"""
    n = names(lib, ACROBOT, 4, 1, 16)
    assert (n["backward"], n["solve"]) == (b"k_sweep_backward", b"k_solve_hex")
    assert names(lib, INTEGRATOR, 4, 2, 16)["solve"] == b"k_solve_tile"
    assert names(lib, ACROBOT, 4, 1, 16, route=capi.ROUTE_QUAD_CHAIN)["solve"] == b"k_solve_tile"
    n = names(lib, ACROBOT, 4, 1, 16, flags=capi.FLAG_STAGED)
    assert (n["backward"], n["solve"]) == (b"k_sweep_backward", b"")
    n = names(lib, ACROBOT, 4, 1, 16, flags=capi.FLAG_UNFUSED)
    assert (n["derivatives"], n["backward"], n["rollout"], n["accept"], n["solve"]) == (b"k_derivatives", b"k_backward_q", b"k_rollout", b"k_accept", b"")
    n = names(lib, ACROBOT, 4, 1, 16, flags=capi.FLAG_BACKWARD_THREAD_PER_TRAJ)
    assert (n["backward"], n["solve"]) == (b"k_backward_t", b"")


@pytest.mark.parametrize("B", [16 * 6 + 16, 32 * 6, 48 * 6 + 3, 80 * 6 + 3])
def test_route_selection_by_batch_size(lib, B):
    """tests/test_gpu_fused_sweep.py::test_route_selection_by_batch_size: six CUs; one tile more than one per CU, two per CU,
    three per CU, five per CU and a ragged last tile"""
    two_per_cu = B <= 32 * 6
    n = names(lib, ACROBOT, 4, 1, B, cus=6)
    assert (n["backward"], n["solve"]) == (b"k_sweep_backward", b"k_solve_tile<2>" if two_per_cu else b"k_solve_wide")
    n = names(lib, ACROBOT, 4, 1, B, cus=6, flags=capi.FLAG_STAGED)
    assert (n["backward"], n["solve"]) == (b"k_sweep_backward" if two_per_cu else b"k_backward_q", b"")
    n = names(lib, ACROBOT, 4, 1, B, cus=6, flags=capi.FLAG_UNFUSED)
    assert (n["backward"], n["solve"]) == (b"k_backward_q", b"")
    assert names(lib, ACROBOT, 4, 1, 64, cus=6)["solve"] == b"k_solve_hex"  # four tiles on six CUs


def test_hex_and_the_quad_chain(lib):
    assert names(lib, ACROBOT, 4, 1, 4096)["solve"] == b"k_solve_hex"  # bench.py's headline
    assert names(lib, ACROBOT, 4, 1, 4096, route=capi.ROUTE_QUAD_CHAIN)["solve"] == b"k_solve_tile"
    assert names(lib, ACROBOT, 4, 1, 32768, route=capi.ROUTE_TILE_PER_CU)["solve"] == b"k_solve_hex"
    assert names(lib, ACROBOT, 4, 1, 32768, route=capi.ROUTE_TILE_PER_CU | capi.ROUTE_QUAD_CHAIN)["solve"] == b"k_solve_tile"
    assert names(lib, ACROBOT, 4, 1, 37, route=capi.ROUTE_TWO_TILES_PER_CU)["solve"] == b"k_solve_tile<2>"
    assert names(lib, USER, 4, 1, 64, user=USER_ACROBOT)["solve"] == b"k_solve_hex"  # the acrobot twin runs every nx = 4 kernel


@pytest.mark.parametrize("fix", [capi.FLAG_REFERENCE_FIXES, capi.FLAG_REGULARIZE_VXX])
def test_opt_in_fixes_leave_hex_and_the_wide_tiles(lib, fix):
    """tests/test_gpu_control_limits.py: with the fixes the persistent route is the 16-trajectory tile"""
    assert names(lib, ACROBOT, 4, 1, 37, flags=fix)["solve"] == b"k_solve_tile"
    assert names(lib, ACROBOT, 4, 1, 37, flags=fix | capi.FLAG_STAGED)["solve"] == b""
    assert names(lib, ACROBOT, 4, 1, 32768, flags=fix)["solve"] == b"k_solve_tile<2>"
    assert names(lib, ACROBOT, 4, 1, 300, flags=fix, route=capi.ROUTE_WIDE_TILES)["solve"] == b"k_solve_tile<2>"
    assert names(lib, INTEGRATOR, 4, 2, 32768, flags=fix)["solve"] == b"k_solve_tile<2>"


def test_wide_tiles(lib):
    """tests/test_gpu_fused_sweep.py, test_gpu_integrator_full_size.py, test_gpu_results.py, test_gpu_parity.py"""
    assert names(lib, ACROBOT, 4, 1, 32768)["solve"] == b"k_solve_wide"
    assert names(lib, ACROBOT, 4, 1, 37, route=capi.ROUTE_WIDE_TILES | capi.ROUTE_WIDE_TWO_PER_CU)["solve"] == b"k_solve_wide"
    assert names(lib, INTEGRATOR, 4, 2, 64, route=capi.ROUTE_WIDE_TILES)["solve"] == b"k_solve_wide2"
    assert names(lib, INTEGRATOR, 4, 2, 4096)["solve"] == b"k_solve_tile"
    assert names(lib, INTEGRATOR, 4, 2, 8192)["solve"] == b"k_solve_tile<2>"
    assert names(lib, INTEGRATOR, 4, 2, 32768)["solve"] == b"k_solve_wide2"
    n = names(lib, ACROBOT, 4, 1, 37, flags=capi.FLAG_STAGED, route=capi.ROUTE_WIDE_TILES)  # staged: the one-producer sweep
    assert (n["backward"], n["solve"]) == (b"k_sweep_backward", b"")


@pytest.mark.parametrize("flags,route,derivatives,backward", [
    (capi.FLAG_ANALYTIC_DERIVATIVES, 0, b"", b"k_backward_w3"),  # the fused LQ route: no sweep
    (capi.FLAG_ANALYTIC_DERIVATIVES, capi.ROUTE_FULL_RECORDS, b"k_analytic_lq", b"k_backward_w3"),
    (capi.FLAG_ANALYTIC_DERIVATIVES | capi.FLAG_REGULARIZE_VXX, 0, b"k_analytic_lq", b"k_backward_w3"),
    (capi.FLAG_ANALYTIC_DERIVATIVES, capi.ROUTE_BACKWARD_W2, b"k_analytic_lq", b"k_backward_w2"),
    (capi.FLAG_ANALYTIC_DERIVATIVES, capi.ROUTE_TWO_CONTROL_TILES, b"k_analytic_lq", b"k_backward_w3w"),
    (0, 0, b"k_derivatives_lq", b"k_backward_w3"),
    (0, capi.ROUTE_LQ_DENSE_FD, b"k_derivatives_g", b"k_backward_w3"),
    (0, capi.ROUTE_BACKWARD_W2, b"k_derivatives_lq", b"k_backward_w2"),
])
def test_lq_derivatives_and_backward(lib, flags, route, derivatives, backward):
    """tests/test_gpu_lq_end_to_end.py, test_gpu_analytic.py, test_gpu_generic_backward.py, test_gpu_control_limits.py"""
    n = names(lib, LQ, 32, 16, 40, flags=flags, route=route)
    assert (n["derivatives"], n["backward"], n["rollout"], n["solve"]) == (derivatives, backward, b"k_rollout_lq", b"")


@pytest.mark.parametrize("route,cands,rollout", [(0, -1, b"k_rollout_lq"), (capi.ROUTE_LQ_RECOMMIT, -1, b"k_rollout_lq"),
                                                 (0, 0, b"k_rollout_lq"), (capi.ROUTE_LQ_THREAD_ROLLOUT, -1, b"k_rollout_g")])
def test_lq_rollouts(lib, route, cands, rollout):
    """tests/test_gpu_lq_end_to_end.py: the matrix-core search with or without candidate buffers, or the thread-per-rollout kernel"""
    assert names(lib, LQ, 6, 3, 30, flags=capi.FLAG_ANALYTIC_DERIVATIVES, route=route, cands=cands)["rollout"] == rollout


def test_more_than_16_controls(lib):
    """tests/test_gpu_wide_controls.py: two control tiles, the thread-per-rollout kernel"""
    for model, nx, nu, user in ((LQ, 32, 32, USER_WIDE), (LQ, 24, 20, USER_WIDE), (USER, 24, 20, USER_WIDE)):
        for flags in (0, capi.FLAG_ANALYTIC_DERIVATIVES):
            n = names(lib, model, nx, nu, 6, flags=flags, user=user)
            assert (n["derivatives"], n["backward"], n["rollout"]) == (b"k_derivatives_g", b"k_backward_w3w", b"k_rollout_g")
    assert names(lib, HOST, 24, 20, 6)["backward"] == b"k_backward_w3w"


ANALYTIC, REGV = capi.FLAG_ANALYTIC_DERIVATIVES, capi.FLAG_REGULARIZE_VXX


@pytest.mark.parametrize("nx,nu,flags,route,dtype,variant,value", [
    # (nt, mt, FULL, LQF, REGV, float storage) of k_backward_w3; FULL: nothing masked, 32 states and 16 controls
    (32, 16, 0, 0, capi.DTYPE_F64, (2, 1, 1, 0, 0, 0), b"k_value_w<2, 1>"),
    (16, 16, 0, 0, capi.DTYPE_F64, (1, 1, 0, 0, 0, 0), b"k_value_w<1, 1>"),
    (6, 3, 0, 0, capi.DTYPE_F64, (1, 1, 0, 0, 0, 0), b"k_value_w<1, 1>"),
    (24, 16, 0, 0, capi.DTYPE_F64, (2, 1, 0, 0, 0, 0), b"k_value_w<2, 1>"),
    (24, 20, 0, 0, capi.DTYPE_F64, (2, 2, 0, 0, 0, 0), b"k_value_w<2, 2>"),  # two control tiles
    (32, 32, ANALYTIC, 0, capi.DTYPE_F64, (2, 2, 0, 0, 0, 0), b"k_value_w<2, 2>"),  # ... never fused, never FULL
    (6, 3, 0, capi.ROUTE_TWO_CONTROL_TILES, capi.DTYPE_F64, (1, 2, 0, 0, 0, 0), b"k_value_w<1, 1>"),  # ... by route bit: the backward pass alone
    (32, 16, ANALYTIC, 0, capi.DTYPE_F64, (2, 1, 1, 1, 0, 0), b"k_value_w<2, 1>"),  # the fused LQ route
    (6, 3, ANALYTIC, 0, capi.DTYPE_F64, (1, 1, 0, 1, 0, 0), b"k_value_w<1, 1>"),
    (32, 16, ANALYTIC, capi.ROUTE_FULL_RECORDS, capi.DTYPE_F64, (2, 1, 1, 0, 0, 0), b"k_value_w<2, 1>"),
    (32, 16, REGV, 0, capi.DTYPE_F64, (2, 1, 0, 0, 1, 0), b"k_value_w<2, 1>"),  # REGULARIZE_VXX: masked, never fused
    (6, 3, ANALYTIC | REGV, 0, capi.DTYPE_F64, (1, 1, 0, 0, 1, 0), b"k_value_w<1, 1>"),
    (32, 16, 0, 0, capi.DTYPE_F32, (2, 1, 1, 0, 0, 1), b"k_value_w<2, 1>"),  # fp32: every one-tile variant again, on float storage
    (6, 3, ANALYTIC, 0, capi.DTYPE_F32, (1, 1, 0, 1, 0, 1), b"k_value_w<1, 1>"),
    (6, 3, REGV, 0, capi.DTYPE_F32, (1, 1, 0, 0, 1, 1), b"k_value_w<1, 1>"),
    (32, 16, 0, capi.ROUTE_BACKWARD_W2, capi.DTYPE_F64, (2, 1, 0, 0, 0, 0), b"k_value_w<2, 1>"),  # k_backward_w2<nt>
    (6, 3, 0, capi.ROUTE_BACKWARD_W2, capi.DTYPE_F64, (1, 1, 0, 0, 0, 0), b"k_value_w<1, 1>"),
])
def test_wave_kernel_variants(lib, nx, nu, flags, route, dtype, variant, value):
    """tests/test_gpu_generic_backward.py, test_gpu_wide_controls.py, test_gpu_generic_fp32.py, test_gpu_analytic.py, test_gpu_value.py: which
    instantiation of the wavefront-per-trajectory backward and value kernels an LQ handle of these sizes launches"""
    out = (C.c_int * 6)()
    name = lib.route_wave_variants(LQ, nx, nu, flags, route, dtype, out)
    assert (tuple(out), name) == (variant, value)
    # what launch.hpp builds of k_backward_w3: FULL over two row tiles only; REGV masked and unfused; two control tiles plain and in fp64
    nt, mt, full, lqf, regv, f32 = variant
    assert not (full and nt != 2) and not (regv and (full or lqf)) and not (mt == 2 and (full or lqf or regv or f32))


def test_tiled_handles_run_the_thread_value_kernel(lib):
    assert lib.route_wave_variants(ACROBOT, 4, 1, 0, 0, capi.DTYPE_F64, (C.c_int * 6)()) == b"k_value_t"


def test_host_evaluated_models(lib):
    for fl in (0, capi.FLAG_REFERENCE_FIXES, capi.FLAG_REGULARIZE_VXX):
        n = names(lib, HOST, 8, 2, 10, flags=fl)
        assert list(n.values()) == [b"k_derivatives_g", b"k_backward_w3", b"k_rollout_g", b"k_accept", b""]
    assert names(lib, HOST, 8, 2, 10, route=capi.ROUTE_BACKWARD_W2)["backward"] == b"k_backward_w2"
    assert names(lib, HOST, 8, 2, 10, route=capi.ROUTE_TWO_CONTROL_TILES)["backward"] == b"k_backward_w3w"


def test_user_twins(lib):
    """tests/test_gpu_user_model.py, test_gpu_user_chain.py"""
    n = names(lib, USER, 6, 2, 40, user=USER_LINEAR6)
    assert (n["derivatives"], n["backward"], n["rollout"], n["solve"]) == (b"k_derivatives", b"k_backward_t", b"k_rollout", b"")
    n = names(lib, USER, 6, 2, 40, user=USER_LINEAR6, route=capi.ROUTE_WAVE_PER_TRAJECTORY)
    assert (n["derivatives"], n["backward"], n["rollout"], n["solve"]) == (b"k_derivatives_g", b"k_backward_w3", b"k_rollout_g", b"")
    for fl in (0, capi.FLAG_ANALYTIC_DERIVATIVES):
        n = names(lib, USER, 16, 4, 23, user=USER_CHAIN, flags=fl)
        assert (n["derivatives"], n["backward"], n["rollout"]) == (b"k_derivatives_g", b"k_backward_w3", b"k_rollout_g")
    assert names(lib, USER, 16, 4, 23, user=USER_CHAIN, route=capi.ROUTE_BACKWARD_W2)["backward"] == b"k_backward_w2"
