"""The multi-start entry points exist in every layer that names them (no GPU): include/ilqr_amd.h declares them under ABI 6 with the enum
of the clone flags, ilqr_amd/capi.py binds them with the declared argument types and carries the two constants, the built library exports
them, and each refuses a null handle before it looks for a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ilqr_amd.h")
ERR_INVALID = -1

_ip = C.POINTER(C.c_int)
# name -> the C parameter list, and its ctypes image
DECLARED = {
    "ilqr_select_best": ("ilqr_batch* h, int group, int* src, void* src_device", [C.c_void_p, C.c_int, _ip, C.c_void_p]),
    "ilqr_clone_trajectories": ("ilqr_batch* h, const int* src, const void* src_device, const void* du_device",
                                [C.c_void_p, _ip, C.c_void_p, C.c_void_p]),
    "ilqr_clone_best": ("ilqr_batch* h, int group, const void* du_device", [C.c_void_p, C.c_int, C.c_void_p]),
    "ilqr_get_clone_flags": ("ilqr_batch* h, int* flags", [C.c_void_p, _ip]),
    "ilqr_copy_clone_flags_to_device": ("ilqr_batch* h, void* flags_device", [C.c_void_p, C.c_void_p]),
}


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def _library():
    from ilqr_amd import _build
    if not os.path.exists(_build.LIB) and not os.path.exists(_build.HIPCC):
        pytest.skip("no built library and no hipcc to build one")
    return C.CDLL(_build.build())  # (loading needs no device)


def test_header_declares_the_clone_calls_under_abi_6():
    text = open(HEADER).read()
    assert re.search(r"#define\s+ILQR_AMD_ABI_VERSION\s+6\b", text)
    for name, (params, _) in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert _norm(m.group(1)) == _norm(params), name
    assert re.search(r"enum\s+ilqr_clone_why\s*\{\s*ILQR_WAS_CLONED\s*=\s*1\s*,\s*ILQR_CLONE_REFUSED\s*=\s*2\s*\}", text)
    # the comment states the definition: the source rule, what is not copied, the du arithmetic and its stale cost
    doc = text[text.index("/* ---- multi-start groups"):text.index("int ilqr_select_best(")]
    for phrase in ("src[s] == s or src[s] < 0", "du[b][t][e]", "ilqr_set_trajectory_params", "ilqr_set_reset_controls",
                   "does NOT re-evaluate", "ilqr_compute_derivatives first"):
        assert phrase in doc, phrase


def test_capi_binds_the_declared_argument_types():
    from ilqr_amd import capi
    assert capi.ABI_VERSION == 6
    for name, (_, argtypes) in DECLARED.items():
        assert name in capi.SYMBOLS, name
        res, args = capi.SYMBOLS[name]
        assert res is C.c_int and list(args) == argtypes, name
    assert (capi.WAS_CLONED, capi.CLONE_REFUSED) == (1, 2)


def test_library_exports_the_clone_calls():
    lib = _library()
    for name in DECLARED:
        assert hasattr(lib, name), name
    lib.ilqr_abi_version.restype = C.c_int
    assert lib.ilqr_abi_version() == 6


def test_a_null_handle_is_refused():
    lib = _library()
    for name, (_, argtypes) in DECLARED.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = C.c_int, argtypes
    one = (C.c_int * 1)(0)
    assert lib.ilqr_select_best(None, 1, one, None) == ERR_INVALID
    assert lib.ilqr_clone_trajectories(None, one, None, None) == ERR_INVALID
    assert lib.ilqr_clone_best(None, 1, None) == ERR_INVALID
    assert lib.ilqr_get_clone_flags(None, one) == ERR_INVALID
    assert lib.ilqr_copy_clone_flags_to_device(None, None) == ERR_INVALID


def test_batch_has_the_five_methods():
    from ilqr_amd import BatchILQR
    for name in ("select_best", "clone_trajectories", "clone_best", "clone_flags", "copy_clone_flags_to_device"):
        assert callable(getattr(BatchILQR, name, None)), name
