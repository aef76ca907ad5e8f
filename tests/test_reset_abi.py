"""The reset entry points exist in every layer that names them (no GPU): the built library exports them, include/ilqr_amd.h declares them,
ilqr_amd/capi.py binds them with the declared argument types, and they came without a new ABI version."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ilqr_amd.h")

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
# name -> the C parameter list of the issue, and its ctypes image
DECLARED = {
    "ilqr_set_reset_controls": ("ilqr_batch* h, const double* u0, const void* u0_device", [C.c_void_p, _dp, C.c_void_p]),
    "ilqr_reset_trajectories": ("ilqr_batch* h, const int* mask, const void* mask_device, int rules", [C.c_void_p, _ip, C.c_void_p, C.c_int]),
    "ilqr_mpc_step_reset": ("ilqr_batch* h, const double* x0, const void* x0_device, int shift, int tail, int n_iters, const int* mask, "
                            "const void* mask_device, int rules",
                            [C.c_void_p, _dp, C.c_void_p, C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, C.c_int]),
    "ilqr_get_reset_flags": ("ilqr_batch* h, int* flags", [C.c_void_p, _ip]),
    "ilqr_copy_reset_flags_to_device": ("ilqr_batch* h, void* flags_device", [C.c_void_p, C.c_void_p]),
}


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def test_header_declares_the_reset_calls_under_abi_6():
    text = open(HEADER).read()
    assert re.search(r"#define\s+ILQR_AMD_ABI_VERSION\s+6\b", text)
    for name, (params, _) in DECLARED.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        assert _norm(m.group(1)) == _norm(params), name
    assert re.search(r"enum\s+ilqr_reset_rule\s*\{\s*ILQR_RESET_NONFINITE\s*=\s*1\s*,\s*ILQR_RESET_LAMBDA_MAX\s*=\s*2\s*\}", text)
    assert re.search(r"enum\s+ilqr_reset_why\s*\{\s*ILQR_WAS_MASKED\s*=\s*1\s*,\s*ILQR_WAS_NONFINITE\s*=\s*2\s*,\s*ILQR_WAS_LAMBDA_MAX\s*=\s*4\s*\}", text)
    # the related fix: ilqr_mpc_step's comment says what happens to a rollout that is not finite, and where to go
    doc = text[text.index("/* One receding-horizon step"):text.index("int ilqr_mpc_step(")]
    assert "not finite" in doc and "ilqr_mpc_step_reset" in doc


def test_capi_binds_the_declared_argument_types():
    from ilqr_amd import capi
    assert capi.ABI_VERSION == 6
    for name, (_, argtypes) in DECLARED.items():
        assert name in capi.SYMBOLS, name
        res, args = capi.SYMBOLS[name]
        assert res is C.c_int and list(args) == argtypes, name
    assert (capi.RESET_NONFINITE, capi.RESET_LAMBDA_MAX) == (1, 2)
    assert (capi.WAS_MASKED, capi.WAS_NONFINITE, capi.WAS_LAMBDA_MAX) == (1, 2, 4)


def test_library_exports_the_reset_calls():
    from ilqr_amd import _build
    if not os.path.exists(_build.LIB) and not os.path.exists(_build.HIPCC):
        pytest.skip("no built library and no hipcc to build one")
    lib = C.CDLL(_build.build())  # (loading needs no device)
    for name in DECLARED:
        assert hasattr(lib, name), name
    lib.ilqr_abi_version.restype = C.c_int
    assert lib.ilqr_abi_version() == 6
