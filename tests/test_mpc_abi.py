"""CPU-side checks of the receding-horizon entry points of ABI 6 (include/ilqr_amd.h): exported, mirrored by ilqr_amd/capi.py, and
ilqr_create still takes a descriptor of ABI 5 (ilqr_desc did not change)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ilqr_shift_horizon", "ilqr_mpc_step", "ilqr_copy_controls_to_device")


def _header():
    src = open(os.path.join(ROOT, "include", "ilqr_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_new_symbols_are_exported_and_bound():
    from ilqr_amd import capi
    lib = capi.load()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, _header()), name
    assert lib.ilqr_abi_version() == capi.ABI_VERSION == 6


def test_tail_constants_match_the_header():
    from ilqr_amd import capi
    tails = {k: int(v) for k, v in re.findall(r"\b(ILQR_TAIL_[A-Z]+)\s*=\s*(\d+)", _header())}
    assert tails == {"ILQR_TAIL_HOLD": capi.TAIL_HOLD, "ILQR_TAIL_ZERO": capi.TAIL_ZERO}
    assert capi.TAIL_HOLD != capi.TAIL_ZERO


def test_abi_5_descriptor_passes_the_version_check():
    from ilqr_amd import capi
    lib = capi.load()
    d = capi.Desc()
    d.abi_version = 5
    d.model, d.nx, d.nu, d.T, d.B, d.dt = capi.MODEL_ACROBOT, 4, 1, 10, 4, 0.02
    h = C.c_void_p()
    rc = lib.ilqr_create(C.byref(d), C.byref(h))
    if rc == 0:
        lib.ilqr_destroy(h)
    else:
        assert b"ABI version" not in lib.ilqr_last_error(), lib.ilqr_last_error()
    d.abi_version = 4  # older descriptors are still refused
    assert lib.ilqr_create(C.byref(d), C.byref(h)) == -1
    assert b"ABI version" in lib.ilqr_last_error()


def test_null_handle_is_refused():
    from ilqr_amd import capi
    lib = capi.load()
    assert lib.ilqr_shift_horizon(None, 1, capi.TAIL_HOLD) == -1
    assert lib.ilqr_mpc_step(None, None, None, 1, capi.TAIL_HOLD, 1) == -1
    assert lib.ilqr_copy_controls_to_device(None, 0, 1, None) == -1
