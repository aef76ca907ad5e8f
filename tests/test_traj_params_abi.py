"""Per-trajectory model parameters at the drop-in boundary, without a device: the four entry points are declared, bound and exported
by the stock library and by the builds that carry a user twin, the ABI version did not move, ilqr_trajectory_params_count() tells
which twin takes them, and a NULL handle is an invalid argument."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ilqr_trajectory_params_count", "ilqr_set_trajectory_params", "ilqr_get_trajectory_params", "ilqr_clear_trajectory_params")


def _chain():
    from ilqr_amd import _build, capi
    if not os.path.exists(_build.HIPCC) and not os.path.exists(_build.USER_CHAIN_LIB):
        pytest.skip("the pendulum-chain build is missing and there is no hipcc to make it")
    return capi.load(path=_build.build_user(_build.USER_CHAIN_HEADER, _build.USER_CHAIN_LIB))


def test_symbols_declared_bound_and_exported():
    from ilqr_amd import capi
    src = open(os.path.join(ROOT, "include", "ilqr_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = capi.load()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), "include/ilqr_amd.h does not declare %s" % n
        assert n in capi.SYMBOLS, n
        assert hasattr(lib, n), "libilqr_amd.so does not export %s" % n
    assert lib.ilqr_abi_version() == 6 == capi.ABI_VERSION  # additive: no new ABI version, ilqr_desc untouched


def test_count_tells_which_build_takes_them():
    from ilqr_amd import capi
    assert capi.load().ilqr_trajectory_params_count() == 0  # no user twin at all
    chain = _chain()
    for n in NEW:
        assert hasattr(chain, n), n
    assert chain.ilqr_trajectory_params_count() == 8 and chain.ilqr_abi_version() == 6


def test_a_twin_without_the_members_counts_zero():
    """examples/user_model_linear6.hpp declares neither NTP nor set_trajectory_params: detected, not required."""
    from ilqr_amd import _build, capi
    if not os.path.exists(_build.HIPCC) and not os.path.exists(_build.USER_EXAMPLE6_LIB):
        pytest.skip("the linear6 build is missing and there is no hipcc to make it")
    lib6 = capi.load(path=_build.build_user(_build.USER_EXAMPLE6_HEADER, _build.USER_EXAMPLE6_LIB))
    assert lib6.ilqr_has_user_model() == 1 and lib6.ilqr_trajectory_params_count() == 0


def test_null_handle_is_an_invalid_argument():
    from ilqr_amd import capi
    p = (C.c_double * 8)()
    for lib in (capi.load(), _chain()):
        assert lib.ilqr_set_trajectory_params(None, p, None, 8) == -1 and b"null handle" in lib.ilqr_last_error()
        assert lib.ilqr_get_trajectory_params(None, p, 8) == -1 and b"null handle" in lib.ilqr_last_error()
        assert lib.ilqr_clear_trajectory_params(None) == -1 and b"null handle" in lib.ilqr_last_error()


def test_python_layer_has_the_three_methods():
    from ilqr_amd import BatchILQR
    for n in ("set_trajectory_params", "trajectory_params", "clear_trajectory_params"):
        assert callable(getattr(BatchILQR, n))
