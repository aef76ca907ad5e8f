"""What ilqr_create refuses, on the real library and without a GPU: every refusal depends on the descriptor (and on the build's
user twin) alone and comes before any device is looked for (ilqr_amd/csrc/capi.hip, check_desc).  Each refusal's code and
message, and which one wins when a descriptor breaks several rules."""
import ctypes as C
import re

import numpy as np
import pytest

from ilqr_amd import _build, capi

INVALID, UNSUPPORTED = -1, -5
ARRAYS = ("u_min", "u_max", "goal", "lq_A", "lq_B", "lq_Q", "lq_R", "lq_Qf", "user_params")


def create(lib=None, **kw):
    """ilqr_create on a host-model descriptor (nx = 8, nu = 4, limits given) with the fields of kw replaced; arrays are sized
    from nx, nu; None leaves a pointer null.  Returns (code, message); a descriptor that is accepted is a failure here."""
    lib = capi.load(path=lib)
    f = dict(abi_version=capi.ABI_VERSION, model=capi.MODEL_HOST, nx=8, nu=4, T=5, B=4, dt=0.01, u_min=-1.0, u_max=1.0)
    f.update(kw)
    d, keep = capi.Desc(), []
    sizes = dict(u_min=f["nu"], u_max=f["nu"], goal=f["nx"], lq_A=f["nx"] ** 2, lq_B=f["nx"] * f["nu"], lq_Q=f["nx"] ** 2,
                 lq_R=f["nu"] ** 2, lq_Qf=f["nx"] ** 2, user_params=f.get("n_user_params", 0))
    for k, v in f.items():
        if k in ARRAYS:
            if v is None:
                continue
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (max(1, sizes[k]),)))
            keep.append(a)
            v = a.ctypes.data_as(C.POINTER(C.c_double))
        setattr(d, k, v)
    h = C.c_void_p()
    rc = lib.ilqr_create(C.byref(d), C.byref(h))
    assert rc != 0, "accepted: %s" % kw
    return rc, lib.ilqr_last_error().decode()


def lq(**kw):
    return dict(dict(model=capi.MODEL_LQ, lq_A=0.0, lq_B=0.0, lq_Q=1.0, lq_R=1.0, lq_Qf=1.0), **kw)


W2, TWO_TILES, DENSE_FD = capi.ROUTE_BACKWARD_W2, capi.ROUTE_TWO_CONTROL_TILES, capi.ROUTE_LQ_DENSE_FD
REGV, F32 = capi.FLAG_REGULARIZE_VXX, capi.DTYPE_F32

# every refusal of the stock library, in check_desc's order: (descriptor fields, code, message pattern)
REFUSALS = [
    (dict(abi_version=999), INVALID, r"^ABI version 999, library is 6 \(accepts 5 and 6\)$"),
    (dict(abi_version=4), INVALID, r"^ABI version 4, "),
    (dict(B=0), INVALID, r"^B, T, nx, nu must be positive$"),
    (dict(T=0), INVALID, r"^B, T, nx, nu must be positive$"),
    (dict(nx=0), INVALID, r"^B, T, nx, nu must be positive$"),
    (dict(nu=-1, u_min=None, u_max=None), INVALID, r"^B, T, nx, nu must be positive$"),
    (dict(nx=33), INVALID, r"^nx <= 32 and nu <= 32$"),
    (dict(nu=33), INVALID, r"^nx <= 32 and nu <= 32$"),
    (dict(dt=0.0), INVALID, r"^dt must be positive$"),
    (dict(route=128), UNSUPPORTED, r"^route bit 128 \(round 1's LDS kernel k_backward_w\) was retired in ABI 5"),
    (dict(model=capi.MODEL_DOUBLE_INTEGRATOR, nx=4, nu=2, route=capi.ROUTE_WIDE_TILES | capi.ROUTE_WIDE_TWO_PER_CU), UNSUPPORTED,
     r"^ILQR_ROUTE_WIDE_TWO_PER_CU: .* one tile per CU"),
    (dict(dtype=7), INVALID, r"^dtype 7: ILQR_DTYPE_F64 or ILQR_DTYPE_F32$"),
    (dict(nu=20, dtype=F32), UNSUPPORTED, r"^fp32 supports at most 16 controls \(nu = 20\)$"),
    (dict(nu=20, route=W2), UNSUPPORTED, r"^ILQR_ROUTE_BACKWARD_W2 supports at most 16 controls \(nu = 20\)$"),
    (dict(nu=20, route=DENSE_FD), UNSUPPORTED, r"^ILQR_ROUTE_LQ_DENSE_FD supports at most 16 controls \(nu = 20\)$"),
    (lq(nu=20, route=DENSE_FD), UNSUPPORTED, r"^ILQR_ROUTE_LQ_DENSE_FD supports at most 16 controls \(nu = 20\)$"),
    (dict(nu=20, flags=REGV), UNSUPPORTED, r"^ILQR_FLAG_REGULARIZE_VXX supports at most 16 controls \(nu = 20\)$"),
    (dict(route=TWO_TILES | W2), UNSUPPORTED, r"^ILQR_ROUTE_TWO_CONTROL_TILES and ILQR_ROUTE_BACKWARD_W2 name two different backward kernels$"),
    (dict(route=TWO_TILES, flags=REGV), UNSUPPORTED, r"^ILQR_FLAG_REGULARIZE_VXX is implemented in k_backward_w3 \(at most 16 controls\): drop ILQR_ROUTE_TWO_CONTROL_TILES$"),
    (dict(dtype=F32), UNSUPPORTED, r"^fp32 is not available for ILQR_MODEL_HOST: "),
    (lq(dtype=F32, route=W2), UNSUPPORTED, r"^fp32 is not available on ILQR_ROUTE_BACKWARD_W2 "),
    (lq(dtype=F32, route=TWO_TILES), UNSUPPORTED, r"^fp32 is not available on ILQR_ROUTE_TWO_CONTROL_TILES: "),
    (dict(model=capi.MODEL_ACROBOT, nx=4, nu=2), INVALID, r"^acrobot is nx=4 nu=1 \(include/acrobot.h:27-28\), got 4/2$"),
    (dict(model=capi.MODEL_DOUBLE_INTEGRATOR, nx=4, nu=1), INVALID, r"^double integrator is nx=4 nu=2 \(include/double_integrator.h:16-17\), got 4/1$"),
    (dict(u_min=None), INVALID, r"^generic handles need u_min/u_max "),
    (lq(u_max=None), INVALID, r"^generic handles need u_min/u_max "),
    (lq(lq_Qf=None), INVALID, r"^ILQR_MODEL_LQ needs lq_A, lq_B, lq_Q, lq_R, lq_Qf$"),
    (dict(model=capi.MODEL_USER, nx=4, nu=1), UNSUPPORTED, r"^model id 4 is not available in this build$"),
    (dict(model=99), UNSUPPORTED, r"^model id 99 is not available in this build$"),
    (dict(route=W2, flags=REGV), UNSUPPORTED, r"^ILQR_FLAG_REGULARIZE_VXX on the generic path is implemented in k_backward_w3: drop ILQR_ROUTE_BACKWARD_W2$"),
    (lq(route=W2, flags=REGV), UNSUPPORTED, r"^ILQR_FLAG_REGULARIZE_VXX on the generic path is implemented in k_backward_w3: "),
]

# descriptors that break two rules: the earlier check wins
ORDER = [
    (dict(abi_version=999, B=0), r"^ABI version"),
    (dict(nx=33, dt=0.0), r"^nx <= 32"),
    (dict(dt=-1.0, route=128), r"^dt must be positive"),
    (dict(route=128 | TWO_TILES | W2, dtype=7), r"^route bit 128"),
    (dict(model=capi.MODEL_DOUBLE_INTEGRATOR, nx=4, nu=2, route=capi.ROUTE_WIDE_TWO_PER_CU, dtype=7), r"^ILQR_ROUTE_WIDE_TWO_PER_CU"),
    (dict(nu=20, dtype=F32, route=W2 | DENSE_FD, flags=REGV), r"^fp32 supports at most 16"),
    (dict(nu=20, route=W2 | DENSE_FD, flags=REGV), r"^ILQR_ROUTE_BACKWARD_W2 supports at most 16"),
    (dict(nu=20, route=TWO_TILES | DENSE_FD), r"^ILQR_ROUTE_LQ_DENSE_FD supports at most 16"),
    (dict(route=TWO_TILES | W2, flags=REGV), r"^ILQR_ROUTE_TWO_CONTROL_TILES and ILQR_ROUTE_BACKWARD_W2"),
    (dict(route=TWO_TILES, flags=REGV, dtype=F32), r"^ILQR_FLAG_REGULARIZE_VXX is implemented in k_backward_w3 \(at most"),
    (dict(dtype=F32, route=W2, u_min=None), r"^fp32 is not available for ILQR_MODEL_HOST"),
    (lq(dtype=F32, route=W2, flags=REGV, lq_A=None), r"^fp32 is not available on ILQR_ROUTE_BACKWARD_W2"),
    (dict(model=capi.MODEL_ACROBOT, nx=4, nu=2, dtype=7), r"^dtype 7"),
    (dict(u_min=None, route=W2, flags=REGV), r"^generic handles need u_min/u_max"),
    (lq(lq_A=None, route=W2, flags=REGV), r"^ILQR_MODEL_LQ needs"),
    (dict(model=99, dtype=7), r"^dtype 7"),
]


def _check(res, code, pattern):
    rc, msg = res
    assert rc == code and re.search(pattern, msg), (rc, msg)


@pytest.mark.parametrize("fields,code,pattern", REFUSALS)
def test_each_refusal_has_its_code_and_message(fields, code, pattern):
    _check(create(**fields), code, pattern)


@pytest.mark.parametrize("fields,pattern", ORDER)
def test_the_earlier_refusal_wins(fields, pattern):
    rc, msg = create(**fields)
    assert rc in (INVALID, UNSUPPORTED) and re.search(pattern, msg), (rc, msg)


def test_null_arguments_and_batch_ilqr():
    lib = capi.load()
    h = C.c_void_p()
    assert lib.ilqr_create(None, C.byref(h)) == INVALID and lib.ilqr_last_error() == b"null argument"
    # through the Python front end: the same messages the GPU suite matches
    from ilqr_amd import BatchILQR
    with pytest.raises(capi.ILQRError, match="retired in ABI 5"):
        BatchILQR("host", 2, 5, 0.01, nx=6, nu=2, u_min=[-1, -1], u_max=[1, 1], route=128)
    with pytest.raises(capi.ILQRError, match=r"error -5: fp32 .*ILQR_MODEL_HOST"):
        BatchILQR("host", 4, 5, 0.01, nx=8, nu=5, dtype="f32", u_min=-np.ones(5), u_max=np.ones(5))


@pytest.fixture(scope="module")
def user_lib():
    return _build.build_user(_build.USER_EXAMPLE_HEADER, _build.USER_EXAMPLE_LIB)


@pytest.fixture(scope="module")
def user6_lib():
    return _build.build_user(_build.USER_EXAMPLE6_HEADER, _build.USER_EXAMPLE6_LIB)


def test_user_model_refusals(user_lib):
    """examples/user_model_acrobot.hpp: nx = 4, nu = 1, a tiled twin without analytic_record()."""
    user = dict(lib=user_lib, model=capi.MODEL_USER, nx=4, nu=1)
    _check(create(**dict(user, nu=2)), INVALID, r"^this build's user model is nx=4 nu=1, got 4/2$")
    _check(create(**dict(user, u_max=None)), INVALID, r"^ILQR_MODEL_USER needs u_min/u_max ")
    _check(create(**dict(user, flags=capi.FLAG_ANALYTIC_DERIVATIVES)), INVALID, r"^this user model has no analytic_record\(\)$")
    _check(create(**dict(user, n_user_params=-1)), INVALID, r"^ILQR_MODEL_USER: n_user_params = -1 with user_params = ")
    _check(create(**dict(user, n_user_params=3, user_params=None)), INVALID, r"^ILQR_MODEL_USER: n_user_params = 3 with user_params = ")
    # two at once: the earlier check wins
    _check(create(**dict(user, nu=2, u_min=None, flags=capi.FLAG_ANALYTIC_DERIVATIVES)), INVALID, r"^this build's user model")
    _check(create(**dict(user, u_min=None, flags=capi.FLAG_ANALYTIC_DERIVATIVES)), INVALID, r"^ILQR_MODEL_USER needs u_min/u_max")
    _check(create(**dict(user, flags=capi.FLAG_ANALYTIC_DERIVATIVES, n_user_params=-1)), INVALID, r"^this user model has no analytic_record")
    # a build with a user twin knows the other models, and the stock library's refusals are its refusals
    _check(create(lib=user_lib, model=99), UNSUPPORTED, r"^model id 99 is not available in this build$")
    _check(create(lib=user_lib, dtype=F32), UNSUPPORTED, r"^fp32 is not available for ILQR_MODEL_HOST: ")


def test_small_user_twin_on_the_generic_route_is_fp64_only(user6_lib):
    """examples/user_model_linear6.hpp (nx = 6, nu = 2): a small twin; ILQR_ROUTE_WAVE_PER_TRAJECTORY sends it to the generic kernels."""
    user = dict(lib=user6_lib, model=capi.MODEL_USER, nx=6, nu=2, n_user_params=0, route=capi.ROUTE_WAVE_PER_TRAJECTORY)
    _check(create(**dict(user, dtype=F32)), INVALID, r"^ILQR_ROUTE_WAVE_PER_TRAJECTORY on a small twin is the fp64 cross-check of its tiled kernels: fp64 only$")
    _check(create(**dict(user, dtype=F32, n_user_params=-1)), INVALID, r"fp64 only$")
    _check(create(**dict(user, route=capi.ROUTE_WAVE_PER_TRAJECTORY | W2, flags=REGV)), UNSUPPORTED, r"^ILQR_FLAG_REGULARIZE_VXX on the generic path")
