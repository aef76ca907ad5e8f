"""What the GPU test files of the stored-model queries share: a host getter stages its arrays through the handle's staging buffer
(ilqr_amd/csrc/staging.hpp), the device form of the same call writes to the caller's device pointers, and both run the same launch -- so
for the same request their results are equal bit for bit, whichever pointers are null and whatever the staging buffer held before."""
import ctypes as C

import numpy as np

DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
CASES = ["all", "last_only", "grow_then_reuse"]


B, T, DT = 3, 5, 0.02
ND, T0, NK = 2, 1, 3  # directions; the window of the calls that take one
WHICH = ["generic", "tiled"]


def handle(which):
    """A handle with a stored policy and non-trivial gains: the LQ model (nx = 6, nu = 3: the generic layout) or the acrobot (nx = 4, nu = 1:
    the tiled layout)."""
    from ilqr_amd import BatchILQR
    from tests.util import acrobot_x0
    rng = np.random.default_rng(5)
    if which == "generic":
        from tests.test_gpu_lq_end_to_end import dense_mats
        g, x0 = BatchILQR("lq", B, T, DT, lq=dense_mats(6, 3), u_min=-0.4, u_max=0.4), rng.uniform(-1, 1, (B, 6))
    else:
        g, x0 = BatchILQR("acrobot", B, T, DT, u_min=-1.5, u_max=1.5), acrobot_x0(B, scale=0.3, seed=4)
    g.init_traj(x0, rng.normal(size=(B, T, g.nu)) * 0.2)
    g.iterate(2)
    return g


def spd(rng, n, scale=1.0):
    """[B][n][n] symmetric positive definite"""
    M = rng.normal(size=(B, n, n)) / np.sqrt(n)
    return scale * (np.eye(n) + 0.5 * M @ np.swapaxes(M, -1, -2))


class Arg:
    """One pointer argument, in the call's order.  kind: "in" (an optional input: `value` is its array), "req" (a required input), "out" (a
    double output: `value` is its shape), "info" (the int output, [B])."""
    def __init__(self, name, kind, value):
        self.name, self.kind, self.value = name, kind, value


def _requests(args, needs_input):
    """(a) every pointer; (b) the smallest request the call accepts that ends in its last output: every optional input null -- but the last
    one where the call refuses a request without inputs --, every output null but the last double output -- and info with it: no call
    accepts info alone."""
    last_in = [a.name for a in args if a.kind == "in"][-1:] if needs_input else []
    last_out = [a.name for a in args if a.kind == "out"][-1]
    everything = {a.name for a in args}
    minimal = {a.name for a in args if a.kind in ("req", "info") or a.name in last_in or a.name == last_out}
    return everything, minimal


def _ask(g, host, device, scalars, args, given):
    """One request through both forms; the bytes of every output given must agree (bytes: a NaN equals itself)."""
    import torch
    h_ptrs, d_ptrs, pairs = [], [], []
    keep = []
    for a in args:
        if a.name not in given:
            h_ptrs.append(None)
            d_ptrs.append(None)
            continue
        if a.kind in ("in", "req"):
            arr = np.ascontiguousarray(a.value, dtype=np.float64)
            dev = torch.from_numpy(arr).cuda()
        elif a.kind == "out":
            arr = np.full(a.value, -7.0)
            dev = torch.full(tuple(a.value), -7.0, dtype=torch.float64, device="cuda")
            pairs.append((a.name, arr, dev))
        else:
            arr = np.full(a.value, -7, dtype=np.int32)
            dev = torch.full(tuple(a.value), -7, dtype=torch.int32, device="cuda")
            pairs.append((a.name, arr, dev))
        keep.append((arr, dev))
        h_ptrs.append(arr.ctypes.data_as(IP if a.kind == "info" else DP))
        d_ptrs.append(dev.data_ptr())
    torch.cuda.synchronize()  # (the copies and fills ran on torch's stream, the calls run on the handle's)
    assert getattr(g.lib, host)(g.h, *scalars, *h_ptrs) == 0, g.lib.ilqr_last_error()
    assert getattr(g.lib, device)(g.h, *scalars, *d_ptrs) == 0, g.lib.ilqr_last_error()
    g.synchronize()
    for name, arr, dev in pairs:
        got = dev.cpu().numpy()
        assert not np.all(arr == -7), (name, "the getter wrote nothing")
        assert arr.tobytes() == got.tobytes(), (name, sorted(given))


def check(make_handle, case, host, device, scalars, make_args, needs_input=False):
    """`case` of CASES on a fresh handle (its staging buffer is as small as the handle's own set-up left it): every pointer; the minimal
    request; the minimal one, then every pointer -- the buffer grows --, then the minimal one again in the buffer that is now too large."""
    g = make_handle()
    args = make_args(g)
    everything, minimal = _requests(args, needs_input)
    for given in {"all": [everything], "last_only": [minimal], "grow_then_reuse": [minimal, everything, minimal]}[case]:
        _ask(g, host, device, scalars, args, given)
    g.close()
