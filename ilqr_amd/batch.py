"""BatchILQR -- numpy-facing host mirror of the reference's iLQR class for B trajectories.

Method names follow include/ilqr.h:28-107 (init_traj, generate_trajectory, its warm-start
overload) plus the stage calls and accessors the reference keeps private (tests reach them
through FRIEND_TEST there).  All arrays use the canonical layouts of include/ilqr_amd.h;
matrices are returned as [..., rows, cols] numpy arrays (transposed views of the column-major
memory), so K[b, t] is the nu x nx gain matrix and fx[b, t] the nx x nx Jacobian.
"""
import ctypes as C

import numpy as np

from . import capi

ALPHAS = np.array([1.0000, 0.5012, 0.2512, 0.1259, 0.0631, 0.0316, 0.0158, 0.0079, 0.0040,
                   0.0020, 0.0010])  # include/ilqr.h:24
STATUS_NAMES = {0: "running", 1: "converged_grad", 2: "converged_cost", 3: "lambda_max", 4: "max_iter"}
_MODELS = {"acrobot": (capi.MODEL_ACROBOT, 4, 1), "double_integrator": (capi.MODEL_DOUBLE_INTEGRATOR, 4, 2),
           "integrator": (capi.MODEL_DOUBLE_INTEGRATOR, 4, 2),
           # host-evaluated model: only the backward pass runs on the device (nx, nu given by the caller)
           "host": (capi.MODEL_HOST, None, None),
           # synthetic LQ model (BASELINE.json configs[4]): lq=(A, B, Q, R, Qf), row-major; nx, nu from their shapes
           "lq": (capi.MODEL_LQ, None, None),
           # the caller's own device twin, compiled into the library given by lib= (ilqr_amd._build.build_user); nx, nu by the caller
           "user": (capi.MODEL_USER, None, None)}
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _pi(a):
    return a.ctypes.data_as(_ip) if a is not None else None


class BatchILQR:
    def __init__(self, model, B, T, dt, u_min=None, u_max=None, goal=None, device=0, flags=0,
                 stream=None, params=None, nx=None, nu=None, lq=None, dtype="f64", lib=None, user_params=None, route=0, assume_cus=0):
        self.lib = capi.load(path=lib)
        self._check = lambda rc: capi.check(rc, self.lib)
        self._ctor = dict(model=model, B=B, T=T, dt=dt, u_min=u_min, u_max=u_max, goal=goal, device=device, flags=flags,
                          stream=stream, params=params, nx=nx, nu=nu, lq=lq, dtype=dtype, lib=lib, user_params=user_params,
                          route=route, assume_cus=assume_cus)
        mid, mnx, mnu = _MODELS[model]
        if lq is not None:
            lq = [_c(a) for a in lq]
            nx, nu = lq[1].shape
        nx, nu = (mnx or nx), (mnu or nu)
        self.model, self.nx, self.nu, self.B, self.T, self.dt = model, nx, nu, int(B), int(T), float(dt)
        self._keep = []
        d = capi.Desc()
        d.abi_version = capi.ABI_VERSION
        d.model, d.nx, d.nu, d.T, d.B, d.dt = mid, nx, nu, self.T, self.B, self.dt
        d.device, d.flags = device, flags
        d.route, d.assume_cus = int(route), int(assume_cus)  # enum ilqr_route: equivalent kernels (A/B runs, bit-identity tests)
        d.dtype = {"f64": capi.DTYPE_F64, "f32": capi.DTYPE_F32}[dtype]
        self.dtype = dtype
        for name, val, n in (("u_min", u_min, nu), ("u_max", u_max, nu), ("goal", goal, nx)):
            if val is not None:
                arr = _c(np.broadcast_to(np.asarray(val, dtype=np.float64), (n,)))
                self._keep.append(arr)
                setattr(d, name, _p(arr))
        if lq is not None:
            assert lq[0].shape == (nx, nx) and lq[2].shape == (nx, nx) and lq[3].shape == (nu, nu) and lq[4].shape == (nx, nx)
            self._keep.extend(lq)
            d.lq_A, d.lq_B, d.lq_Q, d.lq_R, d.lq_Qf = (_p(a) for a in lq)
        d.stream = stream
        if user_params is not None:
            up = _c(user_params).ravel()
            self._keep.append(up)
            d.user_params, d.n_user_params = _p(up), len(up)
        if params is not None:
            p = capi.Params()
            self.lib.ilqr_default_params(C.byref(p))
            for k, v in params.items():
                setattr(p, k, v)
            self._keep.append(p)
            d.params = C.pointer(p)
        self.h = C.c_void_p()
        self._check(self.lib.ilqr_create(C.byref(d), C.byref(self.h)))

    def clone(self):
        """A second, independent handle for the same problem description (own device memory and state)."""
        return BatchILQR(**self._ctor)

    def close(self):
        if getattr(self, "h", None):
            self.lib.ilqr_synchronize(self.h)
            for a in getattr(self, "_pinned", []):
                self.lib.ilqr_host_unregister(a.ctypes.data)
            self._pinned = []
            self.lib.ilqr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- solves (include/ilqr.h:49-54) ----
    def init_traj(self, x0, u0):
        x0, u0 = _c(x0), _c(u0)
        assert x0.shape == (self.B, self.nx) and u0.shape == (self.B, self.T, self.nu)
        cost = np.zeros(self.B)
        self._check(self.lib.ilqr_init_traj(self.h, _p(x0), _p(u0), _p(cost)))
        return cost

    def generate_trajectory(self, x0=None, u0=None):
        if x0 is not None and u0 is not None:
            x0, u0 = _c(x0), _c(u0)
            self._check(self.lib.ilqr_solve(self.h, _p(x0), _p(u0)))
        elif x0 is not None:
            x0 = _c(x0)
            self._check(self.lib.ilqr_warm_start(self.h, _p(x0)))
        else:
            self._check(self.lib.ilqr_generate_trajectory(self.h))

    solve = generate_trajectory  # BASELINE.json's "iLQR::solve()"

    def iterate(self, n=1):
        self._check(self.lib.ilqr_iterate(self.h, int(n)))

    def synchronize(self):
        self._check(self.lib.ilqr_synchronize(self.h))

    # ---- model-predictive control on the device (ilqr_shift_horizon, ilqr_mpc_step, ilqr_copy_controls_to_device) ----
    # Nothing below waits for the GPU.  Stream rule: a caller whose x0 is written, or whose controls are read, by torch passes
    # stream=torch.cuda.current_stream().cuda_stream at construction; torch's kernels and the solver's are then ordered by the stream
    # itself, without a host synchronisation.  torch's default stream is the null stream (0), and a handle given 0 makes a stream of its
    # own: run torch on a stream of its own (`with torch.cuda.stream(torch.cuda.Stream()):`) -- INTEGRATION.md, "MPC on the device".
    _TAILS = {"hold": capi.TAIL_HOLD, "zero": capi.TAIL_ZERO}

    def shift_horizon(self, shift, tail="hold"):
        """Move the stored nominal (xs, us, k, K) `shift` knots toward t = 0, in place.  tail="hold" repeats us[T-1] and K[T-1], "zero"
        zeros them; k's tail is zero and xs's is xs[T] under either (include/ilqr_amd.h, enum ilqr_tail)."""
        self._check(self.lib.ilqr_shift_horizon(self.h, int(shift), self._TAILS[tail]))

    def mpc_step(self, x0=None, x0_ptr=None, shift=1, iters=1, tail="hold", reset_mask=None, reset_mask_ptr=None, reset_nonfinite=False,
                 reset_lambda_max=False):
        """One receding-horizon step: shift_horizon(shift, tail), warm start from the new state, `iters` iterations.  x0: numpy [B][nx];
        x0_ptr: a raw device pointer to [B][nx] float64 on the handle's device (torch.Tensor.data_ptr()).  Exactly one of them.
        With one of the reset arguments (ilqr_mpc_step_reset): the trajectories the mask selects (reset_mask: [B], non-zero = reset;
        reset_mask_ptr: int32 [B] in device memory) start over from the reset controls after the shift; reset_lambda_max: also those the
        previous step left at status lambda_max; reset_nonfinite: also those whose warm rollout is not finite, which are rolled out again.
        reset_flags() says who and why.  Without them the call is ilqr_mpc_step."""
        if (x0 is None) == (x0_ptr is None):
            raise ValueError("mpc_step: exactly one of x0 and x0_ptr")
        if x0 is not None:
            x0 = _c(x0)
            assert x0.shape == (self.B, self.nx)
        if reset_mask is None and reset_mask_ptr is None and not reset_nonfinite and not reset_lambda_max:
            self._check(self.lib.ilqr_mpc_step(self.h, _p(x0), x0_ptr, int(shift), self._TAILS[tail], int(iters)))
            return
        mask = self._mask(reset_mask)
        self._check(self.lib.ilqr_mpc_step_reset(self.h, _p(x0), x0_ptr, int(shift), self._TAILS[tail], int(iters), _pi(mask), reset_mask_ptr,
                                                 self._rules(reset_nonfinite, reset_lambda_max)))

    # ---- single trajectories start over (ilqr_set_reset_controls, ilqr_reset_trajectories, ilqr_get_reset_flags) ----
    def _mask(self, mask):
        if mask is None:
            return None
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.int32)
        if mask.shape != (self.B,):
            raise ValueError("reset mask must be [B], got %s" % (mask.shape,))
        return mask

    @staticmethod
    def _rules(nonfinite, lambda_max):
        return (capi.RESET_NONFINITE if nonfinite else 0) | (capi.RESET_LAMBDA_MAX if lambda_max else 0)

    def set_reset_controls(self, u0=None, ptr=None):
        """The controls a reset trajectory starts from: u0 numpy [B][T][nu], or ptr, a raw device pointer to float64 [B][T][nu]; neither =
        back to zeros (the default).  Enqueued on the handle's stream."""
        if u0 is not None:
            u0 = _c(u0)
            if u0.shape != (self.B, self.T, self.nu):
                raise ValueError("set_reset_controls: u0 must be [B][T][nu], got %s" % (u0.shape,))
        self._check(self.lib.ilqr_set_reset_controls(self.h, _p(u0), ptr))

    def reset_trajectories(self, mask=None, mask_ptr=None, nonfinite=False, lambda_max=False):
        """Reset now, outside a step: the trajectories the mask selects ([B] numpy, or int32 [B] in device memory), with nonfinite those
        whose cost is NaN or inf, with lambda_max those at status lambda_max (include/ilqr_amd.h: what a reset is).  Enqueued."""
        mask = self._mask(mask)
        self._check(self.lib.ilqr_reset_trajectories(self.h, _pi(mask), mask_ptr, self._rules(nonfinite, lambda_max)))

    def reset_flags(self):
        """Why the last mpc_step with resets / reset_trajectories reset each trajectory: int32 [B], bits capi.WAS_MASKED, WAS_NONFINITE,
        WAS_LAMBDA_MAX, 0 = it was not (synchronises)."""
        flags = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.ilqr_get_reset_flags(self.h, flags.ctypes.data_as(_ip)))
        return flags

    def copy_reset_flags_to_device(self, ptr):
        """The same flags as int32 [B] into caller-owned device memory `ptr` (raw pointer); enqueued on the handle's stream."""
        self._check(self.lib.ilqr_copy_reset_flags_to_device(self.h, ptr))

    # ---- multi-start groups (ilqr_select_best, ilqr_clone_trajectories, ilqr_clone_best, ilqr_get_clone_flags) ----
    def select_best(self, group, ptr=None):
        """The winner of every group of `group` consecutive trajectories (the lowest finite cost; ties: the lowest index; a group without a
        finite cost: everyone itself) as a map: returns int32 [B] (synchronises), or with ptr -- a raw device pointer to int32 [B] --
        writes it there, enqueued on the handle's stream, and returns None.  Reads the costs only."""
        if ptr is not None:
            self._check(self.lib.ilqr_select_best(self.h, int(group), None, ptr))
            return None
        src = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.ilqr_select_best(self.h, int(group), _pi(src), None))
        return src

    def clone_trajectories(self, src=None, src_ptr=None, du_ptr=None):
        """Trajectory b takes the state of trajectory src[b] (include/ilqr_amd.h: what a clone is, and the source rule: a source keeps
        itself).  src: int [B] numpy; src_ptr: int32 [B] in device memory.  Exactly one of them.  du_ptr: float64 [B][T][nu] in device
        memory, added to the controls of the cloned trajectories (their cost is not re-evaluated: mpc_step next).  Enqueued."""
        if (src is None) == (src_ptr is None):
            raise ValueError("clone_trajectories: exactly one of src and src_ptr")
        if src is not None:
            src = np.ascontiguousarray(src, dtype=np.int32)
            if src.shape != (self.B,):
                raise ValueError("clone_trajectories: src must be [B], got %s" % (src.shape,))
        self._check(self.lib.ilqr_clone_trajectories(self.h, _pi(src), src_ptr, du_ptr))

    def clone_best(self, group, du_ptr=None):
        """select_best(group) into a buffer of the handle, then clone_trajectories by it: every group becomes copies of its best member
        (plus du).  Enqueued on the handle's stream, nothing waited for."""
        self._check(self.lib.ilqr_clone_best(self.h, int(group), du_ptr))

    def clone_flags(self):
        """What the last clone call did to each trajectory: int32 [B], capi.WAS_CLONED, capi.CLONE_REFUSED or 0 (synchronises)."""
        flags = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.ilqr_get_clone_flags(self.h, flags.ctypes.data_as(_ip)))
        return flags

    def copy_clone_flags_to_device(self, ptr):
        """The same flags as int32 [B] into caller-owned device memory `ptr` (raw pointer); enqueued on the handle's stream."""
        self._check(self.lib.ilqr_copy_clone_flags_to_device(self.h, ptr))

    def copy_controls_to_device(self, t0, n, ptr):
        """us[:, t0 : t0 + n, :] as float64 [B][n][nu] into caller-owned device memory `ptr` (raw pointer); enqueued on the handle's stream."""
        self._check(self.lib.ilqr_copy_controls_to_device(self.h, int(t0), int(n), ptr))

    # ---- per-trajectory model parameters (user twins with NTP / set_trajectory_params on the generic kernels) ----
    def set_trajectory_params(self, p=None, ptr=None):
        """Row b = the model parameters of trajectory b for every later rollout, sweep and mpc_step.  p: numpy [B][NTP]; ptr: a raw
        device pointer to [B][NTP] float64 on the handle's device (torch.Tensor.data_ptr()).  Exactly one of them.  Enqueued on the
        handle's stream (the stream rule above); the stored cost is not re-evaluated -- warm-start or mpc_step next."""
        if (p is None) == (ptr is None):
            raise ValueError("set_trajectory_params: exactly one of p and ptr")
        n = self.lib.ilqr_trajectory_params_count()
        if p is not None:
            p = _c(p)
            if p.ndim != 2 or p.shape[0] != self.B:
                raise ValueError("set_trajectory_params: p must be [B][NTP], got %s" % (p.shape,))
            n = p.shape[1]
        self._check(self.lib.ilqr_set_trajectory_params(self.h, _p(p), ptr, int(n)))

    def trajectory_params(self):
        """The rows set_trajectory_params stored, [B][NTP] (synchronises)."""
        n = self.lib.ilqr_trajectory_params_count()
        p = np.zeros((self.B, max(n, 1)))
        self._check(self.lib.ilqr_get_trajectory_params(self.h, _p(p), int(n)))
        return p

    def clear_trajectory_params(self):
        """Every trajectory back to the handle-wide parameters of the constructor (per-trajectory rows and per-knot rows alike)."""
        self._check(self.lib.ilqr_clear_trajectory_params(self.h))

    def set_knot_params(self, p=None, ptr=None, n_knots=None, k0=0):
        """Per-knot model parameters: the handle takes the window of T + 1 rows starting at row k0 of a reference [B][n_knots][NTP] -- row
        t of the handle is reference row min(k0 + t, n_knots - 1) -- and evaluates knot t of trajectory b under row (b, t) in every later
        rollout, sweep and mpc_step.  p: numpy [B][n_knots][NTP]; ptr: a raw device pointer to such an array of float64 on the handle's
        device (torch.Tensor.data_ptr()), with n_knots given.  Exactly one of them.  Enqueued on the handle's stream (the stream rule
        above); the stored cost is not re-evaluated -- warm-start or mpc_step next.  set_trajectory_params switches back to one row per
        trajectory, clear_trajectory_params to none."""
        if (p is None) == (ptr is None):
            raise ValueError("set_knot_params: exactly one of p and ptr")
        n = self.lib.ilqr_trajectory_params_count()
        if p is not None:
            p = _c(p)
            if p.ndim != 3 or p.shape[0] != self.B or (n_knots is not None and int(n_knots) != p.shape[1]):
                raise ValueError("set_knot_params: p must be [B][n_knots][NTP], got %s" % (p.shape,))
            n_knots, n = p.shape[1], p.shape[2]
        elif n_knots is None:
            raise ValueError("set_knot_params: ptr needs n_knots")
        self._check(self.lib.ilqr_set_knot_params(self.h, _p(p), ptr, int(n), int(n_knots), int(k0)))

    def knot_params(self):
        """The handle's window of per-knot rows as the kernels see them, [B][T+1][NTP] (synchronises)."""
        n = self.lib.ilqr_trajectory_params_count()
        p = np.zeros((self.B, self.T + 1, max(n, 1)))
        self._check(self.lib.ilqr_get_knot_params(self.h, _p(p), int(n)))
        return p

    def param_gradient(self, dxs=None, dus=None, dlam=None, eps_p=0.0, want_lam=False):
        """dL/dp, the gradient of the caller's loss in the rows of set_trajectory_params (include/ilqr_amd.h, ilqr_get_param_gradient), from
        what lq_solve(gx=dL/dxs, gu=dL/dus, dlam=True) returned: dxs, dlam [B][T+1][S][nx], dus [B][T][S][nu] (None = zero, not all three;
        dlam[:, 0] is not read).  Returns gp [B][S][NTP], with want_lam (gp, lam [B][T+1][nx]), lam the nominal costate of the records.
        Inputs without the direction axis are one direction and the axis is dropped again on output.  eps_p: the relative parameter step
        (0 = 1e-3).  The gradient through the records' LQ model: exact for dynamics linear in (x, u), Gauss-Newton otherwise.  Synchronises."""
        X = self._dirs_input(dxs, (self.T + 1,), self.nx, "dxs")
        U = self._dirs_input(dus, (self.T,), self.nu, "dus")
        Lm = self._dirs_input(dlam, (self.T + 1,), self.nx, "dlam")
        given = [a for a in (X, U, Lm) if a[0] is not None]
        if not given:
            raise ValueError("dxs, dus and dlam are all None: the answer would be zero")
        S, flat = given[0][1], given[0][2]
        if any(a[1] != S or a[2] != flat for a in given):
            raise ValueError("dxs, dus and dlam disagree on the directions: %s" % [a[0].shape for a in given])
        gp = np.zeros((self.B, S, max(self.lib.ilqr_trajectory_params_count(), 1)))
        lam = np.zeros((self.B, self.T + 1, self.nx)) if want_lam else None
        self._check(self.lib.ilqr_get_param_gradient(self.h, S, 0, float(eps_p), _p(X[0]), _p(U[0]), _p(Lm[0]), _p(gp), _p(lam)))
        if flat:
            gp = gp[:, 0]
        return (gp, lam) if want_lam else gp

    def param_gradient_on_device(self, S, dxs=None, dus=None, dlam=None, gp=None, lam=None, eps_p=0.0):
        """ilqr_param_gradient_on_device: float64 dxs, dlam [B][T+1][S][nx], dus [B][T][S][nu] (None = zero, not all three), gp [B][S][NTP],
        lam [B][T+1][nx] (either may be None, not both) in device memory, each a torch tensor (contiguous float64 on the handle's device)
        or a raw pointer.  Enqueued on the handle's stream, nothing waited for."""
        ptr = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a
        self._check(self.lib.ilqr_param_gradient_on_device(self.h, int(S), 0, float(eps_p), ptr(dxs), ptr(dus), ptr(dlam), ptr(gp), ptr(lam)))

    # ---- stages ----
    def compute_derivatives(self):
        self._check(self.lib.ilqr_compute_derivatives(self.h))

    def backward_pass(self):
        div = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.ilqr_backward_pass(self.h, div.ctypes.data_as(_ip)))
        return div

    def backward_step(self):
        self._check(self.lib.ilqr_backward_step(self.h))

    def rollout_candidates(self):
        cost = np.zeros((self.B, len(ALPHAS)))
        self._check(self.lib.ilqr_rollout_candidates(self.h, _p(cost)))
        return cost

    def line_search(self):
        self._check(self.lib.ilqr_line_search(self.h))

    def accept_candidates(self, cost_c):
        """Host-evaluated models: STEP 3/4 on the caller's candidate costs cost_c [B][11]; returns the accepted alpha index per
        trajectory (-1 = none; the caller then stores that rollout with set_trajectory)."""
        cost_c = _c(cost_c)
        assert cost_c.shape == (self.B, len(ALPHAS))
        acc = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.ilqr_accept_candidates(self.h, _p(cost_c), acc.ctypes.data_as(_ip)))
        return acc

    def reset_state(self, warm=False):
        """warm=False: the non-rollout part of init_traj; warm=True: a new outer loop on the stored
        solution (status / iteration count / flgChange restart, lambda and gains persist)."""
        self._check(self.lib.ilqr_reset_state(self.h, int(bool(warm))))

    # ---- setters (canonical layouts; matrices given as [..., rows, cols]) ----
    def set_trajectory(self, x0=None, xs=None, us=None, cost=None):
        a = [None if v is None else _c(v) for v in (x0, xs, us, cost)]
        self._check(self.lib.ilqr_set_trajectory(self.h, *[_p(v) for v in a]))

    def set_gains(self, k=None, K=None):
        k = None if k is None else _c(k)
        K = None if K is None else _c(np.swapaxes(np.asarray(K), -1, -2))
        self._check(self.lib.ilqr_set_gains(self.h, _p(k), _p(K)))

    def set_derivatives(self, **d):
        """fx, fu, cx, cu, cxx, cxu, cuu as [B][T+1][rows][cols] (vectors [B][T+1][n])."""
        order = ("fx", "fu", "cx", "cu", "cxx", "cxu", "cuu")
        arrs = []
        for name in order:
            v = d.get(name)
            if v is None:
                arrs.append(None)
            elif name in ("cx", "cu"):
                arrs.append(_c(v))
            else:
                arrs.append(_c(np.swapaxes(np.asarray(v), -1, -2)))
        self._check(self.lib.ilqr_set_derivatives(self.h, *[_p(v) for v in arrs]))

    def set_lambda(self, lam=None, dlam=None):
        lam = None if lam is None else _c(np.broadcast_to(lam, (self.B,)))
        dlam = None if dlam is None else _c(np.broadcast_to(dlam, (self.B,)))
        self._check(self.lib.ilqr_set_lambda(self.h, _p(lam), _p(dlam)))

    # ---- getters ----
    def trajectory(self, out=None):
        """xs [B][T+1][nx], us [B][T][nu].  `out=(xs, us)`: C-contiguous float64 arrays to fill -- a
        caller that keeps its result arrays across solves avoids the first-touch page faults of fresh
        ones, which cost several times the PCIe transfer itself (PCIe-inclusive)."""
        if out is None:
            xs = np.zeros((self.B, self.T + 1, self.nx))
            us = np.zeros((self.B, self.T, self.nu))
        else:
            xs, us = out
            for a, shape in ((xs, (self.B, self.T + 1, self.nx)), (us, (self.B, self.T, self.nu))):
                if a.shape != shape or a.dtype != np.float64 or not a.flags.c_contiguous:
                    raise ValueError("out arrays must be C-contiguous float64 of shape %s" % (shape,))
        self._check(self.lib.ilqr_get_trajectory(self.h, _p(xs), _p(us)))
        return xs, us

    def gains(self):
        k = np.zeros((self.B, self.T, self.nu))
        K = np.zeros((self.B, self.T, self.nx, self.nu))  # memory: column-major nu x nx
        self._check(self.lib.ilqr_get_gains(self.h, _p(k), _p(K)))
        return k, np.swapaxes(K, -1, -2)

    def result_buffers(self, pinned=True, K=True):
        """Result arrays a caller keeps across solves, in the ABI's memory layouts: dict(xs, us, k, K, cost) (K [B][T][nx][nu] in memory =
        column-major nu x nx per knot; K=False: without the gains).  pinned: page-locked with ilqr_host_register, so that results_async's
        copies are DMA transfers that the call does not wait for."""
        bufs = dict(xs=np.zeros((self.B, self.T + 1, self.nx)), us=np.zeros((self.B, self.T, self.nu)), cost=np.zeros(self.B))
        if K:
            bufs.update(k=np.zeros((self.B, self.T, self.nu)), K=np.zeros((self.B, self.T, self.nx, self.nu)))
        if pinned:
            for a in bufs.values():
                self._check(self.lib.ilqr_host_register(a.ctypes.data, a.nbytes))
            self._pinned = getattr(self, "_pinned", []) + [a for a in bufs.values()]
        return bufs

    def results_async(self, bufs):
        """ilqr_get_results_async into `bufs` (result_buffers()): every array in one call, nothing waited for -- valid after synchronize()."""
        self._check(self.lib.ilqr_get_results_async(self.h, _p(bufs.get("xs")), _p(bufs.get("us")), _p(bufs.get("k")), _p(bufs.get("K")), _p(bufs.get("cost"))))

    def copy_trajectory_to_device(self, xs_ptr=None, us_ptr=None):
        """canonical xs [B][T+1][nx] / us [B][T][nu] (double) into caller-owned device memory (raw pointers, e.g. torch.Tensor.data_ptr());
        enqueued on the handle's stream."""
        self._check(self.lib.ilqr_copy_trajectory_to_device(self.h, xs_ptr, us_ptr))

    def copy_gains_to_device(self, k_ptr=None, K_ptr=None):
        self._check(self.lib.ilqr_copy_gains_to_device(self.h, k_ptr, K_ptr))

    def value(self, t0=0, n=None):
        """The value model of the stored policy over the knots [t0, t0 + n) (n=None: up to knot T): Vx [B][n][nx], Vxx [B][n][nx][nx]
        (include/ilqr_amd.h, ilqr_get_value: recomputed on the device from the current records and the stored gains; synchronises)."""
        n = self.T + 1 - int(t0) if n is None else int(n)
        Vx = np.zeros((self.B, max(n, 0), self.nx))
        Vxx = np.zeros((self.B, max(n, 0), self.nx, self.nx))  # memory: column-major nx x nx
        self._check(self.lib.ilqr_get_value(self.h, int(t0), n, _p(Vx), _p(Vxx)))
        return Vx, np.swapaxes(Vxx, -1, -2)

    def copy_value_to_device(self, t0, n, Vx_ptr=None, Vxx_ptr=None):
        """The same window as float64 [B][n][nx] / [B][n][nx*nx] (column-major per knot) into caller-owned device memory (raw pointers,
        e.g. torch.Tensor.data_ptr(); either may be None); enqueued on the handle's stream, nothing waited for."""
        self._check(self.lib.ilqr_copy_value_to_device(self.h, int(t0), int(n), Vx_ptr, Vxx_ptr))

    def evaluate_policy(self, x, t0=0, n=None, clamp=False):
        """The stored feedback policy u = us[t] + K[t](x - xs[t]) applied to the caller's states at knot t0 and rolled through the device
        model for n knots (n=None: up to knot T).  x: [B][S][nx], S samples per trajectory, or [B][nx] (S = 1).  Returns dict(cost [B][S],
        x_end [B][S][nx], u_first [B][S][nu]) -- [B], [B][nx], [B][nu] for a [B][nx] input.  The running costs of the window, plus the
        final cost when it ends at knot T; clamp: controls clamped to the limits (always on a handle with FLAG_REFERENCE_FIXES).  A
        read-only query: the handle's trajectory, cost and solver state stay as they are (include/ilqr_amd.h, ilqr_evaluate_policy;
        synchronises)."""
        x = _c(x)
        flat = x.ndim == 2
        if flat:
            x = x[:, None, :]
        if x.ndim != 3 or x.shape[0] != self.B or x.shape[2] != self.nx:
            raise ValueError("evaluate_policy: x must be [B][S][nx] or [B][nx], got %s" % (x.shape,))
        S = x.shape[1]
        n = self.T - int(t0) if n is None else int(n)
        cost, x_end, u_first = np.zeros((self.B, S)), np.zeros((self.B, S, self.nx)), np.zeros((self.B, S, self.nu))
        self._check(self.lib.ilqr_evaluate_policy(self.h, int(t0), n, S, capi.EVAL_CLAMP if clamp else 0, _p(x), _p(cost), _p(x_end), _p(u_first)))
        if flat:
            cost, x_end, u_first = cost[:, 0], x_end[:, 0], u_first[:, 0]
        return dict(cost=cost, x_end=x_end, u_first=u_first)

    def evaluate_policy_on_device(self, t0, n, S, x_ptr, cost_ptr=None, x_end_ptr=None, u_first_ptr=None, clamp=False):
        """The same with raw device pointers (torch.Tensor.data_ptr()) to float64 x [B][S][nx], cost [B][S], x_end [B][S][nx], u_first
        [B][S][nu] on the handle's device; any output may be None, not all three.  Enqueued on the handle's stream, nothing waited for
        (the stream rule above): x_end of n = shift is the next mpc_step's x0_ptr."""
        self._check(self.lib.ilqr_evaluate_policy_on_device(self.h, int(t0), int(n), int(S), capi.EVAL_CLAMP if clamp else 0, x_ptr, cost_ptr,
                                                            x_end_ptr, u_first_ptr))

    def _cov_input(self, M):
        """[B][nx][nx] or one (nx, nx) matrix for all -> canonical [B][nx*nx], column-major per matrix (None stays None)."""
        if M is None:
            return None
        M = np.broadcast_to(np.asarray(M, dtype=np.float64), (self.B, self.nx, self.nx))
        return np.ascontiguousarray(np.swapaxes(M, -1, -2))

    def covariance(self, Sigma0=None, W=None, t0=0, n=None, Su=False, expected_cost=False):
        """The state covariance of the linearised closed loop x[t+1] - xs[t+1] = (fx + fu K)(x[t] - xs[t]) + w, w ~ (0, W), from
        x[0] - xs[0] ~ (0, Sigma0), over the knots [t0, t0 + n) (n=None: up to knot T, up to knot T - 1 with Su): Sigma [B][n][nx][nx].
        Sigma0, W: [B][nx][nx] or one (nx, nx) matrix for all; None = zero.  Su=True: also the covariance of the feedback controls,
        [B][n][nu][nu]; expected_cost=True: also the expected cost above the nominal's, [B].  Returns Sigma alone, or the tuple
        (Sigma, Su, expected_cost) without the members not asked for (include/ilqr_amd.h, ilqr_get_covariance: recomputed on the device
        from the current records and the stored gains; synchronises)."""
        n = self.T + (0 if Su else 1) - int(t0) if n is None else int(n)
        S0, Wc = self._cov_input(Sigma0), self._cov_input(W)
        Sg = np.zeros((self.B, max(n, 0), self.nx, self.nx))  # memory: column-major nx x nx
        U = np.zeros((self.B, max(n, 0), self.nu, self.nu)) if Su else None
        J = np.zeros(self.B) if expected_cost else None
        self._check(self.lib.ilqr_get_covariance(self.h, int(t0), n, _p(S0), _p(Wc), _p(Sg), _p(U), _p(J)))
        out = [np.swapaxes(Sg, -1, -2)] + ([np.swapaxes(U, -1, -2)] if Su else []) + ([J] if expected_cost else [])
        return out[0] if len(out) == 1 else tuple(out)

    def copy_covariance_to_device(self, t0, n, Sigma0_ptr=None, W_ptr=None, Sigma_ptr=None, Su_ptr=None, expected_cost_ptr=None):
        """The same with raw device pointers (e.g. torch.Tensor.data_ptr()) to float64 Sigma0, W [B][nx*nx] (None = zero), Sigma
        [B][n][nx*nx], Su [B][n][nu*nu] (column-major per matrix), expected_cost [B]; any output may be None, not all three.  Enqueued on
        the handle's stream, nothing waited for."""
        self._check(self.lib.ilqr_copy_covariance_to_device(self.h, int(t0), int(n), Sigma0_ptr, W_ptr, Sigma_ptr, Su_ptr, expected_cost_ptr))

    def _mat_input(self, M, rows, cols):
        """[B][rows][cols] or one (rows, cols) matrix for all -> canonical [B][rows*cols], column-major per matrix (None stays None)."""
        if M is None:
            return None
        M = np.broadcast_to(np.asarray(M, dtype=np.float64), (self.B, rows, cols))
        return np.ascontiguousarray(np.swapaxes(M, -1, -2))

    def estimator(self, H, P0=None, W=None, V=None, t0=0, n_knots=None, Pf=True, L=True, Pp=False, Sigma=False, Su=False, expected_cost=False,
                  info=False):
        """The Kalman filter of the stored linearisation for the measurement y = H x + v, v ~ (0, V), process noise W and prior covariance
        P0, and the covariance of the loop u = us[t] + K[t](xhat[t] - xs[t]) that feeds back on its estimate, over the knots
        [t0, t0 + n_knots) (n_knots=None: up to knot T, up to knot T - 1 with Su).  H: [B][ny][nx], V: [B][ny][ny], P0, W: [B][nx][nx], or
        one matrix for all; P0, W None = zero.  Returns a dict with the members asked for: Pp, Pf, Sigma [B][n_knots][nx][nx] (the
        estimate-error covariance before and after the knot's measurement; the covariance of x - xs), L [B][n_knots][nx][ny] (the Kalman
        gains), Su [B][n_knots][nu][nu], expected_cost [B], info int32 [B] (0, or the knot of a failed factorisation + 1: that
        trajectory's outputs are NaN).  include/ilqr_amd.h, ilqr_get_estimator: recomputed on the device from the current records and the
        stored gains; synchronises."""
        if H is None or V is None:
            raise ValueError("estimator: H and V are required")
        H = np.asarray(H, dtype=np.float64)
        if H.ndim not in (2, 3) or H.shape[-1] != self.nx:
            raise ValueError("estimator: H must be [B][ny][nx] or (ny, nx), got %s" % (H.shape,))
        ny = int(H.shape[-2])
        n = self.T + (0 if Su else 1) - int(t0) if n_knots is None else int(n_knots)
        nk = max(n, 0)
        Hc, Vc = self._mat_input(H, ny, self.nx), self._mat_input(V, ny, ny)
        P0c, Wc = self._cov_input(P0), self._cov_input(W)
        nn = lambda want: np.zeros((self.B, nk, self.nx, self.nx)) if want else None  # memory: column-major nx x nx
        o = dict(Pp=nn(Pp), Pf=nn(Pf), L=np.zeros((self.B, nk, ny, self.nx)) if L else None, Sigma=nn(Sigma),
                 Su=np.zeros((self.B, nk, self.nu, self.nu)) if Su else None, expected_cost=np.zeros(self.B) if expected_cost else None)
        flags = np.zeros(self.B, dtype=np.int32) if info else None
        self._check(self.lib.ilqr_get_estimator(self.h, int(t0), n, ny, _p(Hc), _p(P0c), _p(Wc), _p(Vc), _p(o["Pp"]), _p(o["Pf"]), _p(o["L"]),
                                                _p(o["Sigma"]), _p(o["Su"]), _p(o["expected_cost"]), _pi(flags)))
        out = {name: (a if name == "expected_cost" else np.swapaxes(a, -1, -2)) for name, a in o.items() if a is not None}
        if info:
            out["info"] = flags
        return out

    def copy_estimator_to_device(self, t0, n_knots, ny, H_ptr, V_ptr, P0_ptr=None, W_ptr=None, Pp_ptr=None, Pf_ptr=None, L_ptr=None, Sigma_ptr=None,
                                 Su_ptr=None, expected_cost_ptr=None, info_ptr=None):
        """The same with raw device pointers (e.g. torch.Tensor.data_ptr()) to float64 H [B][ny*nx], V [B][ny*ny], P0, W [B][nx*nx] (None =
        zero), Pp, Pf, Sigma [B][n_knots][nx*nx], L [B][n_knots][nx*ny], Su [B][n_knots][nu*nu] (column-major per matrix), expected_cost [B]
        and int32 info [B]; any output may be None, not all of the first six.  Enqueued on the handle's stream, nothing waited for."""
        self._check(self.lib.ilqr_copy_estimator_to_device(self.h, int(t0), int(n_knots), int(ny), H_ptr, P0_ptr, W_ptr, V_ptr, Pp_ptr, Pf_ptr, L_ptr,
                                                           Sigma_ptr, Su_ptr, expected_cost_ptr, info_ptr))

    def risk_sensitive(self, C, theta, mu=0.0, hold_clamped=False, K=True, k=True, Vx=False, Vxx=False, risk_cost=False, info=False):
        """The risk-sensitive (LEQG) gains and value of the LQ model the records hold, for the noise dx[t+1] += C xi, xi ~ N(0, I):
        (K, k) minimise (1/theta) log E exp(theta J).  C: [B][nx][nw] or one (nx, nw) matrix for all, 1 <= nw <= nx (W = C C' is
        covariance()'s process noise); theta > 0 risk-averse, < 0 risk-seeking, 0 the gains solve_lq computes.  mu, hold_clamped: as
        solve_lq.  Returns a dict with the members asked for: K [B][T][nu][nx], k [B][T][nu] (what set_gains takes), Vx [B][T+1][nx],
        Vxx [B][T+1][nx][nx], risk_cost [B], info int32 [B] (0; -(knot + 1): breakdown, the risk-sensitive cost at this theta is
        infinite; knot + 1: Quu is not positive definite on the free controls; either way that trajectory's outputs are NaN).
        include/ilqr_amd.h, ilqr_get_risk_sensitive: recomputed on the device from the current records; synchronises."""
        if C is None:
            raise ValueError("risk_sensitive: C is required")
        C = np.asarray(C, dtype=np.float64)
        if C.ndim not in (2, 3) or C.shape[-2] != self.nx:
            raise ValueError("risk_sensitive: C must be [B][nx][nw] or (nx, nw), got %s" % (C.shape,))
        nw = int(C.shape[-1])
        Cc = self._mat_input(C, self.nx, nw)
        B, T, n, m = self.B, self.T, self.nx, self.nu
        o = dict(K=np.zeros((B, T, n, m)) if K else None,  # memory: column-major nu x nx
                 k=np.zeros((B, T, m)) if k else None, Vx=np.zeros((B, T + 1, n)) if Vx else None,
                 Vxx=np.zeros((B, T + 1, n, n)) if Vxx else None, risk_cost=np.zeros(B) if risk_cost else None)
        flags = np.zeros(B, dtype=np.int32) if info else None
        self._check(self.lib.ilqr_get_risk_sensitive(self.h, nw, float(theta), capi.LQ_HOLD_CLAMPED if hold_clamped else 0, float(mu), _p(Cc),
                                                     _p(o["K"]), _p(o["k"]), _p(o["Vx"]), _p(o["Vxx"]), _p(o["risk_cost"]), _pi(flags)))
        out = {name: (np.swapaxes(a, -1, -2) if name in ("K", "Vxx") else a) for name, a in o.items() if a is not None}
        if info:
            out["info"] = flags
        return out

    def copy_risk_sensitive_to_device(self, nw, theta, C_ptr, mu=0.0, hold_clamped=False, K_ptr=None, k_ptr=None, Vx_ptr=None, Vxx_ptr=None,
                                      risk_cost_ptr=None, info_ptr=None):
        """The same with raw device pointers (e.g. torch.Tensor.data_ptr()) to float64 C [B][nx*nw], K [B][T][nu*nx], k [B][T][nu], Vx
        [B][T+1][nx], Vxx [B][T+1][nx*nx] (column-major per matrix), risk_cost [B] and int32 info [B]; any output may be None, not all of
        the first five.  Enqueued on the handle's stream, nothing waited for."""
        self._check(self.lib.ilqr_copy_risk_sensitive_to_device(self.h, int(nw), float(theta), capi.LQ_HOLD_CLAMPED if hold_clamped else 0,
                                                                float(mu), C_ptr, K_ptr, k_ptr, Vx_ptr, Vxx_ptr, risk_cost_ptr, info_ptr))

    def _dirs_input(self, a, lead, width, what):
        """[B] + lead + [S][width], or without the direction axis (one direction) -> (canonical array or None, S, one direction?)"""
        if a is None:
            return None, None, False
        a = _c(a)
        flat = a.ndim == 2 + len(lead)
        if flat:
            a = np.ascontiguousarray(a[..., None, :])
        if a.ndim != 3 + len(lead) or a.shape[:1 + len(lead)] != (self.B,) + lead or a.shape[-1] != width or a.shape[-2] < 1:
            raise ValueError("%s must be %s, or the same without the direction axis S; got %s" % (what, ["B"] + list(lead) + ["S", width], a.shape))
        return a, a.shape[-2], flat

    def _dirs_pair(self, x, u, what):
        (x, Sx, fx), (u, Su, fu) = x, u
        if x is None and u is None:
            raise ValueError("%s are both None: the answer would be zero" % what)
        if x is not None and u is not None and (Sx != Su or fx != fu):
            raise ValueError("%s disagree on the directions: %s and %s" % (what, x.shape, u.shape))
        return (Sx if x is not None else Su), (fx if x is not None else fu)

    def _nku(self, t0, n):
        return max(min(int(t0) + n, self.T) - int(t0), 0)

    def tangent(self, dx0=None, dv=None, t0=0, n=None):
        """The tangent (Jacobian-vector product) of the linearised closed loop du[t] = K[t] dx[t] + dv[t], dx[t+1] = fx[t] dx[t] + fu[t] du[t]
        over the knots [t0, t0 + n) (n=None: up to knot T).  dx0: [B][S][nx], S directions per trajectory, perturbs the measured state;
        dv: [B][T][S][nu] perturbs the stored controls over the whole horizon; None = zero, not both.  Returns (dxs [B][n][S][nx],
        dus [B][nku][S][nu]), nku the window's knots that have a control.  A [B][nx] / [B][T][nu] input is one direction and the direction
        axis is dropped again on output (include/ilqr_amd.h, ilqr_get_tangent: recomputed on the device from the current records and the
        stored gains; synchronises)."""
        n = self.T + 1 - int(t0) if n is None else int(n)
        X, V = self._dirs_input(dx0, (), self.nx, "dx0"), self._dirs_input(dv, (self.T,), self.nu, "dv")
        S, flat = self._dirs_pair(X, V, "dx0 and dv")
        nku = self._nku(t0, n)
        dxs = np.zeros((self.B, max(n, 0), S, self.nx))
        dus = np.zeros((self.B, nku, S, self.nu))
        self._check(self.lib.ilqr_get_tangent(self.h, int(t0), n, S, _p(X[0]), _p(V[0]), _p(dxs), _p(dus) if nku else None))
        return (dxs[:, :, 0], dus[:, :, 0]) if flat else (dxs, dus)

    def adjoint(self, gx=None, gu=None, t0=0, n=None):
        """The adjoint (vector-Jacobian product) of the same map: gx [B][n][S][nx] = dL/dxs and gu [B][nku][S][nu] = dL/dus of a caller's
        loss over the knots [t0, t0 + n) (n=None: up to knot T; None = zero, not both).  Returns (g_x0 [B][S][nx] = dL/dx0, g_v [B][T][S][nu] =
        dL/dv, zero after the window).  A [B][n][nx] / [B][nku][nu] input is one direction and the direction axis is dropped again on output
        (include/ilqr_amd.h, ilqr_get_adjoint; synchronises)."""
        n = self.T + 1 - int(t0) if n is None else int(n)
        nku = self._nku(t0, n)
        X, U = self._dirs_input(gx, (max(n, 0),), self.nx, "gx"), self._dirs_input(gu, (nku,), self.nu, "gu")
        S, flat = self._dirs_pair(X, U, "gx and gu")
        g_x0, g_v = np.zeros((self.B, S, self.nx)), np.zeros((self.B, self.T, S, self.nu))
        self._check(self.lib.ilqr_get_adjoint(self.h, int(t0), n, S, _p(X[0]), _p(U[0]), _p(g_x0), _p(g_v)))
        return (g_x0[:, 0], g_v[:, :, 0]) if flat else (g_x0, g_v)

    def transition_matrices(self, t0=0, n=None):
        """The tangent of dx0 = I: (Phi [B][n][nx][nx], KPhi [B][nku][nu][nx]) with dx[t] = Phi[t] dx[0] and du[t] = KPhi[t] dx[0] = K[t] Phi[t]
        dx[0], the first-order change of the whole plan with the measured state (the Gauss-Newton sensitivity of a converged plan)."""
        dxs, dus = self.tangent(dx0=np.broadcast_to(np.eye(self.nx), (self.B, self.nx, self.nx)), t0=t0, n=n)
        return np.swapaxes(dxs, -1, -2), np.swapaxes(dus, -1, -2)

    def copy_tangent_to_device(self, t0, n, S, dx0_ptr=None, dv_ptr=None, dxs_ptr=None, dus_ptr=None):
        """The tangent with raw device pointers (e.g. torch.Tensor.data_ptr()) to float64 dx0 [B][S][nx], dv [B][T][S][nu] (None = zero, not
        both), dxs [B][n][S][nx], dus [B][nku][S][nu] (either may be None, not both).  Enqueued on the handle's stream, nothing waited for."""
        self._check(self.lib.ilqr_copy_tangent_to_device(self.h, int(t0), int(n), int(S), dx0_ptr, dv_ptr, dxs_ptr, dus_ptr))

    def copy_adjoint_to_device(self, t0, n, S, gx_ptr=None, gu_ptr=None, g_x0_ptr=None, g_v_ptr=None):
        """The adjoint with raw device pointers to float64 gx [B][n][S][nx], gu [B][nku][S][nu] (None = zero, not both), g_x0 [B][S][nx],
        g_v [B][T][S][nu] (either may be None, not both).  Enqueued on the handle's stream, nothing waited for."""
        self._check(self.lib.ilqr_copy_adjoint_to_device(self.h, int(t0), int(n), int(S), gx_ptr, gu_ptr, g_x0_ptr, g_v_ptr))

    def lq_solve(self, gx=None, gu=None, dx0=None, mu=0.0, hold_clamped=True, dlam=False):
        """The LQ subproblem of the current records solved for the caller's linear terms (include/ilqr_amd.h, ilqr_solve_lq): gx
        [B][T+1][S][nx], gu [B][T][S][nu] the linear cost terms, dx0 [B][S][nx] the initial perturbation, S directions per trajectory (None =
        zero, not all three); mu >= 0 is added to Quu's diagonal; hold_clamped keeps the controls whose row of the stored K is exactly zero
        at du = 0.  Returns (dxs [B][T+1][S][nx], dus [B][T][S][nu][, dlam [B][T+1][S][nx]], info [B]); info[b] = t + 1 when Quu of knot t was
        not positive definite on the free controls (that trajectory's outputs are NaN), else 0.  Inputs without the direction axis are one
        direction and the axis is dropped again on output.  With gx = cx, gu = cu: the Newton step; with gx = dL/dxs, gu = dL/dus: the
        backward pass of a differentiable MPC layer.  Synchronises."""
        X = self._dirs_input(gx, (self.T + 1,), self.nx, "gx")
        U = self._dirs_input(gu, (self.T,), self.nu, "gu")
        X0 = self._dirs_input(dx0, (), self.nx, "dx0")
        given = [a for a in (X, U, X0) if a[0] is not None]
        if not given:
            raise ValueError("gx, gu and dx0 are all None: the answer would be zero")
        S, flat = given[0][1], given[0][2]
        if any(a[1] != S or a[2] != flat for a in given):
            raise ValueError("gx, gu and dx0 disagree on the directions: %s" % [a[0].shape for a in given])
        dxs, dus = np.zeros((self.B, self.T + 1, S, self.nx)), np.zeros((self.B, self.T, S, self.nu))
        lam = np.zeros((self.B, self.T + 1, S, self.nx)) if dlam else None
        info = np.zeros(self.B, dtype=np.int32)
        self._check(self.lib.ilqr_solve_lq(self.h, S, capi.LQ_HOLD_CLAMPED if hold_clamped else 0, float(mu), _p(X0[0]), _p(X[0]), _p(U[0]), _p(dxs),
                                           _p(dus), _p(lam), _pi(info)))
        out = (dxs, dus) + ((lam,) if dlam else ())
        if flat:
            out = tuple(a[:, :, 0] for a in out)
        return out + (info,)

    def copy_lq_solve_to_device(self, S, mu=0.0, hold_clamped=True, dx0_ptr=None, gx_ptr=None, gu_ptr=None, dxs_ptr=None, dus_ptr=None, dlam_ptr=None,
                                info_ptr=None):
        """ilqr_solve_lq_on_device with raw device pointers (e.g. torch.Tensor.data_ptr()) to float64 dx0 [B][S][nx], gx [B][T+1][S][nx], gu
        [B][T][S][nu] (None = zero, not all three), dxs, dlam [B][T+1][S][nx], dus [B][T][S][nu] (any may be None, not all three), int32 info
        [B] (may be None).  Enqueued on the handle's stream, nothing waited for."""
        self._check(self.lib.ilqr_solve_lq_on_device(self.h, int(S), capi.LQ_HOLD_CLAMPED if hold_clamped else 0, float(mu), dx0_ptr, gx_ptr, gu_ptr,
                                                     dxs_ptr, dus_ptr, dlam_ptr, info_ptr))

    def derivatives(self):
        n, m, B, T1 = self.nx, self.nu, self.B, self.T + 1
        mem = dict(fx=np.zeros((B, T1, n, n)), fu=np.zeros((B, T1, m, n)), cx=np.zeros((B, T1, n)),
                   cu=np.zeros((B, T1, m)), cxx=np.zeros((B, T1, n, n)), cxu=np.zeros((B, T1, m, n)),
                   cuu=np.zeros((B, T1, m, m)))
        order = ("fx", "fu", "cx", "cu", "cxx", "cxu", "cuu")
        self._check(self.lib.ilqr_get_derivatives(self.h, *[_p(mem[k]) for k in order]))
        return {k: (v if k in ("cx", "cu") else np.swapaxes(v, -1, -2)) for k, v in mem.items()}

    def cost(self):
        c = np.zeros(self.B)
        self._check(self.lib.ilqr_get_cost(self.h, _p(c)))
        return c

    def lambdas(self):
        lam, dlam = np.zeros(self.B), np.zeros(self.B)
        self._check(self.lib.ilqr_get_lambda(self.h, _p(lam), _p(dlam)))
        return lam, dlam

    def dV(self):
        d = np.zeros((self.B, 2))
        self._check(self.lib.ilqr_get_dV(self.h, _p(d)))
        return d

    def gnorm(self):
        g = np.zeros(self.B)
        self._check(self.lib.ilqr_get_gnorm(self.h, _p(g)))
        return g

    def status(self):
        st, it, al = (np.zeros(self.B, dtype=np.int32) for _ in range(3))
        self._check(self.lib.ilqr_get_status(self.h, st.ctypes.data_as(_ip), it.ctypes.data_as(_ip),
                                            al.ctypes.data_as(_ip)))
        return st, it, al

    def candidate(self, a):
        xs = np.zeros((self.B, self.T + 1, self.nx))
        us = np.zeros((self.B, self.T, self.nu))
        self._check(self.lib.ilqr_get_candidate(self.h, int(a), _p(xs), _p(us)))
        return xs, us

    def count_running(self):
        n = C.c_int(0)
        self._check(self.lib.ilqr_count_running(self.h, C.byref(n)))
        return n.value

    # ---- measurement ----
    def profile(self, enable=True):
        self._check(self.lib.ilqr_profile_enable(self.h, int(enable)))

    def profile_reset(self):
        self._check(self.lib.ilqr_profile_reset(self.h))

    def profile_read(self):
        ms = (C.c_double * capi.NUM_STAGES)()
        n = (C.c_int * capi.NUM_STAGES)()
        self._check(self.lib.ilqr_profile_read(self.h, ms, n))
        return {capi.STAGE_NAMES[i]: (ms[i], n[i]) for i in range(capi.NUM_STAGES)}

    def shader_clock_mhz(self):
        """clock of the CUs during the persistent kernel's launches since the last profile_reset (ilqr_profile_shader_clock)"""
        mhz = C.c_double(0)
        self._check(self.lib.ilqr_profile_shader_clock(self.h, C.byref(mhz)))
        return mhz.value
