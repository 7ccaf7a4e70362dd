"""Host-side mirror of the reference solver class over the C ABI.

``IterativeLinearQuadraticRegulator`` keeps the class surface of
/root/reference/ilqr.py:12-733 (same constructor signature, setters, ``Solve``
return tuple, ``SaveSolution`` npz keys, attribute names and shapes) so the
solver section of any example script can import it as a drop-in; the `system`
argument is a model descriptor (drake_ddp_amd.models.ModelSystem).  All compute
is in libmi_ilqr.so (HIP, gfx950) — this file only moves arrays across the
boundary.  ``BatchedIterativeLQR`` is the same surface with a leading batch axis.

The two classes are the only place of the front end that calls the library.  What a method accepts is decided in argcheck.py
(the ``check_*`` functions, before the first call on the handle), what it returns is built in results.py (``PolicyStats``,
``SeedSelection``, ...); neither module needs the library, and both are re-exported here under the names they always had.
"""
import ctypes as C
import time
import warnings
import weakref

import numpy as np

from . import _capi
from . import utils_derivs_interpolation
from .argcheck import (MC_DISTS, check_fit_args, check_mc_args, check_mc_observe, check_model_params, check_mppi_args,  # noqa: F401
                       check_noise_args, check_plant_args, check_rollout_args, check_seed_args, check_target_trajectory, integer)
from .models import ModelSystem
from .results import (MPPIResult, ParamFit, PlantLog, PolicyEnvelope, PolicyRollout, PolicySafety, PolicySamples, PolicyStats,  # noqa: F401
                      SeedSelection, _chan)

_KP_IDS = {"setInterval": _capi.KP_SET_INTERVAL, "adaptiveJerk": _capi.KP_ADAPTIVE_JERK,
           "iterativeError": _capi.KP_ITERATIVE_ERROR}
_JAC_IDS = {"fd": _capi.JAC_FD_CENTRAL, "fd_central": _capi.JAC_FD_CENTRAL,
            "autodiff": _capi.JAC_AUTODIFF, "ad": _capi.JAC_AUTODIFF}


from .dist import shard_range, allreduce_min, allreduce_min_async  # noqa: E402,F401


class _PinnedBlock:
    """One page-locked allocation of a solver's result pool and whether an array handed out over it is still alive."""
    __slots__ = ("raw", "addr", "ctype", "count", "busy", "ref", "__weakref__")

    def __init__(self, raw, nbytes, count):
        self.raw, self.addr, self.count, self.busy, self.ref = raw, raw.value, count, False, None
        self.ctype = C.c_char * nbytes

    def _released(self, _ref):
        self.busy = False


class BatchedIterativeLQR:
    """B independent iLQR problems sharing model, horizon and cost, solved on one GPU.

    Same method names as the reference class; array arguments/attributes carry a
    leading batch axis: x0 (B,n), u_guess (B,m,N-1) [or (m,N-1), broadcast],
    x_bar (B,n,N), u_bar (B,m,N-1), K (B,m,n,N-1), kappa (B,m,N-1) ...
    """

    def __init__(self, system, num_timesteps, batch, input_port_index=0, delta=1e-2, beta=0.95, gamma=0.0,
                 derivs_keypoint_method=None, jacobian_mode="fd", fd_step=1e-5, device=0,
                 max_iters=1000, hist_cap=64, kernel_mode="auto", pinned_results=True, on_indefinite="stop",
                 control_limits="ignore"):
        assert isinstance(system, ModelSystem), \
            "system must be a drake_ddp_amd.models.ModelSystem (Drake systems cannot run on the GPU)"
        assert system.IsDifferenceEquationSystem()[0], "must be a discrete-time system"   # ilqr.py:37
        self._lib = _capi.load()
        self.system = system
        self.N = int(num_timesteps)
        self.B = int(batch)
        self.delta, self.beta, self.gamma = delta, beta, gamma
        self.n, self.m = system.n, system.m
        # device-side number of controls: more than m when the model carries padding controls (n > 32 with m % 4 != 0 on the
        # workgroup-per-problem kernels, plugin.device_controls).  Everything a caller passes or receives has m controls;
        # R gets a unit block, guesses zeros, results are cut back - the padding's gains and inputs are exact zeros.
        self._md = int(getattr(system, "m_dev", system.m))
        # ilqr.py:97-100: default = derivatives at every time step
        if derivs_keypoint_method is None:
            derivs_keypoint_method = utils_derivs_interpolation.derivs_interpolation('setInterval', 1, 0, 0, 0)
        self.derivs_interpolation = derivs_keypoint_method
        if derivs_keypoint_method.keypoint_method not in _KP_IDS:
            raise Exception('unknown interpolation method')                               # ilqr.py:404
        d = _capi.Desc()
        d.n, d.m, d.N, d.B = self.n, self._md, self.N, self.B
        d.model_id = system.model_id
        d.n_params = system.params.size
        for i, v in enumerate(system.params):
            d.model_params[i] = float(v)
        d.dt = system.dt
        d.delta, d.beta, d.gamma = float(delta), float(beta), float(gamma)
        d.keypoint_method = _KP_IDS[derivs_keypoint_method.keypoint_method]
        d.minN, d.maxN = int(derivs_keypoint_method.minN), int(derivs_keypoint_method.maxN)
        d.jerk_threshold = float(derivs_keypoint_method.jerk_threshold)
        d.iterative_error_threshold = float(derivs_keypoint_method.iterative_error_threshold)
        d.jacobian_mode = _JAC_IDS[jacobian_mode]
        d.fd_step = float(fd_step)
        d.max_iters, d.hist_cap, d.device_id = int(max_iters), int(hist_cap), int(device)
        d.kernel_mode = {"auto": _capi.KERNEL_AUTO, "latency": _capi.KERNEL_LATENCY,
                         "throughput": _capi.KERNEL_THROUGHPUT}[kernel_mode]
        # a Quu that is not positive definite (workgroup-per-problem kernels): "stop" the problem with STATUS_NOT_PD (this class's
        # default: one such problem does not spoil a batch - it is reported, never raised), or "continue" like the reference, which
        # inverts whatever comes out with np.linalg.inv and carries on (ilqr.py:655; the single-problem drop-in's default)
        d.on_indefinite = {"stop": 0, "continue": 1}[on_indefinite]
        self.on_indefinite = on_indefinite
        self._desc = d
        self.hist_cap = int(hist_cap)
        h = C.c_void_p()
        _capi.check(self._lib.mi_ilqr_create(C.byref(d), C.byref(h)), "mi_ilqr_create")
        self._h = h
        # control_limits: "ignore" (default) keeps the reference's SetControlLimits, a no-op (ilqr.py:158-159); "enforce" makes it
        # bound the controls (include/mi_ilqr.h: mi_ilqr_set_control_limits) - the m <= 2 kernel families and the mid-size family (n <= 32)
        if control_limits not in ("ignore", "enforce"):
            raise ValueError(f'control_limits must be "ignore" or "enforce", got {control_limits!r}')
        self.control_limits = control_limits
        if control_limits == "enforce":
            rc = self._lib.mi_ilqr_set_control_limits(h, None, None, 0)
            if rc == _capi.E_UNSUPPORTED:
                raise ValueError("control_limits='enforce' is served by the m <= 2 kernel families and the mid-size workgroup "
                                 "family (n <= 32) only: the built-in pendulum, acrobot, cart-pole and arm models, family-0 "
                                 "plugins and family-1 plugins with n <= 32 built with control_limits=True; this model runs on "
                                 "other workgroup-per-problem kernels")
            _capi.check(rc, "mi_ilqr_set_control_limits")
        # pinned_results (the default): the arrays the state attributes / Solve() return are views of page-locked buffers
        # (direct DMA, no page faults of freshly allocated arrays; the wave-per-problem kernels write x_bar / u_bar / cost
        # into them themselves).  The reference REBINDS its result arrays on every forward pass and never mutates one it
        # has handed out (ilqr.py:375-376) - so does this class: a buffer is reused only once the caller has
        # dropped every reference to the array it got (a small pool per attribute; `x, u, t, L = ilqr.Solve()` in a loop
        # alternates between two blocks), otherwise a new block is taken.  False: plain pageable arrays and blocking copies.
        self._pinned = {} if pinned_results else None
        self._into = None
        self._result_fields = ((_capi.F_X_BAR, (self.B, self.n, self.N)), (_capi.F_U_BAR, (self.B, self._md, self.N - 1)), (_capi.F_COST, (self.B,)))
        self._sink = None              # pinned_results: whether the kernels of this handle can write the results into host buffers themselves
        # reference defaults (ilqr.py:61-67); NOTE x_nom is undefined until SetTargetState (F12)
        self.x0 = np.zeros((self.B, self.n))
        self.Q, self.R, self.Qf = np.eye(self.n), np.eye(self.m), np.eye(self.n)
        self._u_guess = None
        self.stats = None
        self.time_getDerivs = self.time_backwardsPass = self.time_fp = 0.0
        self.solve_wall_s = 0.0
        self._ref_T = 0                # rows of the reference this object last set (SetTargetTrajectory); the handle says whether it holds one

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.mi_ilqr_destroy(h)           # (synchronizes the stream: no kernel writes a result sink afterwards)

    # ------------------------------------------------------------- setters (ilqr.py:102-159)
    def SetInitialState(self, x0):
        self.x0 = x0

    def SetTargetState(self, x_nom):
        """(n,) or (1, n): one target for the batch (the reference's argument).  (B, n): every problem its own target - the
        reference's SetTargetState called on each problem's own object (include/mi_ilqr.h: "Per-problem targets")."""
        x_nom = np.asarray(x_nom)
        if x_nom.size != self.n and x_nom.shape == (self.B, self.n):
            self.x_nom = x_nom
        else:
            self.x_nom = x_nom.reshape((self.n,))

    def _per_problem_targets(self):
        return np.ndim(self.x_nom) == 2

    def _set_field(self, which, a):
        a = _capi.as_f64(a, (self.B, self.n))
        _capi.check(self._lib.mi_ilqr_set(self._h, which, _capi.ptr(a), a.nbytes), "mi_ilqr_set")

    def SetTargetTrajectory(self, x_ref, clock=0):
        """A reference to TRACK: (B, T, n), every problem its own, or (T, n) for the whole batch (include/mi_ilqr.h: "Reference
        trajectories").  While the solver holds one, time index t of a solve is pulled towards x_ref[b, min(clock + t, T - 1)] instead
        of x_nom - the terminal term towards index N - 1's row; past its end the reference holds its last row.  MPCRun moves the
        clock by replan_steps per re-solve (target_clock).  A one-row reference is the constant target SetTargetState gives, bit
        for bit.  None clears it: the solver is back on x_nom, as if it had never held one.  Takes effect at once; survives
        Reset().  Workgroup-per-problem models only; not together with SetPlant / RolloutPolicy."""
        rows, c = check_target_trajectory(x_ref, clock, self.B, self.n)
        rc = self._lib.mi_ilqr_set(self._h, _capi.F_X_REF, _capi.ptr(rows), 0 if rows is None else rows.nbytes)
        if rc == _capi.E_UNSUPPORTED:
            if self._holds_plant():
                raise ValueError("SetTargetTrajectory: this solver holds a plant (SetPlant), and the plant kernels know constant "
                                 "targets only; ClearPlant() first")
            raise ValueError("SetTargetTrajectory: reference trajectories are served by the workgroup-per-problem kernel family "
                             f"only; this model (n = {self.n}, m = {self.m}) runs on the wave-per-problem or the lane-per-problem "
                             "family")
        _capi.check(rc, "mi_ilqr_set")
        if rows is not None:               # (clearing the reference has reset the clock)
            self._send(_capi.F_REF_CLOCK, np.array([float(c)]))
        self._ref_T = 0 if rows is None else rows.shape[1]

    def _holds_plant(self):
        out = np.empty((self.B, self.n))
        return self._lib.mi_ilqr_get(self._h, _capi.F_PLANT_STATE, _capi.ptr(out), out.nbytes) == _capi.OK

    def _tracking(self):
        """Whether the HANDLE holds a reference (it may have been set, or lost, through the C ABI): MI_F_X_REF answers
        MI_ILQR_E_BAD_ARG without one, and with one MI_ILQR_OK or - a length other than the one this object last set - BAD_SHAPE."""
        probe = np.empty((self.B, max(self._ref_T, 1), self.n))
        return self._lib.mi_ilqr_get(self._h, _capi.F_X_REF, _capi.ptr(probe), probe.nbytes) != _capi.E_BAD_ARG

    def _refuse_tracking(self, who, why, when=True):
        """ValueError "<who>: this solver holds a reference trajectory (SetTargetTrajectory)<why>" if it does (and `when`)."""
        if self._tracking() and when:
            raise ValueError(f"{who}: this solver holds a reference trajectory (SetTargetTrajectory){why}")

    @property
    def target_trajectory(self):
        """(B, T, n): the reference the solver holds (SetTargetTrajectory), or None."""
        return self._fetch(_capi.F_X_REF, (self.B, self._ref_T, self.n)) if self._tracking() else None

    @property
    def target_clock(self):
        """The row of the reference the next solve's window starts at (SetTargetTrajectory's clock, advanced by MPCRun); 0 without one."""
        return int(self._fetch(_capi.F_REF_CLOCK, (1,))[0]) if self._tracking() else 0

    def SetModelParameters(self, params):
        """(B, n_params): every problem its own plant - the reference's one solver object per System, B of them in one handle
        (include/mi_ilqr.h: "Per-problem model parameters").  (n_params,): that row for every problem.  None: back to the
        parameters of the system the solver was built with.  Takes effect for the next solve; survives Reset()."""
        self._send(_capi.F_MODEL_PARAMS, check_model_params(params, self.B, int(self.system.params.size)))

    @property
    def model_params(self):
        """(B, n_params): the parameters each problem is solved with (the system's own row repeated unless SetModelParameters gave others)."""
        return self._fetch(_capi.F_MODEL_PARAMS, (self.B, int(self.system.params.size)))

    def SetRunningCost(self, Q, R):
        """(n, n) and (m, m): one pair for the batch (the reference's arguments).  (B, n, n) / (B, m, m): every problem its own
        weights - the reference's SetRunningCost called on each problem's own object (include/mi_ilqr.h: "Per-problem cost
        matrices").  Any mix of the two forms, with SetTerminalCost's as well: the shared ones are repeated.  With all three
        matrices 2-D again the handle is back on shared matrices.  Takes effect for the next solve; survives Reset()."""
        assert Q.shape in ((self.n, self.n), (self.B, self.n, self.n))
        assert R.shape in ((self.m, self.m), (self.B, self.m, self.m))
        self.Q = Q
        self.R = R

    def SetTerminalCost(self, Qf):
        """(n, n), or (B, n, n): every problem its own terminal weights (SetRunningCost)."""
        assert Qf.shape in ((self.n, self.n), (self.B, self.n, self.n))
        self.Qf = Qf

    def _per_problem_costs(self):
        return any(np.ndim(a) == 3 for a in (self.Q, self.R, self.Qf))

    def _cost_rows(self):
        """(B, 2 n^2 + m_dev^2): row b = Q_b | R_b | Qf_b as the device takes them (MI_F_COST_MATRICES), shared matrices repeated."""
        B, n, md = self.B, self.n, self._md
        R = np.asarray(self.R, dtype=np.float64)
        if self._md != self.m:                      # padding controls: a unit block, like the shared R gets
            Rp = np.zeros(R.shape[:-2] + (md, md))
            Rp[..., :self.m, :self.m] = R
            Rp[..., range(self.m, md), range(self.m, md)] = 1.0
            R = Rp
        parts = [np.broadcast_to(np.asarray(a, dtype=np.float64), (B, k, k)).reshape(B, k * k)
                 for a, k in ((self.Q, n), (R, md), (self.Qf, n))]
        rows = np.ascontiguousarray(np.concatenate(parts, axis=1))
        if not np.isfinite(rows).all():
            raise ValueError("SetRunningCost / SetTerminalCost: NaN or infinity in per-problem cost matrices")
        return rows

    @property
    def cost_matrices(self):
        """(Q, R, Qf) as (B, n, n), (B, m, m), (B, n, n): the weights each problem is solved with, as set (the shared matrices
        repeated where SetRunningCost / SetTerminalCost gave 2-D ones)."""
        B, n, m = self.B, self.n, self.m
        return tuple(np.array(np.broadcast_to(np.asarray(a, dtype=np.float64), (B, k, k)))
                     for a, k in ((self.Q, n), (self.R, m), (self.Qf, n)))

    def SetInitialGuess(self, u_guess):
        assert u_guess.shape in ((self.m, self.N - 1), (self.B, self.m, self.N - 1))
        self._u_guess = u_guess        # aliased like the reference; copied in at Solve()

    def SetControlLimits(self, u_min, u_max):
        """No-op stub in the reference (ilqr.py:158-159), and here unless the solver was built with
        control_limits="enforce": then u_min <= u <= u_max for every rollout and backward pass of later solves.
        Scalars (m = 1), (m,) or (B, m); +-inf allowed; (None, None) clears the limits."""
        if self.control_limits != "enforce":
            return
        if u_min is None and u_max is None:
            _capi.check(self._lib.mi_ilqr_set_control_limits(self._h, None, None, 0), "mi_ilqr_set_control_limits")
            return
        if u_min is None or u_max is None:
            raise ValueError("SetControlLimits: give both bounds, or (None, None) to clear them")
        lo, hi = (np.asarray(v, dtype=np.float64) for v in (u_min, u_max))
        if lo.shape != hi.shape:
            raise ValueError(f"SetControlLimits: u_min {lo.shape} and u_max {hi.shape} differ in shape")
        if lo.ndim == 0 and self.m == 1:
            lo, hi = lo.reshape(1), hi.reshape(1)
        if lo.shape == (self.m,):
            per_problem = 0
        elif lo.shape == (self.B, self.m):
            per_problem = 1
        else:
            raise ValueError(f"SetControlLimits: bounds must be scalars (m = 1), ({self.m},) or ({self.B}, {self.m}); got {lo.shape}")
        if np.isnan(lo).any() or np.isnan(hi).any() or (lo > hi).any():
            raise ValueError("SetControlLimits: u_min > u_max or NaN")
        lo, hi = np.ascontiguousarray(lo), np.ascontiguousarray(hi)
        _capi.check(self._lib.mi_ilqr_set_control_limits(self._h, _capi.ptr(lo), _capi.ptr(hi), per_problem),
                    "mi_ilqr_set_control_limits")

    # ------------------------------------------------------------- boundary traffic
    def _push_problem(self):
        self._push_costs()
        x0 = np.asarray(self.x0, dtype=np.float64).reshape(-1, self.n)
        x0 = np.ascontiguousarray(x0 if len(x0) == self.B else np.broadcast_to(x0, (self.B, self.n)))
        ug = None
        shared = False
        if self._u_guess is not None:
            ug = np.asarray(self._u_guess, dtype=np.float64)
            # one sequence for the whole batch - (m,N-1) or (1,m,N-1), the reference's own argument - crosses the
            # bus once; the device writes the batch's copies
            if ug.shape not in ((self.m, self.N - 1), (1, self.m, self.N - 1), (self.B, self.m, self.N - 1)):
                raise AssertionError(f"initial guess must be (m,N-1) or (B,m,N-1), got {ug.shape}")
            shared = ug.ndim == 2 or (ug.shape[0] == 1 and self.B > 1)
            if shared:
                ug = np.ascontiguousarray(self._pad_u(ug.reshape(self.m, self.N - 1), (0,)))
            else:
                ug = np.ascontiguousarray(self._pad_u(np.broadcast_to(ug, (self.B, self.m, self.N - 1)), (1,)))
            self._u_guess = None       # u_bar is rebound by the forward pass (ilqr.py:375)
        if shared:
            _capi.check(self._lib.mi_ilqr_set_initial_shared(self._h, _capi.ptr(x0), _capi.ptr(ug)), "mi_ilqr_set_initial_shared")
        else:
            _capi.check(self._lib.mi_ilqr_set_initial(self._h, _capi.ptr(x0), _capi.ptr(ug)), "mi_ilqr_set_initial")

    def _push_costs(self):
        """The cost matrices and targets as set on this object, to the handle (what every Solve / stage call does first)."""
        x_nom = self.x_nom             # AttributeError if SetTargetState was never called, as in the reference
        per_problem = np.ndim(x_nom) == 2
        xn = None if per_problem else _capi.as_f64(x_nom, (self.n,))
        if self._per_problem_costs():
            # (B, ..) weights: the handle's per-problem cost matrices; the shared ones stay what they were, x_nom goes alone
            rows = self._cost_rows()
            if xn is not None:
                _capi.check(self._lib.mi_ilqr_set_cost(self._h, None, None, None, _capi.ptr(xn)), "mi_ilqr_set_cost")
            _capi.check(self._lib.mi_ilqr_set(self._h, _capi.F_COST_MATRICES, _capi.ptr(rows), rows.nbytes), "mi_ilqr_set")
        else:                          # (shared matrices switch per-problem cost matrices off again)
            Q, R, Qf = (_capi.as_f64(a) for a in (self.Q, self._pad_u(self.R, (0, 1), diag=1.0), self.Qf))
            _capi.check(self._lib.mi_ilqr_set_cost(self._h, _capi.ptr(Q), _capi.ptr(R), _capi.ptr(Qf), _capi.ptr(xn)),
                        "mi_ilqr_set_cost")
        if per_problem:                # (B, n): the handle's per-problem targets (a shared x_nom above switches them off again)
            self._set_field(_capi.F_X_NOM, x_nom)

    _POOL_CAP = 4

    def _out(self, which, shape, dtype):
        return self._out_addr(which, shape, dtype)[0]

    def _out_addr(self, which, shape, dtype):
        """Destination of a field read and its address: a fresh array, or (pinned_results) a page-locked block nobody else holds.

        Every hand-out wraps the block in a NEW owner array (np.frombuffer); every view a caller derives from what it got has
        that owner as its base, so the owner dies exactly when the last of them does - a weak reference's callback then marks
        the block free.  No reference counts are read (a debugger, a profiler or another interpreter may hold extra ones): a
        block whose owner has not been collected yet simply is not reused."""
        if self._pinned is None:
            a = np.empty(shape, dtype=dtype)
            return a, _capi.ptr(a)
        key = (which, shape if type(shape) is tuple else tuple(shape), dtype)
        pool = self._pinned.get(key)
        if pool is None:
            pool = self._pinned[key] = []
        blk = None
        for b_ in pool:
            if not b_.busy:
                blk = b_
                break
        if blk is None:
            if len(pool) >= self._POOL_CAP:         # the caller keeps many results alive: those stay theirs, this one is pageable
                a = np.empty(shape, dtype=dtype)
                return a, _capi.ptr(a)
            count = int(np.prod(shape))
            nbytes = max(count * np.dtype(dtype).itemsize, 8)
            raw = C.c_void_p()
            _capi.check(self._lib.mi_ilqr_host_alloc(nbytes, C.byref(raw)), "mi_ilqr_host_alloc")
            blk = _PinnedBlock(raw, nbytes, count)
            # the memory lives as long as the block object does: the pool's reference, or a buffer a caller's array still wraps
            weakref.finalize(blk, self._lib.mi_ilqr_host_free, raw).atexit = False
            pool.append(blk)
        buf = blk.ctype.from_address(blk.addr)
        buf._block = blk                            # (an array over the buffer keeps the buffer, the buffer keeps the block - and its memory)
        owner = np.frombuffer(buf, dtype=dtype, count=blk.count)
        blk.busy = True
        blk.ref = weakref.ref(owner, blk._released)
        return owner.reshape(shape), blk.addr

    # axis (from the end) along which a field carries the controls
    _U_AXIS = {_capi.F_U_BAR: -2, _capi.F_KAPPA: -2, _capi.F_U_TRIAL: -2, _capi.F_K: -3, _capi.F_FU: -2}

    def _pad_u(self, a, axes, diag=0.0):
        """`a` with its control axes grown from m to the device's count (zeros; `diag` on the new diagonal of a square block)."""
        if self._md == self.m:
            return a
        a = np.asarray(a, dtype=np.float64)
        shape = list(a.shape)
        for ax in axes:
            shape[ax] = self._md
        out = np.zeros(shape)
        out[tuple(slice(0, self.m) if i in [ax % a.ndim for ax in axes] else slice(None) for i in range(a.ndim))] = a
        if diag and len(axes) == 2:
            for k in range(self.m, self._md):
                out[k, k] = diag
        return out

    def _dev_shape(self, which, shape):
        if self._md == self.m or which not in self._U_AXIS:
            return tuple(shape), None
        ax = len(shape) + self._U_AXIS[which]
        dev = list(shape)
        dev[ax] = self._md
        return tuple(dev), ax

    def _cut_u(self, out, ax):
        return out if ax is None else out[tuple(slice(0, self.m) if i == ax else slice(None) for i in range(out.ndim))]

    def _get(self, which, shape):
        dev, ax = self._dev_shape(which, shape)
        out = self._out(which, dev, np.float64)
        _capi.check(self._lib.mi_ilqr_get(self._h, which, _capi.ptr(out), out.nbytes), "mi_ilqr_get")
        return self._cut_u(out, ax)

    def _get_int(self, which, shape):
        out = self._out(which, shape, np.int32)
        _capi.check(self._lib.mi_ilqr_get_int(self._h, which, _capi.ptr(out), out.nbytes), "mi_ilqr_get_int")
        return out

    def _set(self, which, arr, shape):
        dev, ax = self._dev_shape(which, shape)
        if ax is not None:
            arr, shape = self._pad_u(np.asarray(arr, dtype=np.float64).reshape(shape), (ax,)), dev
        arr = _capi.as_f64(arr, shape)
        _capi.check(self._lib.mi_ilqr_set(self._h, which, _capi.ptr(arr), arr.nbytes), "mi_ilqr_set")

    def _send(self, which, a):
        """A checked, contiguous array to a selector as it is; None: the selector's "no such rows" (no pointer, 0 bytes)."""
        _capi.check(self._lib.mi_ilqr_set(self._h, which, _capi.ptr(a), 0 if a is None else a.nbytes), "mi_ilqr_set")

    def _fetch(self, which, shape, dtype=np.float64):
        """A selector into a fresh pageable array as the device holds it (the pinned pool and the cut of padding controls: _get);
        any dtype but float64 goes through mi_ilqr_get_int."""
        out = np.empty(shape, dtype=dtype)
        entry = "mi_ilqr_get" if dtype is np.float64 else "mi_ilqr_get_int"
        _capi.check(getattr(self._lib, entry)(self._h, which, _capi.ptr(out), out.nbytes), entry)
        return out

    # state attributes with the reference's names (batched)
    x_bar = property(lambda s: s._get(_capi.F_X_BAR, (s.B, s.n, s.N)))
    u_bar = property(lambda s: s._get(_capi.F_U_BAR, (s.B, s.m, s.N - 1)))
    K = property(lambda s: s._get(_capi.F_K, (s.B, s.m, s.n, s.N - 1)))
    kappa = property(lambda s: s._get(_capi.F_KAPPA, (s.B, s.m, s.N - 1)))
    dV_coeff = property(lambda s: s._get(_capi.F_DV, (s.B, s.N - 1)))
    fx = property(lambda s: s._get(_capi.F_FX, (s.B, s.n, s.n, s.N - 1)))
    fu = property(lambda s: s._get(_capi.F_FU, (s.B, s.n, s.m, s.N - 1)))
    cost = property(lambda s: s._get(_capi.F_COST, (s.B,)))
    history = property(lambda s: s._get(_capi.F_HIST, (s.B, s.hist_cap, 4)))
    iteration_cycles = property(lambda s: s._get(_capi.F_ITER_CYCLES, (s.B, s.hist_cap, 4)))
    iterations = property(lambda s: s._get_int(_capi.I_ITERS, (s.B,)))
    status = property(lambda s: s._get_int(_capi.I_STATUS, (s.B,)))
    ls_trials = property(lambda s: s._get_int(_capi.I_LS_TRIALS, (s.B,)))
    keypoint_count = property(lambda s: s._get_int(_capi.I_KP_COUNT, (s.B,)))
    keypoint_list = property(lambda s: s._get_int(_capi.I_KP_LIST, (s.B, s.N - 1)))

    @property
    def percentage_derivs(self):
        return self.keypoint_count / (self.N - 1) * 100.0          # ilqr.py:406

    def set_state(self, **fields):
        """Overwrite persistent state arrays (stage-level tests / checkpoint restore)."""
        table = {"x_bar": (_capi.F_X_BAR, (self.B, self.n, self.N)), "u_bar": (_capi.F_U_BAR, (self.B, self.m, self.N - 1)),
                 "K": (_capi.F_K, (self.B, self.m, self.n, self.N - 1)), "kappa": (_capi.F_KAPPA, (self.B, self.m, self.N - 1)),
                 "dV_coeff": (_capi.F_DV, (self.B, self.N - 1)), "fx": (_capi.F_FX, (self.B, self.n, self.n, self.N - 1)),
                 "fu": (_capi.F_FU, (self.B, self.n, self.m, self.N - 1))}
        for k, v in fields.items():
            self._set(table[k][0], v, table[k][1])

    @property
    def stage_cycles(self):
        """(B,4) in-kernel shader-clock cycles of the last solve: line search, linearization,
        backward pass, whole loop (device counterpart of time_fp/time_getDerivs/time_backwardsPass)."""
        out = np.empty((self.B, 4), dtype=np.int64)
        _capi.check(self._lib.mi_ilqr_get_cycles(self._h, _capi.ptr(out), out.nbytes), "mi_ilqr_get_cycles")
        return out

    @property
    def cluster_stats(self):
        """Workgroup-per-problem kernels, diagnostic: per problem of the last launch - helpers that took part, linearizations shared
        with them the regular way, rounds in which every helper sat on the leader's own XCD, early rounds opened (the helpers
        linearize the line search's first trial while it is rolled out), early rounds whose trial was accepted, candidate-group rounds
        (mid-size kernels: the helpers roll out line-search candidates 4 .. beside the leader's four) - (B,6) int64;
        zeros when the launch was not clustered (mi_ilqr.h: MI_I64_CLUSTER_WORDS)."""
        w = self._fetch(_capi.I64_CLUSTER_WORDS, (self.B, _capi.CLUSTER_WORDS), np.uint64)
        u = np.uint64
        ea_open, ea_hit, groups = w[:, 5] >> u(32), w[:, 5] & u(0xffffffff), w[:, 7]
        return np.stack([w[:, 2] & u(0xffff), (w[:, 3] >> u(32)) - ea_open - groups, (w[:, 3] >> u(8)) & u(0xffffff), ea_open, ea_hit, groups], axis=1).astype(np.int64)

    def last_kernel_ms(self):
        ms = C.c_float()
        _capi.check(self._lib.mi_ilqr_last_kernel_ms(self._h, C.byref(ms)), "mi_ilqr_last_kernel_ms")
        return float(ms.value)

    def set_timing(self, every=1):
        """HIP events on one pipelined solve in `every` (1 = all, the default; 0 = none): see mi_ilqr_set_timing."""
        _capi.check(self._lib.mi_ilqr_set_timing(self._h, int(every)), "mi_ilqr_set_timing")

    def Reset(self):
        """Forget warm-start state: equivalent to constructing a new solver (ilqr.py:70-83)."""
        _capi.check(self._lib.mi_ilqr_reset(self._h), "mi_ilqr_reset")

    def _check_internal(self, stats):
        """A solve aborted inside the kernel (MI_STATUS_INTERNAL: a cluster helper stopped answering) left x_bar / u_bar
        that are not a solution: never hand them out as one.  Problems that met a Quu which is not positive definite do NOT
        abort the batch - the other B - 1 results are valid: they are reported per problem (`status`: STATUS_NOT_PD = stopped
        there with on_indefinite="stop", STATUS_FLAG_INDEFINITE OR-ed onto the outcome with "continue"), counted in
        stats.n_not_pd, and announced by a warning."""
        if stats is not None and stats.n_internal > 0:
            raise RuntimeError(f"{stats.n_internal} problem(s) aborted inside the device kernel (status {_capi.STATUS_INTERNAL}); "
                               "their results are not a solution")
        if stats is not None and stats.n_max_iters > 0:
            # (the reference's loop has no cap, ilqr.py:692: a problem stopped by this class's `max_iters` is not a converged one)
            warnings.warn(f"{stats.n_max_iters} of {self.B} problem(s) stopped at max_iters = {int(self._desc.max_iters)} with the improvement "
                          f"still above delta (status {_capi.STATUS_MAX_ITERS}): not converged", RuntimeWarning, stacklevel=3)
        if stats is not None and stats.n_not_pd > 0:
            how = ("stopped there (status %d): their gains are not to be used" % _capi.STATUS_NOT_PD if self.on_indefinite == "stop"
                   else "inverted it like the reference's np.linalg.inv (ilqr.py:655) and carried on (status flag %d)" % _capi.STATUS_FLAG_INDEFINITE)
            warnings.warn(f"{stats.n_not_pd} of {self.B} problem(s) met a Quu that is not positive definite in a backward pass and {how}",
                          RuntimeWarning, stacklevel=3)

    # ------------------------------------------------------------- Solve (ilqr.py:669-710)
    def Solve(self):
        st = time.time()
        self._push_problem()
        if self._pinned is not None:
            res = self._solve_into_pinned()
            self._check_internal(self.stats)
            self.solve_wall_s = time.time() - st
            return res[0], res[1], self.solve_wall_s, res[2]
        stats = _capi.Stats()
        _capi.check(self._lib.mi_ilqr_solve(self._h, C.byref(stats)), "mi_ilqr_solve")
        self.stats = stats
        self._check_internal(stats)
        self.solve_wall_s = time.time() - st
        return self.x_bar, self.u_bar, self.solve_wall_s, self.cost

    def _solve_into_pinned(self, extra=()):
        """One solve from the inputs just pushed, x_bar / u_bar / cost into page-locked arrays nobody else holds, ONE host
        synchronization.  Wave-per-problem kernels write them themselves as each problem finishes (mi_ilqr_set_result_sink:
        the copy-out overlaps the launch's stragglers) - the sink is set for THIS solve only, so no later kernel of the
        handle (pipelined solves, MPCRun, stage calls) touches arrays a caller holds; the other kernel families enqueue
        three copy-outs behind the solve.  `extra`: (field, destination, its address) triples copied out behind the solve as
        well.  ONE call across the boundary (mi_ilqr_solve_into)."""
        (x, ax), (u, au), (c, ac) = (self._out_addr(which, shp, np.float64) for which, shp in self._result_fields)
        res = [x, u, c]
        pinned = self._sink is not False and x.base is not None and u.base is not None and c.base is not None
        k = len(extra)
        if self._into is None or len(self._into[0]) != k:
            self._into = ((C.c_int32 * k)(), (C.c_void_p * k)(), (C.c_size_t * k)())
        wh, ds, by = self._into
        for i, (which, out, addr) in enumerate(extra):     # further fields of this solve, behind it on the stream
            wh[i], ds[i], by[i] = which, addr, out.nbytes
        stats, used = _capi.Stats(), C.c_int32()
        rc = self._lib.mi_ilqr_solve_into(self._h, ax, au, ac, 1 if pinned else 0, k, wh, ds, by, C.byref(stats), C.byref(used))
        if rc != _capi.OK:
            _capi.check(rc, "mi_ilqr_solve_into")
        self.stats = stats
        if pinned:
            self._sink = bool(used.value)
        if self._md != self.m:
            res[1] = res[1][:, :self.m, :]
        return res

    def solve_resident(self):
        """Solve again from the inputs already resident on the device (no host traffic
        except the aggregate stats): used by bench.py and the on-device MPC loop."""
        stats = _capi.Stats()
        _capi.check(self._lib.mi_ilqr_solve(self._h, C.byref(stats)), "mi_ilqr_solve")
        self.stats = stats
        return stats

    def solve_resident_async(self):
        """Enqueue a solve from the resident inputs on the handle's stream and return at once; up to
        32 may be in flight before `collect(count)` (each keeps its own events and statistics)."""
        _capi.check(self._lib.mi_ilqr_solve_async(self._h), "mi_ilqr_solve_async")

    def collect(self, count=1):
        """Wait for the stream and return the statistics of the last `count` enqueued solves, oldest first."""
        arr = (_capi.Stats * int(count))()
        _capi.check(self._lib.mi_ilqr_collect_stats_n(self._h, int(count), arr), "mi_ilqr_collect_stats_n")
        self.stats = arr[count - 1]
        return list(arr)

    def rearm(self, cold=True):
        if cold:
            _capi.check(self._lib.mi_ilqr_reset(self._h), "mi_ilqr_reset")
        _capi.check(self._lib.mi_ilqr_rearm_initial_guess(self._h), "mi_ilqr_rearm_initial_guess")

    def MPCShift(self, replan_steps):
        """On-device warm start of the receding-horizon loop (acrobot.py:147-152)."""
        _capi.check(self._lib.mi_ilqr_mpc_shift(self._h, int(replan_steps)), "mi_ilqr_mpc_shift")

    def MPCRun(self, num_resolves, replan_steps, target_step=None):
        """The receding-horizon loop (acrobot.py:145-155, mini_cheetah.py:190-201) kept on the device:
        num_resolves x { shift warm start; x_nom += target_step; Solve }.  One launch for the
        wave-per-problem and workgroup-per-problem models (the lane-per-problem "throughput" kernels loop on
        the host).  Returns the aggregate stats; `mpc_log` has the per-re-solve record.
        On a solver that holds a plant (SetPlant) this is the CLOSED loop: before every re-solve the plant advances replan_steps
        steps under the policy of the previous solve, and the re-solve starts from the plant's state instead of the prediction
        x_bar[:, replan_steps] (include/mi_ilqr.h: "Closed-loop MPC"); `plant_log` has the plant's record."""
        self._refuse_tracking("MPCRun", self._MOVES_THE_TARGET, target_step is not None)
        ts = None
        steps = None if target_step is None else np.asarray(target_step, dtype=np.float64)
        per_problem = self._per_problem_targets() or (steps is not None and steps.shape == (self.B, self.n) and steps.size != self.n)
        if per_problem:
            # (B, n) steps, or targets that are per-problem already: every problem's target moves by its own row
            self._set_field(_capi.F_TARGET_STEP, np.zeros((self.B, self.n)) if steps is None
                            else np.broadcast_to(steps.reshape((self.n,)) if steps.size == self.n else steps, (self.B, self.n)))
        elif steps is not None:
            ts = _capi.as_f64(steps, (self.n,))
            self.x_nom = np.asarray(self.x_nom, dtype=np.float64) + num_resolves * ts
        stats = _capi.Stats()
        _capi.check(self._lib.mi_ilqr_mpc_run(self._h, int(num_resolves), int(replan_steps), _capi.ptr(ts), C.byref(stats)),
                    "mi_ilqr_mpc_run")
        self._check_internal(self._mpc_done(num_resolves, replan_steps, per_problem, stats))
        return stats

    _MOVES_THE_TARGET = " - it is the reference that moves the target, replan_steps rows per re-solve; target_step must be None"
    _CONSTANT_TARGET = ", and the policy kernels cost a rollout against a constant target only; SetTargetTrajectory(None) first"

    def _mpc_done(self, num_resolves, replan_steps, per_problem, stats=None):
        """What MPCRun and MPCRunMultiStart do behind the loop: read back the per-problem targets as it left them (x_nom_b + step_b
        added num_resolves times), keep the statistics - None: the last re-solve's are collected - and the loop's sizes -> stats."""
        if per_problem:
            self.x_nom = self._fetch(_capi.F_X_NOM, (self.B, self.n))
        if stats is None:
            stats = _capi.Stats()
            _capi.check(self._lib.mi_ilqr_collect_stats(self._h, C.byref(stats)), "mi_ilqr_collect_stats")
        self.stats = stats
        self._mpc_resolves, self._mpc_replan = int(num_resolves), int(replan_steps)
        return stats

    @property
    def mpc_log(self):
        """(B, num_resolves, n+2): x0 of each re-solve | cost | iterations (written by the single-launch kernels, or after each re-solve of the host loop)."""
        out = np.empty((self.B, self._mpc_resolves, self.n + 2), dtype=np.float64)
        _capi.check(self._lib.mi_ilqr_get_mpc_log(self._h, _capi.ptr(out), out.nbytes), "mi_ilqr_get_mpc_log")
        return out

    def SetTargetStateResident(self, x_nom):
        """Moving target between resident re-solves (mini_cheetah.py:151-156)."""
        self.SetTargetState(x_nom)
        if self._per_problem_targets():
            self._set_field(_capi.F_X_NOM, self.x_nom)
            return
        xn = _capi.as_f64(self.x_nom, (self.n,))
        _capi.check(self._lib.mi_ilqr_set_cost(self._h, None, None, None, _capi.ptr(xn)), "mi_ilqr_set_cost")

    # ------------------------------------------------------------- stage-level entries
    def stage_rollout(self, eps):
        self._push_problem()
        eps = np.ascontiguousarray(np.broadcast_to(np.asarray(eps, dtype=np.float64), (self.B,)))
        _capi.check(self._lib.mi_ilqr_rollout(self._h, _capi.ptr(eps)), "mi_ilqr_rollout")
        tc = self._get(_capi.F_TRIAL_COST, (self.B, 2))
        return (self._get(_capi.F_X_TRIAL, (self.B, self.n, self.N)),
                self._get(_capi.F_U_TRIAL, (self.B, self.m, self.N - 1)), tc[:, 0], tc[:, 1])

    def stage_forward(self, L_last):
        self._push_problem()
        L_last = np.ascontiguousarray(np.broadcast_to(np.asarray(L_last, dtype=np.float64), (self.B,)))
        _capi.check(self._lib.mi_ilqr_forward(self._h, _capi.ptr(L_last)), "mi_ilqr_forward")
        h = self.history[:, 0, :]
        return h[:, 0], h[:, 1], h[:, 2].astype(int)

    def stage_linearize(self):
        self._push_problem()
        _capi.check(self._lib.mi_ilqr_linearize(self._h), "mi_ilqr_linearize")

    def stage_backward(self):
        self._push_problem()
        _capi.check(self._lib.mi_ilqr_backward(self._h), "mi_ilqr_backward")

    # ------------------------------------------------------------- Monte-Carlo rollouts of the policy
    def RolloutPolicy(self, x0, params=None, trajectories=False, *, state_noise=None, control_noise=None, seed=0, first_sample=0,
                      common_noise=False):
        """Roll out S samples per problem under the policy the solver holds - u = u_bar - K (x - x_bar), the reason SaveSolution
        stores K (ilqr.py:712-733) - one GPU lane per sample, in one call (include/mi_ilqr.h: mi_ilqr_policy_rollout).
        x0: (B, S, n), or (S, n) for every problem.  params: None - each problem's own plant - or (B, S, n_params) / (S, n_params),
        a plant per sample.  Costs, targets and control limits are the solver's, per-problem where set.  Returns a PolicyRollout:
        cost (B, S) - +inf for a sample that ended at an infeasible or non-finite step -, x_final (B, S, n), steps (B, S) and, with
        trajectories=True, X (B, S, n, N) and U (B, S, m, N-1) with NaN in the columns a sample did not reach.  Changes nothing in
        the solver: a Solve() after the call is the Solve() without it.
        state_noise (scalar, (n,) or (B, n)) and control_noise (scalar, (m,) or (B, m)): standard deviations of a disturbance at every
        step, x_{t+1} = f(x_t, u_t + sigma_u xi) + sigma_x xi' with independent standard normals generated on the device - U and the
        cost keep the commanded u_t, X holds the noisy states.  A normal depends on (seed, problem, first_sample + sample, step,
        component) only: the same seed gives the same rollouts, S samples from first_sample = k are samples k .. k + S - 1 of one
        long call, common_noise=True gives every problem the same disturbances.  Both None: no noise, today's kernel."""
        x0, params = check_rollout_args(x0, params, self.B, self.n, int(self.system.params.size))
        noisy = state_noise is not None or control_noise is not None
        rows, stream = check_noise_args(state_noise, control_noise, seed, first_sample, common_noise, self.B, self.n, self.m,
                                        self._md if noisy else None, x0.shape[1] if noisy else None)
        self._refuse_tracking("RolloutPolicy", self._CONSTANT_TARGET)
        self._push_costs()
        self._set_policy_noise(rows, stream)
        B, S = self.B, x0.shape[1]
        cost, x_final, steps = np.empty((B, S)), np.empty((B, S, self.n)), np.empty((B, S), dtype=np.int32)
        X = np.empty((B, S, self.n, self.N)) if trajectories else None
        U = np.empty((B, S, self._md, self.N - 1)) if trajectories else None
        _capi.check(self._lib.mi_ilqr_policy_rollout(self._h, S, _capi.ptr(x0), _capi.ptr(params), _capi.ptr(cost), _capi.ptr(x_final),
                                                     _capi.ptr(steps), _capi.ptr(X), _capi.ptr(U)), "mi_ilqr_policy_rollout")
        if U is not None and self._md != self.m:
            U = np.ascontiguousarray(U[:, :, :self.m, :])
        return PolicyRollout(cost, x_final, steps, X, U)

    def _set_policy_noise(self, rows, stream):
        """The disturbances of the next policy launch: the stream always, the sigma rows or - None - their absence."""
        self._send(_capi.F_POLICY_STREAM, stream)
        if rows is not None or getattr(self, "_policy_noise_set", False):
            self._send(_capi.F_POLICY_NOISE, rows)
            self._policy_noise_set = rows is not None

    def RolloutPolicyStats(self, S, x0_mean, x0_spread, *, x0_dist="normal", params_mean=None, params_spread=None, params_dist="uniform",
                           goal=None, state_noise=None, control_noise=None, seed=0, first_sample=0, common_noise=False, samples=False,
                           envelope=False, controls=False, safe_box=None):
        """Monte-Carlo evaluation of the policy the solver holds, entirely on the device (include/mi_ilqr.h: "Monte-Carlo on the
        device"): S samples per problem are DRAWN there - x0 = x0_mean + x0_spread o d with d standard normal (x0_dist="normal") or
        uniform in (-1, 1) ("uniform"), and with params_mean / params_spread / params_dist the plants' parameters likewise -, rolled
        out as RolloutPolicy rolls them out (state_noise, control_noise, seed, first_sample, common_noise: as there) and REDUCED
        there: a PolicyStats of (B,) arrays comes back, nothing of size S crosses the bus.  Means, spreads and goal: (k,) or (B, k).
        A sample is counted iff it ran to the end with a finite cost; success also asks |x_final - x_nom| <= goal component by
        component (goal None: success = counted).  A draw depends on (seed, problem, first_sample + s, component) only: windows of one
        sample set, split over calls with first_sample, are put together with PolicyStats.merge.  samples=True also returns every
        sample's x0, params, cost and steps (PolicyStats.samples) - what RolloutPolicy reproduces: the same arithmetic up to the
        compiler's FMA contraction, bit for bit on the models DESIGN 4.2h lists as measured.  Changes nothing in
        the solver.
        envelope=True / controls=True: the result's `envelope` / `control_envelope` is a PolicyEnvelope, the per-step statistics of the
        states (B, N, n) / the commanded controls (B, N-1, m) over the samples; safe_box=(lo, hi), each None or (n,) / (B, n) with
        +-inf for no bound: its `safety` is a PolicySafety, the samples that stay inside the box and the step at which the others
        first leave it (include/mi_ilqr.h: "Envelopes and a safety box").  All reduced on the device from the trajectories
        RolloutPolicy(trajectories=True) returns for the same samples; the three default to off, cost nothing then, and the solver's
        box and observe settings are after the call what they were before it."""
        n_params = int(self.system.params.size)
        rows, run = check_mc_args(S, x0_mean, x0_spread, self.B, self.n, n_params, x0_dist=x0_dist, params_mean=params_mean,
                                  params_spread=params_spread, params_dist=params_dist, goal=goal, samples=samples, first_sample=first_sample)
        bits, box = check_mc_observe(envelope, controls, safe_box, self.B, self.n)
        noisy = state_noise is not None or control_noise is not None
        noise, stream = check_noise_args(state_noise, control_noise, seed, first_sample, common_noise, self.B, self.n, self.m,
                                         self._md if noisy else None, int(S))
        self._refuse_tracking("RolloutPolicyStats", self._CONSTANT_TARGET)
        self._push_costs()
        self._set_policy_noise(noise, stream)
        self._send(_capi.F_POLICY_MC_DIST, rows)
        before = self._fetch(_capi.F_POLICY_MC_OBSERVE, (1,))
        try:
            if before[0] != bits:
                self._send(_capi.F_POLICY_MC_OBSERVE, np.array([float(bits)]))
            if box is not None:
                self._send(_capi.F_POLICY_MC_BOX, box)
            self._send(_capi.F_POLICY_MC_RUN, run)
        finally:
            if before[0] != bits:
                self._send(_capi.F_POLICY_MC_OBSERVE, np.array([float(before[0])]))
            if box is not None:
                self._send(_capi.F_POLICY_MC_BOX, None)             # (this class leaves no box on the handle between calls)
        out = self._fetch(_capi.F_POLICY_MC_STATS, (self.B, _capi.MC_FIELDS))
        env = cenv = safety = None
        if envelope:
            env = PolicyEnvelope.from_raw(self._fetch(_capi.F_POLICY_MC_ENVELOPE, (self.B, self.N, self.n, _capi.MC_ENV_FIELDS)))
        if controls:
            raw = self._fetch(_capi.F_POLICY_MC_ENVELOPE_U, (self.B, self.N - 1, self._md, _capi.MC_ENV_FIELDS))
            cenv = PolicyEnvelope.from_raw(raw[:, :, :self.m])
        if box is not None:
            safety = PolicySafety.from_rows(np.full(self.B, int(S), dtype=np.int64), self._fetch(_capi.F_POLICY_MC_SAFETY, (self.B, 3 + self.N)))
        smp = None
        if samples:
            n = self.n
            raw = self._fetch(_capi.F_POLICY_MC_SAMPLES, (self.B, int(S), n + n_params + 2))
            smp = PolicySamples(np.ascontiguousarray(raw[:, :, :n]),
                                np.ascontiguousarray(raw[:, :, n:n + n_params]) if params_mean is not None else None,
                                np.ascontiguousarray(raw[:, :, n + n_params]), raw[:, :, n + n_params + 1].astype(np.int32))
        st = PolicyStats.from_rows(out, smp)
        st.envelope, st.control_envelope, st.safety = env, cenv, safety
        return st

    # ------------------------------------------------------------- the plant of the closed MPC loop
    def SetPlant(self, x, params=None, *, state_noise=None, control_noise=None, seed=0, common_noise=False, feedback=True, clock=0):
        """Give every problem a plant of its own: from now on MPCRun is the closed loop (include/mi_ilqr.h: "Closed-loop MPC").
        x: (B, n) states, or (n,) for every problem.  params: None - problem b's own model parameters - or (B, n_params) / (n_params,),
        the TRUE plants the controller's model differs from.  state_noise (scalar, (n,) or (B, n)) and control_noise (scalar, (m,) or
        (B, m)): standard deviations of a disturbance at every plant step, x+ = f(x, u + sigma_u xi) + sigma_x xi'; a normal depends
        on (seed, problem, plant clock, component) only - it is the one sample 0 of RolloutPolicy gets at that step -, common_noise=True
        gives every problem the same disturbances.  feedback=False: the plant gets u_bar alone.  clock: the plant's step counter, which
        MPCRun advances (plant_clock).  Survives Reset(); ClearPlant() returns to the open loop."""
        x, params, noise, stream = check_plant_args(x, params, state_noise, control_noise, seed, common_noise, feedback, clock, self.B, self.n,
                                                    self.m, int(self.system.params.size), self._md)
        self._refuse_tracking("SetPlant", ", and the plant kernels know constant targets only; SetTargetTrajectory(None) first")
        if int(self.system.params.size):
            self._send(_capi.F_PLANT_PARAMS, params)
        self._send(_capi.F_PLANT_NOISE, noise)
        self._send(_capi.F_PLANT_STREAM, stream)
        self._send(_capi.F_PLANT_STATE, x)

    def ClearPlant(self):
        """No plant: MPCRun is the open loop again, bitwise what it is on a solver that never had one."""
        for which in (_capi.F_PLANT_STATE, _capi.F_PLANT_NOISE) + ((_capi.F_PLANT_PARAMS,) if int(self.system.params.size) else ()):
            self._send(which, None)

    @property
    def plant_state(self):
        """(B, n): the plants' current states."""
        return self._fetch(_capi.F_PLANT_STATE, (self.B, self.n))

    @property
    def plant_clock(self):
        """Plant steps taken so far (SetPlant's clock, advanced by every closed-loop MPCRun)."""
        return int(self._fetch(_capi.F_PLANT_STREAM, (4,))[1])

    @property
    def plant_log(self):
        """The record of the last closed-loop MPCRun: a PlantLog."""
        K, n, md = self._mpc_resolves * self._mpc_replan, self.n, self._md
        rows = self._fetch(_capi.F_PLANT_LOG, (self.B, K, n + md + 1))
        X = np.concatenate([np.moveaxis(rows[:, :, :n], 1, 2), self._fetch(_capi.F_PLANT_STATE, (self.B, n))[:, :, None]], axis=2)
        U = np.ascontiguousarray(np.moveaxis(rows[:, :, n:n + self.m], 1, 2))
        steps = (~np.isnan(rows[:, :, n:n + self.m]).any(axis=2)).sum(axis=1).astype(np.int32)
        return PlantLog(X, U, np.ascontiguousarray(rows[:, :, n + md]), steps)

    def plant_kernel_ms(self):
        """Milliseconds of the plant kernels of the last closed-loop MPCRun, summed (HIP events of their own)."""
        return float(self._fetch(_capi.F_PLANT_KERNEL_MS, (1,))[0])

    def policy_mc_passes(self):
        """Passes over windows of sample groups the last RolloutPolicyStats call took (1 unless the samples outgrew the window)."""
        return int(self._fetch(_capi.I_POLICY_MC_PASSES, (1,), np.int32)[0])

    def policy_kernel_ms(self):
        """Milliseconds of the rollout kernel of the last RolloutPolicy call (HIP events of its own)."""
        return float(self._fetch(_capi.F_POLICY_KERNEL_MS, (1,))[0])

    # ------------------------------------------------------------- multi-start (include/mi_ilqr.h: "Multi-start")
    def _seeds_command(self, rows, *command):
        """The sigma_u rows - None: none are sent -, then the command vector to MI_F_SEEDS_RUN -> the library's answer to the command:
        what it means is the caller's to say."""
        if rows is not None:
            self._send(_capi.F_SEEDS_SIGMA, rows)
        v = np.array(command, dtype=np.float64)
        assert v.size in (_capi.SEEDS_RUN_DOUBLES, _capi.SEEDS_MPC_RUN_DOUBLES, _capi.SEEDS_MPPI_RUN_DOUBLES)
        return self._lib.mi_ilqr_set(self._h, _capi.F_SEEDS_RUN, _capi.ptr(v), v.nbytes)

    def _seeds_run(self, op, K, rows=None, seed=0, round=0, hold=1):   # noqa: A002
        rc = self._seeds_command(rows, K, op, seed, round, hold, 0)
        if rc == _capi.E_UNSUPPORTED:
            raise ValueError("multi-start: a solver of at most 4 problems on the wave-per-problem kernels keeps its inputs in host "
                             "memory and has no seed groups to join; use a larger batch")
        _capi.check(rc, "mi_ilqr_set")

    def _seeds_best(self, K):
        return SeedSelection.from_rows(K, self._fetch(_capi.F_SEEDS_BEST, (self.B // K, 3)))

    def PerturbInitialGuess(self, K, sigma_u, seed=0, round=0, hold=1):   # noqa: A002
        """Read the batch as B / K groups of K consecutive problems - the same problem under K guesses - and draw the guesses on
        the device: every member k >= 1 of every group gets base + sigma_u o z, member 0 keeps base (the elite slot: best-of-K is
        never worse than the single start).  base is what the next Solve would have started from: the guess given to
        SetInitialGuess, else the controls the solver holds, else zeros.  z: standard normals of (seed, round, problem, step div
        hold, control) alone; hold > 1 keeps a disturbance over `hold` steps.  sigma_u: scalar, (m,) or (B, m).  The next Solve
        starts cold from these guesses.  Nothing of the size of the guesses crosses the bus."""
        K, rows, seed, round, hold = check_seed_args(K, self.B, self.m, sigma_u, seed, round, hold, self._md)   # noqa: A001
        if rows is None:
            raise ValueError("PerturbInitialGuess: sigma_u is required")
        self._push_problem()                                   # (a guess given to SetInitialGuess is the base)
        self._seeds_run(_capi.SEEDS_PERTURB, K, rows, seed, round, hold)

    def SelectBest(self, K):
        """The best member of every group of K: the eligible one (converged or stopped at max_iters, finite cost) of least cost,
        ties to the lowest index -> SeedSelection.  Reads the last solve's cost and status on the device; changes nothing."""
        K = check_seed_args(K, self.B, self.m, what="SelectBest")[0]
        self._seeds_run(_capi.SEEDS_SELECT, K)
        return self._seeds_best(K)

    def ReseedFromBest(self, K, sigma_u, seed=0, round=0, hold=1):   # noqa: A002
        """SelectBest, then new guesses around the winners: the winner's slot gets its own controls unperturbed, every other member
        of its group the winner's controls + sigma_u o z (PerturbInitialGuess' noise at this `round`).  A group without a winner
        is perturbed around each member's own controls (non-finite entries read as 0).  -> the SeedSelection it used.  The next
        Solve starts cold from these guesses."""
        K, rows, seed, round, hold = check_seed_args(K, self.B, self.m, sigma_u, seed, round, hold, self._md, "ReseedFromBest")   # noqa: A001
        if rows is None:
            raise ValueError("ReseedFromBest: sigma_u is required")
        self._seeds_run(_capi.SEEDS_RESEED, K, rows, seed, round, hold)
        return self._seeds_best(K)

    def GatherBest(self, K):
        """SelectBest, then the winners' results -> (x_bar (G, n, N), u_bar (G, m, N-1), cost (G,), SeedSelection); a group without a
        winner: NaN rows and cost +inf.  Only these G rows cross the bus; changes nothing."""
        K = check_seed_args(K, self.B, self.m, what="GatherBest")[0]
        self._seeds_run(_capi.SEEDS_GATHER, K)
        G = self.B // K
        x, u, c = (self._fetch(which, shape) for which, shape in ((_capi.F_SEEDS_X_BAR, (G, self.n, self.N)),
                                                                  (_capi.F_SEEDS_U_BAR, (G, self._md, self.N - 1)), (_capi.F_SEEDS_COST, (G,))))
        return x, np.ascontiguousarray(u[:, :self.m, :]), c, self._seeds_best(K)

    def SolveMultiStart(self, K, rounds, sigma_u, seed=0, hold=1, shrink=1.0):
        """Multi-start on the device: PerturbInitialGuess -> Solve -> (ReseedFromBest with sigma_u shrink^r at round r -> Solve)
        x (rounds - 1) -> GatherBest.  -> (x_bar (G, n, N), u_bar (G, m, N-1), cost (G,), selections): the winners of the last
        round and the SeedSelection of every round, the last one the gather's."""
        rounds = integer(rounds, "SolveMultiStart", "rounds", 1, None, ">= 1", floats=False)
        if not (isinstance(shrink, (int, float, np.integer, np.floating)) and np.isfinite(shrink) and shrink >= 0.0):
            raise ValueError(f"SolveMultiStart: shrink must be a finite number >= 0; got {shrink!r}")
        sigma = check_seed_args(K, self.B, self.m, sigma_u, seed, 0, hold, self._md, "SolveMultiStart")[1]
        if sigma is None:
            raise ValueError("SolveMultiStart: sigma_u is required")
        sigma = sigma[:, :self.m]
        selections = []
        self.PerturbInitialGuess(K, sigma, seed, 0, hold)
        self.Solve()
        for r in range(1, rounds):
            selections.append(self.ReseedFromBest(K, sigma * float(shrink) ** r, seed, r, hold))
            self.Solve()
        x, u, c, sel = self.GatherBest(K)
        selections.append(sel)
        return x, u, c, selections

    def MPCRunMultiStart(self, K, num_resolves, replan_steps, sigma_u, seed=0, round=0, hold=1, target_step=None):   # noqa: A002
        """The receding-horizon loop with the seeds of every group joined between its re-solves, on the device (include/mi_ilqr.h:
        "Multi-start in the receding-horizon loop"): num_resolves x { SelectBest; every member of a group gets the winner's plan
        shifted by replan_steps - the members that are not the winner plus sigma_u o z at round + r - and the winner's predicted state
        x_bar[:, replan_steps]; the targets move; Solve }, then one more SelectBest.  A group without a winner continues each
        member's own plan.  The solver must hold a solve.  -> the num_resolves + 1 SeedSelections; `mpc_log` has the per-re-solve
        record, `stats` the last re-solve's.  K = 1 is the plain loop of MPCShift + solve_resident, bitwise.  target_step: as in
        MPCRun, (n,) or (B, n); it is turned into per-problem rows.  On a solver that holds a plant (SetPlant) this is the closed
        loop with ONE plant per group, member 0's: it advances replan_steps steps under the winner's policy, every member re-solves
        from its state, and `plant_log` / `plant_state` report the group's plant in every member's row.
        The sigma_u rows and - with target_step or per-problem targets - the target-step rows are sent before the command, as
        ReseedFromBest sends its rows: when the library then refuses the command for the state of the handle (no solve to select
        on), these two fields keep the new values and a shared target has become per-problem rows; nothing else has changed."""
        what = "MPCRunMultiStart"
        K, rows, seed, round, hold = check_seed_args(K, self.B, self.m, sigma_u, seed, round, hold, self._md, what)   # noqa: A001
        if rows is None:
            raise ValueError(f"{what}: sigma_u is required")
        num_resolves = integer(num_resolves, what, "num_resolves", 1, 1 << 31, f"in [1, {1 << 31})", floats=False)
        replan_steps = integer(replan_steps, what, "replan_steps", 1, self.N - 1, f"in [1, {self.N - 1})", floats=False)
        if round + num_resolves > 1 << 32:
            raise ValueError(f"{what}: round + num_resolves must not exceed 2^32 (re-solve r draws at round + r)")
        self._refuse_tracking(what, self._MOVES_THE_TARGET, target_step is not None)
        steps = None if target_step is None else np.asarray(target_step, dtype=np.float64)
        if steps is not None and steps.shape not in ((self.n,), (self.B, self.n)):
            raise ValueError(f"{what}: target_step must be ({self.n},) or ({self.B}, {self.n}); got {steps.shape}")
        per_problem = self._per_problem_targets() or steps is not None
        if per_problem:                # the long form carries no shared step: every problem's target moves by its own row
            self._set_field(_capi.F_TARGET_STEP, np.zeros((self.B, self.n)) if steps is None else np.broadcast_to(steps, (self.B, self.n)))
        rc = self._seeds_command(rows, K, _capi.SEEDS_RESEED, seed, round, hold, 0, num_resolves, replan_steps)
        if rc == _capi.E_UNSUPPORTED:
            raise ValueError(f"{what}: not on this solver - at most 4 problems on the wave-per-problem kernels keep their inputs in "
                             "host memory and have no seed groups to join")
        if rc == _capi.E_BAD_ARG:      # (the arguments were checked above: what is left is the state of the handle)
            raise ValueError(f"{what}: the solver holds no solve to select on (Solve() first; a reseed or a Reset() since then leaves "
                             "none), or the reference's clock would pass its end")
        _capi.check(rc, "mi_ilqr_set")
        self._check_internal(self._mpc_done(num_resolves, replan_steps, per_problem))
        log = self._fetch(_capi.F_SEEDS_BEST, (num_resolves + 1, self.B // K, 3))
        return [SeedSelection.from_rows(K, log[r]) for r in range(num_resolves + 1)]

    def mpc_winner_log(self, selections):
        """(G, R, n + 2): for re-solve r the `mpc_log` row x0 | cost | iterations of the member that selection r + 1 names - the
        trajectory of each group's best -, NaN where no member won.  selections: what MPCRunMultiStart returned."""
        R = self._mpc_resolves
        if len(selections) != R + 1:
            raise ValueError(f"mpc_winner_log: {R + 1} selections belong to the last run of {R} re-solves; got {len(selections)}")
        log = self.mpc_log
        out = np.full((selections[0].winner.size, R, self.n + 2), np.nan)
        for r in range(R):
            p = selections[r + 1].problem
            out[p >= 0, r] = log[p[p >= 0], r]
        return out

    # ------------------------------------------------------------- sampling-based MPC (include/mi_ilqr.h: "Sampling-based MPC")
    def MPPIRun(self, S, iterations, sigma_u, temperature, seed=0, first_sample=0, hold=1, shift=0):
        """MPPI / predictive sampling on the device, the derivative-free counterpart of Solve: every problem improves its own nominal
        plan - what the next Solve would start from: the guess given to SetInitialGuess, else the controls the solver holds, else
        zeros - by `iterations` rounds of { S samples clip(u + sigma_u o z), sample 0 the unperturbed plan; open-loop rollouts costed
        on the applied controls; weights exp(-(cost - best) / temperature) over the samples with a finite cost; their weighted
        mean }.  temperature = 0 takes the best sample alone (the nominal's cost then never rises).  z: standard normals of (seed,
        global sample number first_sample + i S + s, step div hold, problem, control) alone.  sigma_u: scalar, (m,) or (B, m).
        Afterwards the final plans, shifted by `shift` steps as MPCShift shifts, are the pending guess of a cold solver: Solve()
        polishes them, SetInitialState + MPPIRun again is the receding-horizon loop.  -> MPPIResult.  Nothing of size S crosses
        the bus.  Not on a solver that holds a reference trajectory, nor on one of at most 4 problems on the wave-per-problem kernels."""
        S, iterations, rows, temperature, seed, first_sample, hold, shift = check_mppi_args(
            S, iterations, self.B, self.m, self.N, sigma_u, temperature, seed, first_sample, hold, shift, self._md)
        self._push_problem()                                   # (x0, costs, targets; a guess given to SetInitialGuess is the nominal)
        rc = self._seeds_command(rows, S, _capi.SEEDS_RESEED, seed, first_sample, hold, 0, iterations, shift, temperature, 0)
        if rc == _capi.E_UNSUPPORTED:
            raise ValueError("MPPIRun: not on this solver - it holds a reference trajectory (SetTargetTrajectory), or it has at most 4 "
                             "problems on the wave-per-problem kernels, which keep their inputs in host memory; use a larger batch")
        _capi.check(rc, "mi_ilqr_set")
        best = self._fetch(_capi.F_SEEDS_BEST, (iterations, self.B, 3))
        cost = self._fetch(_capi.F_SEEDS_COST, (iterations + 1, self.B, 2))
        u = self._fetch(_capi.F_SEEDS_U_BAR, (self.B, self._md, self.N - 1))
        return MPPIResult.from_rows(np.ascontiguousarray(u[:, :self.m, :]), best, cost, self.seeds_kernel_ms())

    def seeds_kernel_ms(self):
        """Milliseconds of the kernel of the last multi-start command (HIP events of its own)."""
        return float(self._fetch(_capi.F_SEEDS_KERNEL_MS, (1,))[0])

    # ------------------------------------------------------------- parameter identification (include/mi_ilqr.h: "Parameter identification")
    def FitModelParameters(self, x, u, x_next, *, free, count=None, weights=None, params0=None, damping=1e-3, bounds=None, iterations=20,
                           ftol=1e-12, fd_rel=1e-6, fd_floor=1e-8, apply=False):   # noqa: A002
        """From logged transitions to the rows SetModelParameters takes, on the device: every problem b fits the parameters `free`
        (strictly increasing indices, at most 8; the others stay at params0) of its own row to its own transitions x[b, j], u[b, j]
        -> x_next[b, j] - (B, T, n), (B, T, m), (B, T, n); rows need not be consecutive in time - by Levenberg-Marquardt on the
        weighted one-step prediction error sum_j r_j' W r_j, with central differences of the model's step over the parameters
        (steps fd_rel max(|theta_k|, fd_floor)).  count: (B,) the leading rows each problem uses (None: all T; plant_log's `steps`
        goes straight in).  weights: (n,) or (B, n), the diagonal of W (None: ones).  params0: (B, n_params) or (n_params,); None:
        the rows the solver holds (model_params).  damping: the first mu, a scalar or (B,).  bounds: (lo, hi), each (n_params,) or
        None, +-inf allowed: every trial's free entries are clipped into them.  iterations counts trials; a problem stops earlier
        when an accepted trial lowers the cost by no more than ftol times it.  apply=True makes the fitted rows the solver's
        per-problem parameters, exactly as SetModelParameters(fit.params) would; apply=False touches nothing a solve uses.
        -> ParamFit.  Nothing of size T crosses the bus after the upload."""
        np_ = int(self.system.params.size)
        p0 = params0 if params0 is not None or np_ == 0 else self.model_params
        data, wrows, start, brows, run = check_fit_args(x, u, x_next, self.B, self.n, self.m, np_, free=free, params0=p0, count=count,
                                                        weights=weights, damping=damping, bounds=bounds, iterations=iterations, ftol=ftol,
                                                        fd_rel=fd_rel, fd_floor=fd_floor, apply=apply, m_dev=self._md)
        self._send(_capi.F_FIT_DATA, data)
        self._send(_capi.F_FIT_WEIGHTS, wrows)
        self._send(_capi.F_FIT_START, start)
        self._send(_capi.F_FIT_BOUNDS, brows)
        self._send(_capi.F_FIT_RUN, run)
        P = int(run[5])
        return ParamFit.from_rows(self._fetch(_capi.F_FIT_RESULT, (self.B, np_ + _capi.FIT_RESULT_EXTRA)),
                                  self._fetch(_capi.F_FIT_NORMAL, (self.B, P + P * P)), np_, P, self.fit_kernel_ms())

    def fit_kernel_ms(self):
        """Milliseconds of the kernels of the last FitModelParameters call, first to last (HIP events of its own)."""
        return float(self._fetch(_capi.F_FIT_KERNEL_MS, (1,))[0])

    # ------------------------------------------------------------- multi-GPU helper
    def best_cost_allreduce(self):
        """min over all ranks of the best converged cost — the ONE collective of the
        path: a single RCCL all-reduce(min) per batched solve, off
        the per-iteration path.  No-op without an initialized process group."""
        best = float(self.stats.best_cost) if self.stats is not None else float(np.min(self.cost))
        return allreduce_min(best, self._desc.device_id)

    def best_cost_allreduce_async(self):
        """Same collective, non-blocking: returns a handle whose .wait() yields the global best
        cost, so the 8-byte RCCL reduction overlaps the next batched solve."""
        best = float(self.stats.best_cost) if self.stats is not None else float(np.min(self.cost))
        return allreduce_min_async(best, self._desc.device_id)


class IterativeLinearQuadraticRegulator(BatchedIterativeLQR):
    """Drop-in for the reference class (single problem): same constructor signature
    (ilqr.py:21-22), same setters, Solve() -> (x_bar (n,N), u_bar (m,N-1), solve_time,
    cost), SaveSolution(fname)."""

    def __init__(self, system, num_timesteps, input_port_index=0, delta=1e-2, beta=0.95, gamma=0.0,
                 derivs_keypoint_method=None, **device_options):
        self.verbose = device_options.pop("verbose", True)
        # the reference inverts every Quu with np.linalg.inv and never looks at its definiteness (ilqr.py:655): so does the drop-in.
        # `status` then carries STATUS_FLAG_INDEFINITE; on_indefinite="stop" raises RuntimeError at the first such Quu instead.
        device_options.setdefault("on_indefinite", "continue")
        # The reference's loop has no iteration cap (`while improvement > delta`, ilqr.py:692) and prints a row per iteration
        # (:704): so does the drop-in - no cap unless the caller gives `max_iters` (a solve that then runs into it RAISES: it is
        # not a converged one), and a log of 4096 rows (128 KB; `hist_cap`), of which the first 64 ride with the solve and the
        # rest is fetched only after a solve that took more iterations (cart_pole.py's problem takes 108).
        self._capped = "max_iters" in device_options
        device_options.setdefault("max_iters", 2 ** 31 - 1)
        device_options.setdefault("hist_cap", 4096)
        hc = min(int(device_options["hist_cap"]), self._LOG_ROWS_WITH_SOLVE)
        # what Solve() copies out behind the solve besides x_bar / u_bar / cost (field, shape, dtype)
        self._single_extra = ((_capi.I_ITERS, (1,), np.int32), (_capi.I_STATUS, (1,), np.int32), (_capi.F_HIST, (1, hc, 4), np.float64),
                              (_capi.F_ITER_CYCLES, (1, hc, 4), np.float64), (_capi.I64_STAGE_CYCLES, (1, 4), np.int64))
        super().__init__(system, num_timesteps, 1, input_port_index=input_port_index, delta=delta, beta=beta,
                         gamma=gamma, derivs_keypoint_method=derivs_keypoint_method, **device_options)
        self.x0 = np.zeros(self.n)

    _LOG_ROWS_WITH_SOLVE = 64

    def SetInitialGuess(self, u_guess):
        assert u_guess.shape == (self.m, self.N - 1)          # ilqr.py:155
        self._u_guess = u_guess

    x_bar = property(lambda s: s._get(_capi.F_X_BAR, (s.n, s.N)))
    u_bar = property(lambda s: s._get(_capi.F_U_BAR, (s.m, s.N - 1)))
    K = property(lambda s: s._get(_capi.F_K, (s.m, s.n, s.N - 1)))
    kappa = property(lambda s: s._get(_capi.F_KAPPA, (s.m, s.N - 1)))
    dV_coeff = property(lambda s: s._get(_capi.F_DV, (s.N - 1,)))
    fx = property(lambda s: s._get(_capi.F_FX, (s.n, s.n, s.N - 1)))
    fu = property(lambda s: s._get(_capi.F_FU, (s.n, s.m, s.N - 1)))

    @property
    def percentage_derivs(self):
        return float(self.keypoint_count[0]) / (self.N - 1) * 100.0

    def Solve(self):
        st = time.time()
        self._push_problem()
        res = None
        if self._pinned is not None:
            # ONE host synchronization for the whole call: results into page-locked arrays (by the kernel itself where it
            # can), the iteration log and the stopwatches copied out behind the solve on the same stream
            small = [(k,) + self._out_addr(k, shp, dt) for k, shp, dt in self._single_extra]
            res = self._solve_into_pinned(extra=small)
            stats = self.stats
            iters, status, hist, iter_cyc, loop_cycles = int(small[0][1][0]), int(small[1][1][0]), small[2][1][0], small[3][1][0], float(small[4][1][0, 3])
        else:
            stats = _capi.Stats()
            _capi.check(self._lib.mi_ilqr_solve(self._h, C.byref(stats)), "mi_ilqr_solve")
            self.stats = stats
            iters, status = int(self.iterations[0]), int(self.status[0])
            r0 = max(1, min(iters, self.hist_cap))
            # (the leading rows of the per-iteration records: mi_ilqr.h, partial reads of MI_F_HIST / MI_F_ITER_CYCLES)
            hist, iter_cyc = self._fetch(_capi.F_HIST, (r0, 4)), self._fetch(_capi.F_ITER_CYCLES, (r0, 4))
            loop_cycles = float(self.stage_cycles[0, 3])
        total_time = time.time() - st
        self.solve_wall_s = total_time
        # the reference's stopwatches (ilqr.py:364-372,696-702) from the in-kernel cycle counters, PER ITERATION:
        # cycles of the whole solve loop (stage_cycles[3]) span the kernel's HIP-event time
        sec_per_cycle = stats.kernel_ms * 1e-3 / max(loop_cycles, 1.0)
        rows = min(iters, self.hist_cap)
        if rows > len(hist):                                          # a long solve: the rest of the log (the reference prints every row, ilqr.py:704)
            hist, iter_cyc = self._fetch(_capi.F_HIST, (rows, 4)), self._fetch(_capi.F_ITER_CYCLES, (rows, 4))
        t_iter = iter_cyc[:rows] * sec_per_cycle                      # columns: fp (line search), derivs, bp, iteration
        if rows:                                                      # like the reference: the LAST iteration's stopwatches
            self.time_fp, self.time_getDerivs, self.time_backwardsPass = (float(v) for v in t_iter[-1, :3])
        if self.verbose:
            # same table as ilqr.py:685-704
            print("----------------------------------------------------------------------------------------------------------------------------------")
            print("|    iter    |    cost    |    eps    |    ls    | derivs time | derivs '%'  | bp time  | fp time  |   iter time    |    time    |")
            print("----------------------------------------------------------------------------------------------------------------------------------")
            elapsed = 0.0
            for i in range(rows):
                L_new, eps, ls, pct = hist[i]
                t_fp, t_derivs, t_bp, t_it = t_iter[i]
                elapsed += t_it
                print(f"{i + 1:^14}{L_new:11.4f}  {eps:^12.4f}{int(ls):^11}   {t_derivs:1.5f}         {pct:.1f}       "
                      f"{t_bp:1.5f}    {t_fp:1.5f}      {t_it:1.5f}          {elapsed:4.2f}")
            if iters > rows:
                print(f"note: iterations {rows + 1} .. {iters} are not in the log (hist_cap = {self.hist_cap} rows)")
        self.met_indefinite_quu = bool(status & _capi.STATUS_FLAG_INDEFINITE)
        status &= ~_capi.STATUS_FLAG_INDEFINITE
        if self.met_indefinite_quu and self.verbose:
            print("note: a Quu of this solve was not positive definite; inverted like np.linalg.inv (ilqr.py:655) and carried on")
        if status == _capi.STATUS_LINESEARCH_FAILED:
            # ilqr.py:337 reports the trials of the FAILING line search (not the solve's running total): every step
            # size eps = beta^k >= 1e-8 was tried, counted with the reference's own float recurrence (ilqr.py:299-335)
            n_trials, eps = 0, 1.0
            while eps >= 1e-8:
                n_trials += 1
                eps *= self.beta
            raise RuntimeError("linesearch failed after %s iterations" % n_trials)
        if status == _capi.STATUS_INTERNAL:
            raise RuntimeError("solve aborted inside the device kernel (cluster hand-shake lost); results are not a solution")
        if status == _capi.STATUS_MAX_ITERS:
            # the reference has no cap (ilqr.py:692): what a capped solve returns is NOT what the reference would have returned
            raise RuntimeError(f"no convergence after max_iters = {int(self._desc.max_iters)} iterations (improvement still above delta = {self.delta}); "
                               "the state attributes hold the last iterate")
        if status == _capi.STATUS_NOT_PD:
            raise RuntimeError("Quu is not positive definite in the backward pass (indefinite cost expansion, or round-off) and "
                               "on_indefinite=\"stop\" was asked for; the default, \"continue\", inverts it like the reference (ilqr.py:655)")
        if res is not None:
            return res[0].reshape(self.n, self.N), res[1][0], total_time, float(res[2][0])
        return self.x_bar, self.u_bar, total_time, float(self.cost[0])

    def RolloutPolicy(self, x0, params=None, trajectories=False, *, state_noise=None, control_noise=None, seed=0, first_sample=0,
                      common_noise=False):
        """x0 (S, n), params None or (S, n_params): cost (S,), x_final (S, n), steps (S,)[, X (S, n, N), U (S, m, N-1)].
        state_noise scalar or (n,), control_noise scalar or (m,), seed, first_sample, common_noise: BatchedIterativeLQR.RolloutPolicy."""
        if np.ndim(x0) != 2:
            raise ValueError(f"RolloutPolicy: x0 must be (S, {self.n}); got {np.shape(x0)}")
        return super().RolloutPolicy(x0, params, trajectories, state_noise=state_noise, control_noise=control_noise, seed=seed,
                                     first_sample=first_sample, common_noise=common_noise)._without_batch_axis()

    def FitModelParameters(self, x, u, x_next, *, count=None, weights=None, params0=None, damping=1e-3, bounds=None, **kw):
        """x, x_next (T, n), u (T, m), count None or an integer, weights None or (n,), params0 None or (n_params,), damping a scalar:
        BatchedIterativeLQR.FitModelParameters with the leading batch axis dropped, in the arguments and in the ParamFit."""
        for name, v in (("x", x), ("u", u), ("x_next", x_next)):
            if np.ndim(v) != 2:
                raise ValueError(f"FitModelParameters: {name} must be (T, {self.m if name == 'u' else self.n}); got {np.shape(v)}")
        for name, v, nd in (("count", count, 0), ("weights", weights, 1), ("params0", params0, 1), ("damping", damping, 0)):
            if v is not None and np.ndim(v) != nd:
                raise ValueError(f"FitModelParameters: {name} must be {'a scalar' if nd == 0 else 'one row'}; got shape {np.shape(v)}")
        return super().FitModelParameters(np.asarray(x)[None], np.asarray(u)[None], np.asarray(x_next)[None],
                                          count=None if count is None else [count], weights=weights, params0=params0, damping=damping,
                                          bounds=bounds, **kw)._without_batch_axis()

    def SetTargetTrajectory(self, x_ref, clock=0):
        """x_ref (T, n) or None: BatchedIterativeLQR.SetTargetTrajectory."""
        if x_ref is not None and np.ndim(x_ref) != 2:
            raise ValueError(f"SetTargetTrajectory: the reference must be (T, {self.n}); got {np.shape(x_ref)}")
        super().SetTargetTrajectory(x_ref, clock)

    def SetPlant(self, x, params=None, **kw):
        """x (n,), params None or (n_params,), sigmas scalar or (n,) / (m,): BatchedIterativeLQR.SetPlant."""
        if np.ndim(x) != 1:
            raise ValueError(f"SetPlant: x must be ({self.n},); got {np.shape(x)}")
        if params is not None and np.ndim(params) != 1:
            raise ValueError(f"SetPlant: params must be ({int(self.system.params.size)},); got {np.shape(params)}")
        super().SetPlant(x, params, **kw)

    plant_state = property(lambda s: BatchedIterativeLQR.plant_state.fget(s)[0])
    target_trajectory = property(lambda s: (lambda r: None if r is None else r[0])(BatchedIterativeLQR.target_trajectory.fget(s)),
                                 doc="(T, n): the reference the solver holds (SetTargetTrajectory), or None.")
    plant_log = property(lambda s: BatchedIterativeLQR.plant_log.fget(s)._without_batch_axis())

    def SaveSolution(self, fname):
        """ilqr.py:712-733: npz with t, x_bar (last step dropped), u_bar, K."""
        dt = self.system.GetSubsystemByName("plant").time_step()
        T = (self.N - 1) * dt
        t = np.arange(0, T, dt)
        x_bar = self.x_bar[:, :-1]
        np.savez(fname, t=t, x_bar=x_bar, u_bar=self.u_bar, K=self.K)
