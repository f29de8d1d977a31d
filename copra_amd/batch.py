"""BatchLMPC -- host-side handle of one batched LMPC controller (thin ctypes layer over include/copra_hip.h).

Mirrors the call sequence of the reference controller (src/LMPC.cpp): construct with the preview-system dimensions,
costs and constraints (LMPC::LMPC / addCost / addConstraint), hand over A, B, d, x0 for every instance
(PreviewSystem::system), solve() (LMPC::solve), then control() / trajectory() (LMPC.h:108-110).

Arrays given as numpy use natural indexing (A[b] is the nx x nx state matrix of instance b) and are converted to
the ABI layout (column-major per instance).  torch CUDA tensors are used in place and must already be in ABI layout
(i.e. A_abi[b] = A[b].T contiguous); see to_abi_layout().
"""
import ctypes as C

import numpy as np

from . import _args, _capi


def to_abi_layout(A, B, d, x0):
    """numpy (b,nx,nx),(b,nx,nu),(b,nx),(b,nx) natural indexing -> contiguous per-instance column-major arrays"""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    Ab = np.ascontiguousarray(np.transpose(A, (0, 2, 1)))
    Bb = np.ascontiguousarray(np.transpose(B, (0, 2, 1)))
    return Ab, Bb, np.ascontiguousarray(d, dtype=np.float64), np.ascontiguousarray(x0, dtype=np.float64)


class BatchLMPC:
    def __init__(self, nx, nu, N, batch, costs, cstrs, initial_state=None, options=None):
        """initial_state = dict(R=(nx,nx), r=(nx,)) turns the controller into a batched InitialStateLMPC
        (include/InitialStateLMPC.h): decision vector [x0; U], see set_initial_state_bounds / initial_state.
        options: dict of engine options (copra_options_t, include/copra_hip.h; names in _capi.OPTION_NAMES) on top of _capi.OPTIONS --
        they choose which kernels run, never what they compute."""
        self._lib = _capi.lib()
        self.nx, self.nu, self.N, self.batch = int(nx), int(nu), int(N), int(batch)
        self.n = self.nu * self.N
        self.X = self.nx * (self.N + 1)
        self._keep = []
        # The tensors the library reads or writes in place, by slot; a setter fills its slot AFTER the library accepted the call (a refused
        # call leaves the tensors in force alive) and a host copy or None in a tensor's place empties it (_hold).  What else ends a slot:
        #   "system", "x0", "outputs", "tick"   only their own next call
        #   "bias", "noise", "score", "trace"   X(None)
        #   "observer", "target"                X(None); set_shared_system (the library ends both)
        #   ("reference", k)                    set_cost_reference(k, ..); set_reference_schedule(k, ..); set_target(.., costs with k)
        #   ("weights", k)                      set_cost_weights(k, None)
        #   ("schedule", k)                     set_reference_schedule(k, None); set_cost_reference(k, ..)
        #   ("limit", k)                        set_constraint_schedule(k, None); set_constraint_rhs(k, ..)
        #   ("limit", "bounds")                 set_control_bound_schedule(None, None); set_control_bounds(..)
        self._held = {}
        self._ny = 0  # the observer's number of outputs (set_observer), 0: off
        self._costs = list(costs)  # the cost dicts as given: set_target builds the maps [M N] of the driven costs from them
        cc = _capi.pack_costs(costs, self._keep)
        # rows per cost as created: what a per-instance weight vector holds (None: a dense cost, which the library refuses)
        self._cost_rows = [None if cc[i].kind == _capi.COST_KINDS["dense"] else int(cc[i].rows) for i in range(len(costs))]
        kk = _capi.pack_cstrs(cstrs, self._keep)
        dims = _capi.Dims(self.nx, self.nu, self.N, self.batch)
        self._h = C.c_void_p()
        self.is_initial_state = initial_state is not None
        opts = _capi.make_options(options)
        isd = None
        if self.is_initial_state:
            Rm, rv = _capi.fcol(initial_state["R"]), _capi.fcol(initial_state["r"])
            self._keep.extend([Rm, rv])
            isd = C.byref(_capi.InitialStateDesc(_capi.dptr(Rm), _capi.dptr(rv)))
        _capi.check(self._lib.copra_batch_create_with_options(C.byref(self._h), C.byref(dims), len(costs), cc, len(cstrs), kk, isd,
                                                              C.byref(opts)))

    def _hold(self, slot, *args):
        """slot <- the tensors among the _args.Arg records `args` (one record: its tensor itself); host copies and None only: emptied"""
        owners = [a.owner for a in args if a is not None and a.on_device]
        if owners:
            self._held[slot] = owners[0] if len(args) == 1 else owners
        else:
            self._held.pop(slot, None)

    def _release(self, *slots):
        for slot in slots:
            self._held.pop(slot, None)

    def specialise(self, cache_dir=None, lint=True):
        """compile this controller's shape into its own kernels (hipcc --genco, cached); see copra_batch_specialise.
        lint: every code object -- cached or freshly compiled -- goes through copra_amd/hazard_lint.py BEFORE the library loads it
        (matrix-instruction results read too early on some path of the compiled control flow: a defect of the compiler that round 4
        met in the library's own kernels).  One that fails is deleted by copra_batch_specialise_checked, never loaded, and this
        call raises; the handle is untouched and keeps solving on the library's kernels.  Objects that passed carry a `.lint_ok`
        mark next to them and are not disassembled again."""
        cdir = cache_dir.encode() if cache_dir else None
        if not lint:
            _capi.check(self._lib.copra_batch_specialise(self._h, cdir))
            return
        import os
        from . import hazard_lint
        turned_away = []

        def fingerprint(path):
            import hashlib
            with open(path, "rb") as fh:
                return hashlib.sha256(fh.read()).hexdigest()

        def gate(path, _user):
            path = path.decode()
            mark = path + ".lint_ok"
            if not os.path.exists(hazard_lint.OBJDUMP):
                import warnings
                warnings.warn("copra_batch_specialise: %s is missing, the code object %s is loaded WITHOUT the matrix-instruction hazard check"
                              % (hazard_lint.OBJDUMP, os.path.basename(path)))
                return 0
            # (round-5 advisor: the mark belongs to ONE build of the object -- an object rebuilt under the same name, e.g. by another hipcc, is
            #  disassembled again: the mark holds the checked object's SHA-256)
            try:
                if os.path.exists(mark) and open(mark).read().strip() == fingerprint(path):
                    return 0
            except OSError:
                pass
            try:
                hits = hazard_lint.lint_code_object(path)
            except Exception as e:  # (a code object that cannot be disassembled is not loaded either)
                hits = [repr(e)]
            if hits:
                turned_away.append((os.path.basename(path), hits[0]))
                return 1
            with open(mark, "w") as fh:
                fh.write(fingerprint(path))
            return 0

        cb = _capi.CODE_OBJECT_CHECK(gate)
        rc = self._lib.copra_batch_specialise_checked(self._h, cdir, cb, None)
        if turned_away:
            raise RuntimeError("copra_batch_specialise: the compiled kernels fail the matrix-instruction hazard check (%s: %r); the code object "
                               "was removed without being loaded -- this controller keeps the library's kernels" % turned_away[0])
        _capi.check(rc)

    def layout_info(self):
        """dict(lds_bytes, active_capacity, factor_only, two_tier) of the next solve (copra_batch_layout_info)"""
        v = [C.c_int() for _ in range(4)]
        _capi.check(self._lib.copra_batch_layout_info(self._h, *[C.byref(x) for x in v]))
        return dict(lds_bytes=v[0].value, active_capacity=v[1].value, factor_only=bool(v[2].value), two_tier=bool(v[3].value))

    def lanes_per_instance(self):
        """16 / 32: several small problems per wavefront; 64: one wavefront each; > 64: one workgroup each"""
        return int(self._lib.copra_batch_lanes_per_instance(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.copra_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # PreviewSystem::system for every instance
    def _system(self, what, A, B, d, x0, matrix):
        """the four records of a system and their on_device; host arrays must have the system's shapes (a tensor's shape is not checked)"""
        b, nx, nu = self.batch, self.nx, self.nu
        args = [_args.marshal(a, what, matrix=matrix and i < 2) for i, a in enumerate((A, B, d, x0))]
        on_device, _ = _args.same_way(what, args)
        if not on_device:
            for a, shape in zip(args, ((b, nx, nx), (b, nx, nu), (b, nx), (b, nx))):
                _args.expect(a, shape, what)
        return args, on_device

    def set_system(self, A, B, d, x0):
        args, on_device = self._system("set_system", A, B, d, x0, True)
        _capi.check(self._lib.copra_batch_set_system(self._h, *[a.ptr for a in args], on_device))
        self._hold("system", *args)

    def set_system_rowmajor_async(self, A, B, d, x0, stream=None):
        """torch CUDA tensors in numpy's natural (row-major) indexing, (b,nx,nx), (b,nx,nu), (b,nx), (b,nx): the library
        transposes A and B on `stream` (an integer hipStream_t handle); nothing blocks the host"""
        args, on_device = self._system("set_system_rowmajor_async", A, B, d, x0, False)
        if not on_device:
            raise ValueError("set_system_rowmajor_async: contiguous CUDA float64 tensors are needed")
        _capi.check(self._lib.copra_batch_set_system_rowmajor_async(self._h, *[a.ptr for a in args], C.c_void_p(stream or 0)))
        self._hold("system", *args)

    # PreviewSystem::xInit for every instance
    def set_shared_system(self, A, B, d):
        """Shared-model receding-horizon fast path: ONE system (A (nx,nx), B (nx,nu), d (nx)) for the whole batch;
        the per-instance initial states come from set_x0.  The factorisation is done once, at the next solve()."""
        args = [_args.marshal(np.asarray(a), "set_shared_system", matrix=m) for a, m in ((A, True), (B, True), (d, False))]  # (host only)
        _capi.check(self._lib.copra_batch_set_shared_system(self._h, *[a.ptr for a in args], 0))
        self._ny = 0
        self._release("observer", "target")  # (the library ends the observer and the steady-state targets)

    def set_cost_reference(self, cost_index, p):
        """per-instance reference of cost `cost_index`: p of shape (batch, rows) (numpy, or a torch CUDA tensor used in
        place); p of shape (rows,): ONE new reference for every instance (copra_batch_set_cost_reference_all: copied); None
        restores the controller-wide reference given at creation"""
        k, what = int(cost_index), "set_cost_reference"
        arg = _args.marshal(p, what)
        one = arg is not None and len(arg.shape) == 1
        if arg is not None:
            rows = self._cost_rows[k] if 0 <= k < len(self._cost_rows) else None  # (None: the library refuses the cost)
            if arg.on_device and rows is not None:  # (the kernels read that many doubles from the tensor)
                _args.expect(arg, (rows,) if one else (self.batch, rows), what)
            elif not one and arg.shape[:1] != (self.batch,):
                raise _capi.CopraDomainError("%s: expected (%d, rows), got %s" % (what, self.batch, arg.shape))
        if one:  # (copied also from a tensor: the library waits for its broadcast before it returns)
            _capi.check(self._lib.copra_batch_set_cost_reference_all(self._h, k, arg.ptr, arg.on_device))
            arg = None
        elif arg is None:
            _capi.check(self._lib.copra_batch_set_cost_reference(self._h, k, None, 0))
        else:
            _capi.check(self._lib.copra_batch_set_cost_reference(self._h, k, arg.ptr, arg.on_device))
        self._hold(("reference", k), arg)  # one slot per cost: the previous tensor is released
        self._release(("schedule", k))  # (the library ends the cost's schedule, and takes the cost off the targets' list)

    def cost_reference(self, cost_index):
        """the per-instance reference of cost `cost_index` in force, (batch, rows of the cost), as a numpy copy (copra_batch_get_cost_reference:
        waits for the last tick): what set_target, a schedule's window or set_cost_reference wrote; raises while the controller-wide
        reference given at creation is in force"""
        rows = self._cost_rows[int(cost_index)]
        if rows is None:
            raise _capi.CopraUnsupported("cost_reference: a dense (host-evaluated) cost has no reference p")
        out = np.empty((self.batch, rows))
        _capi.check(self._lib.copra_batch_get_cost_reference(self._h, int(cost_index), out.ctypes.data))
        return out

    def set_reference_schedule(self, cost_index, schedule, rows_per_step, offset=0):
        """The reference of cost `cost_index` follows a signal (copra_batch_set_reference_schedule): schedule of shape (steps, r) -- one for the
        batch -- or (batch, steps, r) -- one per instance --, r = rows_per_step; numpy: copied; a torch CUDA float64 tensor: used in place and
        kept alive, never written.  With S = rows of the cost / r the solve at tick tau reads the blocks min(tau + offset + s, steps - 1),
        s = 0 .. S-1: a reference trajectory has r = nx and S = N + 1, a moving goal S = 1, a TargetCost offset = N.  advance() / rollout()
        move the window by one step per tick, on the device (schedule_tick(), schedule_seek()).  None ends the schedule and keeps the last
        window; set_cost_reference on that cost ends it too."""
        k, r = int(cost_index), int(rows_per_step)
        if schedule is None:
            _capi.check(self._lib.copra_batch_set_reference_schedule(self._h, k, None, 0, 0, 0, 0, 0))
            self._release(("schedule", k))
            return
        arg, steps, per = _args.signal(schedule, r, self.batch, False, "set_reference_schedule")
        _capi.check(self._lib.copra_batch_set_reference_schedule(self._h, k, arg.ptr, steps, r, int(offset), per, arg.on_device))
        self._release(("reference", k))  # (the cost's reference is the library's window now)
        self._hold(("schedule", k), arg)

    def set_constraint_schedule(self, cstr_index, schedule, rows_per_step, offset=0, preview=True):
        """The right-hand side f of the Trajectory / Control / Mixed constraint `cstr_index` follows a signal (copra_batch_set_constraint_schedule):
        schedule of shape (steps, r) -- one for the batch -- or (batch, steps, r) -- one per instance --, r = rows_per_step (the rows of a per-step
        constraint; a divisor of the rows of a full-size one); numpy: copied; a torch CUDA float64 tensor: used in place and kept alive, never
        written.  The solve at tick tau reads, for the S steps of the constraint, the blocks min(tau + offset + s, steps - 1) -- preview=True: the
        horizon sees the future limits -- or block min(tau + offset, steps - 1) at every step (preview=False).  advance() / rollout() move the
        window by one step per tick, on the device.  None ends the schedule and keeps the last window; set_constraint_rhs on that constraint
        ends it too."""
        k, r = int(cstr_index), int(rows_per_step)
        if schedule is None:
            _capi.check(self._lib.copra_batch_set_constraint_schedule(self._h, k, None, 0, 0, 0, 0, 0, 0))
            self._release(("limit", k))
            return
        arg, steps, per = _args.signal(schedule, r, self.batch, False, "set_constraint_schedule")
        _capi.check(self._lib.copra_batch_set_constraint_schedule(self._h, k, arg.ptr, steps, r, int(offset), 1 if preview else 0, per, arg.on_device))
        self._hold(("limit", k), arg)

    def set_control_bound_schedule(self, lower, upper, offset=0, preview=True):
        """The bounds of the controller's ControlBoundConstraint follow two signals (copra_batch_set_control_bound_schedule): lower and upper of
        shape (steps, nu) or (batch, steps, nu), both numpy (copied) or both torch CUDA float64 tensors (used in place and kept alive); infinite
        entries are allowed.  Windows and `preview` as in set_constraint_schedule, with the N steps of the horizon.  None, None ends the
        schedule and keeps the last window; set_control_bounds ends it too."""
        if lower is None and upper is None:
            _capi.check(self._lib.copra_batch_set_control_bound_schedule(self._h, None, None, 0, 0, 0, 0, 0))
            self._release(("limit", "bounds"))
            return
        what = "set_control_bound_schedule"
        if lower is None or upper is None:
            raise ValueError("%s: both of lower and upper are needed (None, None ends the schedule)" % what)
        lo, steps, per = _args.signal(lower, self.nu, self.batch, False, what)
        up, steps_u, per_u = _args.signal(upper, self.nu, self.batch, False, what)
        if steps != steps_u or lo.on_device != up.on_device:
            raise _capi.CopraDomainError("%s: lower and upper differ in shape or in where they live" % what)
        on_device, per = _args.same_way(what, (lo, up), (per, per_u))
        _capi.check(self._lib.copra_batch_set_control_bound_schedule(self._h, lo.ptr, up.ptr, steps, int(offset), 1 if preview else 0, per, on_device))
        self._hold(("limit", "bounds"), lo, up)

    def schedule_seek(self, tick):
        """the controller's tick counter <- tick, the windows of all scheduled costs and limits rewritten (copra_batch_schedule_seek; asynchronous)"""
        _capi.check(self._lib.copra_batch_schedule_seek(self._h, int(tick)))

    def schedule_tick(self):
        """the controller's tick counter: the advances so far, or what schedule_seek set (copra_batch_schedule_tick)"""
        return int(self._lib.copra_batch_schedule_tick(self._h))

    def set_cost_weights(self, cost_index, w):
        """per-instance weights of cost `cost_index` (copra_batch_set_cost_weights): w of shape (batch, rows) with the rows of that
        cost as created (numpy: copied; a torch CUDA float64 tensor: used in place and kept alive -- changing it changes the next
        solve); w of shape (rows,): the same weights for every instance; None restores the weights given at creation"""
        k, what = int(cost_index), "set_cost_weights"
        if w is not None and getattr(w, "ndim", np.ndim(w)) == 1:  # the same weights for every instance: written out
            w = w.unsqueeze(0).expand(self.batch, -1) if _args.is_torch(w) else np.broadcast_to(w, (self.batch, len(w)))
        if _args.is_torch(w):
            w = w.contiguous()  # (a copy where it was not: that copy is what the library reads, and what is kept)
        arg = _args.marshal(w, what)
        if arg is not None and self._cost_rows[k] is not None:  # (the kernels read batch x rows doubles from it)
            _args.expect(arg, (self.batch, self._cost_rows[k]), what)
        _capi.check(self._lib.copra_batch_set_cost_weights(self._h, k, arg and arg.ptr, arg.on_device if arg else 0))
        self._hold(("weights", k), arg)  # one slot per cost: the previous tensor is released

    def set_constraint_rhs(self, cstr_index, f):
        """per-instance right-hand side f (batch, rows) of the Trajectory / Control / Mixed constraint `cstr_index`"""
        arg = _args.marshal(np.asarray(f), "set_constraint_rhs")  # (host only)
        if arg.shape[:1] != (self.batch,):
            raise _capi.CopraDomainError("set_constraint_rhs: expected (%d, rows), got %s" % (self.batch, arg.shape))
        _capi.check(self._lib.copra_batch_set_constraint_rhs(self._h, int(cstr_index), arg.ptr, 0))
        self._release(("limit", int(cstr_index)))  # (the library ends the constraint's schedule)

    def _bounds(self, lower, upper, cols):
        """host copies of lower / upper broadcast to (batch, cols)"""
        return [_args.marshal(np.broadcast_to(a, (self.batch, cols)), "bounds") for a in (lower, upper)]

    def set_control_bounds(self, lower, upper):
        """per-instance ControlBoundConstraint: lower / upper broadcastable to (batch, nu * N)"""
        lo, up = self._bounds(lower, upper, self.n)
        _capi.check(self._lib.copra_batch_set_control_bounds(self._h, lo.ptr, up.ptr, 0))
        self._release(("limit", "bounds"))  # (the library ends the bound schedule)

    def set_x0(self, x0):
        arg = _args.expect(_args.marshal(x0, "set_x0"), (self.batch, self.nx), "set_x0")
        _capi.check(self._lib.copra_batch_set_x0(self._h, arg.ptr, arg.on_device))
        self._hold("x0", arg)

    # InitialStateLMPC::resetInitialStateBounds, per instance
    def set_initial_state_bounds(self, x0lb, x0ub):
        lo, up = self._bounds(x0lb, x0ub, self.nx)
        _capi.check(self._lib.copra_batch_set_initial_state_bounds(self._h, lo.ptr, up.ptr, 0))

    # InitialStateLMPC::initialState()
    def initial_state(self):
        out = np.empty((self.batch, self.nx))
        _capi.check(self._lib.copra_batch_get_initial_state(self._h, out.ctypes.data))
        return out

    def set_outputs(self, control, trajectory, status, iters):
        """torch CUDA tensors (float64 [b,n], float64 [b,X], int32 [b], int32 [b,2]) that receive the results"""
        self._held["outputs"] = (control, trajectory, status, iters)
        _capi.check(self._lib.copra_batch_set_outputs(self._h, control.data_ptr(), trajectory.data_ptr(),
                                                      status.data_ptr(), iters.data_ptr()))

    def set_warm_start(self, on=True):
        """shared-model path: start every solve from the previous solve's active set, moved one step towards the present
        (receding horizon); instances where that set is not dual feasible restart cold.  Same results either way."""
        _capi.check(self._lib.copra_batch_set_warm_start(self._h, 1 if on else 0))

    SOLVERS = {"default": 0, "quadprog_dense": 1, "riccati_ipm": 2}

    def select_solver(self, solver):
        """LMPC::selectQPSolver (src/LMPC.cpp:62-65) for the batch: "default" (the engine picks: condensed
        Goldfarb-Idnani up to 64 variables, the stage-wise Riccati interior-point kernel for long horizons when the
        controller is stage-wise), "quadprog_dense" (always Goldfarb-Idnani: the reference's QuadProgDense arithmetic and
        iteration counts) or "riccati_ipm" (CopraUnsupported when the controller is not stage-wise)."""
        _capi.check(self._lib.copra_batch_select_solver(self._h, self.SOLVERS[solver] if isinstance(solver, str) else int(solver)))

    def solver(self):
        """the solver the next solve() runs: 'quadprog_dense' or 'riccati_ipm'"""
        return {1: "quadprog_dense", 2: "riccati_ipm"}[self._lib.copra_batch_solver_info(self._h)]

    def solve(self, stream=None):
        """LMPC::solve for the whole batch; asynchronous on `stream` (an integer hipStream_t handle or None)"""
        _capi.check(self._lib.copra_batch_solve(self._h, C.c_void_p(stream or 0)))

    # ---- the receding-horizon tick (copra_batch_advance / copra_batch_rollout): u = control().head(nu); x = plant(x, u); xInit(x) ----
    def _device(self, a, shape, what, dtype="float64"):
        """the _args.Arg of `a` on the device (None: None), which must have `shape`: a torch CUDA tensor is used in place, anything else is
        copied to the device (through torch) -- the tick's arrays are device-only"""
        if a is None:
            return None
        arg = _args.marshal(a, what, dtype)
        if not arg.on_device:
            import torch
            arg = _args.marshal(torch.from_numpy(arg.owner).cuda(), what, dtype)
        return _args.expect(arg, shape, what)

    def _output(self, a, shape, what, dtype="float64"):
        """an output of the tick: a torch CUDA tensor written in place; True: one is allocated here"""
        if a is None or a is False:
            return None
        if a is True:
            import torch
            a = torch.empty(tuple(shape), dtype=getattr(torch, dtype), device="cuda")
        elif not _args.is_torch(a):
            raise ValueError("%s: outputs stay on the device -- a torch CUDA tensor (or True: allocated for you)" % what)
        return self._device(a, shape, what, dtype)

    def set_backup_steps(self, steps):
        """backup plans of the tick (copra_batch_set_backup_steps): with steps = K in 1 .. N - 1 the library keeps the controls of horizon steps
        1 .. K of every instance's last successful solve, and a tick without a fresh solution for an instance -- its solve failed, or no solve
        was launched since the last advance() -- applies the next of them before it falls back (fallback_control) or holds the state.
        0: off.  Every call forgets all plans, also with the K in force; set_x0 / set_system do not: call this again for a new episode."""
        _capi.check(self._lib.copra_batch_set_backup_steps(self._h, int(steps)))

    def set_bias_estimator(self, gain):
        """The disturbance estimator of the tick (copra_batch_set_bias_estimator): after every advance() the d of each instance's model moves
        by gain @ (x+ - prediction of the model for the applied control), so a constant load or a mismatched plant no longer leaves an
        offset.  gain of shape (nx,): one diagonal gain for the batch; (batch, nx): one per instance; (nx, nx): one dense gain L in natural
        indexing (transposed here to the ABI's column-major); (batch, nx, nx): one per instance -- with batch == nx a 2-d gain is read as
        (nx, nx).  numpy: copied; a torch CUDA float64 tensor: in ABI layout already, used in place and kept alive.  The estimates live in a
        buffer of the library that becomes the controller's d (bias(), bias_ptr()); a tensor given to set_system is not written.  None
        ends the estimator and keeps the last estimates as d.  set_system while on restarts the estimates from the new d;
        set_shared_system ends the estimator."""
        if gain is None:
            _capi.check(self._lib.copra_batch_set_bias_estimator(self._h, None, 0, 0, 0))
            self._release("bias")
            return
        arg, dense, per = _args.weight(gain, self.nx, self.batch, "set_bias_estimator")
        _capi.check(self._lib.copra_batch_set_bias_estimator(self._h, arg.ptr, dense, per, arg.on_device))
        self._hold("bias", arg)

    def set_bias(self, d):
        """restart the estimates (copra_batch_set_bias): d of shape (batch, nx), numpy (copied) or a torch CUDA float64 tensor (copied on the
        stream of the last tick)"""
        arg = _args.expect(_args.marshal(d, "set_bias"), (self.batch, self.nx), "set_bias")
        _capi.check(self._lib.copra_batch_set_bias(self._h, arg.ptr, arg.on_device))

    def bias(self):
        """the d the next solve reads, (batch, nx), as a numpy copy (copra_batch_get_bias: waits for the last tick): the estimates while the
        estimator is or was on"""
        out = np.empty((self.batch, self.nx))
        _capi.check(self._lib.copra_batch_get_bias(self._h, out.ctypes.data))
        return out

    def bias_ptr(self):
        """device pointer of the d the next solve reads (copra_batch_bias_device)"""
        return int(self._lib.copra_batch_bias_device(self._h) or 0)

    def set_observer(self, C_out, Lx=None, Ld=None):
        """The state observer of the tick (copra_batch_set_observer): output feedback.  From now on the plant keeps a state of its own
        (plant_state(), seeded with the x0 in force) and the controller's x0 is the estimate: after every advance()
          y = C xp+ (+ noise) | y_meas;   xpred = A xhat + B u + d;   xhat+ = xpred + Lx (y - C xpred);   d+ = d + Ld (y - C xpred)
        C_out of shape (ny, nx), Lx and Ld of shape (nx, ny) in natural indexing, or (batch, ny, nx) / (batch, nx, ny): one per instance
        (with one of them per instance, numpy matrices given once are written out per instance; tensors all the same way).  numpy: transposed to the ABI's column-major and copied; torch CUDA float64 tensors: in ABI layout already
        ((.., nx, ny) for C_out, (.., ny, nx) for the gains), used in place and kept alive.  Ld None: a state observer only, d is not touched.
        With Ld the estimates of d live in the library's buffer (bias(), bias_ptr(), set_bias()).  A call while on replaces C and the gains
        and keeps every state; C_out None ends the observer.  Excludes set_bias_estimator; set_shared_system ends it."""
        if C_out is None:
            _capi.check(self._lib.copra_batch_set_observer(self._h, 0, None, None, None, 0, 0))
            self._release("observer")
            self._ny = 0
            return
        if Lx is None:
            raise ValueError("set_observer: C needs a gain Lx")
        b, nx = self.batch, self.nx
        args = [_args.marshal(m, "set_observer", matrix=True) for m in (C_out, Lx, Ld) if m is not None]
        on_device, _ = _args.same_way("set_observer", args)
        if not on_device and any(len(a.shape) == 3 for a in args):  # (one flag covers all three: a matrix given once is written out per instance)
            args = [_args.written_out(a, b) if len(a.shape) == 2 else a for a in args]
        shapes = [a.shape for a in args]
        ny = shapes[0][-2] if len(shapes[0]) >= 2 else 0
        per = int(len(shapes[0]) == 3)
        lead = (b,) if per else ()
        if ny < 1 or shapes != [lead + (ny, nx)] + [lead + (nx, ny)] * (len(args) - 1):
            raise _capi.CopraDomainError("set_observer: expected C %s and gains %s (or one of each per instance), got %s" % ((ny, nx), (nx, ny), shapes))
        _capi.check(self._lib.copra_batch_set_observer(self._h, ny, *[a.ptr for a in args], *[None] * (3 - len(args)), per, on_device))
        self._hold("observer", *args)
        self._ny = ny

    def set_plant_state(self, x):
        """the plant's own state while the observer is or was on (copra_batch_set_plant_state): (batch, nx), numpy (copied) or a torch CUDA
        float64 tensor (copied on the stream of the last tick).  set_x0 sets the estimate; a new episode sets both."""
        arg = _args.expect(_args.marshal(x, "set_plant_state"), (self.batch, self.nx), "set_plant_state")
        _capi.check(self._lib.copra_batch_set_plant_state(self._h, arg.ptr, arg.on_device))

    def plant_state(self):
        """the plant's own state, (batch, nx), as a numpy copy (copra_batch_get_plant_state: waits for the last tick)"""
        out = np.empty((self.batch, self.nx))
        _capi.check(self._lib.copra_batch_get_plant_state(self._h, out.ctypes.data))
        return out

    def plant_state_ptr(self):
        """device pointer of the plant's own state (copra_batch_plant_state_device); 0 while the observer was never on"""
        return int(self._lib.copra_batch_plant_state_device(self._h) or 0)

    def set_noise(self, seed, process=None, sensor=None, first_instance=0):
        """Noise drawn on the device (copra_batch_set_noise): from now on every advance() / tick of rollout() adds process * n to the plant's
        disturbance and, with the observer on, sensor * n to its outputs, n standard normal from a counter-based generator -- the draw of
        instance b at noise tick t depends on (seed, first_instance + b, row, t) alone, so it is the same in any batch, on any shard, and for
        every controller variant run on the same seed; no array of noise is held.  process: standard deviations (nx,) or (batch, nx); sensor:
        (ny,) or (batch, ny) (both the same way); numpy: copied; torch CUDA float64 tensors: used in place and kept alive.  A given
        disturbance / noise is kept and the drawn term added.  Resets noise_tick to 0.  Both None: off."""
        n = _capi.Noise()
        self._lib.copra_noise_init(C.byref(n))
        if process is None and sensor is None:
            _capi.check(self._lib.copra_batch_set_noise(self._h, None))
            self._release("noise")
            return
        pw, pv = _args.marshal(process, "set_noise"), _args.marshal(sensor, "set_noise")
        pers = []
        for arg, rows, what in ((pw, self.nx, "process"), (pv, self._ny, "sensor")):
            if arg is None:
                continue
            if what == "sensor" and rows == 0:
                rows = arg.shape[-1] if arg.shape else 0  # (the observer is off: the library says so)
            pers.append(_args.weight_form(arg.shape, rows, self.batch, "set_noise: " + what, dense_allowed=False)[1])
        n.on_device, n.per_instance = _args.same_way("set_noise", (pw, pv), pers)
        n.seed, n.first_instance = int(seed), int(first_instance)
        n.sigma_w, n.sigma_v = pw and pw.ptr, pv and pv.ptr
        _capi.check(self._lib.copra_batch_set_noise(self._h, C.byref(n)))
        self._hold("noise", pw, pv)

    def noise_seek(self, tick):
        """the noise tick the next advance() draws at (copra_batch_noise_seek)"""
        _capi.check(self._lib.copra_batch_noise_seek(self._h, int(tick)))

    @property
    def noise_tick(self):
        """plant steps since set_noise, or what noise_seek set plus the steps since (copra_batch_noise_tick)"""
        return int(self._lib.copra_batch_noise_tick(self._h))

    def draw_noise(self, tick, stream="process", out=None, hip_stream=None):
        """the noise terms of one noise tick (copra_batch_draw_noise), bit for bit what the plant step of that tick adds: a torch CUDA tensor
        (batch, nx) for stream "process", (batch, ny) for "sensor"; written into `out` if given"""
        if stream not in ("process", "sensor"):
            raise ValueError("draw_noise: stream is 'process' or 'sensor'")
        rows = self.nx if stream == "process" else self._ny
        if out is None:
            import torch
            out = torch.empty((self.batch, rows), dtype=torch.float64, device="cuda")
        arg = self._device(out, (self.batch, rows), "draw_noise out")
        _capi.check(self._lib.copra_batch_draw_noise(self._h, int(tick), 0 if stream == "process" else 1, arg.ptr, C.c_void_p(hip_stream or 0)))
        return arg.owner

    # ---- closed-loop scores (copra_batch_set_score, ABI 14): the tick keeps one record per instance on the device ----
    def set_score(self, state_weights=None, control_weights=None, state_ref=None, state_limits=None, control_limits=None, tol=0.0):
        """Closed-loop scores (copra_batch_set_score): from now on every advance() / tick of rollout() updates one record per instance on the
        device -- jx += e' Qx e with e = x - state_ref at the schedule tick, ju += u' Ru u, the violations of the box limits on the true state
        and the applied control, the ticks held / replayed / on the fallback -- so a closed-loop study needs no x_hist / u_hist.
        state_weights: (nx,) diagonal or (nx, nx) dense, or with a leading batch axis one per instance (a 2-d array with batch == nx is read
        as (nx, nx)); control_weights likewise with nu; one of them dense makes both dense.  state_ref: (nx,) a constant goal, (steps, nx) a
        signal read at min(schedule_tick, steps - 1), (batch, steps, nx) one per instance.  state_limits / control_limits: (lower, upper),
        each (nx,) / (nu,) or with a leading batch axis, or None; infinite entries are allowed.  tol: a tick counts as violating when its
        largest violation exceeds it.  A mix of shared and per-instance arrays is written out per instance here.  numpy: natural indexing,
        copied; torch CUDA float64 tensors (all of them then, all shared or all per instance, dense weights in the ABI's column-major):
        used in place and kept alive.  Zeroes the records.  Every argument None (set_score(None)): scoring ends."""
        xl, xh = state_limits if state_limits is not None else (None, None)
        ul, uh = control_limits if control_limits is not None else (None, None)
        given = dict(qx=state_weights, ru=control_weights, x_ref=state_ref, x_lo=xl, x_hi=xh, u_lo=ul, u_hi=uh)
        if all(v is None for v in given.values()):
            _capi.check(self._lib.copra_batch_set_score(self._h, None))
            self._release("score")
            return
        b, nx, nu, what = self.batch, self.nx, self.nu, "set_score"
        rows = dict(qx=nx, ru=nu, x_lo=nx, x_hi=nx, u_lo=nu, u_hi=nu)
        args, dense, per, steps = {}, {}, {}, 1
        for k, v in given.items():
            if v is None:
                continue
            if k == "x_ref":
                args[k], steps, per[k] = _args.signal(v, nx, b, True, what + ": state_ref")
            else:
                args[k], d, per[k] = _args.weight(v, rows[k], b, "%s: %s" % (what, k), dense_allowed=k in ("qx", "ru"))
                if k in ("qx", "ru"):
                    dense[k] = d
        any_dense, any_per = int(any(dense.values())), int(any(per.values()))
        on_device, _ = _args.same_way(what, args.values())
        if on_device:  # used in place: nothing can be written out
            _args.same_way(what, args.values(), per.values(), ValueError)
            if len(set(dense.values())) > 1:
                raise ValueError("set_score: tensors are used in place -- both weights diagonal or both dense")
        else:  # a diagonal beside a dense weight, an array given once beside per-instance ones: written out
            for k, a in args.items():
                if any_dense and not dense.get(k, 1):
                    a = _args.diagonal_as_dense(a)
                args[k] = _args.written_out(a, b) if any_per and not per[k] else a
        m = _capi.Score()
        self._lib.copra_score_init(C.byref(m))
        for k in given:
            setattr(m, k, args[k].ptr if k in args else None)
        m.dense, m.per_instance, m.on_device = any_dense, any_per, on_device
        m.ref_steps, m.tol = int(steps), float(tol)
        _capi.check(self._lib.copra_batch_set_score(self._h, C.byref(m)))
        self._hold("score", *args.values())

    def reset_score(self):
        """zero the records, in stream order behind the last tick (copra_batch_score_reset): a new episode"""
        _capi.check(self._lib.copra_batch_score_reset(self._h))

    def score(self):
        """the records, one per instance, as a numpy structured array (_capi.SCORE_RECORD_DTYPE: jx, ju, viol_sum, viol_max, peak, ticks, held,
        replayed, fallback, violating, first_violation); waits for the last tick (copra_batch_get_score)"""
        out = np.zeros(self.batch, dtype=_capi.SCORE_RECORD_DTYPE)
        _capi.check(self._lib.copra_batch_get_score(self._h, out.ctypes.data))
        return out

    @property
    def score_ptr(self):
        """device pointer of the records (copra_batch_score_device); 0 while scoring is off"""
        return int(self._lib.copra_batch_score_device(self._h) or 0)

    def score_summary(self):
        """the records reduced over the batch on the device (copra_batch_score_summary; waits for the last tick): for jx, ju, viol_sum, viol_max
        and peak a dict(n, mean, m2, min, max, argmin, argmax) over the finite values (variance = m2 / (n - 1)); the totals ticks, held,
        replayed, fallback, violating; instances_violating and instances_held.  The same records give the same bits."""
        s = _capi.ScoreSummary()
        _capi.check(self._lib.copra_batch_score_summary(self._h, C.byref(s)))
        out = {f: {k: getattr(getattr(s, f), k) for k, _ in _capi.ScoreStat._fields_} for f in ("jx", "ju", "viol_sum", "viol_max", "peak")}
        out.update({k: int(getattr(s, k)) for k in ("ticks", "held", "replayed", "fallback", "violating", "instances_violating", "instances_held")})
        return out

    # ---- ensemble traces (copra_batch_set_trace, ABI 17): every recorded tick reduces the batch to one slot on the device ----
    def set_trace(self, capacity, state=True, control=True, estimate_error=False, state_limits=None, control_limits=None, tol=0.0, every=1):
        """Ensemble traces (copra_batch_set_trace): from now on every advance() / tick of rollout() whose count t since this call (or
        reset_trace()) has t % every == 0 reduces the batch into the next of `capacity` slots on the device -- n, mean, m2, min, max, argmin,
        argmax over the instances of every row of the true state (state), the applied control (control; a held instance has none), the
        estimate minus the plant's state while the observer simulates a plant (estimate_error; empty on other ticks), and, with any limit,
        the tick's largest violation (the score's rule) with the number of instances beyond tol -- so an envelope needs no x_hist / u_hist.
        state_limits / control_limits: (lower, upper), each (nx,) / (nu,), one for the batch, or None; infinite entries are allowed.  numpy:
        copied; torch CUDA float64 tensors (all of them then): used in place and kept alive.  A full trace records nothing further
        (trace_info()["missed"] counts).  set_trace(None): tracing ends."""
        if capacity is None:
            _capi.check(self._lib.copra_batch_set_trace(self._h, None))
            self._release("trace")
            return
        xl, xh = state_limits if state_limits is not None else (None, None)
        ul, uh = control_limits if control_limits is not None else (None, None)
        rows = dict(x_lo=self.nx, x_hi=self.nx, u_lo=self.nu, u_hi=self.nu)
        args = {k: _args.expect(_args.marshal(v, "set_trace: " + k), (rows[k],), "set_trace: " + k)
                for k, v in dict(x_lo=xl, x_hi=xh, u_lo=ul, u_hi=uh).items() if v is not None}
        on_device = _args.same_way("set_trace", args.values())[0] if args else 0
        m = _capi.Trace()
        self._lib.copra_trace_init(C.byref(m))
        for k in rows:
            setattr(m, k, args[k].ptr if k in args else None)
        m.capacity, m.every, m.tol, m.on_device = int(capacity), int(every), float(tol), on_device
        m.what = (_capi.TRACE_X if state else 0) | (_capi.TRACE_U if control else 0) | (_capi.TRACE_ERR if estimate_error else 0)
        _capi.check(self._lib.copra_batch_set_trace(self._h, C.byref(m)))
        self._trace_groups = [(name, n) for name, n, on in (("x", self.nx, state), ("u", self.nu, control), ("err", self.nx, estimate_error)) if on]
        self._trace_viol = bool(args)
        self._hold("trace", *args.values())

    def reset_trace(self):
        """the trace's tick count back to 0, in stream order behind the last tick (copra_batch_trace_reset): the next recorded tick is slot 0"""
        _capi.check(self._lib.copra_batch_trace_reset(self._h))

    def trace_info(self):
        """dict(recorded, missed, rows, slot_bytes) of copra_batch_trace_info: slots written, recordable ticks a full trace let pass, the
        statistics per slot and its size (64 + 56 rows)"""
        rec, mis, rows, size = C.c_longlong(), C.c_longlong(), C.c_int(), C.c_longlong()
        _capi.check(self._lib.copra_batch_trace_info(self._h, C.byref(rec), C.byref(mis), C.byref(rows), C.byref(size)))
        return dict(recorded=rec.value, missed=mis.value, rows=rows.value, slot_bytes=size.value)

    def trace_slots(self):
        """the recorded slots as they lie on the device: a numpy structured array (_capi.trace_slot_dtype(rows): head, stat[rows]); waits for
        the last tick (copra_batch_get_trace)"""
        info = self.trace_info()
        out = np.zeros(info["recorded"], dtype=_capi.trace_slot_dtype(info["rows"]))
        assert out.dtype.itemsize == info["slot_bytes"]
        _capi.check(self._lib.copra_batch_get_trace(self._h, 0, info["recorded"], out.ctypes.data))
        return out

    def trace(self):
        """the trace as a dict: head, a structured array (tick, tau, solved, replayed, fallback, held, violating, reserved) with one entry
        per recorded tick; x, u, err: structured (ticks, rows) arrays of n / mean / m2 / min / max / argmin / argmax for the groups that
        set_trace asked for; viol (ticks,) likewise where limits were given (variance = m2 / (n - 1)).  Waits for the last tick."""
        slots = self.trace_slots()
        out, at = dict(head=slots["head"].copy()), 0
        for name, n in self._trace_groups:
            out[name] = slots["stat"][:, at:at + n].copy()
            at += n
        if self._trace_viol:
            out["viol"] = slots["stat"][:, at].copy()
        return out

    @property
    def trace_ptr(self):
        """device pointer of the slots (copra_batch_trace_device); 0 while tracing is off"""
        return int(self._lib.copra_batch_trace_device(self._h) or 0)

    # ---- trace quantiles (copra_batch_set_trace_quantiles, ABI 18): exact order statistics of every row of a recorded tick ----
    def set_trace_quantiles(self, levels):
        """Trace quantiles (copra_batch_set_trace_quantiles): from now on every recorded tick of the trace in force also selects, for every
        row of its slot and every level p in `levels` (at most 8, each in [0, 1], in any order, repeats allowed), the order statistic
        k = min(n - 1, max(0, ceil(p n) - 1)) of the row's n finite values -- numpy's method="inverted_cdf": 0 the minimum, 1 the maximum, 0.5
        the lower median; NaN for a row without a finite value -- so a percentile band needs no x_hist / u_hist.  Needs set_trace first and
        restarts the trace, so every recorded slot has its quantiles.  None or an empty list ends quantiles and keeps the trace; set_trace
        ends them too."""
        lv = np.zeros(0) if levels is None else np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
        if lv.size == 0:
            _capi.check(self._lib.copra_batch_set_trace_quantiles(self._h, None, 0))
            return
        _capi.check(self._lib.copra_batch_set_trace_quantiles(self._h, lv.ctypes.data_as(C.POINTER(C.c_double)), int(lv.size)))

    def trace_quantiles(self):
        """the quantiles of the recorded ticks as a dict: levels (nq,); x, u, err: (ticks, rows, nq) float64 for the groups set_trace asked
        for; viol (ticks, nq) where limits were given -- the groups trace() returns, slot k of one beside slot k of the other.  Waits for the
        last tick (copra_batch_get_trace_quantiles)."""
        nq, lv = C.c_int(), (C.c_double * _capi.TRACE_QUANT_MAX)()
        _capi.check(self._lib.copra_batch_trace_quantile_info(self._h, C.byref(nq), lv))
        info = self.trace_info()
        flat = np.zeros((info["recorded"], info["rows"], nq.value))
        if flat.size:
            _capi.check(self._lib.copra_batch_get_trace_quantiles(self._h, 0, info["recorded"], flat.ctypes.data))
        out, at = dict(levels=np.array(lv[:nq.value], dtype=np.float64)), 0
        for name, n in self._trace_groups:
            out[name] = flat[:, at:at + n].copy()
            at += n
        if self._trace_viol:
            out["viol"] = flat[:, at].copy()
        return out

    @property
    def trace_quantiles_ptr(self):
        """device pointer of the quantile buffer [capacity][rows][levels] (copra_batch_trace_quantiles_device); 0 while quantiles are off"""
        return int(self._lib.copra_batch_trace_quantiles_device(self._h) or 0)

    # ---- steady-state targets (copra_batch_set_target, ABI 15): the references of the driven costs follow d and a setpoint ----
    def _step_map(self, cost_index):
        """T_c = [M_c N_c] of the step form of cost `cost_index` (natural indexing) and its rows r_c, from the dict the constructor received: a
        per-step entry as it is; of a full-size entry (a reference trajectory: blkdiag of one block) its first block"""
        c = self._costs[cost_index]
        nx, nu, N = self.nx, self.nu, self.N
        if c["kind"] == "dense":  # (no step form: the library refuses it)
            return np.zeros((1, nx + nu)), 1
        M = None if c.get("M") is None else np.atleast_2d(np.asarray(c["M"], dtype=np.float64))
        Nm = None if c.get("N") is None else np.atleast_2d(np.asarray(c["N"], dtype=np.float64))
        R = (M if M is not None else Nm).shape[0]
        r = R
        if M is not None and M.shape[1] != nx:
            steps = N + 1 if c["kind"] == "trajectory" else N
            r = R // steps if R % steps == 0 else R
        elif Nm is not None and Nm.shape[1] != nu:
            r = R // N if R % N == 0 else R
        T = np.zeros((r, nx + nu))
        if M is not None:
            T[:, :nx] = M[:r, :nx]
        if Nm is not None:
            T[:, nx:] = Nm[:r, :nu]
        return T, r

    def set_target(self, outputs, setpoint=None, costs=None, offset=0):
        """Steady-state targets (copra_batch_set_target): from now on every advance() / tick of rollout(), and set_system, set_bias and
        schedule_seek, recompute on the device, per instance, the steady state z = [xs; us] with (A - I) xs + B us = -d and
        outputs @ xs = setpoint, and write M xs + N us into the references of the costs in `costs` -- the references follow the model's d
        (the estimates while the estimator or the observer's Ld is on) and the setpoint, so a constant load leaves no offset.
        outputs: (nu, nx), the controlled outputs H, natural indexing.  setpoint: (nu,) a constant, (steps, nu) a signal read at
        min(schedule_tick + offset, steps - 1), (batch, steps, nu) one per instance.  costs: a list of cost indices; their maps [M N] are
        built from the cost dicts the constructor received.  numpy: copied; torch CUDA float64 tensors (outputs then in the ABI's
        column-major, i.e. outputs.T contiguous, and the setpoint): used in place and kept alive.  An instance whose system is singular
        keeps its references and its z (target_status() == 1).  set_cost_reference / set_reference_schedule on a driven cost takes it off
        the list.  outputs None (set_target(None)) ends the targets and keeps the last references."""
        if outputs is None:
            _capi.check(self._lib.copra_batch_set_target(self._h, None))
            self._release("target")
            return
        b, nx, nu = self.batch, self.nx, self.nu
        if setpoint is None or costs is None:
            raise ValueError("set_target: outputs, setpoint and costs are needed")
        idx = [int(k) for k in costs]
        if not 1 <= len(idx) <= 8:
            raise ValueError("set_target: 1 .. 8 driven costs")
        if any(k < 0 or k >= len(self._costs) for k in idx):
            raise ValueError("set_target: no such cost")
        H = _args.expect(_args.marshal(outputs, "set_target", matrix=True), (nu, nx), "set_target: outputs")
        sp, steps, per = _args.signal(setpoint, nu, b, True, "set_target: setpoint")
        on_device, _ = _args.same_way("set_target", (H, sp))
        if int(offset) < 0:
            raise ValueError("set_target: offset < 0")
        maps, rows = [], []
        for k in idx:
            T, r = self._step_map(k)
            m = np.ascontiguousarray(T.T)  # column-major [r x n]
            if on_device:  # (the maps live where outputs and setpoint do)
                import torch
                m = torch.from_numpy(m).cuda()
            maps.append(_args.marshal(m, "set_target"))
            rows.append(r)
        t = _capi.Target()
        self._lib.copra_target_init(C.byref(t))
        ci, cr, cm = (C.c_int * len(idx))(*idx), (C.c_int * len(idx))(*rows), (C.c_void_p * len(idx))(*[m.ptr for m in maps])
        t.nr, t.H, t.r, t.steps, t.offset, t.per_instance = nu, H.ptr, sp.ptr, int(steps), int(offset), per
        t.n_costs, t.cost_index, t.cost_rows, t.cost_map, t.on_device = len(idx), ci, cr, cm, on_device
        _capi.check(self._lib.copra_batch_set_target(self._h, C.byref(t)))
        self._release(*[("reference", k) for k in idx])  # (the costs' references are the library's now)
        self._hold("target", H, sp, *maps)

    def target(self):
        """the steady states z = [xs; us], (batch, nx + nu), as a numpy copy (copra_batch_get_target: waits for the last tick)"""
        out = np.empty((self.batch, self.nx + self.nu))
        _capi.check(self._lib.copra_batch_get_target(self._h, out.ctypes.data, None))
        return out

    def target_status(self):
        """(batch,) int32: 1 where the last target calculation found the instance's system singular -- its references and its z kept"""
        out = np.empty(self.batch, dtype=np.int32)
        _capi.check(self._lib.copra_batch_get_target(self._h, None, out.ctypes.data))
        return out

    @property
    def target_ptr(self):
        """device pointer of the steady states (copra_batch_target_device); 0 while targets are off"""
        return int(self._lib.copra_batch_target_device(self._h) or 0)

    def _plant_step(self, plant, shared, disturbance, fallback_control, x_out, u_out, status_out, age_out=None, d_out=None, noise=None,
                    y_meas=None, y_out=None, xhat_out=None):
        """(the struct of a tick, {its pointer fields: the _args.Arg behind each, None where not given})"""
        st = _capi.PlantStepObs()
        self._lib.copra_plant_step_obs_init(C.byref(st))
        b, nx, nu = self.batch, self.nx, self.nu
        args = {}
        if plant is not None:
            A, B, d = plant
            lead = () if shared else (b,)
            for name, arr, shape in (("A", A, lead + (nx, nx)), ("B", B, lead + (nu, nx)), ("d", d, lead + (nx,))):
                if arr is not None and not _args.is_torch(arr) and name != "d":  # natural indexing -> the ABI's column-major blocks (torch
                    arr = np.swapaxes(np.asarray(arr, dtype=np.float64), -1, -2)  # tensors are in ABI layout already, as for set_system)
                args[name] = self._device(arr, shape, "plant " + name)  # (some but not all of them: the library's COPRA_ERR_ARG)
            st.shared = 1 if shared else 0
        args["w"] = self._device(disturbance, (b, nx), "disturbance")
        args["fallback_u"] = self._device(fallback_control, (b, nu), "fallback_control")
        args["x_out"] = self._output(x_out, (b, nx), "x_out")
        args["u_out"] = self._output(u_out, (b, nu), "u_out")
        args["status_out"] = self._output(status_out, (b,), "status_out", "int32")
        args["age_out"] = self._output(age_out, (b,), "age_out", "int32")
        args["d_out"] = self._output(d_out, (b, nx), "d_out")
        ny = self._ny  # (the observer's outputs: shapes are known only while it is on)
        if ny == 0 and any(a is not None and a is not False for a in (noise, y_meas, y_out, xhat_out)):
            raise ValueError("noise, y_meas, y_out and xhat_out belong to the observer (set_observer)")
        args["v"] = self._device(noise, (b, ny), "noise")
        args["y_meas"] = self._device(y_meas, (b, ny), "y_meas")
        args["y_out"] = self._output(y_out, (b, ny), "y_out")
        args["xhat_out"] = self._output(xhat_out, (b, nx), "xhat_out")
        return st, args

    @staticmethod
    def _fill(st, args):
        for field, arg in args.items():
            if arg is not None:  # (what is not given stays the null of copra_plant_step_obs_init)
                setattr(st, field, arg.ptr)

    def _ticked(self, args, names):
        """the library took the tick: its tensors are held until the next one; {name: the tensor, None where not asked for}"""
        self._hold("tick", *args.values())
        return {k: args[k] and args[k].owner for k in names}

    OUTS = ("x_out", "u_out", "status_out", "age_out", "d_out", "y_out", "xhat_out")
    HISTS = ("x_hist", "u_hist", "status_hist", "age_hist", "d_hist", "y_hist", "xhat_hist")

    def advance(self, plant=None, shared=False, disturbance=None, fallback_control=None, x_out=None, u_out=None, status_out=None, stream=None,
                age_out=None, d_out=None, noise=None, y_meas=None, y_out=None, xhat_out=None):
        """The second half of a tick (copra_batch_advance): apply the first control of the last solve to the plant and make the result the next
        initial state -- x+ = A x0 + B u + d (+ disturbance) where the solve succeeded (or fallback_control (batch, nu) is given); an instance
        whose solve failed keeps its state otherwise.  Asynchronous on `stream`, behind the solve.
        plant: (A, B, d) -- numpy in natural indexing ((batch, nx, nx), (batch, nx, nu), (batch, nx); with shared=True ONE system (nx, nx),
        (nx, nu), (nx,)): copied to the device; torch CUDA tensors in ABI layout (as set_system): used in place; None: the controller's model.
        x_out / u_out / status_out: torch CUDA tensors (batch, nx) / (batch, nu) / int32 (batch,) that receive copies, or True (allocated
        here).  age_out: int32 (batch,), the same way: where each instance's control came from -- 0 this tick's solve, j >= 1 step j of its
        backup plan (set_backup_steps), _capi.PLAN_FALLBACK (-1) fallback_control, _capi.PLAN_HELD (-2) the state was kept; on a tick without
        a solve status_out is the last solve's and only age_out tells.  Returns dict(x_out, u_out, status_out, age_out) of those tensors
        (None where not asked for).  d_out: (batch, nx), the same way: the disturbance estimates after the tick (set_bias_estimator; not written
        while the estimator is off), returned under "d_out".  The state lives in a buffer of the library afterwards (state(), state_ptr()): a tensor given to set_x0
        is not written.
        With the observer on (set_observer): x_out is the plant's own state; noise (batch, ny) is added to the outputs; y_out (batch, ny) and
        xhat_out (batch, nx) receive the outputs and the new estimates.  y_meas (batch, ny): the measurement of a REAL plant after it applied
        the control -- no plant is simulated, plant_state() is left alone, x_out is not written, plant / disturbance / noise are ignored."""
        st, args = self._plant_step(plant, shared, disturbance, fallback_control, x_out, u_out, status_out, age_out, d_out, noise, y_meas, y_out,
                                    xhat_out)
        self._fill(st, args)
        _capi.check(self._lib.copra_batch_advance(self._h, C.byref(st), C.c_void_p(stream or 0)))
        return self._ticked(args, self.OUTS)

    def rollout(self, ticks, plant=None, shared=False, disturbance=None, fallback_control=None, x_out=None, u_out=None, status_out=None,
                disturbances=None, x_hist=None, u_hist=None, status_hist=None, stream=None, age_out=None, age_hist=None, solve_every=1,
                d_out=None, d_hist=None, noise=None, y_out=None, xhat_out=None, y_hist=None, xhat_hist=None):
        """`ticks` x (solve(), advance(...)) enqueued on `stream` by ONE call (copra_batch_rollout): the closed loop never returns to the host.
        disturbances: (ticks, batch, nx), tick t's replaces `disturbance`; x_hist (ticks + 1, batch, nx) -- [0] is the state the first solve
        read --, u_hist (ticks, batch, nu), status_hist int32 (ticks, batch): torch CUDA tensors written in place, or True (allocated here).
        age_hist int32 (ticks, batch): tick t's age_out (see advance).  solve_every = k > 1: a solve at the ticks t with t % k == 0 only, the
        ticks in between play the backup plan -- needs set_backup_steps(K) with K >= k - 1.
        d_hist (ticks, batch, nx): tick t's d_out, the disturbance estimates the solve of tick t + 1 reads (set_bias_estimator).
        With the observer on (set_observer): x_hist is the plant's own state ([0]: before the first tick); noise (batch, ny), or
        (ticks, batch, ny): tick t's; y_hist (ticks, batch, ny): tick t's outputs; xhat_hist (ticks, batch, nx): the estimate the solve of
        tick t + 1 reads.
        Returns dict(x_hist, u_hist, status_hist, age_hist, d_hist, y_hist, xhat_hist, x_out, u_out, status_out, age_out, d_out, y_out,
        xhat_out)."""
        ticks = int(ticks)
        if ticks < 0:
            raise ValueError("rollout: ticks < 0")
        ny = self._ny
        noise_seq = noise is not None and len(getattr(noise, "shape", ())) == 3
        st, args = self._plant_step(plant, shared, disturbance, fallback_control, x_out, u_out, status_out, age_out, d_out,
                                    None if noise_seq else noise, None, y_out, xhat_out)
        b, nx, nu = self.batch, self.nx, self.nu
        if ny == 0 and any(a is not None and a is not False for a in (y_hist, xhat_hist)):
            raise ValueError("y_hist and xhat_hist belong to the observer (set_observer)")
        args["v_seq"] = self._device(noise if noise_seq else None, (ticks, b, ny), "noise")
        args["y_hist"] = self._output(y_hist, (ticks, b, ny), "y_hist")
        args["xhat_hist"] = self._output(xhat_hist, (ticks, b, nx), "xhat_hist")
        seq = dict(w_seq=self._device(disturbances, (ticks, b, nx), "disturbances"),  # (the call's own arguments, in its order)
                   x_hist=self._output(x_hist, (ticks + 1, b, nx), "x_hist"),
                   u_hist=self._output(u_hist, (ticks, b, nu), "u_hist"),
                   status_hist=self._output(status_hist, (ticks, b), "status_hist", "int32"))
        args["age_hist"] = self._output(age_hist, (ticks, b), "age_hist", "int32")
        st.solve_every = int(solve_every)
        args["d_hist"] = self._output(d_hist, (ticks, b, nx), "d_hist")
        self._fill(st, args)
        _capi.check(self._lib.copra_batch_rollout(self._h, C.byref(st), ticks, *[a and a.ptr for a in seq.values()], C.c_void_p(stream or 0)))
        return self._ticked(dict(args, **seq), self.OUTS + self.HISTS)

    DELAY_MAX = 8  # COPRA_DELAY_MAX

    def set_input_delay(self, steps, u_init=None):
        """Input delay in the tick (copra_batch_set_input_delay): the command a solve issues reaches the plant `steps` = D ticks later, D in
        0 .. DELAY_MAX.  The library queues the D commands already issued, keeps the state at the current tick (delay_state()) and makes
        the controller's x0 (state()) the state PREDICTED for the time the next command will act: the queue applied to the current state
        with the controller's model.  advance() / rollout() then apply the queue's oldest command -- u_out, status_out and age_out describe
        the command that reached the plant -- push the last solve's and predict again, all on the device.  u_init (batch, nu): what the
        plant gets for the first D ticks, numpy (copied) or a torch CUDA float64 tensor (read in stream order); None: zeros.  Every call
        resets the queue; 0 turns delay off.  Schedules and set_target take offset + D in a delayed loop.  Excludes set_backup_steps and
        solve_every > 1."""
        steps = int(steps)
        arg = None if u_init is None or steps == 0 else _args.expect(_args.marshal(u_init, "set_input_delay"), (self.batch, self.nu), "set_input_delay")
        _capi.check(self._lib.copra_batch_set_input_delay(self._h, steps, arg and arg.ptr, arg.on_device if arg else 0))
        self._hold("delay", arg)  # (a tensor is read in stream order: kept until the next call)

    def delay_state(self):
        """the state at the current tick while input delay is on, (batch, nx), as a numpy copy (copra_batch_get_delay_state: waits for the
        last tick): the measured state, or with the observer the estimate"""
        out = np.empty((self.batch, self.nx))
        _capi.check(self._lib.copra_batch_get_delay_state(self._h, out.ctypes.data))
        return out

    def delay_state_ptr(self):
        """device pointer of the state at the current tick (copra_batch_delay_state_device); 0 while input delay is off"""
        return int(self._lib.copra_batch_delay_state_device(self._h) or 0)

    def delay_queue(self):
        """(commands (batch, D, nu), statuses int32 (batch, D)) of the pending commands, OLDEST first, as numpy copies
        (copra_batch_get_delay_queue: waits for the last tick); the command of a failed solve reads NaN"""
        D = int(self._lib.copra_batch_input_delay(self._h))
        q, s = np.empty((self.batch, max(D, 0), self.nu)), np.empty((self.batch, max(D, 0)), dtype=np.int32)
        _capi.check(self._lib.copra_batch_get_delay_queue(self._h, q.ctypes.data, s.ctypes.data))
        return q, s

    def state(self):
        """the controller's current initial states -- what the next solve reads --, (batch, nx), as a numpy copy (copra_batch_get_x0: waits for
        the last tick); while input delay is on (set_input_delay) this is the prediction, delay_state() the state at the current tick"""
        out = np.empty((self.batch, self.nx))
        _capi.check(self._lib.copra_batch_get_x0(self._h, out.ctypes.data))
        return out

    def state_ptr(self):
        """device pointer of the controller's current initial states (copra_batch_x0_device): after advance() a buffer of the library"""
        return int(self._lib.copra_batch_x0_device(self._h) or 0)

    def synchronize(self):
        _capi.check(self._lib.copra_batch_synchronize(self._h))

    def last_solve_seconds(self):
        s = C.c_double()
        _capi.check(self._lib.copra_batch_last_solve_seconds(self._h, C.byref(s)))
        return s.value

    def last_first_tier_seconds(self):
        """device time of the FIRST launch of the last solve (the dominant kernel; what a rocprofv3 kernel trace shows)"""
        s = C.c_double()
        _capi.check(self._lib.copra_batch_last_first_tier_seconds(self._h, C.byref(s)))
        return s.value

    def lane_pass_info(self):
        """(ran, finished): whether the last solve ran the one-instance-per-lane pass in front of the first tier, and how many
        instances ended in it (their unconstrained minimiser violates nothing); waits for the solve"""
        ran, fin = C.c_int(), C.c_int()
        _capi.check(self._lib.copra_batch_lane_pass_info(self._h, C.byref(ran), C.byref(fin)))
        return bool(ran.value), fin.value

    def axis_solver_ran(self):
        """whether the last solve's first kernel was the one-(instance, axis)-per-lane solver (lmpc_axis.hpp): lane_pass_info() then counts
        the instances that ended in IT"""
        ran = C.c_int()
        _capi.check(self._lib.copra_batch_lane_pass_info(self._h, C.byref(ran), None))
        return ran.value == 2

    PHASES = ("preview", "costs", "norms", "cholesky", "inverse_x0", "active_set", "results", "total")

    def enable_phase_profile(self, on=True):
        _capi.check(self._lib.copra_batch_phase_profile(self._h, 1 if on else 0, None))

    def phase_profile(self):
        """per-instance shader-clock cycles of the kernel phases, shape (batch, 8) -- see PHASES"""
        out = np.zeros((self.batch, 8), dtype=np.int64)
        _capi.check(self._lib.copra_batch_phase_profile(self._h, 1, out.ctypes.data))
        return out

    def results(self):
        u = np.empty((self.batch, self.n))
        tr = np.empty((self.batch, self.X))
        st = np.empty(self.batch, dtype=np.int32)
        it = np.empty((self.batch, 2), dtype=np.int32)
        _capi.check(self._lib.copra_batch_get_results(self._h, u.ctypes.data, tr.ctypes.data, st.ctypes.data,
                                                      it.ctypes.data))
        return dict(control=u, trajectory=tr, status=st, iter=it)

    def qp_sizes(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _capi.check(self._lib.copra_batch_qp_sizes(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def dump_qp(self, instance):
        """The dense QP of one instance as LMPC exposes it (LMPC.h:112-127), condensed on the device."""
        n, neq, nineq = self.qp_sizes()
        Q = np.zeros((n, n), order="F")
        c = np.zeros(n)
        Aeq = np.zeros((neq, n), order="F")
        beq = np.zeros(neq)
        Aineq = np.zeros((nineq, n), order="F")
        bineq = np.zeros(nineq)
        lb, ub = np.zeros(n), np.zeros(n)
        _capi.check(self._lib.copra_batch_dump_qp(self._h, instance, Q.ctypes.data, c.ctypes.data, Aeq.ctypes.data,
                                                  beq.ctypes.data, Aineq.ctypes.data, bineq.ctypes.data,
                                                  lb.ctypes.data, ub.ctypes.data))
        return dict(Q=np.array(Q), c=c, Aeq=np.array(Aeq), beq=beq, Aineq=np.array(Aineq), bineq=bineq, lb=lb, ub=ub)


def qp_dense_specialise(n, cache_dir=None):
    """Compile the dense-QP kernels for problems with `n` variables (copra_qp_dense_specialise): later
    qp_solve_dense_batch calls with that n run on them.  Needs hipcc on the machine; cached on disk."""
    _capi.check(_capi.lib().copra_qp_dense_specialise(int(n), cache_dir.encode() if cache_dir else None))


def qp_solve_dense_batch(Q, c, Aeq, beq, Aineq, bineq, XL, XU):
    """Batched QuadProgDenseSolver::SI_solve (src/QuadProgSolver.cpp:54-72) on the GPU; numpy, natural indexing:
    Q (b,n,n), c (b,n), Aeq (b,meq,n) or None, ...  Returns x (b,n), fail (b,), iter (b,2)."""
    L = _capi.lib()
    _capi.apply_default_options()  # (this entry point has no handle: the process-wide defaults steer it)
    Q = np.asarray(Q, dtype=np.float64)
    b, n = Q.shape[0], Q.shape[1]
    Aeq = np.zeros((b, 0, n)) if Aeq is None else np.asarray(Aeq, dtype=np.float64).reshape(b, -1, n)
    Aineq = np.zeros((b, 0, n)) if Aineq is None else np.asarray(Aineq, dtype=np.float64).reshape(b, -1, n)
    beq = np.zeros((b, 0)) if beq is None else np.asarray(beq, dtype=np.float64).reshape(b, -1)
    bineq = np.zeros((b, 0)) if bineq is None else np.asarray(bineq, dtype=np.float64).reshape(b, -1)
    neq, nineq = Aeq.shape[1], Aineq.shape[1]

    def cm(a):
        return np.ascontiguousarray(np.transpose(a, (0, 2, 1)))

    Qb, Aeqb, Aineqb = cm(Q), cm(Aeq), cm(Aineq)
    cb = np.ascontiguousarray(c, dtype=np.float64)
    beqb, bineqb = np.ascontiguousarray(beq), np.ascontiguousarray(bineq)
    XLb, XUb = np.ascontiguousarray(XL, dtype=np.float64), np.ascontiguousarray(XU, dtype=np.float64)
    x = np.full((b, n), np.nan)
    fail = np.full(b, -1, dtype=np.int32)
    it = np.zeros((b, 2), dtype=np.int32)
    _capi.check(L.copra_qp_solve_dense_batch(b, n, neq, nineq, Qb.ctypes.data, cb.ctypes.data, Aeqb.ctypes.data,
                                             beqb.ctypes.data, Aineqb.ctypes.data, bineqb.ctypes.data,
                                             XLb.ctypes.data, XUb.ctypes.data, x.ctypes.data, fail.ctypes.data,
                                             it.ctypes.data, 0, None))
    return x, fail, it
