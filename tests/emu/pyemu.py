"""ctypes front-end of the CPU wave emulator (tests/emu/emu_harness.cpp) -- TEST INFRASTRUCTURE ONLY.

Runs the HIP kernel BODIES (copra_amd/csrc/*.hpp) lane-by-lane on the CPU so that `pytest -m "not gpu"` can compare
the kernel logic with the oracle without a GPU.  Never used by the product path.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "..", ".."))
from copra_amd import _capi  # noqa: E402  (struct definitions only; does not load the HIP library)

_lib = None


def lib():
    global _lib
    if _lib is None:
        import fcntl
        with open(os.path.join(_HERE, ".build.lock"), "w") as lock:  # (pytest -n: one worker builds, the others wait for it)
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-C", _HERE, "libcopra_emu.so"], stdout=subprocess.DEVNULL)
        _lib = C.CDLL(os.path.join(_HERE, "libcopra_emu.so"))
        _lib.emu_lmpc_solve.restype = C.c_int
        _lib.emu_qp_dense.restype = C.c_int
        _lib.emu_lmpc_solve_shared.restype = C.c_int
        _lib.emu_lmpc_solve_riccati.restype = C.c_int
    return _lib


AXIS_FAMILIES = ("first", "first_w", "list", "list_w")  # (axis_builds.hpp: AxisFamily)


def axis_build(nx, nu, N, axis_const, axis_rpa, stage_refs, weights, list_):
    """the build of the (instance, axis)-per-lane solver the library picks for a controller (axis_builds.hpp: pick_axis_build):
    (family, NXA, NU, NMAX, QMAX, EXACT, CT, RPA), or None"""
    out = (C.c_int * 8)()
    if not lib().emu_axis_build(nx, nu, N, int(axis_const), axis_rpa, int(stage_refs), int(weights), int(list_), out):
        return None
    return (AXIS_FAMILIES[out[0]], out[1], out[2], out[3], out[4], bool(out[5]), bool(out[6]), out[7])


def last_axis_run():
    """what the (instance, axis)-per-lane solver of the last lmpc_solve ran: dict(first, second: the builds of its two launches as axis_build
    reports them, listed_first: instances the first launch left to the second, listed_second: instances the second left to the tier), or None:
    the solver did not run"""
    v = (C.c_int * 4)()
    lib().emu_last_axis_run(v)
    if v[0] < 0:
        return None
    picks = []
    for k in (v[0], v[1]):
        out = (C.c_int * 8)()
        assert lib().emu_axis_build_entry(k, out)
        picks.append((AXIS_FAMILIES[out[0]], out[1], out[2], out[3], out[4], bool(out[5]), bool(out[6]), out[7]))
    return dict(first=picks[0], second=picks[1], listed_first=v[2], listed_second=v[3])


TIER_LISTS = ("first", "second", "lane", "lane_shared", "shared")  # (tier_builds.hpp: the lists, as emu_tier_build numbers them)
TIER_STANDINS = ("first_standins", "lane_standins")  # (the emulator's own: what copra_batch_specialise compiles)
TIER_KINDS = ("ric", "tri", "square", "w4", "second", "lane", "lane_shared", "shared_tri", "shared_first", "shared_w4", "shared_tier2")  # (TierKind)


def _tier_entry(v):
    return (TIER_KINDS[v[0]], v[1], v[2], v[3], v[4], v[5], bool(v[6]), bool(v[7]))


def tier_build_entry(list_, k):
    """entry k of a list of tier_builds.hpp, or of the emulator's stand-ins (TIER_STANDINS): (kind, nx, nu, nh, rp, qr, srefs, spec) -- the fields a list
    does not have are zero --, or None"""
    out = (C.c_int * 8)()
    return _tier_entry(out) if lib().emu_tier_build_entry((TIER_LISTS + TIER_STANDINS).index(list_), k, out) else None


def tier_build(list_, nx, nu, N, rmax=0, rfull=0, tri=0, ric=0, q1regs=0, lds_total=0, stage_refs=0, lane_spec=0, tier2=0, specialised=True):
    """the library's pick from a list of tier_builds.hpp (pick_first_tier, pick_second_tier, pick_lane, pick_lane_shared, pick_shared) for a plan with
    these fields, as tier_build_entry reports an entry, or None"""
    f = (C.c_int * 12)(nx, nu, N, rmax, rfull, tri, ric, q1regs, lds_total, stage_refs, lane_spec, tier2)
    out = (C.c_int * 8)()
    return _tier_entry(out) if lib().emu_tier_build(TIER_LISTS.index(list_), f, int(specialised), out) else None


def last_tier_run():
    """what the last lmpc_solve / lmpc_solve_shared ran: dict(first, second, lane, lane_shared, shared, shared_second) of entries as tier_build_entry
    reports them; None: that launch did not run"""
    v = (C.c_int * 54)()
    lib().emu_last_tier_run(v)
    return {name: (_tier_entry(v[9 * i + 1:9 * i + 9]) if v[9 * i] else None)
            for i, name in enumerate(("first", "second", "lane", "lane_shared", "shared", "shared_second"))}


def front_end(A, B, N, costs, cstrs, batch=1, initial_state=None, cost_refs=None, row_rhs=None, bounds=None, cost_weights=None):
    """front_end.hpp on the plan of a controller with these per-solve inputs (arguments as lmpc_solve; A, B: the systems, or None): dict(axis, lane: what
    axis_solver_covers and lane_pass_covers answer, reroute: None, or the (two_tier, dense, lds_total, tri, ric, rcap) of weights_layout, host_plan: the
    fields of the HostPlan weights_layout reads -- dense, safe_two_tier, and (total, tri, ric, rcap) of lds_safe and lds_full)"""
    _sync_options()
    keep = [np.ascontiguousarray(v, dtype=np.float64) if v is not None else None for v in (row_rhs, *(bounds or (None, None)))]
    lib().emu_set_instance_rows(*[_capi.dptr(v) if v is not None else C.c_void_p() for v in keep])
    refs = {int(k): np.ascontiguousarray(v, dtype=np.float64) for k, v in (cost_refs or {}).items()}
    for k in range(8):
        lib().emu_set_cost_reference(k, _capi.dptr(refs[k]) if k in refs else C.c_void_p())
    ws = _set_weights(cost_weights)
    try:
        Ab = Bb = None
        if A is not None:
            Ab, Bb, _, _ = _batchify(A, B, np.zeros(np.asarray(A).shape[-1]), np.zeros(np.asarray(A).shape[-1]))
        nx, nu = (Bb.shape[2], Bb.shape[1]) if A is not None else (None, None)
        cc = _capi.pack_costs(costs, keep)
        kk = _capi.pack_cstrs(cstrs, keep)
        dims = _capi.Dims(nx, nu, N, batch)
        isd = C.c_void_p()
        if initial_state is not None:
            Rm, rv = _capi.fcol(initial_state["R"]), _capi.fcol(initial_state["r"])
            keep.extend([Rm, rv])
            isd = C.byref(_capi.InitialStateDesc(_capi.dptr(Rm), _capi.dptr(rv)))
        out = (C.c_int * 19)()
        rc = lib().emu_front_end(C.byref(dims), len(costs), cc, len(cstrs), kk, isd, _capi.dptr(Ab), _capi.dptr(Bb), out)
        if rc != 0:
            raise RuntimeError("emu_front_end rc=%d" % rc)
        return dict(axis=bool(out[0]), lane=bool(out[1]), reroute=tuple(out[3:9]) if out[2] else None,
                    host_plan=dict(dense=bool(out[9]), safe_two_tier=bool(out[10]), lds_safe=tuple(out[11:15]), lds_full=tuple(out[15:19])))
    finally:
        del ws
        _clear_weights()
        lib().emu_set_instance_rows(C.c_void_p(), C.c_void_p(), C.c_void_p())
        for k in range(8):
            lib().emu_set_cost_reference(k, C.c_void_p())


def _sync_options():
    """hand _capi.OPTIONS (what BatchLMPC would pass to copra_batch_create_with_options) to the harness"""
    o = _capi.make_options()
    lib().emu_set_options(C.byref(o))


def last_lane_hist():
    """histogram (32 bins, the last one open) of the violated-row counts of the instances the last lane pass left to the first tier"""
    out = (C.c_int * 32)()
    lib().emu_last_lane_hist(out)
    return np.array(list(out))


def _set_weights(cost_weights):
    """hand per-instance weights {cost_index: (batch, prows)} to the harness (emu_set_cost_weights); returns the arrays, to be kept alive
    until _clear_weights()"""
    ws = {int(k): np.ascontiguousarray(v, dtype=np.float64) for k, v in (cost_weights or {}).items() if v is not None}
    for k in range(8):
        lib().emu_set_cost_weights(k, _capi.dptr(ws[k]) if k in ws else C.c_void_p())
    return ws


def _clear_weights():
    for k in range(8):
        lib().emu_set_cost_weights(k, C.c_void_p())


def _batchify(A, B, d, x0):
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    if A.ndim == 2:
        A, B = A[None], B[None]
        d, x0 = np.asarray(d, dtype=np.float64)[None], np.asarray(x0, dtype=np.float64)[None]
    # per-instance column-major
    Ab = np.ascontiguousarray(np.transpose(A, (0, 2, 1)))
    Bb = np.ascontiguousarray(np.transpose(B, (0, 2, 1)))
    return Ab, Bb, np.ascontiguousarray(d, dtype=np.float64), np.ascontiguousarray(x0, dtype=np.float64)


def lmpc_solve(A, B, d, x0, N, costs, cstrs, dump_instance=-1, specialised=True, initial_state=None, cost_refs=None,
               row_rhs=None, bounds=None, cost_weights=None):
    """cost_weights: {cost_index: array (batch, prows)} per-instance weights (copra_batch_set_cost_weights), cleared again after the solve"""
    ws = _set_weights(cost_weights)
    try:
        return _lmpc_solve(A, B, d, x0, N, costs, cstrs, dump_instance, specialised, initial_state, cost_refs, row_rhs, bounds, ws)
    finally:
        _clear_weights()


def _lmpc_solve(A, B, d, x0, N, costs, cstrs, dump_instance, specialised, initial_state, cost_refs, row_rhs, bounds, ws):
    """cost_refs: {cost_index: array (batch, rows)} per-instance references (copra_batch_set_cost_reference);
    row_rhs: (batch, mgen) per-instance right-hand sides in stacked row order; bounds: (lower, upper) each (batch, n)"""
    _sync_options()
    rr = None if row_rhs is None else np.ascontiguousarray(row_rhs, dtype=np.float64)
    lo = None if bounds is None else np.ascontiguousarray(bounds[0], dtype=np.float64)
    up = None if bounds is None else np.ascontiguousarray(bounds[1], dtype=np.float64)
    lib().emu_set_instance_rows(_capi.dptr(rr) if rr is not None else C.c_void_p(),
                                _capi.dptr(lo) if lo is not None else C.c_void_p(),
                                _capi.dptr(up) if up is not None else C.c_void_p())
    Ab, Bb, db, xb = _batchify(A, B, d, x0)
    refs = {int(k): np.ascontiguousarray(v, dtype=np.float64) for k, v in (cost_refs or {}).items()}
    for k in range(8):
        lib().emu_set_cost_reference(k, _capi.dptr(refs[k]) if k in refs else C.c_void_p())
    batch, nu, nx = Bb.shape[0], Bb.shape[1], Bb.shape[2]
    for k, w in ws.items():  # (the kernels index [instance][row of the whole reference]: a wrong shape would read past the array)
        rows = np.atleast_1d(np.asarray(costs[k]["p"])).size if k < len(costs) and costs[k].get("p") is not None else w.shape[-1]
        if w.shape != (batch, rows):
            raise ValueError("cost_weights[%d]: shape %r, expected %r" % (k, w.shape, (batch, rows)))
    keep = []
    cc = _capi.pack_costs(costs, keep)
    kk = _capi.pack_cstrs(cstrs, keep)
    dims = _capi.Dims(nx, nu, N, batch)
    sizes = (C.c_int * 9)()
    vp = C.c_void_p
    isd, x0lb, x0ub, x0o = vp(), None, None, None
    if initial_state is not None:
        Rm = _capi.fcol(initial_state["R"])
        rv = _capi.fcol(initial_state["r"])
        keep.extend([Rm, rv])
        isd = _capi.InitialStateDesc(_capi.dptr(Rm), _capi.dptr(rv))
        if initial_state.get("x0lb") is not None:
            x0lb = np.ascontiguousarray(np.broadcast_to(initial_state["x0lb"], (batch, nx)), dtype=np.float64)
            x0ub = np.ascontiguousarray(np.broadcast_to(initial_state["x0ub"], (batch, nx)), dtype=np.float64)
        x0o = np.full((batch, nx), np.nan)
        isd = C.byref(isd)
    rc = lib().emu_lmpc_solve(C.byref(dims), len(costs), cc, len(cstrs), kk, vp(), vp(), vp(), vp(), vp(), vp(), vp(),
                              vp(), -1, vp(), vp(), vp(), vp(), sizes, 0, isd, vp(), vp(), vp())
    if rc == _capi.COPRA_ERR_DOMAIN:
        raise _capi.CopraDomainError("emu")
    if rc == _capi.COPRA_ERR_RUNTIME:
        raise _capi.CopraRuntimeError("emu")
    if rc == _capi.COPRA_ERR_UNSUPPORTED:
        raise _capi.CopraUnsupported("emu")
    n, neq, nineq = sizes[0], sizes[1], sizes[2]  # n = number of decision variables of the QP
    mgen = neq + nineq
    if rr is not None and rr.shape != (batch, mgen):  # (the kernels index [instance][stacked row]: a wrong shape would read past the array)
        raise ValueError("row_rhs: shape %r, expected %r" % (rr.shape, (batch, mgen)))
    if lo is not None and (lo.shape != (batch, nu * N) or up.shape != (batch, nu * N)):
        raise ValueError("bounds: shapes %r and %r, expected %r" % (lo.shape, up.shape, (batch, nu * N)))
    X = nx * (N + 1)
    u = np.full((batch, nu * N), np.nan)
    tr = np.full((batch, X), np.nan)
    st = np.full(batch, -1, dtype=np.int32)
    it = np.zeros((batch, 2), dtype=np.int32)
    dQ = np.zeros((n, n), order="F")
    dc = np.zeros(n)
    dA = np.zeros((max(mgen, 1), n), order="F")
    db_ = np.zeros(max(mgen, 1))
    p = _capi.dptr
    rc = lib().emu_lmpc_solve(C.byref(dims), len(costs), cc, len(cstrs), kk, p(Ab), p(Bb), p(db), p(xb), p(u), p(tr),
                              st.ctypes.data_as(C.POINTER(C.c_int)), it.ctypes.data_as(C.POINTER(C.c_int)),
                              dump_instance, p(dQ), p(dc), p(dA), p(db_), sizes, 1 if specialised else 0, isd,
                              p(x0lb) if x0lb is not None else vp(), p(x0ub) if x0ub is not None else vp(),
                              p(x0o) if x0o is not None else vp())
    if rc == _capi.COPRA_ERR_UNSUPPORTED:
        raise _capi.CopraUnsupported("emu")
    if rc != 0:
        raise RuntimeError("emulator failed rc=%d" % rc)
    out = dict(control=u, trajectory=tr, status=st, iter=it, lds_bytes=sizes[3], overflowed=sizes[4], rcap=sizes[5], factor_only=bool(sizes[6]),
               riccati_factor=bool(sizes[7]), lane_pass_finished=sizes[8])
    if x0o is not None:
        out["x0_opt"] = x0o
    if dump_instance >= 0:
        out.update(Q=np.array(dQ), c=dc, Aeq=np.array(dA[:neq]), beq=db_[:neq], Aineq=np.array(dA[neq:mgen]),
                   bineq=db_[neq:mgen])
    return out


def lmpc_solve_riccati(A, B, d, x0, N, costs, cstrs, initial_state=None, cost_refs=None, row_rhs=None, bounds=None, cost_weights=None):
    """lmpc_riccati.hpp (stage-wise interior-point body) for every instance; returns None when the controller is not
    stage-wise.  Arguments as lmpc_solve.  cost_weights: refused (CopraUnsupported), as copra_batch_solve refuses them for this solver."""
    ws = _set_weights(cost_weights)
    try:
        return _lmpc_solve_riccati(A, B, d, x0, N, costs, cstrs, initial_state, cost_refs, row_rhs, bounds)
    finally:
        del ws
        _clear_weights()


def _lmpc_solve_riccati(A, B, d, x0, N, costs, cstrs, initial_state, cost_refs, row_rhs, bounds):
    _sync_options()
    rr = None if row_rhs is None else np.ascontiguousarray(row_rhs, dtype=np.float64)
    lo = None if bounds is None else np.ascontiguousarray(bounds[0], dtype=np.float64)
    up = None if bounds is None else np.ascontiguousarray(bounds[1], dtype=np.float64)
    vp = C.c_void_p
    p = _capi.dptr
    lib().emu_set_instance_rows(p(rr) if rr is not None else vp(), p(lo) if lo is not None else vp(),
                                p(up) if up is not None else vp())
    Ab, Bb, db, xb = _batchify(A, B, d, x0)
    refs = {int(k): np.ascontiguousarray(v, dtype=np.float64) for k, v in (cost_refs or {}).items()}
    for k in range(8):
        lib().emu_set_cost_reference(k, p(refs[k]) if k in refs else vp())
    batch, nu, nx = Bb.shape[0], Bb.shape[1], Bb.shape[2]
    keep = []
    cc = _capi.pack_costs(costs, keep)
    kk = _capi.pack_cstrs(cstrs, keep)
    dims = _capi.Dims(nx, nu, N, batch)
    isd, x0lb, x0ub, x0o = vp(), None, None, None
    if initial_state is not None:
        Rm = _capi.fcol(initial_state["R"])
        rv = _capi.fcol(initial_state["r"])
        keep.extend([Rm, rv])
        isd = C.byref(_capi.InitialStateDesc(p(Rm), p(rv)))
        if initial_state.get("x0lb") is not None:
            x0lb = np.ascontiguousarray(np.broadcast_to(initial_state["x0lb"], (batch, nx)), dtype=np.float64)
            x0ub = np.ascontiguousarray(np.broadcast_to(initial_state["x0ub"], (batch, nx)), dtype=np.float64)
        x0o = np.full((batch, nx), np.nan)
    u = np.full((batch, nu * N), np.nan)
    tr = np.full((batch, nx * (N + 1)), np.nan)
    st = np.full(batch, -1, dtype=np.int32)
    it = np.zeros((batch, 2), dtype=np.int32)
    nc = (C.c_int * 2)()
    rc = lib().emu_lmpc_solve_riccati(C.byref(dims), len(costs), cc, len(cstrs), kk, p(Ab), p(Bb), p(db), p(xb), p(u),
                                      p(tr), st.ctypes.data_as(C.POINTER(C.c_int)), it.ctypes.data_as(C.POINTER(C.c_int)),
                                      isd, p(x0lb) if x0lb is not None else vp(), p(x0ub) if x0ub is not None else vp(),
                                      p(x0o) if x0o is not None else vp(), nc)
    if rc == -200:
        return None
    if rc == _capi.COPRA_ERR_UNSUPPORTED:
        raise _capi.CopraUnsupported("emu")
    if rc != 0:
        raise RuntimeError("emulator failed rc=%d" % rc)
    out = dict(control=u, trajectory=tr, status=st, iter=it, not_converged=nc[0], lds_resident=bool(nc[1]))
    if x0o is not None:
        out["x0_opt"] = x0o
    return out


WARM_CAP = 32  # plan.hpp::kWarmCap


def lmpc_solve_shared(A, B, d, x0, N, costs, cstrs, warm=None, cost_refs=None, cost_weights=None):
    """cost_weights: refused (CopraUnsupported): the shared model holds the creation weights (copra_batch_set_cost_weights)"""
    ws = _set_weights(cost_weights)
    try:
        return _lmpc_solve_shared(A, B, d, x0, N, costs, cstrs, warm, cost_refs, bool(ws))
    finally:
        del ws
        _clear_weights()


def _lmpc_solve_shared(A, B, d, x0, N, costs, cstrs, warm, cost_refs, weighted):
    """shared-model fast path: ONE system (A, B, d), x0 of shape (batch, nx).  warm: int32 array (batch, WARM_CAP) kept by
    the caller across receding-horizon ticks (initialised to -1): the active set of the previous tick, shifted by one step.
    cost_refs: {cost_index: array (batch, rows)} per-instance references -- the records form with the pass in front only"""
    _sync_options()
    refs = {int(k): np.ascontiguousarray(v, dtype=np.float64) for k, v in (cost_refs or {}).items()}
    for k in range(8):
        lib().emu_set_cost_reference(k, _capi.dptr(refs[k]) if k in refs else C.c_void_p())
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=np.float64)
    batch, nx, nu = x0.shape[0], A.shape[0], B.shape[1]
    keep = []
    cc = _capi.pack_costs(costs, keep)
    kk = _capi.pack_cstrs(cstrs, keep)
    dims = _capi.Dims(nx, nu, N, batch)
    Ac, Bc = np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)  # column-major
    dc = np.ascontiguousarray(d, dtype=np.float64)
    u = np.full((batch, nu * N), np.nan)
    tr = np.full((batch, nx * (N + 1)), np.nan)
    st = np.full(batch, -1, dtype=np.int32)
    it = np.zeros((batch, 2), dtype=np.int32)
    sizes = (C.c_int * 3)()
    p = _capi.dptr
    rc = lib().emu_lmpc_solve_shared(C.byref(dims), len(costs), cc, len(cstrs), kk, p(Ac), p(Bc), p(dc), p(x0), p(u),
                                     p(tr), st.ctypes.data_as(C.POINTER(C.c_int)),
                                     it.ctypes.data_as(C.POINTER(C.c_int)), sizes,
                                     warm.ctypes.data_as(C.POINTER(C.c_int)) if warm is not None else C.c_void_p())
    for k in range(8):
        lib().emu_set_cost_reference(k, C.c_void_p())
    if rc == _capi.COPRA_ERR_UNSUPPORTED and weighted:
        raise _capi.CopraUnsupported("emu")
    if rc != 0:
        raise RuntimeError("emulator failed rc=%d" % rc)
    return dict(control=u, trajectory=tr, status=st, iter=it, overflowed=sizes[0], riccati_factor=bool(sizes[1]), lane_pass_finished=sizes[2])


def qp_dense(Q, c, Aeq, beq, Aineq, bineq, XL, XU):
    """batched: Q (b,n,n), c (b,n), Aeq (b,meq,n) ... natural numpy indexing"""
    _sync_options()
    Q = np.asarray(Q, dtype=np.float64)
    if Q.ndim == 2:
        Q, c, XL, XU = Q[None], np.asarray(c)[None], np.asarray(XL)[None], np.asarray(XU)[None]
        Aeq = None if Aeq is None else np.asarray(Aeq)[None]
        beq = None if beq is None else np.asarray(beq)[None]
        Aineq = None if Aineq is None else np.asarray(Aineq)[None]
        bineq = None if bineq is None else np.asarray(bineq)[None]
    b, n = Q.shape[0], Q.shape[1]
    Aeq = np.zeros((b, 0, n)) if Aeq is None else np.asarray(Aeq, dtype=np.float64).reshape(b, -1, n)
    Aineq = np.zeros((b, 0, n)) if Aineq is None else np.asarray(Aineq, dtype=np.float64).reshape(b, -1, n)
    beq = np.zeros((b, 0)) if beq is None else np.asarray(beq, dtype=np.float64).reshape(b, -1)
    bineq = np.zeros((b, 0)) if bineq is None else np.asarray(bineq, dtype=np.float64).reshape(b, -1)
    neq, nineq = Aeq.shape[1], Aineq.shape[1]
    cm = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 1)))  # per-instance column-major
    Qb, Aeqb, Aineqb = cm(Q), cm(Aeq), cm(Aineq)
    cb = np.ascontiguousarray(c, dtype=np.float64)
    beqb, bineqb = np.ascontiguousarray(beq), np.ascontiguousarray(bineq)
    XLb, XUb = np.ascontiguousarray(XL, dtype=np.float64), np.ascontiguousarray(XU, dtype=np.float64)
    x = np.full((b, n), np.nan)
    fail = np.full(b, -1, dtype=np.int32)
    it = np.zeros((b, 2), dtype=np.int32)
    p = _capi.dptr
    rc = lib().emu_qp_dense(b, n, neq, nineq, p(Qb), p(cb), p(Aeqb), p(beqb), p(Aineqb), p(bineqb), p(XLb), p(XUb),
                            p(x), fail.ctypes.data_as(C.POINTER(C.c_int)), it.ctypes.data_as(C.POINTER(C.c_int)))
    if rc != 0:
        raise RuntimeError("emulator failed rc=%d" % rc)
    return x, fail, it
