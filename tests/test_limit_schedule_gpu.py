"""Limit schedules on the device (copra_batch_set_constraint_schedule / copra_batch_set_control_bound_schedule; BatchLMPC.set_constraint_schedule,
set_control_bound_schedule): moving limits inside rollout, against the CPU oracle tick by tick -- the oracle solves every tick from the state the
DEVICE held at that tick (x_hist[t]) with the windows of that tick stated its way (tests/limit_cases.py), so nothing compounds (the method of
tests/test_reference_schedule_gpu.py::_check_history).

Measures: statuses equal to the oracle's AND all zero (a condition on the inputs, which tests/test_limit_schedule_inputs.py establishes with the
oracle alone); first controls entry-wise 1e-6 with an absolute floor of 1e-3; a plant step within the bound derived in
tests/test_closed_loop_abi.py; the moved share at the last tick at least one half; two routes through the kernels within 1e-9 (ROUTES)."""
import numpy as np
import pytest

import limit_cases as lc
import tracking_cases as tc
from test_closed_loop_abi import reference_step, step_bound

pytestmark = pytest.mark.gpu

RTOL = lc.RTOL
ROUTES = 1e-9
BOTH, V_ONLY, B_ONLY = ("v", "bounds"), ("v",), ("bounds",)


def _workload(name):
    return lc.integrator_limits() if name == "integrator" else lc.com_limits(coupled=name == "coupled")


def _engine(wl, shared_model=False, cstrs=None, **kw):
    from copra_amd import BatchLMPC
    nx, nu, batch = wl["B"].shape[1], wl["B"].shape[2], wl["x0"].shape[0]
    eng = BatchLMPC(nx, nu, wl["N"], batch, wl["costs"], wl["cstrs"] if cstrs is None else cstrs, **kw)
    if shared_model:
        eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
        eng.set_x0(wl["x0"])
    else:
        eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    return eng


def _pick(signal, groups, per_instance):
    """what a setter gets: (steps, r) for the batch, or (batch, steps, r)"""
    return np.ascontiguousarray(signal[groups]) if per_instance else np.ascontiguousarray(signal[0])


def _set_schedules(eng, sig, groups, per_instance, preview, use):
    if "v" in use:
        eng.set_constraint_schedule(0, _pick(sig[lc.vkey(preview, use)], groups, per_instance), 3, preview=preview)
    if "bounds" in use:
        eng.set_control_bound_schedule(_pick(sig["lo"], groups, per_instance), _pick(sig["up"], groups, per_instance), preview=preview)


def _assert_step(x_next, wl, x, u, w, what):
    nx, nu = wl["B"].shape[1], wl["B"].shape[2]
    ref, S = reference_step(wl["A"], wl["B"], wl["d"], x, u, w)
    err = np.abs(x_next.astype(np.longdouble) - ref)
    assert (err <= step_bound(nx, nu, S)).all(), what


def _np(hist):
    return tuple(np.asarray(hist[k].cpu().numpy() if hasattr(hist[k], "cpu") else hist[k]) for k in ("x_hist", "u_hist", "status_hist"))


def _check_history(oracle, wl, sig, groups, hist, w_seq, preview, use, what, p_signals=None, moved_bar=True):
    """every tick of a rollout against the oracle, from the device's x_hist[t] with the windows of tick t; at the last tick the moved windows must
    matter.  p_signals: the reference signals (groups, steps, r) of cost 0 where a reference schedule runs along (S = 1)"""
    xh, uh, sh = _np(hist)
    nu = wl["B"].shape[2]
    ticks = uh.shape[0]
    assert not np.isnan(xh).any() and not np.isnan(uh).any()

    def p_at(t):
        return None if p_signals is None else [tc.window(s, t, 1) for s in p_signals]

    for t in range(ticks):
        ref = lc.oracle_tick(oracle, wl, xh[t], groups, lc.windows_at(wl, sig, t, preview, use), p_at(t))
        assert np.array_equal(sh[t], ref["status"]), (what, t)
        assert (sh[t] == 0).all(), (what, t, np.nonzero(sh[t])[0][:8])
        e = float(tc.rel(uh[t], ref["control"][:, :nu]).max())
        print("%s tick %d: first control against the oracle %.2e" % (what, t, e))
        assert e <= RTOL, (what, t)
        _assert_step(xh[t + 1], wl, xh[t], uh[t], w_seq[t], "%s tick %d" % (what, t))
    last = ticks - 1
    share = lc.moved_share(oracle, wl, xh[last], groups, lc.windows_at(wl, sig, last, preview, use), lc.windows_at(wl, sig, 0, preview, use), nu,
                           p_at(last), p_at(last))
    print("%s: the moved windows change the first control of %.0f %% of the instances at tick %d" % (what, 100 * share, last))
    assert share >= 0.5 or not moved_bar, what


# (workload, which limits move, noise seed) as tests/test_limit_schedule_inputs.py runs them.  The constraint schedule alone WITHOUT preview takes
# the mild velocity signal (limit_cases.V_LIMITS says why: a limit that includes x_0 cannot be ridden while it tightens), which never binds: that
# run is checked against the oracle like the others, only the moved-share bar does not apply to it.
ROLLOUTS = [(name, use, seed, per, preview) for name, use, seed in (("com", BOTH, 31), ("coupled", BOTH, 32), ("integrator", B_ONLY, 33), ("com", V_ONLY, 31),
                                                                   ("com", B_ONLY, 31)) for per in (False, True) for preview in (True, False)]


@pytest.mark.parametrize("name,use,seed,per_instance,preview", ROLLOUTS)
def test_rollout_against_the_oracle(oracle, name, use, seed, per_instance, preview):
    wl, sig = _workload(name)
    groups = lc.group_of(lc.BATCH, per_instance)
    w_seq = lc.noise(wl, seed)
    eng = _engine(wl)
    if name == "integrator":
        assert eng.lanes_per_instance() in (16, 32)
    _set_schedules(eng, sig, groups, per_instance, preview, use)
    hist = eng.rollout(lc.TICKS, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True)
    assert np.array_equal(hist["x_hist"][0].cpu().numpy(), wl["x0"])
    assert eng.schedule_tick() == lc.TICKS
    ran = eng.axis_solver_ran()
    print("%s: the axis solver ran the last tick: %s" % (name, ran))
    if name == "coupled":
        assert not ran
    _check_history(oracle, wl, sig, groups, hist, w_seq, preview, use, "%s %s per instance %d preview %d" % (name, "+".join(use), per_instance, preview),
                   moved_bar=preview or use != V_ONLY)


def _goal_signals(steps):
    """the goal of cost 0 (a per-step TrajectoryCost: r = 6, S = 1) drifts, one signal per group"""
    from copra_amd import workloads
    k = np.arange(steps)[:, None]
    return np.stack([workloads.COM_X_GOAL + k * d * np.array([1.0, -1.0, 0.5, 0.0, 0.0, 0.0]) for d in (0.004, 0.006, -0.004, 0.008)])


def test_limit_and_reference_schedules_together(oracle):
    wl, sig = lc.com_limits()
    groups = lc.group_of(lc.BATCH, True)
    w_seq = lc.noise(wl, 31)
    goals = _goal_signals(sig["up"].shape[1])
    eng = _engine(wl)
    _set_schedules(eng, sig, groups, True, True, BOTH)
    eng.set_reference_schedule(0, np.ascontiguousarray(goals[groups]), 6)
    hist = eng.rollout(lc.TICKS, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True)
    _check_history(oracle, wl, sig, groups, hist, w_seq, True, BOTH, "limits and a reference schedule", p_signals=goals)


def test_bound_schedule_on_a_shared_model(oracle):
    wl, sig = lc.com_limits()
    wl["A"], wl["B"], wl["d"] = (np.ascontiguousarray(np.broadcast_to(wl[k][0], wl[k].shape)) for k in ("A", "B", "d"))
    groups = lc.group_of(lc.BATCH, True)
    w_seq = lc.noise(wl, 31)
    eng = _engine(wl, shared_model=True)
    _set_schedules(eng, sig, groups, True, True, B_ONLY)
    hist = eng.rollout(lc.TICKS, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True)
    _check_history(oracle, wl, sig, groups, hist, w_seq, True, B_ONLY, "shared model, bound schedule")


@pytest.mark.parametrize("preview", [True, False])
@pytest.mark.parametrize("name", ["com", "coupled"])
def test_rollout_is_the_host_loop(name, preview):
    """the same 8 ticks with ONE rollout on the schedules, and with the calls that existed before them on a second controller: per tick
    set_control_bounds(window) and set_constraint_rhs(full window), solve, advance.  That controller is created with the FULL-SIZE
    TrajectoryConstraint, which takes a right-hand side per step.
    Iteration counters of the last tick are compared where both controllers run the same tier: coupled_limits, whose axes are not decoupled, so
    that neither controller runs the axis solver (asserted) and both solve every instance with the active-set kernels of the tiers.  On
    com_limits the scheduled controller keeps the axis solver for its per-step constraint (its counters are that solver's own), so only statuses,
    states and controls are compared there."""
    import torch
    wl, sig = _workload(name)
    N = wl["N"]
    groups = lc.group_of(lc.BATCH, True)
    w_seq = lc.noise(wl, 34)
    wd = torch.from_numpy(w_seq).cuda()
    a = _engine(wl)
    _set_schedules(a, sig, groups, True, preview, BOTH)
    ha = a.rollout(lc.TICKS, disturbances=wd, x_hist=True, u_hist=True, status_hist=True)
    full = [dict(kind="trajectory", E=np.kron(np.eye(N + 1), np.asarray(wl["cstrs"][0]["E"])), f=np.full(3 * (N + 1), lc.V_MILD[0][0])), wl["cstrs"][1]]
    b = _engine(wl, cstrs=full)
    v, lo, up = (_pick(sig[k], groups, True) for k in (lc.vkey(preview, BOTH), "lo", "up"))
    xs, us, ss = [wl["x0"]], [], []
    for t in range(lc.TICKS):
        b.set_control_bounds(lc.window(lo, t, N, preview), lc.window(up, t, N, preview))
        b.set_constraint_rhs(0, lc.window(v, t, N + 1, preview))
        b.solve()
        o = b.advance(disturbance=wd[t], status_out=True, u_out=True)
        ss.append(o["status_out"].cpu().numpy()), us.append(o["u_out"].cpu().numpy()), xs.append(b.state())
    xa, ua, sa = _np(ha)
    assert np.array_equal(sa, np.stack(ss)) and (sa == 0).all()
    dx, du = np.abs(xa - np.stack(xs)).max(), np.abs(ua - np.stack(us)).max()
    print("rollout on the schedules against set_control_bounds + set_constraint_rhs + solve + advance: states %.2e, controls %.2e" % (dx, du))
    assert dx <= ROUTES and du <= ROUTES
    if name == "coupled":
        assert not a.axis_solver_ran() and not b.axis_solver_ran()
        assert np.array_equal(a.results()["iter"], b.results()["iter"])


def test_which_kernels_ran(oracle):
    """preview=False on com_limits: every window is the same along the horizon, the axis solver's register builds take it"""
    from copra_amd import _capi
    import ctypes as C
    wl, sig = lc.com_limits()
    groups = lc.group_of(lc.BATCH, True)
    eng = _engine(wl)
    _set_schedules(eng, sig, groups, True, False, BOTH)
    eng.rollout(2)
    ran, fin = C.c_int(), C.c_int()
    _capi.check(_capi.lib().copra_batch_lane_pass_info(eng._h, C.byref(ran), C.byref(fin)))
    print("preview off: ran %d, finished %d of %d" % (ran.value, fin.value, lc.BATCH))
    assert ran.value == 2 and fin.value > 0


def test_no_axis_solver_on_a_build_that_reads_controller_wide_limits(oracle):
    """jerk_preview(nu = 3, N = 14, a_max = 2.0): two rows per axis and step, whose build of the axis solver reads the controller's limits only.
    With a bound schedule live the solver must stay off; results match the oracle; ending the schedule leaves the handle solvable."""
    from copra_amd import workloads
    wl = workloads.jerk_preview(lc.BATCH, nu=3, N=14, a_max=2.0)
    N = wl["N"]
    steps = 12
    up = np.repeat(lc.ramp(steps, 20.0, 6.0, 8)[:, None], 3, axis=1)
    plain = _engine(wl)
    plain.solve()
    before = plain.axis_solver_ran()
    assert before  # (rpa = 2: the build picked for this shape is not a register build -- without that the guard below is not exercised)
    eng = _engine(wl)
    eng.set_control_bound_schedule(-up, up, preview=True)
    for k in (0, 5):
        eng.schedule_seek(k)
        eng.set_x0(wl["x0"])
        eng.solve()
        assert not eng.axis_solver_ran()
        res = eng.results()
        cstrs = [wl["cstrs"][0], dict(kind="control_bound", lower=-lc.window(up, k, N), upper=lc.window(up, k, N))]
        ref = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], wl["x0"], N, wl["costs"], cstrs, nthreads=8)
        assert np.array_equal(res["status"], ref["status"]) and (res["status"] == 0).all()
        assert float(tc.rel(res["control"], ref["control"]).max()) <= RTOL
    eng.set_control_bound_schedule(None, None)
    eng.set_x0(wl["x0"])
    eng.solve()
    again = eng.results()
    assert np.array_equal(again["status"], res["status"]) and np.abs(again["control"] - res["control"]).max() <= ROUTES


def _solve_at(eng, wl):
    eng.set_x0(wl["x0"])
    eng.solve()
    return eng.results()


def _oracle_at(oracle, wl, sig, groups, k, preview=True, use=BOTH):
    return lc.oracle_tick(oracle, wl, wl["x0"], groups, lc.windows_at(wl, sig, k, preview, use))


def test_seek(oracle):
    wl, sig = lc.com_limits()
    groups = lc.group_of(lc.BATCH, True)
    eng = _engine(wl)
    _set_schedules(eng, sig, groups, True, True, B_ONLY)
    steps = sig["up"].shape[1]
    for k in (0, 6, steps + 5):
        eng.schedule_seek(k)
        assert eng.schedule_tick() == k
        res, ref = _solve_at(eng, wl), _oracle_at(oracle, wl, sig, groups, k, use=B_ONLY)
        assert np.array_equal(res["status"], ref["status"]) and (res["status"] == 0).all(), k
        assert float(tc.rel(res["control"], ref["control"]).max()) <= RTOL, k


def test_ending_and_replacing(oracle):
    wl, sig = lc.com_limits()
    N = wl["N"]
    groups = lc.group_of(lc.BATCH, True)
    eng = _engine(wl)
    _set_schedules(eng, sig, groups, True, True, BOTH)
    eng.schedule_seek(5)
    first = _solve_at(eng, wl)
    # None keeps the last window: ticks do not move it any more
    eng.set_control_bound_schedule(None, None)
    eng.set_constraint_schedule(0, None, 3)
    eng.schedule_seek(1)
    second = _solve_at(eng, wl)
    # (two solves of one controller around its first adaptation decisions agree to rounding, not bit for bit -- include/copra_hip.h documents 1e-11
    #  relative; the bar is the suite's for two routes through the kernels.  The window of tick 1 is another problem by far more than that.)
    d = float(np.abs(first["control"] - second["control"]).max())
    moved = float(np.abs(_oracle_at(oracle, wl, sig, groups, 1)["control"] - second["control"]).max())
    print("the last window is kept: the two solves differ by %.2e; the window of tick 1 would differ by %.2e" % (d, moved))
    assert np.array_equal(first["status"], second["status"]) and d <= ROUTES and moved > 1e-3
    ref = _oracle_at(oracle, wl, sig, groups, 5)
    assert (first["status"] == 0).all() and float(tc.rel(first["control"], ref["control"]).max()) <= RTOL
    # set_control_bounds / set_constraint_rhs after a live schedule take effect, and the later ticks of a rollout use them, not a stale window
    _set_schedules(eng, sig, groups, True, True, BOTH)
    eng.set_control_bounds(-2.5, 2.5)
    eng.set_constraint_rhs(0, np.full((lc.BATCH, 3 * (N + 1)), 0.85))
    eng.set_x0(wl["x0"])
    hist = eng.rollout(3, x_hist=True, u_hist=True, status_hist=True)
    xh, uh, sh = _np(hist)
    fixed = dict(wl, cstrs=[dict(wl["cstrs"][0], f=[0.85] * 3), dict(kind="control_bound", lower=[-2.5] * 3, upper=[2.5] * 3)])
    for t in range(3):
        ref = tc.oracle_tick(oracle, fixed, xh[t], np.zeros(lc.BATCH, dtype=int), [fixed["costs"][0]["p"]])
        assert np.array_equal(sh[t], ref["status"]) and (sh[t] == 0).all(), t
        assert float(tc.rel(uh[t], ref["control"][:, :3]).max()) <= RTOL, t
    # a replacement schedule of a different length
    short = dict(sig, lo=sig["lo"][:, :5], up=sig["up"][:, :5])
    eng.set_constraint_rhs(0, np.full((lc.BATCH, 3 * (N + 1)), lc.V_MILD[0][0]))
    _set_schedules(eng, short, groups, True, True, B_ONLY)
    eng.schedule_seek(9)
    res, ref = _solve_at(eng, wl), _oracle_at(oracle, wl, short, groups, 9, use=B_ONLY)
    assert (res["status"] == 0).all() and float(tc.rel(res["control"], ref["control"]).max()) <= RTOL


def test_error_codes(oracle):
    from copra_amd import BatchLMPC, _capi, workloads
    wl, sig = lc.com_limits(batch=64)
    N = wl["N"]
    eng = _engine(wl)
    L, h = _capi.lib(), eng._h
    v, up = np.ascontiguousarray(sig["v_mild"][0]), np.ascontiguousarray(sig["up"][0])
    lo = np.ascontiguousarray(-up)
    steps = v.shape[0]

    def cs(k, ptr, steps_, r, offset):
        rc = L.copra_batch_set_constraint_schedule(h, k, ptr, steps_, r, offset, 1, 0, 0)
        assert rc == _capi.COPRA_OK or L.copra_last_error()
        return rc

    def bs(lp, upp, steps_, offset, handle=None):
        rc = L.copra_batch_set_control_bound_schedule(handle or h, lp, upp, steps_, offset, 1, 0, 0)
        assert rc == _capi.COPRA_OK or L.copra_last_error()
        return rc

    assert cs(0, v.ctypes.data, steps, 2, 0) == _capi.COPRA_ERR_DOMAIN  # a per-step constraint of 3 rows
    assert cs(0, v.ctypes.data, steps, 0, 0) == _capi.COPRA_ERR_DOMAIN
    assert cs(0, v.ctypes.data, 0, 3, 0) == _capi.COPRA_ERR_ARG
    assert cs(0, v.ctypes.data, steps, 3, -1) == _capi.COPRA_ERR_ARG
    assert cs(2, v.ctypes.data, steps, 3, 0) == _capi.COPRA_ERR_ARG  # no such constraint
    assert cs(-1, v.ctypes.data, steps, 3, 0) == _capi.COPRA_ERR_ARG
    assert cs(1, v.ctypes.data, steps, 3, 0) == _capi.COPRA_ERR_UNSUPPORTED  # the ControlBoundConstraint
    assert bs(lo.ctypes.data, None, steps, 0) == _capi.COPRA_ERR_ARG  # exactly one of lower / upper
    assert bs(None, up.ctypes.data, steps, 0) == _capi.COPRA_ERR_ARG
    assert bs(lo.ctypes.data, up.ctypes.data, 0, 0) == _capi.COPRA_ERR_ARG
    assert bs(lo.ctypes.data, up.ctypes.data, steps, -1) == _capi.COPRA_ERR_ARG
    # a TrajectoryBoundConstraint and a dense constraint have no schedule; a controller without a ControlBoundConstraint has no bound schedule
    cw = workloads.com_preview(64)
    n = 3 * cw["N"]
    other = BatchLMPC(6, 3, cw["N"], 64, cw["costs"], [cw["cstrs"][0], dict(kind="dense", A=np.ones((1, n)), b=[1e3])])
    z = np.zeros((4, 6))
    for k in (0, 1):
        assert L.copra_batch_set_constraint_schedule(other._h, k, z.ctypes.data, 4, 1, 0, 1, 0, 0) == _capi.COPRA_ERR_UNSUPPORTED
        assert L.copra_last_error()
    assert bs(lo.ctypes.data, up.ctypes.data, steps, 0, handle=other._h) == _capi.COPRA_ERR_UNSUPPORTED
    # a full-size constraint takes any divisor of its rows; more than eight live windows are refused
    E = np.kron(np.eye(N + 1), np.hstack([np.zeros((3, 3)), np.eye(3)]))
    many = _engine(wl, cstrs=[dict(kind="trajectory", E=E[3 * k:3 * k + 3], f=[0.9] * 3) for k in range(9)] + [wl["cstrs"][1]])
    f = np.full((4, 3), 0.9)
    assert L.copra_batch_set_constraint_schedule(many._h, 0, f.ctypes.data, 4, 2, 0, 1, 0, 0) == _capi.COPRA_ERR_DOMAIN
    for k in range(8):
        assert L.copra_batch_set_constraint_schedule(many._h, k, f.ctypes.data, 4, (3, 1)[k % 2], 0, 1, 0, 0) == _capi.COPRA_OK, k
    assert L.copra_batch_set_constraint_schedule(many._h, 8, f.ctypes.data, 4, 3, 0, 1, 0, 0) == _capi.COPRA_ERR_UNSUPPORTED
    assert L.copra_last_error()
    assert bs(lo.ctypes.data, up.ctypes.data, steps, 0, handle=many._h) == _capi.COPRA_ERR_UNSUPPORTED
    with pytest.raises(_capi.CopraDomainError):
        eng.set_constraint_schedule(0, v, 2)  # (the binding: the last axis is not rows_per_step)
    with pytest.raises(_capi.CopraDomainError):
        eng.set_control_bound_schedule(np.zeros((63, steps, 3)), np.zeros((63, steps, 3)))
    # the handles solve correctly afterwards: nothing of the refused calls stuck
    for e in (eng, many):
        e.solve()
        res = e.results()
        ref = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], wl["x0"], N, wl["costs"], wl["cstrs"], nthreads=8)
        assert np.array_equal(res["status"], ref["status"]) and (res["status"] == 0).all()
        assert float(tc.rel(res["control"], ref["control"]).max()) <= RTOL


def test_without_a_limit_schedule_nothing_changes():
    """a controller whose schedules were set and ended before its first solve... is another matter; THIS one never has a live limit schedule at a
    tick, and its rollout is bit for bit the rollout of a handle that never saw the new calls: the new launch is not made"""
    wl, _ = lc.com_limits()
    w_seq = lc.noise(wl, 35)
    a, b = _engine(wl), _engine(wl)
    assert a._lib.copra_batch_set_control_bound_schedule(a._h, None, None, 0, 0, 0, 0, 0) == 0  # ending a schedule that is not live
    a.set_constraint_schedule(0, None, 3)
    ha = a.rollout(lc.TICKS, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True)
    hb = b.rollout(lc.TICKS, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True)
    for x, y in zip(_np(ha), _np(hb)):
        assert x.tobytes() == y.tobytes()
