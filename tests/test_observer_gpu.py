"""The state observer of the tick on the device (copra_batch_set_observer; BatchLMPC.set_observer, set_plant_state, plant_state,
advance(noise=, y_meas=, y_out=, xhat_out=), rollout(noise=, y_hist=, xhat_hist=)) against the CPU oracle and the longdouble statement of the rule,
tick by tick.

Positions are measured (ny = 3, or 1 for the double integrator); the plant is the model with the constant offset of OFFSET on d
(tests/test_bias_estimator_gpu.py); the controller starts from the true state plus an error on the unmeasured rows; small sensor noise.  At every
tick t the oracle solves from the device's own xhat_hist[t - 1] (x0 at t = 0) with d_t: statuses equal, first controls entry-wise within 1e-6 with
the floor 1e-3 (the parity suite's), at least 75 % solved.  That the solve read the ESTIMATE is a condition on the inputs, checked from the oracle
and reference_observer alone (_estimate_matters): at tick 1 the oracle's control from the restated xhat_1 differs from its control from the true
xp_1 by more than 1e-3 on at least half of the solved instances.  The plant step stays within step_bound from x_hist, the truth; y_hist, xhat_hist
and d_hist within the bounds derived in tests/test_observer_abi.py, all computed from the device's own histories.  Held instances keep xp, xhat and
dhat bit for bit.  Two routes through the kernels agree within 1e-9 (ROUTES)."""
import numpy as np
import pytest

from test_bias_estimator_gpu import HELD, ROUTES, SMALL, _scenario
from test_closed_loop_abi import reference_step
from test_closed_loop_gpu import RTOL, _assert_step, _engine
from test_observer_abi import LD, reference_observer
from tracking_cases import BATCH, TICKS, rel

pytestmark = pytest.mark.gpu

# per workload: outputs, the rows of d the observer estimates (one per output: the last ny states, which every position integrates), and the
# initial error of the estimate on the unmeasured rows -- large enough for the condition of _estimate_matters
CASES = {"com": dict(ny=3, err=0.1), "jerk": dict(ny=3, err=0.1), "double_integrator": dict(ny=1, err=4.0)}
V_NOISE = 1e-3
DEADBEAT_SHARE = 0.5  # Lx at most this share of what kalman_gain gives for a tiny Rv (largest entry): not deadbeat


def _numpy(hist):
    return {k: v.cpu().numpy() for k, v in hist.items() if v is not None}


def _setup(name, batch=BATCH, ticks=TICKS, per_instance=False, with_Ld=True, seed=31):
    """dict(wl, plant, w_seq, held, C, Lx, Ld, xhat0, v_seq): the scenario of the bias tests without the perturbed A, gains from kalman_gain"""
    from copra_amd.observer_design import kalman_gain
    wl, plant, w_seq, held = _scenario(name, batch=batch, ticks=ticks, perturb=False)
    nx = wl["B"].shape[1]
    ny, err = CASES[name]["ny"], CASES[name]["err"]
    rng = np.random.default_rng(seed)
    C = np.eye(nx)[:ny]
    G = np.zeros((nx, ny))
    G[nx - ny:] = np.eye(ny)
    Qw, Rv, Qd = 1e-4 * np.eye(nx), 1e-3 * np.eye(ny), 1e-5 * np.eye(ny)
    if with_Ld:
        Lx, Ld = kalman_gain(wl["A"], C, Qw, Rv, with_bias=True, Qd=Qd, Gd=G)
        fast = kalman_gain(wl["A"], C, Qw, 1e-12 * np.eye(ny), with_bias=True, Qd=Qd, Gd=G)[0]
    else:
        Lx, Ld = kalman_gain(wl["A"], C, Qw, Rv), None
        fast = kalman_gain(wl["A"], C, Qw, 1e-12 * np.eye(ny))
    assert np.abs(Lx).max() <= DEADBEAT_SHARE * np.abs(fast).max()  # (not deadbeat: the estimate keeps an error for several ticks)
    if per_instance:
        C = np.ascontiguousarray(np.broadcast_to(C, (batch, ny, nx)))  # (one flag covers C and the gains)
    else:
        Lx, Ld = Lx.mean(axis=0), (None if Ld is None else Ld.mean(axis=0))
    xhat0 = wl["x0"].copy()
    xhat0[:, ny:] += err * rng.choice([-1.0, 1.0], (batch, nx - ny))
    xhat0[list(held)] = wl["x0"][list(held)]  # (stuck by their estimate, as by their state)
    return dict(wl=wl, plant=plant, w_seq=w_seq, held=held, C=C, Lx=Lx, Ld=Ld, xhat0=xhat0, v_seq=V_NOISE * rng.standard_normal((ticks, batch, ny)), ny=ny)


def _start(S, **kw):
    eng = _engine(S["wl"], **kw)
    eng.set_observer(S["C"], S["Lx"], S["Ld"])  # (the plant starts from the x0 in force: the truth)
    eng.set_x0(S["xhat0"])
    return eng


def _rollout(eng, S, ticks=TICKS, plant=True, **kw):
    return _numpy(eng.rollout(ticks, plant=S["plant"] if plant else None, disturbances=S["w_seq"][:ticks], noise=S["v_seq"][:ticks], x_hist=True, u_hist=True,
                              status_hist=True, d_hist=S["Ld"] is not None, y_hist=True, xhat_hist=True, **kw))


def _solve(oracle, wl, d, x):
    return oracle.lmpc_solve_batch(wl["A"], wl["B"], d, x, wl["N"], wl["costs"], wl["cstrs"], nthreads=8)


def _estimate_matters(oracle, S, what):
    """the condition on the inputs, from the oracle and reference_observer alone: tick 0 restated, then the control from xhat_1 against the
    control from the true xp_1"""
    wl = S["wl"]
    nu = wl["B"].shape[2]
    first = _solve(oracle, wl, wl["d"], S["xhat0"])
    ok = first["status"] == 0
    u = np.where(ok[:, None], first["control"][:, :nu], 0.0)
    xp1, Sx = reference_step(*S["plant"], wl["x0"], u, S["w_seq"][0])
    R = reference_observer(wl["A"], wl["B"], wl["d"], S["xhat0"], u, S["C"], S["Lx"], S["Ld"], xplus=xp1, Sx=Sx, v=S["v_seq"][0])
    pick = lambda new, old: np.where(ok[:, None], np.asarray(new, dtype=np.float64), old)  # noqa: E731  (held: nothing moves)
    xhat1, d1, true1 = pick(R["xhat"], S["xhat0"]), pick(R["dhat"], wl["d"]), pick(xp1, wl["x0"])
    a, b = _solve(oracle, wl, d1, xhat1), _solve(oracle, wl, d1, true1)
    both = (a["status"] == 0) & (b["status"] == 0)
    share = float((rel(b["control"][both, :nu], a["control"][both, :nu]).max(axis=1) > 1e-3).sum()) / max(1, int((a["status"] == 0).sum()))
    print("%s: the control from the true state differs by more than 1e-3 on %.0f %% of the solved instances" % (what, 100 * share))
    assert share >= 0.5, what


def _within(got, ref, bound, moved, what):
    err = np.abs(got[moved].astype(LD) - ref[moved])
    print("%s: max err / bound = %.3f" % (what, float((err / np.maximum(bound[moved], np.finfo(float).tiny)).max()) if err.size else 0.0))
    assert (err <= bound[moved]).all(), what


def _check(oracle, S, hist, what, plant=True, ages=None, solved_at=None):
    """every tick of a rollout with the observer on; hist holds numpy arrays.  ages: the expected age_hist (backup plans), solved_at: the ticks
    with a solve (all of them by default)"""
    wl, held, with_Ld = S["wl"], S["held"], S["Ld"] is not None
    xh, uh, sh, yh, hh = hist["x_hist"], hist["u_hist"], hist["status_hist"], hist["y_hist"], hist["xhat_hist"]
    dh = hist["d_hist"] if with_Ld else None
    nu = wl["B"].shape[2]
    ticks = uh.shape[0]
    assert not any(np.isnan(a).any() for a in (xh, yh, hh)) and (dh is None or not np.isnan(dh).any())
    assert np.array_equal(xh[0], wl["x0"])  # x_hist[0]: the plant's state before the first tick
    for t in range(ticks):
        xhat_t = S["xhat0"] if t == 0 else hh[t - 1]
        d_t = wl["d"] if (t == 0 or not with_Ld) else dh[t - 1]
        if solved_at is None or t in solved_at:
            ref = _solve(oracle, wl, d_t, xhat_t)  # from the device's own ESTIMATE
            assert np.array_equal(sh[t], ref["status"]), (what, t)
            assert (sh[t][list(held)] != 0).all() and (sh[t] == 0).mean() >= 0.75, (what, t, float((sh[t] == 0).mean()))
            ok = sh[t] == 0
            e = float(rel(uh[t][ok], ref["control"][ok, :nu]).max())
            print("%s tick %d: first controls against the oracle from xhat_t, d_t: %.2e" % (what, t, e))
            assert e <= RTOL, (what, t)
        moved = ~np.isnan(uh[t]).any(axis=1) if ages is None else ages[t] != HELD
        if ages is None:
            assert np.array_equal(moved, sh[t] == 0), (what, t)
        u = np.where(moved[:, None], uh[t], 0.0)
        Ap, Bp, dp = S["plant"] if plant else (wl["A"], wl["B"], d_t)  # (no plant given: the model with d = dhat)
        _assert_step(xh[t + 1], Ap, Bp, dp, xh[t], u, S["w_seq"][t], moved, "%s tick %d" % (what, t))
        xref, Sx = reference_step(Ap, Bp, dp, xh[t], u, S["w_seq"][t])
        R = reference_observer(wl["A"], wl["B"], d_t, xhat_t, u, S["C"], S["Lx"], S["Ld"], xplus=xref, Sx=Sx, v=S["v_seq"][t])
        _within(yh[t], R["y"], R["Ey"], moved, "%s tick %d y" % (what, t))
        _within(hh[t], R["xhat"], R["Eh"], moved, "%s tick %d xhat" % (what, t))
        assert xh[t + 1][~moved].tobytes() == xh[t][~moved].tobytes(), (what, t)  # held: the plant's state ...
        assert hh[t][~moved].tobytes() == np.ascontiguousarray(xhat_t[~moved]).tobytes(), (what, t)  # ... the estimate ...
        if with_Ld:
            _within(dh[t], R["dhat"], R["Ed"], moved, "%s tick %d dhat" % (what, t))
            assert dh[t][~moved].tobytes() == np.ascontiguousarray(d_t[~moved]).tobytes(), (what, t)  # ... and dhat, bit for bit


# ---- 1. tick by tick against the oracle ----
@pytest.mark.parametrize("name,per_instance,with_Ld", [("com", False, True), ("jerk", True, True), ("double_integrator", True, False)])
def test_tick_by_tick_against_the_oracle(oracle, name, per_instance, with_Ld):
    S = _setup(name, per_instance=per_instance, with_Ld=with_Ld)
    what = "%s, %s gains%s" % (name, "per-instance" if per_instance else "shared", ", Ld" if with_Ld else "")
    _estimate_matters(oracle, S, what)
    eng = _start(S)
    if name == "double_integrator":
        assert eng.lanes_per_instance() in (16, 32)  # the packed kernels
    hist = _rollout(eng, S)
    if name == "com":
        assert eng.axis_solver_ran()
    assert np.array_equal(eng.plant_state(), hist["x_hist"][-1]) and np.array_equal(eng.state(), hist["xhat_hist"][-1])
    if with_Ld:
        assert np.array_equal(eng.bias(), hist["d_hist"][-1])
    else:
        assert np.array_equal(eng.bias(), S["wl"]["d"])  # a state observer only: d is not touched
    for b in S["held"]:  # STUCK, no fallback: constant bit for bit, and equal to where they started
        assert (hist["x_hist"][:, b] == S["wl"]["x0"][b]).all() and (hist["xhat_hist"][:, b] == S["xhat0"][b]).all()
        if with_Ld:
            assert (hist["d_hist"][:, b] == S["wl"]["d"][b]).all()
    if name != "double_integrator":
        assert len(S["held"]) >= 1
    _check(oracle, S, hist, what)


# ---- 2. no plant given, no Ld ----
def test_the_model_as_plant_without_Ld(oracle):
    """step.A == NULL: the plant is the model with d = dhat, moved from its OWN state; per-instance gains, d is never touched"""
    S = _setup("com", batch=SMALL, per_instance=True, with_Ld=False)
    eng = _start(S)
    hist = _rollout(eng, S, plant=False)
    assert np.array_equal(eng.bias(), S["wl"]["d"])
    _check(oracle, S, hist, "model as plant", plant=False)


# ---- 3. backup plans ----
def test_backup_plans_and_solve_every(oracle):
    """set_backup_steps(3), solve_every = 2: ages 0, 1, 0, 1, ...; the states move on the ticks without a solve, with the plan's control"""
    S = _setup("com", batch=SMALL, per_instance=True)
    eng = _start(S)
    eng.set_backup_steps(3)
    hist = _rollout(eng, S, solve_every=2, age_hist=True)
    sh = hist["status_hist"]
    ages, nxt = np.zeros((TICKS, SMALL), dtype=np.int32), np.zeros(SMALL, dtype=np.int32)
    for t in range(TICKS):  # the rule of ABI 10 from the statuses: a solve at the even ticks
        fresh = (sh[t] == 0) if t % 2 == 0 else np.zeros(SMALL, dtype=bool)
        plan = ~fresh & (nxt >= 1) & (nxt <= 3)
        ages[t] = np.where(fresh, 0, np.where(plan, nxt, HELD))
        nxt = np.where(fresh, 1, np.where(plan, nxt + 1, nxt))
    assert np.array_equal(hist["age_hist"], ages)
    assert (ages[:, list(S["held"])] == HELD).all() and len(S["held"]) >= 1
    assert ((ages[0::2] == 0).mean(axis=1) >= 0.75).all() and ((ages[1::2] == 1).mean(axis=1) >= 0.75).all()
    for t in range(1, TICKS, 2):  # no solve at t: the estimate moved all the same
        played = ages[t] == 1
        assert (hist["xhat_hist"][t][played] != hist["xhat_hist"][t - 1][played]).any(axis=1).all(), t
    _check(oracle, S, hist, "backup plans", ages=ages, solved_at=set(range(0, TICKS, 2)))


# ---- 4. measured outputs ----
def test_measured_outputs_reproduce_the_rollout():
    """advance(y_meas=) tick by tick, fed with the y_hist of a rollout from the same start: xhat_hist and d_hist bit for bit (the arithmetic
    after y is the same), and the plant's state is left alone"""
    import torch
    S = _setup("com", batch=SMALL)
    ticks = 4
    hist = _rollout(_start(S), S, ticks=ticks)
    eng = _start(S)
    before = eng.plant_state()
    marker = torch.full((SMALL, 6), -7.0, dtype=torch.float64, device="cuda")
    for t in range(ticks):
        eng.solve()
        out = eng.advance(plant=S["plant"], disturbance=S["w_seq"][t], noise=S["v_seq"][t], y_meas=hist["y_hist"][t], x_out=marker, u_out=True, y_out=True,
                          xhat_out=True, d_out=True)
        got = _numpy(out)
        assert got["u_out"].tobytes() == hist["u_hist"][t].tobytes(), t  # (the same solve from the same estimate)
        assert got["y_out"].tobytes() == hist["y_hist"][t].tobytes(), t
        assert got["xhat_out"].tobytes() == hist["xhat_hist"][t].tobytes(), t
        assert got["d_out"].tobytes() == hist["d_hist"][t].tobytes(), t
    assert np.array_equal(eng.state(), hist["xhat_hist"][-1]) and np.array_equal(eng.bias(), hist["d_hist"][-1])
    assert np.array_equal(eng.plant_state(), before) and (marker == -7.0).all()  # no plant: xp untouched, x_out not written
    # COPRA_ERR_ARG: a rollout has no measurements
    import ctypes
    from copra_amd import _capi
    st = _capi.PlantStepObs()
    eng._lib.copra_plant_step_obs_init(ctypes.byref(st))
    st.y_meas = marker.data_ptr()
    with pytest.raises(ValueError):
        _capi.check(eng._lib.copra_batch_rollout(eng._h, ctypes.byref(st), 1, None, None, None, None, None))


# ---- 5. two routes ----
def test_two_routes_agree():
    S = _setup("com")
    a, b = _start(S), _start(S, options={"no_axis_solver": 1})
    out = [_rollout(eng, S) for eng in (a, b)]
    assert a.axis_solver_ran() and not b.axis_solver_ran()
    assert np.array_equal(out[0]["status_hist"], out[1]["status_hist"])
    du = np.nanmax(np.abs(out[0]["u_hist"] - out[1]["u_hist"]))
    dx = max(np.abs(out[0][k] - out[1][k]).max() for k in ("x_hist", "xhat_hist", "d_hist", "y_hist"))
    print("axis solver against the general kernels: u_hist %.2e, states and estimates %.2e" % (du, dx))
    assert du <= ROUTES and dx <= ROUTES
    assert np.array_equal(np.isnan(out[0]["u_hist"]), np.isnan(out[1]["u_hist"]))


# ---- 6. ownership and life cycle ----
def test_life_cycle_and_errors():
    import torch
    from copra_amd import BatchLMPC, _capi
    S = _setup("com", batch=SMALL)
    wl = S["wl"]
    fresh = BatchLMPC(6, 3, wl["N"], SMALL, wl["costs"], wl["cstrs"])
    with pytest.raises(_capi.CopraRuntimeError):  # no system yet
        fresh.set_observer(S["C"], S["Lx"])
    fresh.set_observer(None)  # (ending what never began is no error)
    with pytest.raises(_capi.CopraRuntimeError):  # the plant has no state of its own yet
        fresh.plant_state()
    with pytest.raises(_capi.CopraRuntimeError):
        fresh.set_plant_state(wl["x0"])
    assert fresh.plant_state_ptr() == 0
    eng = _engine(wl)
    one = np.ones(64)
    for args in ((0, one.ctypes.data, one.ctypes.data, None, 0, 0), (3, one.ctypes.data, None, None, 0, 0)):  # ny < 1; C without Lx
        with pytest.raises(ValueError):
            _capi.check(eng._lib.copra_batch_set_observer(eng._h, *args))
    with pytest.raises(ValueError):  # a NULL x
        _capi.check(eng._lib.copra_batch_set_plant_state(eng._h, None, 0))
    with pytest.raises(ValueError):
        _capi.check(eng._lib.copra_batch_get_plant_state(eng._h, None))
    with pytest.raises(_capi.CopraDomainError):
        eng.set_observer(np.ones((3, 5)), np.ones((6, 3)))
    # ny > nx is no error: redundant sensors
    eng.set_observer(np.vstack([np.eye(6), np.eye(6)[:2]]), 0.1 * np.ones((6, 8)))
    eng.set_observer(None)
    # the observer and the bias estimator refuse each other
    eng.set_observer(S["C"], S["Lx"], S["Ld"])
    with pytest.raises(_capi.CopraRuntimeError, match="copra_batch_set_observer"):
        eng.set_bias_estimator(np.ones(6))
    eng.set_observer(None)
    eng.set_bias_estimator(np.ones(6))
    with pytest.raises(_capi.CopraRuntimeError, match="copra_batch_set_bias_estimator"):
        eng.set_observer(S["C"], S["Lx"], S["Ld"])
    eng.set_bias_estimator(None)
    # set_x0 moves only the estimate, set_plant_state only the truth; a call while on keeps both
    eng.set_observer(S["C"], S["Lx"], S["Ld"])
    assert eng.plant_state_ptr() not in (0, eng.state_ptr()) and np.array_equal(eng.plant_state(), wl["x0"])
    eng.set_x0(S["xhat0"])
    assert np.array_equal(eng.plant_state(), wl["x0"]) and np.array_equal(eng.state(), S["xhat0"])
    eng.set_plant_state(wl["x0"] + 1.0)
    assert np.array_equal(eng.plant_state(), wl["x0"] + 1.0) and np.array_equal(eng.state(), S["xhat0"])
    eng.set_plant_state(torch.from_numpy(wl["x0"]).cuda())
    eng.set_observer(S["C"], 0.5 * S["Lx"])  # new gains, no Ld from now on: the states and d stay
    assert np.array_equal(eng.plant_state(), wl["x0"]) and np.array_equal(eng.state(), S["xhat0"]) and np.array_equal(eng.bias(), wl["d"])
    # set_system keeps the observer on; with Ld, dhat restarts from the new d
    eng.set_observer(S["C"], S["Lx"], S["Ld"])
    eng.set_bias(wl["d"] + 1.0)
    eng.set_system(wl["A"], wl["B"], wl["d"], S["xhat0"])
    assert np.array_equal(eng.bias(), wl["d"]) and np.array_equal(eng.plant_state(), wl["x0"])
    first = _rollout(eng, S, ticks=2)
    twin = _rollout(_start(S), S, ticks=2)
    assert np.array_equal(first["status_hist"], twin["status_hist"]) and np.abs(first["xhat_hist"] - twin["xhat_hist"]).max() <= ROUTES
    # the observer off: the new outputs are not written, the tick is the tick of ABI 11
    eng.set_observer(None)
    with pytest.raises(ValueError):
        eng.advance(xhat_out=True)
    # set_shared_system ends the observer; a shared model refuses it
    eng.set_observer(S["C"], S["Lx"], S["Ld"])
    eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
    eng.set_x0(wl["x0"])
    eng.rollout(2)  # (the tick of a shared model, without an observer)
    for opts in ({}, {"no_axis_solver": 1}):
        sh = _engine(wl, shared_model=True, options=opts)
        with pytest.raises(_capi.CopraUnsupported):
            sh.set_observer(S["C"], S["Lx"])
    pb = __import__("fixtures").bounded_system("trajectory", N=12)
    ise = BatchLMPC(2, 1, 12, 4, pb["costs"], pb["cstrs"], initial_state=dict(R=1e-2 * np.eye(2), r=np.zeros(2)))
    with pytest.raises(_capi.CopraUnsupported):
        ise.set_observer(np.ones((1, 2)), np.ones((2, 1)))
