"""The disturbance estimator of the tick on the device (copra_batch_set_bias_estimator; BatchLMPC.set_bias_estimator, set_bias, bias,
advance(d_out=), rollout(d_hist=)) against the CPU oracle and the longdouble statement of the rule, tick by tick.

The plant is the model with a per-instance offset on d and every entry of A perturbed by up to 2 %; small position noise.  At every tick t the
oracle solves from the device's own x_hist[t] with d_t -- the initial d at t = 0, d_hist[t - 1] afterwards: statuses equal, first controls
entry-wise within 1e-6 with the floor 1e-3 (the parity suite's).  That is the test that the solve read the new estimate, under a condition on
the inputs checked from the oracle alone: at the last tick its control with the initial d differs from its control with d_t by more than 1e-3
on at least half of the solved instances.  The plant step stays within step_bound (tests/test_closed_loop_abi.py), d_hist[t] within bias_bound
(derived in tests/test_bias_estimator_abi.py), both computed from the device's own x_hist, u_hist.  Held instances keep x and dhat bit for bit.
Two routes through the kernels agree within 1e-9 (ROUTES, as tests/test_reference_schedule_gpu.py)."""
import numpy as np
import pytest

from test_bias_estimator_abi import LD, reference_bias
from test_closed_loop_abi import reference_step
from test_closed_loop_gpu import RTOL, STUCK, _assert_step, _engine, _position_noise
from tracking_cases import BATCH, TICKS, rel

pytestmark = pytest.mark.gpu

ROUTES = 1e-9
SMALL = 67  # where no particular solver has to run: odd, several groups, a partial last one
HELD = -2


def _numpy(hist):
    return {k: v.cpu().numpy() for k, v in hist.items() if v is not None}


def _scenario(name, batch=BATCH, ticks=TICKS, stuck=True, noise=True, perturb=True, seed=21):
    """(workload, plant (A, B, d) in natural indexing, w_seq, the stuck instances)"""
    from copra_amd import workloads
    make = {"com": workloads.com_preview, "jerk": workloads.jerk_preview}.get(name)
    wl = make(batch) if make else workloads.double_integrator(batch, N=16)
    wl = dict(wl, x0=wl["x0"].copy())
    rng = np.random.default_rng(seed)
    nx = wl["B"].shape[1]
    held = tuple(b for b in STUCK if b < batch) if (stuck and make) else ()
    for b in held:
        wl["x0"][b, 3] = 50.0  # far outside the velocity bound: infeasible at every tick, no fallback -- held
    c = OFFSET[name] * rng.uniform(0.5, 1.0, (batch, nx)) * rng.choice([-1.0, 1.0], (batch, nx))
    Ap = wl["A"] * (1.0 - (0.02 * rng.uniform(0.0, 1.0, wl["A"].shape) if perturb else 0.0))  # (towards zero: no velocity grows past its bound)
    npos = 3 if make else 1
    w_seq = _position_noise(ticks, batch, nx, npos, seed=seed + 1) if noise else np.zeros((ticks, batch, nx))
    return wl, (Ap, wl["B"], wl["d"] + c), w_seq, held


# the size of the constant load per workload, in the units of its d: large enough to move the first control by far more than 1e-3 once it is
# learnt, small enough to leave every instance that is not stuck feasible
OFFSET = {"com": 0.004, "jerk": 0.004, "double_integrator": 0.05}


def _gain(kind, batch, nx, seed=3):
    rng = np.random.default_rng(seed)
    if kind == "diag_shared":
        return np.linspace(0.5, 0.9, nx)
    if kind == "diag_each":
        return rng.uniform(0.4, 0.9, (batch, nx))
    if kind == "dense_shared":
        return 0.7 * np.eye(nx) + 0.05 * rng.uniform(-1.0, 1.0, (nx, nx))
    return 0.7 * np.eye(nx) + 0.05 * rng.uniform(-1.0, 1.0, (batch, nx, nx))  # dense_each


def _check(oracle, wl, hist, plant, w_seq, gain, held, what, ages=None, solved_at=None, moved_share=True):
    """every tick of a rollout with the estimator on; hist holds numpy arrays.  ages: the expected age_hist (backup plans), solved_at: the ticks
    with a solve (all of them by default)"""
    xh, uh, sh, dh = hist["x_hist"], hist["u_hist"], hist["status_hist"], hist["d_hist"]
    Ap, Bp, dp = plant
    nx, nu = wl["B"].shape[1], wl["B"].shape[2]
    ticks, batch = uh.shape[0], uh.shape[1]
    dense = np.shape(gain)[-2:] == (nx, nx)  # (no batch here equals nx)
    assert not np.isnan(xh).any() and not np.isnan(dh).any()
    for t in range(ticks):
        d_t = wl["d"] if t == 0 else dh[t - 1]
        if solved_at is None or t in solved_at:
            ref = oracle.lmpc_solve_batch(wl["A"], wl["B"], d_t, xh[t], wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
            assert np.array_equal(sh[t], ref["status"]), (what, t)
            # (a run in which everything failed cannot pass; an instance the mismatch pushes past its velocity bound fails and is held, as the rule says)
            assert (sh[t][list(held)] != 0).all() and (sh[t] == 0).mean() >= 0.75, (what, t, float((sh[t] == 0).mean()))
            ok = sh[t] == 0
            e = float(rel(uh[t][ok], ref["control"][ok, :nu]).max())
            print("%s tick %d: first controls against the oracle with d_t: %.2e" % (what, t, e))
            assert e <= RTOL, (what, t)
        moved = ~np.isnan(uh[t]).any(axis=1) if ages is None else ages[t] != HELD
        if ages is None:
            assert np.array_equal(moved, sh[t] == 0), (what, t)
        u = np.where(moved[:, None], uh[t], 0.0)
        _assert_step(xh[t + 1], Ap, Bp, dp, xh[t], u, w_seq[t], moved, "%s tick %d" % (what, t))
        xref, Sx = reference_step(Ap, Bp, dp, xh[t], u, w_seq[t])
        dref, dbound = reference_bias(wl["A"], wl["B"], d_t, xh[t], u, xref, Sx, gain, dense)
        derr = np.abs(dh[t][moved].astype(LD) - dref[moved])
        print("%s tick %d: estimates max err / bound = %.3f" % (what, t, float((derr / dbound[moved]).max())))
        assert (derr <= dbound[moved]).all(), (what, t)
        assert dh[t][~moved].tobytes() == np.ascontiguousarray(d_t[~moved]).tobytes(), (what, t)  # held: the estimate ...
        assert xh[t + 1][~moved].tobytes() == xh[t][~moved].tobytes(), (what, t)  # ... and the state, bit for bit
    if moved_share:  # the condition on the inputs, from the oracle alone: the estimate the last solve read matters
        t = ticks - 1
        a = oracle.lmpc_solve_batch(wl["A"], wl["B"], dh[t - 1], xh[t], wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
        b = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], xh[t], wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
        both = (a["status"] == 0) & (b["status"] == 0)
        share = float((rel(b["control"][both, :nu], a["control"][both, :nu]).max(axis=1) > 1e-3).sum()) / max(1, int((a["status"] == 0).sum()))
        print("%s: the control with the initial d differs by more than 1e-3 on %.0f %% of the solved instances" % (what, 100 * share))
        assert share >= 0.5, what


def _rollout(eng, ticks, w_seq, plant, **kw):
    return _numpy(eng.rollout(ticks, plant=plant, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True, d_hist=True, **kw))


# ---- 1. tick by tick against the oracle ----
@pytest.mark.parametrize("name,kind", [("com", "diag_shared"), ("jerk", "dense_each"), ("double_integrator", "diag_each")])
def test_tick_by_tick_against_the_oracle(oracle, name, kind):
    wl, plant, w_seq, held = _scenario(name)
    nx = wl["B"].shape[1]
    gain = _gain(kind, BATCH, nx)
    eng = _engine(wl)
    if name == "double_integrator":
        assert eng.lanes_per_instance() in (16, 32)  # the packed kernels
    eng.set_bias_estimator(gain)
    hist = _rollout(eng, TICKS, w_seq, plant)
    if name == "com":
        assert eng.axis_solver_ran()
    assert np.array_equal(hist["x_hist"][0], wl["x0"])
    assert np.array_equal(eng.bias(), hist["d_hist"][-1]) and np.array_equal(eng.state(), hist["x_hist"][-1])
    for b in held:  # constant bit for bit, and equal to where they started
        assert (hist["d_hist"][:, b] == wl["d"][b]).all() and (hist["x_hist"][:, b] == wl["x0"][b]).all()
    _check(oracle, wl, hist, plant, w_seq, gain, held, "%s, %s" % (name, kind))


# ---- 2. two routes ----
def test_two_routes_agree():
    wl, plant, w_seq, held = _scenario("com")
    gain = _gain("dense_shared", BATCH, 6)
    a, b = _engine(wl), _engine(wl, options={"no_axis_solver": 1})
    out = []
    for eng in (a, b):
        eng.set_bias_estimator(gain)
        out.append(_rollout(eng, TICKS, w_seq, plant))
    assert a.axis_solver_ran() and not b.axis_solver_ran()
    assert np.array_equal(out[0]["status_hist"], out[1]["status_hist"])
    du = np.nanmax(np.abs(out[0]["u_hist"] - out[1]["u_hist"]))
    dd = np.abs(out[0]["d_hist"] - out[1]["d_hist"]).max()
    print("axis solver against the general kernels: u_hist %.2e, d_hist %.2e" % (du, dd))
    assert du <= ROUTES and dd <= ROUTES
    assert np.array_equal(np.isnan(out[0]["u_hist"]), np.isnan(out[1]["u_hist"]))


# ---- 3. deadbeat ----
@pytest.mark.parametrize("dense", [False, True])
def test_deadbeat_on_the_device(dense):
    """L = I, plant = model with d + c, no noise: from the first tick on the estimate is d + c within bias_bound, on every instance that solved at
    tick 0 -- also on one whose later solve fails: it is held, bit for bit"""
    wl, plant, w_seq, held = _scenario("com", batch=SMALL, noise=False, perturb=False)
    gain = np.eye(6) if dense else np.ones(6)
    eng = _engine(wl)
    eng.set_bias_estimator(gain)
    hist = _rollout(eng, TICKS, w_seq, plant)
    xh, uh, sh, dh = hist["x_hist"], hist["u_hist"], hist["status_hist"], hist["d_hist"]
    first = sh[0] == 0
    assert first.sum() == SMALL - len(held) and len(held) >= 1
    target = plant[2].astype(LD)
    for t in range(TICKS):
        d_t = wl["d"] if t == 0 else dh[t - 1]
        moved = sh[t] == 0
        u = np.where(moved[:, None], uh[t], 0.0)
        xref, Sx = reference_step(plant[0], plant[1], plant[2], xh[t], u, None)
        _, dbound = reference_bias(wl["A"], wl["B"], d_t, xh[t], u, xref, Sx, gain, dense)
        m = first & moved
        err = np.abs(dh[t][m].astype(LD) - target[m])
        print("deadbeat tick %d: max err / bound = %.3f" % (t, float((err / dbound[m]).max())))
        assert (err <= dbound[m]).all(), t
        assert dh[t][first & ~moved].tobytes() == np.ascontiguousarray(d_t[first & ~moved]).tobytes()
    assert (sh[1:, first] == 0).mean() > 0.9  # (the loop is the nominal loop: it keeps solving)


# ---- 4. backup plans ----
def test_backup_plans_move_the_estimate(oracle):
    """set_backup_steps(3), solve_every = 2: ages 0, 1, 0, 1, ...; the estimate moves on the ticks without a solve, with the plan's control"""
    wl, plant, w_seq, held = _scenario("com", batch=SMALL)
    gain = _gain("diag_each", SMALL, 6)
    eng = _engine(wl)
    eng.set_backup_steps(3)
    eng.set_bias_estimator(gain)
    hist = _rollout(eng, TICKS, w_seq, plant, solve_every=2, age_hist=True)
    sh = hist["status_hist"]
    ages, nxt = np.zeros((TICKS, SMALL), dtype=np.int32), np.zeros(SMALL, dtype=np.int32)
    for t in range(TICKS):  # the rule of ABI 10 from the statuses: a solve at the even ticks
        fresh = (sh[t] == 0) if t % 2 == 0 else np.zeros(SMALL, dtype=bool)
        plan = ~fresh & (nxt >= 1) & (nxt <= 3)
        ages[t] = np.where(fresh, 0, np.where(plan, nxt, HELD))
        nxt = np.where(fresh, 1, np.where(plan, nxt + 1, nxt))
    assert np.array_equal(hist["age_hist"], ages)
    assert (ages[:, list(held)] == HELD).all() and len(held) >= 1
    assert ((ages[0::2] == 0).mean(axis=1) >= 0.75).all() and ((ages[1::2] == 1).mean(axis=1) >= 0.75).all()
    for t in range(1, TICKS, 2):  # no solve at t: the estimate moved all the same, with the plan's control
        played = ages[t] == 1
        assert (hist["d_hist"][t][played] != hist["d_hist"][t - 1][played]).any(axis=1).all(), t
    _check(oracle, wl, hist, plant, w_seq, gain, held, "backup plans", ages=ages, solved_at=set(range(0, TICKS, 2)), moved_share=False)


# ---- 5. ownership and life cycle ----
def test_the_callers_d_is_never_written(oracle):
    """a device d given to set_system is read for the seed and stays bit-identical; a plant given as misaligned views takes the copies that go
    double by double and passes the same checks"""
    import torch
    from copra_amd.batch import to_abi_layout
    wl, plant, w_seq, held = _scenario("com", batch=SMALL)
    gain = _gain("dense_each", SMALL, 6)
    Ab, Bb, db, xb = (torch.from_numpy(v).cuda() for v in to_abi_layout(wl["A"], wl["B"], wl["d"], wl["x0"]))
    d_before = db.clone()
    eng = _engine(wl)
    eng.set_system(Ab, Bb, db, xb)
    eng.set_bias_estimator(gain)
    assert eng.bias_ptr() not in (0, db.data_ptr())
    pa, pb, pd = to_abi_layout(*plant, wl["x0"])[:3]

    def misaligned(a):  # a view 8 bytes into a 16-byte aligned buffer
        buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
        view = buf[1:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        return view
    hist = _numpy(eng.rollout(TICKS, plant=(misaligned(pa), misaligned(pb), misaligned(pd)), disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True,
                              d_hist=True))
    assert torch.equal(db, d_before) and torch.equal(xb, torch.from_numpy(wl["x0"]).cuda())
    _check(oracle, wl, hist, plant, w_seq, gain, held, "device d, misaligned plant", moved_share=False)
    aligned = _engine(wl)
    aligned.set_bias_estimator(gain)
    twin = _rollout(aligned, TICKS, w_seq, plant)
    assert np.abs(twin["d_hist"] - hist["d_hist"]).max() <= ROUTES and np.array_equal(twin["status_hist"], hist["status_hist"])


def test_life_cycle(oracle):
    import torch
    wl, plant, w_seq, held = _scenario("com", batch=SMALL)
    nu = 3
    gain = _gain("diag_shared", SMALL, 6)
    eng = _engine(wl)
    eng.set_bias_estimator(gain)
    hist = _rollout(eng, 4, w_seq[:4], plant)
    last = hist["d_hist"][-1]
    assert np.array_equal(eng.bias(), last) and (last != wl["d"]).any()
    # None ends the estimator and keeps the last estimate in force: the next solve matches the oracle with it, and a tick no longer moves it
    eng.set_bias_estimator(None)
    eng.solve()
    res = eng.results()
    ref = oracle.lmpc_solve_batch(wl["A"], wl["B"], last, hist["x_hist"][-1], wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
    ok = ref["status"] == 0
    assert np.array_equal(res["status"], ref["status"]) and ok.sum() >= SMALL - 8
    assert float(rel(res["control"][ok, :nu], ref["control"][ok, :nu]).max()) <= RTOL
    other = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], hist["x_hist"][-1], wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
    assert (rel(other["control"][ok, :nu], ref["control"][ok, :nu]).max(axis=1) > 1e-3).mean() >= 0.5  # (the estimate matters here)
    out = eng.advance(plant=plant, d_out=True)
    assert np.array_equal(eng.bias(), last)
    # on again: the estimates in force are kept; advance(d_out=) is the rollout's first d_hist
    eng.set_x0(wl["x0"])
    eng.set_bias_estimator(gain)
    assert np.array_equal(eng.bias(), last)
    # set_system while on restarts from the new d, which is copied
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    assert np.array_equal(eng.bias(), wl["d"])
    eng.solve()
    out = eng.advance(plant=plant, disturbance=torch.from_numpy(w_seq[0]).cuda(), d_out=True)
    d1 = out["d_out"].cpu().numpy()
    assert np.abs(d1 - hist["d_hist"][0]).max() <= ROUTES and np.array_equal(eng.bias(), d1)
    # set_bias restarts (a new episode), from the host and from the device
    eng.set_bias(wl["d"] + 1.0)
    assert np.array_equal(eng.bias(), wl["d"] + 1.0)
    eng.set_bias(torch.from_numpy(wl["d"]).cuda())
    eng.set_x0(wl["x0"])
    again = _rollout(eng, 4, w_seq[:4], plant)
    assert np.abs(again["d_hist"] - hist["d_hist"]).max() <= ROUTES and np.array_equal(again["status_hist"], hist["status_hist"])
    # the estimator off: d_out is not written, the tick is the tick of ABI 10
    never = _engine(wl)
    marker = torch.full((SMALL, 6), -7.0, dtype=torch.float64, device="cuda")
    never.solve()
    never.advance(plant=plant, d_out=marker)
    never.synchronize()
    assert (marker == -7.0).all() and np.array_equal(never.bias(), wl["d"])


def test_errors_of_the_header():
    from copra_amd import BatchLMPC, _capi
    wl, plant, w_seq, held = _scenario("com", batch=SMALL)
    gain = np.ones(6)
    fresh = BatchLMPC(6, 3, wl["N"], SMALL, wl["costs"], wl["cstrs"])
    with pytest.raises(_capi.CopraRuntimeError):  # no system yet
        fresh.set_bias_estimator(gain)
    fresh.set_bias_estimator(None)  # (ending what never began is no error)
    with pytest.raises(_capi.CopraDomainError):
        fresh.set_bias_estimator(np.ones(5))
    eng = _engine(wl)
    with pytest.raises(_capi.CopraRuntimeError):  # the library's estimates are not the d in force
        eng.set_bias(wl["d"])
    with pytest.raises(ValueError):  # COPRA_ERR_ARG: a NULL d
        _capi.check(eng._lib.copra_batch_set_bias(eng._h, None, 0))
    # one model for the batch: written out per instance at this shape, or on the shared-model kernels -- refused both ways
    for opts in ({}, {"no_axis_solver": 1}):
        sh = _engine(wl, shared_model=True, options=opts)
        with pytest.raises(_capi.CopraUnsupported):
            sh.set_bias_estimator(gain)
    # ... and set_shared_system ends an estimator that is on
    eng.set_bias_estimator(gain)
    eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
    eng.set_x0(wl["x0"])
    eng.rollout(2)  # (the tick of a shared model, without an estimator)
    with pytest.raises(_capi.CopraUnsupported):
        eng.set_bias_estimator(gain)
    pb = __import__("fixtures").bounded_system("trajectory", N=12)
    ise = BatchLMPC(2, 1, 12, 4, pb["costs"], pb["cstrs"], initial_state=dict(R=1e-2 * np.eye(2), r=np.zeros(2)))
    with pytest.raises(_capi.CopraUnsupported):
        ise.set_bias_estimator(np.ones(2))
