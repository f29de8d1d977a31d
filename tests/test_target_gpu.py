"""Steady-state targets on the device (copra_batch_set_target, ABI 15; BatchLMPC.set_target / target / target_status / cost_reference): the
steady states and the driven costs' references against tests/target_ref.py with the bound of tests/test_target_abi.py
(|z - z_true|_inf <= n^2 cond_inf(M) 2^-53 |z_true|_inf, for a reference row in addition (n + 1) 2^-53 (|T| |z|)_i; z_true in extended
precision); after every launch point (set_target, advance, schedule_seek, set_bias, set_system); one solve with the written references
against the CPU oracle; the device loop against the host-driven loop; the point of the feature; the combinations; the errors."""
import numpy as np
import pytest

import target_ref
from test_closed_loop_gpu import RTOL, _engine
from tracking_cases import rel

pytestmark = pytest.mark.gpu

WORST = {"z": 0.0, "p": 0.0}


def _wl(name, batch):
    from copra_amd import workloads
    if name == "double_integrator":
        return workloads.double_integrator(batch)
    return getattr(workloads, name)(batch)


def _outputs(nx, nu):
    """the controlled outputs: the first nu states (the positions of every workload here)"""
    return np.eye(nx)[:nu]


def _maps(wl):
    nx, nu = wl["B"].shape[1], wl["B"].shape[2]
    return [target_ref.step_map(c, nx, nu, wl["N"])[0] for c in wl["costs"]]


def _check_targets(eng, wl, H, sig, offset=0, what="", singular=(), kept=None, B=None, maps=None, costs=(0, 1)):
    """target(), target_status() and the references of the driven costs (0 and 1; `costs` with their step maps `maps` otherwise) against the
    reference computed from bias() and the schedule tick; kept: (z, [p0, p1, ...]) a singular instance must still hold"""
    A, B = wl["A"], wl["B"] if B is None else B
    batch, nu = A.shape[0], B.shape[2]
    d, tau = eng.bias(), eng.schedule_tick()
    r = target_ref.setpoint(sig, tau, offset, batch)
    M, rhs = target_ref.systems(A, B, d, H, r)
    _, st_rule = target_ref.gepp(M, rhs)
    z, status = eng.target(), eng.target_status()
    assert np.array_equal(status, st_rule), (what, np.nonzero(status != st_rule)[0][:8])
    for i in singular:
        assert status[i] == 1, (what, i)
    assert status.sum() == len(singular), what
    good = status == 0
    zt = target_ref.solve_true(M[good], rhs[good])
    bound = target_ref.z_bound(M[good], zt)
    e64 = np.abs(target_ref.solve64(M[good], rhs[good]) - zt).max(axis=1).astype(np.float64)
    assert (e64 <= bound).all(), what  # numpy's own float64 solve stays inside the bound
    err = np.abs(z[good] - zt).max(axis=1).astype(np.float64)
    assert np.isfinite(z[good]).all() and (err <= bound).all(), (what, float((err / bound).max()))
    WORST["z"] = max(WORST["z"], float((err / bound).max()))
    refs = [eng.cost_reference(k) for k in costs]
    for k, T in enumerate(_maps(wl) if maps is None else maps):
        p, pb = target_ref.p_true_and_bound(T, M[good], zt)
        S = refs[k].shape[1] // T.shape[0]
        got = refs[k][good].reshape(int(good.sum()), S, T.shape[0])
        for s in range(S):
            ep = np.abs(got[:, s] - p)
            assert np.isfinite(got).all() and (ep <= pb).all(), (what, k, s, float((ep / pb).max()))
            WORST["p"] = max(WORST["p"], float((ep / np.maximum(pb, 1e-300)).max()))
    if kept is not None:
        bad = ~good
        assert z[bad].tobytes() == kept[0][bad].tobytes(), what
        for k in range(len(refs)):
            assert refs[k][bad].tobytes() == kept[1][k][bad].tobytes(), (what, k)
    print("%s: largest error / bound so far: z %.3g, references %.3g" % (what, WORST["z"], WORST["p"]))
    return z, refs


# ---- 1 ----
@pytest.mark.parametrize("name,batch", [("com_preview", 65), ("jerk_preview", 300), ("double_integrator", 65), ("com_preview", 1)])
def test_targets_and_references_after_set_target(name, batch):
    """shapes (6, 3), (9, 3) and (2, 1); a zero column of B and a NaN in d among good instances: status 1, z at its zeros, the references at
    the ones given at creation"""
    wl = _wl(name, batch)
    nx, nu = wl["B"].shape[1], wl["B"].shape[2]
    rng = np.random.default_rng(batch + nx)
    wl["d"] = wl["d"] + 0.004 * rng.uniform(-1, 1, wl["d"].shape)
    singular = ()
    if batch > 1:
        singular = (2, 64)
        wl["B"][2][:, nu - 1] = 0.0
        wl["d"][64][0] = np.nan
    H = _outputs(nx, nu)
    sig = rng.standard_normal((batch, 3, nu)) if batch > 1 else rng.standard_normal(nu)
    eng = _engine(wl)
    eng.set_target(H, sig, [0, 1], offset=1)
    assert eng.target_ptr != 0
    created = [np.tile(np.asarray(c["p"], dtype=np.float64), (batch, 1)) for c in wl["costs"]]
    _check_targets(eng, wl, H, sig, offset=1, what="%s x %d after set_target" % (name, batch), singular=singular, kept=(np.zeros((batch, nx + nu)), created))
    eng.set_target(None)
    assert eng.target_ptr == 0
    assert eng.cost_reference(0).shape == (batch, nx)  # (the last references are kept)


# ---- 2 ----
def _loaded(batch, seed=4, load=0.004):
    """the CoM fleet under a constant load per instance (the plant's d), instance 0 without one"""
    wl = _wl("com_preview", batch)
    rng = np.random.default_rng(seed)
    c = load * rng.uniform(-1.0, 1.0, (batch, 6))
    c[0] = 0.0
    return wl, (wl["A"], wl["B"], wl["d"] + c), c


def test_targets_follow_the_estimates_and_every_launch_point():
    batch = 65
    wl, plant, c = _loaded(batch)
    H = _outputs(6, 3)
    rng = np.random.default_rng(1)
    sig = np.asarray(wl["costs"][0]["p"])[:3] + 0.05 * rng.standard_normal((4, 3))  # a goal that moves for three ticks, then stays
    eng = _engine(wl)
    eng.set_bias_estimator(np.ones(6))
    eng.set_target(H, sig, [0, 1])
    for t in range(5):
        eng.solve()
        eng.advance(plant=plant)
        assert eng.schedule_tick() == t + 1
        _check_targets(eng, wl, H, sig, what="tick %d" % t)
    assert np.abs(eng.bias() - plant[2]).max() <= 1e-12  # (gain 1, no noise: the load is known)
    eng.schedule_seek(1)
    z1, _ = _check_targets(eng, wl, H, sig, what="after schedule_seek")
    eng.schedule_seek(9)
    z9, _ = _check_targets(eng, wl, H, sig, what="after schedule_seek past the end")
    assert np.abs(z1 - z9).max() > 1e-3
    eng.set_bias(wl["d"] + 2.0 * c)
    z2, _ = _check_targets(eng, wl, H, sig, what="after set_bias")
    assert np.abs(z2 - z9)[1:].max() > 1e-6 and np.abs(z2[0] - z9[0]).max() <= 1e-12  # (instance 0 carries no load)
    B2 = wl["B"] * rng.uniform(0.8, 1.2, (batch, 1, 1))
    eng.set_system(wl["A"], B2, wl["d"] + c, eng.state())
    z3, _ = _check_targets(eng, wl, H, sig, what="after set_system", B=B2)
    assert np.abs(z3 - z2).max() > 1e-6


# ---- 3 ----
def _oracle_with_references(oracle, wl, x0, d, refs):
    """the CPU oracle instance by instance, cost k's p replaced by refs[k][i]"""
    batch = x0.shape[0]
    out = dict(control=[], trajectory=[], status=[], iter=[])
    for i in range(batch):
        costs = [dict(c, p=refs[k][i]) for k, c in enumerate(wl["costs"])]
        r = oracle.lmpc_solve_batch(wl["A"][i:i + 1], wl["B"][i:i + 1], d[i:i + 1], x0[i:i + 1], wl["N"], costs, wl["cstrs"])
        for k in out:
            out[k].append(r[k][0])
    return {k: np.stack(v) for k, v in out.items()}


@pytest.mark.parametrize("options", [None, dict(no_axis_solver=1)], ids=["axis solver", "no_axis_solver"])
def test_one_solve_with_the_written_references_against_the_oracle(oracle, options):
    """catches a solver build that ignores a per-instance ControlCost reference: us is far from zero under these loads"""
    batch = 65
    wl, plant, c = _loaded(batch, load=0.05)
    wl["d"] = plant[2]  # the model knows the load: d is what the targets read
    H = _outputs(6, 3)
    eng = _engine(wl, options=options)
    eng.set_target(H, np.asarray(wl["costs"][0]["p"])[:3], [0, 1])
    refs = [eng.cost_reference(k) for k in (0, 1)]
    assert np.abs(refs[1]).max() > 0.3  # (the ControlCost's reference is not the zero it was created with)
    eng.solve()
    res = eng.results()
    ref = _oracle_with_references(oracle, wl, wl["x0"], wl["d"], refs)
    assert np.array_equal(res["status"], ref["status"]) and (res["status"] == 0).all()
    assert np.array_equal(res["iter"], ref["iter"])
    for k in ("control", "trajectory"):
        e = float(rel(res[k], ref[k]).max())
        print("%s against the oracle with the same references: %.2e" % (k, e))
        assert e <= RTOL, k
    zero = _oracle_with_references(oracle, wl, wl["x0"], wl["d"], [refs[0], np.zeros_like(refs[1])])
    assert float(rel(zero["control"], ref["control"]).max()) > 100 * RTOL  # (the ControlCost's reference matters)


# ---- 4, 5 ----
TICKS = 40


def _host_targets(wl, H, goal, d):
    """the host's own target calculation: numpy's solve per instance; (xs, us)"""
    batch = d.shape[0]
    M, rhs = target_ref.systems(wl["A"], wl["B"], d, H, np.tile(goal, (batch, 1)))
    z = target_ref.solve64(M, rhs)
    return z[:, :6], z[:, 6:]


@pytest.fixture(scope="module")
def loops():
    """the same fleet, load and estimator (gain 1) four times: the device loop as one rollout, as 40 x (solve, advance), the host-driven
    loop (bias(), a numpy target calculation and two set_cost_reference per tick) and the loop without targets"""
    import torch
    batch = 65
    wl, plant, c = _loaded(batch)
    H = _outputs(6, 3)
    goal = np.asarray(wl["costs"][0]["p"], dtype=np.float64)[:3]
    out = dict(wl=wl, c=c, goal=goal)

    def fresh(targets):
        eng = _engine(wl)
        eng.set_bias_estimator(np.ones(6))
        if targets:
            eng.set_target(H, goal, [0, 1])
        return eng

    eng = fresh(True)
    h = eng.rollout(TICKS, plant=plant, x_hist=True, u_hist=True, status_hist=True)
    torch.cuda.synchronize()
    out["rollout"] = {k: h[k].cpu().numpy() for k in ("x_hist", "u_hist", "status_hist")}
    out["rollout_z"] = eng.target()

    eng = fresh(True)
    xs, us, ss = [eng.state()], [], []
    for t in range(TICKS):
        eng.solve()
        o = eng.advance(plant=plant, x_out=True, u_out=True, status_out=True)
        xs.append(o["x_out"].cpu().numpy()), us.append(o["u_out"].cpu().numpy()), ss.append(o["status_out"].cpu().numpy())
    out["steps"] = dict(x_hist=np.stack(xs), u_hist=np.stack(us), status_hist=np.stack(ss))

    eng = fresh(False)
    xs, us, ss = [eng.state()], [], []
    for t in range(TICKS):
        x_s, u_s = _host_targets(wl, H, goal, eng.bias())
        eng.set_cost_reference(0, x_s)
        eng.set_cost_reference(1, u_s)
        eng.solve()
        o = eng.advance(plant=plant, x_out=True, u_out=True, status_out=True)
        xs.append(o["x_out"].cpu().numpy()), us.append(o["u_out"].cpu().numpy()), ss.append(o["status_out"].cpu().numpy())
    out["host"] = dict(x_hist=np.stack(xs), u_hist=np.stack(us), status_hist=np.stack(ss))

    eng = fresh(False)
    h = eng.rollout(TICKS, plant=plant, x_hist=True, status_hist=True)
    torch.cuda.synchronize()
    out["without"] = {k: h[k].cpu().numpy() for k in ("x_hist", "status_hist")}
    return out


def test_the_device_loop_is_the_host_driven_loop(loops):
    dev, host = loops["rollout"], loops["host"]
    assert np.array_equal(dev["status_hist"], host["status_hist"])
    for t in range(TICKS):
        ex, eu = float(rel(dev["x_hist"][t + 1], host["x_hist"][t + 1]).max()), float(rel(dev["u_hist"][t], host["u_hist"][t]).max())
        assert ex <= RTOL and eu <= RTOL, (t, ex, eu)
    print("device loop against the host-driven loop over %d ticks: states %.2e, controls %.2e" % (
        TICKS, float(rel(dev["x_hist"], host["x_hist"]).max()), float(rel(dev["u_hist"], host["u_hist"]).max())))


def test_rollout_is_the_loop_of_solves_and_advances(loops):
    """the same launches in the same order: the same bits"""
    for k in ("x_hist", "u_hist", "status_hist"):
        assert loops["rollout"][k].tobytes() == loops["steps"][k].tobytes(), k


def test_the_targets_take_the_offset_away(loops):
    goal, c = loops["goal"], loops["c"]
    dist = lambda h: np.linalg.norm(h["x_hist"][-1][:, :3] - goal, axis=1)  # noqa: E731
    with_t, without, host = dist(loops["rollout"]), dist(loops["without"]), dist(loops["host"])
    assert (loops["rollout"]["status_hist"] == 0).all() and (loops["without"]["status_hist"] == 0).all()
    loaded = np.abs(c).max(axis=1) > 0
    assert loaded.sum() == len(c) - 1
    print("mean distance to the setpoint after %d ticks: with targets %.3e, without %.3e, host-driven %.3e" % (TICKS, with_t.mean(), without.mean(), host.mean()))
    assert (with_t[loaded] < without[loaded]).all(), np.nonzero(~(with_t < without))[0][:8]
    assert float(rel(with_t, host).max()) <= RTOL  # (the suite's parity rule: 1e-6 entry-wise with a floor of 1e-3)


# ---- 6 ----
@pytest.mark.parametrize("combo", ["backup", "observer", "noise", "score"])
def test_combinations(combo):
    batch, ticks = 65, 6
    wl, plant, c = _loaded(batch)
    H = _outputs(6, 3)
    rng = np.random.default_rng(8)
    sig = np.asarray(wl["costs"][0]["p"])[:3] + 0.02 * rng.standard_normal((batch, 3, 3))
    eng = _engine(wl)
    kw = {}
    if combo == "observer":
        C_out = np.eye(6)
        eng.set_observer(C_out, 0.9 * np.eye(6), 0.5 * np.eye(6))
    else:
        eng.set_bias_estimator(np.full(6, 0.7))
    if combo == "backup":
        eng.set_backup_steps(2)
        kw["solve_every"] = 2
    if combo == "noise":
        eng.set_noise(5, process=np.full(6, 1e-3))
    if combo == "score":
        eng.set_score(np.ones(6), np.ones(3))
    eng.set_target(H, sig, [0, 1])
    eng.rollout(ticks, plant=plant, **kw)
    assert eng.schedule_tick() == ticks
    _check_targets(eng, wl, H, sig, what=combo)
    assert np.abs(eng.bias() - wl["d"]).max() > 1e-4  # (the estimates moved, and the targets with them)
    if combo == "score":
        assert (eng.score()["ticks"] == ticks).all()


# ---- 7 ----
def test_error_codes():
    import ctypes as C

    from copra_amd import BatchLMPC, CopraDomainError, CopraRuntimeError, CopraUnsupported, _capi, workloads
    batch = 4
    wl = _wl("com_preview", batch)
    H, goal = _outputs(6, 3), np.zeros(3)
    eng = BatchLMPC(6, 3, wl["N"], batch, wl["costs"], wl["cstrs"])
    with pytest.raises(CopraRuntimeError):
        eng.set_target(H, goal, [0, 1])  # no system set yet
    with pytest.raises(CopraRuntimeError):
        eng.target()  # targets are off
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    eng.set_bias_estimator(np.ones(6))
    with pytest.raises(CopraRuntimeError):
        eng.target_status()
    with pytest.raises(CopraRuntimeError):
        eng.cost_reference(0)  # the controller-wide reference is in force
    eng.set_target(None)  # (ending what never began is no error)
    with pytest.raises(CopraDomainError):
        eng.set_target(np.eye(6)[:2], np.zeros(2), [0])  # outputs of the wrong shape
    with pytest.raises(CopraDomainError):
        eng.set_target(H, np.zeros((batch + 1, 2, 3)), [0])
    with pytest.raises(ValueError):
        eng.set_target(H, goal, [])
    with pytest.raises(ValueError):
        eng.set_target(H, goal, [5])

    def raw(**kw):
        """copra_batch_set_target with one field off"""
        Hc, r = np.ascontiguousarray(H.T), np.zeros(3)
        maps = [np.ascontiguousarray(T.T) for T in _maps(wl)]
        t = _capi.Target()
        eng._lib.copra_target_init(C.byref(t))
        ci, cr, cm = (C.c_int * 2)(0, 1), (C.c_int * 2)(6, 3), (C.c_void_p * 2)(*[m.ctypes.data for m in maps])
        t.nr, t.H, t.r, t.steps, t.offset, t.per_instance, t.n_costs, t.cost_index, t.cost_rows, t.cost_map = 3, Hc.ctypes.data, r.ctypes.data, 1, 0, 0, 2, ci, cr, cm
        for k, v in kw.items():
            if k == "index":
                ci[1] = v
            elif k == "rows":
                cr[0] = v
            elif k == "map":
                cm[1] = v
            else:
                setattr(t, k, v)
        return eng._lib.copra_batch_set_target(eng._h, C.byref(t))

    assert raw() == _capi.COPRA_OK
    for kw in (dict(steps=0), dict(offset=-1), dict(n_costs=0), dict(n_costs=9), dict(index=7), dict(index=-1), dict(index=0), dict(H=None), dict(r=None),
               dict(cost_index=None), dict(cost_rows=None), dict(cost_map=None), dict(map=None), dict(struct_size=0)):
        assert raw(**kw) == _capi.COPRA_ERR_ARG, kw
    assert raw(nr=2) == _capi.COPRA_ERR_DOMAIN
    assert raw(rows=4) == _capi.COPRA_ERR_DOMAIN and raw(rows=0) == _capi.COPRA_ERR_DOMAIN
    assert eng.target().shape == (batch, 9)  # (an attempt refused for its arguments leaves the targets as they were)
    # a driven cost cannot also follow a schedule; the setters of a reference take a cost off the list
    eng.set_reference_schedule(0, np.zeros((3, 6)), 6)
    with pytest.raises(CopraRuntimeError):
        eng.set_target(H, goal, [0, 1])
    eng.set_target(H, goal, [1])  # (cost 1 has none)
    eng.set_reference_schedule(0, None, 6)
    eng.set_target(H, goal + 1.0, [0, 1])
    p0 = eng.cost_reference(0)
    assert np.abs(p0[:, :3] - 1.0).max() < 1e-12
    eng.set_cost_reference(0, np.full(6, 3.0))  # by hand: cost 0 leaves the list, cost 1 stays
    eng.set_bias(wl["d"] + 0.01)
    assert (eng.cost_reference(0) == 3.0).all() and np.abs(eng.cost_reference(1)).max() > 1e-3
    eng.set_reference_schedule(1, np.zeros((2, 3)), 3)
    eng.set_bias(wl["d"])
    assert (eng.cost_reference(1) == 0.0).all() and eng.target_status().sum() == 0
    # one model for the batch: refused, and set_shared_system ends the targets
    eng.set_reference_schedule(1, None, 3)
    eng.set_target(H, goal, [0, 1])
    eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
    with pytest.raises(CopraRuntimeError):
        eng.target()
    with pytest.raises(CopraUnsupported):
        eng.set_target(H, goal, [0, 1])
    # an InitialStateLMPC controller; a dense cost; a full-size cost the controller does not evaluate step by step; an image that does not fit
    li = workloads.long_horizon_initial_state(2, N=6)
    ise = BatchLMPC(12, 6, 6, 2, li["costs"], li["cstrs"], initial_state=li["initial_state"])
    ise.set_system(li["A"], li["B"], li["d"], li["x0"])
    with pytest.raises(CopraUnsupported):
        ise.set_target(np.eye(12)[:6], np.zeros(6), [0, 1])
    n = 3 * wl["N"]
    dense = BatchLMPC(6, 3, wl["N"], batch, wl["costs"] + [dict(kind="dense", Q=np.eye(n), c=np.zeros(n))], wl["cstrs"])
    dense.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    with pytest.raises(CopraUnsupported):
        dense.set_target(H, goal, [2])
    dense.set_target(H, goal, [0, 1])
    N = wl["N"]
    full = dict(kind="trajectory", M=np.kron(np.eye(N + 1), np.eye(6)), p=np.zeros(6 * (N + 1)), weights=np.ones(6 * (N + 1)))
    fs = BatchLMPC(6, 3, N, batch, [full, wl["costs"][1]], wl["cstrs"], options=dict(no_stage_refs=1))
    fs.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    with pytest.raises(CopraUnsupported):
        fs.set_target(H, goal, [0, 1])
    st = BatchLMPC(6, 3, N, batch, [full, wl["costs"][1]], wl["cstrs"])  # ... and one it does: S = N + 1 blocks
    st.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    st.set_target(H, goal, [0, 1])
    p = st.cost_reference(0).reshape(batch, N + 1, 6)
    assert np.abs(p[:, :, :3] - goal).max() < 1e-12 and all(p[:, s].tobytes() == p[:, 0].tobytes() for s in range(N + 1))
    rng = np.random.default_rng(0)
    nx, nu = 14, 4  # (18 x 19 doubles per lane: 175 KB for one wave)
    big = BatchLMPC(nx, nu, 4, 2, [dict(kind="trajectory", M=np.eye(nx), p=np.zeros(nx)), dict(kind="control", N=np.eye(nu), p=np.zeros(nu))],
                    [dict(kind="control_bound", lower=[-1.0] * nu, upper=[1.0] * nu)])
    big.set_system(np.tile(np.eye(nx) * 0.9, (2, 1, 1)), rng.standard_normal((2, nx, nu)), np.zeros((2, nx)), np.zeros((2, nx)))
    with pytest.raises(CopraUnsupported):
        big.set_target(np.eye(nx)[:nu], np.zeros(nu), [0, 1])
