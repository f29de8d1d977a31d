"""Backup plans in the tick on the device (copra_batch_set_backup_steps; BatchLMPC.set_backup_steps, advance(age_out=), rollout(age_hist=,
solve_every=)) against the CPU oracle and numpy's plant step, tick by tick, batch 64 and ten ticks throughout.

The scenario makes every branch of the rule happen at known ticks: a kick of +50 on the first velocity (state index 3; the bound is 0.6) makes
an instance infeasible from the next tick on, a kick of -50 brings it back -- unless its state is being held, then the kick never arrives.
  G1 (3, 17): +50 at tick 1, -50 at tick 3     G2 (8, 40): +50 at tick 1     G3 (21, 63): +50 at tick 1, -50 at tick 7
  G4 (0, 33): no kick, they start with x0[b, 3] = 50 and never solve
The expected age columns below are asserted exactly: that is the condition that the run went through every branch.

Measures: statuses equal to the oracle's from the device's own x_hist[t] at every tick with a solve; controls entry-wise 1e-6 with the floor 1e-3
(the parity suite's, as tests/test_closed_loop_gpu.py) -- the first control where the age is 0, entries j nu .. (j + 1) nu of the oracle's control
of tick t - j where the age is j >= 1; the plant step within the bound derived in tests/test_closed_loop_abi.py wherever a control was applied;
held states bit for bit."""
import ctypes

import numpy as np
import pytest

from test_closed_loop_gpu import RTOL, STUCK, _assert_step, _engine, _rel

pytestmark = pytest.mark.gpu

BATCH, TICKS, K = 64, 10, 3
G1, G2, G3, G4 = (3, 17), (8, 40), (21, 63), (0, 33)
FALLBACK, HELD = -1, -2
AGES = {  # [with a fallback control][group]
    False: {G1: [0, 0, 1, 2, 0, 0, 0, 0, 0, 0], G2: [0, 0, 1, 2, 3] + [HELD] * 5, G3: [0, 0, 1, 2, 3] + [HELD] * 5, G4: [HELD] * 10},
    True: {G1: [0, 0, 1, 2, 0, 0, 0, 0, 0, 0], G2: [0, 0, 1, 2, 3] + [FALLBACK] * 5, G3: [0, 0, 1, 2, 3, FALLBACK, FALLBACK, FALLBACK, 0, 0],
           G4: [FALLBACK] * 10},
}
# solve_every = k, no fallback: a held instance never receives its second kick, so G3 goes the way of G2
AGES_EVERY = {
    2: {None: [0, 1] * 5, G1: [0, 1, 2, 3, 0, 1, 0, 1, 0, 1], G2: [0, 1, 2, 3] + [HELD] * 6, G3: [0, 1, 2, 3] + [HELD] * 6, G4: [HELD] * 10},
    4: {None: [0, 1, 2, 3, 0, 1, 2, 3, 0, 1], G1: [0, 1, 2, 3, 0, 1, 2, 3, 0, 1], G2: [0, 1, 2, 3] + [HELD] * 6, G3: [0, 1, 2, 3] + [HELD] * 6,
        G4: [HELD] * 10},
}


def _columns(table, default):
    """(ticks, batch) ages: `default` for every instance outside the groups of `table`"""
    want = np.tile(np.asarray(default, dtype=np.int32)[:, None], (1, BATCH))
    for group, col in table.items():
        if group is not None:
            want[:, list(group)] = np.asarray(col, dtype=np.int32)[:, None]
    return want


def _scenario(name, kicks=True):
    from copra_amd import workloads
    wl = {"com": workloads.com_preview, "jerk": workloads.jerk_preview}[name](BATCH) if name != "double_integrator" else workloads.double_integrator(BATCH, N=16)
    wl = dict(wl, x0=wl["x0"].copy())
    nx = wl["B"].shape[1]
    npos = 3 if kicks else 1
    w_seq = np.zeros((TICKS, BATCH, nx))
    w_seq[:, :, :npos] = 0.002 * np.random.default_rng(5).standard_normal((TICKS, BATCH, npos))
    if kicks:
        for group, when in ((G1, ((1, 50.0), (3, -50.0))), (G2, ((1, 50.0),)), (G3, ((1, 50.0), (7, -50.0)))):
            for t, kick in when:
                w_seq[t, list(group), 3] += kick
        wl["x0"][list(G4), 3] = 50.0
    return wl, w_seq


def _numpy(hist):
    return {k: v.cpu().numpy() for k, v in hist.items() if v is not None}


def _check(oracle, wl, hist, w_seq, plant, fallback, want_ages, every, what):
    """every tick of a rollout with backup plans; hist holds numpy arrays"""
    xh, uh, sh, ah = hist["x_hist"], hist["u_hist"], hist["status_hist"], hist["age_hist"]
    A, B, d = plant
    nu = wl["B"].shape[2]
    assert not np.isnan(xh).any()
    assert np.array_equal(ah, want_ages), (what, [(b, ah[:, b].tolist()) for b in np.nonzero((ah != want_ages).any(axis=0))[0][:4]])
    refs = {}
    for t in range(uh.shape[0]):
        age = ah[t]
        if every <= 1 or t % every == 0:
            refs[t] = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], xh[t], wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
            assert np.array_equal(sh[t], refs[t]["status"]), (what, t)
            assert np.array_equal(age == 0, sh[t] == 0), (what, t)  # on a tick with a solve: a fresh control exactly where it solved
        else:
            assert np.array_equal(sh[t], sh[t - t % every]) and (age != 0).all(), (what, t)  # the last solve's status, stale
        for j in range(0, K + 1):
            m = age == j
            if not m.any():
                continue
            e = _rel(uh[t][m], refs[t - j]["control"][m, j * nu:(j + 1) * nu])
            print("%s tick %d: %d instances at age %d, control against the oracle's of tick %d: %.2e" % (what, t, m.sum(), j, t - j, e))
            assert e <= RTOL, (what, t, j)
        moved = age != HELD
        _assert_step(xh[t + 1], A, B, d, xh[t], np.where(moved[:, None], uh[t], 0.0), w_seq[t], moved, "%s tick %d" % (what, t))
        assert np.array_equal(xh[t + 1][~moved], xh[t][~moved]), (what, t)  # held, bit for bit
        assert np.array_equal(np.isnan(uh[t]).any(axis=1), ~moved), (what, t)
        if fallback is not None:
            assert np.array_equal(uh[t][age == FALLBACK], fallback[age == FALLBACK]), (what, t)
        else:
            assert not (age == FALLBACK).any()


def _rollout(eng, w_seq, fallback=None, **kw):
    return _numpy(eng.rollout(TICKS, disturbances=w_seq, fallback_control=fallback, x_hist=True, u_hist=True, status_hist=True, age_hist=True, **kw))


@pytest.mark.parametrize("name", ["com", "jerk"])
@pytest.mark.parametrize("with_fb", [False, True])
def test_scenario_against_the_oracle(oracle, name, with_fb):
    wl, w_seq = _scenario(name)
    fb = np.zeros((BATCH, wl["B"].shape[2])) if with_fb else None
    eng = _engine(wl)
    eng.set_backup_steps(K)
    hist = _rollout(eng, w_seq, fb)
    assert np.array_equal(hist["x_hist"][0], wl["x0"])
    _check(oracle, wl, hist, w_seq, (wl["A"], wl["B"], wl["d"]), fb, _columns(AGES[with_fb], [0] * TICKS), 1, name + (" with fallback" if with_fb else ""))


@pytest.mark.parametrize("with_fb", [False, True])
def test_a_played_control_is_the_stored_tail_bit_for_bit(with_fb):
    """a second route, solve() / results() / advance(): where the age is j >= 1 the applied control is entries j nu .. (j + 1) nu of the device's
    own results()["control"] of tick t - j, bit for bit; the ages are the scenario's"""
    import torch
    wl, w_seq = _scenario("com")
    nu = 3
    fb = np.zeros((BATCH, nu)) if with_fb else None
    eng = _engine(wl)
    eng.set_backup_steps(K)
    wd = torch.from_numpy(w_seq).cuda()
    fbd = None if fb is None else torch.from_numpy(fb).cuda()
    controls, ages, played = [], [], 0
    for t in range(TICKS):
        eng.solve()
        controls.append(eng.results()["control"])
        o = eng.advance(disturbance=wd[t], fallback_control=fbd, u_out=True, age_out=True)
        age, u = o["age_out"].cpu().numpy(), o["u_out"].cpu().numpy()
        ages.append(age)
        for b in np.nonzero(age >= 1)[0]:
            j = int(age[b])
            assert u[b].tobytes() == controls[t - j][b, j * nu:(j + 1) * nu].tobytes(), (t, b, j)
            played += 1
        ok = age == 0
        assert u[ok].tobytes() == controls[t][ok, :nu].tobytes()
    assert np.array_equal(np.stack(ages), _columns(AGES[with_fb], [0] * TICKS))
    assert played == 2 * (2 + 3 + 3)


@pytest.mark.parametrize("name", ["com", "double_integrator"])
@pytest.mark.parametrize("every", [2, 4])
def test_multi_rate(oracle, name, every):
    """solve_every = k: the plant runs every tick, the controller every k-th; the oracle runs at the solve ticks only"""
    import torch
    kicks = name == "com"
    wl, w_seq = _scenario(name, kicks=kicks)
    table = AGES_EVERY[every] if kicks else {}
    want = _columns(table, AGES_EVERY[every][None])
    eng = _engine(wl)
    if name == "double_integrator":
        assert eng.lanes_per_instance() in (16, 32)  # the packed kernels
    eng.set_backup_steps(K)
    hist = _rollout(eng, w_seq, solve_every=every)
    _check(oracle, wl, hist, w_seq, (wl["A"], wl["B"], wl["d"]), None, want, every, "%s, a solve every %d ticks" % (name, every))
    # ... and the loop a caller would write: solve(); advance() at the solve ticks, advance() alone at the others
    twin = _engine(wl)
    twin.set_backup_steps(K)
    wd = torch.from_numpy(w_seq).cuda()
    xs, ages = [wl["x0"]], []
    for t in range(TICKS):
        if t % every == 0:
            twin.solve()
        ages.append(twin.advance(disturbance=wd[t], age_out=True)["age_out"].cpu().numpy())
        xs.append(twin.state())
    assert np.array_equal(np.stack(ages), want)
    dmax = np.abs(hist["x_hist"] - np.stack(xs)).max()
    print("rollout(solve_every=%d) against the loop: max difference of the states %.2e" % (every, dmax))
    assert dmax <= 1e-9  # (the figure of test_rollout_is_the_loop)


def test_multi_rate_needs_a_plan_long_enough():
    wl, _ = _scenario("com")
    eng = _engine(wl)
    eng.set_backup_steps(2)
    with pytest.raises(ValueError):  # COPRA_ERR_ARG: k = 4 needs K >= 3
        eng.rollout(4, solve_every=4)
    with pytest.raises(ValueError):
        eng.rollout(4, solve_every=-1)
    eng.rollout(4, solve_every=3)
    eng.set_backup_steps(0)
    with pytest.raises(ValueError):
        eng.rollout(4, solve_every=2)
    eng.rollout(2, solve_every=1)
    eng.rollout(2, solve_every=0)


def test_lifecycle():
    """K outside 0 .. N - 1 is refused; the setter forgets every plan, also when it repeats the K in force"""
    from copra_amd import BatchLMPC, _capi
    wl, w_seq = _scenario("com")
    eng, twin = _engine(wl), _engine(wl)
    for bad in (-1, wl["N"], wl["N"] + 5):
        with pytest.raises(ValueError):
            eng.set_backup_steps(bad)
    eng.set_backup_steps(wl["N"] - 1)
    for e in (eng, twin):
        e.set_backup_steps(K)
        e.rollout(2, disturbances=w_seq[:2])  # (every kicked instance has a plan now and will fail at the next tick)
    eng.set_backup_steps(K)
    kicked = list(G1 + G2 + G3)
    a = eng.rollout(1, disturbances=w_seq[2:3], age_hist=True)["age_hist"].cpu().numpy()[0]
    b = twin.rollout(1, disturbances=w_seq[2:3], age_hist=True)["age_hist"].cpu().numpy()[0]
    assert (a[kicked] == HELD).all() and (b[kicked] == 1).all()
    rest = np.setdiff1d(np.arange(BATCH), kicked + list(G4))
    assert (a[rest] == 0).all() and (b[rest] == 0).all() and (a[list(G4)] == HELD).all()
    pb = __import__("fixtures").bounded_system("trajectory", N=12)
    ise = BatchLMPC(2, 1, 12, 4, pb["costs"], pb["cstrs"], initial_state=dict(R=1e-2 * np.eye(2), r=np.zeros(2)))
    with pytest.raises(_capi.CopraUnsupported):
        ise.set_backup_steps(1)


def test_a_caller_built_against_abi_9():
    """a copra_plant_step_t whose struct_size is the ABI-9 size: the tick is the one every other caller gets -- backup plans are state of the
    handle --, only age_out, which lies beyond that size, is not written"""
    import torch
    from copra_amd import _capi
    wl, w_seq = _scenario("com")
    eng, twin = _engine(wl), _engine(wl)
    wd = torch.from_numpy(w_seq).cuda()
    abi9 = _capi.PlantStep.age_out.offset
    assert abi9 == 80 and abi9 < ctypes.sizeof(_capi.PlantStep)
    L = _capi.lib()
    for K_set in (K, 0):
        for e in (eng, twin):
            e.set_x0(wl["x0"])
            e.set_backup_steps(K_set)
        for t in range(4):  # (tick 2 plays a plan where K > 0)
            twin.solve()
            o = twin.advance(disturbance=wd[t], u_out=True, status_out=True, age_out=True)
            eng.solve()
            u = torch.full((BATCH, 3), 7.0, dtype=torch.float64, device="cuda")
            s = torch.full((BATCH,), -5, dtype=torch.int32, device="cuda")
            age = torch.full((BATCH,), -99, dtype=torch.int32, device="cuda")
            st = _capi.PlantStep()
            L.copra_plant_step_init(ctypes.byref(st))
            st.w, st.u_out, st.status_out, st.age_out = wd[t].data_ptr(), u.data_ptr(), s.data_ptr(), age.data_ptr()
            st.struct_size = abi9
            _capi.check(L.copra_batch_advance(eng._h, ctypes.byref(st), None))
            assert np.array_equal(eng.state(), twin.state()), (K_set, t)
            assert np.array_equal(u.cpu().numpy(), o["u_out"].cpu().numpy(), equal_nan=True) and torch.equal(s, o["status_out"])
            assert (age == -99).all()
        want = [0, 0, 1, 2] if K_set else [0, 0, HELD, HELD]
        assert o["age_out"].cpu().numpy()[list(G2)].tolist() == [want[3]] * 2


def test_off_is_the_tick_of_abi_9():
    """K = 0: histories bit-identical to an engine on which the setter was never called"""
    from copra_amd import workloads
    wl = workloads.com_preview(512)
    wl = dict(wl, x0=wl["x0"].copy())
    for b in STUCK:
        wl["x0"][b, 3] = 50.0
    w_seq = np.zeros((8, 512, 6))
    w_seq[:, :, :3] = 0.002 * np.random.default_rng(6).standard_normal((8, 512, 3))
    eng, never = _engine(wl), _engine(wl)
    eng.set_backup_steps(K)
    eng.set_backup_steps(0)
    a = eng.rollout(8, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True, age_hist=True)
    b = never.rollout(8, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True)
    for k in ("x_hist", "u_hist", "status_hist"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    age = a["age_hist"].cpu().numpy()
    assert np.array_equal(age == HELD, a["status_hist"].cpu().numpy() != 0) and (age[:, list(STUCK)] == HELD).all() and ((age == 0) | (age == HELD)).all()


@pytest.mark.parametrize("mode", ["shared_model", "other_plant"])
def test_shared_model_and_other_plant(oracle, mode):
    """the plan is applied to the PLANT: nothing is taken from the model's trajectory"""
    wl, w_seq = _scenario("com")
    shared_model = mode == "shared_model"
    if shared_model:
        wl["A"], wl["B"], wl["d"] = (np.ascontiguousarray(np.broadcast_to(wl[k][0], wl[k].shape)) for k in ("A", "B", "d"))
    eng = _engine(wl, shared_model=shared_model)
    eng.set_backup_steps(K)
    plant, kw = (wl["A"], wl["B"], wl["d"]), {}
    if mode == "other_plant":
        plant = (wl["A"], 0.9 * wl["B"], wl["d"])
        kw = dict(plant=plant)
    hist = _rollout(eng, w_seq, **kw)
    _check(oracle, wl, hist, w_seq, plant, None, _columns(AGES[False], [0] * TICKS), 1, mode)
