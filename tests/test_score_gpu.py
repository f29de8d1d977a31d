"""Closed-loop scores on the device (copra_batch_set_score, ABI 14; BatchLMPC.set_score / score / score_summary): rollouts of 7 - 10 ticks that
also ask for x_hist, u_hist and age_hist -- the records must equal tests/score_ref.py applied to the device's OWN histories: counters and
viol_max exactly, the sums within the bound tests/test_score_abi.py derives (2 gamma_k S, k = 2 max(nx, nu) + 2 + T: the device may contract a
product and a sum into one rounding, the restatement rounds each); the summary against the records read back, within that file's bound for
the pairwise merge, counts, min, max and args exactly."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import score_ref
from test_backup_plan_gpu import AGES, AGES_EVERY, BATCH, K, TICKS, _columns, _scenario
from test_closed_loop_gpu import _engine
from test_score_abi import check_summary, gamma, merge_depth, sum_ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELD, FALLBACK = score_ref.HELD, score_ref.FALLBACK
MEASURE = ("qx", "ru", "x_ref", "x_lo", "x_hi", "u_lo", "u_hi")


def _numpy(hist):
    return {k: v.cpu().numpy() for k, v in hist.items() if v is not None}


def _com_measure(batch=None, dense=False, seed=0, u_box=1e3):
    """the measure of examples/monte_carlo.py with limits: |p - goal|^2 + 1e-3 |u|^2, the velocity bound 0.6 of the workload, a control box;
    batch: every array per instance; dense: full symmetric weights"""
    rng = np.random.default_rng(seed)
    lead = () if batch is None else (batch,)
    m = dict(dense=dense, per=batch is not None, tol=1e-9)
    if dense:
        m["qx"] = np.eye(6) * [1, 1, 1, 0, 0, 0] + 0.05 * (lambda a: a + np.swapaxes(a, -1, -2))(rng.standard_normal(lead + (6, 6)))
        m["ru"] = 1e-3 * np.eye(3) + 1e-4 * (lambda a: a + np.swapaxes(a, -1, -2))(rng.standard_normal(lead + (3, 3)))
    else:
        m["qx"] = np.broadcast_to(np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0]), lead + (6,)) * rng.uniform(0.5, 1.5, lead + (6,))
        m["ru"] = 1e-3 * rng.uniform(0.5, 1.5, lead + (3,))
    m["x_ref"] = 0.1 * rng.standard_normal(lead + (1, 6))
    m["x_lo"] = np.broadcast_to(np.array([-np.inf] * 3 + [-0.6] * 3), lead + (6,)).copy()
    m["x_hi"] = np.broadcast_to(np.array([np.inf] * 3 + [0.6] * 3), lead + (6,)).copy()
    m["u_lo"], m["u_hi"] = np.full(lead + (3,), -u_box), np.full(lead + (3,), u_box)
    return m


def _set(eng, m):
    eng.set_score(m.get("qx"), m.get("ru"), m.get("x_ref"), (m.get("x_lo"), m.get("x_hi")), (m.get("u_lo"), m.get("u_hi")), tol=m["tol"])


def _replay(hist, m, tau0=0, rec=None, x_key="x_hist"):
    """score_ref over the device's own histories; returns (records, S per field)"""
    xh, uh, ah = hist[x_key], hist["u_hist"], hist["age_hist"]
    ticks, batch = ah.shape
    rec = score_ref.zero_records(batch) if rec is None else rec
    S = {f: np.zeros(batch) for f in ("jx", "ju", "peak")}
    kw = {k: m.get(k) for k in MEASURE}
    off = 1 if xh.shape[0] == ticks + 1 else 0  # (x_hist[0] is the state before the first tick; xhat_hist has no such row)
    for t in range(ticks):
        tau = tau0 + t + 1
        score_ref.update(rec, xh[t + off], uh[t], ah[t], tau, tol=m["tol"], dense=m["dense"], per_instance=m["per"], **kw)
        ax, au = score_ref.abs_terms(xh[t + off], uh[t], ah[t], tau, qx=m.get("qx"), ru=m.get("ru"), x_ref=m.get("x_ref"), dense=m["dense"], per_instance=m["per"])
        S["jx"] += ax
        S["ju"] += au
        S["peak"] = np.maximum(S["peak"], ax + au)
    S["viol_sum"] = rec["viol_sum"].copy()
    return rec, S


def _compare(got, want, S, ticks, what, nx=6, nu=3):
    k = sum_ops(nx, nu, ticks)
    for f in ("ticks", "held", "replayed", "fallback", "violating", "first_violation"):
        assert np.array_equal(got[f], want[f]), (what, f, np.nonzero(got[f] != want[f])[0][:8])
    assert got["viol_max"].tobytes() == want["viol_max"].tobytes(), what
    worst = 0.0
    for f in ("jx", "ju", "viol_sum", "peak"):
        bound = 2.0 * gamma(k) * S[f]
        err = np.abs(got[f] - want[f])
        fin = np.isfinite(want[f])
        assert np.array_equal(np.isfinite(got[f]), fin), (what, f)
        assert (err[fin] <= bound[fin]).all(), (what, f, float(err[fin].max()), float(bound[fin].max()))
        worst = max(worst, float((err[fin] / np.maximum(bound[fin], 1e-300)).max()) if fin.any() else 0.0)
    print("%s: largest error / bound of the sums %.3g" % (what, worst))
    assert (got["ticks"] == ticks).all()


def _rollout(eng, ticks, **kw):
    return _numpy(eng.rollout(ticks, x_hist=True, u_hist=True, age_hist=True, **kw))


# ---- the kick scenario: fresh, replayed, fallback and held ticks at known times ----
@pytest.mark.parametrize("with_fb", [False, True])
def test_the_kick_scenario(with_fb):
    wl, w_seq = _scenario("com")
    fb = np.zeros((BATCH, 3)) if with_fb else None
    m = _com_measure()
    eng = _engine(wl)
    eng.set_backup_steps(K)
    _set(eng, m)
    hist = _rollout(eng, TICKS, disturbances=w_seq, fallback_control=fb)
    ages = _columns(AGES[with_fb], [0] * TICKS)
    assert np.array_equal(hist["age_hist"], ages)
    got = eng.score()
    assert np.array_equal(got["held"], (ages == HELD).sum(axis=0)) and np.array_equal(got["replayed"], (ages >= 1).sum(axis=0))
    assert np.array_equal(got["fallback"], (ages == FALLBACK).sum(axis=0))
    assert (got["held"].sum() == 0) == with_fb and got["replayed"].sum() > 0 and (got["fallback"].sum() > 0) == with_fb
    want, S = _replay(hist, m)
    _compare(got, want, S, TICKS, "kicks%s" % (", fallback" if with_fb else ""))
    kicked = [3, 17, 8, 40, 21, 63, 0, 33]
    assert (got["violating"][kicked] > 0).all() and (got["first_violation"][kicked] >= 1).all()  # a velocity of 50 against a bound of 0.6
    quiet = np.setdiff1d(np.arange(BATCH), kicked)
    assert (got["first_violation"][quiet] == 0).all() and (got["viol_max"][quiet] <= 1e-9).all()  # (a velocity may sit ON its bound)
    s = eng.score_summary()
    assert s["held"] == int(got["held"].sum()) and s["instances_violating"] == int((got["violating"] > 0).sum()) and s["ticks"] == BATCH * TICKS


def test_solve_every_two():
    wl, w_seq = _scenario("com")
    m = _com_measure()
    eng = _engine(wl)
    eng.set_backup_steps(K)
    _set(eng, m)
    hist = _rollout(eng, TICKS, disturbances=w_seq, solve_every=2)
    ages = _columns(AGES_EVERY[2], AGES_EVERY[2][None])
    assert np.array_equal(hist["age_hist"], ages)
    got = eng.score()
    assert np.array_equal(got["replayed"], (ages >= 1).sum(axis=0)) and np.array_equal(got["held"], (ages == HELD).sum(axis=0))
    want, S = _replay(hist, m)
    _compare(got, want, S, TICKS, "solve_every = 2")


# ---- the observer: the scored state is the truth ----
def test_the_observer_is_scored_on_the_plant_state():
    from test_noise_gpu import _observer, _wl
    batch, ticks = 33, 8
    wl = _wl(batch, stuck=(5,))
    m = _com_measure()
    eng = _engine(wl)
    _observer(eng, 6)
    xhat0 = wl["x0"].copy()
    xhat0[:, 3:] += 0.05
    xhat0[5] = wl["x0"][5]
    eng.set_x0(xhat0)
    _set(eng, m)
    plant = (wl["A"], 0.9 * wl["B"], wl["d"])
    hist = _rollout(eng, ticks, plant=plant, xhat_hist=True)
    got = eng.score()
    want, S = _replay(hist, m)
    _compare(got, want, S, ticks, "observer, a plant of its own")
    wrong, _ = _replay(hist, m, x_key="xhat_hist")
    assert not np.allclose(got["jx"], wrong["jx"], rtol=1e-9, atol=0)  # (the estimate would have given another score)
    assert got["held"][5] == ticks and (got["held"][np.arange(batch) != 5] == 0).all()
    # a y_meas tick has no truth: the estimate is scored
    eng.reset_score()
    eng.solve()
    import torch
    ym = torch.zeros((batch, 3), dtype=torch.float64, device="cuda")
    out = eng.advance(y_meas=ym, u_out=True, age_out=True, xhat_out=True)
    one = dict(x_hist=out["xhat_out"].cpu().numpy()[None], u_hist=out["u_out"].cpu().numpy()[None], age_hist=out["age_out"].cpu().numpy()[None])
    want, S = _replay(one, m, tau0=ticks)
    _compare(eng.score(), want, S, 1, "observer, y_meas")


# ---- noise ----
def test_noise_on_and_no_history_at_all():
    """device-drawn noise; and the same rollout (same seed) without any history gives the same records bit for bit"""
    from test_noise_gpu import SEED, _wl
    batch, ticks = 33, 8
    wl = _wl(batch)
    m = _com_measure(batch=batch, seed=4)
    sw = np.array([2e-3] * 3 + [2e-2] * 3)
    eng, bare = _engine(wl), _engine(wl)
    for e in (eng, bare):
        e.set_noise(SEED, process=sw)
        _set(e, m)
    hist = _rollout(eng, ticks)
    bare.rollout(ticks)
    got = eng.score()
    want, S = _replay(hist, m)
    _compare(got, want, S, ticks, "noise, per-instance measure")
    assert got.tobytes() == bare.score().tobytes()
    assert bare.score_ptr != 0 and eng.score_ptr != bare.score_ptr


# ---- tracking: x_ref is the signal of the reference schedule ----
def test_tracking_after_a_seek():
    import tracking_cases as tc
    wl, signals = tc.tracking_workload()
    ticks = 8
    w_seq = tc.position_noise(ticks, tc.BATCH, tc.NX, 3, seed=21)
    sig = np.ascontiguousarray(signals[0])
    assert sig.ndim == 2 and sig.shape[1] == tc.NX and sig.shape[0] > 3 + ticks
    eng = _engine(wl)
    eng.set_reference_schedule(0, sig, tc.NX)
    eng.schedule_seek(3)
    m = dict(dense=False, per=False, tol=0.0, qx=np.array(tc.TRACK_W), x_ref=sig)
    eng.set_score(state_weights=m["qx"], state_ref=sig)
    hist = _rollout(eng, ticks, disturbances=w_seq)
    assert eng.schedule_tick() == 3 + ticks
    got = eng.score()
    want, S = _replay(hist, m, tau0=3)
    _compare(got, want, S, ticks, "tracking, seek(3)", nx=tc.NX, nu=wl["B"].shape[2])
    frozen, _ = _replay(hist, dict(m, x_ref=sig[3:4]), tau0=0)
    assert not np.allclose(got["jx"], frozen["jx"], rtol=1e-6, atol=0)  # (the row did move with tau)
    assert (got["ju"] == 0).all() and (got["viol_sum"] == 0).all()
    # beyond the end of the signal the last row is held
    short = np.ascontiguousarray(sig[:6])
    eng2 = _engine(wl)
    eng2.set_score(state_weights=m["qx"], state_ref=short)
    eng2.schedule_seek(3)
    h2 = _rollout(eng2, 6, disturbances=w_seq[:6])
    want2, S2 = _replay(h2, dict(m, x_ref=short), tau0=3)
    _compare(eng2.score(), want2, S2, 6, "a signal that ends", nx=tc.NX, nu=wl["B"].shape[2])


# ---- per-instance measures, dense weights, small batches ----
@pytest.mark.parametrize("batch", [5, 33])
@pytest.mark.parametrize("dense,per", [(True, True), (True, False), (False, True)])
def test_per_instance_and_dense_measures(batch, dense, per):
    from test_noise_gpu import _wl
    ticks = 7
    wl = _wl(batch, stuck=(2,))
    m = _com_measure(batch=batch if per else None, dense=dense, seed=batch, u_box=0.05)  # (a control box the loop exceeds)
    if per:
        m["x_ref"] = 0.1 * np.random.default_rng(1).standard_normal((batch, 4, 6))  # a signal per instance: rows 1 .. 3, then the last
    eng = _engine(wl)
    _set(eng, m)
    w_seq = 0.002 * np.random.default_rng(batch).standard_normal((ticks, batch, 6))
    hist = _rollout(eng, ticks, disturbances=w_seq)
    got = eng.score()
    want, S = _replay(hist, m)
    _compare(got, want, S, ticks, "batch %d dense %d per %d" % (batch, dense, per))
    assert got["held"][2] == ticks and got["ju"][2] == 0.0 and got["violating"].sum() > ticks


# ---- lifetime ----
def test_advance_is_rollout_and_the_lifetime():
    import torch
    wl, w_seq = _scenario("com")
    m = _com_measure()
    a, b, never = _engine(wl), _engine(wl), _engine(wl)
    for e in (a, b):
        _set(e, m)
    wd = torch.from_numpy(w_seq).cuda()
    a.rollout(2, disturbances=wd[:2])
    never.rollout(2, disturbances=wd[:2])  # (the handle that never scores goes through the same solves: what it has learnt is the same)
    for t in range(2):
        b.solve()
        b.advance(disturbance=wd[t])
    ra, rb = a.score(), b.score()
    assert ra.tobytes() == rb.tobytes() and (ra["ticks"] == 2).all()
    # a held instance's ju keeps its bits across ticks: G4 is held from tick 0 on, G1's members only later -- take their ju, run on
    before = a.score()
    a.rollout(3, disturbances=wd[2:5])
    never.rollout(3, disturbances=wd[2:5])
    after = a.score()
    held_now = (after["held"] - before["held"]) == 3
    assert held_now.any() and after["ju"][held_now].tobytes() == before["ju"][held_now].tobytes()
    assert (after["ju"][~held_now] != before["ju"][~held_now]).all()
    # set_x0 leaves the records, reset_score zeroes them
    a.set_x0(wl["x0"])
    assert a.score().tobytes() == after.tobytes()
    a.reset_score()
    assert a.score().tobytes() == score_ref.zero_records(BATCH).tobytes()
    a.rollout(1, disturbances=wd[:1])
    never.set_x0(wl["x0"])
    never.rollout(2, disturbances=wd[:2])
    assert (a.score()["ticks"] == 1).all() and (a.score()["first_violation"][[0, 33]] == 1).all()
    # a call while on replaces the measure and zeroes the records
    _set(a, dict(m, tol=1e9))
    assert a.score().tobytes() == score_ref.zero_records(BATCH).tobytes()
    a.rollout(1, disturbances=wd[:1])
    assert (a.score()["violating"] == 0).all() and a.score()["viol_max"].max() > 1.0
    # off: score() raises, and the tick is the tick of a handle that never scored
    a.set_score(None)
    assert a.score_ptr == 0
    from copra_amd import _capi
    for call in (a.score, a.score_summary, a.reset_score, never.score):
        with pytest.raises(_capi.CopraRuntimeError):
            call()
    a.set_x0(wl["x0"])
    never.set_x0(wl["x0"])
    ha = _numpy(a.rollout(4, disturbances=wd[:4], x_hist=True, u_hist=True, status_hist=True, age_hist=True))
    hn = _numpy(never.rollout(4, disturbances=wd[:4], x_hist=True, u_hist=True, status_hist=True, age_hist=True))
    for k in ("x_hist", "u_hist", "status_hist", "age_hist"):
        assert ha[k].tobytes() == hn[k].tobytes(), k


def test_errors():
    from copra_amd import BatchLMPC, _capi
    from test_noise_gpu import _wl
    wl = _wl(5)
    eng = _engine(wl)
    with pytest.raises(ValueError):
        eng.set_score(np.ones(6), tol=-1.0)
    with pytest.raises(ValueError):
        eng.set_score(np.ones(6), tol=float("nan"))
    with pytest.raises(ValueError):
        eng.set_score(np.array([1.0, np.nan, 1, 1, 1, 1]))
    with pytest.raises(ValueError):
        eng.set_score(np.ones(6), state_limits=(np.ones(6), np.zeros(6)))
    with pytest.raises(_capi.CopraDomainError):
        eng.set_score(np.ones(5))
    with pytest.raises(_capi.CopraRuntimeError):
        eng.score()  # (none of the refused calls turned scoring on)
    L = _capi.lib()
    s = _capi.Score()
    L.copra_score_init(ctypes.byref(s))
    ref = np.zeros(6)
    s.x_ref, s.ref_steps = ref.ctypes.data, 0
    assert L.copra_batch_set_score(eng._h, ctypes.byref(s)) == _capi.COPRA_ERR_ARG
    eng.set_score(np.ones(6), state_limits=(np.full(6, -np.inf), np.full(6, np.inf)))
    assert L.copra_batch_get_score(eng._h, None) == _capi.COPRA_ERR_ARG and L.copra_batch_score_summary(eng._h, None) == _capi.COPRA_ERR_ARG
    pb = __import__("fixtures").bounded_system("trajectory", N=12)
    ise = BatchLMPC(2, 1, 12, 4, pb["costs"], pb["cstrs"], initial_state=dict(R=1e-2 * np.eye(2), r=np.zeros(2)))
    with pytest.raises(_capi.CopraUnsupported):
        ise.set_score(np.ones(2))


# ---- the summary ----
@pytest.mark.parametrize("batch", [65, score_ref.CHUNK + 1, 2 * score_ref.CHUNK + 1])
def test_the_summary(batch):
    from test_noise_gpu import SEED, _wl
    wl = _wl(batch, stuck=(7, 40))
    m = _com_measure(batch=batch, seed=2)
    m["x_ref"][11] = np.nan  # a NaN reference: that instance is counted out of jx and in for ju
    eng = _engine(wl)
    eng.set_noise(SEED, process=np.array([2e-3] * 3 + [0.15] * 3))  # (velocities near their bound: some instances violate it)
    _set(eng, m)
    eng.rollout(4)
    rec = eng.score()
    s = eng.score_summary()
    assert np.isnan(rec["jx"][11]) and np.isfinite(np.delete(rec["jx"], 11)).all() and np.isfinite(rec["ju"]).all()
    assert s["jx"]["n"] == batch - 1 and s["ju"]["n"] == batch and s["peak"]["n"] == batch  # (peak ignores a NaN tick: `>`)
    worst = check_summary(s, rec, merge_depth(batch))
    print("batch %d: largest error / bound of mean and m2 against longdouble %.3g" % (batch, worst))
    assert s["instances_held"] >= 2 and s["held"] >= 8 and 0 < s["instances_violating"] < batch
    want = score_ref.summary(rec)  # the written order, on the host: the device may contract, so within twice the bound, not bit for bit
    from test_score_abi import summary_bounds
    for f in score_ref.FIELDS:
        E, B = summary_bounds(rec[f], merge_depth(batch))
        assert abs(s[f]["mean"] - want[f]["mean"]) <= 2 * E and abs(s[f]["m2"] - want[f]["m2"]) <= 2 * B, f
        assert all(s[f][k] == want[f][k] for k in ("n", "min", "max", "argmin", "argmax")), f
    again = eng.score_summary()
    for f in score_ref.FIELDS:
        assert all(np.float64(s[f][k]).tobytes() == np.float64(again[f][k]).tobytes() for k in ("mean", "m2", "min", "max")), f
        assert all(s[f][k] == again[f][k] for k in ("n", "argmin", "argmax")), f
    assert all(s[k] == again[k] for k in score_ref.TOTALS)


# ---- a C caller ----
def test_c_caller_scores_a_rollout(tmp_path):
    """tests/cpp/test_score.cpp against include/copra_hip.h, as a fresh child process"""
    from copra_amd import _capi
    exe = str(tmp_path / "test_score")
    csrc = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_score.cpp"),
                           "-o", exe, "-L", csrc, "-lcopra_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- misaligned arrays used in place ----
def test_misaligned_device_arrays_give_the_same_records():
    import torch
    from test_noise_gpu import _wl
    batch, ticks = 33, 7
    wl = _wl(batch)
    w_seq = torch.from_numpy(0.002 * np.random.default_rng(3).standard_normal((ticks, batch, 6))).cuda()
    for per in (False, True):
        m = _com_measure(batch=batch if per else None, seed=6)
        host = [m["qx"], m["ru"], m["x_ref"], m["x_lo"], m["x_hi"], m["u_lo"], m["u_hi"]]
        records = []
        for shift in (0, 1):
            tens = []
            for a in host:
                room = torch.zeros(a.size + 2, dtype=torch.float64, device="cuda")
                view = room[shift:shift + a.size].view(a.shape)
                view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
                assert view.data_ptr() % 16 == 8 * shift and view.is_contiguous()
                tens.append(view)
            eng = _engine(wl)
            eng.set_score(tens[0], tens[1], tens[2], (tens[3], tens[4]), (tens[5], tens[6]), tol=1e-9)
            hist = _rollout(eng, ticks, disturbances=w_seq)
            records.append(eng.score())
            if shift == 0:
                want, S = _replay(hist, m)
                _compare(records[0], want, S, ticks, "tensors in place, per %d" % per)
        assert records[0].tobytes() == records[1].tobytes(), per
