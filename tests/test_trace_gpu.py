"""Ensemble traces on the device (copra_batch_set_trace, ABI 17; BatchLMPC.set_trace / trace / trace_info): every case makes one rollout that
also writes x_hist, u_hist, age_hist (and xhat_hist where it applies) and compares the trace with the reduction of those histories -- n, min,
max, argmin, argmax and every head count exactly, mean and m2 against numpy's longdouble within summary_bounds(values, merge_depth(batch)) of
tests/test_score_abi.py, which are derived there for this very merge.  The rows' values themselves (a state, a control, ONE subtraction for
the estimation error, the score's violation rule) are formed from the histories by tests/trace_ref.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import score_ref
import trace_ref
from test_backup_plan_gpu import BATCH, G1, G2, G3, G4, K, TICKS, _scenario
from test_closed_loop_gpu import _engine
from test_score_abi import merge_depth, summary_bounds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELD, FALLBACK = score_ref.HELD, score_ref.FALLBACK
CHUNK = score_ref.CHUNK
VEL = dict(state_limits=(np.array([-np.inf] * 3 + [-0.6] * 3), np.array([np.inf] * 3 + [0.6] * 3)))  # the velocity bound of the workload


def _numpy(hist):
    return {k: v.cpu().numpy() for k, v in hist.items() if v is not None}


def _kicks(batch):
    """the kick scenario of tests/test_backup_plan_gpu.py at any batch: instance i gets the disturbances and the start of the scenario's i % 64"""
    from copra_amd import workloads
    _, w64 = _scenario("com")
    wl = workloads.com_preview(batch)
    wl = dict(wl, x0=wl["x0"].copy())
    src = np.arange(batch) % BATCH
    wl["x0"][np.isin(src, G4), 3] = 50.0
    return wl, np.ascontiguousarray(w64[:, src])


def _limits(kw):
    xl, xh = kw.get("state_limits") or (None, None)
    ul, uh = kw.get("control_limits") or (None, None)
    return {k: v for k, v in dict(x_lo=xl, x_hi=xh, u_lo=ul, u_hi=uh).items() if v is not None}


def _check(eng, hist, ticks, what, tau0=0, x_key="x_hist", est_key=None, first_tick=0, **kw):
    """the recorded slots against the histories: history row t belongs to the slot whose head says tick first_tick + k for the k-th entry of
    `ticks`.  Returns the largest error / bound of mean and m2"""
    slots, batch = eng.trace_slots(), eng.batch
    assert len(slots) == len(ticks)
    lim, tol = _limits(kw), kw.get("tol", 0.0)
    off = 1 if x_key == "x_hist" else 0  # (x_hist[0] is the state before the first tick)
    worst = 0.0
    for k, t in enumerate(ticks):
        x, u, age = hist[x_key][t + off], hist["u_hist"][t], hist["age_hist"][t]
        est = hist[est_key][t] if est_key else None
        with np.errstate(invalid="ignore"):
            vals = trace_ref.values(what, x, u, age, est, **lim)
        head, stat = slots["head"][k], slots["stat"][k]
        assert stat.shape[0] == vals.shape[0]
        want = trace_ref.counts(age, vals[-1] if lim else None, tol)
        assert (head["tick"], head["tau"], head["reserved"]) == (first_tick + t, tau0 + t + 1, 0), (k, head)
        assert all(head[c] == want[c] for c in trace_ref.COUNTS), (k, head, want)
        assert head["solved"] + head["replayed"] + head["fallback"] + head["held"] == batch
        for r in range(vals.shape[0]):
            worst = max(worst, trace_ref.check_stat(stat[r], vals[r], lambda v: summary_bounds(v, merge_depth(batch)), (k, r)))
    return worst


def _rollout(eng, ticks, **kw):
    return _numpy(eng.rollout(ticks, x_hist=True, u_hist=True, age_hist=True, **kw))


def _join(a, b):
    return dict(x_hist=np.concatenate([a["x_hist"], b["x_hist"][1:]]), u_hist=np.concatenate([a["u_hist"], b["u_hist"]]), age_hist=np.concatenate([a["age_hist"], b["age_hist"]]))


# ---- 1: the kick scenario, every age, at the batches where the reduction changes ----
@pytest.mark.parametrize("batch", [1, 65, 257, CHUNK + 1, 2 * CHUNK + 1])
def test_the_kick_scenario(batch):
    """backup plans of K steps; five ticks without a fallback control (a failed instance without a plan is HELD), five with one (FALLBACK): fresh,
    replayed, fallback and held ticks all occur, and a held instance has no u rows"""
    import torch
    wl, w_seq = _kicks(batch)
    eng = _engine(wl)
    eng.set_backup_steps(K)
    lim = dict(VEL, control_limits=(np.full(3, -2.0), np.full(3, 2.0)), tol=1e-9)
    eng.set_trace(TICKS, **lim)
    wd = torch.from_numpy(w_seq).cuda()
    first = _rollout(eng, 5, disturbances=wd[:5])
    hist = _join(first, _rollout(eng, 5, disturbances=wd[5:], fallback_control=np.zeros((batch, 3))))
    ages = hist["age_hist"]
    if batch >= BATCH:
        assert all((ages == a).any() for a in (0, 1, 2, 3, FALLBACK, HELD))
    assert np.isnan(hist["u_hist"][ages == HELD]).all()
    worst = _check(eng, hist, range(TICKS), 3, **lim)
    print("kicks, batch %d: largest error / bound of mean and m2 %.3g" % (batch, worst))
    info = eng.trace_info()
    assert info == dict(recorded=TICKS, missed=0, rows=10, slot_bytes=64 + 56 * 10)
    tr = eng.trace()
    assert tr["x"].shape == (TICKS, 6) and tr["u"].shape == (TICKS, 3) and tr["viol"].shape == (TICKS,) and "err" not in tr
    held = (ages == HELD).sum(axis=1)
    assert np.array_equal(tr["head"]["held"], held) and np.array_equal(tr["u"]["n"], np.tile((batch - held)[:, None], (1, 3)))
    assert np.array_equal(tr["x"]["n"], np.full((TICKS, 6), batch))
    before = eng.trace_slots().tobytes()
    eng.rollout(1, disturbances=wd[:1])  # the trace is full: the tick runs, nothing is recorded
    assert eng.trace_info()["recorded"] == TICKS and eng.trace_info()["missed"] == 1 and eng.trace_slots().tobytes() == before


# ---- 2: more chunks than stage 2 has threads ----
def test_more_chunks_than_threads():
    """256 x 1024 + 1 instances of the (2, 1) system of tests/test_noise_gpu.py, 2 ticks: thread 0 of stage 2 folds partials 0 and 256"""
    from test_noise_gpu import _small
    batch = 256 * CHUNK + 1
    wl = _small(2, 1, batch, N=2)
    eng = _engine(wl)
    eng.set_trace(2)
    hist = _rollout(eng, 2)
    worst = _check(eng, hist, range(2), 3)
    tr = eng.trace()
    assert (tr["x"]["n"] == batch).all() and (tr["head"]["solved"] > 256 * CHUNK // 2).all()
    print("batch %d: largest error / bound of mean and m2 %.3g" % (batch, worst))


# ---- 3: the observer ----
def test_the_observer_simulating_a_plant_and_a_measured_tick():
    import torch
    from test_noise_gpu import SEED, _observer, _wl
    batch, ticks = 33, 6
    wl = _wl(batch, stuck=(5,))
    eng = _engine(wl)
    _observer(eng, 6)
    xhat0 = wl["x0"].copy()
    xhat0[:, 3:] += 0.05
    xhat0[5] = wl["x0"][5]
    eng.set_x0(xhat0)
    eng.set_noise(SEED, sensor=np.array([1e-3, 2e-3, 3e-3]))
    eng.set_trace(ticks + 1, estimate_error=True, **VEL)
    hist = _rollout(eng, ticks, plant=(wl["A"], 0.9 * wl["B"], wl["d"]), xhat_hist=True)
    worst = _check(eng, hist, range(ticks), 7, est_key="xhat_hist", **VEL)  # x rows: the plant's state; err rows: xhat_hist - xp
    print("observer: largest error / bound of mean and m2 %.3g" % worst)
    tr = eng.trace()
    assert (tr["err"]["n"] == batch).all() and (tr["err"]["m2"] > 0).all()
    est_mean = hist["xhat_hist"][:, :, 3].mean(axis=1)
    assert not np.allclose(tr["x"]["mean"][:, 3], est_mean, rtol=1e-9, atol=0)  # (the estimate would have given other x rows)
    # a y_meas tick has no truth: the x rows read the estimate, the err rows are empty
    eng.solve()
    out = eng.advance(y_meas=torch.zeros((batch, 3), dtype=torch.float64, device="cuda"), u_out=True, age_out=True, xhat_out=True)
    one = dict(xhat=out["xhat_out"].cpu().numpy()[None], u_hist=out["u_out"].cpu().numpy()[None], age_hist=out["age_out"].cpu().numpy()[None])
    slot = eng.trace_slots()[ticks]
    with np.errstate(invalid="ignore"):
        vals = trace_ref.values(7, one["xhat"][0], one["u_hist"][0], one["age_hist"][0], None, x_lo=VEL["state_limits"][0], x_hi=VEL["state_limits"][1])
    for r in range(16):
        trace_ref.check_stat(slot["stat"][r], vals[r], lambda v: summary_bounds(v, merge_depth(batch)), r)
    assert (slot["stat"]["n"][9:15] == 0).all() and (slot["stat"]["argmin"][9:15] == -1).all() and slot["head"]["tick"] == ticks


# ---- 4: input delay ----
def test_input_delay_reads_the_state_at_the_current_tick():
    from test_noise_gpu import _wl
    batch, ticks = 33, 6
    wl = _wl(batch, stuck=(5,))
    eng = _engine(wl)
    eng.set_input_delay(2, 0.05 * np.random.default_rng(1).standard_normal((batch, 3)))
    eng.set_trace(ticks)
    w_seq = 0.002 * np.random.default_rng(2).standard_normal((ticks, batch, 6))
    hist = _rollout(eng, ticks, disturbances=w_seq)
    assert not np.array_equal(hist["x_hist"][-1], eng.state())  # (x0 is the prediction; x_hist is xnow)
    assert np.array_equal(hist["x_hist"][-1], eng.delay_state())
    worst = _check(eng, hist, range(ticks), 3)
    print("delay 2: largest error / bound of mean and m2 %.3g" % worst)


# ---- 5: limits the kicks violate at known ticks, tol on both sides of one violation ----
def test_violations_at_known_ticks_and_tol_on_both_sides():
    wl, w_seq = _scenario("com")
    kicked = sorted(G1 + G2 + G3)

    def run(tol):
        eng = _engine(wl)
        eng.set_backup_steps(K)
        eng.set_trace(TICKS, control=False, tol=tol, **VEL)
        hist = _rollout(eng, TICKS, disturbances=w_seq)
        _check(eng, hist, range(TICKS), 1, tol=tol, **VEL)
        return eng.trace(), hist

    tr, hist = run(1e-9)
    # G4 starts at a velocity of 50 and is held; the kick of tick 1 shows in the state after tick 1
    assert tr["head"]["violating"][0] == len(G4) and tr["head"]["violating"][1] == len(G4) + len(kicked)
    assert tr["viol"]["max"][1] > 40.0 and tr["viol"]["argmax"][1] in kicked + list(G4)
    vm = trace_ref.vmax(hist["x_hist"][2], hist["u_hist"][1], hist["age_hist"][1], x_lo=VEL["state_limits"][0], x_hi=VEL["state_limits"][1])
    top = float(vm.max())
    assert top == tr["viol"]["max"][1]
    at, below = run(top)[0], run(np.nextafter(top, 0.0))[0]
    assert at["head"]["violating"][1] == int((vm > top).sum()) == 0  # `>`: a violation equal to tol does not count
    assert below["head"]["violating"][1] == int((vm > np.nextafter(top, 0.0)).sum()) >= 1
    assert at["viol"].tobytes() == below["viol"].tobytes() == tr["viol"].tobytes()  # (tol moves the count, never the row)


# ---- 6, 8: scores on or off, the caller's u_out / age_out or the library's: the same bytes; and twice the same run ----
def test_scores_and_the_callers_buffers_change_no_byte():
    wl, w_seq = _scenario("com")
    got = []
    for score, outs in ((False, False), (True, False), (False, True), (True, True), (False, False)):
        eng = _engine(wl)
        eng.set_backup_steps(K)
        if score:
            eng.set_score(np.ones(6), 1e-3 * np.ones(3), state_limits=VEL["state_limits"])
        eng.set_trace(TICKS, control_limits=(np.full(3, -2.0), np.full(3, 2.0)), **VEL)
        eng.rollout(TICKS, disturbances=w_seq, u_hist=outs or None, age_hist=outs or None)
        got.append(eng.trace_slots().tobytes())
        assert eng.trace_ptr != 0
    assert all(g == got[0] for g in got[1:])


# ---- 7: the lifetime ----
def test_advance_is_rollout_and_the_lifetime():
    import torch
    from copra_amd import _capi
    wl, w_seq = _scenario("com")
    wd = torch.from_numpy(w_seq).cuda()
    a, b, c, never = _engine(wl), _engine(wl), _engine(wl), _engine(wl)
    for e in (a, b, c, never):
        e.set_backup_steps(K)
    a.set_trace(6, **VEL)
    b.set_trace(6, **VEL)
    c.set_trace(6, every=2, **VEL)
    a.rollout(6, disturbances=wd[:6])
    c.rollout(6, disturbances=wd[:6])
    never.rollout(6, disturbances=wd[:6])
    for t in range(6):
        b.solve()
        b.advance(disturbance=wd[t])
        if t == 2:
            b.reset_trace()  # in the middle: the trace's tick goes back to 0, the schedule tick does not
    sa, sb, sc = a.trace_slots(), b.trace_slots(), c.trace_slots()
    assert sc.tobytes() == sa[[0, 2, 4]].tobytes() and c.trace_info()["recorded"] == 3 and c.trace_info()["missed"] == 0
    assert len(sb) == 3 and sb["stat"].tobytes() == sa["stat"][3:].tobytes()
    assert sb["head"]["tick"].tolist() == [0, 1, 2] and sb["head"]["tau"].tolist() == [4, 5, 6]
    for k in trace_ref.COUNTS:
        assert np.array_equal(sb["head"][k], sa["head"][k][3:]), k
    # a call while on replaces the trace and restarts it
    a.set_trace(4, state=False)
    assert a.trace_info() == dict(recorded=0, missed=0, rows=3, slot_bytes=64 + 56 * 3)
    a.rollout(1, disturbances=wd[6:7])
    never.rollout(1, disturbances=wd[6:7])
    one = a.trace()
    assert list(one) == ["head", "u"] and one["head"]["tick"].tolist() == [0] and one["head"]["tau"].tolist() == [7]
    # off: the getters raise, and the tick is the tick of a handle that never traced
    a.set_trace(None)
    assert a.trace_ptr == 0
    for call in (a.trace_info, a.trace, a.reset_trace, never.trace_info):
        with pytest.raises(_capi.CopraRuntimeError):
            call()
    ha = _numpy(a.rollout(3, disturbances=wd[7:10], x_hist=True, u_hist=True, status_hist=True, age_hist=True))
    hn = _numpy(never.rollout(3, disturbances=wd[7:10], x_hist=True, u_hist=True, status_hist=True, age_hist=True))
    for k in ("x_hist", "u_hist", "status_hist", "age_hist"):
        assert ha[k].tobytes() == hn[k].tobytes(), k


# ---- 9: limits used in place, 8 bytes off a 16-byte boundary ----
def test_misaligned_device_limits_give_the_bytes_of_the_aligned_run():
    import torch
    wl, w_seq = _scenario("com")
    host = [VEL["state_limits"][0], VEL["state_limits"][1], np.full(3, -2.0), np.full(3, 2.0)]
    got = []
    for shift in (0, 1, None):
        tens = []
        for arr in host:
            room = torch.zeros(arr.size + 2, dtype=torch.float64, device="cuda")
            view = room[shift or 0:(shift or 0) + arr.size]
            view.copy_(torch.from_numpy(arr))
            assert view.data_ptr() % 16 == 8 * (shift or 0)
            tens.append(view if shift is not None else arr)
        eng = _engine(wl)
        eng.set_backup_steps(K)
        eng.set_trace(4, state_limits=(tens[0], tens[1]), control_limits=(tens[2], tens[3]), tol=1e-9)
        eng.rollout(4, disturbances=w_seq[:4])
        got.append(eng.trace_slots().tobytes())
    assert got[0] == got[1] == got[2]  # (aligned tensors, misaligned tensors, host copies)


# ---- 10: the error table ----
def test_errors():
    from copra_amd import BatchLMPC, _capi
    from test_noise_gpu import _wl
    eng = _engine(_wl(5))
    for bad in (dict(capacity=0), dict(capacity=4, state=False, control=False), dict(capacity=4, every=-1), dict(capacity=4, tol=-1.0),
                dict(capacity=4, tol=float("nan")), dict(capacity=4, state_limits=(np.ones(6), np.zeros(6))),
                dict(capacity=4, control_limits=(np.array([0.0, np.nan, 0.0]), None))):
        with pytest.raises(ValueError):
            eng.set_trace(**bad)
    with pytest.raises(_capi.CopraDomainError):
        eng.set_trace(4, state_limits=(np.zeros(5), None))
    for call in (eng.trace_info, eng.trace, eng.reset_trace):  # (none of the refused calls turned tracing on)
        with pytest.raises(_capi.CopraRuntimeError):
            call()
    assert eng.trace_ptr == 0
    L = _capi.lib()
    room = np.zeros(1024)
    assert L.copra_batch_get_trace(eng._h, 0, 0, room.ctypes.data) == _capi.COPRA_ERR_RUNTIME
    eng.set_trace(3, state_limits=(np.full(6, -np.inf), np.full(6, np.inf)))
    eng.rollout(2)
    assert L.copra_batch_get_trace(eng._h, 0, 2, None) == _capi.COPRA_ERR_ARG
    for first, count in ((0, 3), (1, 2), (-1, 1), (0, -1), (3, 0)):
        assert L.copra_batch_get_trace(eng._h, first, count, room.ctypes.data) == _capi.COPRA_ERR_ARG, (first, count)
    assert L.copra_batch_get_trace(eng._h, 2, 0, room.ctypes.data) == _capi.COPRA_OK and L.copra_batch_get_trace(eng._h, 1, 1, room.ctypes.data) == _capi.COPRA_OK
    t = _capi.Trace()
    L.copra_trace_init(ctypes.byref(t))
    t.capacity, t.what = 2, 8
    assert L.copra_batch_set_trace(eng._h, ctypes.byref(t)) == _capi.COPRA_ERR_ARG  # an unknown bit
    pb = __import__("fixtures").bounded_system("trajectory", N=12)
    ise = BatchLMPC(2, 1, 12, 4, pb["costs"], pb["cstrs"], initial_state=dict(R=1e-2 * np.eye(2), r=np.zeros(2)))
    with pytest.raises(_capi.CopraUnsupported):
        ise.set_trace(4)
    ise.set_trace(None)  # (nothing to end is no error)


# ---- 11: a C caller ----
def test_c_caller_traces_a_rollout(tmp_path):
    """tests/cpp/test_trace.cpp against include/copra_hip.h, as a fresh child process"""
    from copra_amd import _capi
    exe = str(tmp_path / "test_trace")
    csrc = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_trace.cpp"),
                           "-o", exe, "-L", csrc, "-lcopra_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- shards: two handles over halves of the batch ----
def test_merge_traces_of_two_handles():
    from copra_amd import sharding
    batch, cut = 2 * BATCH, BATCH
    wl, w_seq = _kicks(batch)
    part = lambda lo, hi: dict(wl, **{k: wl[k][lo:hi] for k in ("A", "B", "d", "x0")})  # noqa: E731
    traces, hists = [], []
    for lo, hi in ((0, cut), (cut, batch)):
        eng = _engine(part(lo, hi))
        eng.set_backup_steps(K)
        eng.set_trace(4, **VEL)
        hists.append(_rollout(eng, 4, disturbances=np.ascontiguousarray(w_seq[:4, lo:hi])))
        traces.append(eng.trace())
    merged = sharding.merge_traces(traces, [0, cut])
    both = {k: np.concatenate([h[k] for h in hists], axis=1) for k in ("x_hist", "u_hist", "age_hist")}
    worst = 0.0
    for t in range(4):
        with np.errstate(invalid="ignore"):
            vals = trace_ref.values(3, both["x_hist"][t + 1], both["u_hist"][t], both["age_hist"][t], None, x_lo=VEL["state_limits"][0], x_hi=VEL["state_limits"][1])
        flat = np.concatenate([merged[g][t].reshape(-1) for g in ("x", "u", "viol")])
        for r in range(10):
            worst = max(worst, trace_ref.check_stat(flat[r], vals[r], lambda v: summary_bounds(v, merge_depth(cut, 1)), (t, r)))
        want = trace_ref.counts(both["age_hist"][t], vals[-1], 0.0)
        assert all(merged["head"][t][c] == want[c] for c in trace_ref.COUNTS) and merged["head"][t]["tick"] == t and merged["head"][t]["tau"] == t + 1
    assert (merged["x"]["argmax"] >= cut).any() and (merged["x"]["argmax"] < cut).any()
    print("two handles merged: largest error / bound %.3g" % worst)
