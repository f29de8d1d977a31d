"""Trace quantiles on the device (copra_batch_set_trace_quantiles, ABI 18; BatchLMPC.set_trace_quantiles / trace_quantiles): every case makes
a rollout that also writes x_hist, u_hist, age_hist (and xhat_hist where it applies) and compares trace_quantiles() BYTE FOR BYTE with
tests/trace_quant_ref.py -- a stable sort by the key and the rank rule -- on the values tests/trace_ref.py forms from those histories.  An
order statistic is an element of the data: there is no bound."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import score_ref
import trace_quant_ref
import trace_ref
from test_backup_plan_gpu import BATCH, K, TICKS, _scenario
from test_closed_loop_gpu import _engine
from test_trace_gpu import VEL, _join, _kicks, _limits, _rollout

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELD = score_ref.HELD
CHUNK = score_ref.CHUNK
BAND = (0.0, 0.05, 0.5, 0.95, 1.0)
EIGHT = [0.0, 1.0, 0.5, 1.0 / 3.0, 1e-9, 0.999, 0.5, 0.05]
NAN = 0x7FF8000000000000
GROUPS = (("x", 1), ("u", 2), ("err", 4))


def _want(hist, ticks, what, levels, x_key="x_hist", est_key=None, **kw):
    """(len(ticks), rows, nq): the rule on history rows `ticks`"""
    lim = _limits(kw)
    off = 1 if x_key == "x_hist" else 0  # (x_hist[0] is the state before the first tick)
    out = []
    for t in ticks:
        with np.errstate(invalid="ignore"):
            vals = trace_ref.values(what, hist[x_key][t + off], hist["u_hist"][t], hist["age_hist"][t], hist[est_key][t] if est_key else None, **lim)
        out.append(trace_quant_ref.rows(vals, levels))
    return np.stack(out)


def _flat(tq, what, limits):
    """trace_quantiles() back in the slot's row order: (ticks, rows, nq)"""
    parts = [tq[name] for name, bit in GROUPS if what & bit] + ([tq["viol"][:, None, :]] if limits else [])
    assert set(tq) == {"levels"} | {name for name, bit in GROUPS if what & bit} | ({"viol"} if limits else set())
    return np.concatenate(parts, axis=1)


def _check(eng, hist, ticks, what, levels, **kw):
    tq = eng.trace_quantiles()
    assert tq["levels"].tobytes() == np.asarray(levels, dtype=np.float64).tobytes()
    got, want = _flat(tq, what, bool(_limits(kw))), _want(hist, ticks, what, levels, **kw)
    assert got.dtype == np.float64 and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        at = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        raise AssertionError("%d of %d quantiles differ; the first at (tick, row, level) %s: %r against %r" % (len(at), got.size, at[0], got[tuple(at[0])], want[tuple(at[0])]))
    return got


# ---- 1: the kick scenario, every age, at the batches where a thread's loop changes ----
@pytest.mark.parametrize("batch", [1, 65, 257, CHUNK + 1, 2 * CHUNK + 1])
def test_the_kick_scenario(batch):
    """backup plans of K steps; five ticks without a fallback control (a failed instance without a plan is HELD), five with one: every age
    occurs, and a held instance has no u rows.  The slots are byte for byte those of the same run without quantiles"""
    import torch
    wl, w_seq = _kicks(batch)
    lim = dict(VEL, control_limits=(np.full(3, -2.0), np.full(3, 2.0)), tol=1e-9)
    wd = torch.from_numpy(w_seq).cuda()
    slots = []
    for quantiles in (True, False):
        eng = _engine(wl)
        eng.set_backup_steps(K)
        eng.set_trace(TICKS, **lim)
        if quantiles:
            eng.set_trace_quantiles(BAND)
        first = _rollout(eng, 5, disturbances=wd[:5])
        hist = _join(first, _rollout(eng, 5, disturbances=wd[5:], fallback_control=np.zeros((batch, 3))))
        slots.append(eng.trace_slots())
        if not quantiles:
            assert eng.trace_quantiles_ptr == 0
            continue
        ages = hist["age_hist"]
        if batch >= BATCH:
            assert (ages == HELD).any() and (ages == 0).any() and (ages > 0).any()
        got = _check(eng, hist, range(TICKS), 3, BAND, **lim)
        tr = eng.trace()
        for name, at in (("x", slice(0, 6)), ("u", slice(6, 9))):
            some = tr[name]["n"] > 0
            assert np.array_equal(got[:, at, 0][some], tr[name]["min"][some]) and np.array_equal(got[:, at, -1][some], tr[name]["max"][some])
            assert (got[:, at][~some].view(np.uint64) == NAN).all()
        assert np.array_equal(got[:, 9, -1], tr["viol"]["max"])
        before = eng.trace_quantiles()
        eng.rollout(1, disturbances=wd[:1])  # the trace is full: the tick runs, nothing is recorded
        assert eng.trace_info()["missed"] == 1 and all(eng.trace_quantiles()[k].tobytes() == before[k].tobytes() for k in before)
    assert slots[0].tobytes() == slots[1].tobytes()


# ---- 2: a thread's loop of 65 rounds ----
def test_a_quarter_of_a_million_instances():
    """256 x 1024 + 1 instances of the (2, 1) system of tests/test_noise_gpu.py, 2 ticks, eight levels"""
    from test_noise_gpu import _small
    batch = 256 * CHUNK + 1
    eng = _engine(_small(2, 1, batch, N=2))
    eng.set_trace(2)
    eng.set_trace_quantiles(EIGHT)
    hist = _rollout(eng, 2)
    got = _check(eng, hist, range(2), 3, EIGHT)
    assert np.isfinite(got).all() and (got[:, :, 0] < got[:, :, 1]).all()


# ---- 3: every row one value `batch` times ----
def test_identical_instances():
    wl, _ = _scenario("com")
    batch = 300
    one = {k: np.ascontiguousarray(np.repeat(wl[k][:1], batch, axis=0)) for k in ("A", "B", "d", "x0")}
    eng = _engine(dict(wl, **one))
    eng.set_trace(3, **VEL)
    eng.set_trace_quantiles(EIGHT)
    hist = _rollout(eng, 3)
    got = _check(eng, hist, range(3), 3, EIGHT, **VEL)
    assert np.ptp(hist["x_hist"], axis=1).max() < 1e-9 and np.ptp(got[:, :6], axis=2).max() < 1e-9  # (the top digits of every key agree)


# ---- 4: the observer ----
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
    eng.set_trace_quantiles(BAND)
    hist = _rollout(eng, ticks, plant=(wl["A"], 0.9 * wl["B"], wl["d"]), xhat_hist=True)
    # x rows: the plant's state; err rows: xhat_hist - xp, live
    want = _want(hist, range(ticks), 7, BAND, est_key="xhat_hist", **VEL)
    assert np.isfinite(want[:, 9:15]).all()
    # a y_meas tick has no truth: the x rows read the estimate, the err rows are empty
    eng.solve()
    out = eng.advance(y_meas=torch.zeros((batch, 3), dtype=torch.float64, device="cuda"), u_out=True, age_out=True, xhat_out=True)
    one = dict(xhat=out["xhat_out"].cpu().numpy()[None], u_hist=out["u_out"].cpu().numpy()[None], age_hist=out["age_out"].cpu().numpy()[None])
    last = _want(one, [0], 7, BAND, x_key="xhat", **VEL)
    got = _flat(eng.trace_quantiles(), 7, True)
    assert got.shape == (ticks + 1, 16, 5)
    assert got[:ticks].tobytes() == want.tobytes() and got[ticks:].tobytes() == last.tobytes()
    assert (got[ticks, 9:15].view(np.uint64) == NAN).all()


# ---- 5: every and a full trace ----
def test_every_three_with_room_for_two():
    wl, w_seq = _scenario("com")
    eng = _engine(wl)
    eng.set_backup_steps(K)
    eng.set_trace(2, every=3)
    eng.set_trace_quantiles(BAND)
    hist = _rollout(eng, 4, disturbances=w_seq[:4])  # ticks 0 and 3 are recorded: the trace is full
    after4 = eng.trace_quantiles()
    rest = _rollout(eng, 6, disturbances=w_seq[4:10])
    assert eng.trace_info() == dict(recorded=2, missed=2, rows=9, slot_bytes=64 + 56 * 9)  # (ticks 6 and 9 were recordable)
    _check(eng, _join(hist, rest), [0, 3], 3, BAND)
    now = eng.trace_quantiles()
    assert all(now[k].tobytes() == after4[k].tobytes() for k in now)  # the later ticks changed nothing


# ---- 6, 7, 8: the lifetime ----
def test_advance_is_rollout_and_the_lifetime():
    import torch
    from copra_amd import _capi
    wl, w_seq = _scenario("com")
    wd = torch.from_numpy(w_seq).cuda()
    a, b = _engine(wl), _engine(wl)
    for e in (a, b):
        e.set_backup_steps(K)
        e.set_trace(6, **VEL)
        e.set_trace_quantiles(BAND)
    ha = _rollout(a, 6, disturbances=wd[:6])
    for t in range(6):
        b.solve()
        b.advance(disturbance=wd[t])
    qa, qb = a.trace_quantiles(), b.trace_quantiles()
    assert list(qa) == ["levels", "x", "u", "viol"] and all(qa[k].tobytes() == qb[k].tobytes() for k in qa)
    assert qa["x"].shape == (6, 6, 5) and qa["u"].shape == (6, 3, 5) and qa["viol"].shape == (6, 5)
    _check(a, ha, range(6), 3, BAND, **VEL)
    # reset_trace keeps the levels and the next recorded tick rewrites slot 0
    ptr = a.trace_quantiles_ptr
    a.reset_trace()
    assert a.trace_quantiles_ptr == ptr != 0 and a.trace_quantiles()["x"].shape == (0, 6, 5)
    h2 = _rollout(a, 1, disturbances=wd[6:7])
    got = _check(a, h2, [0], 3, BAND, **VEL)
    assert got.tobytes() != _flat(qa, 3, True)[:1].tobytes()
    # the setter restarts the trace, so every recorded slot has its quantiles; other levels, another count
    a.set_trace_quantiles([0.25])
    assert a.trace_info()["recorded"] == 0 and a.trace_quantiles()["levels"].tolist() == [0.25]
    h3 = _rollout(a, 2, disturbances=wd[7:9])
    _check(a, h3, range(2), 3, [0.25], **VEL)
    # None ends quantiles and keeps the trace and its slots
    slots = a.trace_slots().tobytes()
    a.set_trace_quantiles(None)
    assert a.trace_quantiles_ptr == 0 and a.trace_ptr != 0 and a.trace_slots().tobytes() == slots
    with pytest.raises(_capi.CopraRuntimeError):
        a.trace_quantiles()
    a.rollout(1, disturbances=wd[9:10])
    assert a.trace_info()["recorded"] == 3
    # set_trace, replacing the trace or ending it, ends quantiles
    b.set_trace(4, **VEL)
    assert b.trace_quantiles_ptr == 0
    with pytest.raises(_capi.CopraRuntimeError):
        b.trace_quantiles()
    b.set_trace_quantiles([])
    b.set_trace_quantiles(BAND)
    assert b.trace_quantiles_ptr != 0
    b.set_trace(None)
    assert b.trace_quantiles_ptr == 0 and b.trace_ptr == 0


# ---- 9: the error table ----
def test_errors():
    from copra_amd import _capi
    from test_noise_gpu import _wl
    eng = _engine(_wl(5))
    L = _capi.lib()
    room = np.zeros(1024)
    with pytest.raises(_capi.CopraRuntimeError):  # tracing off
        eng.set_trace_quantiles(BAND)
    assert L.copra_batch_get_trace_quantiles(eng._h, 0, 0, room.ctypes.data) == _capi.COPRA_ERR_RUNTIME
    assert L.copra_batch_trace_quantile_info(eng._h, None, None) == _capi.COPRA_ERR_RUNTIME and eng.trace_quantiles_ptr == 0
    eng.set_trace(3)
    with pytest.raises(_capi.CopraRuntimeError):  # quantiles off
        eng.trace_quantiles()
    assert L.copra_batch_get_trace_quantiles(eng._h, 0, 0, room.ctypes.data) == _capi.COPRA_ERR_RUNTIME
    for bad in ([0.5] * 9, [np.nan], [-1e-9], [1.0 + 1e-9], [0.5, np.inf]):
        with pytest.raises(ValueError):
            eng.set_trace_quantiles(bad)
        assert eng.trace_quantiles_ptr == 0
    lv = np.array([0.5, 0.9])
    as_ptr = lv.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.copra_batch_set_trace_quantiles(eng._h, as_ptr, -1) == _capi.COPRA_ERR_ARG
    eng.set_trace_quantiles(lv)
    eng.rollout(2)
    assert L.copra_batch_get_trace_quantiles(eng._h, 0, 2, None) == _capi.COPRA_ERR_ARG
    for first, count in ((0, 3), (1, 2), (-1, 1), (0, -1), (3, 0)):
        assert L.copra_batch_get_trace_quantiles(eng._h, first, count, room.ctypes.data) == _capi.COPRA_ERR_ARG, (first, count)
    assert L.copra_batch_get_trace_quantiles(eng._h, 2, 0, room.ctypes.data) == _capi.COPRA_OK
    assert L.copra_batch_get_trace_quantiles(eng._h, 1, 1, room.ctypes.data) == _capi.COPRA_OK
    assert room[:18].tobytes() == eng.trace_quantiles()["x"][1].tobytes() + eng.trace_quantiles()["u"][1].tobytes()


# ---- 10: a C caller ----
def test_c_caller_reads_the_band_of_a_row(tmp_path):
    """tests/cpp/test_trace_quant.cpp against include/copra_hip.h, as a fresh child process"""
    from copra_amd import _capi
    exe = str(tmp_path / "test_trace_quant")
    csrc = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_trace_quant.cpp"),
                           "-o", exe, "-L", csrc, "-lcopra_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
