"""Reference schedules on the device (copra_batch_set_reference_schedule / _schedule_seek / _schedule_tick; BatchLMPC.set_reference_schedule,
schedule_seek, schedule_tick): tracking inside rollout, against the CPU oracle tick by tick -- the oracle solves every tick from the state the
DEVICE held at that tick (x_hist[t]) with the window of that tick as the cost's p, so nothing compounds (the method of
tests/test_closed_loop_gpu.py).

Measures: statuses equal to the oracle's AND all zero (a condition on the inputs, which tests/test_reference_schedule_inputs.py establishes with
the oracle alone); first controls entry-wise 1e-6 with an absolute floor of 1e-3 (the parity suite's); a plant step within the bound derived in
tests/test_closed_loop_abi.py; two routes through the kernels within 1e-9 (the bar of test_rollout_is_the_loop; the header documents 1e-11 per
solve around adaptation decisions)."""
import os
import subprocess

import numpy as np
import pytest

import tracking_cases as tc
from test_closed_loop_abi import reference_step, step_bound

pytestmark = pytest.mark.gpu

RTOL = tc.RTOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = 1e-9


def _engine(wl, shared_model=False, **kw):
    from copra_amd import BatchLMPC
    nx, nu, batch = wl["B"].shape[1], wl["B"].shape[2], wl["x0"].shape[0]
    eng = BatchLMPC(nx, nu, wl["N"], batch, wl["costs"], wl["cstrs"], **kw)
    if shared_model:
        eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
        eng.set_x0(wl["x0"])
    else:
        eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    return eng


def _schedule(signals, groups, per_instance):
    """what set_reference_schedule gets: (steps, r) for the batch, or (batch, steps, r)"""
    return np.ascontiguousarray(signals[groups]) if per_instance else signals[0]


def _assert_step(x_next, wl, x, u, w, what):
    nx, nu = wl["B"].shape[1], wl["B"].shape[2]
    ref, S = reference_step(wl["A"], wl["B"], wl["d"], x, u, w)
    err = np.abs(x_next.astype(np.longdouble) - ref)
    bound = step_bound(nx, nu, S)
    print("%s: plant step max err / bound = %.3f" % (what, float((err / np.maximum(bound, np.finfo(float).tiny)).max())))
    assert (err <= bound).all(), what


def _check_history(oracle, wl, signals, groups, hist, w_seq, S, offset, what, cost_index=0):
    """every tick of a tracking rollout against the oracle, from the device's x_hist[t] with the window of tick t; the vacuous pass excluded at the
    last tick: there the moved window must matter"""
    xh, uh, sh = (np.asarray(hist[k].cpu().numpy() if hasattr(hist[k], "cpu") else hist[k]) for k in ("x_hist", "u_hist", "status_hist"))
    nu = wl["B"].shape[2]
    ticks = uh.shape[0]
    assert not np.isnan(xh).any() and not np.isnan(uh).any()
    for t in range(ticks):
        ref = tc.oracle_tick(oracle, wl, xh[t], groups, [tc.window(s, t + offset, S) for s in signals], cost_index)
        assert np.array_equal(sh[t], ref["status"]), (what, t)
        assert (sh[t] == 0).all(), (what, t, np.nonzero(sh[t])[0][:8])
        e = float(tc.rel(uh[t], ref["control"][:, :nu]).max())
        print("%s tick %d: first control against the oracle %.2e" % (what, t, e))
        assert e <= RTOL, (what, t)
        _assert_step(xh[t + 1], wl, xh[t], uh[t], w_seq[t], "%s tick %d" % (what, t))
    last = ticks - 1
    share = tc.moved_share(oracle, wl, xh[last], groups, [tc.window(s, last + offset, S) for s in signals], [tc.window(s, offset, S) for s in signals], nu,
                           cost_index)
    print("%s: the moved window changes the first control of %.0f %% of the instances at tick %d" % (what, 100 * share, last))
    assert share >= 0.5, what


@pytest.mark.parametrize("per_instance", [False, True])
def test_tracking_rollout_against_the_oracle(oracle, per_instance):
    wl, signals = tc.tracking_workload()
    groups = tc.group_of(tc.BATCH, per_instance)
    w_seq = tc.position_noise(tc.TICKS, tc.BATCH, tc.NX, 3, seed=21)
    eng = _engine(wl)
    eng.set_reference_schedule(0, _schedule(signals, groups, per_instance), tc.NX)
    hist = eng.rollout(tc.TICKS, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True)
    assert np.array_equal(hist["x_hist"][0].cpu().numpy(), wl["x0"])
    assert eng.schedule_tick() == tc.TICKS
    _check_history(oracle, wl, signals, groups, hist, w_seq, wl["N"] + 1, 0, "tracking, %s" % ("per-instance schedules" if per_instance else "one schedule"))


@pytest.mark.parametrize("per_instance", [False, True])
def test_rollout_is_the_host_loop(per_instance):
    """the same 8 ticks with ONE rollout on the schedule, and with the calls that existed before schedules: set_cost_reference(window of the tick),
    solve, advance, once per tick.  The iteration counters of every tick come from a third controller that is rolled out tick by tick."""
    import torch
    wl, signals = tc.tracking_workload()
    S = wl["N"] + 1
    groups = tc.group_of(tc.BATCH, per_instance)
    w_seq = tc.position_noise(tc.TICKS, tc.BATCH, tc.NX, 3, seed=23)
    wd = torch.from_numpy(w_seq).cuda()
    a, b, c = _engine(wl), _engine(wl), _engine(wl)
    sched = _schedule(signals, groups, per_instance)
    a.set_reference_schedule(0, sched, tc.NX)
    ha = a.rollout(tc.TICKS, disturbances=wd, x_hist=True, u_hist=True, status_hist=True)
    c.set_reference_schedule(0, sched, tc.NX)
    xs, us, ss, its_b, its_c = [wl["x0"]], [], [], [], []
    for t in range(tc.TICKS):
        b.set_cost_reference(0, tc.window(sched, t, S))  # (1-D: one reference for the batch; 2-D: per instance)
        b.solve()
        its_b.append(b.results()["iter"])
        o = b.advance(disturbance=wd[t], status_out=True, u_out=True)
        ss.append(o["status_out"].cpu().numpy()), us.append(o["u_out"].cpu().numpy()), xs.append(b.state())
        c.rollout(1, disturbances=wd[t:t + 1])
        its_c.append(c.results()["iter"])
    assert b.schedule_tick() == tc.TICKS  # (the advances are counted, schedule or not)
    sa = ha["status_hist"].cpu().numpy()
    assert np.array_equal(sa, np.stack(ss)) and (sa == 0).all()
    assert np.array_equal(np.stack(its_c), np.stack(its_b))
    assert np.array_equal(a.results()["iter"], its_b[-1])
    dx = np.abs(ha["x_hist"].cpu().numpy() - np.stack(xs)).max()
    du = np.abs(ha["u_hist"].cpu().numpy() - np.stack(us)).max()
    print("rollout on the schedule against set_cost_reference + solve + advance: max difference of the states %.2e, of the controls %.2e" % (dx, du))
    assert dx <= ROUTES and du <= ROUTES
    assert np.abs(c.state() - xs[-1]).max() <= ROUTES


def _same_solve(x, y, what):
    rx, ry = x.results(), y.results()
    assert np.array_equal(rx["status"], ry["status"]) and (rx["status"] == 0).all(), what
    assert np.array_equal(rx["iter"], ry["iter"]), what
    d = max(np.abs(rx[k] - ry[k]).max() for k in ("control", "trajectory"))
    print("%s: max difference %.2e" % (what, d))
    assert d <= ROUTES, what
    return rx


def test_seek_tick_and_the_end_of_the_schedule():
    wl, signals = tc.tracking_workload()
    S, steps = wl["N"] + 1, signals.shape[1]
    sig = signals[1]

    def fresh(p):
        e = _engine(wl)
        if p is not None:
            e.set_cost_reference(0, p)
        e.solve()
        return e

    eng = _engine(wl)
    assert eng.schedule_tick() == 0
    eng.set_reference_schedule(0, sig, tc.NX)
    eng.solve()
    at0 = _same_solve(eng, fresh(tc.window(sig, 0, S)), "tick 0")
    # schedule_tick() counts the advances
    eng.rollout(3)
    assert eng.schedule_tick() == 3
    eng.solve()
    eng.advance()
    assert eng.schedule_tick() == 4
    # schedule_seek(k), then solve: a fresh controller given window k
    for k in (5, 2, steps - 3, steps + 5):
        eng.schedule_seek(k)
        assert eng.schedule_tick() == k
        eng.set_x0(wl["x0"])
        eng.solve()
        got = _same_solve(eng, fresh(tc.window(sig, k, S)), "seek %d" % k)
        assert np.abs(got["control"] - at0["control"]).max() > 1e-3  # (another window than tick 0's: the seek was not a no-op)
    # ... past the end the window is the last block, repeated
    _same_solve(eng, fresh(np.tile(sig[-1], S)), "past the end")
    # set_cost_reference(cost, None) ends the schedule: the creation reference, and ticks do not bring a window back
    eng.set_cost_reference(0, None)
    eng.set_x0(wl["x0"])
    eng.solve()
    _same_solve(eng, fresh(None), "creation reference")
    eng.advance()
    eng.set_x0(wl["x0"])
    eng.solve()
    _same_solve(eng, fresh(None), "creation reference after a tick")
    # sched = None ends the schedule and keeps the last window
    eng.set_reference_schedule(0, sig, tc.NX)
    eng.schedule_seek(6)
    eng.set_reference_schedule(0, None, tc.NX)
    eng.schedule_seek(1)
    assert eng.schedule_tick() == 1
    eng.set_x0(wl["x0"])
    eng.solve()
    _same_solve(eng, fresh(tc.window(sig, 6, S)), "the last window is kept")


def test_target_cost_reads_the_end_of_the_horizon():
    """a TargetCost with offset = N reads block tau + N (S = 1), on the packed small controller"""
    wl, signals = tc.integrator_workload()
    N = wl["N"]
    eng = _engine(wl)
    assert eng.lanes_per_instance() in (16, 32)
    eng.set_reference_schedule(0, signals[0], 2, offset=N)
    for k in (0, 3):
        eng.schedule_seek(k)
        eng.set_x0(wl["x0"])
        eng.solve()
        other = _engine(wl)
        other.set_cost_reference(0, signals[0][k + N])
        other.solve()
        _same_solve(eng, other, "target cost, tick %d" % k)
    wrong = _engine(wl)
    wrong.set_cost_reference(0, signals[0][3])  # (block tau, not tau + N: another solution)
    wrong.solve()
    assert np.abs(wrong.results()["control"] - eng.results()["control"]).max() > 1e-3


def test_torch_schedule_is_used_in_place_and_never_written():
    import torch
    wl, signals = tc.tracking_workload()
    S = wl["N"] + 1
    groups = tc.group_of(tc.BATCH, True)
    sched = torch.from_numpy(_schedule(signals, groups, True)).cuda()
    keep = sched.clone()
    eng = _engine(wl)
    eng.set_reference_schedule(0, sched, tc.NX)
    assert eng._held[("schedule", 0)] is sched
    eng.rollout(tc.TICKS + 25)  # (to beyond the end of the signal)
    eng.synchronize()
    assert torch.equal(sched, keep)
    # in place: what is written into the tensor is what the next window holds
    sched[:, 4:, 2] += 0.01
    eng.schedule_seek(4)
    eng.set_x0(wl["x0"])
    eng.solve()
    other = _engine(wl)
    other.set_cost_reference(0, tc.window(sched.cpu().numpy(), 4, S))
    other.solve()
    _same_solve(eng, other, "schedule tensor changed in place")
    stale = _engine(wl)
    stale.set_cost_reference(0, tc.window(keep.cpu().numpy(), 4, S))
    stale.solve()
    assert np.abs(stale.results()["control"] - eng.results()["control"]).max() > 1e-3
    eng.set_cost_reference(0, None)  # drops the kept tensor
    assert ("schedule", 0) not in eng._held


def test_error_codes():
    from copra_amd import BatchLMPC, _capi, workloads
    wl, signals = tc.tracking_workload(batch=64)
    eng = _engine(wl)
    L, h = _capi.lib(), eng._h
    sig = np.ascontiguousarray(signals[0])
    steps = sig.shape[0]

    def call(cost, ptr, steps_, r, offset, per=0):
        return L.copra_batch_set_reference_schedule(h, cost, ptr, steps_, r, offset, per, 0)

    assert call(0, sig.ctypes.data, steps, 6, 0) == _capi.COPRA_OK
    assert call(0, sig.ctypes.data, steps, 5, 0) == _capi.COPRA_ERR_DOMAIN  # 5 does not divide 126
    assert call(0, sig.ctypes.data, steps, 3, 0) == _capi.COPRA_ERR_DOMAIN  # divides, but the plan evaluates the cost step by step with 6 rows
    assert call(0, sig.ctypes.data, steps, 0, 0) == _capi.COPRA_ERR_DOMAIN
    assert call(0, sig.ctypes.data, 0, 6, 0) == _capi.COPRA_ERR_ARG
    assert call(0, sig.ctypes.data, steps, 6, -1) == _capi.COPRA_ERR_ARG
    assert call(2, sig.ctypes.data, steps, 6, 0) == _capi.COPRA_ERR_ARG  # no such cost
    assert call(-1, sig.ctypes.data, steps, 6, 0) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_schedule_seek(h, -1) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_schedule_seek(None, 0) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_set_reference_schedule(None, 0, sig.ctypes.data, steps, 6, 0, 0, 0) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_schedule_tick(None) == -1
    assert eng.schedule_tick() == 0  # (a refused seek changes nothing)
    with pytest.raises(_capi.CopraDomainError):
        eng.set_reference_schedule(0, sig, 5)  # (the binding: the last axis is not rows_per_step)
    with pytest.raises(_capi.CopraDomainError):
        eng.set_reference_schedule(0, np.zeros((63, steps, 6)), 6)  # (per instance, but not one per instance)
    # the control cost is a per-step cost of 3 rows: r = 3, S = 1; a full-size cost that is NOT evaluated step by step takes any divisor
    z3 = np.zeros((4, 3))
    assert call(1, z3.ctypes.data, 4, 3, 0) == _capi.COPRA_OK
    full = BatchLMPC(6, 3, wl["N"], 64, wl["costs"], wl["cstrs"], options=dict(no_stage_refs=1))
    z = np.zeros((4, 126))
    assert L.copra_batch_set_reference_schedule(full._h, 0, z.ctypes.data, 4, 3, 0, 0, 0) == _capi.COPRA_OK
    assert L.copra_batch_set_reference_schedule(full._h, 0, z.ctypes.data, 4, 126, 0, 0, 0) == _capi.COPRA_OK
    # a dense (host-evaluated) cost has no reference
    cw = workloads.com_preview(64)
    n = 3 * cw["N"]
    dense = BatchLMPC(6, 3, cw["N"], 64, [cw["costs"][0], dict(kind="dense", Q=1e-3 * np.eye(n), c=np.zeros(n))], cw["cstrs"])
    with pytest.raises(_capi.CopraUnsupported):
        dense.set_reference_schedule(1, np.zeros((4, 3)), 3)


@pytest.mark.parametrize("path", ["shared_model", "shared_model_kernels", "packed"])
def test_tracking_on_the_other_paths(oracle, path, monkeypatch):
    """the window is plain per-instance reference data: a shared-model controller (its model written out per instance at this shape, or on the
    shared-model kernels themselves) and a packed small controller take it"""
    from copra_amd import _capi
    if path == "shared_model_kernels":
        monkeypatch.setitem(_capi.OPTIONS, "no_axis_solver", 1)
    if path == "packed":
        wl, signals = tc.integrator_workload()
        groups = np.arange(tc.BATCH) % 2
        w_seq = tc.position_noise(tc.TICKS, tc.BATCH, 2, 1, seed=22)
        eng = _engine(wl)
        assert eng.lanes_per_instance() in (16, 32)
        eng.set_reference_schedule(0, np.ascontiguousarray(signals[groups]), 2, offset=wl["N"])
        S, offset = 1, wl["N"]
    else:
        wl, signals = tc.tracking_workload(shared_model=True)
        groups = tc.group_of(tc.BATCH, True)
        w_seq = tc.position_noise(tc.TICKS, tc.BATCH, tc.NX, 3, seed=21)
        eng = _engine(wl, shared_model=True)
        eng.set_reference_schedule(0, _schedule(signals, groups, True), tc.NX)
        S, offset = wl["N"] + 1, 0
    hist = eng.rollout(tc.TICKS, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True)
    _check_history(oracle, wl, signals, groups, hist, w_seq, S, offset, path)


def test_tracking_loop_from_c(oracle, tmp_path):
    """tests/cpp/test_tracking_loop.cpp: copra_batch_set_reference_schedule and copra_batch_rollout from a C++ caller that includes
    include/copra_hip.h alone.  It compares its histories with the ones this test hands it (the Python route's, which get the per-tick check
    against the oracle here) and writes them out; they get the same check."""
    from copra_amd import _capi
    _capi.build_library()
    src = os.path.join(ROOT, "tests", "cpp", "test_tracking_loop.cpp")
    exe = str(tmp_path / "test_tracking_loop")
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-o", exe, "-L", libdir, "-lcopra_hip", "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    batch, ticks = tc.BATCH, 4
    wl, signals = tc.tracking_workload()
    N = wl["N"]
    groups = tc.group_of(batch, True)
    sched = _schedule(signals, groups, True)
    w_seq = tc.position_noise(ticks, batch, tc.NX, 3, seed=24)
    eng = _engine(wl)
    eng.set_reference_schedule(0, sched, tc.NX)
    hist = eng.rollout(ticks, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True)
    _check_history(oracle, wl, signals, groups, hist, w_seq, N + 1, 0, "Python route")
    cst = wl["cstrs"]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        np.array([batch, N, ticks, sched.shape[1], 1], dtype=np.int32).tofile(fh)
        for v in (tc.TRACK_W, wl["costs"][1]["weights"], cst[0]["upper"], cst[1]["upper"], np.swapaxes(wl["A"], 1, 2), np.swapaxes(wl["B"], 1, 2),
                  wl["d"], wl["x0"], w_seq, sched, hist["x_hist"].cpu().numpy(), hist["u_hist"].cpu().numpy()):
            np.ascontiguousarray(v, dtype=np.float64).tofile(fh)
        np.ascontiguousarray(hist["status_hist"].cpu().numpy(), dtype=np.int32).tofile(fh)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = np.fromfile(fout, dtype=np.uint8)
    nxh, nuh = (ticks + 1) * batch * 6, ticks * batch * 3
    xh = raw[:8 * nxh].view(np.float64).reshape(ticks + 1, batch, 6)
    uh = raw[8 * nxh:8 * (nxh + nuh)].view(np.float64).reshape(ticks, batch, 3)
    sh = raw[8 * (nxh + nuh):].view(np.int32).reshape(ticks, batch)
    assert np.abs(xh - hist["x_hist"].cpu().numpy()).max() <= ROUTES and np.abs(uh - hist["u_hist"].cpu().numpy()).max() <= ROUTES
    _check_history(oracle, wl, signals, groups, dict(x_hist=xh, u_hist=uh, status_hist=sh), w_seq, N + 1, 0, "C caller")
