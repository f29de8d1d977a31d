"""Closed-loop ticks on the device (copra_batch_advance / copra_batch_rollout; BatchLMPC.advance / rollout / state) against the CPU oracle and
numpy's plant step, tick by tick: the oracle solves every tick from the state the DEVICE held at that tick (x_hist[t]), so nothing compounds.

Measures: statuses (and, where results() is compared, both iteration counters) equal; controls and trajectories entry-wise 1e-6 with an absolute
floor of 1e-3 (the parity suite's); a plant step within the bound derived in tests/test_closed_loop_abi.py."""
import os
import subprocess

import numpy as np
import pytest

from test_closed_loop_abi import reference_step, step_bound

pytestmark = pytest.mark.gpu

RTOL = 1e-6
ABS_FLOOR = 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = 0.002  # position noise of examples/tracking.py
STUCK = (0, 77, 300, 511)  # instances that start far outside the velocity bound: infeasible at every tick (reference quirk Q5)


def _rel(a, b, floor=ABS_FLOOR):
    return np.nanmax(np.abs(a - b) / np.maximum(np.abs(b), floor))


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


def _assert_step(x_next, A, B, d, x, u, w, picks, what):
    """x_next[picks] against numpy's plant step in extended precision, within the derived bound"""
    nx, nu = B.shape[-2], B.shape[-1]
    Ap, Bp, dp = (v[picks] if v.ndim == n else v for v, n in ((A, 3), (B, 3), (d, 2)))
    ref, S = reference_step(Ap, Bp, dp, x[picks], u[picks], None if w is None else w[picks])
    err = np.abs(x_next[picks].astype(np.longdouble) - ref)
    bound = step_bound(nx, nu, S)
    print("%s: plant step max err / bound = %.3f" % (what, float((err / np.maximum(bound, np.finfo(float).tiny)).max())))
    assert (err <= bound).all(), what


def _position_noise(ticks, batch, nx, npos, seed):
    w = np.zeros((ticks, batch, nx))
    w[:, :, :npos] = NOISE * np.random.default_rng(seed).standard_normal((ticks, batch, npos))
    return w


def _check_history(oracle, wl, hist, w_seq, plant, fallback, stuck, what):
    """every tick of a rollout: the oracle from the device's x_hist[t]; the plant step from (x_hist[t], u_hist[t], w_seq[t])"""
    xh, uh, sh = (hist[k].cpu().numpy() for k in ("x_hist", "u_hist", "status_hist"))
    A, B, d = plant
    nu, batch = wl["B"].shape[2], wl["x0"].shape[0]
    ticks = uh.shape[0]
    assert not np.isnan(xh).any()
    want = np.zeros(batch, dtype=np.int32)
    want[list(stuck)] = 1
    for t in range(ticks):
        ref = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], xh[t], wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
        assert np.array_equal(sh[t], ref["status"]), (what, t)
        assert np.array_equal(sh[t], want), (what, t, np.nonzero(sh[t] != want)[0][:8])  # (a condition: a run in which everything failed cannot pass)
        ok = sh[t] == 0
        e = _rel(uh[t][ok], ref["control"][ok, :nu])
        print("%s tick %d: %d solved, first control against the oracle %.2e" % (what, t, ok.sum(), e))
        assert e <= RTOL, (what, t)
        _assert_step(xh[t + 1], A, B, d, xh[t], uh[t], w_seq[t], ok, "%s tick %d" % (what, t))
        if stuck:
            if fallback is None:
                assert np.array_equal(xh[t + 1][~ok], xh[t][~ok])  # held, bit for bit
                assert np.isnan(uh[t][~ok]).all()
            else:
                assert np.array_equal(uh[t][~ok], fallback[~ok])
                _assert_step(xh[t + 1], A, B, d, xh[t], fallback, w_seq[t], ~ok, "%s tick %d, fallback" % (what, t))


def test_one_tick(oracle):
    from copra_amd import workloads
    wl = workloads.com_preview(4096)
    eng = _engine(wl)
    eng.solve()
    before = eng.results()
    assert (before["status"] == 0).all()
    eng.advance()
    x1 = eng.state()
    _assert_step(x1, wl["A"], wl["B"], wl["d"], wl["x0"], before["control"][:, :3], None, np.ones(4096, dtype=bool), "one tick")
    after = eng.results()
    for k in before:
        assert np.array_equal(before[k], after[k], equal_nan=True), k  # the results are only read
    eng.solve()
    res = eng.results()
    ref = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], x1, wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
    assert np.array_equal(res["status"], ref["status"]) and np.array_equal(res["iter"], ref["iter"])
    ok = ref["status"] == 0
    assert ok.any()
    assert _rel(res["control"][ok], ref["control"][ok]) <= RTOL
    assert _rel(res["trajectory"][ok], ref["trajectory"][ok]) <= RTOL
    assert np.abs(res["trajectory"][:, :6] - x1).max() <= 1e-12 < np.abs(x1 - wl["x0"]).min(axis=1).max()  # the second solve read the new state


def _workload(name):
    from copra_amd import workloads
    if name == "com":
        return workloads.com_preview(512), 3, True
    if name == "com_tight":
        return workloads.com_preview(512, v_max=0.25), 3, True
    if name == "jerk":
        return workloads.jerk_preview(512), 3, True
    return workloads.double_integrator(512, N=16), 1, False


@pytest.mark.parametrize("name", ["com", "com_tight", "jerk", "double_integrator"])
@pytest.mark.parametrize("fallback", [False, True])
def test_closed_loop_against_the_oracle(oracle, name, fallback):
    wl, npos, has_bound = _workload(name)
    wl = dict(wl, x0=wl["x0"].copy())
    stuck = STUCK if has_bound else ()
    for b in stuck:
        wl["x0"][b, 3] = 50.0
    batch, nx, nu = wl["x0"].shape[0], wl["B"].shape[1], wl["B"].shape[2]
    w_seq = _position_noise(8, batch, nx, npos, seed=11)
    fb = np.zeros((batch, nu)) if fallback else None
    eng = _engine(wl)
    if name == "double_integrator":
        assert eng.lanes_per_instance() in (16, 32)  # the packed kernels
    hist = eng.rollout(8, disturbances=w_seq, fallback_control=fb, x_hist=True, u_hist=True, status_hist=True)
    assert np.array_equal(hist["x_hist"][0].cpu().numpy(), wl["x0"])
    assert np.array_equal(eng.state(), hist["x_hist"][8].cpu().numpy())
    _check_history(oracle, wl, hist, w_seq, (wl["A"], wl["B"], wl["d"]), fb, stuck, name + (" with fallback" if fallback else ""))


@pytest.mark.parametrize("mode", ["shared_model", "shared_model_kernels", "other_plant", "other_plant_shared"])
def test_closed_loop_shared_model_and_other_plants(oracle, mode, monkeypatch):
    from copra_amd import workloads, _capi
    if mode == "shared_model_kernels":  # (the shared-model kernels themselves; otherwise the model is written out per instance at this shape)
        monkeypatch.setitem(_capi.OPTIONS, "no_axis_solver", 1)
    wl = workloads.com_preview(512)
    wl = dict(wl, x0=wl["x0"].copy())
    shared_model = mode.startswith("shared_model")
    if shared_model:
        wl["A"], wl["B"], wl["d"] = (np.ascontiguousarray(np.broadcast_to(wl[k][0], wl[k].shape)) for k in ("A", "B", "d"))
    for b in STUCK:
        wl["x0"][b, 3] = 50.0
    w_seq = _position_noise(8, 512, 6, 3, seed=12)
    eng = _engine(wl, shared_model=shared_model)
    plant, kw = (wl["A"], wl["B"], wl["d"]), {}
    if mode == "other_plant":
        plant = (wl["A"], 0.9 * wl["B"], wl["d"])
        kw = dict(plant=plant)
    elif mode == "other_plant_shared":
        plant = (wl["A"][5], 0.9 * wl["B"][5], wl["d"][5] + 1e-3)
        kw = dict(plant=plant, shared=True)
    hist = eng.rollout(8, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True, **kw)
    _check_history(oracle, wl, hist, w_seq, plant, None, STUCK, mode)


def test_rollout_is_the_loop():
    """rollout(5) and five solve(); advance() calls: 1e-9 between two routes through the kernels (the figure of tests/test_emu_kernels.py; the
    header promises 1e-11 per solve across adaptation decisions, not bit-identity)"""
    import torch
    from copra_amd import workloads
    wl = workloads.com_preview(2048)
    w_seq = _position_noise(5, 2048, 6, 3, seed=13)
    a, b = _engine(wl), _engine(wl)
    ha = a.rollout(5, disturbances=w_seq, x_hist=True, status_hist=True)
    wd = torch.from_numpy(w_seq).cuda()
    xs, ss = [wl["x0"]], []
    for t in range(5):
        b.solve()
        o = b.advance(disturbance=wd[t], status_out=True)
        ss.append(o["status_out"].cpu().numpy())
        xs.append(b.state())
    assert np.array_equal(ha["status_hist"].cpu().numpy(), np.stack(ss))
    assert (np.stack(ss) == 0).any()
    d = np.abs(ha["x_hist"].cpu().numpy() - np.stack(xs)).max()
    print("rollout against solve + advance: max difference of the states %.2e" % d)
    assert d <= 1e-9


def test_ownership_outputs_and_errors():
    import torch
    from copra_amd import BatchLMPC, _capi, workloads
    from copra_amd.sharding import alloc_result_slab
    wl = workloads.com_preview(1024)
    eng = _engine(wl)
    with pytest.raises(_capi.CopraRuntimeError):  # no solve yet
        eng.advance()
    x = torch.from_numpy(wl["x0"]).cuda()
    keep = x.clone()
    eng.set_x0(x)
    assert eng.state_ptr() == x.data_ptr()
    eng.solve()
    first = eng.results()
    eng.advance()
    eng.synchronize()
    assert torch.equal(x, keep)  # the caller's tensor is read, never written
    assert eng.state_ptr() not in (0, x.data_ptr())
    with pytest.raises(ValueError):  # a partial plant: COPRA_ERR_ARG
        eng.advance(plant=(wl["A"], None, wl["d"]))
    with pytest.raises(_capi.CopraDomainError):
        eng.advance(disturbance=np.zeros((1024, 5)))
    # copra_batch_set_outputs: the buffers of the last LAUNCHED solve are the ones read
    slab, out = alloc_result_slab(1024, 3 * wl["N"], 6 * (wl["N"] + 1), torch.device("cuda:0"))
    eng.set_outputs(out["control"], out["trajectory"], out["status"], out["iter"])
    with pytest.raises(_capi.CopraRuntimeError):  # nothing has been solved into them
        eng.advance()
    x1 = eng.state()
    eng.solve()
    torch.cuda.synchronize()
    u = out["control"][:, :3].cpu().numpy()
    assert (out["status"] == 0).all() and not np.array_equal(u, first["control"][:, :3])
    eng.advance()
    _assert_step(eng.state(), wl["A"], wl["B"], wl["d"], x1, u, None, np.ones(1024, dtype=bool), "set_outputs")
    # InitialStateLMPC: its x0 is a decision variable
    pb = __import__("fixtures").bounded_system("trajectory", N=12)
    ise = BatchLMPC(2, 1, 12, 4, pb["costs"], pb["cstrs"], initial_state=dict(R=1e-2 * np.eye(2), r=np.zeros(2)))
    with pytest.raises(_capi.CopraUnsupported):
        ise.advance()
    with pytest.raises(_capi.CopraUnsupported):
        ise.rollout(2)
    L = _capi.lib()
    assert L.copra_batch_advance(None, None, None) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_rollout(eng._h, None, -1, None, None, None, None, None) == _capi.COPRA_ERR_ARG


def test_rollout_from_c(oracle, tmp_path):
    """tests/cpp/test_closed_loop.cpp: copra_batch_rollout from a C++ caller that includes include/copra_hip.h alone; its histories get the
    per-tick check of the Python route"""
    import torch
    from copra_amd import _capi, workloads
    _capi.build_library()
    src = os.path.join(ROOT, "tests", "cpp", "test_closed_loop.cpp")
    exe = str(tmp_path / "test_closed_loop")
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", src,
                           "-o", exe, "-L", libdir, "-lcopra_hip", "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    batch, ticks = 512, 4
    wl = workloads.com_preview(batch)
    wl = dict(wl, x0=wl["x0"].copy())
    for b in STUCK:
        wl["x0"][b, 3] = 50.0
    w_seq = _position_noise(ticks, batch, 6, 3, seed=14)
    cst = wl["cstrs"]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        np.array([batch, wl["N"], ticks], dtype=np.int32).tofile(fh)
        for v in (wl["costs"][0]["p"], wl["costs"][0]["weights"], wl["costs"][1]["weights"], cst[0]["upper"], cst[1]["upper"],
                  np.swapaxes(wl["A"], 1, 2), np.swapaxes(wl["B"], 1, 2), wl["d"], wl["x0"], w_seq):
            np.ascontiguousarray(v, dtype=np.float64).tofile(fh)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    raw = np.fromfile(fout, dtype=np.uint8)
    nxh, nuh = (ticks + 1) * batch * 6, ticks * batch * 3
    xh = raw[:8 * nxh].view(np.float64).reshape(ticks + 1, batch, 6)
    uh = raw[8 * nxh:8 * (nxh + nuh)].view(np.float64).reshape(ticks, batch, 3)
    sh = raw[8 * (nxh + nuh):].view(np.int32).reshape(ticks, batch)
    hist = dict(x_hist=torch.from_numpy(xh.copy()), u_hist=torch.from_numpy(uh.copy()), status_hist=torch.from_numpy(sh.copy()))
    _check_history(oracle, wl, hist, w_seq, (wl["A"], wl["B"], wl["d"]), None, STUCK, "C caller")
