"""The tick at its launch edges on the device: what copra_hip_plant.hip decides at shapes no other GPU test reaches -- group 1 (every copy
the scalar loop), an image above 48 KiB (the dynamic-LDS opt-in), refusals instead of launches, rows of a rollout that are only 8-byte
aligned on every other tick, a caller's misaligned arrays, and flag combinations whose image no other GPU test lays out.

The controller of each shape is the cheapest there is (scenario): one TargetCost with a single row, a ControlCost, a wide control bound and an
upper bound on the last state alone -- that state is decoupled (x+ = x / 2 + 0.01, no control, no disturbance), so an instance that starts far above
the bound is infeasible at every tick (the stuck instances of tests/test_closed_loop_gpu.py) and every other one never meets it.  Batch 5
from nx 40 on, else 13.

Every check of a history is one of the neighbouring files' own (test_closed_loop_gpu._check_history, test_bias_estimator_gpu._check,
test_observer_gpu._check): the oracle solves every tick from the DEVICE's own state, estimate and d (statuses equal, first controls within
RTOL), and the plant step, the estimates and the outputs stay within step_bound, bias_bound and Ey / Eh / Ed computed from the device's own
previous history and its own u_hist / status_hist / age_hist; held instances bit for bit.  Where noise is drawn on top of a given w the
reference gets w + term in longdouble: the one rounding of that sum on the device is the rounding step_bound counts beyond the
2 (nx + nu) + 1 the chain has.

The launch rule is asked of tests/emu (emu_plant_launch_group, emu_plant_image_bytes: plant_step.hpp's own functions), never restated."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_bias_estimator_gpu import _check as bias_history
from test_closed_loop_gpu import RTOL, _assert_step, _check_history, _engine, _rel
from test_observer_abi import LD, reference_observer
from test_observer_gpu import _check as observer_history

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALLBACK, HELD = -1, -2
SEED = 0x7ed9e5
KIND = dict(plain=0, est=1, obs=2)
V_MAX = 0.6


@pytest.fixture(scope="module")
def geo(tmp_path_factory):
    """the launch geometry of plant_step.hpp, through the emulator's exports"""
    so = str(tmp_path_factory.mktemp("emu_geometry") / "libemu_plant.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "emu", "emu_plant.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.emu_plant_image_bytes.restype, lib.emu_plant_image_bytes.argtypes = ctypes.c_longlong, [ctypes.c_int] * 5
    lib.emu_plant_launch_group.restype, lib.emu_plant_launch_group.argtypes = ctypes.c_int, [ctypes.c_int] * 5
    lib.emu_plant_lds_max.restype = ctypes.c_longlong
    return lib


def _numpy(hist):
    return {k: v.cpu().numpy() for k, v in hist.items() if v is not None}


def _bits(a, b):
    import torch
    if not torch.is_tensor(a):
        a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all())


def scenario(nx, nu, ny, N, ticks, seed=1, batch=None):
    """dict(wl, plant, w_seq, v_seq, held, fb, gains ...) of one shape; every matrix in natural indexing"""
    batch = batch or (5 if nx >= 40 else 13)
    held = (1,) if batch < 10 else (1, batch - 2)
    rng = np.random.default_rng(1000 * nx + 10 * nu + seed)
    j = nx - 1  # the bounded state: x+ = x / 2 + 0.01 in the model and in every plant
    A = 0.5 * rng.standard_normal((batch, nx, nx)) / np.sqrt(nx)
    B = rng.standard_normal((batch, nx, nu))
    d = 0.1 * rng.standard_normal((batch, nx))
    x0 = rng.standard_normal((batch, nx))
    x0[:, j] = rng.uniform(-0.2, 0.2, batch)
    x0[list(held), j] = 50.0  # 25, 12.5, ... : above the bound for more ticks than any test here runs
    Ap, Bp, dp = A * (1.0 - 0.02 * rng.uniform(0.0, 1.0, A.shape)), 0.95 * B, d + 0.01 * rng.standard_normal((batch, nx))
    for M in (A, Ap):
        M[:, j, :] = 0.0
        M[:, j, j] = 0.5
    B[:, j], Bp[:, j], d[:, j], dp[:, j] = 0.0, 0.0, 0.01, 0.01  # (a d_j that is not zero: the bound on the estimate of d_j is not zero either)
    w_seq = 0.01 * rng.standard_normal((ticks, batch, nx))
    w_seq[:, :, j] = 0.0
    inf = np.inf
    costs = [dict(kind="target", M=rng.standard_normal((1, nx)) / np.sqrt(nx), p=[0.3], weights=[1.0]),
             dict(kind="control", N=np.eye(nu), p=np.zeros(nu), weights=[0.5] * nu)]
    cstrs = [dict(kind="trajectory_bound", lower=[-inf] * nx, upper=[inf] * (nx - 1) + [V_MAX]), dict(kind="control_bound", lower=[-1e3] * nu, upper=[1e3] * nu)]
    # gains that leave row j alone: neither d_j nor the estimate of x_j learns anything, an instance stays on its side of the bound
    gd = 0.5 * np.eye(nx) + 0.05 * rng.uniform(-1.0, 1.0, (batch, nx, nx))
    gl = rng.uniform(0.3, 0.8, (batch, nx))
    gd[:, j, :], gl[:, j] = 0.0, 0.0
    ny = max(ny, 1)
    C = rng.standard_normal((batch, ny, nx)) / np.sqrt(nx)
    Lx, Ld = 0.3 * rng.uniform(-1.0, 1.0, (batch, nx, ny)) / np.sqrt(ny), 0.1 * rng.uniform(-1.0, 1.0, (batch, nx, ny)) / np.sqrt(ny)
    Lx[:, j, :], Ld[:, j, :] = 0.0, 0.0
    xhat0 = x0 + 0.05 * rng.standard_normal((batch, nx))
    xhat0[:, j] = x0[:, j]
    return dict(wl=dict(A=A, B=B, d=d, x0=x0, N=N, costs=costs, cstrs=cstrs), plant=(Ap, Bp, dp), w_seq=w_seq, held=held, ny=ny, batch=batch,
                v_seq=1e-3 * rng.standard_normal((ticks, batch, ny)), fb=0.1 * rng.standard_normal((batch, nu)), gd=gd, gl=gl, C=C, Lx=Lx, Ld=Ld,
                xhat0=xhat0, sw=np.where(np.arange(nx) == j, 0.0, 0.01) * np.ones((batch, nx)), sv=1e-3 * np.ones((batch, ny)))


def first_creatable(nx, nu, ny, N, ticks, keeps, what):
    """the scenario and a controller of the largest nx' <= nx that BatchLMPC accepts and that keeps the case's property"""
    from copra_amd import _capi
    for n in range(nx, 1, -1):
        k = ny if ny < nx // 2 else (n // 2 if ny == nx // 2 else n)  # (ny follows nx where the issue names it as nx / 2)
        if not keeps(n, k):
            break
        S = scenario(n, nu, k, N, ticks)
        try:
            eng = _engine(S["wl"])
            eng.solve()
        except _capi.CopraUnsupported as e:
            print("%s: nx %d refused (%s)" % (what, n, e))
            continue
        if n != nx:
            print("%s: nx stepped down from %d to %d" % (what, nx, n))
        return S, eng
    raise AssertionError("%s: no creatable shape keeps the property" % what)


def ages_of(sh, fallback):
    return np.where(sh == 0, 0, FALLBACK if fallback else HELD).astype(np.int32)


def mixed(sh):
    """every tick shows a solved and a failed instance"""
    assert ((sh == 0).any(axis=-1) & (sh != 0).any(axis=-1)).all(), sh


def run(eng, S, mode, ticks, w_seq="given", backup=0, per=True, dense=True, with_Ld=True, plant=True, shared=False, fallback=False, noise=None):
    """a rollout of `ticks` in mode plain | est | obs; returns (histories as numpy, the arguments of the neighbouring file's check)"""
    kw = {}
    if backup:
        eng.set_backup_steps(backup)
        kw["age_hist"] = True
    P = None
    if plant:
        P = tuple(m[0] for m in S["plant"]) if shared else S["plant"]
        kw.update(plant=P, shared=shared)
    if fallback:
        kw["fallback_control"] = S["fb"]
    if isinstance(w_seq, str):
        w_seq = S["w_seq"][:ticks]
    if w_seq is not None:
        kw["disturbances"] = np.ascontiguousarray(w_seq, dtype=np.float64)
    gain = None
    if mode == "est":
        gain = (S["gd"] if dense else S["gl"]) if per else (S["gd"][0] if dense else S["gl"][0])
        eng.set_bias_estimator(gain)
        kw["d_hist"] = True
    if mode == "obs":
        pick = (lambda m: m) if per else (lambda m: m[0])
        C, Lx, Ld = pick(S["C"]), pick(S["Lx"]), pick(S["Ld"]) if with_Ld else None
        eng.set_observer(C, Lx, Ld)
        eng.set_x0(S["xhat0"])
        kw.update(noise=S["v_seq"][:ticks], y_hist=True, xhat_hist=True, d_hist=with_Ld)
    if noise:
        eng.set_noise(SEED, process=S["sw"], sensor=S["sv"] if mode == "obs" else None)
    hist = _numpy(eng.rollout(ticks, x_hist=True, u_hist=True, status_hist=True, **kw))
    return hist, dict(P=P if plant else None, gain=gain, obs=(C, Lx, Ld) if mode == "obs" else None, fallback=fallback, backup=backup, w_seq=w_seq)


def check(oracle, S, mode, hist, a, what, w_seq=None, v_seq=None):
    """the neighbouring files' own per-tick checks; w_seq / v_seq: what the ticks really added (given + drawn)"""
    wl, held = S["wl"], S["held"]
    sh = hist["status_hist"]
    ticks = sh.shape[0]
    mixed(sh)
    w_seq = a["w_seq"] if w_seq is None else w_seq
    w_seq = np.zeros((ticks,) + S["wl"]["x0"].shape) if w_seq is None else w_seq
    ages = ages_of(sh, a["fallback"])
    if a["backup"]:  # a solve at every tick: no instance ever plays its plan
        assert np.array_equal(hist["age_hist"], ages), what
    plant = a["P"] if a["P"] is not None else (wl["A"], wl["B"], wl["d"])
    if mode == "plain":
        import torch
        fb = S["fb"] if a["fallback"] else None
        want = np.zeros(S["batch"], dtype=bool)
        want[list(held)] = True
        assert np.array_equal(sh != 0, np.broadcast_to(want, sh.shape)), what
        _check_history(oracle, wl, {k: torch.from_numpy(np.ascontiguousarray(hist[k])) for k in ("x_hist", "u_hist", "status_hist")}, w_seq, plant, fb, held, what)
    elif mode == "est":
        bias_history(oracle, wl, hist, plant, w_seq, a["gain"], held, what, ages=ages, moved_share=False)
    else:
        C, Lx, Ld = a["obs"]
        T = dict(wl=wl, held=held, Ld=Ld, C=C, Lx=Lx, xhat0=S["xhat0"], plant=plant, w_seq=w_seq, v_seq=S["v_seq"][:ticks] if v_seq is None else v_seq)
        observer_history(oracle, T, hist, what, plant=a["P"] is not None, ages=ages)
    u = hist["u_hist"]
    assert np.array_equal(np.isnan(u).any(axis=2), ages == HELD), what


# ---- 1: group 1 on the device ----
@pytest.mark.parametrize("mode,nx,nu,ny", [("plain", 40, 1, 0), ("est", 23, 1, 0), ("obs", 23, 1, 11)])
def test_group_one_on_the_device(oracle, geo, mode, nx, nu, ny):
    """plain (40, 1), dense estimator (23, 1), observer (23, 1, 11): one instance per workgroup, every copy the scalar loop; four ticks"""
    keeps = lambda n, k: geo.emu_plant_launch_group(KIND[mode], n, nu, k, 1) == 1  # noqa: E731
    S, eng = first_creatable(nx, nu, ny, 1, 4, keeps, "group 1 " + mode)  # nx used: as named (40; 23; 23)
    hist, a = run(eng, S, mode, 4)
    check(oracle, S, mode, hist, a, "group 1 %s nx %d" % (mode, S["wl"]["A"].shape[1]))


# ---- 2: an image above 48 KiB ----
def _replayed(S, mode, ticks, drawn_w, backup):
    eng = _engine(S["wl"])
    return run(eng, S, mode, ticks, w_seq=drawn_w, backup=backup)[0]


@pytest.mark.parametrize("mode,nx,nu,ny,N,noise", [("plain", 78, 1, 0, 1, False), ("plain", 78, 1, 0, 1, True), ("est", 56, 1, 0, 2, False), ("est", 56, 1, 0, 2, True),
                                                   ("obs", 56, 1, 28, 2, False)])
def test_image_above_48_kib(oracle, geo, mode, nx, nu, ny, N, noise):
    """plain (78, 1) at N = 1; dense estimator (56, 1) and observer (56, 1, 28) at N = 2 with backup plans of one step: the launch opts in to
    more than 48 KiB of dynamic LDS; two ticks.  With noise drawn on the device: the same checks with the drawn terms as w, and a fresh
    controller handed draw_noise's terms gives the same bits (the replay of tests/test_noise_gpu.py)"""
    keeps = lambda n, k: geo.emu_plant_image_bytes(KIND[mode], n, nu, k, 1) > 48 * 1024  # noqa: E731
    S, eng = first_creatable(nx, nu, ny, N, 2, keeps, "above 48 KiB " + mode)  # nx used: as named (78; 56; 56)
    backup = N - 1
    what = "above 48 KiB %s nx %d%s" % (mode, S["wl"]["A"].shape[1], " noise" if noise else "")
    if not noise:
        hist, a = run(eng, S, mode, 2, backup=backup)
        check(oracle, S, mode, hist, a, what)
        return
    hist, a = run(eng, S, mode, 2, w_seq=None, backup=backup, noise=True)
    assert eng.noise_tick == 2
    drawn = np.stack([eng.draw_noise(t).cpu().numpy() for t in range(2)])
    assert np.abs(drawn).max() > 0 and (drawn[:, :, -1] == 0).all()
    check(oracle, S, mode, hist, a, what, w_seq=drawn)
    again = _replayed(S, mode, 2, drawn, backup)
    for k in hist:
        assert _bits(hist[k], again[k]), (what, k)


# ---- 3: refusals, not faults ----
def test_what_does_not_fit_is_refused(geo):
    """the observer at the first ny whose widest image passes the LDS, the dense estimator at the first such nx (where a controller of that nx
    can be created at all): COPRA_ERR_UNSUPPORTED, and the handle ticks on.  The limit is the exported geometry's; the library's answer on
    either side of it is asserted"""
    from copra_amd import _capi
    top = geo.emu_plant_lds_max()
    nx, nu = 56, 1
    S = scenario(nx, nu, 1, 1, 1)
    eng = _engine(S["wl"])
    ny = next(k for k in range(1, 4 * nx) if geo.emu_plant_image_bytes(2, nx, nu, k, 0) > top)
    assert ny > 1 and geo.emu_plant_image_bytes(2, nx, nu, ny - 1, 0) <= top
    print("observer at nx %d: ny %d is the first that does not fit" % (nx, ny))
    with pytest.raises(_capi.CopraUnsupported):
        eng.set_observer(np.zeros((ny, nx)), np.zeros((nx, ny)), np.zeros((nx, ny)))
    eng.set_observer(np.zeros((ny - 1, nx)), np.zeros((nx, ny - 1)), np.zeros((nx, ny - 1)))  # the last that fits is taken ...
    eng.set_observer(None)  # ... and ended: the tick below is the plain one
    eng.set_x0(S["wl"]["x0"])
    eng.solve()
    out = _numpy(eng.advance(x_out=True, u_out=True, status_out=True))
    mixed(out["status_out"])
    moved = out["status_out"] == 0
    _assert_step(out["x_out"], S["wl"]["A"], S["wl"]["B"], S["wl"]["d"], S["wl"]["x0"], np.where(moved[:, None], out["u_out"], 0.0), None, moved, "after the refusal")
    assert np.array_equal(out["x_out"][~moved], S["wl"]["x0"][~moved])
    # the dense estimator
    bad = next(n for n in range(2, 400) if geo.emu_plant_image_bytes(1, n, nu, 0, 1) > top)
    assert geo.emu_plant_image_bytes(1, bad - 1, nu, 0, 1) <= top
    T = scenario(bad, nu, 1, 1, 1)
    try:
        big = _engine(T["wl"])
    except _capi.CopraUnsupported as e:
        print("dense estimator: nx %d is the first that does not fit, and no controller of that nx can be created (%s)" % (bad, e))
        return
    with pytest.raises(_capi.CopraUnsupported):
        big.set_bias_estimator(np.zeros((bad, bad)))
    big.set_bias_estimator(np.zeros(bad))  # (the diagonal gain fits)
    big.solve()
    out = _numpy(big.advance(status_out=True))
    mixed(out["status_out"])


# ---- 4: odd rows in a rollout ----
@pytest.mark.parametrize("mode,nx,nu,ny", [("plain", 5, 2, 0), ("est", 5, 2, 0), ("obs", 5, 2, 2), ("plain", 9, 3, 0), ("est", 9, 3, 0), ("obs", 9, 3, 3)])
def test_odd_rows_of_a_rollout_are_the_aligned_loop(mode, nx, nu, ny):
    """batch 13: batch nx is odd (and batch ny at ny = 3), so w_seq + t batch nx and v_seq + t batch ny are only 8-byte aligned on the odd ticks
    of rollout(6) -- those ticks copy double by double, the even ones two doubles per lane.  Six solve(); advance() calls that are each given
    a separately allocated copy of the tick's row copy two doubles per lane at every tick: every history is bit-equal"""
    import torch
    ticks = 6
    S = scenario(nx, nu, ny, 3, ticks)
    assert (S["batch"] * nx) % 2 == 1
    a, b = _engine(S["wl"]), _engine(S["wl"])
    hist, _ = run(a, S, mode, ticks, dense=True, per=True)
    mixed(hist["status_hist"])
    # the loop: the same set-up, then solve(); advance() with rows of their own (torch allocates on 512 bytes)
    if mode == "est":
        b.set_bias_estimator(S["gd"])
    if mode == "obs":
        b.set_observer(S["C"], S["Lx"], S["Ld"])
        b.set_x0(S["xhat0"])
    wd, vd = torch.from_numpy(S["w_seq"]).cuda(), torch.from_numpy(S["v_seq"]).cuda()
    rows = [(wd[t].clone(), vd[t].clone()) for t in range(ticks)]
    assert all(w.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0 for w, v in rows) and any((wd[t].data_ptr() % 16) == 8 for t in range(ticks))
    outs = []
    for t in range(ticks):
        b.solve()
        kw = dict(d_out=True) if mode != "plain" else {}
        if mode == "obs":
            kw.update(noise=rows[t][1], y_out=True, xhat_out=True)
        outs.append(b.advance(plant=S["plant"], disturbance=rows[t][0], x_out=True, u_out=True, status_out=True, **kw))
    names = dict(x_out="x_hist", u_out="u_hist", status_out="status_hist", d_out="d_hist", y_out="y_hist", xhat_out="xhat_hist")
    for t in range(ticks):
        for k, h in names.items():
            if outs[t].get(k) is not None:
                got = outs[t][k].cpu().numpy()
                assert _bits(hist[h][t + 1 if k == "x_out" else t], got), (mode, nx, t, k)


# ---- 5: a caller's misaligned arrays ----
@pytest.mark.parametrize("mode", ["plain", "est", "obs"])
def test_a_callers_misaligned_arrays(mode):
    """(6, 3, 3), batch 14: the plant, w, v and the fallback control as views one double into larger CUDA tensors -- contiguous, 8 bytes past
    a 16-byte boundary -- against the same tick with tensors of their own: bit-equal"""
    import torch
    nx, nu, ny = 6, 3, 3
    S = scenario(nx, nu, ny, 3, 1, batch=14)
    Ap, Bp, dp = S["plant"]
    arrays = dict(A=np.swapaxes(Ap, 1, 2), B=np.swapaxes(Bp, 1, 2), d=dp, w=S["w_seq"][0], v=S["v_seq"][0], fb=S["fb"])  # (the ABI's layout)
    outs = {}
    for mis in (False, True):
        t = {}
        for k, a in arrays.items():
            a = np.ascontiguousarray(a)
            big = torch.zeros(a.size + 2, dtype=torch.float64, device="cuda")
            off = 1 if mis else 0
            big[off:off + a.size] = torch.from_numpy(a.ravel()).cuda()
            t[k] = big[off:off + a.size].view(a.shape)
            assert t[k].is_contiguous() and t[k].data_ptr() % 16 == (8 if mis else 0)
        eng = _engine(S["wl"])
        kw = {}
        if mode == "est":
            eng.set_bias_estimator(S["gd"])
            kw["d_out"] = True
        if mode == "obs":
            eng.set_observer(S["C"], S["Lx"], S["Ld"])
            eng.set_x0(S["xhat0"])
            kw.update(noise=t["v"], y_out=True, xhat_out=True, d_out=True)
        eng.solve()
        outs[mis] = _numpy(eng.advance(plant=(t["A"], t["B"], t["d"]), disturbance=t["w"], fallback_control=t["fb"], x_out=True, u_out=True, status_out=True,
                                       age_out=True, **kw))
    mixed(outs[False]["status_out"])
    assert (outs[False]["age_out"][list(S["held"])] == FALLBACK).all()
    assert set(outs[False]) == set(outs[True]) and len(outs[False]) >= 4
    for k in outs[False]:
        assert _bits(outs[False][k], outs[True][k]), (mode, k)
    moved = np.ones(14, dtype=bool)  # (and the tick is the right one: everything moved, the stuck instances by the fallback)
    x0 = S["wl"]["x0"]
    _assert_step(outs[False]["x_out"], Ap, Bp, dp, x0, outs[False]["u_out"], S["w_seq"][0], moved, "misaligned " + mode)


# ---- 6: images no other GPU test lays out ----
COMBOS = {
    # shared other-plant x dense per-instance estimator x backup plans x given w (and a fallback: the stuck instances move too)
    "est": dict(mode="est", backup=1, dense=True, per=True, shared=True, fallback=True),
    # observer with per-instance gains x Ld x backup plans x a plant of its own x w x v
    "obs": dict(mode="obs", backup=1, per=True, with_Ld=True),
}


@pytest.mark.parametrize("combo,noise", [("est", False), ("obs", False), ("est", True), ("obs", True)])
def test_flag_combinations_of_the_image(oracle, combo, noise):
    """one tick each at (5, 2, 2), batch 13, N = 2; with noise drawn on the device on top of the given w (and v)"""
    kw = dict(COMBOS[combo])
    mode = kw.pop("mode")
    S = scenario(5, 2, 2, 2, 1)
    eng = _engine(S["wl"])
    hist, a = run(eng, S, mode, 1, noise=noise, **kw)
    w_seq = v_seq = None
    if noise:  # what the tick added: given + drawn, in longdouble (see the head of this file)
        w_seq = S["w_seq"][:1].astype(LD) + eng.draw_noise(0).cpu().numpy()[None].astype(LD)
        if mode == "obs":
            v_seq = S["v_seq"][:1].astype(LD) + eng.draw_noise(0, "sensor").cpu().numpy()[None].astype(LD)
        quiet, _ = run(_engine(S["wl"]), S, mode, 1, **kw)
        assert not _bits(quiet["x_hist"], hist["x_hist"])
    check(oracle, S, mode, hist, a, "combination %s%s" % (combo, " noise" if noise else ""), w_seq=w_seq, v_seq=v_seq)


def test_measured_outputs_with_backup_plans(oracle):
    """(5, 2, 2), batch 13: the observer fed y_meas with backup plans on -- the image without a plant, with the age slot.  xhat+ and dhat+
    against reference_observer within Eh and Ed, y_out the measurement, the plant's state untouched, held instances bit for bit"""
    nx, nu, ny = 5, 2, 2
    S = scenario(nx, nu, ny, 2, 1)
    wl = S["wl"]
    eng = _engine(wl)
    eng.set_backup_steps(1)
    eng.set_observer(S["C"], S["Lx"], S["Ld"])
    eng.set_x0(S["xhat0"])
    ym = np.random.default_rng(5).standard_normal((S["batch"], ny))
    eng.solve()
    ref = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], S["xhat0"], wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
    out = _numpy(eng.advance(y_meas=ym, u_out=True, status_out=True, age_out=True, y_out=True, xhat_out=True, d_out=True))
    sh = out["status_out"]
    mixed(sh)
    ok = sh == 0
    assert np.array_equal(sh, ref["status"]) and np.array_equal(out["age_out"], ages_of(sh, False))
    assert _rel(out["u_out"][ok], ref["control"][ok, :nu]) <= RTOL
    assert np.array_equal(eng.plant_state(), wl["x0"]) and _bits(out["y_out"], ym)
    R = reference_observer(wl["A"], wl["B"], wl["d"], S["xhat0"], np.where(ok[:, None], out["u_out"], 0.0), S["C"], S["Lx"], S["Ld"], y_meas=ym)
    for got, want, bound, old, name in ((out["xhat_out"], R["xhat"], R["Eh"], S["xhat0"], "xhat"), (out["d_out"], R["dhat"], R["Ed"], wl["d"], "dhat")):
        err = np.abs(got[ok].astype(LD) - want[ok])
        print("y_meas with backup plans, %s: max err / bound = %.3f" % (name, float((err / bound[ok]).max())))
        assert (err <= bound[ok]).all(), name
        assert _bits(got[~ok], np.ascontiguousarray(old[~ok])), name
    assert _bits(eng.state(), out["xhat_out"]) and _bits(eng.bias(), out["d_out"])
