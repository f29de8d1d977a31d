"""Input delay in the tick on the device (copra_batch_set_input_delay; BatchLMPC.set_input_delay, delay_state, delay_queue) against
tests/delay_ref.py, tick by tick, at the smallest shapes at which the launch can go wrong.

Every tick is driven as solve() / results() / advance(): the reference gets the DEVICE's own controls and statuses and starts every tick from
the device's own xnow, so nothing compounds and no solver tolerance enters.  Measures, after every tick:
  u_out, status_out, age_out, the queue and its statuses, a held instance's xnow        exact (bit for bit, NaN where NaN)
  x_out = xnow of an instance that moved     within step_bound of tests/test_closed_loop_abi.py (the plant step's own, unchanged)
  x0, the prediction                         within delay_ref's running bound of the same walk in numpy.longdouble
The controller of a shape is the cheapest there is, as in tests/test_tick_edges_gpu.py: the last state is decoupled (x+ = x / 2 + 0.01)
and bounded above, so a kick w on it makes the NEXT solve infeasible and a second kick brings the instance back: one failed entry then
travels through the ring -- newest, middle, head -- and is held or replaced by fallback_u when it reaches the plant."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import delay_ref
from launch_edge_cases import largest_nx
from test_bias_estimator_abi import reference_bias
from test_closed_loop_abi import reference_step, step_bound
from test_closed_loop_gpu import ABS_FLOOR, RTOL, _engine, _rel
from test_observer_abi import reference_observer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FALLBACK, HELD = delay_ref.FALLBACK, delay_ref.HELD
V_MAX = 0.6


@pytest.fixture(scope="module")
def geo(tmp_path_factory):
    """the launch geometry of delay_step.hpp (and of plant_step.hpp beside it), through the emulator's exports"""
    so = str(tmp_path_factory.mktemp("emu_delay_geometry") / "libemu_delay.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "emu", "emu_delay.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.emu_delay_image_bytes.restype, lib.emu_delay_image_bytes.argtypes = ctypes.c_longlong, [ctypes.c_int] * 3
    lib.emu_delay_launch_group.restype, lib.emu_delay_launch_group.argtypes = ctypes.c_int, [ctypes.c_int] * 3
    lib.emu_plant_image_bytes.restype, lib.emu_plant_image_bytes.argtypes = ctypes.c_longlong, [ctypes.c_int] * 5
    lib.emu_plant_lds_max.restype = ctypes.c_longlong
    return lib


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same(a, b):
    """equal, NaN where NaN (copied doubles whose NaN payload is not part of the contract)"""
    return np.array_equal(a, b, equal_nan=True)


def _np(t):
    return None if t is None else t.cpu().numpy()


def case(nx, nu, batch, N, D, ticks, seed=1, stuck=None, kicked=None):
    """dict(wl, plant, w_seq, fb, u_init, stuck, kicked): every matrix in natural indexing.  stuck instances fail at every tick; a kicked
    instance fails at the solves of ticks 2 and D + 4 alone"""
    rng = np.random.default_rng(1000 * nx + 10 * nu + 7 * D + seed)
    j = nx - 1
    stuck = ((1,) if batch >= 5 else ()) if stuck is None else stuck
    kicked = ((0,) if batch < 5 else (0, 3)) if kicked is None else kicked
    A = 0.5 * rng.standard_normal((batch, nx, nx)) / np.sqrt(nx)
    B = rng.standard_normal((batch, nx, nu))
    d = 0.1 * rng.standard_normal((batch, nx))
    x0 = rng.standard_normal((batch, nx))
    x0[:, j] = rng.uniform(-0.2, 0.2, batch)
    x0[list(stuck), j] = 1e9  # (halved every tick: above the bound, and so is its prediction, for more ticks than any test here runs)
    Ap, Bp, dp = A * (1.0 - 0.02 * rng.uniform(0.0, 1.0, A.shape)), 0.95 * B, d + 0.01 * rng.standard_normal((batch, nx))
    for M in (A, Ap):
        M[:, j, :] = 0.0
        M[:, j, j] = 0.5
    B[:, j], Bp[:, j], d[:, j], dp[:, j] = 0.0, 0.0, 0.01, 0.01
    w_seq = 0.01 * rng.standard_normal((ticks, batch, nx))
    w_seq[:, :, j] = 0.0
    kick = 4.0 * 2.0 ** D  # (the prediction halves it D times: still above the bound)
    for t in (1, D + 3):
        if t + 1 < ticks:
            w_seq[t, list(kicked), j] += kick
            w_seq[t + 1, list(kicked), j] -= kick
    inf = np.inf
    costs = [dict(kind="target", M=rng.standard_normal((1, nx)) / np.sqrt(nx), p=[0.3], weights=[1.0]),
             dict(kind="control", N=np.eye(nu), p=np.zeros(nu), weights=[0.5] * nu)]
    cstrs = [dict(kind="trajectory_bound", lower=[-inf] * nx, upper=[inf] * (nx - 1) + [V_MAX]), dict(kind="control_bound", lower=[-1e3] * nu, upper=[1e3] * nu)]
    return dict(wl=dict(A=A, B=B, d=d, x0=x0, N=N, costs=costs, cstrs=cstrs), plant=(Ap, Bp, dp), w_seq=w_seq, fb=0.1 * rng.standard_normal((batch, nu)),
                u_init=0.1 * rng.standard_normal((batch, nu)), stuck=stuck, kicked=kicked, D=D, ticks=ticks, nx=nx, nu=nu, batch=batch)


def check_step(x_next, plant, x, u, w, moved, what):
    """the plant step of the instances that moved within step_bound, the others bit for bit; returns the exact step and its scale"""
    A, B, d = delay_ref.model_of(*plant, batch=x.shape[0])
    ref, S = reference_step(A, B, d, x, np.where(moved[:, None], u, 0.0), w)
    err = np.abs(x_next.astype(np.longdouble) - ref)
    bound = step_bound(B.shape[-2], B.shape[-1], S)
    assert (err[moved] <= bound[moved]).all(), (what, float((err[moved] / np.maximum(bound[moved], 1e-300)).max()))
    assert _bits(x_next[~moved], x[~moved]), what
    return ref, S


def check_prediction(eng, model, loop, fb, what, worst):
    """x0 against the walk over the device's own xnow and queue in longdouble, within the running bound"""
    got, xnow = eng.state(), eng.delay_state()
    q, qs = eng.delay_queue()
    assert _same(q, loop.q) and np.array_equal(qs, loop.qs), what
    want, err = delay_ref.predict_exact(model, xnow, q, qs, fb)
    e = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
    assert np.isfinite(got).all() and (e <= err).all(), (what, float((e / np.maximum(err, 1e-300)).max()))
    if fb is None:  # nothing but held entries: the prediction is the state itself
        all_failed = (qs != 0).all(axis=1)
        assert _bits(got[all_failed], xnow[all_failed]), what
    return max(worst, float((e / np.maximum(err, 1e-300)).max()))


def drive(eng, c, model, plant=None, with_fb=False, ticks=None, loop=None, shared_plant=False, fb_tensor=None):
    """2 D + 3 ticks of solve / advance with delay on; every output of every tick against delay_ref.  Returns (the loop, what was seen)"""
    import torch
    D, nu = c["D"], c["nu"]
    ticks = c["ticks"] if ticks is None else ticks
    fb = c["fb"] if with_fb else None
    fbd = None if fb is None else torch.from_numpy(np.ascontiguousarray(fb)).cuda() if fb_tensor is None else fb_tensor
    loop = delay_ref.DelayLoop(D, eng.delay_state(), nu, c["u_init"]) if loop is None else loop
    the_plant = model if plant is None else plant
    worst = check_prediction(eng, model, loop, None, "the setter's prediction", 0.0)
    seen = dict(held=0, fallback=0, failed_at=set(), worst=0.0)
    for t in range(ticks):
        what = "tick %d" % t
        eng.solve()
        res = eng.results()
        xnow = eng.delay_state()
        loop.xnow = xnow.copy()
        o = eng.advance(plant=plant, shared=shared_plant, disturbance=torch.from_numpy(c["w_seq"][t]).cuda(), fallback_control=fbd, x_out=True, u_out=True,
                        status_out=True, age_out=True)
        x_out, u_out, s_out, a_out = (_np(o[k]) for k in ("x_out", "u_out", "status_out", "age_out"))
        _, want_u, want_s, want_a = loop.tick(the_plant, model, res["control"], res["status"], fb, c["w_seq"][t])
        assert _same(u_out, want_u) and np.array_equal(s_out, want_s) and np.array_equal(a_out, want_a), what
        moved = a_out != HELD
        check_step(x_out, the_plant, xnow, u_out, c["w_seq"][t], moved, what)
        assert _bits(eng.delay_state(), x_out), what
        loop.xnow = x_out.copy()
        worst = check_prediction(eng, model, loop, fb, what, worst)
        seen["held"] += int((a_out == HELD).sum())
        seen["fallback"] += int((a_out == FALLBACK).sum())
        for b in c["kicked"]:
            seen["failed_at"] |= set(np.nonzero(loop.qs[b] != 0)[0].tolist())
    seen["worst"] = worst
    print("largest prediction error / running bound %.3g; held %d, fallback %d, failed entries seen at %s" % (worst, seen["held"], seen["fallback"], sorted(seen["failed_at"])))
    return loop, seen


def start(c, D=None, shared=False, u_init="given"):
    eng = _engine(c["wl"], shared_model=shared)
    eng.set_input_delay(c["D"] if D is None else D, c["u_init"] if isinstance(u_init, str) else u_init)
    return eng


def model_of(c, shared=False):
    wl = c["wl"]
    return (wl["A"][0], wl["B"][0], wl["d"][0]) if shared else (wl["A"], wl["B"], wl["d"])


def coverage(c, seen, with_fb):
    """the conditions that the run went through every branch"""
    D = c["D"]
    assert seen["failed_at"] == set(range(D)), seen  # a kicked instance's failed entry was seen as the newest, in the middle and at the head
    if with_fb:
        assert seen["fallback"] > 0 and seen["held"] == 0
    else:
        assert seen["held"] > 0 and seen["fallback"] == 0


# ---- the launch edges ----
EDGES = [("batch 1", 6, 3, 1, 5, 1), ("batch 5, a partial group", 6, 3, 5, 5, 3), ("odd sizes (3, 1)", 3, 1, 13, 4, 8), ("D = 8 at (6, 3)", 6, 3, 13, 5, 8)]


@pytest.mark.parametrize("with_fb", [False, True])
@pytest.mark.parametrize("name,nx,nu,batch,N,D", EDGES, ids=[e[0] for e in EDGES])
def test_every_tick_against_the_rule(name, nx, nu, batch, N, D, with_fb):
    c = case(nx, nu, batch, N, D, 2 * D + 3)
    eng = start(c)
    assert eng.delay_state_ptr() != 0 and _bits(eng.delay_state(), c["wl"]["x0"])
    _, seen = drive(eng, c, model_of(c), plant=c["plant"], with_fb=with_fb)
    coverage(c, seen, with_fb)


@pytest.mark.parametrize("with_fb", [False, True])
def test_arrays_that_are_8_but_not_16_bytes_aligned(with_fb):
    """(6, 3): A, B, d, x0, u_init and the fallback controls handed over as device tensors one double off a 16-byte boundary"""
    import torch
    c = case(6, 3, 13, 5, 3, 9)
    wl = c["wl"]

    def off(a):
        a = np.ascontiguousarray(a)
        room = torch.zeros(a.size + 1, dtype=torch.float64, device="cuda")
        view = room[1:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 16 == 8
        return view
    from copra_amd import BatchLMPC
    eng = BatchLMPC(6, 3, wl["N"], 13, wl["costs"], wl["cstrs"])
    keep = [off(np.swapaxes(wl["A"], -1, -2)), off(np.swapaxes(wl["B"], -1, -2)), off(wl["d"]), off(wl["x0"]), off(c["u_init"]), off(c["fb"])]
    eng.set_system(*keep[:4])
    eng.set_input_delay(3, keep[4])
    _, seen = drive(eng, c, model_of(c), with_fb=with_fb, fb_tensor=keep[5])
    coverage(c, seen, with_fb)
    assert _bits(keep[3].cpu().numpy(), wl["x0"])  # (a caller's buffer is read, never written)


def test_one_instance_per_workgroup_and_an_image_above_48_kib(geo):
    """the largest nx whose image the geometry admits: the group is 1, every copy the scalar loop, the dynamic LDS is opted into"""
    from copra_amd import _capi
    D, nu, top = 1, 1, geo.emu_plant_lds_max()
    fits = lambda n: geo.emu_delay_image_bytes(n, nu, D) <= top and geo.emu_plant_image_bytes(0, n, nu, 0, 0) <= top  # noqa: E731
    nx = largest_nx(144, fits, "group 1")
    for n in range(nx, 40, -1):
        c = case(n, nu, 5, 1, D, 2 * D + 3)
        try:
            eng = start(c)
            eng.solve()
        except _capi.CopraUnsupported as e:
            print("nx %d refused (%s)" % (n, e))
            continue
        break
    assert geo.emu_delay_launch_group(n, nu, D) == 1 and geo.emu_delay_image_bytes(n, nu, D) > 48 * 1024
    print("group 1 at nx %d: image %d bytes" % (n, geo.emu_delay_image_bytes(n, nu, D)))
    _, seen = drive(eng, c, model_of(c), plant=c["plant"])
    coverage(c, seen, False)


@pytest.mark.parametrize("with_fb", [False, True])
def test_batch_257_with_the_shared_model(with_fb):
    c = case(6, 3, 257, 5, 3, 9, stuck=(1, 200), kicked=(0, 3, 256))
    eng = start(c, shared=True)
    one = tuple(m[0] for m in c["plant"])
    _, seen = drive(eng, c, model_of(c, shared=True), plant=one, shared_plant=True, with_fb=with_fb)
    coverage(c, seen, with_fb)


# ---- the property that makes this a predictor ----
def test_the_prediction_is_the_state_the_plant_reaches(oracle):
    """plant = model, no w, no failures, D = 2: the x0 the solve of tick t read lies within the running bound of the x_out of tick t + D - 1,
    and the applied controls are those of a delay-free handle started from the state reached under u_init, shifted by D ticks"""
    from copra_amd import workloads
    D, T, batch = 2, 6, 64
    wl = workloads.com_preview(batch)
    nu = wl["B"].shape[2]
    model = (wl["A"], wl["B"], wl["d"])
    u_init = 0.05 * np.random.default_rng(3).standard_normal((batch, nu))
    eng = _engine(wl)
    eng.set_input_delay(D, u_init)
    read, errs, x_out, u_out = [], [], [], []
    for t in range(T + D):
        q, qs = eng.delay_queue()
        read.append(eng.state())
        errs.append(delay_ref.predict_exact(model, eng.delay_state(), q, qs)[1])
        eng.solve()
        assert (eng.results()["status"] == 0).all()
        o = eng.advance(x_out=True, u_out=True)
        x_out.append(_np(o["x_out"])), u_out.append(_np(o["u_out"]))
    worst = 0.0
    for t in range(T + 1):
        e = np.abs(read[t] - x_out[t + D - 1])
        assert (e <= errs[t]).all(), (t, float((e / np.maximum(errs[t], 1e-300)).max()))
        worst = max(worst, float((e / np.maximum(errs[t], 1e-300)).max()))
    print("prediction against the state reached: largest error / running bound %.3g" % worst)
    assert all(_bits(u_out[t], u_init) for t in range(D))
    # the delay-free twin from the state reached under u_init; its spread against the CPU oracle from its own states is the parity rule's
    twin = _engine(dict(wl, x0=x_out[D - 1]))
    spread = 0.0
    for t in range(T):
        xt = twin.state()
        twin.solve()
        ref = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], xt, wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
        near = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], xt * (1.0 + 1e-9), wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
        # (no instance at an active-set tie, on the reference alone: the same iterations from a state 1e-9 away)
        assert (ref["status"] == 0).all() and np.array_equal(ref["iter"], near["iter"]), t
        u = _np(twin.advance(u_out=True)["u_out"])
        spread = max(spread, _rel(u, ref["control"][:, :nu]))
        e = _rel(u_out[t + D], u)
        print("tick %d: delayed loop against the delay-free twin %.2e, twin against the oracle %.2e" % (t, e, spread))
        assert spread <= RTOL and e <= RTOL, t
    assert ABS_FLOOR == 1e-3 and RTOL == 1e-6  # (entry-wise 1e-6 with the floor 1e-3)


# ---- composition ----
def test_estimator_and_delay():
    """a constant load: dhat converges, the estimator sees the APPLIED control, and the prediction uses the updated dhat of the same tick"""
    import torch
    c = case(6, 3, 13, 5, 2, 14, stuck=(), kicked=())
    wl = c["wl"]
    load = 0.05 * np.random.default_rng(2).standard_normal((13, 6))
    plant = (wl["A"], wl["B"], wl["d"] + load)
    gain = np.full(6, 0.5)
    eng = _engine(wl)
    eng.set_bias_estimator(gain)
    eng.set_input_delay(2, c["u_init"])
    loop = delay_ref.DelayLoop(2, wl["x0"], 3, c["u_init"])
    worst = 0.0
    for t in range(14):
        eng.solve()
        res = eng.results()
        xnow, dhat = eng.delay_state(), eng.bias()
        loop.xnow = xnow.copy()
        o = eng.advance(plant=plant, x_out=True, u_out=True, d_out=True)
        x_out, u_out, d_out = (_np(o[k]) for k in ("x_out", "u_out", "d_out"))
        m_before = (wl["A"], wl["B"], dhat)
        _, want_u, _, _ = loop.tick(plant, m_before, res["control"], res["status"])
        assert _same(u_out, want_u) and (res["status"] == 0).all(), t
        xp, Sx = check_step(x_out, plant, xnow, u_out, None, np.ones(13, dtype=bool), "tick %d" % t)
        dref, dbound = reference_bias(wl["A"], wl["B"], dhat, xnow, u_out, xp, Sx, gain, False)
        assert (np.abs(d_out - dref) <= dbound).all() and _bits(eng.bias(), d_out), t
        loop.xnow = x_out.copy()
        worst = check_prediction(eng, (wl["A"], wl["B"], d_out), loop, None, "tick %d" % t, worst)
        if t == 0:  # the prediction with the dhat of BEFORE the tick is another one: the bound tells them apart
            old, err = delay_ref.predict_exact(m_before, x_out, loop.q, loop.qs)
            assert (np.abs(eng.state() - old) > err).any()
    assert np.abs(eng.bias() - plant[2]).max() <= 1e-3 * np.abs(load).max()  # (gain 1/2: the error halves every tick)
    torch.cuda.synchronize()


def test_observer_and_delay_with_a_y_meas_tick():
    """C = I, Lx = 0.7 I: xnow is the estimate, the plant keeps its own state; then one tick of a real plant (y_meas)"""
    import torch
    c = case(6, 3, 13, 5, 2, 6, stuck=(), kicked=())
    wl = c["wl"]
    C, Lx = np.eye(6), 0.7 * np.eye(6)
    rng = np.random.default_rng(4)
    xhat0 = wl["x0"] + 0.05 * rng.standard_normal((13, 6))
    eng = _engine(wl)
    eng.set_input_delay(2, c["u_init"])
    eng.set_observer(C, Lx)  # (delay already on: the plant's own state starts from xnow, not from the prediction)
    eng.set_x0(xhat0)
    assert _bits(eng.delay_state(), xhat0) and _bits(eng.plant_state(), wl["x0"])
    loop = delay_ref.DelayLoop(2, xhat0, 3, c["u_init"])
    model = model_of(c)
    worst = 0.0
    for t in range(6):
        eng.solve()
        res = eng.results()
        xhat, xp = eng.delay_state(), eng.plant_state()
        meas = t == 5
        v = 1e-3 * rng.standard_normal((13, 6))
        y = xp + v
        kw = dict(y_meas=torch.from_numpy(y).cuda()) if meas else dict(plant=c["plant"], disturbance=torch.from_numpy(c["w_seq"][t]).cuda(),
                                                                        noise=torch.from_numpy(v).cuda(), x_out=True)
        o = eng.advance(u_out=True, xhat_out=True, y_out=True, **kw)
        u_out, xhat_out = _np(o["u_out"]), _np(o["xhat_out"])
        loop.xnow = xhat.copy()
        _, want_u, _, _ = loop.tick(model, model, res["control"], res["status"])
        assert _same(u_out, want_u) and (res["status"] == 0).all(), t
        if meas:
            R = reference_observer(wl["A"], wl["B"], wl["d"], xhat, u_out, C, Lx, y_meas=y)
            assert _bits(eng.plant_state(), xp)
        else:
            xplus, Sx = check_step(_np(o["x_out"]), c["plant"], xp, u_out, c["w_seq"][t], np.ones(13, dtype=bool), "tick %d" % t)
            assert _bits(eng.plant_state(), _np(o["x_out"]))
            R = reference_observer(wl["A"], wl["B"], wl["d"], xhat, u_out, C, Lx, xplus=xplus, Sx=Sx, v=v)
        assert (np.abs(xhat_out - R["xhat"]) <= R["Eh"]).all(), t
        assert _bits(eng.delay_state(), xhat_out), t
        loop.xnow = xhat_out.copy()
        worst = check_prediction(eng, model, loop, None, "tick %d" % t, worst)


def test_noise_and_delay_draw_what_draw_noise_writes():
    """the same seed: the x_out of a delayed loop that draws its process noise is the x_out of its twin fed the copra_batch_draw_noise
    arrays (4 ulp, the measure of tests/test_noise_gpu.py); the twin starts every tick from the first loop's state"""
    c = case(6, 3, 13, 5, 2, 5, stuck=(), kicked=())
    sw = np.where(np.arange(6) == 5, 0.0, 0.01) * np.ones((13, 6))
    eng, twin = start(c), start(c)
    eng.set_noise(0x5eed, process=sw)
    for t in range(5):
        twin.set_x0(eng.delay_state())  # (keeps the queue, predicts again)
        assert _bits(twin.state(), eng.state()) and _same(twin.delay_queue()[0], eng.delay_queue()[0]), t
        eng.solve(), twin.solve()
        assert eng.noise_tick == t
        w = eng.draw_noise(t)
        got = _np(eng.advance(x_out=True)["x_out"])
        ref = _np(twin.advance(disturbance=w, x_out=True)["x_out"])
        assert (np.abs(got - ref) <= 4 * np.spacing(np.abs(ref))).all() and np.abs(_np(w)).max() > 0, t


def test_score_rollout_histories_and_a_schedule_with_offset_plus_d():
    """one rollout with every history: x_hist[0] is xnow, the records are against xnow (x_hist), u_hist / age_hist / status_hist describe the
    command that reached the plant, and the reference window of a cost scheduled with offset + D shows the rows of time t + D"""
    import score_ref
    from launch_edge_cases import measure
    from test_score_gpu import _compare, _replay, _set
    D, T = 2, 7
    c = case(6, 3, 13, 5, D, T)
    wl = c["wl"]
    eng = start(c)
    m = measure(6, 3, steps=3, seed=5)
    _set(eng, m)
    steps = T + wl["N"] + D + 2
    sched = 0.3 + 0.01 * np.arange(steps, dtype=np.float64)[:, None]
    eng.set_reference_schedule(0, sched, 1, offset=wl["N"] + D)
    xnow0 = eng.delay_state()
    hist = {k: _np(v) for k, v in eng.rollout(T, plant=c["plant"], disturbances=c["w_seq"], x_hist=True, u_hist=True, status_hist=True, age_hist=True).items()
            if v is not None}
    assert _bits(hist["x_hist"][0], xnow0) and _bits(hist["x_hist"][-1], eng.delay_state())
    assert all(_bits(hist["u_hist"][t], c["u_init"]) for t in range(D)) and (hist["status_hist"][:D] == 0).all()
    assert (hist["status_hist"][D:, list(c["stuck"])] != 0).all() and (hist["age_hist"][D:, list(c["stuck"])] == HELD).all()
    for t in range(T):
        moved = hist["age_hist"][t] != HELD
        check_step(hist["x_hist"][t + 1], c["plant"], hist["x_hist"][t], hist["u_hist"][t], c["w_seq"][t], moved, "tick %d" % t)
    want, S = _replay(hist, m)
    _compare(eng.score(), want, S, T, "score with delay")
    assert score_ref is not None and eng.schedule_tick() == T
    assert _bits(eng.cost_reference(0), np.broadcast_to(sched[min(T + wl["N"] + D, steps - 1)], (13, 1)))


def test_setters_mid_run_predict_again_and_keep_the_queue():
    """set_x0, set_bias and set_system keep the queue, move xnow / d / the model and predict again; the setter called again resets the queue
    and keeps xnow; D = 0 makes xnow the x0 again and the next ticks are those of a handle that never had delay, bit for bit"""
    c = case(6, 3, 13, 5, 3, 9, stuck=(), kicked=())
    wl = c["wl"]
    eng = start(c)
    loop, _ = drive(eng, c, model_of(c), ticks=4)
    rng = np.random.default_rng(9)
    model = model_of(c)
    # set_x0
    xnew = wl["x0"] + 0.1 * rng.standard_normal((13, 6))
    eng.set_x0(xnew)
    loop.xnow = xnew.copy()
    assert _bits(eng.delay_state(), xnew)
    check_prediction(eng, model, loop, None, "set_x0", 0.0)
    # set_bias (the library's estimates become d with the estimator)
    eng.set_bias_estimator(np.full(6, 0.25))
    dnew = wl["d"] + 0.02 * rng.standard_normal((13, 6))
    eng.set_bias(dnew)
    model = (wl["A"], wl["B"], dnew)
    check_prediction(eng, model, loop, None, "set_bias", 0.0)
    eng.set_bias_estimator(None)
    # set_system
    A2 = wl["A"] * 0.9
    x2 = xnew + 0.05
    eng.set_system(A2, wl["B"], wl["d"], x2)
    model = (A2, wl["B"], wl["d"])
    loop.xnow = x2.copy()
    assert _bits(eng.delay_state(), x2)
    check_prediction(eng, model, loop, None, "set_system", 0.0)
    # the setter again: the queue is reset, xnow stays
    u2 = 0.2 * rng.standard_normal((13, 3))
    eng.set_input_delay(3, u2)
    loop.reset(3, u2)
    assert _bits(eng.delay_state(), x2)
    check_prediction(eng, model, loop, None, "the setter again", 0.0)
    c2 = dict(c, wl=dict(wl, A=A2), u_init=u2)
    drive(eng, c2, model, ticks=2, loop=loop)
    # off: the ABI-15 tick from xnow
    xnow = eng.delay_state()
    eng.set_input_delay(0)
    assert eng.delay_state_ptr() == 0 and _bits(eng.state(), xnow)
    twin = _engine(dict(wl, A=A2, x0=xnow))
    for t in range(3):
        eng.solve(), twin.solve()
        a, b = eng.advance(x_out=True, u_out=True, age_out=True), twin.advance(x_out=True, u_out=True, age_out=True)
        for k in ("x_out", "u_out", "age_out"):
            assert _bits(_np(a[k]), _np(b[k])), (t, k)
        assert _bits(eng.state(), twin.state())


def test_a_handle_that_never_enabled_delay_runs_the_plant_steps_formula():
    """D = 0 of delay_ref is the plant step of ABI 15: u_out, status_out and age_out exact, x_out within step_bound, the state is x_out"""
    import torch
    c = case(6, 3, 13, 5, 0, 4)
    eng = _engine(c["wl"])
    assert eng.delay_state_ptr() == 0
    loop = delay_ref.DelayLoop(0, c["wl"]["x0"], 3)
    model = model_of(c)
    for t in range(4):
        x = eng.state()
        eng.solve()
        res = eng.results()
        o = eng.advance(plant=c["plant"], disturbance=torch.from_numpy(c["w_seq"][t]).cuda(), x_out=True, u_out=True, status_out=True, age_out=True)
        loop.xnow = x.copy()
        _, want_u, want_s, want_a = loop.tick(c["plant"], model, res["control"], res["status"], None, c["w_seq"][t])
        assert _same(_np(o["u_out"]), want_u) and np.array_equal(_np(o["status_out"]), want_s) and np.array_equal(_np(o["age_out"]), want_a), t
        check_step(_np(o["x_out"]), c["plant"], x, _np(o["u_out"]), c["w_seq"][t], want_a != HELD, "tick %d" % t)
        assert _bits(eng.state(), _np(o["x_out"]))
    assert (want_a[list(c["stuck"])] == HELD).all()


def test_errors_and_the_two_exclusions():
    from copra_amd import BatchLMPC, _capi
    c = case(6, 3, 13, 5, 2, 5)
    wl = c["wl"]
    eng = BatchLMPC(6, 3, wl["N"], 13, wl["costs"], wl["cstrs"])
    with pytest.raises(_capi.CopraRuntimeError):
        eng.set_input_delay(2)  # no system, no x0
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    for bad in (-1, 9):
        with pytest.raises(Exception) as e:
            eng.set_input_delay(bad)
        assert "outside" in str(e.value)
    for getter in (eng.delay_state, eng.delay_queue):
        with pytest.raises(_capi.CopraRuntimeError):
            getter()
    # backup plans first, then delay
    eng.set_backup_steps(2)
    with pytest.raises(_capi.CopraRuntimeError):
        eng.set_input_delay(2)
    eng.set_backup_steps(0)
    # delay first, then backup plans and solve_every
    eng.set_input_delay(2)
    with pytest.raises(_capi.CopraRuntimeError):
        eng.set_backup_steps(2)
    with pytest.raises(_capi.CopraRuntimeError):
        eng.rollout(4, solve_every=2)
    eng.rollout(2)  # (and the loop still runs)
    assert np.isfinite(eng.state()).all()
    # one model for the batch keeps delay on: the prediction is formed again, from the one system
    eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
    q, qs = eng.delay_queue()
    want, err = delay_ref.predict_exact((wl["A"][0], wl["B"][0], wl["d"][0]), eng.delay_state(), q, qs)
    assert (np.abs(eng.state() - want) <= err).all() and eng.delay_state_ptr() != 0
    own, _ = delay_ref.predict_exact(model_of(c), eng.delay_state(), q, qs)
    assert (np.abs(eng.state() - own) > err).any()  # (the instances' own systems give another prediction: the bound tells them apart)
