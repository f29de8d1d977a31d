"""Noise drawn on the device (copra_batch_set_noise; BatchLMPC.set_noise, noise_seek, noise_tick, draw_noise) on the GPU.

Two kinds of check.  The DRAW: with a plant A = 0, B = 0, d = 0 the new state of one tick is the noise term itself -- bit-equal to what
copra_batch_draw_noise writes for that tick and within 1e-13 sigma of tests/noise_ref.py (the bound of that file).  The TICK: a rollout that
draws its noise is bit-equal, in every history, to the same rollout of a fresh controller with noise off that is handed the drawn terms as w_seq /
v_seq -- whatever else is on (disturbance estimator, observer, backup plans, solve_every), on shards of the batch, and next to held instances."""
import numpy as np
import pytest

import noise_ref

pytestmark = pytest.mark.gpu

BATCH = 70
TICKS = 12
SEED = 0x5eed0123456789


def _wl(batch=BATCH, stuck=()):
    from copra_amd import workloads
    wl = workloads.com_preview(batch)
    wl = dict(wl, x0=wl["x0"].copy())
    for b in stuck:
        wl["x0"][b, 3] = 50.0  # far outside the velocity bound: infeasible at every tick (tests/test_closed_loop_gpu.py)
    return wl


def _small(nx, nu, batch=BATCH, N=5):
    """a stable system of any shape with a target and a control cost and a wide control bound"""
    rng = np.random.default_rng(10 * nx + nu)
    A = 0.8 * np.eye(nx) + 0.05 * rng.standard_normal((batch, nx, nx))
    B = rng.standard_normal((batch, nx, nu))
    costs = [dict(kind="target", M=np.eye(nx), p=np.zeros(nx), weights=[1.0] * nx), dict(kind="control", N=np.eye(nu), p=np.zeros(nu), weights=[1e-2] * nu)]
    cstrs = [dict(kind="control_bound", lower=[-50.0] * nu, upper=[50.0] * nu)]
    return dict(A=A, B=B, d=np.zeros((batch, nx)), x0=rng.standard_normal((batch, nx)), N=N, costs=costs, cstrs=cstrs)


def _engine(wl, lo=0, hi=None):
    from copra_amd import BatchLMPC
    hi = wl["x0"].shape[0] if hi is None else hi
    nx, nu = wl["B"].shape[1], wl["B"].shape[2]
    eng = BatchLMPC(nx, nu, wl["N"], hi - lo, wl["costs"], wl["cstrs"])
    eng.set_system(wl["A"][lo:hi], wl["B"][lo:hi], wl["d"][lo:hi], wl["x0"][lo:hi])
    return eng


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    import torch
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _sigmas(rows, batch, per, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 2.0, (batch, rows) if per else (rows,))


OBS_NY = 3


def _observer(eng, nx, ny=OBS_NY, zero_C=False):
    C = np.zeros((ny, nx)) if zero_C else np.eye(nx)[:ny]
    Lx = np.zeros((nx, ny))
    Lx[:ny] = 0.4 * np.eye(ny)
    Lx[nx - ny:] += 0.2 * np.eye(ny)
    eng.set_observer(C, Lx)


# ---- 1: the draw, read directly ----
@pytest.mark.parametrize("nx,nu,ny", [(6, 3, 3), (3, 1, 1), (1, 1, 1)])
@pytest.mark.parametrize("per", [False, True])
def test_direct_read_of_the_draw(nx, nu, ny, per):
    wl = _wl() if nx == 6 else _small(nx, nu)
    zero = (np.zeros((BATCH, nx, nx)), np.zeros((BATCH, nx, nu)), np.zeros((BATCH, nx)))
    sw, sv = _sigmas(nx, BATCH, per, 1), _sigmas(ny, BATCH, per, 2)
    first = 2 ** 32 - BATCH  # the last global index is 2^32 - 1
    eng = _engine(wl)
    eng.set_noise(SEED, process=sw, first_instance=first)
    eng.solve()
    assert (eng.results()["status"] == 0).all()
    for tick in (0, 1):
        assert eng.noise_tick == tick
        out = eng.advance(plant=zero, x_out=True)
        eng.set_x0(wl["x0"])  # (the noise itself is no state to solve from; the counter is left alone)
        drawn = eng.draw_noise(tick, "process")
        assert _same(out["x_out"], drawn), tick
        ref = noise_ref.terms(SEED, first, BATCH, sw, tick, 0)
        err = np.abs(out["x_out"].cpu().numpy() - ref) / sw
        print("nx %d per %d tick %d: max |term - reference| / sigma = %.3g" % (nx, per, tick, err.max()))
        assert (err <= noise_ref.TOL).all()
        eng.solve()
    # the sensor stream: y = C xp+ + v with C = 0
    eng = _engine(wl)
    C, Lx = np.zeros((ny, nx)), np.zeros((nx, ny))
    eng.set_observer(C, Lx)
    eng.set_noise(SEED, process=sw, sensor=sv, first_instance=first)
    eng.noise_seek(2 ** 32 + 5)
    eng.solve()
    out = eng.advance(plant=zero, x_out=True, y_out=True)
    assert _same(out["y_out"], eng.draw_noise(2 ** 32 + 5, "sensor")) and _same(out["x_out"], eng.draw_noise(2 ** 32 + 5, "process"))
    assert (np.abs(out["y_out"].cpu().numpy() - noise_ref.terms(SEED, first, BATCH, sv, 2 ** 32 + 5, 1)) <= noise_ref.TOL * sv).all()
    assert (np.abs(out["x_out"].cpu().numpy() - noise_ref.terms(SEED, first, BATCH, sw, 2 ** 32 + 5, 0)) <= noise_ref.TOL * sw).all()
    assert eng.noise_tick == 2 ** 32 + 6


# ---- 2: replay ----
HIST = dict(plain=("x_hist", "u_hist", "status_hist"), bias=("x_hist", "u_hist", "status_hist", "d_hist"),
            observer=("x_hist", "u_hist", "status_hist", "y_hist", "xhat_hist"))


def _start(wl, mode, backup, lo=0, hi=None):
    eng = _engine(wl, lo, hi)
    nx = wl["B"].shape[1]
    if mode == "bias":
        eng.set_bias_estimator(np.full(nx, 0.3))
    if mode == "observer":
        _observer(eng, nx)
    if backup:
        eng.set_backup_steps(3)
    return eng


def _roll(eng, mode, backup, ticks=TICKS, **kw):
    want = {k: True for k in HIST[mode]}
    return eng.rollout(ticks, solve_every=2 if backup else 1, **want, **kw)


def _drawn(eng, ticks, stream):
    import torch
    return torch.stack([eng.draw_noise(t, stream) for t in range(ticks)])


SW = np.array([0.002, 0.002, 0.002, 0.001, 0.001, 0.001])
SV = np.array([0.001, 0.002, 0.003])


def _noisy_and_replayed(wl, mode, backup, per=False, lo=0, hi=None, first=0, ticks=TICKS, seed=SEED):
    """(histories with device noise, histories of a fresh controller given the drawn terms, the noisy controller)"""
    b = (wl["x0"].shape[0] if hi is None else hi) - lo
    sw = np.ascontiguousarray(np.broadcast_to(SW, (b, 6))) * (1.0 + np.arange(b)[:, None] / b) if per else SW
    sv = np.ascontiguousarray(np.broadcast_to(SV, (b, 3))) * (1.0 + np.arange(b)[:, None] / b) if per else SV
    sensor = sv if mode == "observer" else None
    eng = _start(wl, mode, backup, lo, hi)
    eng.set_noise(seed, process=sw, sensor=sensor, first_instance=first)
    got = _roll(eng, mode, backup, ticks)
    w_seq = _drawn(eng, ticks, "process")
    kw = dict(noise=_drawn(eng, ticks, "sensor")) if mode == "observer" else {}
    ref = _roll(_start(wl, mode, backup, lo, hi), mode, backup, ticks, disturbances=w_seq, **kw)
    return got, ref, eng


@pytest.mark.parametrize("backup", [False, True])
@pytest.mark.parametrize("mode", ["plain", "bias", "observer"])
def test_replay_with_the_drawn_terms(mode, backup):
    wl = _wl()
    for per in (False, True):
        got, ref, eng = _noisy_and_replayed(wl, mode, backup, per)
        for k in HIST[mode]:
            assert _same(got[k], ref[k]), (mode, backup, per, k)
        sh = got["status_hist"].cpu().numpy()
        assert (sh[0] == 0).mean() >= 0.75  # (a run in which everything failed shows nothing)
        quiet = _roll(_start(wl, mode, backup), mode, backup)
        assert not _same(quiet["x_hist"], got["x_hist"])  # ... and so does a run without noise
        assert eng.noise_tick == TICKS  # (the ticks of solve_every without a solve included)


# ---- 3: a given w plus the drawn term ----
def test_given_disturbance_plus_noise():
    import torch
    wl = _wl()
    w = torch.as_tensor(0.01 * np.random.default_rng(5).standard_normal((BATCH, 6)), device="cuda")
    eng = _engine(wl)
    eng.set_noise(SEED, process=SW)
    eng.solve()
    got = eng.advance(disturbance=w, x_out=True)["x_out"]
    ref_eng = _engine(wl)
    ref_eng.solve()
    ref = ref_eng.advance(disturbance=w + eng.draw_noise(0), x_out=True)["x_out"]
    quiet_eng = _engine(wl)
    quiet_eng.solve()
    quiet = quiet_eng.advance(disturbance=w, x_out=True)["x_out"]
    ulp = torch.as_tensor(np.spacing(np.abs(ref.cpu().numpy())), device="cuda")
    print("given w + noise: max error %.3g ulp" % float(((got - ref).abs() / ulp).max()))
    assert bool(((got - ref).abs() <= 4 * ulp).all()) and not _same(got, quiet)


# ---- 4: reproducibility ----
def test_seed_seek_and_tick_counter():
    wl = _wl()
    a, _, _ = _noisy_and_replayed(wl, "plain", False, ticks=6)
    eng = _start(wl, "plain", False)
    eng.set_noise(SEED, process=SW)
    b = _roll(eng, "plain", False, 6)
    other = _start(wl, "plain", False)
    other.set_noise(SEED + 1, process=SW)
    c = _roll(other, "plain", False, 6)
    for k in HIST["plain"]:
        assert _same(a[k], b[k]), k
    assert not _same(a["x_hist"], c["x_hist"])
    # seek: tick 0 of the next run draws tick 5's terms, and the counter goes on from there
    assert eng.noise_tick == 6
    zero = (np.zeros((BATCH, 6, 6)), np.zeros((BATCH, 6, 3)), np.zeros((BATCH, 6)))
    eng.noise_seek(5)
    assert eng.noise_tick == 5
    eng.solve()
    x = eng.advance(plant=zero, x_out=True)["x_out"]
    assert _same(x, eng.draw_noise(5)) and not _same(x, eng.draw_noise(0)) and eng.noise_tick == 6
    # set_x0, set_system and schedule_seek leave the counter alone; set_noise resets it
    eng.set_x0(wl["x0"])
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    assert eng.noise_tick == 6
    eng.set_noise(SEED, process=SW)
    assert eng.noise_tick == 0
    bk = _start(wl, "plain", True)
    bk.set_noise(SEED, process=SW)
    bk.rollout(5, solve_every=2)
    assert bk.noise_tick == 5


# ---- 5: shards ----
@pytest.mark.parametrize("mode", ["plain", "observer"])
def test_shards_draw_the_rows_of_the_full_batch(mode):
    import torch
    wl = _wl()
    full, _, eng = _noisy_and_replayed(wl, mode, False, per=True, ticks=6)
    base = (SW * (1.0 + np.arange(BATCH)[:, None] / BATCH), SV * (1.0 + np.arange(BATCH)[:, None] / BATCH))
    for lo, hi in ((0, 40), (40, 70)):
        sh = _start(wl, mode, False, lo, hi)
        sh.set_noise(SEED, process=base[0][lo:hi], sensor=base[1][lo:hi] if mode == "observer" else None, first_instance=lo)
        for t in (0, 3):
            assert _same(sh.draw_noise(t), eng.draw_noise(t)[lo:hi])
            if mode == "observer":
                assert _same(sh.draw_noise(t, "sensor"), eng.draw_noise(t, "sensor")[lo:hi])
        part = _roll(sh, mode, False, 6)
        for k in HIST[mode]:
            assert _same(part[k], full[k][:, lo:hi].contiguous()), (mode, lo, k)
    torch.cuda.synchronize()


# ---- 6: held instances ----
@pytest.mark.parametrize("mode", ["plain", "bias", "observer"])
def test_held_instances_keep_their_bits(mode):
    stuck = (0, 13, 41, 69)
    wl = _wl(stuck=stuck)
    got, ref, _ = _noisy_and_replayed(wl, mode, False, ticks=5)
    sh = got["status_hist"].cpu().numpy()
    ok = np.ones(BATCH, dtype=bool)
    ok[list(stuck)] = False
    assert (sh[:, ~ok] != 0).all() and (sh[:, ok] == 0).mean() >= 0.75
    xh = got["x_hist"]
    for t in range(1, 6):
        assert _same(xh[t][list(stuck)], xh[0][list(stuck)]), t  # held through every tick, bit for bit
    assert xh[0][list(stuck)].cpu().numpy().tobytes() == np.ascontiguousarray(wl["x0"][list(stuck)]).tobytes()
    for k in HIST[mode]:
        assert _same(got[k], ref[k]), (mode, k)  # the others: the terms they get anyway
    assert not _same(xh[1][1:13], xh[0][1:13])


# ---- 7: errors ----
def test_error_codes():
    import ctypes
    import torch
    from copra_amd import BatchLMPC, _capi
    wl = _wl()
    eng = _engine(wl)
    L, h = eng._lib, eng._h
    out = torch.empty((BATCH, 6), dtype=torch.float64, device="cuda")

    def noise(**kw):
        n = _capi.Noise()
        L.copra_noise_init(ctypes.byref(n))
        for k, v in kw.items():
            setattr(n, k, v.ctypes.data if isinstance(v, np.ndarray) else v)
        return ctypes.byref(n)
    ones6, ones3 = np.ones(6), np.ones(3)
    assert L.copra_batch_set_noise(None, noise(sigma_w=ones6)) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_set_noise(h, noise(sigma_w=np.array([1.0, 1.0, -1e-300, 1.0, 1.0, 1.0]))) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_set_noise(h, noise(sigma_w=np.array([1.0, np.nan, 1.0, 1.0, 1.0, 1.0]))) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_set_noise(h, noise(sigma_w=ones6, first_instance=2 ** 32 - BATCH + 1)) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_set_noise(h, noise(sigma_w=ones6, first_instance=2 ** 64 - 1)) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_set_noise(h, noise(sigma_w=ones6, first_instance=2 ** 32 - BATCH)) == _capi.COPRA_OK
    assert L.copra_batch_draw_noise(h, 0, 2, out.data_ptr(), None) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_draw_noise(h, 0, -1, out.data_ptr(), None) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_draw_noise(h, 0, 0, None, None) == _capi.COPRA_ERR_ARG
    assert L.copra_batch_draw_noise(None, 0, 0, out.data_ptr(), None) == _capi.COPRA_ERR_ARG
    # the observer is off: no sensor noise, no stream 1
    assert L.copra_batch_set_noise(h, noise(sigma_w=ones6, sigma_v=ones3)) == _capi.COPRA_ERR_RUNTIME
    assert L.copra_batch_draw_noise(h, 0, 1, out.data_ptr(), None) == _capi.COPRA_ERR_RUNTIME
    with pytest.raises(_capi.CopraRuntimeError):
        eng.set_noise(1, sensor=ones3)
    # a stream whose sigma is not set
    eng.set_noise(1)
    assert L.copra_batch_draw_noise(h, 0, 0, out.data_ptr(), None) == _capi.COPRA_ERR_RUNTIME
    _observer(eng, 6)
    eng.set_noise(1, sensor=ones3)
    with pytest.raises(_capi.CopraRuntimeError):
        eng.draw_noise(0, "process")
    assert eng.draw_noise(0, "sensor").shape == (BATCH, 3)
    with pytest.raises(ValueError):
        eng.draw_noise(0, "other")
    # the observer off drops the sensor noise; on again with another ny asks for a new set_noise
    eng.set_observer(None)
    eng.solve()
    eng.advance()
    assert L.copra_batch_draw_noise(h, 0, 1, out.data_ptr(), None) == _capi.COPRA_ERR_RUNTIME
    with pytest.raises(_capi.CopraRuntimeError):
        _observer(eng, 6, ny=2)
    _observer(eng, 6)  # (the same ny: the sensor noise is back)
    assert eng.draw_noise(0, "sensor").shape == (BATCH, 3)
    eng.set_observer(None)
    eng.set_noise(1)
    _observer(eng, 6, ny=2)
    eng.set_noise(1, process=ones6, sensor=np.ones(2))
    # an InitialStateLMPC controller
    pb = __import__("fixtures").bounded_system("trajectory", N=12)
    ise = BatchLMPC(2, 1, 12, 4, pb["costs"], pb["cstrs"], initial_state=dict(R=1e-2 * np.eye(2), r=np.zeros(2)))
    with pytest.raises(_capi.CopraUnsupported):
        ise.set_noise(1, process=np.ones(2))
    with pytest.raises(_capi.CopraUnsupported):
        ise.noise_seek(1)
    assert L.copra_batch_draw_noise(ise._h, 0, 0, out.data_ptr(), None) == _capi.COPRA_ERR_UNSUPPORTED
    torch.cuda.synchronize()


# ---- 8: never set == set and ended ----
@pytest.mark.parametrize("mode", ["plain", "bias", "observer"])
def test_noise_ended_is_noise_never_set(mode):
    wl = _wl()
    never = _start(wl, mode, False)
    ended = _start(wl, mode, False)
    ended.set_noise(SEED, process=SW, sensor=SV if mode == "observer" else None)
    ended.set_noise(SEED)
    assert ended.noise_tick == 0
    for eng in (never, ended):
        eng.solve()
    a, b = never.advance(x_out=True, u_out=True), ended.advance(x_out=True, u_out=True)
    assert _same(a["x_out"], b["x_out"]) and _same(a["u_out"], b["u_out"])
    ra, rb = _roll(never, mode, False, 4), _roll(ended, mode, False, 4)
    for k in HIST[mode]:
        assert _same(ra[k], rb[k]), (mode, k)
    assert never.noise_tick == ended.noise_tick == 5
