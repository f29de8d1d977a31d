"""Noise drawn on the device (copra_batch_set_noise, ABI 13) without a GPU: declared, exported, bound -- and the generator and the tick's rule
on the phase bodies of all three builds of the plant-step kernel (copra_amd/csrc/plant_step.hpp, plant_noise.hpp), which compile on the host:
tests/emu/emu_plant_noise.cpp walks them thread by thread over a NaN-filled image, this file compiles that harness itself.

The expectation for the generator is tests/noise_ref.py: the 32-bit words are exact, the terms within 1e-13 sigma (ten times what 2 ulp in log,
sin and cos can give at |rad| <= 8.5).  The tick's rule is checked bit for bit: a walk that draws its noise equals the same walk given the
drawn terms as explicit w / v, whatever the group; a walk without noise equals the emulators of the earlier ABIs."""
import ctypes
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import noise_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
NEW = ("copra_noise_init", "copra_batch_set_noise", "copra_batch_noise_seek", "copra_batch_noise_tick", "copra_batch_draw_noise")
FIELDS = ["struct_size", "seed", "first_instance", "sigma_w", "sigma_v", "per_instance", "on_device"]
SHAPES = [(6, 3, 3), (3, 1, 1), (1, 1, 1), (5, 2, 2)]  # (nx, nu, ny)
BATCH, GROUP = 5, 4  # a partial last group
BUILDS = (0, 1, 2)  # the plain tick, the disturbance estimator, the observer
VP, CI, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulonglong


def _lib():
    from copra_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_capi.LIB_PATH)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- surface ----
def test_header_declares_the_noise():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    end = code.index("} copra_noise_t;")
    body = code[code.rindex("typedef struct {", 0, end):end]
    assert re.findall(r"(\w+)\s*;", body) == FIELDS
    assert re.search(r"unsigned\s+long\s+long\s+seed\s*;", body) and re.search(r"unsigned\s+long\s+long\s+first_instance\s*;", body)
    assert re.search(r"copra_batch_draw_noise\s*\(\s*copra_batch_t\s*\*\s*\w*\s*,\s*unsigned\s+long\s+long\s+tick\s*,\s*int\s+stream\s*,\s*double\s*\*\s*out_device\s*,"
                     r"\s*void\s*\*\s*hip_stream\s*\)", code)
    assert "Philox4x32-10" in text and "first_instance + batch <= 2^32" in text


def test_library_exports_the_noise_with_abi_13():
    lib = _lib()
    for name in NEW:
        assert hasattr(lib, name), name
    lib.copra_abi_version.restype = ctypes.c_int
    assert lib.copra_abi_version() >= 13
    from copra_amd import _capi
    lib.copra_batch_set_noise.restype = CI
    lib.copra_batch_set_noise.argtypes = [VP, VP]
    lib.copra_batch_noise_seek.restype = CI
    lib.copra_batch_noise_seek.argtypes = [VP, U64]
    lib.copra_batch_noise_tick.restype = U64
    lib.copra_batch_noise_tick.argtypes = [VP]
    lib.copra_batch_draw_noise.restype = CI
    lib.copra_batch_draw_noise.argtypes = [VP, U64, CI, VP, VP]
    one = np.ones(4)
    # (a NULL handle is refused before anything touches a device)
    assert lib.copra_batch_set_noise(None, None) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_noise_seek(None, 3) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_draw_noise(None, 0, 0, one.ctypes.data, None) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_noise_tick(None) == 0


def test_noise_init_sets_the_size():
    from copra_amd import _capi
    lib = _lib()
    assert [n for n, _ in _capi.Noise._fields_] == FIELDS
    n = _capi.Noise()
    ctypes.memset(ctypes.byref(n), 0xff, ctypes.sizeof(n))
    lib.copra_noise_init.restype = None
    lib.copra_noise_init.argtypes = [ctypes.POINTER(_capi.Noise)]
    lib.copra_noise_init(ctypes.byref(n))
    assert n.struct_size == ctypes.sizeof(_capi.Noise) == 48
    assert not any(getattr(n, f) for f in FIELDS[1:])
    # the three step structs keep their sizes
    assert ctypes.sizeof(_capi.PlantStepObs) == ctypes.sizeof(_capi.PlantStepEx) + 7 * ctypes.sizeof(VP)
    assert ctypes.sizeof(_capi.PlantStepEx) == ctypes.sizeof(_capi.PlantStep) + 2 * ctypes.sizeof(VP)


def test_python_binding_has_the_noise():
    from copra_amd import BatchLMPC, sharding
    for name in ("set_noise", "noise_seek", "draw_noise"):
        assert callable(getattr(BatchLMPC, name, None)), name
    assert isinstance(inspect.getattr_static(BatchLMPC, "noise_tick"), property)
    sn = inspect.signature(BatchLMPC.set_noise).parameters
    assert list(sn)[1:] == ["seed", "process", "sensor", "first_instance"]
    assert sn["process"].default is None and sn["sensor"].default is None and sn["first_instance"].default == 0
    dn = inspect.signature(BatchLMPC.draw_noise).parameters
    assert dn["stream"].default == "process" and dn["out"].default is None
    assert "first_instance" in inspect.getsource(sharding)


# ---- the kernel bodies on the host ----
class Tick(ctypes.Structure):
    """EmuNoiseTick of tests/emu/emu_plant_noise.h"""
    _fields_ = ([(n, CI) for n in ("build", "knoise", "batch", "nx", "nu", "ny", "N", "group", "threads", "shared")]
                + [(n, VP) for n in ("A", "B", "d", "x", "w", "fallback_u", "status", "control", "x_out", "u_out", "status_out")]
                + [("backup_steps", CI), ("fresh", CI), ("plan", VP), ("next", VP), ("age_out", VP), ("gain_dense", CI), ("gain_shared", CI)]
                + [(n, VP) for n in ("Am", "Bm", "gain", "dhat", "d_out", "xhat", "C", "Lx", "Ld", "v", "y_meas", "y_out", "xhat_out")]
                + [("seed", U64), ("first", U64), ("tick", U64), ("sigma_w", VP), ("sigma_v", VP), ("per_instance", CI), ("lds_doubles", CI)])


def _compile(src, out, extra=()):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", *extra, os.path.join(EMU, src), "-o", out])
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    lib = _compile("emu_plant_noise.cpp", str(tmp_path_factory.mktemp("emu_plant_noise") / "libemu_plant_noise.so"))
    lib.emu_plant_noise_tick.restype = CI
    lib.emu_plant_noise_tick.argtypes = [ctypes.POINTER(Tick)]
    lib.emu_noise_fill.restype = None
    lib.emu_noise_fill.argtypes = [CI] * 6 + [U64] * 3 + [VP, VP]
    lib.emu_philox.restype = None
    lib.emu_philox.argtypes = [VP, VP, VP]
    lib.emu_noise_words.restype = None
    lib.emu_noise_words.argtypes = [CI] + [VP] * 6
    return lib


@pytest.fixture(scope="module")
def old(tmp_path_factory):
    """the emulators of ABI 7, 11 and 12, as their own tests build them"""
    d = tmp_path_factory.mktemp("emu_plant_old")
    plain = _compile("emu_plant.cpp", str(d / "libemu_plant.so"))
    plain.emu_plant_step.restype = CI
    plain.emu_plant_step.argtypes = [CI] * 7 + [VP] * 13
    plain.emu_plant_lds_doubles.restype = CI
    bias = _compile("emu_plant_bias.cpp", str(d / "libemu_plant_bias.so"))
    bias.emu_plant_bias_step.restype = CI
    bias.emu_plant_bias_step.argtypes = [CI] * 7 + [VP] * 13 + [CI, CI] + [VP] * 3 + [CI] * 3 + [VP] * 5 + [CI]
    bias.emu_plant_bias_est_doubles.restype = CI
    obs = _compile("emu_plant_observer.cpp", str(d / "libemu_plant_observer.so"))
    from test_observer_abi import Tick as ObsTick
    obs.emu_plant_observer_step.restype = CI
    obs.emu_plant_observer_step.argtypes = [ctypes.POINTER(ObsTick)]
    obs.emu_plant_observer_lds_doubles.restype = CI
    return dict(plain=plain, bias=bias, obs=obs, ObsTick=ObsTick)


def _ptr(a):
    return None if a is None else a.ctypes.data


def fill(emu, batch, sigma, seed, first, tick, stream, group=7, threads=64):
    """the fill kernel's body: the terms [batch][rows] of one tick and one stream"""
    sigma = np.ascontiguousarray(sigma, dtype=np.float64)
    rows = sigma.shape[-1]
    out = np.full(batch * rows + 2, -3.5)
    emu.emu_noise_fill(batch, rows, stream, int(sigma.ndim == 2), group, threads, seed, first, tick, sigma.ctypes.data, out.ctypes.data)
    assert (out[batch * rows:] == -3.5).all()
    return out[:batch * rows].reshape(batch, rows).copy()


def _case(nx, nu, ny, batch, seed, failed=0, N=4):
    """a model, a plant of its own, states, the last solve's results, a given w and v, gains and standard deviations; everything in the ABI's
    layout (column-major blocks)"""
    rng = np.random.default_rng(seed)
    status = np.zeros(batch, dtype=np.int32)
    bad = rng.choice(batch, failed, replace=False) if failed else np.zeros(0, dtype=int)
    status[bad] = rng.integers(1, 4, bad.size)
    control = rng.standard_normal((batch, nu * N))
    control[bad] = np.nan
    x = rng.standard_normal((batch, nx))
    return dict(nx=nx, nu=nu, ny=ny, batch=batch, N=N, A=0.5 * rng.standard_normal((batch, nx, nx)), B=rng.standard_normal((batch, nx, nu)),
                d=rng.standard_normal((batch, nx)), Am=0.5 * rng.standard_normal((batch, nx, nx)), Bm=rng.standard_normal((batch, nx, nu)),
                dhat=rng.standard_normal((batch, nx)), x=x, xhat=x + 0.1 * rng.standard_normal((batch, nx)), w=0.01 * rng.standard_normal((batch, nx)),
                v=0.01 * rng.standard_normal((batch, ny)), status=status, control=control, fb=rng.standard_normal((batch, nu)),
                gain=rng.uniform(-1.0, 1.0, (batch, nx)), C=rng.standard_normal((ny, nx)), Lx=rng.uniform(-1.0, 1.0, (nx, ny)),
                Ld=rng.uniform(-0.5, 0.5, (nx, ny)), sw=rng.uniform(0.1, 2.0, (batch, nx)), sv=rng.uniform(0.1, 2.0, (batch, ny)))


def _cut(c, lo, hi):
    """instances lo .. hi of a case"""
    per = ("A", "B", "d", "Am", "Bm", "dhat", "x", "xhat", "w", "v", "status", "control", "fb", "gain", "sw", "sv")
    return dict(c, batch=hi - lo, **{k: np.ascontiguousarray(c[k][lo:hi]) for k in per})


def run(emu, c, build, group=GROUP, threads=64, knoise=1, w=None, v=None, sigma_w=None, sigma_v=None, seed=0, first=0, tick=0, with_fb=True, with_plant=True):
    """one tick, in place; returns every state and copy and the image's size"""
    b, nx, nu, ny = c["batch"], c["nx"], c["nu"], c["ny"]
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    keep = dict(A=f(c["A"]), B=f(c["B"]), d=f(c["d"]), Am=f(c["Am"]), Bm=f(c["Bm"]), gain=f(c["gain"]), C=f(c["C"]), Lx=f(c["Lx"]), Ld=f(c["Ld"]),
                w=f(w), v=f(v), sw=f(sigma_w), sv=f(sigma_v), fb=f(c["fb"]))
    out = dict(x=c["x"].copy(), dhat=c["dhat"].copy(), xhat=c["xhat"].copy(), x_out=np.full((b, nx), -3.5), u_out=np.full((b, nu), 7.0),
               d_out=np.full((b, nx), -3.5), y_out=np.full((b, ny), -3.5), xhat_out=np.full((b, nx), -3.5), s_out=np.full(b, -1, dtype=np.int32),
               a_out=np.full(b, -99, dtype=np.int32))
    T = Tick()
    T.build, T.knoise, T.batch, T.nx, T.nu, T.ny, T.N, T.group, T.threads = build, knoise, b, nx, nu, ny, c["N"], group, threads
    if with_plant or build == 0:
        T.A, T.B, T.d = _ptr(keep["A"]), _ptr(keep["B"]), _ptr(keep["d"])
    T.x, T.w, T.fallback_u, T.status, T.control = _ptr(out["x"]), _ptr(keep["w"]), _ptr(keep["fb"] if with_fb else None), _ptr(c["status"]), _ptr(c["control"])
    T.x_out, T.u_out, T.status_out, T.age_out, T.fresh = _ptr(out["x_out"]), _ptr(out["u_out"]), _ptr(out["s_out"]), _ptr(out["a_out"]), 1
    T.gain_dense, T.gain_shared = 0, 1 if build == 2 else 0
    T.Am, T.Bm, T.gain, T.dhat, T.d_out = _ptr(keep["Am"]), _ptr(keep["Bm"]), _ptr(keep["gain"]), _ptr(out["dhat"]), _ptr(out["d_out"])
    T.xhat, T.C, T.Lx, T.Ld, T.v = _ptr(out["xhat"]), _ptr(keep["C"]), _ptr(keep["Lx"]), _ptr(keep["Ld"]), _ptr(keep["v"])
    T.y_out, T.xhat_out = _ptr(out["y_out"]), _ptr(out["xhat_out"])
    T.seed, T.first, T.tick, T.sigma_w, T.sigma_v = seed, first, tick, _ptr(keep["sw"]), _ptr(keep["sv"])
    T.per_instance = int(any(a is not None and a.ndim == 2 for a in (keep["sw"], keep["sv"])))
    assert emu.emu_plant_noise_tick(ctypes.byref(T)) == 0
    out["lds"] = T.lds_doubles
    return out


KEYS = {0: ("x", "x_out", "u_out", "s_out", "a_out"), 1: ("x", "x_out", "u_out", "s_out", "a_out", "dhat", "d_out"),
        2: ("x", "x_out", "u_out", "s_out", "a_out", "dhat", "d_out", "xhat", "xhat_out", "y_out")}


def _equal(a, b, build, what, rows=slice(None)):
    for k in KEYS[build]:
        same = _same_bits(a[k][rows], b[k][rows]) if a[k].dtype == np.float64 else np.array_equal(a[k][rows], b[k][rows])
        assert same, (what, k)


# ---- the generator ----
def test_philox_known_answers(emu):
    known = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for counter, key, want in known:
        c, k, o = np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
        emu.emu_philox(c.ctypes.data, k.ctypes.data, o.ctypes.data)
        assert " ".join("%08x" % v for v in o) == want
        assert " ".join("%08x" % int(v) for v in noise_ref.philox(counter, key)) == want


def test_words_equal_the_restatement(emu):
    """random (seed, first_instance + b, j, t, s), t beyond 2^32 and first_instance + b = 2^32 - 1 among them: exact"""
    rng = np.random.default_rng(3)
    n = 4000
    seed = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    gi = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    t = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    t[:1000] = rng.integers(0, 1000, 1000, dtype=np.uint64)
    t[1000] = 2 ** 32
    t[1001] = 2 ** 32 + 5
    gi[:50] = 2 ** 32 - 1
    gi[50] = 0
    s = rng.integers(0, 2, n).astype(np.int32)
    j = rng.integers(0, 70, n).astype(np.int32)
    assert (t >= 2 ** 32).sum() > 1000
    out = np.zeros((n, 4), dtype=np.uint32)
    emu.emu_noise_words(n, seed.ctypes.data, gi.ctypes.data, s.ctypes.data, j.ctypes.data, t.ctypes.data, out.ctypes.data)
    assert np.array_equal(out.astype(np.uint64), noise_ref.words(seed, gi, s, j, t))


def test_terms_within_the_bound_of_the_restatement(emu):
    """the issue's table, then random sigma: |term - reference| <= 1e-13 sigma"""
    got = fill(emu, 2, np.ones(3), 1, 0, 0, 0)
    want = np.array([[-0.41389781465270736, -0.24733359080497033, 0.7513551541630653], [-0.8811635467900178, 0.13619777101788777, 0.2035289053135785]])
    assert np.abs(got - want).max() <= noise_ref.TOL
    got = fill(emu, 1, np.ones(4), 0x123456789abcdef, 7, 2 ** 32 + 5, 1)
    assert np.abs(got - [[-0.4214795461789664, 0.3905513384320346, 0.7764167790323104, 0.16029143904622967]]).max() <= noise_ref.TOL
    rng = np.random.default_rng(4)
    worst = 0.0
    for rows, batch, per, stream in itertools.product((1, 2, 5, 6), (1, 70), (False, True), (0, 1)):
        sigma = rng.uniform(0.0, 3.0, (batch, rows) if per else (rows,))
        sigma[..., 0] = 0.0 if rows > 1 else sigma[..., 0]
        seed, first, tick = int(rng.integers(0, 2 ** 63)), 2 ** 32 - batch, int(rng.integers(0, 2 ** 40))
        got = fill(emu, batch, sigma, seed, first, tick, stream)
        want = noise_ref.terms(seed, first, batch, sigma, tick, stream)
        ok = sigma > 0
        worst = max(worst, float((np.abs(got - want)[np.broadcast_to(ok, got.shape)] / np.broadcast_to(sigma, got.shape)[np.broadcast_to(ok, got.shape)]).max()))
        assert (np.abs(got - want) <= noise_ref.TOL * sigma).all()
        for group, threads in ((1, 1), (3, 64), (64, 256)):  # the grid of the fill does not matter
            assert _same_bits(got, fill(emu, batch, sigma, seed, first, tick, stream, group, threads))
    print("max |term - reference| / sigma = %.3g" % worst)


# ---- the tick's rule ----
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("nx,nu,ny", SHAPES)
def test_the_tick_draws_what_the_fill_gives(emu, nx, nu, ny, build):
    """noise on == the same walk given the terms as explicit w / v, bit for bit: without and with a given w / v (then w_given + term, formed in
    numpy), sigma shared and per instance; the walk at group 2 draws the same terms; sigma = 0 is the walk without noise"""
    c = _case(nx, nu, ny, BATCH, seed=100 * nx + 10 * nu + build)
    seed, first, tick = 0xfeedbeef12345, 11, 2 ** 32 + 3
    sensor = build == 2
    for given, per in itertools.product((False, True), (False, True)):
        sw, sv = (c["sw"], c["sv"]) if per else (c["sw"][0], c["sv"][0])
        tw, tv = fill(emu, BATCH, sw, seed, first, tick, 0), fill(emu, BATCH, sv, seed, first, tick, 1)
        w, v = (c["w"], c["v"]) if given else (None, None)
        what = (nx, nu, ny, build, given, per)
        got = run(emu, c, build, w=w, v=v if sensor else None, sigma_w=sw, sigma_v=sv if sensor else None, seed=seed, first=first, tick=tick)
        want = run(emu, c, build, knoise=0, w=c["w"] + tw if given else tw, v=(c["v"] + tv if given else tv) if sensor else None)
        _equal(got, want, build, what)
        assert got["lds"] == want["lds"], what  # (the image has its w / yv slot whether the pointer is given or not)
        assert not _same_bits(got["x"], run(emu, c, build, w=w, v=v if sensor else None)["x"]), what  # (and the noise did move the state)
        for group, threads in ((2, 64), (2, 3), (1, 256), (GROUP, 1)):
            again = run(emu, c, build, group=group, threads=threads, w=w, v=v if sensor else None, sigma_w=sw, sigma_v=sv if sensor else None, seed=seed,
                        first=first, tick=tick)
            _equal(got, again, build, what + (group, threads))
        # one stream alone
        only_w = run(emu, c, build, w=w, v=v if sensor else None, sigma_w=sw, seed=seed, first=first, tick=tick)
        _equal(only_w, run(emu, c, build, knoise=0, w=c["w"] + tw if given else tw, v=v if sensor else None), build, what + ("w only",))
        if sensor:
            only_v = run(emu, c, build, w=w, v=v, sigma_v=sv, seed=seed, first=first, tick=tick)
            _equal(only_v, run(emu, c, build, knoise=0, w=w, v=c["v"] + tv if given else tv), build, what + ("v only",))
        # sigma = 0: the walk without noise (a given w / v stays exactly)
        zero = run(emu, c, build, w=w, v=v if sensor else None, sigma_w=0.0 * sw, sigma_v=0.0 * sv if sensor else None, seed=seed, first=first, tick=tick)
        quiet = run(emu, c, build, knoise=0, w=w, v=v if sensor else None)
        _equal(zero, quiet, build, what + ("sigma 0",))
        if nx > 1:  # one row with sigma = 0: that row of x+ is the quiet walk's
            s1 = np.array(sw, copy=True)
            s1[..., nx - 1] = 0.0
            one = run(emu, c, build, w=w, v=v if sensor else None, sigma_w=s1, seed=seed, first=first, tick=tick)
            assert _same_bits(one["x"][:, nx - 1], quiet["x"][:, nx - 1]) and not _same_bits(one["x"][:, 0], quiet["x"][:, 0]), what


def test_measured_outputs_draw_no_sensor_noise(emu):
    """y_meas: no plant and no v -- neither sigma is looked at"""
    c = _case(6, 3, 3, BATCH, seed=9)
    ym = np.ascontiguousarray(c["v"] * 50.0)

    def meas(**kw):
        b, nx, nu, ny = c["batch"], 6, 3, 3
        out = dict(x=c["x"].copy(), dhat=c["dhat"].copy(), xhat=c["xhat"].copy(), y_out=np.full((b, ny), -3.5), u_out=np.full((b, nu), 7.0))
        keep = [np.ascontiguousarray(c[k]) for k in ("Am", "Bm", "C", "Lx", "Ld", "fb")]
        T = Tick()
        T.build, T.knoise, T.batch, T.nx, T.nu, T.ny, T.N, T.group, T.threads, T.fresh, T.gain_shared = 2, 1, b, nx, nu, ny, c["N"], GROUP, 64, 1, 1
        T.x, T.fallback_u, T.status, T.control, T.u_out = _ptr(out["x"]), _ptr(keep[5]), _ptr(c["status"]), _ptr(c["control"]), _ptr(out["u_out"])
        T.Am, T.Bm, T.dhat, T.xhat, T.C, T.Lx, T.Ld = _ptr(keep[0]), _ptr(keep[1]), _ptr(out["dhat"]), _ptr(out["xhat"]), _ptr(keep[2]), _ptr(keep[3]), _ptr(keep[4])
        T.y_meas, T.y_out = _ptr(ym), _ptr(out["y_out"])
        T.seed, T.sigma_w, T.sigma_v = 5, _ptr(kw.get("sw")), _ptr(kw.get("sv"))
        assert emu.emu_plant_noise_tick(ctypes.byref(T)) == 0
        return out
    quiet, noisy = meas(), meas(sw=np.ones(6), sv=np.ones(3))
    for k in ("x", "dhat", "xhat", "y_out", "u_out"):
        assert _same_bits(quiet[k], noisy[k]), k
    assert _same_bits(noisy["y_out"], ym) and _same_bits(noisy["x"], c["x"])


@pytest.mark.parametrize("build", BUILDS)
def test_draws_do_not_depend_on_the_batch(emu, build):
    """instances 40 .. 63 of a batch of 64 equal a batch of 24 with first_instance = 40"""
    nx, nu, ny = 6, 3, 3
    c = _case(nx, nu, ny, 64, seed=21 + build)
    sensor = build == 2
    for per in (False, True):
        sw, sv = (c["sw"], c["sv"]) if per else (c["sw"][0], c["sv"][0])
        whole = run(emu, c, build, group=12, sigma_w=sw, sigma_v=sv if sensor else None, seed=77, first=0, tick=9)
        part = run(emu, _cut(c, 40, 64), build, group=10, sigma_w=sw[40:] if per else sw, sigma_v=(sv[40:] if per else sv) if sensor else None, seed=77,
                   first=40, tick=9)
        for k in KEYS[build]:
            same = _same_bits(whole[k][40:], part[k]) if whole[k].dtype == np.float64 else np.array_equal(whole[k][40:], part[k])
            assert same, (build, per, k)
        other = run(emu, _cut(c, 40, 64), build, group=10, sigma_w=sw[40:] if per else sw, sigma_v=(sv[40:] if per else sv) if sensor else None, seed=77,
                    first=41, tick=9)
        assert not _same_bits(other["x"], part["x"])


# ---- noise off: the earlier ABIs' walks ----
@pytest.mark.parametrize("nx,nu,ny", SHAPES)
def test_noise_off_is_the_earlier_tick(emu, old, nx, nu, ny):
    """without a sigma both sets of bodies (kNoise or not) give the bits of emu_plant.cpp, emu_plant_bias.cpp and emu_plant_observer.cpp, over
    images of the same size"""
    c = _case(nx, nu, ny, BATCH, seed=31 * nx + nu, failed=1)
    b, N = BATCH, c["N"]
    for with_w, knoise in itertools.product((False, True), (0, 1)):
        w = c["w"] if with_w else None
        v = c["v"] if with_w else None
        # ABI 7
        x, x_out, u_out, s_out = c["x"].copy(), np.full((b, nx), -3.5), np.full((b, nu), 7.0), np.full(b, -1, dtype=np.int32)
        assert old["plain"].emu_plant_step(b, nx, nu, N, GROUP, 64, 0, _ptr(c["A"]), _ptr(c["B"]), _ptr(c["d"]), _ptr(x), _ptr(w), _ptr(c["fb"]), _ptr(c["status"]),
                                           _ptr(c["control"]), _ptr(x), _ptr(x_out), _ptr(u_out), _ptr(s_out), None) == 0
        got = run(emu, c, 0, knoise=knoise, w=w)
        assert _same_bits(got["x"], x) and _same_bits(got["x_out"], x_out) and _same_bits(got["u_out"], u_out) and np.array_equal(got["s_out"], s_out)
        assert got["lds"] == old["plain"].emu_plant_lds_doubles(nx, nu, GROUP, 0, int(with_w))
        # ABI 11
        x, dhat, d_out, a_out = c["x"].copy(), c["dhat"].copy(), np.full((b, nx), -3.5), np.full(b, -99, dtype=np.int32)
        x_out, u_out = np.full((b, nx), -3.5), np.full((b, nu), 7.0)
        assert old["bias"].emu_plant_bias_step(b, nx, nu, N, GROUP, 64, 0, _ptr(c["A"]), _ptr(c["B"]), _ptr(c["d"]), _ptr(x), _ptr(w), _ptr(c["fb"]),
                                               _ptr(c["status"]), _ptr(c["control"]), _ptr(x), _ptr(x_out), _ptr(u_out), _ptr(s_out), None, 0, 1, None, None,
                                               _ptr(a_out), 1, 0, 0, _ptr(c["Am"]), _ptr(c["Bm"]), _ptr(c["gain"]), _ptr(dhat), _ptr(d_out), -1) == 0
        got = run(emu, c, 1, knoise=knoise, w=w)
        for k, ref in (("x", x), ("x_out", x_out), ("u_out", u_out), ("dhat", dhat), ("d_out", d_out)):
            assert _same_bits(got[k], ref), (k, with_w, knoise)
        assert np.array_equal(got["a_out"], a_out)
        assert got["lds"] == old["bias"].emu_plant_bias_est_doubles(nx, nu, GROUP, 0, int(with_w), 0, 0, 0, 0)
        # ABI 12
        ref = dict(x=c["x"].copy(), dhat=c["dhat"].copy(), xhat=c["xhat"].copy(), x_out=np.full((b, nx), -3.5), u_out=np.full((b, nu), 7.0),
                   d_out=np.full((b, nx), -3.5), y_out=np.full((b, ny), -3.5), xhat_out=np.full((b, nx), -3.5))
        T = old["ObsTick"]()
        T.batch, T.nx, T.nu, T.ny, T.N, T.group, T.threads, T.fresh, T.gain_shared, T.vec2_mode = b, nx, nu, ny, N, GROUP, 64, 1, 1, -1
        T.A, T.B, T.d, T.xp, T.w, T.fallback_u = _ptr(c["A"]), _ptr(c["B"]), _ptr(c["d"]), _ptr(ref["x"]), _ptr(w), _ptr(c["fb"])
        T.status, T.control, T.x_out, T.u_out = _ptr(c["status"]), _ptr(c["control"]), _ptr(ref["x_out"]), _ptr(ref["u_out"])
        T.Am, T.Bm, T.dhat, T.xhat, T.xhat_next = _ptr(c["Am"]), _ptr(c["Bm"]), _ptr(ref["dhat"]), _ptr(ref["xhat"]), _ptr(ref["xhat"])
        T.C, T.Lx, T.Ld, T.v = _ptr(c["C"]), _ptr(c["Lx"]), _ptr(c["Ld"]), _ptr(v)
        T.y_out, T.xhat_out, T.d_out = _ptr(ref["y_out"]), _ptr(ref["xhat_out"]), _ptr(ref["d_out"])
        assert old["obs"].emu_plant_observer_step(ctypes.byref(T)) == 0
        got = run(emu, c, 2, knoise=knoise, w=w, v=v)
        for k in ref:
            assert _same_bits(got[k], ref[k]), (k, with_w, knoise)
        assert got["lds"] == old["obs"].emu_plant_observer_lds_doubles(nx, nu, ny, GROUP, 0, int(with_w), 0, 0, 0, 1, 1, int(with_w))


def test_image_sizes_are_unchanged(old):
    """the layout functions with their earlier arguments: the figures of the launch at (6, 3, 3)"""
    assert old["plain"].emu_plant_lds_doubles(6, 3, 32, 0, 1) == 32 * (36 + 18 + 6 + 6 + 6 + 3) + 16
    assert 8 * old["obs"].emu_plant_observer_lds_doubles(6, 3, 3, 1, 0, 1, 1, 0, 0, 1, 0, 1) == 1760


# ---- held instances ----
@pytest.mark.parametrize("build", BUILDS)
def test_held_instances_keep_their_bits(emu, build):
    """no fallback: a failed instance keeps x (and xhat, dhat) bit for bit with noise on; the others of its group get the terms they would
    get anyway"""
    nx, nu, ny = 6, 3, 3
    c = _case(nx, nu, ny, 13, seed=40 + build, failed=4)
    ok = c["status"] == 0
    assert 0 < (~ok).sum() < 13
    sensor = build == 2
    tw, tv = fill(emu, 13, c["sw"], 8, 100, 3, 0), fill(emu, 13, c["sv"], 8, 100, 3, 1)
    got = run(emu, c, build, sigma_w=c["sw"], sigma_v=c["sv"] if sensor else None, seed=8, first=100, tick=3, with_fb=False)
    want = run(emu, c, build, knoise=0, w=tw, v=tv if sensor else None, with_fb=False)
    _equal(got, want, build, "held")
    assert _same_bits(got["x"][~ok], c["x"][~ok]) and (got["a_out"][~ok] == -2).all() and np.isnan(got["u_out"][~ok]).all()
    assert not np.isnan(got["x"]).any()
    if build >= 1:
        assert _same_bits(got["dhat"][~ok], c["dhat"][~ok])
    if build == 2:
        assert _same_bits(got["xhat"][~ok], c["xhat"][~ok])
    quiet = run(emu, c, build, knoise=0, with_fb=False)
    assert not _same_bits(got["x"][ok], quiet["x"][ok])


# ---- the law ----
def test_moments_of_the_draws(emu):
    """seed 2026, 4096 instances x 6 rows x ticks 0 .. 15 of the fill's body: mean, variance, fourth moment and the mean products between
    neighbours, each within five standard errors"""
    n0 = np.stack([fill(emu, 4096, np.ones(6), 2026, 0, t, 0, 32, 96) for t in range(16)])
    v0 = fill(emu, 4096, np.ones(6), 2026, 0, 0, 1, 32, 96)
    n = n0.size
    assert n == 393216
    se = 1.0 / np.sqrt(n)
    figures = dict(mean=n0.mean(), var=n0.var(), m4=(n0 ** 4).mean(), ticks=(n0[:-1] * n0[1:]).mean(), instances=(n0[:, :-1] * n0[:, 1:]).mean(),
                   rows=(n0[:, :, :-1] * n0[:, :, 1:]).mean(), streams=(n0[0] * v0).mean())
    print(" ".join("%s %.4g" % kv for kv in figures.items()))
    assert abs(figures["mean"]) <= 5 * se
    assert abs(figures["var"] - 1.0) <= 5 * np.sqrt(2.0 / n)
    assert abs(figures["m4"] - 3.0) <= 5 * np.sqrt(96.0 / n)
    for k in ("ticks", "instances", "rows", "streams"):
        assert abs(figures[k]) <= 5 * se, k


# ---- memory errors on the host ----
def test_kernel_bodies_under_the_address_and_ub_sanitizers(tmp_path):
    """tests/emu/emu_plant_noise_main.cpp -- (6, 3, 3) and (3, 1, 1), batch 5, group 4, all three builds with noise on, and the fill -- as a
    stand-alone program built with -fsanitize=address,undefined; every array has exactly the elements the kernel may touch.  Exit status 0
    and an empty stderr."""
    exe = str(tmp_path / "emu_plant_noise_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(EMU, "emu_plant_noise.cpp"), os.path.join(EMU, "emu_plant_noise_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
