"""The tick at its launch edges, without a GPU: the five walkers of tests/emu (the phase bodies of copra_amd/csrc/plant_step.hpp, compiled by
this file itself) asked what the existing files never ask them.

  1  order independence: the threads of every phase and the workgroups of the grid walked ascending, descending and in seeded permutations
     (tests/emu/emu_walk.h) give the same bits in every output and every in-place state.  On the device no order holds: a phase that reads what
     another thread of the SAME phase wrote passes an ascending walk and races on the GPU.
  2  the guard zone behind the image -- sized by the layout function the launch uses -- stays untouched, and no NaN of the NaN-filled image or
     of a failed instance's control reaches an output.
  3  shapes at which copra_hip_plant.hip changes what it launches: the group falls to 2 and to 1, the image passes 48 KiB, the last group is
     partial at odd nx -- each at the launch's OWN group, asked of the emulator (emu_plant_launch_group), against the numpy.longdouble
     statements and derived bounds of the neighbouring files: reference_step / step_bound (test_closed_loop_abi.py), reference_bias and its
     bound (test_bias_estimator_abi.py), reference_observer with Ey / Eh / Ed (test_observer_abi.py); with noise the terms of noise_ref.py.
  4  each input array in turn 8 bytes past a 16-byte boundary: the launch must give up the 16-byte copies (vec2 == 0) and every output keeps
     the bits of the all-aligned run at the same group.
  5  the launch geometry (plant_group, *_image_bytes, the layout structs), swept: the group is 1 or even and at most 32, the launched image is
     at most max(24 KiB, the one-instance image that was checked against the LDS), and no two parts of an image overlap -- from the offsets the
     layout structs give and the number of doubles the phase bodies put at each.

No bound here is new and none is fitted: the figures printed are max error / bound."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import noise_ref
from test_bias_estimator_abi import _check as bias_check
from test_bias_estimator_abi import _expect as bias_expect
from test_bias_estimator_abi import abi_gain
from test_closed_loop_abi import reference_step, step_bound
from test_noise_abi import Tick as NoiseTick
from test_observer_abi import Tick as ObsTick
from test_observer_abi import _check as obs_check
from test_observer_abi import _expect as obs_expect
from test_observer_abi import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
VP, CI, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulonglong
LD = np.longdouble
FALLBACK, HELD = -1, -2
SENTINEL = -3.5  # what an output holds that the tick did not write (GUARD of test_observer_abi.py)
ORDERS = ((0, 0), (1, 0), (2, 0x5eed), (2, 77))  # (order, seed) of emu_walk.h: ascending, descending, two permutations
PLAIN_ARGS = [CI] * 7 + [VP] * 13
BACKUP_ARGS = PLAIN_ARGS + [CI, CI] + [VP] * 3
BIAS_ARGS = BACKUP_ARGS + [CI] * 3 + [VP] * 5 + [CI]
KIND = dict(plain=0, est=1, obs=2)


# ---- the walkers ----
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_tick_edges")
    libs = {}
    for name in ("emu_plant", "emu_plant_backup", "emu_plant_bias", "emu_plant_observer", "emu_plant_noise"):
        so = str(d / ("lib%s.so" % name))
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(EMU, name + ".cpp"), "-o", so])
        libs[name] = ctypes.CDLL(so)
    for fn, args in ((libs["emu_plant"].emu_plant_step_walk, PLAIN_ARGS), (libs["emu_plant_backup"].emu_plant_backup_step_walk, BACKUP_ARGS),
                     (libs["emu_plant_bias"].emu_plant_bias_step_walk, BIAS_ARGS)):
        fn.restype, fn.argtypes = CI, args + [CI, U64]
    libs["emu_plant_observer"].emu_plant_observer_step_walk.restype = CI
    libs["emu_plant_observer"].emu_plant_observer_step_walk.argtypes = [ctypes.POINTER(ObsTick), CI, U64]
    libs["emu_plant_noise"].emu_plant_noise_tick_walk.restype = CI
    libs["emu_plant_noise"].emu_plant_noise_tick_walk.argtypes = [ctypes.POINTER(NoiseTick), CI, U64, VP]
    libs["emu_plant_noise"].emu_noise_fill.restype = None
    libs["emu_plant_noise"].emu_noise_fill.argtypes = [CI] * 6 + [U64] * 3 + [VP, VP]
    for lib in libs.values():  # the geometry: every emulator exports the same functions of plant_step.hpp
        lib.emu_plant_image_bytes.restype, lib.emu_plant_image_bytes.argtypes = ctypes.c_longlong, [CI] * 5
        lib.emu_plant_launch_group.restype, lib.emu_plant_launch_group.argtypes = CI, [CI] * 5
        lib.emu_plant_lds_max.restype = lib.emu_plant_lds_target.restype = ctypes.c_longlong
        lib.emu_plant_group_max.restype = lib.emu_plant_guard_doubles.restype = CI
        lib.emu_plant_layouts.restype, lib.emu_plant_layouts.argtypes = CI, [CI, CI, VP, VP]
    return libs


def launch_group(emu, build, nx, nu, ny=0, dense=0):
    return emu["emu_plant_noise"].emu_plant_launch_group(KIND[build], nx, nu, ny, dense)


def image_bytes(emu, build, nx, nu, ny=0, dense=0):
    return emu["emu_plant_noise"].emu_plant_image_bytes(KIND[build], nx, nu, ny, dense)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _same_bits(a, b):
    if a.dtype != np.float64:
        return np.array_equal(a, b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


class Placed:
    """arrays at a chosen alignment: 16 bytes, or -- for the names in `mis` -- 8 bytes past a 16-byte boundary"""

    def __init__(self, mis=()):
        self.mis, self.keep = set(mis), []

    def __call__(self, name, a, tail=0):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        raw = np.full(a.size + tail + 3, SENTINEL)
        off = (-(raw.ctypes.data // 8) % 2) + (1 if name in self.mis else 0)
        view = raw[off:off + a.size + tail]
        view[:a.size] = a.ravel()
        assert view.ctypes.data % 16 == (8 if name in self.mis else 0)
        self.keep.append(raw)
        return view


# ---- cases ----
def make_case(nx, nu, ny, batch, seed, failed, N=3, K=2):
    """everything any build reads, in natural indexing: a plant per instance and one for the batch, the model, the states, the last solve's
    results (`failed` instances without a solution hold NaN), plans of K steps with every value of next[b] (none, a step, used up), gains,
    noise given and standard deviations"""
    rng = np.random.default_rng(seed)
    status = np.zeros(batch, dtype=np.int32)
    bad = rng.choice(batch, failed, replace=False) if failed else np.zeros(0, dtype=int)
    status[bad] = rng.integers(1, 4, bad.size)
    control = rng.standard_normal((batch, nu * N))
    control[bad] = np.nan  # what the engine leaves in a failed instance
    xp = rng.standard_normal((batch, nx)) * 10.0 ** rng.integers(-2, 2, (batch, 1))
    nxt = rng.integers(0, K + 2, batch).astype(np.int32)
    nxt[bad[:1]] = 0  # one failed instance has no plan: it falls back or is held with backup plans as well
    return dict(nx=nx, nu=nu, ny=ny, batch=batch, N=N, K=K, status=status, control=control, fb=rng.standard_normal((batch, nu)),
                own=(0.5 * rng.standard_normal((batch, nx, nx)), rng.standard_normal((batch, nx, nu)), rng.standard_normal((batch, nx))),
                shared=(0.5 * rng.standard_normal((nx, nx)), rng.standard_normal((nx, nu)), rng.standard_normal(nx)),
                Am=0.5 * rng.standard_normal((batch, nx, nx)), Bm=rng.standard_normal((batch, nx, nu)), dhat=rng.standard_normal((batch, nx)),
                xp=xp, x=xp, xhat=xp + 0.1 * rng.standard_normal((batch, nx)), w=0.01 * rng.standard_normal((batch, nx)),
                v=0.01 * rng.standard_normal((batch, ny)), ym=rng.standard_normal((batch, ny)), plan=rng.standard_normal((batch, K, nu)), next=nxt,
                gl=rng.uniform(-1.0, 1.0, (batch, nx)), gd=rng.uniform(-1.0, 1.0, (batch, nx, nx)), C=rng.standard_normal((batch, ny, nx)),
                Lx=rng.uniform(-1.0, 1.0, (batch, nx, ny)), Ld=rng.uniform(-0.5, 0.5, (batch, nx, ny)), sw=rng.uniform(0.1, 2.0, (batch, nx)),
                sv=rng.uniform(0.1, 2.0, (batch, ny)))


def cfg(build, plant="own", w=True, v=True, meas=False, fb=True, K=0, fresh=1, dense=0, per=1, Ld=True, noise=False):
    """one tick's switches.  build: plain | est | obs; plant: own | shared | none (the model with its estimates); K: backup steps; per: the
    gains (est: the gain, obs: C, Lx, Ld) hold one block per instance; noise: drawn in phase 1 (the walker of emu_plant_noise.cpp)"""
    if meas:
        plant, w, v = "none", False, False
    return dict(build=build, plant=plant, w=w, v=v and build == "obs", meas=meas, fb=fb, K=K, fresh=fresh, dense=dense, per=per, Ld=Ld, noise=noise)


def _gain(c, g):
    return c["gd" if g["dense"] else "gl"] if g["per"] else c["gd" if g["dense"] else "gl"][0]


def _gains(c, g):
    return tuple(c[k] if g["per"] else c[k][0] for k in ("C", "Lx", "Ld"))


def rule(c, g):
    """(u applied, age) per instance, the rule of plant_step.hpp's head"""
    ok, nu, K = c["status"] == 0, c["nu"], g["K"]
    last = FALLBACK if g["fb"] else HELD
    if K == 0:
        age = np.where(ok, 0, last)
    else:
        nxt = c["next"]
        age = np.where(ok & bool(g["fresh"]), 0, np.where((nxt >= 1) & (nxt <= K), nxt, last))
    u = np.full((c["batch"], nu), np.nan)
    for b, a in enumerate(age):
        u[b] = c["control"][b, :nu] if a == 0 else c["plan"][b, a - 1] if a > 0 else c["fb"][b] if a == FALLBACK else np.nan
    return u, age.astype(np.int32)


NOISE_SEED, NOISE_FIRST, NOISE_TICK = 0xfeedbeef12345, 11, 2 ** 32 + 3


def tick(emu, c, g, group, threads=64, order=0, seed=0, mis=()):
    """one tick of the build g describes through its own walker (noise: emu_plant_noise.cpp's), every state in place; returns every output,
    the walker's return code and whether it copied two doubles per lane"""
    b, nx, nu, ny, N, K = c["batch"], c["nx"], c["nu"], c["ny"], c["N"], g["K"]
    at = Placed(mis)
    build, kind = g["build"], g["plant"]
    A = B = d = None
    if kind != "none":
        A, B, d = at("A", abi(c[kind][0])), at("B", abi(c[kind][1])), at("d", c[kind][2])
    shared = int(kind == "shared")
    xs, dhat, xhat = at("x0", c["xp"], 4), at("dhat", c["dhat"], 4), at("xhat", c["xhat"], 4)
    x_out, d_out, xhat_out = (np.full(b * nx + 4, SENTINEL) for _ in range(3))
    y_out, u_out = np.full(b * ny + 4, SENTINEL), np.full(b * nu + 4, 7.0)
    s_out, a_out = np.full(b + 2, -1, dtype=np.int32), np.full(b + 2, -99, dtype=np.int32)
    w, fb = at("w", c["w"]) if g["w"] else None, at("fb", c["fb"]) if g["fb"] else None
    control, plan = at("control", c["control"]), at("plan", c["plan"], 4) if K else None
    nxt = np.concatenate([c["next"], np.full(2, -7, dtype=np.int32)]) if K else None
    Am, Bm = at("Am", abi(c["Am"])), at("Bm", abi(c["Bm"]))
    gain = at("gain", abi_gain(_gain(c, g), g["dense"])) if build == "est" else None
    C = Lx = Ld = v = ym = None
    if build == "obs":
        Cn, Lxn, Ldn = _gains(c, g)
        C, Lx, Ld = at("C", abi(Cn)), at("Lx", abi(Lxn)), at("Ld", abi(Ldn)) if g["Ld"] else None
        v, ym = at("v", c["v"]) if g["v"] else None, at("v", c["ym"]) if g["meas"] else None
    vec2 = ctypes.c_int(-1)
    head = [b, nx, nu, N, group, threads, shared, _ptr(A), _ptr(B), _ptr(d), _ptr(xs), _ptr(w), _ptr(fb), _ptr(c["status"]), _ptr(control), _ptr(xs),
            _ptr(x_out), _ptr(u_out), _ptr(s_out), ctypes.addressof(vec2)]
    back = [K, g["fresh"], _ptr(plan), _ptr(nxt), _ptr(a_out)]
    if g["noise"]:
        T = NoiseTick()
        T.build, T.knoise, T.batch, T.nx, T.nu, T.ny, T.N, T.group, T.threads, T.shared = KIND[build], 1, b, nx, nu, ny, N, group, threads, shared
        T.A, T.B, T.d, T.x, T.w, T.fallback_u, T.status, T.control = _ptr(A), _ptr(B), _ptr(d), _ptr(xs), _ptr(w), _ptr(fb), _ptr(c["status"]), _ptr(control)
        T.x_out, T.u_out, T.status_out, T.age_out = _ptr(x_out), _ptr(u_out), _ptr(s_out), _ptr(a_out)
        T.backup_steps, T.fresh, T.plan, T.next = K, g["fresh"], _ptr(plan), _ptr(nxt)
        T.gain_dense, T.gain_shared = g["dense"], int(not g["per"])
        T.Am, T.Bm, T.gain, T.dhat, T.d_out = _ptr(Am), _ptr(Bm), _ptr(gain), _ptr(dhat), _ptr(d_out)
        T.xhat, T.C, T.Lx, T.Ld, T.v, T.y_meas = _ptr(xhat), _ptr(C), _ptr(Lx), _ptr(Ld), _ptr(v), _ptr(ym)
        T.y_out, T.xhat_out = _ptr(y_out), _ptr(xhat_out)
        sw, sv = at("sw", c["sw"]), at("sv", c["sv"]) if build == "obs" else None
        T.seed, T.first, T.tick, T.sigma_w, T.sigma_v, T.per_instance = NOISE_SEED, NOISE_FIRST, NOISE_TICK, _ptr(sw), _ptr(sv), 1
        rc = emu["emu_plant_noise"].emu_plant_noise_tick_walk(ctypes.byref(T), order, seed, ctypes.addressof(vec2))
    elif build == "plain" and K == 0:
        rc = emu["emu_plant"].emu_plant_step_walk(*head, order, seed)
    elif build == "plain":
        rc = emu["emu_plant_backup"].emu_plant_backup_step_walk(*head, *back, order, seed)
    elif build == "est":
        rc = emu["emu_plant_bias"].emu_plant_bias_step_walk(*head, *back, 1, g["dense"], int(not g["per"]), _ptr(Am), _ptr(Bm), _ptr(gain), _ptr(dhat),
                                                            _ptr(d_out), -1, order, seed)
    else:
        T = ObsTick()
        T.batch, T.nx, T.nu, T.ny, T.N, T.group, T.threads, T.shared = b, nx, nu, ny, N, group, threads, shared
        T.A, T.B, T.d, T.xp, T.w, T.fallback_u, T.status, T.control = _ptr(A), _ptr(B), _ptr(d), _ptr(xs), _ptr(w), _ptr(fb), _ptr(c["status"]), _ptr(control)
        T.x_out, T.u_out, T.status_out, T.age_out = _ptr(x_out), _ptr(u_out), _ptr(s_out), _ptr(a_out)
        T.backup_steps, T.fresh, T.plan, T.next, T.gain_shared = K, g["fresh"], _ptr(plan), _ptr(nxt), int(not g["per"])
        T.Am, T.Bm, T.dhat, T.xhat, T.xhat_next = _ptr(Am), _ptr(Bm), _ptr(dhat), _ptr(xhat), _ptr(xhat)
        T.C, T.Lx, T.Ld, T.v, T.y_meas = _ptr(C), _ptr(Lx), _ptr(Ld), _ptr(v), _ptr(ym)
        T.y_out, T.xhat_out, T.d_out = _ptr(y_out), _ptr(xhat_out), _ptr(d_out)
        T.vec2_mode, T.vec2_used = -1, -1
        rc = emu["emu_plant_observer"].emu_plant_observer_step_walk(ctypes.byref(T), order, seed)
        vec2.value = T.vec2_used
    what = (g, group, threads, order, seed, mis)
    for buf, n in ((xs, b * nx), (dhat, b * nx), (xhat, b * nx), (x_out, b * nx), (d_out, b * nx), (xhat_out, b * nx), (y_out, b * ny)):
        assert (buf[n:] == SENTINEL).all(), what  # nothing behind the batch's last instance is written
    assert (u_out[b * nu:] == 7.0).all() and (s_out[b:] == -1).all() and (a_out[b:] == -99).all(), what
    assert plan is None or ((plan[b * K * nu:] == SENTINEL).all() and (nxt[b:] == -7).all()), what
    cut = lambda buf, n: buf[:b * n].reshape(b, n).copy()  # noqa: E731
    out = dict(x=cut(xs, nx), dhat=cut(dhat, nx), xhat=cut(xhat, nx), x_out=cut(x_out, nx), d_out=cut(d_out, nx), xhat_out=cut(xhat_out, nx),
               y_out=cut(y_out, ny), u_out=cut(u_out, nu), s_out=s_out[:b].copy(), a_out=a_out[:b].copy(), rc=rc, vec2=vec2.value)
    out["xp"] = out["x"]
    if K:
        out["plan"], out["next"] = plan[:b * K * nu].reshape(b, K, nu).copy(), nxt[:b].copy()
    return out


OUTPUTS = ("x", "dhat", "xhat", "x_out", "d_out", "xhat_out", "y_out", "u_out", "s_out", "a_out", "plan", "next")


def assert_same(a, b, what):
    for k in OUTPUTS:
        if k in a:
            assert _same_bits(a[k], b[k]), (what, k)


# ---- the references ----
def noise_terms(emu, c, stream):
    """what phase 1 draws, from the fill kernel's body: [batch][rows] of NOISE_TICK"""
    sigma = np.ascontiguousarray(c["sw" if stream == 0 else "sv"])
    out = np.zeros(sigma.shape)
    emu["emu_plant_noise"].emu_noise_fill(c["batch"], sigma.shape[1], stream, 1, 7, 64, NOISE_SEED, NOISE_FIRST, NOISE_TICK, sigma.ctypes.data, out.ctypes.data)
    return out


def check(c, g, got, what):
    """one tick without noise against the longdouble statements within the derived bounds; returns max error / bound"""
    nx, nu = c["nx"], c["nu"]
    u, age = rule(c, g)
    moved = age != HELD
    u0 = np.where(moved[:, None], u, 0.0)
    assert got["rc"] == 0, what
    assert _same_bits(got["u_out"], u) and np.array_equal(got["s_out"], c["status"]), what
    if g["K"] or g["build"] != "plain" or g["noise"]:  # (the walker of the tick of ABI 7 has no age_out)
        assert np.array_equal(got["a_out"], age), what
    plant = None if g["plant"] == "none" else c[g["plant"]]
    if g["build"] == "plain":
        ref, S = reference_step(plant[0], plant[1], plant[2], c["xp"], u0, c["w"] if g["w"] else None)
        err, bound = np.abs(got["x"][moved].astype(LD) - ref[moved]), step_bound(nx, nu, S[moved])
        assert not np.isnan(got["x"]).any() and (err <= bound).all(), (what, float((err / bound).max()))
        assert _same_bits(got["x"][~moved], c["xp"][~moved]) and _same_bits(got["x_out"], got["x"]), what
        return float((err / bound).max())
    if g["build"] == "est":
        ref, Sx, dref, dbound = bias_expect(c, plant, u0, g["w"], _gain(c, g), g["dense"])
        worst = bias_check(got, c, ref, Sx, dref, dbound, moved, what)
        return max(worst, float((np.abs(got["x"][moved].astype(LD) - ref[moved]) / step_bound(nx, nu, Sx[moved])).max()))
    gains = _gains(c, g)
    ref, Sx, R = obs_expect(c, plant, u0, gains, g["Ld"], g["w"], g["v"], g["meas"])
    return obs_check(got, c, ref, Sx, R, moved, gains, g["Ld"], g["v"], g["meas"], what)


# ---- 1, 2: the matrix of builds ----
def builds(kind):
    if kind == "plain":
        return [cfg("plain"), cfg("plain", plant="shared", w=False)]
    if kind == "backup":
        return [cfg("plain", K=2, fresh=1), cfg("plain", K=2, fresh=0), cfg("plain", plant="shared", K=2, fresh=1, w=False)]
    if kind == "est":
        return [cfg("est", plant=p, dense=dn, per=per, K=2 * (dn ^ per), fresh=per) for dn, per, p in itertools.product((0, 1), (0, 1), ("own", "none"))]
    return [cfg("obs", plant=p, meas=m, Ld=ld, per=ld ^ (p == "own"), K=2 * (p == "none"), fresh=int(ld))
            for (p, m), ld in itertools.product((("own", False), ("none", False), ("none", True)), (True, False))]


MATRIX = list(itertools.product(("plain", "backup", "est", "obs"), (False, True)))
MATRIX_IDS = ["%s%s" % (k, "-noise" if n else "") for k, n in MATRIX]
SMALL = ((5, 2, 2), (6, 3, 3))


def matrix(emu, kind, noise):
    """(case, cfg, group, threads) of the matrix: shapes (5, 2, 2) and (6, 3, 3), batch 13 with three failed instances, with and without a
    fallback, the launch's own group and group 2, 64 threads and 3"""
    for nx, nu, ny in SMALL:
        c = make_case(nx, nu, ny, 13, seed=100 * nx + nu, failed=3)
        for g0, fb in itertools.product(builds(kind), (True, False)):
            g = dict(g0, fb=fb, noise=noise)
            own = launch_group(emu, g["build"], nx, nu, ny, g["dense"])
            assert own % 2 == 0 and 13 % own != 0  # (a partial last group)
            for group, threads in itertools.product(sorted({own, 2}), (64, 3)):
                yield c, g, group, threads


@pytest.mark.parametrize("kind,noise", MATRIX, ids=MATRIX_IDS)
def test_every_walk_order_gives_the_same_bits(emu, kind, noise):
    """every output array and every in-place state (x, dhat, xhat, plan, next) is bit-identical under the four orders"""
    runs = 0
    for c, g, group, threads in matrix(emu, kind, noise):
        first = tick(emu, c, g, group, threads, *ORDERS[0])
        ok = c["status"] == 0
        assert 0 < ok.sum() < c["batch"]
        for order, seed in ORDERS[1:]:
            again = tick(emu, c, g, group, threads, order, seed)
            assert_same(first, again, (g, group, threads, order, seed))
            assert again["vec2"] == first["vec2"] == 1
            runs += 1
    assert runs >= 2 * 2 * 2 * 2 * 2 * 3


@pytest.mark.parametrize("kind,noise", MATRIX, ids=MATRIX_IDS)
def test_the_guard_stays_and_no_nan_leaves_the_image(emu, kind, noise):
    """the walkers' return code is 0 (the guard behind the image is untouched after every workgroup), and the only NaN in any output is the
    u_out of a held instance"""
    assert emu["emu_plant_noise"].emu_plant_guard_doubles() >= 64
    for c, g, group, threads in matrix(emu, kind, noise):
        for order, seed in (ORDERS[0], ORDERS[2]):
            got = tick(emu, c, g, group, threads, order, seed)
            what = (g, group, threads, order)
            assert got["rc"] == 0, what
            _, age = rule(c, g)
            for k in OUTPUTS:
                if k in got and k != "u_out":
                    assert not np.isnan(got[k].astype(np.float64)).any(), (what, k)
            assert np.array_equal(np.isnan(got["u_out"]).any(axis=1), age == HELD) and np.array_equal(np.isnan(got["u_out"]).all(axis=1), age == HELD), what


@pytest.mark.parametrize("kind", ("plain", "backup", "est", "obs"))
def test_the_matrix_holds_the_rule(emu, kind):
    """the same matrix without noise, ascending: every output within the derived bounds (so the bits the orders agree on are the right ones);
    with noise: the bits of the walk that is GIVEN the drawn terms"""
    worst = 0.0
    for c, g, group, threads in matrix(emu, kind, False):
        got = tick(emu, c, g, group, threads)
        worst = max(worst, check(c, g, got, (g, group, threads)))
        if threads == 64 and not g["meas"]:
            tw, tv = noise_terms(emu, c, 0), noise_terms(emu, c, 1)
            given = dict(c, w=c["w"] + tw if g["w"] else tw, v=c["v"] + tv if g["v"] else tv)
            drawn = tick(emu, c, dict(g, noise=True), group, threads)
            replay = tick(emu, given, dict(g, w=True, v=g["build"] == "obs"), group, threads)
            assert_same({k: a for k, a in drawn.items() if k != "a_out"}, replay, (g, group, "noise"))  # (the walker of ABI 7 has no age_out)
    print("%s: max err / bound = %.3f" % (kind, worst))
    assert worst <= 1.0


# ---- 3: launch-edge shapes at the launch's own group ----
EDGES = [  # (build, nx, nu, ny, dense, batch, what the launch does there)
    ("plain", 31, 1, 0, 0, 13, "group 2"), ("plain", 40, 1, 0, 0, 5, "group 1"), ("plain", 78, 1, 0, 0, 5, "above 48 KiB"),
    ("plain", 5, 2, 0, 0, 13, "partial"), ("plain", 7, 3, 0, 0, 13, "partial"),
    ("est", 23, 1, 0, 1, 13, "group 1"), ("est", 23, 1, 0, 0, 13, "group 2"), ("est", 56, 1, 0, 1, 5, "above 48 KiB"), ("est", 56, 1, 0, 0, 5, "group 1"),
    ("est", 5, 2, 0, 1, 13, "partial"), ("est", 7, 3, 0, 0, 13, "partial"),
    ("obs", 23, 1, 11, 0, 13, "group 1"), ("obs", 56, 1, 28, 0, 5, "above 48 KiB"), ("obs", 40, 3, 1, 0, 5, "group 1"),
    ("obs", 5, 2, 2, 0, 13, "partial"), ("obs", 7, 3, 3, 0, 13, "partial"),
]


def edge_cfgs(build, dense):
    """the tick, and the tick with backup plans: the widest image of the build (a plant of its own, w, v, ages, Ld, per-instance gains) once
    with and once without a fallback, then the narrowest"""
    if build == "plain":
        return [cfg("plain", K=0, fb=True), cfg("plain", K=2, fresh=1, fb=False), cfg("plain", K=2, fresh=0, fb=True), cfg("plain", plant="shared", w=False, fb=False)]
    if build == "est":
        return [cfg("est", dense=dense, per=1, K=2, fresh=1, fb=False), cfg("est", dense=dense, per=1, fb=True), cfg("est", plant="none", dense=dense, per=0, w=False, fb=False)]
    return [cfg("obs", K=2, fresh=1, fb=False), cfg("obs", fb=True), cfg("obs", plant="none", per=0, Ld=False, w=False, v=False, fb=False), cfg("obs", meas=True, per=0, K=2, fresh=0)]


@pytest.mark.parametrize("build,nx,nu,ny,dense,batch,edge", EDGES, ids=["%s-%d-%d-%d-%s" % (e[0], e[1], e[2], e[3], "dense" if e[4] else "diag") for e in EDGES])
def test_launch_edge_shapes_at_the_launch_group(emu, build, nx, nu, ny, dense, batch, edge):
    """the arithmetic at the group the launch itself picks, 256 threads: within the derived bounds, held instances bit for bit; the group and the
    copy (vec2 exactly when the group is even) are what the issue says of the shape; descending and permuted walks give the same bits"""
    group, one = launch_group(emu, build, nx, nu, ny, dense), image_bytes(emu, build, nx, nu, ny, dense)
    assert one <= emu["emu_plant_noise"].emu_plant_lds_max()
    if edge == "group 2":
        assert group == 2
    elif edge == "group 1":
        assert group == 1
    elif edge == "above 48 KiB":
        assert group == 1 and one > 48 * 1024
    else:
        assert group % 2 == 0 and batch % group != 0 and nx % 2 == 1
    c = make_case(nx, nu, ny, batch, seed=7 * nx + nu + ny, failed=2)
    worst = 0.0
    for g in edge_cfgs(build, dense):
        got = tick(emu, c, g, group, 256)
        assert got["vec2"] == (1 if group % 2 == 0 else 0), (g, group)
        worst = max(worst, check(c, g, got, (g, group)))
        for order, seed in ORDERS[1:3]:
            assert_same(got, tick(emu, c, g, group, 256, order, seed), (g, group, order))
    g = dict(edge_cfgs(build, dense)[0], noise=True)  # ... and with noise drawn: the guard, and x+ against the terms of noise_ref.py
    drawn = tick(emu, c, g, group, 256)
    assert drawn["rc"] == 0 and drawn["vec2"] == (1 if group % 2 == 0 else 0)
    if build == "plain":
        u, age = rule(c, g)
        moved = age != HELD
        tw = noise_ref.terms(NOISE_SEED, NOISE_FIRST, batch, c["sw"], NOISE_TICK, 0)
        ref, S = reference_step(c["own"][0], c["own"][1], c["own"][2], c["xp"], np.where(moved[:, None], u, 0.0), c["w"].astype(LD) + np.asarray(tw, dtype=LD))
        # (the drawn term is within noise_ref.TOL sigma of the reference's, and w + term is rounded once more before the sum)
        bound = step_bound(nx, nu, S) + (noise_ref.TOL * c["sw"] + 2.0 ** -53 * (np.abs(c["w"]) + np.abs(tw))) * (1 + step_bound(nx, nu, 1.0))
        err = np.abs(drawn["x"].astype(LD) - ref)
        assert (err[moved] <= bound[moved]).all(), float((err[moved] / bound[moved]).max())
        assert _same_bits(drawn["x"][~moved], c["xp"][~moved])
    print("%s (%d, %d, %d) %s: group %d, one instance %d B, max err / bound = %.3f" % (build, nx, nu, ny, "dense" if dense else "", group, one, worst))


# ---- 4: misaligned pointers ----
def inputs_of(g):
    """the arrays the launch looks at before it copies 16 bytes per lane (plant_vec2_ok, plant_obs_vec2_ok)"""
    names = ["x0"] if not g["meas"] else []
    if g["plant"] != "none":
        names += ["A", "B", "d"]
    if g["w"]:
        names.append("w")
    if g["build"] == "est":
        names += ["Am", "Bm", "gain", "dhat"]
    if g["build"] == "obs":
        names += ["Am", "Bm", "dhat", "xhat", "C", "Lx"] + (["Ld"] if g["Ld"] else []) + (["v"] if g["v"] or g["meas"] else [])
    return names


MISALIGNED = [cfg("plain"), cfg("plain", K=2, fresh=1), cfg("plain", plant="shared", fb=False), cfg("est", dense=1, per=1, K=2, fresh=1), cfg("est", dense=0, per=0, fb=False),
              cfg("est", plant="none", dense=1, per=0), cfg("obs", K=2, fresh=1), cfg("obs", plant="none", per=0, Ld=False, fb=False), cfg("obs", meas=True)]


@pytest.mark.parametrize("nx,nu,ny", SMALL[::-1])
def test_one_misaligned_array_gives_up_the_wide_copy_and_keeps_the_bits(emu, nx, nu, ny):
    """every input array in turn 8 bytes past a 16-byte boundary, at an even group: vec2 comes out 0 and every output is bit-identical to the
    all-aligned run (vec2 1) at that group.  control, plan and the fallback are not copied through the image's wide copy: misaligned they
    leave vec2 alone and change no bit either (phase 2 then moves the plans' tails double by double)"""
    c = make_case(nx, nu, ny, 13, seed=31 * nx + nu, failed=3)
    seen = set()
    for g0, noise in itertools.product(MISALIGNED, (False, True)):
        g = dict(g0, noise=noise)
        for group in sorted({2, launch_group(emu, g["build"], nx, nu, ny, g["dense"])}):
            want = tick(emu, c, g, group)
            assert want["vec2"] == 1 and want["rc"] == 0, (g, group)
            for name in inputs_of(g):
                got = tick(emu, c, g, group, mis=(name,))
                assert got["vec2"] == 0 and got["rc"] == 0, (g, group, name)
                assert_same(want, got, (g, group, name))
                seen.add(name)
            for name in ("control", "plan", "fb"):
                got = tick(emu, c, g, group, mis=(name,))
                assert got["vec2"] == 1 and got["rc"] == 0, (g, group, name)
                assert_same(want, got, (g, group, name))
    assert seen == {"x0", "A", "B", "d", "w", "Am", "Bm", "gain", "dhat", "xhat", "C", "Lx", "Ld", "v"}


# ---- 5: the geometry ----
NX = np.arange(1, 145)
NU = (1, 2, 3, 6)
# the order of emu_plant_layout's rows (emu_walk.h) and of its nine flags
BASE = ("A", "B", "d", "x", "w", "u", "st", "ag", "base_total")
PARTS = {0: BASE, 1: BASE + ("Am", "Bm", "dh", "G", "xn", "e", "total"),
         2: BASE + ("Am", "Bm", "dh", "xh", "C", "Lx", "Ld", "yv", "xn", "xp", "in", "total")}
FLAGS = ("shared", "has_w", "backup", "same_model", "gain_dense", "gain_shared", "meas", "has_Ld", "has_yv")
USED = {0: FLAGS[:3], 1: FLAGS[:6], 2: FLAGS[:4] + FLAGS[5:]}


def sweep(emu, kind, odd_group=0):
    """every (nx, nu, ny, flags) of the sweep as columns, with the launch's group (or odd_group) and the layout's offsets"""
    nys = (0,) if kind != 2 else (1, -2, -1)  # 1, nx / 2, nx
    flags = np.array([f for f in itertools.product((0, 1), repeat=9) if all(v == 0 for k, v in zip(FLAGS, f) if k not in USED[kind])], dtype=np.int32)
    rows = np.array(list(itertools.product(NX, NU, nys)), dtype=np.int32)
    rows[:, 2] = np.where(rows[:, 2] == -2, np.maximum(rows[:, 0] // 2, 1), np.where(rows[:, 2] == -1, rows[:, 0], rows[:, 2]))
    lib = emu["emu_plant_noise"]
    p = np.zeros((rows.shape[0], flags.shape[0], 13), dtype=np.int32)
    p[:, :, :3] = rows[:, None, :]
    p[:, :, 4:] = flags[None, :, :]
    p = p.reshape(-1, 13)
    col = {k: p[:, 4 + i].astype(np.int64) for i, k in enumerate(FLAGS)}
    nx, nu, ny = (p[:, i].astype(np.int64) for i in range(3))
    shapes = list(zip(nx.tolist(), nu.tolist(), ny.tolist(), col["gain_dense"].tolist()))
    ones = {t: lib.emu_plant_image_bytes(kind, *t) for t in set(shapes)}
    groups = {t: lib.emu_plant_launch_group(kind, *t) for t in set(shapes)}
    one = np.array([ones[t] for t in shapes], dtype=np.int64)
    p[:, 3] = odd_group if odd_group else [groups[t] for t in shapes]
    p = np.ascontiguousarray(p)
    out = np.zeros((p.shape[0], 24), dtype=np.int32)
    assert lib.emu_plant_layouts(kind, p.shape[0], p.ctypes.data, out.ctypes.data) == len(PARTS[kind])
    off = {k: out[:, i].astype(np.int64) for i, k in enumerate(PARTS[kind])}
    return nx, nu, ny, p[:, 3].astype(np.int64), col, one, off


def needs(kind, nx, nu, ny, group, f):
    """how many doubles the phase bodies put at each part of the image (0: the build has no such part, its offset means nothing): the counts
    of phase 1's copies and of the later phases' stores in plant_step.hpp -- what must fit, not how the layout pads it"""
    gs = np.where(f["shared"] == 1, 1, group)
    ints = (group + 1) // 2  # `group` ints
    n = dict(A=gs * nx * nx, B=gs * nx * nu, d=gs * nx, x=group * nx, w=f["has_w"] * group * nx, u=group * nu, st=ints, ag=f["backup"] * ints)
    if kind == 0:
        return n
    own = 1 - f["same_model"]
    n.update(Am=own * group * nx * nx, Bm=own * group * nx * nu, dh=own * group * nx)
    if kind == 1:
        n.update(G=np.where(f["gain_shared"] == 1, 1, group) * np.where(f["gain_dense"] == 1, nx * nx, nx), xn=group * nx, e=group * nx)
        return n
    gg = np.where(f["gain_shared"] == 1, 1, group)
    sim = 1 - f["meas"]
    n.update(xh=sim * group * nx, C=gg * ny * nx, Lx=gg * nx * ny, Ld=f["has_Ld"] * gg * nx * ny, yv=f["has_yv"] * group * ny, xn=sim * group * nx, xp=group * nx)
    n["in"] = group * ny
    return n


@pytest.mark.parametrize("kind", (0, 1, 2), ids=("plain", "est", "obs"))
def test_the_launch_geometry_swept(emu, kind):
    """nx 1 .. 144, nu 1, 2, 3, 6, ny 1, nx / 2, nx, every combination of the build's flags"""
    lib = emu["emu_plant_noise"]
    target, top, gmax = lib.emu_plant_lds_target(), lib.emu_plant_lds_max(), lib.emu_plant_group_max()
    assert (target, top, gmax) == (24 * 1024, 160 * 1024, 32)
    for odd_group in (0, 3):
        nx, nu, ny, group, f, one, off = sweep(emu, kind, odd_group)
        if not odd_group:
            assert (((group == 1) | (group % 2 == 0)) & (group >= 1) & (group <= gmax)).all()
            assert ((group == 1) | (group * one <= target)).all() and ((group == gmax) | ((group + 2) * one > target)).all()
            # the flags a launch can pass: without a plant of its own the model is never `shared`; measured outputs have no plant, no w and a y
            can = np.ones(nx.shape, dtype=bool)
            if kind >= 1:
                can &= ~((f["same_model"] == 1) & (f["shared"] == 1))
            if kind == 2:
                can &= ~((f["meas"] == 1) & ((f["same_model"] == 0) | (f["has_w"] == 1) | (f["has_yv"] == 0)))
            launched = 8 * off["total" if kind else "base_total"]
            assert (launched[can] <= np.maximum(target, one[can])).all()
            assert (launched[can & (one <= top)] <= top).all() and (one > top).any() and (8 * off["base_total"] > 48 * 1024).any()
        need = needs(kind, nx, nu, ny, group, f)
        total = off["total" if kind else "base_total"]
        names = [k for k in PARTS[kind] if k in need]
        assert set(names) == set(need)
        for k in names:  # every part starts on 16 bytes and ends inside the image
            there = need[k] > 0
            assert (off[k][there] % 2 == 0).all() and (off[k][there] >= 0).all() and ((off[k] + need[k])[there] <= total[there]).all(), k
        for a, b in itertools.combinations(names, 2):  # no two parts overlap
            both = (need[a] > 0) & (need[b] > 0)
            apart = (off[a] + need[a] <= off[b]) | (off[b] + need[b] <= off[a])
            assert apart[both].all(), (a, b, [v[both & ~apart][:1] for v in (nx, nu, ny, group)])
        assert (off["A"] == 0).all()


def test_every_emulator_exports_the_same_geometry(emu):
    """the functions are plant_step.hpp's own in each of the five libraries; the plain tick sizes its widest image WITH the ages"""
    ref = emu["emu_plant_noise"]
    shapes = [(0, 38, 1, 0, 0), (0, 77, 1, 0, 0), (1, 23, 1, 0, 1), (1, 23, 1, 0, 0), (2, 23, 1, 11, 0), (2, 6, 3, 3, 0), (0, 6, 3, 0, 0)]
    for lib in emu.values():
        for s in shapes:
            assert lib.emu_plant_launch_group(*s) == ref.emu_plant_launch_group(*s) and lib.emu_plant_image_bytes(*s) == ref.emu_plant_image_bytes(*s)
    assert ref.emu_plant_launch_group(2, 6, 3, 3, 0) == 12 and ref.emu_plant_launch_group(0, 6, 3, 0, 0) == 32
    p = np.array([[6, 3, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    out = np.zeros((1, 24), dtype=np.int32)
    ref.emu_plant_layouts(0, 1, p.ctypes.data, out.ctypes.data)
    assert 8 * int(out[0, 8]) == ref.emu_plant_image_bytes(0, 6, 3, 0, 0)  # (has_w and backup set: the image advance() checks)
