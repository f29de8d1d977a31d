"""The inputs of the score and target kernels at their launch edges, shared by tests/test_score_target_edges_emu.py (the kernels' bodies on
the host, bit for bit) and tests/test_score_target_edges_gpu.py (the device, within the bounds tests/test_score_abi.py and
tests/test_target_abi.py derive): one definition of every case, so that a case which passes on the host and fails on the device is a fault
of the device side -- addressing, the dynamic-LDS opt-in, the grid, a contraction -- and not of the arithmetic.

Models: scenario() of tests/test_tick_edges_gpu.py (per-instance random A, B, d; the last state decoupled and bounded, two instances held
at every tick; the cheapest controller that can be created at every shape).  measure(): a closed-loop measure for any shape.
target_case(): H, a setpoint signal, the step maps of the controller's costs, planted singular instances.  The launch geometry is asked of
the emulators' exports (score_step.hpp's and target_step.hpp's own functions), never restated."""
import collections
import ctypes
import os
import subprocess

import numpy as np

import score_ref
import target_ref
from test_score_abi import MEASURE, Tick
from test_target_abi import Run
from test_tick_edges_gpu import scenario

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
HELD = score_ref.HELD
KIB48 = 48 * 1024
CI, LL, VP = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p

Geo = collections.namedtuple("Geo", "score target")


def build_emulators(tmp):
    """tests/emu/emu_score.cpp and emu_target.cpp as shared libraries (every product and every sum rounded), their exports typed"""
    libs = []
    for name in ("score", "target"):
        so = os.path.join(str(tmp), "libemu_%s.so" % name)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(EMU, "emu_%s.cpp" % name), "-o", so])
        libs.append(ctypes.CDLL(so))
    s, t = libs
    s.emu_score_tick.restype, s.emu_score_tick.argtypes = CI, [ctypes.POINTER(Tick)]
    s.emu_score_image_bytes.restype, s.emu_score_image_bytes.argtypes = LL, [CI] * 3
    s.emu_score_launch_group.restype, s.emu_score_launch_group.argtypes = CI, [CI] * 3
    s.emu_score_layout.restype, s.emu_score_layout.argtypes = CI, [CI, CI, CI, VP, VP]
    t.emu_target_run.restype, t.emu_target_run.argtypes = CI, [ctypes.POINTER(Run)]
    t.emu_target_image_bytes.restype, t.emu_target_image_bytes.argtypes = LL, [CI] * 3
    t.emu_target_launch_group.restype, t.emu_target_launch_group.argtypes = CI, [CI] * 3
    t.emu_target_layout.restype, t.emu_target_layout.argtypes = CI, [CI, CI, CI, CI, VP]
    t.emu_target_lds_max.restype = LL
    return Geo(s, t)


# ---- the score: a measure for any shape ----
def measure(nx, nu, batch=None, dense=False, steps=1, seed=0, leave=()):
    """the generalisation of test_score_gpu._com_measure: weights near the identity on the states and 1e-3 on the controls (diagonal, or
    full symmetric when dense), a reference signal of `steps` rows, a state box of about 1.5 with one infinite entry and a control box of
    about 0.05 -- boxes a closed loop from states of unit size crosses on some ticks and not on others; batch: every array per instance;
    leave: the arrays the caller does not hand over (they stay in the dict, given() takes them out)"""
    rng = np.random.default_rng(seed)
    lead = () if batch is None else (batch,)
    sym = lambda a: a + np.swapaxes(a, -1, -2)  # noqa: E731
    m = dict(nx=nx, nu=nu, dense=dense, per=batch is not None, tol=1e-9, steps=steps, leave=tuple(leave))
    if dense:
        m["qx"] = np.eye(nx) + 0.05 / np.sqrt(nx) * sym(rng.standard_normal(lead + (nx, nx)))
        m["ru"] = 1e-3 * np.eye(nu) + 1e-4 * sym(rng.standard_normal(lead + (nu, nu)))
    else:
        m["qx"] = rng.uniform(0.5, 1.5, lead + (nx,))
        m["ru"] = 1e-3 * rng.uniform(0.5, 1.5, lead + (nu,))
    m["x_ref"] = 0.1 * rng.standard_normal(lead + (steps, nx))
    m["x_lo"], m["x_hi"] = -1.5 * rng.uniform(0.8, 1.2, lead + (nx,)), 1.5 * rng.uniform(0.8, 1.2, lead + (nx,))
    m["x_lo"][..., 0] = -np.inf
    m["u_lo"], m["u_hi"] = -0.05 * rng.uniform(0.8, 1.2, lead + (nu,)), 0.05 * rng.uniform(0.8, 1.2, lead + (nu,))
    assert not set(leave) - set(MEASURE)
    return m


def given(m):
    """the measure as the caller hands it over: the left-out arrays None"""
    return dict(m, **{k: None for k in m["leave"]})


def tiled(m, batch):
    """a measure given once, written out per instance: the same values through the per-instance paths (the gather of the reference row)"""
    assert not m["per"]
    return dict(m, per=True, **{k: np.ascontiguousarray(np.broadcast_to(m[k], (batch,) + m[k].shape)) for k in MEASURE})


def score_geometry(geo, m):
    """what launch_score decides for measure m: dict(group, bytes: the image the launch asks for, one: an instance's widest image); every
    part of that image starts on 16 bytes (what the paired LDS accesses and the records need)"""
    g = given(m)
    nx, nu, dense = m["nx"], m["nu"], int(m["dense"])
    group = geo.score.emu_score_launch_group(nx, nu, dense)
    flags = np.asarray([dense, int(m["per"])] + [int(g[k] is not None) for k in MEASURE], dtype=np.int32)
    out = np.zeros(14, dtype=np.int32)
    assert geo.score.emu_score_layout(nx, nu, group, flags.ctypes.data, out.ctypes.data) == 14
    assert (out % 2 == 0).all(), out
    return dict(group=group, bytes=8 * int(out[13]), one=int(geo.score.emu_score_image_bytes(nx, nu, dense)))


def synthetic_history(S, ticks, seed=3):
    """histories of the shape a rollout returns, from the scenario's own model and random controls: the held instances never move, their
    controls are NaN and their age HELD -- what the emulator scores where no device gives a history"""
    wl, batch = S["wl"], S["batch"]
    rng = np.random.default_rng(seed)
    held = np.zeros(batch, dtype=bool)
    held[list(S["held"])] = True
    x = wl["x0"].copy()
    xs, us, ages = [x.copy()], [], []
    for _ in range(ticks):
        u = 0.1 * rng.standard_normal((batch, wl["B"].shape[2]))
        xn = np.einsum("bij,bj->bi", wl["A"], x) + np.einsum("bij,bj->bi", wl["B"], u) + wl["d"]
        xn[held], u[held] = x[held], np.nan
        x = xn
        xs.append(x.copy()), us.append(u), ages.append(np.where(held, HELD, 0).astype(np.int32))
    return dict(x_hist=np.stack(xs), u_hist=np.stack(us), age_hist=np.stack(ages), status_hist=np.stack([held.astype(np.int32)] * ticks))


def reference_rows(m, ticks, tau0=0):
    """the row of the reference signal every tick of a rollout reads (the schedule tick AFTER the tick)"""
    return [min(tau0 + t + 1, m["steps"] - 1) for t in range(ticks)]


def first_beyond(geo, nu, dense, top):
    """the first nx whose widest image passes `top` bytes"""
    bad = next(n for n in range(2, 4000) if geo.score.emu_score_image_bytes(n, nu, dense) > top)
    assert geo.score.emu_score_image_bytes(bad - 1, nu, dense) <= top
    return bad


# ---- the targets ----
def _even(v):
    return (v + 1) & ~1


def pivot_orders(M):
    """the rows partial pivoting picks, per instance, by a plain restatement of the elimination: the largest |entry| of column k among
    rows k .. n - 1, ties to the lowest row (argmax returns the first)"""
    out = []
    with np.errstate(all="ignore"):
        for W in np.array(M, dtype=np.float64):
            n, order = W.shape[0], []
            for k in range(n):
                p = k + int(np.argmax(np.abs(W[k:, k])))
                order.append(p)
                W[[k, p]] = W[[p, k]]
                W[k + 1:] -= np.outer(W[k + 1:, k] / W[k, k], W[k])
            out.append(tuple(order))
    return out


def eight_costs(nx, nu, N, rows0):
    """eight costs whose reference has S_c = 1, N and N + 1 blocks (per-step entries and full-size entries of one repeating block), odd and
    even r_c S_c; rows0: the rows of cost 0.  Returns (cost dicts, [(r_c, S_c)])"""
    rng = np.random.default_rng(31)
    rn = lambda r, c: rng.standard_normal((r, c)) / np.sqrt(c)  # noqa: E731
    full = lambda blk, S: np.kron(np.eye(S), blk)  # noqa: E731
    shapes = [(rows0, 1), (nu, N), (5, N + 1), (5, 1), (4, 1), (nu, 1), (nx, N + 1), (2, N)]
    w = lambda r, S: [1.0] * (r * S)  # noqa: E731
    p = lambda r, S: 0.1 * rng.standard_normal(r * S)  # noqa: E731
    costs = [dict(kind="trajectory", M=rn(rows0, nx), p=p(rows0, 1), weights=w(rows0, 1)),
             dict(kind="control", N=full(np.eye(nu), N), p=p(nu, N), weights=w(nu, N)),
             dict(kind="trajectory", M=full(rn(5, nx), N + 1), p=p(5, N + 1), weights=w(5, N + 1)),
             dict(kind="target", M=rn(5, nx), p=p(5, 1), weights=w(5, 1)),
             dict(kind="mixed", M=rn(4, nx), N=rn(4, nu), p=p(4, 1), weights=w(4, 1)),
             dict(kind="control", N=0.5 * np.eye(nu), p=p(nu, 1), weights=w(nu, 1)),
             dict(kind="trajectory", M=full(np.eye(nx), N + 1), p=p(nx, N + 1), weights=w(nx, N + 1)),
             dict(kind="control", N=full(rn(2, nu), N), p=p(2, N), weights=w(2, N))]
    return costs, shapes


def target_case(nx, nu, batch, N=1, per=False, steps=1, offset=0, costs=None, blocks=None):
    """the scenario of the shape with H, a setpoint signal and the step maps of its costs.  costs / blocks: another list of costs and their
    S_c (eight_costs); else the scenario's two, S_c = 1.  The dict also serves test_target_abi.run / check (z0 / out0: what the device
    holds before its first launch -- zeros, and the references given at creation)"""
    S = scenario(nx, nu, 0, N, 1, batch=batch)
    wl = S["wl"]
    if costs is not None:
        wl["costs"] = costs
    H = np.random.default_rng(7 * nx + nu).standard_normal((nu, nx))
    sig = np.random.default_rng(100 * nx + nu + batch).standard_normal(((batch,) if per else ()) + (steps, nu))
    maps = [target_ref.step_map(c, nx, nu, N)[0] for c in wl["costs"]]
    blocks = [1] * len(maps) if blocks is None else list(blocks)
    c = dict(wl=wl, nx=nx, nu=nu, batch=batch, N=N, H=H, r=sig, per=per, steps=steps, offset=offset, maps=maps, planted=())
    c["costs"] = list(zip(maps, blocks))
    c["A"], c["B"], c["d"] = wl["A"], wl["B"], wl["d"]  # (the same arrays: plant() below changes both views)
    c["z0"] = np.zeros((batch, nx + nu))
    c["out0"] = [np.tile(np.asarray(k["p"], dtype=np.float64), (batch, 1)) for k in wl["costs"]]
    assert all(o.shape[1] == T.shape[0] * s for o, (T, s) in zip(c["out0"], c["costs"]))
    return c


def map_doubles(c):
    return sum(_even(T.shape[0] * (c["nx"] + c["nu"])) for T in c["maps"])


def target_geometry(geo, c):
    """what launch_target decides for case c: dict(group, bytes: one wave's image -- the launch's own at group 64, top: the LDS limit);
    every part of the launch's image starts on 16 bytes"""
    maps = map_doubles(c)
    group, out = geo.target.emu_target_launch_group(c["nx"], c["nu"], maps), (CI * 5)()
    assert geo.target.emu_target_layout(c["nx"], c["nu"], group, maps, out) == 5 and all(v % 2 == 0 for v in out), list(out)
    return dict(group=group, bytes=int(geo.target.emu_target_image_bytes(c["nx"], c["nu"], maps)),
                top=int(geo.target.emu_target_lds_max()))


def plant(c, group):
    """singular instances among the good ones: a zero column of B at index 2, a NaN in d at index == group, a zero column of B in the last
    instance of the batch"""
    nu, batch = c["nu"], c["batch"]
    assert 2 < group < batch - 1
    c["B"][2][:, nu - 1] = 0.0
    c["d"][group][0] = np.nan
    c["B"][batch - 1][:, 0] = 0.0
    c["planted"] = (2, group, batch - 1)
    return c


def target_preconditions(c, what):
    """what must be true of the inputs, on the reference alone: numpy's float64 solve inside the bound, cond_inf(M) <= 1e6, the rule's
    status 0 everywhere except the planted instances, at least three different pivot orders among the first 64 instances.  Returns
    (largest cond, numpy error / bound, distinct pivot orders)"""
    r = target_ref.setpoint(c["r"], 0, c["offset"], c["batch"])
    M, rhs = target_ref.systems(c["A"], c["B"], c["d"], c["H"], r)
    want = np.zeros(c["batch"], dtype=np.int32)
    want[list(c["planted"])] = 1
    _, status = target_ref.gepp(M, rhs)
    assert np.array_equal(status, want), (what, np.nonzero(status != want)[0][:8])
    good = status == 0
    cond = target_ref.cond_inf(M[good])
    assert cond.max() <= 1e6, (what, cond.max())
    zt = target_ref.solve_true(M[good], rhs[good])
    bound = target_ref.z_bound(M[good], zt)
    e64 = np.abs(target_ref.solve64(M[good], rhs[good]) - zt).max(axis=1).astype(np.float64)
    assert (e64 <= bound).all(), (what, float((e64 / bound).max()))
    orders = set(pivot_orders(M[:64][good[:64]]))
    assert len(orders) >= 3, (what, orders)
    print("%s: cond_inf(M) <= %.3g, numpy error / bound %.3g, %d pivot orders among the first 64" % (what, cond.max(), float((e64 / bound).max()), len(orders)))
    return float(cond.max()), float((e64 / bound).max()), len(orders)


# ---- the cases: one table for the host and the device ----
def _s(name, nx, nu, batch, N, ticks, dense, per, steps=1, leave=()):
    return dict(id=name, nx=nx, nu=nu, batch=batch, N=N, ticks=ticks, dense=dense, per=per, steps=steps, leave=tuple(leave))


LIMITS = ("x_lo", "x_hi", "u_lo", "u_hi")
S1 = [_s("S1 dense per (40, 1)", 40, 1, 5, 1, 3, True, True)]
S2 = [_s("S2 dense shared (78, 1)", 78, 1, 5, 1, 2, True, False), _s("S2 dense per (78, 1)", 78, 1, 5, 1, 2, True, True)]
S3 = [_s("S3 dense per (23, 1)", 23, 1, 13, 1, 3, True, True), _s("S3 diagonal shared (40, 1)", 40, 1, 13, 1, 3, False, False),
      _s("S3 dense per (9, 3)", 9, 3, 33, 2, 3, True, True)]
S4 = [_s("S4 diagonal (5, 2)", 5, 2, 13, 2, 6, False, False, steps=3), _s("S4 dense (9, 3)", 9, 3, 13, 2, 6, True, False, steps=3)]
S5 = [_s("S5 qx alone", 5, 2, 13, 2, 3, False, False, leave=("ru", "x_ref") + LIMITS),
      _s("S5 the control box alone", 5, 2, 13, 2, 3, False, True, leave=("qx", "ru", "x_ref", "x_lo", "x_hi")),
      _s("S5 dense qx and x_ref, no limits", 5, 2, 13, 2, 3, True, True, steps=2, leave=("ru",) + LIMITS)]


def score_case(case, nx=None):
    """(scenario, measure) of a row of the tables above, at another nx where the launch rule has moved"""
    nx = case["nx"] if nx is None else nx
    S = scenario(nx, case["nu"], 0, case["N"], case["ticks"], batch=case["batch"])
    m = measure(nx, case["nu"], case["batch"] if case["per"] else None, case["dense"], case["steps"], seed=10 * nx + case["nu"], leave=case["leave"])
    return S, m


def largest_nx(nx, keeps, what):
    """the largest nx' <= nx that keeps the case's property (the named nx at HEAD)"""
    for n in range(nx, 1, -1):
        if keeps(n):
            if n != nx:
                print("%s: nx stepped down from %d to %d" % (what, nx, n))
            return n
    raise AssertionError("%s: no shape keeps the property" % what)


def score_property(geo, case):
    """keeps(nx) of a case, from the geometry alone: S1 group 1; S2 the launch's image above 48 KiB; S3 a small even group, more than one
    workgroup and a partial last one; the others none"""
    def G(n):
        return score_geometry(geo, score_case(dict(case, ticks=1), n)[1])
    tag = case["id"][:2]
    if tag == "S1":
        return lambda n: G(n)["group"] == 1
    if tag == "S2":
        return lambda n: G(n)["bytes"] > KIB48
    if tag == "S3":
        return lambda n: 2 <= G(n)["group"] <= 16 and G(n)["group"] % 2 == 0 and case["batch"] > G(n)["group"] and case["batch"] % G(n)["group"] != 0
    return lambda n: True


def _t(name, nx, nu, batch, N=1, per=False, steps=1, offset=0):
    return dict(id=name, nx=nx, nu=nu, batch=batch, N=N, per=per, steps=steps, offset=offset)


T1 = [_t("T1 (3, 2) x 513", 3, 2, 513), _t("T1 (4, 2) x 257", 4, 2, 257, per=True, steps=3, offset=1), _t("T1 (6, 1) x 257", 6, 1, 257),
      _t("T1 (6, 3) x 129", 6, 3, 129, per=True, steps=3, offset=1)]
T2 = [_t("T2 (14, 3) x 65", 14, 3, 65), _t("T2 (13, 3) x 65", 13, 3, 65)]
T4 = [_t("T4 (5, 2) x 14", 5, 2, 14, N=2, steps=3, offset=1), _t("T4 (6, 3) x 14", 6, 3, 14, N=2, per=True, steps=3, offset=1)]


def target_of(case):
    return target_case(case["nx"], case["nu"], case["batch"], N=case["N"], per=case["per"], steps=case["steps"], offset=case["offset"])


def eight_cost_case(geo):
    """T3: (6, 3) x 70, N = 2, eight driven costs; the rows of cost 0 stepped up until the maps push one wave's image above 48 KiB"""
    nx, nu, batch, N = 6, 3, 70, 2
    for rows0 in range(9, 64):
        costs, shapes = eight_costs(nx, nu, N, rows0)
        c = target_case(nx, nu, batch, N=N, costs=costs, blocks=[s for _, s in shapes])
        if target_geometry(geo, c)["bytes"] > KIB48:
            return c, shapes
    raise AssertionError("T3: the maps never pass 48 KiB")
