"""Ensemble traces (copra_batch_set_trace, ABI 17) without a GPU: declared, exported, bound -- and the slot, the vmax rule and the order of the
reduction on the kernel's own bodies (copra_amd/csrc/trace_step.hpp), which compile on the host: tests/emu/emu_trace.cpp walks stage 1's copy
thread by thread over a NaN-filled image with the guard and the walk orders of tests/emu/emu_walk.h, takes every thread's own fold, applies
the tree lane by lane and runs stage 2 over the partials; this file compiles that harness itself (-ffp-contract=off).  The expectation is
tests/trace_ref.py, bit for bit on every byte of the slot.  Against numpy's longdouble, mean and m2 are held to summary_bounds of
tests/test_score_abi.py (derived there for this very merge), at the depth merge_depth gives for the instance count."""
import ctypes
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import score_ref
import trace_ref
from test_score_abi import merge_depth, summary_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
NEW = ("copra_trace_init", "copra_batch_set_trace", "copra_batch_trace_reset", "copra_batch_trace_info", "copra_batch_trace_device", "copra_batch_get_trace")
TRACE_FIELDS = ["struct_size", "capacity", "what", "every", "x_lo", "x_hi", "u_lo", "u_hi", "tol", "on_device"]
HEAD_FIELDS = ["tick", "tau", "solved", "replayed", "fallback", "held", "violating", "reserved"]
SHAPES = [(6, 3), (3, 1), (1, 1), (5, 2)]
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
VP, CI, LL, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong
HELD, FALLBACK = score_ref.HELD, score_ref.FALLBACK


def _lib():
    from copra_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_capi.LIB_PATH)


# ---- surface ----
def _struct_fields(code, name):
    end = code.index("} %s;" % name)
    body = code[code.rindex("typedef struct {", 0, end):end]
    out = []
    for m in re.finditer(r"\b(?:const\s+)?(?:long\s+long|double|int)\s*\*?\s*([^;]+);", body):
        out += [n.strip().lstrip("*") for n in m.group(1).split(",")]
    return out


def test_header_declares_the_traces():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert _struct_fields(code, "copra_trace_t") == TRACE_FIELDS
    assert _struct_fields(code, "copra_trace_head_t") == HEAD_FIELDS
    for name, bit in (("COPRA_TRACE_X", 1), ("COPRA_TRACE_U", 2), ("COPRA_TRACE_ERR", 4)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, bit), code), name
    assert re.search(r"copra_batch_set_trace\s*\(\s*copra_batch_t\s*\*\s*\w*\s*,\s*const\s+copra_trace_t\s*\*\s*\w*\s*\)", code)
    assert re.search(r"copra_batch_get_trace\s*\(\s*copra_batch_t\s*\*\s*\w*\s*,\s*long\s+long\s+\w*\s*,\s*long\s+long\s+\w*\s*,\s*void\s*\*\s*\w*\s*\)", code)
    section = text[text.index("ensemble traces"):text.index("#define COPRA_TRACE_X")]
    assert "instances 1024 c + t, + 256, + 512, + 768 in ascending order" in section and "lane l <- merge(lane l, lane l + off)" in section  # (the order is written down)
    assert "64 + 56 rows" in section


def test_library_exports_the_traces_with_abi_17():
    lib = _lib()
    for name in NEW:
        assert hasattr(lib, name), name
    lib.copra_abi_version.restype = CI
    assert lib.copra_abi_version() >= 17
    from copra_amd import _capi
    lib.copra_batch_set_trace.restype = CI
    lib.copra_batch_set_trace.argtypes = [VP, VP]
    lib.copra_batch_trace_reset.restype = CI
    lib.copra_batch_trace_reset.argtypes = [VP]
    lib.copra_batch_trace_info.restype = CI
    lib.copra_batch_trace_info.argtypes = [VP, VP, VP, VP, VP]
    lib.copra_batch_trace_device.restype = VP
    lib.copra_batch_trace_device.argtypes = [VP]
    lib.copra_batch_get_trace.restype = CI
    lib.copra_batch_get_trace.argtypes = [VP, LL, LL, VP]
    room = np.zeros(64)
    # (a NULL handle is refused before anything touches a device: the first line of the error table; the rest runs in tests/test_trace_gpu.py)
    assert lib.copra_batch_set_trace(None, None) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_set_trace(None, room.ctypes.data) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_trace_reset(None) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_trace_info(None, room.ctypes.data, None, None, None) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_get_trace(None, 0, 0, room.ctypes.data) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_trace_device(None) is None


def test_struct_sizes(emu):
    from copra_amd import _capi
    lib = _lib()
    assert [n for n, _ in _capi.Trace._fields_] == TRACE_FIELDS
    assert [n for n, _ in _capi.TraceHead._fields_] == HEAD_FIELDS
    assert ctypes.sizeof(_capi.TraceHead) == 64 == _capi.TRACE_HEAD_DTYPE.itemsize == trace_ref.HEAD.itemsize
    assert ctypes.sizeof(_capi.ScoreStat) == 56 == _capi.SCORE_STAT_DTYPE.itemsize == trace_ref.STAT.itemsize
    assert list(_capi.TRACE_HEAD_DTYPE.names) == HEAD_FIELDS == list(trace_ref.HEAD.names)
    assert list(_capi.SCORE_STAT_DTYPE.names) == [n for n, _ in _capi.ScoreStat._fields_] == list(trace_ref.STAT.names)
    head, stat = CI(), CI()
    emu.emu_trace_sizes(ctypes.byref(head), ctypes.byref(stat))
    assert (head.value, stat.value) == (64, 56)
    for rows in (1, 2, 16, 31):
        assert _capi.trace_slot_dtype(rows).itemsize == 64 + 56 * rows == trace_ref.slot_dtype(rows).itemsize == emu.emu_trace_slot_bytes(rows)
    assert (_capi.TRACE_X, _capi.TRACE_U, _capi.TRACE_ERR) == (trace_ref.X, trace_ref.U, trace_ref.ERR) == (1, 2, 4)
    for what, limits in itertools.product(range(1, 8), (0, 1)):
        assert emu.emu_trace_rows(what, 6, 3, limits) == trace_ref.rows_of(what, 6, 3, limits)
    assert trace_ref.rows_of(7, 6, 3, True) == 16
    m = _capi.Trace()
    ctypes.memset(ctypes.byref(m), 0xff, ctypes.sizeof(m))
    lib.copra_trace_init.restype = None
    lib.copra_trace_init.argtypes = [ctypes.POINTER(_capi.Trace)]
    lib.copra_trace_init(ctypes.byref(m))
    assert m.struct_size == ctypes.sizeof(_capi.Trace) == 72
    assert not any(getattr(m, f) for f in TRACE_FIELDS[1:])


def test_python_binding_has_the_traces():
    from copra_amd import BatchLMPC, sharding
    for name in ("set_trace", "reset_trace", "trace_info", "trace"):
        assert callable(getattr(BatchLMPC, name, None)), name
    assert isinstance(inspect.getattr_static(BatchLMPC, "trace_ptr"), property)
    p = inspect.signature(BatchLMPC.set_trace).parameters
    assert list(p)[1:] == ["capacity", "state", "control", "estimate_error", "state_limits", "control_limits", "tol", "every"]
    assert (p["state"].default, p["control"].default, p["estimate_error"].default, p["tol"].default, p["every"].default) == (True, True, False, 0.0, 1)
    assert p["state_limits"].default is None and p["control_limits"].default is None
    assert list(inspect.signature(sharding.merge_traces).parameters) == ["traces", "first_instances"]


# ---- the kernel bodies on the host ----
class Tick(ctypes.Structure):
    """EmuTraceTick of tests/emu/emu_trace.h"""
    _fields_ = ([(n, CI) for n in ("batch", "nx", "nu", "what", "order", "lds_mode", "vec2_mode")] + [("seed", U64)]
                + [(n, VP) for n in ("x", "u", "est", "age", "x_lo", "x_hi", "u_lo", "u_hi")] + [("tol", ctypes.c_double), ("tick", LL), ("tau", LL), ("slot", VP)]
                + [(n, CI) for n in ("rows", "lds_doubles", "lds_used", "vec2_used")])


class Clock(ctypes.Structure):
    """EmuTraceClock of tests/emu/emu_trace.h"""
    _fields_ = [("tick", LL), ("recorded", LL), ("missed", LL), ("capacity", LL), ("every", CI)]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_trace") / "libemu_trace.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(EMU, "emu_trace.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_trace_tick.restype = CI
    lib.emu_trace_tick.argtypes = [ctypes.POINTER(Tick)]
    lib.emu_trace_record.restype = LL
    lib.emu_trace_record.argtypes = [ctypes.POINTER(Tick), ctypes.POINTER(Clock), VP]
    lib.emu_trace_stage2.restype = CI
    lib.emu_trace_stage2.argtypes = [CI, LL, VP, LL, LL, VP]
    lib.emu_trace_rows.argtypes = [CI] * 4
    lib.emu_trace_slot_bytes.restype = LL
    lib.emu_trace_slot_bytes.argtypes = [CI]
    lib.emu_trace_in_lds.argtypes = [CI] * 5
    lib.emu_trace_sizes.argtypes = [VP, VP]
    return lib


LIMITS = ("x_lo", "x_hi", "u_lo", "u_hi")


def _case(nx, nu, batch, seed, ages=(0, 2, FALLBACK, HELD), held_u=np.nan):
    """one tick's states, controls, estimates and ages -- the four ages drawn at random, `held_u` in the held instances' controls -- and
    limits, infinite entries among the finite ones, that a good share of the batch violates"""
    rng = np.random.default_rng(seed)
    c = dict(nx=nx, nu=nu, batch=batch)
    c["x"], c["u"], c["est"] = 1.5 * rng.standard_normal((batch, nx)), 1.5 * rng.standard_normal((batch, nu)), 1.5 * rng.standard_normal((batch, nx))
    c["age"] = rng.choice(np.asarray(ages, dtype=np.int32), batch).astype(np.int32)
    c["u"][c["age"] == HELD] = held_u
    c["x_lo"], c["x_hi"] = rng.uniform(-2.5, -1.5, nx), rng.uniform(1.5, 2.5, nx)
    c["u_lo"], c["u_hi"] = rng.uniform(-2.5, -1.5, nu), rng.uniform(1.5, 2.5, nu)
    c["x_hi"][0] = np.inf
    c["u_lo"][nu - 1] = -np.inf
    return c


def _tick(c, what, limits=LIMITS, live=True, tick=3, tau=4, tol=0.25, order=0, seed=1, lds_mode=-1, vec2_mode=-1, misalign=()):
    keep = {k: np.ascontiguousarray(c[k]) for k in ("x", "u", "est", "age") + tuple(limits)}
    for k in misalign:
        room = np.zeros(keep[k].size + 3)
        off = next(o for o in (1, 2) if (room.ctypes.data + 8 * o) % 16 == 8)
        room[off:off + keep[k].size] = keep[k].reshape(-1)
        keep[k] = room[off:off + keep[k].size].reshape(keep[k].shape)
    T = Tick()
    T.batch, T.nx, T.nu, T.what, T.order, T.lds_mode, T.vec2_mode, T.seed = c["batch"], c["nx"], c["nu"], what, order, lds_mode, vec2_mode, seed
    T.x, T.u, T.age = keep["x"].ctypes.data, keep["u"].ctypes.data, keep["age"].ctypes.data
    T.est = keep["est"].ctypes.data if live else None
    for k in limits:
        setattr(T, k, keep[k].ctypes.data)
    T.tol, T.tick, T.tau = tol, tick, tau
    return T, keep


def run(emu, c, what, **kw):
    """one recorded tick of case c on the emulator: (the slot as a 0-d structured array, the Tick with its outputs)"""
    T, keep = _tick(c, what, **kw)
    rows = trace_ref.rows_of(what, c["nx"], c["nu"], bool(kw.get("limits", LIMITS)))
    slot = np.zeros((), dtype=trace_ref.slot_dtype(rows))
    T.slot = slot.ctypes.data
    assert emu.emu_trace_tick(ctypes.byref(T)) == 0  # (-2: the guard behind the image was touched)
    assert T.rows == rows
    return slot, T


def ref(c, what, limits=LIMITS, live=True, tick=3, tau=4, tol=0.25):
    lim = {k: c[k] for k in limits}
    return trace_ref.slot(tick, tau, what, c["x"], c["u"], c["age"], est=c["est"] if live else None, tol=tol, **lim)


def _same(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("nx,nu", SHAPES)
def test_every_what_with_and_without_limits_equals_the_rule(emu, nx, nu):
    """every non-empty `what`, with all limits, with one side only and with none, with an estimate and without: every byte of the slot; batch
    65 (two waves, one of them one lane) and an odd share of held instances"""
    c = _case(nx, nu, 65, seed=100 * nx + nu)
    for what, limits, live in itertools.product(range(1, 8), (LIMITS, ("x_hi",), ("u_lo", "u_hi"), ()), (True, False)):
        got, _ = run(emu, c, what, limits=limits, live=live)
        want = ref(c, what, limits=limits, live=live)
        assert _same(got, want), (what, limits, live, got, want)
        h = got["head"]
        assert (h["tick"], h["tau"], h["reserved"]) == (3, 4, 0) and h["solved"] + h["replayed"] + h["fallback"] + h["held"] == 65
        if limits == LIMITS:
            assert 0 < h["violating"] < 65 and got["stat"][-1]["max"] > 0.25
        if not limits:
            assert h["violating"] == 0
        if what & 4 and not live:  # no estimate on this tick: the err rows are empty statistics
            at = (nx if what & 1 else 0) + (nu if what & 2 else 0)
            for s in got["stat"][at:at + nx]:
                assert (s["n"], s["mean"], s["m2"], s["min"], s["max"], s["argmin"], s["argmax"]) == (0, 0.0, 0.0, np.inf, -np.inf, -1, -1)


@pytest.mark.parametrize("nx,nu", SHAPES)
def test_instance_counts_around_a_wave_a_workgroup_and_a_chunk(emu, nx, nu):
    """all three groups and the viol row at every instance count at which the fold, the tree or the chunks change; the same bytes as the rule,
    and n, min, max, args exact and mean, m2 within the summary's bound of numpy's longdouble"""
    worst = 0.0
    for count in COUNTS:
        c = _case(nx, nu, count, seed=7 * count + nx)
        got, T = run(emu, c, 7)
        assert _same(got, ref(c, 7)), count
        assert T.lds_used == 1 and T.lds_doubles == 1024 * (2 * nx + nu) + 512
        with np.errstate(invalid="ignore"):
            vals = trace_ref.values(7, c["x"], c["u"], c["age"], c["est"], c["x_lo"], c["x_hi"], c["u_lo"], c["u_hi"])
        for r in range(vals.shape[0]):
            worst = max(worst, trace_ref.check_stat(got["stat"][r], vals[r], lambda v: summary_bounds(v, merge_depth(count)), (count, r)))
        want = trace_ref.counts(c["age"], vals[-1], 0.25)
        assert all(got["head"][k] == want[k] for k in trace_ref.COUNTS)
    print("(%d, %d): largest error / bound of mean and m2 against longdouble %.3g" % (nx, nu, worst))


def test_stage_two_alone_on_more_partials_than_threads(emu):
    """257 and 513 synthetic partials: thread t folds partials t, t + 256, t + 512 before the tree"""
    rng = np.random.default_rng(3)
    for chunks, rows in ((257, 2), (513, 3), (1, 1)):
        part = np.zeros(chunks, dtype=trace_ref.slot_dtype(rows))
        stats = [[None] * chunks for _ in range(rows)]
        for i, r in itertools.product(range(chunks), range(rows)):
            s = score_ref.stat_merge(score_ref.stat_one(rng.standard_normal(), 2 * i), score_ref.stat_one(rng.standard_normal() if (i + r) % 5 else np.nan, 2 * i + 1))
            if (i + r) % 11 == 0:
                s = score_ref.stat_empty()
            stats[r][i] = s
            for f in trace_ref.STAT.names:
                part["stat"][i, r][f] = s[f]
        counts = rng.integers(0, 1000, (chunks, 5))
        words = part.view(np.int64).reshape(chunks, -1)
        # a partial keeps its counts in its first 56 bytes in the order of ScoreCounts: solved (ticks), held, replayed, fallback, violating, 0, 0
        words[:, 0:5] = counts
        slot = np.zeros((), dtype=trace_ref.slot_dtype(rows))
        assert emu.emu_trace_stage2(rows, chunks, part.ctypes.data, 12, 13, slot.ctypes.data) == 0
        for r in range(rows):
            want = trace_ref.reduce_parts(stats[r])
            for f in trace_ref.STAT.names:
                assert np.asarray(slot["stat"][r][f]).tobytes() == np.asarray(want[f], dtype=trace_ref.STAT[f]).tobytes(), (chunks, r, f)
        h = slot["head"]
        assert (h["tick"], h["tau"], h["reserved"]) == (12, 13, 0)
        assert [h[k] for k in ("solved", "held", "replayed", "fallback", "violating")] == counts.sum(axis=0).tolist()


def test_a_nan_state_and_an_all_held_batch(emu):
    """a NaN state is counted out of its row alone and counts 0 in vmax; the held instances' u is never read -- NaN or any finite bits give the
    same slot --; an all-held batch has empty u rows"""
    c = _case(6, 3, 300, seed=5)
    c["x"][17, 2] = np.nan
    c["x"][40, 0] = np.inf
    got, _ = run(emu, c, 7)
    assert _same(got, ref(c, 7))
    assert got["stat"][2]["n"] == 299 and got["stat"][0]["n"] == 299 and got["stat"][1]["n"] == 300
    assert got["stat"][9 + 2]["n"] == 299  # (err = est - NaN)
    finite = dict(c, u=np.where(np.isnan(c["u"]), 1e9, c["u"]))
    again, _ = run(emu, finite, 7)
    assert _same(again, got)  # (1e9 in a held row would be the maximum and a violation, were it read)
    assert _same(ref(finite, 7), got)
    held = int((c["age"] == HELD).sum())
    assert held > 0 and all(got["stat"][6 + k]["n"] == 300 - held for k in range(3))
    c = _case(6, 3, 70, seed=6, ages=(HELD,))
    got, _ = run(emu, c, 7)
    assert _same(got, ref(c, 7))
    for s in got["stat"][6:9]:
        assert (s["n"], s["mean"], s["m2"], s["min"], s["max"], s["argmin"], s["argmax"]) == (0, 0.0, 0.0, np.inf, -np.inf, -1, -1)
    assert got["head"]["held"] == 70 and got["head"]["solved"] == 0


def test_ties_go_to_the_lowest_index(emu):
    c = _case(3, 1, 1500, seed=8, ages=(0,))
    top, low = c["x"][:, 1].max() + 1.0, c["x"][:, 1].min() - 1.0
    c["x"][[1400, 70, 1030], 1] = top  # (in two chunks, and in two waves of the first)
    c["x"][[1499, 300], 1] = low
    got, _ = run(emu, c, 1, limits=())
    assert (got["stat"][1]["argmax"], got["stat"][1]["argmin"]) == (70, 300)
    assert _same(got, ref(c, 1, limits=()))


def test_every_walk_order_and_both_ways_to_the_data_give_the_same_bytes(emu):
    """ascending, descending and three permutations of the threads and the chunks; the image and direct loads; pairs and single doubles; one
    array off its 16-byte boundary (no pairs then)"""
    for (nx, nu), count in itertools.product(SHAPES, (65, 1025)):
        c = _case(nx, nu, count, seed=count + nu)
        first, T = run(emu, c, 7)
        assert T.vec2_used == 1
        for lds, (order, seed) in itertools.product((1, 0), ((0, 0), (1, 0), (2, 11), (2, 12), (2, 13))):
            got, T = run(emu, c, 7, order=order, seed=seed, lds_mode=lds)
            assert T.lds_used == lds and _same(got, first), (nx, nu, count, lds, order, seed)
        got, T = run(emu, c, 7, vec2_mode=0)
        assert T.vec2_used == 0 and _same(got, first)
        for k in ("x", "u", "est"):
            got, T = run(emu, c, 7, misalign=(k,))
            assert T.vec2_used == 0 and _same(got, first), k
        got, T = run(emu, c, 7, misalign=LIMITS)  # (the limits are read where they lie: their alignment decides nothing)
        assert T.vec2_used == 1 and _same(got, first)
    # an image that does not fit the LDS: the launch's own rule chooses direct loads
    assert emu.emu_trace_in_lds(6, 3, 7, 1, 1) == 1 and emu.emu_trace_in_lds(9, 1, 7, 0, 0) == 1 and emu.emu_trace_in_lds(10, 1, 7, 0, 0) == 0
    assert emu.emu_trace_in_lds(19, 1, 1, 0, 0) == 1 and emu.emu_trace_in_lds(20, 1, 1, 0, 0) == 0
    c = _case(10, 1, 1025, seed=2)
    got, T = run(emu, c, 7)
    assert T.lds_used == 0 and T.lds_doubles == 0 and _same(got, ref(c, 7))


def _drive(emu, c, what, ticks, capacity, every, fill=0xA5):
    rows = trace_ref.rows_of(what, c["nx"], c["nu"], True)
    size = trace_ref.slot_dtype(rows).itemsize
    buf = np.full(capacity * size + 64, fill, dtype=np.uint8)  # (64 bytes behind the trace that nothing may touch)
    clock = Clock(0, 0, 0, capacity, every)
    written = []
    for t in range(ticks):
        T, keep = _tick(c, what, tau=t + 1)
        before = buf.copy()
        slot = emu.emu_trace_record(ctypes.byref(T), ctypes.byref(clock), buf.ctypes.data)
        assert slot >= -1
        changed = np.nonzero(before != buf)[0]
        if slot < 0:
            assert changed.size == 0, t
        else:  # bytes of the buffer outside the written slot are untouched
            assert changed.size and slot * size <= changed.min() and changed.max() < (slot + 1) * size, (t, slot)
            written.append((t, slot))
    return buf, clock, written, size


def test_a_full_trace_records_nothing_further_and_every_picks_the_ticks(emu):
    c = _case(3, 1, 70, seed=9)
    buf, clock, written, size = _drive(emu, c, 3, ticks=6, capacity=4, every=0)
    assert written == [(0, 0), (1, 1), (2, 2), (3, 3)] and (clock.tick, clock.recorded, clock.missed) == (6, 4, 2)
    assert (buf[4 * size:] == 0xA5).all()
    slots = buf[:4 * size].view(trace_ref.slot_dtype(trace_ref.rows_of(3, 3, 1, True)))
    assert slots["head"]["tick"].tolist() == [0, 1, 2, 3] and slots["head"]["tau"].tolist() == [1, 2, 3, 4]
    assert _same(slots[2], ref(c, 3, tick=2, tau=3))
    buf, clock, written, size = _drive(emu, c, 3, ticks=8, capacity=5, every=3)
    assert written == [(0, 0), (3, 1), (6, 2)] and (clock.tick, clock.recorded, clock.missed) == (8, 3, 0)
    assert (buf[3 * size:] == 0xA5).all()
    assert trace_ref.recorded_ticks(8, 3, 5) == ([0, 3, 6], 0) and trace_ref.recorded_ticks(6, 0, 4) == ([0, 1, 2, 3], 2)
    buf, clock, written, size = _drive(emu, c, 3, ticks=7, capacity=2, every=2)
    assert written == [(0, 0), (2, 1)] and (clock.tick, clock.recorded, clock.missed) == (7, 2, 2)  # (ticks 4 and 6 were recordable; 1, 3, 5 never)


# ---- shards ----
def _as_trace(slots, nx, nu, what, limits):
    out, at = dict(head=slots["head"].copy()), 0
    for name, n, bit in (("x", nx, 1), ("u", nu, 2), ("err", nx, 4)):
        if what & bit:
            out[name] = slots["stat"][:, at:at + n].copy()
            at += n
    if limits:
        out["viol"] = slots["stat"][:, at].copy()
    return out


def test_merge_traces_of_two_halves(emu):
    """two ticks of a batch of 2049 cut at a chunk boundary, merged on the host: n, min, max, args and every head count of the whole, mean and m2
    within the summary's bound, one merge deeper"""
    from copra_amd import sharding
    nx, nu, count, cut = 3, 1, 2 * score_ref.CHUNK + 1, score_ref.CHUNK
    ticks = [_case(nx, nu, count, seed=20 + t) for t in range(2)]
    half = lambda c, lo, hi: dict(c, batch=hi - lo, **{k: c[k][lo:hi] for k in ("x", "u", "est", "age")})  # noqa: E731
    stack = lambda cs: _as_trace(np.stack([run(emu, c, 7, tick=t, tau=t + 1)[0] for t, c in enumerate(cs)]), nx, nu, 7, True)  # noqa: E731
    whole = stack(ticks)
    parts = [stack([half(c, 0, cut) for c in ticks]), stack([half(c, cut, count) for c in ticks])]
    merged = sharding.merge_traces(parts, [0, cut])
    assert merged["head"].tobytes() == whole["head"].tobytes()
    worst = 0.0
    for t, c in enumerate(ticks):
        with np.errstate(invalid="ignore"):
            vals = trace_ref.values(7, c["x"], c["u"], c["age"], c["est"], c["x_lo"], c["x_hi"], c["u_lo"], c["u_hi"])
        flat = np.concatenate([merged[g][t].reshape(-1) for g in ("x", "u", "err", "viol")])
        flat_whole = np.concatenate([whole[g][t].reshape(-1) for g in ("x", "u", "err", "viol")])
        for r in range(vals.shape[0]):
            for k in ("n", "min", "max", "argmin", "argmax"):
                assert flat[r][k] == flat_whole[r][k], (t, r, k)
            worst = max(worst, trace_ref.check_stat(flat[r], vals[r], lambda v: summary_bounds(v, merge_depth(count, 1)), (t, r)))
    print("two halves merged: largest error / bound %.3g" % worst)
    args = np.concatenate([merged[g][k].reshape(-1) for g in ("x", "u", "err") for k in ("argmin", "argmax")])
    assert (args >= cut).any() and (0 <= args).all() and (args < cut).any()  # (args of both shards survive, the second's shifted)
    with pytest.raises(ValueError):
        sharding.merge_traces(parts, [0])
    other = dict(parts[1], head=parts[1]["head"].copy())
    other["head"]["tau"][1] += 1
    with pytest.raises(ValueError):
        sharding.merge_traces([parts[0], other], [0, cut])


# ---- memory errors on the host ----
def test_kernel_bodies_under_the_address_and_ub_sanitizers(tmp_path):
    """tests/emu/emu_trace_main.cpp -- (6, 3) and (3, 1), instance counts 1 .. 1025, every `what`, with and without limits and an estimate, the
    image and direct loads, three walk orders, and a trace of 3 slots driven over 10 ticks -- as a stand-alone program built with
    -fsanitize=address,undefined; every array has exactly the elements the kernel may touch.  Exit status 0 and an empty stderr."""
    exe = str(tmp_path / "emu_trace_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(EMU, "emu_trace.cpp"), os.path.join(EMU, "emu_trace_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
