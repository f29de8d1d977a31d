"""Trace quantiles (copra_batch_set_trace_quantiles, ABI 18) without a GPU: declared, exported, bound -- and the selection on the kernel's own
bodies (copra_amd/csrc/trace_quant_step.hpp), which compile on the host: tests/emu/emu_trace_quant.cpp walks one workgroup per row, every
pass thread by thread in the walk orders of tests/emu/emu_walk.h over an LDS block and a key buffer that start out as garbage, and the scan
lane by lane; this file compiles that harness itself.  The expectation is tests/trace_quant_ref.py -- a stable sort by the key and the rank
rule -- on the values tests/trace_ref.py forms, byte for byte: an order statistic is an element of the data, there is no bound to argue."""
import ctypes
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import trace_quant_ref
import trace_ref
from test_trace_abi import LIMITS, _case, _lib
from test_trace_abi import emu  # noqa: F401  (the trace's own emulator, a fixture: the slot of the same tick)
from test_trace_abi import run as run_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
NEW = ("copra_batch_set_trace_quantiles", "copra_batch_trace_quantile_info", "copra_batch_trace_quantiles_device", "copra_batch_get_trace_quantiles")
SHAPES = [(6, 3), (1, 1), (5, 2)]
BATCHES = [1, 2, 63, 64, 65, 255, 257, 1023, 1025, 2049]
LEVELS = [0.0, 1.0, 0.5, 1.0 / 3.0, 1e-9, 0.999, 0.5, 0.05]  # (0.5 twice: levels may repeat, and need not be sorted)
VP, CI, LL, U64, DP = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_double)
HELD = trace_ref.HELD


# ---- surface ----
def test_header_declares_the_quantiles():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+COPRA_TRACE_QUANT_MAX\s+8\b", code)
    assert re.search(r"copra_batch_set_trace_quantiles\s*\(\s*copra_batch_t\s*\*\s*\w*\s*,\s*const\s+double\s*\*\s*\w*\s*,\s*int\s+\w*\s*\)", code)
    assert re.search(r"copra_batch_get_trace_quantiles\s*\(\s*copra_batch_t\s*\*\s*\w*\s*,\s*long\s+long\s+\w*\s*,\s*long\s+long\s+\w*\s*,\s*double\s*\*\s*\w*\s*\)", code)
    section = text[text.index("trace quantiles: exact"):text.index("#define COPRA_TRACE_QUANT_MAX")]
    for rule in ("key = b ^ (b >> 63 ? ~0ull : 1ull << 63)", "c = ceil(p * (double)n)", "k = min(n - 1, max(0, c - 1))", "0x7FF8000000000000", "-0.0 before +0.0"):
        assert rule in section, rule  # (the rule is written down)
    trace = text[text.index("ensemble traces"):text.index("#define COPRA_TRACE_X")]
    assert "quantiles" not in trace[trace.index("Not covered yet"):]  # (no longer a follow-up)


def test_library_exports_the_quantiles_with_abi_18():
    lib = _lib()
    for name in NEW:
        assert hasattr(lib, name), name
    lib.copra_abi_version.restype = CI
    assert lib.copra_abi_version() >= 18
    from copra_amd import _capi
    lib.copra_batch_set_trace_quantiles.restype = CI
    lib.copra_batch_set_trace_quantiles.argtypes = [VP, VP, CI]
    lib.copra_batch_trace_quantile_info.restype = CI
    lib.copra_batch_trace_quantile_info.argtypes = [VP, VP, VP]
    lib.copra_batch_trace_quantiles_device.restype = VP
    lib.copra_batch_trace_quantiles_device.argtypes = [VP]
    lib.copra_batch_get_trace_quantiles.restype = CI
    lib.copra_batch_get_trace_quantiles.argtypes = [VP, LL, LL, VP]
    room = np.zeros(64)
    # (a NULL handle is refused before anything touches a device; the rest of the error table runs in tests/test_trace_quant_gpu.py)
    assert lib.copra_batch_set_trace_quantiles(None, room.ctypes.data, 3) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_set_trace_quantiles(None, None, 0) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_trace_quantile_info(None, room.ctypes.data, None) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_get_trace_quantiles(None, 0, 0, room.ctypes.data) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_trace_quantiles_device(None) is None


def test_python_binding_has_the_quantiles():
    from copra_amd import BatchLMPC, _capi
    for name in ("set_trace_quantiles", "trace_quantiles"):
        assert callable(getattr(BatchLMPC, name, None)), name
    assert isinstance(inspect.getattr_static(BatchLMPC, "trace_quantiles_ptr"), property)
    assert list(inspect.signature(BatchLMPC.set_trace_quantiles).parameters)[1:] == ["levels"]
    assert _capi.TRACE_QUANT_MAX == 8 == trace_quant_ref.QUANT_MAX


def test_the_rule_is_numpys_inverted_cdf():
    assert trace_quant_ref.self_check()
    v = np.array([3.0, -0.0, 0.0, np.nan, -1.0, np.inf])
    got = trace_quant_ref.row(v, [0.0, 0.5, 0.75, 1.0])  # finite, ascending by key: -1, -0.0, +0.0, 3
    assert got.tolist() == [np.float64(x).view(np.uint64) for x in (-1.0, -0.0, 0.0, 3.0)]
    assert trace_quant_ref.row(np.array([np.nan, np.inf]), [0.5]).tolist() == [0x7FF8000000000000]
    assert [trace_quant_ref.rank(p, 4) for p in (0.0, 0.25, 0.26, 0.5, 1.0)] == [0, 0, 1, 1, 3]  # (n even, p = 0.5: the lower median)


# ---- the kernel bodies on the host ----
class QTick(ctypes.Structure):
    """EmuQuantTick of tests/emu/emu_trace_quant.h"""
    _fields_ = ([(n, CI) for n in ("batch", "nx", "nu", "what", "order", "nq")] + [("seed", U64)]
                + [(n, VP) for n in ("x", "u", "est", "age", "x_lo", "x_hi", "u_lo", "u_hi")] + [("level", ctypes.c_double * 8), ("out", VP), ("rows", CI)])


class QClock(ctypes.Structure):
    """EmuQuantClock of tests/emu/emu_trace_quant.h"""
    _fields_ = [("tick", LL), ("recorded", LL), ("missed", LL), ("capacity", LL), ("every", CI)]


@pytest.fixture(scope="module")
def qemu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_trace_quant") / "libemu_trace_quant.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(EMU, "emu_trace_quant.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_trace_quant_tick.restype = CI
    lib.emu_trace_quant_tick.argtypes = [ctypes.POINTER(QTick)]
    lib.emu_trace_quant_record.restype = LL
    lib.emu_trace_quant_record.argtypes = [ctypes.POINTER(QTick), ctypes.POINTER(QClock), VP]
    lib.emu_trace_quant_key.restype = U64
    lib.emu_trace_quant_key.argtypes = [ctypes.c_double]
    lib.emu_trace_quant_rank.restype = LL
    lib.emu_trace_quant_rank.argtypes = [ctypes.c_double, LL]
    lib.emu_trace_quant_sizes.argtypes = [VP, VP, VP]
    return lib


def _qtick(c, what, levels, limits=LIMITS, live=True, order=0, seed=1):
    keep = {k: np.ascontiguousarray(c[k]) for k in ("x", "u", "est", "age") + tuple(limits)}
    T = QTick()
    T.batch, T.nx, T.nu, T.what, T.order, T.nq, T.seed = c["batch"], c["nx"], c["nu"], what, order, len(levels), seed
    T.x, T.u, T.age = keep["x"].ctypes.data, keep["u"].ctypes.data, keep["age"].ctypes.data
    T.est = keep["est"].ctypes.data if live else None
    for k in limits:
        setattr(T, k, keep[k].ctypes.data)
    for q, p in enumerate(levels):
        T.level[q] = p
    return T, keep


def qrun(qemu, c, what, levels, **kw):
    """one recorded tick of case c on the emulator: the quantiles, (rows, nq) float64, with one word behind them that nothing may touch"""
    T, keep = _qtick(c, what, levels, **kw)
    rows = trace_ref.rows_of(what, c["nx"], c["nu"], bool(kw.get("limits", LIMITS)))
    out = np.full(rows * len(levels) + 1, -7.25)
    T.out = out.ctypes.data
    assert qemu.emu_trace_quant_tick(ctypes.byref(T)) == 0  # (-2: the guard behind the key buffer was touched)
    assert T.rows == rows and out[-1] == -7.25
    return out[:-1].reshape(rows, len(levels)).copy()


def qref(c, what, levels, limits=LIMITS, live=True):
    lim = {k: c[k] for k in limits}
    with np.errstate(invalid="ignore", over="ignore"):
        vals = trace_ref.values(what, c["x"], c["u"], c["age"], c["est"] if live else None, **lim)
    return trace_quant_ref.rows(vals, levels)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_key_rank_and_sizes_are_the_rules(qemu):
    vals = np.array([0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 1e308, -1e308, np.inf, -np.inf, np.nan, 1.7976931348623157e308, -1.7976931348623157e308])
    assert [qemu.emu_trace_quant_key(float(v)) for v in vals] == trace_quant_ref.keys(vals).tolist()
    for n, p in itertools.product(list(range(1, 70)) + [255, 256, 257, 1000, 65536, 262145], LEVELS + [0.95, 0.25, 2.0 / 3.0]):
        assert qemu.emu_trace_quant_rank(p, n) == trace_quant_ref.rank(p, n), (n, p)
    m, t, lds = CI(), CI(), CI()
    qemu.emu_trace_quant_sizes(ctypes.byref(m), ctypes.byref(t), ctypes.byref(lds))
    assert m.value == 8 and t.value % 64 == 0 and t.value // 64 >= 8 and 8 * 256 * 4 <= lds.value <= 8 * 256 * 4 + 256


@pytest.mark.parametrize("nx,nu", SHAPES)
def test_every_what_with_and_without_limits_equals_the_sort(qemu, nx, nu):
    """every non-empty `what`, with and without limits, with and without an estimate, eight levels and one: every byte; batches 65 (two
    waves, one of them one lane) and 1025 (every thread an instance, one thread two) with an odd share of held instances"""
    for batch in (65, 1025):
        c = _case(nx, nu, batch, seed=100 * nx + nu + batch)
        for n, (what, limits, live) in enumerate(itertools.product(range(1, 8), (LIMITS, ()), (True, False))):
            for levels in (LEVELS, [LEVELS[n % 8]]):
                got, want = qrun(qemu, c, what, levels, limits=limits, live=live), qref(c, what, levels, limits=limits, live=live)
                assert _same(got, want), (batch, what, limits, live, levels, got, want)
            if what & 4 and not live:  # no estimate on this tick: no instance has a value
                at = (nx if what & 1 else 0) + (nu if what & 2 else 0)
                assert (got[at:at + nx].view(np.uint64) == 0x7FF8000000000000).all()


@pytest.mark.parametrize("nx,nu", SHAPES)
def test_batches_around_a_wave_a_workgroup_and_a_second_round(qemu, nx, nu):
    """all three groups and the viol row at every batch at which a thread's loop or the last wave changes (one workgroup of 1024 threads
    takes four instances per thread and round)"""
    for n, batch in enumerate(BATCHES):
        c = _case(nx, nu, batch, seed=7 * batch + nx)
        assert _same(qrun(qemu, c, 7, LEVELS), qref(c, 7, LEVELS)), batch
        assert _same(qrun(qemu, c, 1 + n % 7, [LEVELS[n % 8]], limits=()), qref(c, 1 + n % 7, [LEVELS[n % 8]], limits=())), batch


def _column(v):
    """a (1, 1) case whose one state row is v"""
    v = np.asarray(v, dtype=np.float64)
    b = v.size
    return dict(nx=1, nu=1, batch=b, x=v.reshape(b, 1).copy(), u=np.zeros((b, 1)), est=np.zeros((b, 1)), age=np.zeros(b, dtype=np.int32))


def _edge_rows():
    rng = np.random.default_rng(42)
    base = np.float64(1.2345678).view(np.uint64)
    low = (np.uint64(base) & ~np.uint64(0xFF)) | rng.integers(0, 256, 700).astype(np.uint64)
    spread = np.concatenate([rng.uniform(1.0, 2.0, 100), -rng.uniform(1.0, 2.0, 100)])  # two top-digit bins of 100: ranks 99 and 100 are a bin's last and first
    out = {
        "all equal": np.full(300, 0.7),
        "two values": np.where(rng.random(301) < 0.3, -2.5, 4.0),
        "lowest byte": low.view(np.float64),
        "signed zeros": np.where(rng.random(200) < 0.5, -0.0, 0.0),
        "zeros below a value": np.concatenate([np.full(3, 0.0), np.full(3, -0.0), [1.0]]),
        "huge": np.where(rng.random(129) < 0.5, -1e308, 1e308) * rng.uniform(0.9, 1.0, 129),
        "mixed signs": rng.standard_normal(1500) * 10.0 ** rng.integers(-200, 200, 1500),
        "bins of 100": spread,
        "one": np.array([-3.5]),
        "pair": np.array([2.0, -2.0]),
    }
    den = rng.integers(1, 1 << 40, 300).astype(np.uint64)
    den[150:] |= np.uint64(1) << np.uint64(63)
    out["denormals"] = den.view(np.float64)
    bad = rng.standard_normal(500)
    bad[rng.random(500) < 0.3] = np.nan
    bad[rng.random(500) < 0.1] = np.inf
    bad[rng.random(500) < 0.1] = -np.inf
    bad[7] = -np.nan
    out["non-finite counted out"] = bad
    out["nothing finite"] = np.array([np.nan, np.inf, -np.inf] * 30)
    return out


def test_rows_built_to_break_a_radix_select(qemu):
    rows = _edge_rows()
    levels = LEVELS[:6] + [0.5 + 1e-12, 0.505]
    for name, v in rows.items():
        for order in (0, 1, 2):
            c = _column(v[::-1] if order == 1 else v)
            got, want = qrun(qemu, c, 1, levels, limits=(), order=order, seed=3), trace_quant_ref.rows([c["x"][:, 0]], levels)
            assert _same(got, want), (name, order, got.view(np.uint64), want.view(np.uint64))
    z = qrun(qemu, _column(rows["zeros below a value"]), 1, [0.0, 3 / 7, 4 / 7, 6 / 7, 1.0], limits=())[0]
    assert np.signbit(z).tolist() == [True, True, False, False, False] and z.tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]  # -0.0 three times, then +0.0
    b = qrun(qemu, _column(rows["bins of 100"]), 1, [0.5, 0.505], limits=())[0]
    assert b[0] == rows["bins of 100"][100:].max() and b[1] == rows["bins of 100"][:100].min()  # the last of one bin, the first of the next
    assert (qrun(qemu, _column(rows["nothing finite"]), 1, LEVELS, limits=()).view(np.uint64) == 0x7FF8000000000000).all()
    den = qrun(qemu, _column(rows["denormals"]), 1, [0.0, 1.0], limits=())[0]
    assert 0 < den[1] < 2.3e-308 and -2.3e-308 < den[0] < 0


def test_an_all_held_batch_and_a_tick_without_an_estimate(qemu):
    c = _case(6, 3, 70, seed=6, ages=(HELD,))
    got = qrun(qemu, c, 7, LEVELS)
    assert _same(got, qref(c, 7, LEVELS))
    assert (got[6:9].view(np.uint64) == 0x7FF8000000000000).all() and np.isfinite(got[:6]).all() and np.isfinite(got[9:]).all()
    c = _case(6, 3, 300, seed=5)
    c["x"][17, 2], c["x"][40, 0] = np.nan, np.inf
    got = qrun(qemu, c, 7, LEVELS, live=False)
    assert _same(got, qref(c, 7, LEVELS, live=False)) and (got[9:15].view(np.uint64) == 0x7FF8000000000000).all()
    finite = dict(c, u=np.where(np.isnan(c["u"]), 1e9, c["u"]))  # (1e9 in a held row would be the maximum, were it read)
    assert _same(qrun(qemu, finite, 7, LEVELS, live=False), got)


def test_every_walk_order_gives_the_same_bytes(qemu):
    for (nx, nu), batch in itertools.product(SHAPES, (65, 1025, 2049)):
        c = _case(nx, nu, batch, seed=batch + nu)
        first = qrun(qemu, c, 7, LEVELS)
        for order, seed in ((1, 0), (2, 11), (2, 12), (2, 13)):
            assert _same(qrun(qemu, c, 7, LEVELS, order=order, seed=seed), first), (nx, nu, batch, order, seed)


def test_levels_0_and_1_are_the_slots_min_and_max(emu, qemu):  # noqa: F811
    """two ties to the slot of the same tick, numerically (the slot's min of -0.0 and +0.0 is whichever came first)"""
    for (nx, nu), batch in itertools.product(SHAPES, (65, 1025)):
        c = _case(nx, nu, batch, seed=3 * batch + nx)
        c["x"][5 % batch, 0] = np.nan
        slot, _ = run_trace(emu, c, 7)
        got = qrun(qemu, c, 7, [0.0, 1.0])
        assert np.array_equal(got[:, 0], slot["stat"]["min"]) and np.array_equal(got[:, 1], slot["stat"]["max"])
        assert slot["stat"]["n"][0] == batch - 1 and (slot["stat"]["n"] > 0).all()


def test_a_full_trace_records_nothing_further_and_every_picks_the_ticks(qemu):
    c = _case(3, 1, 70, seed=9)
    rows, nq = trace_ref.rows_of(3, 3, 1, True), 3
    levels = [0.05, 0.5, 0.95]
    for ticks, capacity, every, want, missed in ((6, 4, 0, [0, 1, 2, 3], 2), (8, 5, 3, [0, 3, 6], 0), (7, 2, 2, [0, 2], 2)):
        buf = np.full(capacity * rows * nq + 8, -7.25)  # (8 doubles behind the buffer that nothing may touch)
        clock, written = QClock(0, 0, 0, capacity, every), []
        for t in range(ticks):
            T, keep = _qtick(c, 3, levels)
            before = buf.copy()
            slot = qemu.emu_trace_quant_record(ctypes.byref(T), ctypes.byref(clock), buf.ctypes.data)
            assert slot >= -1
            changed = np.nonzero(before.view(np.uint64) != buf.view(np.uint64))[0]
            if slot < 0:
                assert changed.size == 0, t
            else:
                assert changed.size and slot * rows * nq <= changed.min() and changed.max() < (slot + 1) * rows * nq, (t, slot)
                written.append(t)
        assert written == want and (clock.tick, clock.recorded, clock.missed) == (ticks, len(want), missed)
        assert trace_ref.recorded_ticks(ticks, every, capacity) == (want, missed)
        assert _same(buf[:rows * nq].reshape(rows, nq), qref(c, 3, levels))


# ---- memory errors on the host ----
def test_kernel_bodies_under_the_address_and_ub_sanitizers(tmp_path):
    """tests/emu/emu_trace_quant_main.cpp -- (6, 3) and (1, 1), batches 1 .. 2049, every `what`, with and without limits and an estimate, one
    level and eight, three walk orders, the edge rows of this file and a buffer of 3 slots driven over 10 ticks -- as a stand-alone program
    built with -fsanitize=address,undefined; every array has exactly the elements the kernel may touch, and the program checks every
    quantile against a sort of its own.  Exit status 0 and an empty stderr."""
    exe = str(tmp_path / "emu_trace_quant_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(EMU, "emu_trace_quant.cpp"), os.path.join(EMU, "emu_trace_quant_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
