"""Limit schedules at the C ABI (copra_batch_set_constraint_schedule / copra_batch_set_control_bound_schedule, ABI 9) without a GPU: declared,
exported, bound -- and the arithmetic of the window kernel (copra_amd/csrc/limit_window.hpp), whose body compiles on the host:
tests/emu/emu_limit_window.cpp walks it thread by thread, this file compiles that harness itself.

The kernel copies: its output is compared BIT FOR BIT with numpy's statement of the header's formula
    out[b][row0 + s r + i] = sched[b or 0][preview ? min(first + s, steps - 1) : min(first, steps - 1)][i],  s = 0 .. S-1,  first = tau + offset
and every double the formula does not name -- guards in front of and behind every buffer, the rows between a window's end and the next instance's
window, the rows of another constraint's window -- must come back untouched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("copra_batch_set_constraint_schedule", "copra_batch_set_control_bound_schedule")
N = 7  # the horizon of the cases below: S in {1, N, N + 1}, offset in {0, N}
GUARD = 16  # doubles in front of and behind every buffer
FILL = -7.25


def _lib():
    from copra_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_capi.LIB_PATH)


def test_header_declares_limit_schedules():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert code.index(name) > code.index("copra_batch_schedule_tick")  # behind the reference-schedule block
    assert "constraints.h:114-308" in text and "LMPC.cpp:233-247" in text


def test_library_exports_limit_schedules_with_abi_9():
    lib = _lib()
    for name in NEW:
        assert hasattr(lib, name), name
    lib.copra_abi_version.restype = ctypes.c_int
    assert lib.copra_abi_version() >= 9


def test_null_handle_is_an_argument_error():
    from copra_amd import _capi
    lib = _lib()
    lib.copra_batch_set_constraint_schedule.restype = ctypes.c_int
    lib.copra_batch_set_constraint_schedule.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_int] * 5
    lib.copra_batch_set_control_bound_schedule.restype = ctypes.c_int
    lib.copra_batch_set_control_bound_schedule.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_longlong] + [ctypes.c_int] * 4
    z = np.zeros(4)
    assert lib.copra_batch_set_constraint_schedule(None, 0, z.ctypes.data, 1, 1, 0, 1, 0, 0) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_set_control_bound_schedule(None, z.ctypes.data, z.ctypes.data, 1, 0, 1, 0, 0) == _capi.COPRA_ERR_ARG
    lib.copra_last_error.restype = ctypes.c_char_p
    assert lib.copra_last_error()


def test_python_binding_has_limit_schedules():
    from copra_amd import BatchLMPC
    for name in ("set_constraint_schedule", "set_control_bound_schedule"):
        assert callable(getattr(BatchLMPC, name, None)), name


# ---- the kernel's arithmetic ----
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_limit_window") / "libemu_limit_window.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "emu", "emu_limit_window.cpp"),
                           "-o", so])
    lib = ctypes.CDLL(so)
    lib.emu_limit_window.restype = ctypes.c_int
    lib.emu_limit_window.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 11
    lib.emu_limit_window_group.restype = ctypes.c_int
    lib.emu_limit_window_max.restype = ctypes.c_int
    return lib


def window(sched, first, S, preview, batch):
    """the header's formula in numpy: sched (steps, r) or (batch, steps, r) -> (batch, S r)"""
    steps = sched.shape[-2]
    idx = np.minimum(first + (np.arange(S) if preview else np.zeros(S, dtype=int)), steps - 1)
    w = sched[..., idx, :].reshape(sched.shape[:-2] + (-1,))
    return np.ascontiguousarray(np.broadcast_to(w, (batch, w.shape[-1])))


def _aligned(count, shift):
    """`count` doubles whose first one lies `shift` doubles behind a 16-byte boundary (0: aligned, 1: 8 bytes off)"""
    raw = np.full(count + 3, np.nan)
    off = (-(raw.ctypes.data // 8) % 2 + shift) % 2
    v = raw[off:off + count]
    assert (v.ctypes.data % 16 == 0) == (shift == 0)
    return v


def vec2_rule(out_ptr, sched_ptr, w, steps, first):
    """16-byte stores exactly where every address of the copy is a multiple of 16, stated without the kernel's helpers: the output's base, an even
    stride, an even first row and an even window; for a per-instance schedule also its base, an even schedule per instance, and an even start and
    an even length of the part of the window that is read contiguously (preview: from block min(first, steps - 1) to the end of the schedule or of
    the window; without preview there is none, but the start is still looked at)"""
    r, S = w["r"], w["S"]
    ok = out_ptr % 16 == 0 and w["stride"] % 2 == 0 and w["row0"] % 2 == 0 and (r * S) % 2 == 0
    if w["per_instance"]:
        f0 = min(first, steps - 1)
        live = min(steps - f0, S) * r if w["preview"] else 0
        ok = ok and sched_ptr % 16 == 0 and (steps * r) % 2 == 0 and (f0 * r) % 2 == 0 and live % 2 == 0
    return int(ok)


def _launch(emu, batch, buffers, wins, group=None, threads=256):
    """buffers: dict name -> (stride, shift_out); wins: list of dict(buf, row0, sched, first, S, per_instance, preview, shift_in).  Every buffer is
    written by the windows that name it and by nothing else: returned as name -> (batch, stride) after the guards were checked; and the vec2 flags"""
    bufs, fulls = {}, {}
    for name, (stride, shift) in buffers.items():
        full = _aligned(batch * stride + 2 * GUARD, shift)
        full[:] = FILL
        fulls[name], bufs[name] = full, full[GUARD:GUARD + batch * stride]
    k = len(wins)
    scheds, keep = [], []
    for w in wins:
        s = _aligned(w["sched"].size, w.get("shift_in", 0))
        s[:] = w["sched"].reshape(-1)
        scheds.append(s), keep.append(s.copy())
        w["r"], w["stride"] = w["sched"].shape[-1], buffers[w["buf"]][0]
    pp, ll, ii = ctypes.c_void_p * k, ctypes.c_longlong * k, ctypes.c_int * k
    vec2 = ii(*([-1] * k))
    rc = emu.emu_limit_window(batch, k, group or emu.emu_limit_window_group(), threads, pp(*[s.ctypes.data for s in scheds]),
                              pp(*[bufs[w["buf"]].ctypes.data for w in wins]), ll(*[w["sched"].shape[-2] for w in wins]), ll(*[w["first"] for w in wins]),
                              ii(*[w["stride"] for w in wins]), ii(*[w["row0"] for w in wins]), ii(*[w["r"] for w in wins]), ii(*[w["S"] for w in wins]),
                              ii(*[int(w["per_instance"]) for w in wins]), ii(*[int(w["preview"]) for w in wins]), vec2)
    assert rc == 0
    for w, s, s0, v in zip(wins, scheds, keep, vec2):
        assert np.array_equal(s, s0)  # the schedule is only read
        assert v == vec2_rule(bufs[w["buf"]].ctypes.data, s.ctypes.data, w, w["sched"].shape[-2], w["first"]), w
    out = {}
    for name, full in fulls.items():
        assert (full[:GUARD] == FILL).all() and (full[GUARD + bufs[name].size:] == FILL).all(), name  # the guards
        out[name] = bufs[name].reshape(batch, -1).copy()
    return out, list(vec2)


def _expect(batch, buffers, wins):
    out = {name: np.full((batch, stride), FILL) for name, (stride, _) in buffers.items()}
    for w in wins:
        W = w["S"] * w["sched"].shape[-1]
        out[w["buf"]][:, w["row0"]:w["row0"] + W] = window(w["sched"], w["first"], w["S"], w["preview"], batch)
    return out


def _check(emu, batch, buffers, wins, what=None, **kw):
    got, vec2 = _launch(emu, batch, buffers, wins, **kw)
    want = _expect(batch, buffers, wins)
    for name in buffers:
        assert got[name].tobytes() == want[name].tobytes(), (what, name)  # the windows bit for bit, every other double untouched
    return vec2


def _sched(rng, batch, steps, r, per_instance):
    return rng.standard_normal(((batch,) if per_instance else ()) + (steps, r))


@pytest.mark.parametrize("per_instance", [False, True])
@pytest.mark.parametrize("preview", [0, 1])
@pytest.mark.parametrize("r", [1, 2, 3])
@pytest.mark.parametrize("S", [1, N, N + 1])
def test_window_is_the_formula_bit_for_bit(emu, per_instance, preview, r, S):
    """one window inside a wider row: row0 in {0, odd, even}, strides larger than the window, odd and even; tau before the end of the schedule,
    straddling it and beyond it; offset 0 and N; aligned, and each side 8 bytes off (the 8-byte path)"""
    batch, steps = 63, 12
    rng = np.random.default_rng(1000 * r + 100 * S + 10 * preview + per_instance)
    sched = _sched(rng, batch, steps, r, per_instance)
    W = r * S
    seen = set()
    for row0, pad in ((0, 2), (3, 1), (4, 4), (2, 3)):  # (pad: the doubles behind the window that belong to somebody else)
        stride = row0 + W + pad
        for offset in (0, N):
            for tau in (0, 1, 2, steps - S - N if steps - S - N > 2 else 3, steps - 2, steps - 1, steps + 4):
                for shift_in, shift_out in ((0, 0), (1, 0), (0, 1)):
                    w = dict(buf="f", row0=row0, sched=sched, first=tau + offset, S=S, per_instance=per_instance, preview=preview, shift_in=shift_in)
                    (v,) = _check(emu, batch, dict(f=(stride, shift_out)), [w], (row0, stride, offset, tau, shift_in, shift_out))
                    seen.add(v)
                    if shift_out or stride % 2 or row0 % 2 or W % 2 or (per_instance and shift_in):
                        assert v == 0
    assert 0 in seen
    if W % 2 == 0:
        assert 1 in seen  # both forms of the copy were walked


@pytest.mark.parametrize("per_instance", [False, True])
@pytest.mark.parametrize("preview", [0, 1])
def test_one_step_schedule(emu, per_instance, preview):
    """steps = 1: every block of every window is that one block"""
    rng = np.random.default_rng(3)
    for r, S in ((2, N + 1), (3, 1), (1, N)):
        sched = _sched(rng, 40, 1, r, per_instance)
        for first in (0, 1, N, 1000):
            got, _ = _launch(emu, 40, dict(f=(r * S + 5, 0)), [dict(buf="f", row0=2, sched=sched, first=first, S=S, per_instance=per_instance, preview=preview)])
            want = np.ascontiguousarray(np.broadcast_to(np.tile(sched[..., 0, :], S), (40, r * S)))
            assert got["f"][:, 2:2 + r * S].tobytes() == want.tobytes()
            assert (got["f"][:, :2] == FILL).all() and (got["f"][:, 2 + r * S:] == FILL).all()


@pytest.mark.parametrize("batch", [1, 63, 64, 130])
@pytest.mark.parametrize("threads", [64, 256])
def test_bounds_and_a_constraint_in_one_launch(emu, batch, threads):
    """lower and upper write two different buffers (r = nu, S = N, row0 = 0, stride = nu N) while a constraint's window and ANOTHER constraint's
    window share the right-hand sides: two descriptors, then four; a window wider than the workgroup"""
    rng = np.random.default_rng(batch)
    nu = 3
    lo, up = _sched(rng, batch, 15, nu, False), _sched(rng, batch, 15, nu, True)
    vel = _sched(rng, batch, 15, 3, True)
    wide = _sched(rng, batch, 30, 3, False)  # S r = 120 x 3 = 360 doubles: more than one pass of the lanes
    mgen = 5 + 3 * (N + 1) + 4 + 360 + 1
    buffers = dict(lb=(nu * N, 0), ub=(nu * N, 0), f=(mgen, 0))
    for tau in (0, 5, 13, 14, 15, 40):
        for preview in (0, 1):
            bounds = [dict(buf="lb", row0=0, sched=lo, first=tau, S=N, per_instance=False, preview=preview),
                      dict(buf="ub", row0=0, sched=up, first=tau, S=N, per_instance=True, preview=preview)]
            _check(emu, batch, buffers, bounds, (tau, preview, 2), threads=threads)
            rows = [dict(buf="f", row0=5, sched=vel, first=tau + N, S=N + 1, per_instance=True, preview=preview),
                    dict(buf="f", row0=5 + 3 * (N + 1) + 4, sched=wide, first=tau, S=120, per_instance=False, preview=1 - preview)]
            _check(emu, batch, buffers, bounds + rows, (tau, preview, 4), threads=threads)


def test_group_sizes_and_the_largest_launch(emu):
    """eight windows -- the most one launch serves -- in three buffers, and workgroups of 1, 5 and 64 instances; a ninth is refused"""
    rng = np.random.default_rng(8)
    batch = 37
    assert emu.emu_limit_window_max() == 8
    buffers = dict(a=(100, 0), b=(61, 1), c=(64, 0))
    wins, row = [], dict(a=0, b=1, c=2)
    for k in range(8):
        r, S, buf = 1 + k % 3, (1, N, N + 1)[k % 3], "abc"[k % 3]
        wins.append(dict(buf=buf, row0=row[buf], sched=_sched(rng, batch, 9 + k, r, k % 2 == 1), first=3 * k, S=S, per_instance=k % 2 == 1, preview=k % 4 < 2))
        row[buf] += r * S + k % 2
    for group in (1, 5, 64):
        _check(emu, batch, buffers, wins, group, group=group)
    k = 9
    z = (ctypes.c_void_p * k)()
    assert emu.emu_limit_window(batch, k, 64, 256, z, z, z, z, z, z, z, z, z, z, None) == -1
