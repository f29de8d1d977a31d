"""Reference schedules at the C ABI (copra_batch_set_reference_schedule / _schedule_seek / _schedule_tick, ABI 8) without a GPU: declared,
exported, bound -- and the arithmetic of the window kernel (copra_amd/csrc/ref_window.hpp), whose body compiles on the host:
tests/emu/emu_ref_window.cpp walks it thread by thread, this file compiles that harness itself.

The kernel copies: its output is compared BIT FOR BIT with numpy's statement of the header's formula
    p[b][s r + i] = sched[b or 0][min(first + s, steps - 1)][i],  s = 0 .. S-1,  first = tau + offset
and the doubles around the output (guards in front of it, behind it, and the rest of its allocation) must come back untouched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("copra_batch_set_reference_schedule", "copra_batch_schedule_seek", "copra_batch_schedule_tick")
N = 7  # the horizon of the cases below: S in {1, N, N + 1}, offset in {0, N}
GUARD = 16  # doubles in front of and behind every output


def _lib():
    from copra_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_capi.LIB_PATH)


def test_header_declares_reference_schedules():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert code.index("copra_batch_set_reference_schedule") > code.index("copra_batch_get_x0")  # behind the tick block
    assert re.search(r"long long\s+copra_batch_schedule_tick\s*\(\s*const copra_batch_t\s*\*", code)
    assert "costFunctions.h:103-219" in text and "LMPC.cpp:233-247" in text


def test_library_exports_reference_schedules_with_abi_8():
    lib = _lib()
    for name in NEW:
        assert hasattr(lib, name), name
    lib.copra_abi_version.restype = ctypes.c_int
    assert lib.copra_abi_version() >= 8


def test_null_handle_is_an_argument_error():
    from copra_amd import _capi
    lib = _lib()
    lib.copra_batch_set_reference_schedule.restype = ctypes.c_int
    lib.copra_batch_set_reference_schedule.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong] + [ctypes.c_int] * 4
    lib.copra_batch_schedule_seek.restype = ctypes.c_int
    lib.copra_batch_schedule_seek.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.copra_batch_schedule_tick.restype = ctypes.c_longlong
    lib.copra_batch_schedule_tick.argtypes = [ctypes.c_void_p]
    assert lib.copra_batch_set_reference_schedule(None, 0, None, 1, 1, 0, 0, 0) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_schedule_seek(None, 0) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_schedule_tick(None) == -1


def test_python_binding_has_reference_schedules():
    from copra_amd import BatchLMPC
    for name in ("set_reference_schedule", "schedule_seek", "schedule_tick"):
        assert callable(getattr(BatchLMPC, name, None)), name


# ---- the kernel's arithmetic ----
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_ref_window") / "libemu_ref_window.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "emu", "emu_ref_window.cpp"),
                           "-o", so])
    lib = ctypes.CDLL(so)
    lib.emu_ref_window.restype = ctypes.c_int
    lib.emu_ref_window.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 8
    lib.emu_ref_window_group.restype = ctypes.c_int
    return lib


def window(sched, first, S, batch):
    """the header's formula in numpy: sched (steps, r) or (batch, steps, r) -> (batch, S r)"""
    steps = sched.shape[-2]
    idx = np.minimum(first + np.arange(S), steps - 1)
    w = sched[..., idx, :].reshape(sched.shape[:-2] + (-1,))
    return np.ascontiguousarray(np.broadcast_to(w, (batch, w.shape[-1])))


def _aligned(count, shift):
    """`count` doubles whose first one lies `shift` doubles behind a 16-byte boundary (0: aligned, 1: 8 bytes off), NaN-filled"""
    raw = np.full(count + 3, np.nan)
    off = (-(raw.ctypes.data // 8) % 2 + shift) % 2
    v = raw[off:off + count]
    assert (v.ctypes.data % 16 == 0) == (shift == 0)
    return v


def _launch(emu, batch, costs, group=None, threads=256):
    """costs: list of dict(sched, first, S, per_instance, shift_in, shift_out); returns the outputs and which of them went 16 bytes per lane"""
    k = len(costs)
    keep, scheds, outs, fulls = [], [], [], []
    for c in costs:
        s = _aligned(c["sched"].size, c.get("shift_in", 0))
        s[:] = c["sched"].reshape(-1)
        W = c["S"] * c["sched"].shape[-1]
        full = _aligned(batch * W + 2 * GUARD, c.get("shift_out", 0))
        full[:] = -7.25  # guards and output alike
        scheds.append(s)
        fulls.append(full)
        outs.append(full[GUARD:GUARD + batch * W])
        keep.append(s.copy())
    pp = ctypes.c_void_p * k
    ll = ctypes.c_longlong * k
    ii = ctypes.c_int * k
    vec2 = ii(*([-1] * k))
    rc = emu.emu_ref_window(batch, k, group or emu.emu_ref_window_group(), threads, pp(*[s.ctypes.data for s in scheds]), pp(*[o.ctypes.data for o in outs]),
                            ll(*[c["sched"].shape[-2] for c in costs]), ll(*[c["first"] for c in costs]), ii(*[c["sched"].shape[-1] for c in costs]),
                            ii(*[c["S"] for c in costs]), ii(*[int(c["per_instance"]) for c in costs]), vec2)
    assert rc == 0
    res = []
    for c, s, s0, full, o in zip(costs, scheds, keep, fulls, outs):
        assert np.array_equal(s, s0)  # the schedule is only read
        assert (full[:GUARD] == -7.25).all() and (full[GUARD + o.size:] == -7.25).all()  # nothing outside [batch][S r] is written
        res.append(o.reshape(batch, -1).copy())
    return res, list(vec2)


def _sched(rng, batch, steps, r, per_instance):
    return rng.standard_normal(((batch,) if per_instance else ()) + (steps, r))


@pytest.mark.parametrize("per_instance", [False, True])
@pytest.mark.parametrize("r", [1, 3, 6])
@pytest.mark.parametrize("S", [1, N, N + 1])
@pytest.mark.parametrize("offset", [0, N])
def test_window_is_the_formula_bit_for_bit(emu, per_instance, r, S, offset):
    batch, steps = 77, 24  # (77: not a multiple of a workgroup's share -- the last workgroup is partial)
    rng = np.random.default_rng(100 * r + 10 * S + offset + per_instance)
    sched = _sched(rng, batch, steps, r, per_instance)
    seen = set()
    for tau in list(range(0, steps + 3)) + [10 * steps]:  # ... to well past the end: the clamp holds the last block
        for shift_in, shift_out in ((0, 0), (1, 0), (0, 1)):  # aligned, and each side 8 bytes off: the 8-byte path
            (got,), (v,) = _launch(emu, batch, [dict(sched=sched, first=tau + offset, S=S, per_instance=per_instance, shift_in=shift_in, shift_out=shift_out)])
            seen.add(v)
            want = window(sched, tau + offset, S, batch)
            assert got.tobytes() == want.tobytes(), (tau, shift_in, shift_out)
            if shift_out:
                assert v == 0
            if tau + offset >= steps - 1:
                assert np.array_equal(got, np.tile(sched[..., -1, :], S) if per_instance else np.tile(sched[-1], (batch, S)))  # the last block, repeated
    if (r * S) % 2 == 0:
        assert seen == {0, 1}  # both forms of the copy were walked
    else:
        assert seen == {0}  # an odd window: its instances do not all start on 16 bytes


@pytest.mark.parametrize("per_instance", [False, True])
def test_one_step_schedule(emu, per_instance):
    """steps = 1: every block of every window is that one block"""
    rng = np.random.default_rng(3)
    for r, S in ((6, N + 1), (3, 1), (5, N)):
        sched = _sched(rng, 40, 1, r, per_instance)
        for first in (0, 1, N, 1000):
            (got,), _ = _launch(emu, 40, [dict(sched=sched, first=first, S=S, per_instance=per_instance)])
            assert got.tobytes() == window(sched, first, S, 40).tobytes()
            assert got.tobytes() == np.ascontiguousarray(np.broadcast_to(np.tile(sched[..., 0, :], S), (40, r * S))).tobytes()


@pytest.mark.parametrize("batch", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("threads", [64, 256])
def test_two_costs_in_one_launch(emu, batch, threads):
    """a shared reference trajectory and a per-instance goal of the horizon's end (TargetCost: S = 1, offset = N) in ONE launch, with a third cost
    whose window is wider than the workgroup; batches around the workgroup's share"""
    rng = np.random.default_rng(batch)
    traj = _sched(rng, batch, 31, 6, False)
    goal = _sched(rng, batch, 31, 3, True)
    wide = _sched(rng, batch, 50, 9, True)  # S r = 9 x 40 = 360 doubles: more than one pass of the lanes
    for tau in (0, 5, 24, 29, 30, 31, 45):
        costs = [dict(sched=traj, first=tau, S=N + 1, per_instance=False), dict(sched=goal, first=tau + N, S=1, per_instance=True),
                 dict(sched=wide, first=tau, S=40, per_instance=True)]
        got, _ = _launch(emu, batch, costs, threads=threads)
        for g, c in zip(got, costs):
            assert g.tobytes() == window(c["sched"], c["first"], c["S"], batch).tobytes(), tau


def test_group_sizes_and_the_largest_launch(emu):
    """eight costs -- the most one launch serves -- and workgroups of 1, 5 and 64 instances"""
    rng = np.random.default_rng(8)
    batch = 37
    costs = [dict(sched=_sched(rng, batch, 12 + k, 2 + k % 3, k % 2 == 1), first=3 * k, S=(1, N, N + 1)[k % 3], per_instance=k % 2 == 1) for k in range(8)]
    for group in (1, 5, 64):
        got, _ = _launch(emu, batch, costs, group=group)
        for g, c in zip(got, costs):
            assert g.tobytes() == window(c["sched"], c["first"], c["S"], batch).tobytes(), group
