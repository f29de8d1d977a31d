"""Backup plans in the tick (copra_batch_set_backup_steps, ABI 10) without a GPU: declared, exported, bound -- and the rule itself on the two
phases of the plant-step kernel (copra_amd/csrc/plant_step.hpp), which compile on the host: tests/emu/emu_plant_backup.cpp walks them thread
by thread over a NaN-filled image, this file compiles that harness itself and drives it for several ticks on the same plan / next arrays.

The expectation is a numpy restatement of the rule in include/copra_hip.h.  u_out, plan, next and age_out are copies and integers: compared bit
for bit.  A new state is compared with reference_step within step_bound, both of tests/test_closed_loop_abi.py (the bound is derived there).

An age of -1 needs a fallback control and an age of -2 needs its absence, so one run cannot show both: every run must show every age from 0 to K
and its own one of the two, and the pair of runs that differ only in the fallback shows every age from -2 to K."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from test_closed_loop_abi import SHAPES, _case, _ptr, _run, reference_step, step_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
FALLBACK, HELD = -1, -2


def _lib():
    from copra_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_capi.LIB_PATH)


# ---- surface ----
def test_header_declares_backup_plans():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bcopra_batch_set_backup_steps\s*\(\s*copra_batch_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", code)
    assert re.search(r"#define\s+COPRA_PLAN_FALLBACK\s+\(-1\)", code) and re.search(r"#define\s+COPRA_PLAN_HELD\s+\(-2\)", code)
    end = code.index("} copra_plant_step_t;")
    body = code[code.rindex("typedef struct {", 0, end):end]
    fields = re.findall(r"(\w+)\s*;", body)
    at = fields.index("status_out")
    assert fields[at + 1:] == ["age_out", "age_hist", "solve_every"]  # appended, in this order: the struct is append-only
    assert re.search(r"int\s*\*\s*age_out\s*;", body) and re.search(r"int\s*\*\s*age_hist\s*;", body) and re.search(r"int\s+solve_every\s*;", body)


def test_library_exports_backup_plans_with_abi_10():
    lib = _lib()
    assert hasattr(lib, "copra_batch_set_backup_steps")
    lib.copra_abi_version.restype = ctypes.c_int
    assert lib.copra_abi_version() >= 10
    lib.copra_batch_set_backup_steps.restype = ctypes.c_int
    lib.copra_batch_set_backup_steps.argtypes = [ctypes.c_void_p, ctypes.c_int]
    from copra_amd import _capi
    assert lib.copra_batch_set_backup_steps(None, 1) == _capi.COPRA_ERR_ARG  # (a NULL handle is refused before anything touches a device)


def test_plant_step_init_zeroes_the_new_fields():
    from copra_amd import _capi
    lib = _lib()
    names = [n for n, _ in _capi.PlantStep._fields_]
    assert names[names.index("status_out") + 1:] == ["age_out", "age_hist", "solve_every"]
    st = _capi.PlantStep()
    ctypes.memset(ctypes.byref(st), 0xff, ctypes.sizeof(st))
    lib.copra_plant_step_init.restype = None
    lib.copra_plant_step_init.argtypes = [ctypes.POINTER(_capi.PlantStep)]
    lib.copra_plant_step_init(ctypes.byref(st))
    assert st.struct_size == ctypes.sizeof(_capi.PlantStep)
    assert not st.age_out and not st.age_hist and st.solve_every == 0
    assert (_capi.PLAN_FALLBACK, _capi.PLAN_HELD) == (FALLBACK, HELD)


def test_python_binding_has_backup_plans():
    import inspect
    from copra_amd import BatchLMPC
    assert callable(getattr(BatchLMPC, "set_backup_steps", None))
    assert inspect.signature(BatchLMPC.advance).parameters["age_out"].default is None
    ro = inspect.signature(BatchLMPC.rollout).parameters
    assert ro["age_hist"].default is None and ro["solve_every"].default == 1


# ---- the kernel bodies on the host ----
STEP_ARGS = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 13 + [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_plant_backup") / "libemu_plant_backup.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(EMU, "emu_plant_backup.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.emu_plant_backup_step.restype = ctypes.c_int
    lib.emu_plant_backup_step.argtypes = STEP_ARGS
    return lib


@pytest.fixture(scope="module")
def emu_abi9(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_plant_abi9") / "libemu_plant.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(EMU, "emu_plant.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.emu_plant_step.restype = ctypes.c_int
    lib.emu_plant_step.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 13
    return lib


# The five-tick script, batch 5.  Instance 0 solves at every tick; 1 never solves; 2 solves once, then fails until its plan is used up (K = 3:
# exactly at the last tick); 3 solves, fails two ticks, solves again; 4 starts with a failure (no plan yet), then alternates.  Tick 4 has no
# solve for anyone (fresh = 0): status and control are what tick 3 left, as on the device.
STATUS = np.array([[0, 1, 0, 0, 1], [0, 1, 1, 1, 0], [0, 1, 2, 1, 3], [0, 1, 3, 0, 0]], dtype=np.int32)
FRESH = (1, 1, 1, 1, 0)
BATCH = 5
GUARD = 4
PLAN_GUARD, NEXT_GUARD = -7.25, -77


def _script(nx, nu, N, shared, seed):
    rng = np.random.default_rng(seed)
    lead = () if shared else (BATCH,)
    c = dict(A=0.5 * rng.standard_normal(lead + (nx, nx)), B=rng.standard_normal(lead + (nx, nu)), d=rng.standard_normal(lead + (nx,)),
             x0=rng.standard_normal((BATCH, nx)), w=0.01 * rng.standard_normal((len(FRESH), BATCH, nx)), fb=rng.standard_normal((BATCH, nu)))
    status, control = [], []
    for t in range(len(FRESH)):
        if FRESH[t]:
            st = STATUS[t].copy()
            u = rng.standard_normal((BATCH, nu * N))  # exactly nu N doubles per instance
            u[st != 0] = np.nan  # what the engine leaves in a failed instance, first controls and tail
        status.append(st)
        control.append(u)
    c["status"], c["control"] = status, control
    return c


def _rule(c, t, K, nu, with_fb, plan, nxt):
    """the rule of include/copra_hip.h for one tick, restated: (u, age) and the new plan / next"""
    st, ctrl = c["status"][t], c["control"][t]
    u = np.full((BATCH, nu), np.nan)
    age = np.zeros(BATCH, dtype=np.int32)
    plan, nxt = plan.copy(), nxt.copy()
    for b in range(BATCH):
        if FRESH[t] and st[b] == 0:
            u[b] = ctrl[b, :nu]
            plan[b] = ctrl[b, nu:(K + 1) * nu].reshape(K, nu)
            nxt[b], age[b] = 1, 0
        elif 1 <= nxt[b] <= K:
            u[b] = plan[b, nxt[b] - 1]
            age[b] = nxt[b]
            nxt[b] += 1
        elif with_fb:
            u[b], age[b] = c["fb"][b], FALLBACK
        else:
            age[b] = HELD
    return u, age, plan, nxt


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _play(emu, c, nx, nu, N, K, group, threads, shared, with_w, with_fb, in_place):
    """the script on the emulator against the rule; returns the ages seen, (ticks, batch)"""
    A = np.ascontiguousarray(np.swapaxes(c["A"], -1, -2))  # the ABI's column-major blocks
    B = np.ascontiguousarray(np.swapaxes(c["B"], -1, -2))
    plan_buf = np.full(BATCH * K * nu + GUARD, PLAN_GUARD)
    plan_buf[:BATCH * K * nu] = np.nan  # (a plan is read only after it has been stored: a NaN that reaches a state shows)
    next_buf = np.full(BATCH + GUARD, NEXT_GUARD, dtype=np.int32)
    next_buf[:BATCH] = 0
    want_plan, want_next = plan_buf[:BATCH * K * nu].reshape(BATCH, K, nu).copy(), next_buf[:BATCH].copy()
    x = c["x0"].copy()
    ages = []
    what = (nx, nu, N, K, group, threads, shared, with_w, with_fb, in_place)
    for t in range(len(FRESH)):
        w = c["w"][t] if with_w else None
        u, age, want_plan, want_next = _rule(c, t, K, nu, with_fb, want_plan, want_next)
        moved = age != HELD
        ref, S = reference_step(c["A"], c["B"], c["d"], x, np.where(moved[:, None], u, 0.0), w)
        x_in = x.copy()
        nxt = x_in if in_place else np.full((BATCH, nx), np.nan)
        x_out, u_out = np.full((BATCH, nx), np.nan), np.full((BATCH, nu), 7.0)
        s_out, a_out = np.full(BATCH, -1, dtype=np.int32), np.full(BATCH, -99, dtype=np.int32)
        rc = emu.emu_plant_backup_step(BATCH, nx, nu, N, group, threads, int(shared), _ptr(A), _ptr(B), _ptr(c["d"]), _ptr(x_in), _ptr(w),
                                       _ptr(c["fb"] if with_fb else None), _ptr(c["status"][t]), _ptr(c["control"][t]), _ptr(nxt), _ptr(x_out), _ptr(u_out),
                                       _ptr(s_out), None, K, FRESH[t], _ptr(plan_buf), _ptr(next_buf), _ptr(a_out))
        assert rc == 0
        assert np.array_equal(a_out, age), (what, t, a_out, age)
        assert _same_bits(u_out, u), (what, t)  # (NaN exactly where the age is -2: the rule's u is NaN there and nowhere else)
        assert np.array_equal(np.isnan(u_out).any(axis=1), age == HELD) and np.array_equal(np.isnan(u_out).all(axis=1), age == HELD), (what, t)
        assert _same_bits(plan_buf[:BATCH * K * nu].reshape(BATCH, K, nu), want_plan), (what, t)
        assert np.array_equal(next_buf[:BATCH], want_next), (what, t, next_buf[:BATCH], want_next)
        assert (plan_buf[BATCH * K * nu:] == PLAN_GUARD).all() and (next_buf[BATCH:] == NEXT_GUARD).all(), (what, t)
        assert np.array_equal(s_out, c["status"][t]), (what, t)  # the status buffer's content, stale on the tick without a solve
        assert not np.isnan(nxt).any(), (what, t)  # no NaN of a failed instance's control or of an unwritten plan reaches a state
        err = np.abs(nxt[moved].astype(np.longdouble) - ref[moved])
        assert (err <= step_bound(nx, nu, S[moved])).all(), (what, t, float((err / step_bound(nx, nu, S[moved])).max()))
        assert _same_bits(nxt[~moved], x[~moved]), (what, t)  # held, bit for bit
        assert _same_bits(x_out, nxt), (what, t)
        if not in_place:
            assert _same_bits(x_in, x)  # (the old state is only read)
        x = nxt.copy()
        ages.append(age)
    return np.stack(ages)


# (nx, nu, N) with K in {1, N - 1}; at N = 2 the two are one case
@pytest.mark.parametrize("nx,nu,N,K", [(2, 2, 3, 1), (2, 2, 3, 2), (6, 3, 4, 1), (6, 3, 4, 3), (2, 1, 2, 1)])
def test_backup_plan_rule_on_the_kernel_bodies(emu, nx, nu, N, K):
    runs = 0
    for shared, with_w, in_place in itertools.product((0, 1), (False, True), (False, True)):
        c = _script(nx, nu, N, shared, seed=100 * nx + 10 * nu + N + 1000 * shared)
        for group, threads in itertools.product((1, 2, 4), (3, 64)):  # group 1: no vec2; 2 and 4: a partial last group; 3 threads < cnt nu
            seen = set()
            for with_fb in (False, True):
                ages = _play(emu, c, nx, nu, N, K, group, threads, shared, with_w, with_fb, in_place)
                own = set(range(0, K + 1)) | {FALLBACK if with_fb else HELD}
                assert set(ages.ravel().tolist()) == own, (K, with_fb, ages)  # a script in which nothing failed cannot pass
                seen |= set(ages.ravel().tolist())
                runs += 1
            assert seen == set(range(-2, K + 1))
    assert runs == 8 * 6 * 2


def test_the_script_is_the_one_described():
    """the ages of the script at K = 3 without a fallback, written out: the rule restated above is what the header says"""
    c = _script(6, 3, 4, 0, seed=1)
    plan, nxt = np.full((BATCH, 3, 3), np.nan), np.zeros(BATCH, dtype=np.int32)
    ages = []
    for t in range(5):
        _, age, plan, nxt = _rule(c, t, 3, 3, False, plan, nxt)
        ages.append(age.tolist())
    assert ages == [[0, -2, 0, 0, -2], [0, -2, 1, 1, 0], [0, -2, 2, 2, 1], [0, -2, 3, 0, 0], [1, -2, -2, 1, 1]]


# ---- off means off ----
@pytest.mark.parametrize("nx,nu", SHAPES)
def test_without_backup_steps_the_tick_is_the_abi9_tick(emu, emu_abi9, nx, nu):
    """backup_steps = 0: the new entry gives the bits of emu_plant_step for the cases of test_plant_step_arithmetic, whatever `fresh` says and
    with no plan / next arrays at all; age_out reports today's three cases"""
    batch = 77
    for shared, with_w, with_fb in itertools.product((False, True), (False, True), (False, True)):
        c = _case(nx, nu, batch, shared, seed=1000 * nx + nu + 7 * shared)
        A = np.ascontiguousarray(np.swapaxes(c["A"], -1, -2))
        B = np.ascontiguousarray(np.swapaxes(c["B"], -1, -2))
        for in_place, group, fresh in itertools.product((False, True), (1, 6, 32), (0, 1)):
            want = _run(emu_abi9, c, nx, nu, shared, with_w, with_fb, in_place, group)
            x0 = c["x0"].copy()
            nxt = x0 if in_place else np.full((batch, nx), np.nan)
            x_out, u_out = np.full((batch, nx), np.nan), np.full((batch, nu), 7.0)
            s_out, a_out = np.full(batch, -1, dtype=np.int32), np.full(batch, -99, dtype=np.int32)
            vec2 = ctypes.c_int(-1)
            rc = emu.emu_plant_backup_step(batch, nx, nu, c["N"], group, 256, int(shared), _ptr(A), _ptr(B), _ptr(c["d"]), _ptr(x0),
                                           _ptr(c["w"] if with_w else None), _ptr(c["fb"] if with_fb else None), _ptr(c["status"]), _ptr(c["control"]),
                                           _ptr(nxt), _ptr(x_out), _ptr(u_out), _ptr(s_out), ctypes.addressof(vec2), 0, fresh, None, None, _ptr(a_out))
            assert rc == 0
            for got, ref in zip((nxt, x_out, u_out, s_out), want[:4]):
                assert _same_bits(got, ref), (shared, with_w, with_fb, in_place, group, fresh)
            assert vec2.value == want[4]
            ok = c["status"] == 0
            assert (a_out[ok] == 0).all() and (a_out[~ok] == (FALLBACK if with_fb else HELD)).all()
    # ... and the image is the one of ABI 9: the ages take LDS only with backup plans
    emu.emu_plant_backup_lds_doubles.restype = ctypes.c_int
    emu_abi9.emu_plant_lds_doubles.restype = ctypes.c_int
    for group, shared, has_w in itertools.product((1, 6, 32), (0, 1), (0, 1)):
        assert emu.emu_plant_backup_lds_doubles(nx, nu, group, shared, has_w, 0) == emu_abi9.emu_plant_lds_doubles(nx, nu, group, shared, has_w)
        assert emu.emu_plant_backup_lds_doubles(nx, nu, group, shared, has_w, 1) > emu_abi9.emu_plant_lds_doubles(nx, nu, group, shared, has_w)


# ---- memory errors on the host ----
def test_kernel_bodies_under_the_address_and_ub_sanitizers(tmp_path):
    """tests/emu/emu_plant_backup_main.cpp: the script at (6, 3, 4), K = 3, batch 5, group 4 as a stand-alone program built with
    -fsanitize=address,undefined; every array has exactly the elements the kernel may touch.  Exit status 0 and an empty stderr."""
    exe = str(tmp_path / "emu_plant_backup_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(EMU, "emu_plant_backup.cpp"), os.path.join(EMU, "emu_plant_backup_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
