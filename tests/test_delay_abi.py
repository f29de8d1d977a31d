"""Input delay in the tick (copra_batch_set_input_delay, ABI 16) without a GPU: declared, exported, bound -- and the rule of the push and the
prediction on the kernel's own bodies (copra_amd/csrc/delay_step.hpp), which compile on the host: tests/emu/emu_delay.cpp walks the stage
and the D prediction steps thread by thread over a NaN-filled image with the guard and the walk orders of tests/emu/emu_walk.h; this file
compiles that harness itself (-ffp-contract=off).  The expectation is tests/delay_ref.py, whose row sum is written in the order of plant_row:
on the host both sides round alike and agree BIT FOR BIT; tests/test_delay_gpu.py holds the device to delay_ref's running bound."""
import ctypes
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import delay_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
NEW = ("copra_batch_set_input_delay", "copra_batch_input_delay", "copra_batch_delay_state_device", "copra_batch_get_delay_state",
       "copra_batch_delay_queue_device", "copra_batch_get_delay_queue")
VP, CI, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulonglong
SHAPES = [(6, 3), (3, 1), (5, 2)]
BATCH = 5
FAILED = 2


def _lib():
    from copra_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_capi.LIB_PATH)


# ---- surface ----
def test_header_declares_the_input_delay():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"#define\s+COPRA_DELAY_MAX\s+8\b", code)
    assert re.search(r"copra_batch_set_input_delay\s*\(\s*copra_batch_t\s*\*\s*\w*\s*,\s*int\s+\w*\s*,\s*const\s+double\s*\*\s*\w*\s*,\s*int\s+\w*\s*\)", code)
    # the rule, the shift of the schedules and the follow-ups are written down
    for words in ("oldest first", "offset + D", "backup plans", "solve_every", "per-instance delays", "fractional delays", "fusing the push"):
        assert words in text, words


def test_library_exports_the_input_delay_with_abi_16():
    lib = _lib()
    for name in NEW:
        assert hasattr(lib, name), name
    lib.copra_abi_version.restype = CI
    assert lib.copra_abi_version() >= 16
    from copra_amd import _capi
    lib.copra_batch_set_input_delay.restype = CI
    lib.copra_batch_set_input_delay.argtypes = [VP, CI, VP, CI]
    lib.copra_batch_input_delay.restype = CI
    lib.copra_batch_input_delay.argtypes = [VP]
    lib.copra_batch_delay_state_device.restype = VP
    lib.copra_batch_delay_state_device.argtypes = [VP]
    lib.copra_batch_get_delay_state.restype = CI
    lib.copra_batch_get_delay_state.argtypes = [VP, VP]
    lib.copra_batch_delay_queue_device.restype = CI
    lib.copra_batch_delay_queue_device.argtypes = [VP, VP, VP, VP]
    lib.copra_batch_get_delay_queue.restype = CI
    lib.copra_batch_get_delay_queue.argtypes = [VP, VP, VP]
    room = np.zeros(64)
    # (a NULL handle is refused before anything touches a device)
    for D in (0, 2, -1, 9):
        assert lib.copra_batch_set_input_delay(None, D, None, 0) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_input_delay(None) == -1
    assert lib.copra_batch_delay_state_device(None) is None
    assert lib.copra_batch_get_delay_state(None, room.ctypes.data) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_delay_queue_device(None, None, None, None) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_get_delay_queue(None, room.ctypes.data, None) == _capi.COPRA_ERR_ARG
    lib.copra_last_error.restype = ctypes.c_char_p
    assert b"copra_batch_get_delay_queue" in lib.copra_last_error()


def test_python_binding_has_the_input_delay():
    from copra_amd import BatchLMPC, _capi
    for name in ("set_input_delay", "delay_state", "delay_state_ptr", "delay_queue"):
        assert callable(getattr(BatchLMPC, name, None)), name
    p = inspect.signature(BatchLMPC.set_input_delay).parameters
    assert list(p)[1:] == ["steps", "u_init"] and p["u_init"].default is None
    assert BatchLMPC.DELAY_MAX == 8
    assert "prediction" in BatchLMPC.state.__doc__
    src = inspect.getsource(_capi)
    for name in NEW:
        assert "L.%s.argtypes" % name in src, name
    assert "_args.marshal" in inspect.getsource(BatchLMPC.set_input_delay)  # (host arrays and device tensors: the one path of every setter)


# ---- the kernel bodies on the host ----
class Run(ctypes.Structure):
    """EmuDelayRun of tests/emu/emu_delay.h"""
    _fields_ = ([(n, CI) for n in ("batch", "nx", "nu", "D", "head", "push", "ctrl_stride", "group", "threads", "shared", "order", "vec2_mode")]
                + [("seed", U64)] + [(n, VP) for n in ("A", "B", "d", "xnow", "q", "qs", "fallback_u", "status", "control", "x0")]
                + [("lds_doubles", CI), ("vec2_used", CI)])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_delay") / "libemu_delay.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(EMU, "emu_delay.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_delay_run.restype = CI
    lib.emu_delay_run.argtypes = [ctypes.POINTER(Run)]
    lib.emu_delay_image_bytes.restype = ctypes.c_longlong
    lib.emu_delay_image_bytes.argtypes = [CI] * 3
    lib.emu_delay_launch_group.argtypes = [CI] * 3
    lib.emu_delay_layout.argtypes = [CI] * 6 + [VP]
    return lib


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _shifted(a):
    """the same values one double off a 16-byte boundary"""
    room = np.zeros(a.size + 3, dtype=a.dtype)
    off = next(o for o in (0, 1, 2) if (room.ctypes.data + 8 * o) % 16 == 8)
    view = room[off:off + a.size].reshape(a.shape)
    view[...] = a
    assert view.ctypes.data % 16 == 8
    return view


def _model(rng, nx, nu, shared, batch=BATCH):
    lead = () if shared else (batch,)
    return 0.6 * rng.standard_normal(lead + (nx, nx)), rng.standard_normal(lead + (nx, nu)), 0.1 * rng.standard_normal(lead + (nx,))


class Device:
    """the library's state as the kernel sees it -- the ring, its statuses, xnow, x0, head -- and one launch on the emulator"""

    def __init__(self, emu, model, xnow, D, nu, u_init, N=4):
        self.emu, self.D, self.nu, self.N = emu, D, nu, N
        b = xnow.shape[0]
        A, B, d = model
        self.shared = int(A.ndim == 2)
        self.A, self.B = np.ascontiguousarray(np.swapaxes(A, -1, -2)), np.ascontiguousarray(np.swapaxes(B, -1, -2))  # (the ABI's column-major)
        self.d = np.ascontiguousarray(d)
        self.xnow = np.ascontiguousarray(xnow, dtype=np.float64).copy()
        self.ring = np.ascontiguousarray(np.repeat(u_init[:, None, :], D, axis=1))
        self.rs = np.zeros((D, b), dtype=np.int32)
        self.x0 = np.full_like(self.xnow, np.nan)
        self.head = 0

    def launch(self, push, control=None, status=None, fallback_u=None, group=4, threads=64, order=0, seed=1, vec2_mode=-1, misalign=()):
        b, nx = self.xnow.shape
        keep = dict(A=self.A, B=self.B, d=self.d, xnow=self.xnow, q=self.ring, fallback_u=fallback_u)
        for k in misalign:
            keep[k] = _shifted(keep[k])
        if push:
            self.head = (self.head + 1) % self.D
            control = np.ascontiguousarray(control, dtype=np.float64)
            status = np.ascontiguousarray(status, dtype=np.int32)
        R = Run()
        R.batch, R.nx, R.nu, R.D, R.head, R.push, R.ctrl_stride = b, nx, self.nu, self.D, self.head, int(push), self.nu * self.N
        R.group, R.threads, R.shared, R.order, R.vec2_mode, R.seed = group, threads, self.shared, order, vec2_mode, seed
        for k in ("A", "B", "d", "xnow", "q", "fallback_u"):
            setattr(R, k, None if keep[k] is None else keep[k].ctypes.data)
        R.qs, R.x0 = self.rs.ctypes.data, self.x0.ctypes.data
        R.status = status.ctypes.data if push else None
        R.control = control.ctypes.data if push else None
        assert self.emu.emu_delay_run(ctypes.byref(R)) == 0  # (-2: the guard behind the image was touched)
        if "q" in misalign:
            self.ring[...] = keep["q"]
        return R.lds_doubles, R.vec2_used

    def queue(self):
        return delay_ref.from_ring(self.ring, self.rs, self.head)


def _solve(rng, t, nx, nu, N, fail_at):
    """the `solve` of tick t: controls of a whole horizon, NaN where the instance failed"""
    control = rng.standard_normal((BATCH, nu * N))
    status = np.zeros(BATCH, dtype=np.int32)
    for i in fail_at.get(t, ()):
        status[i] = FAILED
        control[i] = np.nan
    return control, status


def _loop(emu, nx, nu, D, shared, with_fb, seed, group=4, threads=64, order=0, wseed=1, misalign=(), vec2_mode=-1, check=True):
    """2 D + 3 ticks -- the head wraps more than once -- with failed solves that reach the head, the middle and the newest slot of their
    ring, then a prediction without push from a new state; the emulator against delay_ref after every launch.  Returns what the device holds"""
    rng = np.random.default_rng(seed)
    N = 4
    model = _model(rng, nx, nu, shared)
    x0 = rng.standard_normal((BATCH, nx))
    u_init = rng.standard_normal((BATCH, nu))
    fb = rng.standard_normal((BATCH, nu)) if with_fb else None
    ref = delay_ref.DelayLoop(D, x0, nu, u_init)
    dev = Device(emu, model, x0, D, nu, u_init, N)
    kw = dict(group=group, threads=threads, order=order, seed=wseed, misalign=misalign, vec2_mode=vec2_mode)
    used = dev.launch(False, fallback_u=None, **kw)[1]  # the setter's first prediction
    ref.repredict(model)
    trace = [dev.x0.copy()]
    fail_at = {0: (1,), 1: (1, 3), 2: (4,), D + 1: (0, 2), 2 * D + 2: (3,)}
    ticks = 2 * D + 3
    untouched_x = dev.xnow.copy()
    for t in range(ticks):
        control, status = _solve(rng, t, nx, nu, N, fail_at)
        # the plant step between two launches: delay_ref's own, on the popped command (the kernel under test does not move xnow)
        want = ref.tick(model, model, control, status, fb)
        dev.xnow[...] = ref.xnow
        untouched_x = dev.xnow.copy()
        before_ring, before_rs, slot = dev.ring.copy(), dev.rs.copy(), dev.head
        dev.launch(True, control, status, fb, **kw)
        assert want is not None
        if check:
            q, qs = dev.queue()
            assert _same_bits(q, ref.q) and np.array_equal(qs, ref.qs), (nx, nu, D, t)
            assert _same_bits(dev.x0, ref.x0), (nx, nu, D, shared, with_fb, t, np.abs(dev.x0 - ref.x0).max())
            assert dev.head == ref.head
            # every double the formula does not name is unchanged: xnow, and every slot of the ring but the one that was pushed
            assert _same_bits(dev.xnow, untouched_x)
            mask = np.ones(D, dtype=bool)
            mask[slot] = False
            assert _same_bits(dev.ring[:, mask], before_ring[:, mask]) and np.array_equal(dev.rs[mask], before_rs[mask])
            assert np.isnan(dev.ring[status != 0, slot]).all()  # (a failed instance's control is never loaded: its slot reads NaN)
        trace.append(dev.x0.copy())
    # set_x0 / set_bias / set_system: the queue is kept, the prediction formed again with the push off and no fallback
    xnew = rng.standard_normal((BATCH, nx))
    ref.set_state(xnew, model)
    dev.xnow[...] = xnew
    ring, rs = dev.ring.copy(), dev.rs.copy()
    dev.launch(False, **kw)
    if check:
        assert _same_bits(dev.x0, ref.x0) and _same_bits(dev.ring, ring) and np.array_equal(dev.rs, rs) and _same_bits(dev.xnow, xnew)
    trace.append(dev.x0.copy())
    return np.stack(trace), dev, ref, used


@pytest.mark.parametrize("group", [4, 1])
@pytest.mark.parametrize("D", [1, 2, 8])
@pytest.mark.parametrize("nx,nu", SHAPES)
def test_push_and_prediction_equal_the_rule_bit_for_bit(emu, nx, nu, D, group):
    """D 1 (the slot is read by the plant and written in the same tick), 2 and 8; a model per instance and one for the batch; with and without
    fallback controls; failed entries at the head, in the middle and as the newest; batch 5 at group 4 (a partial last group) and group 1"""
    seen = set()
    for shared, with_fb in itertools.product((False, True), (False, True)):
        trace, dev, ref, _ = _loop(emu, nx, nu, D, shared, with_fb, seed=100 * nx + 10 * nu + D, group=group)
        assert np.isfinite(trace).all()
        seen |= set(np.unique(ref.qs).tolist())
    assert FAILED in seen and 0 in seen  # (failed entries were still pending at the end)


def test_a_held_entry_is_skipped_and_a_fallback_entry_moves(emu):
    """the three cases of an entry, one by one, at D = 3 with the failed entry in the middle"""
    rng = np.random.default_rng(3)
    nx, nu, D = 6, 3, 3
    model = _model(rng, nx, nu, False)
    x0, u = rng.standard_normal((BATCH, nx)), rng.standard_normal((BATCH, nu))
    fb = rng.standard_normal((BATCH, nu))
    dev = Device(emu, model, x0, D, nu, u)
    dev.rs[1, 2] = FAILED
    dev.ring[2, 1] = np.nan
    q, qs = dev.queue()
    dev.launch(False)
    want, _ = delay_ref.predict(model, x0, q, qs)
    assert _same_bits(dev.x0, want)
    two = delay_ref.DelayLoop(2, x0, nu, u)  # the held entry skipped: instance 2 is predicted over the two others alone
    assert _same_bits(dev.x0[2], two.repredict(model)[2])
    dev.launch(False, fallback_u=fb)
    want_fb, _ = delay_ref.predict(model, x0, q, qs, fb)
    assert _same_bits(dev.x0, want_fb) and not _same_bits(want_fb[2], want[2])
    mask = np.arange(BATCH) != 2
    assert _same_bits(want_fb[mask], want[mask])


def test_every_walk_order_gives_the_same_bits(emu):
    """ascending, descending and permutations, thread counts 1, 3, 64, 256, groups 1, 2, 4: the same predictions and the same queue bit for
    bit; the guard behind the image stays (launch() asserts the walker's return code)"""
    for (nx, nu), D in itertools.product(SHAPES, (1, 2, 8)):
        first = None
        for group, threads, (order, seed) in itertools.product((4, 1, 2), (64, 1, 3, 256), ((0, 0), (1, 0), (2, 11), (2, 12))):
            trace, dev, _, _ = _loop(emu, nx, nu, D, False, True, seed=7 + nx + D, group=group, threads=threads, order=order, wseed=seed, check=first is None)
            got = (trace.tobytes(), dev.ring.tobytes(), dev.rs.tobytes())
            first = got if first is None else first
            assert got == first, (nx, nu, D, group, threads, order, seed)


@pytest.mark.parametrize("nx,nu", SHAPES)
def test_one_misaligned_array_gives_the_bits_of_the_aligned_run(emu, nx, nu):
    for D, shared in itertools.product((1, 3), (False, True)):
        base, _, _, wide = _loop(emu, nx, nu, D, shared, True, seed=nx + D)
        assert wide == 1  # (numpy's arrays start on 16 bytes and the group is even)
        narrow, _, _, used = _loop(emu, nx, nu, D, shared, True, seed=nx + D, vec2_mode=0, check=False)
        assert used == 0 and _same_bits(narrow, base)
        for k in ("A", "B", "d", "xnow", "q"):
            got, _, _, used = _loop(emu, nx, nu, D, shared, True, seed=nx + D, misalign=(k,), check=False)
            assert used == 0 and _same_bits(got, base), (k, D, shared)
        odd, _, _, used = _loop(emu, nx, nu, D, shared, True, seed=nx + D, group=3, check=False)  # an odd group: no pairs
        assert used == 0 and _same_bits(odd, base)


def _layout(emu, nx, nu, D, group, shared, has_fb):
    out = np.zeros(10, dtype=np.int32)
    assert emu.emu_delay_layout(nx, nu, D, group, shared, has_fb, out.ctypes.data) == 10
    return dict(zip(("A", "B", "d", "xa", "xb", "q", "fb", "unew", "st", "total"), out.tolist()))


def test_the_launch_geometry_swept(emu):
    """nx 1 .. 144, nu 1, 2, 3, 6, D 1 .. 8, at the launch's own group and at an odd one: every part starts on 16 bytes, lies inside the image
    and overlaps no other; the group is 1 or even, at most 32, and fills the LDS target (the plant step's rule)"""
    target, top, gmax = 24 * 1024, 160 * 1024, 32
    big = 0
    for nx, nu, D in itertools.product(list(range(1, 13)) + [16, 23, 38, 64, 100, 130, 144], (1, 2, 3, 6), range(1, 9)):
        one = emu.emu_delay_image_bytes(nx, nu, D)
        group = emu.emu_delay_launch_group(nx, nu, D)
        assert one == 8 * _layout(emu, nx, nu, D, 1, 0, 1)["total"]
        assert 1 <= group <= gmax and (group == 1 or group % 2 == 0)
        assert (group == 1 or group * one <= target) and (group == gmax or (group + 2) * one > target)
        big += one > top
        for shared, has_fb, g in itertools.product((0, 1), (0, 1), (group, 3)):
            L = _layout(emu, nx, nu, D, g, shared, has_fb)
            gs = 1 if shared else g
            need = dict(A=gs * nx * nx, B=gs * nx * nu, d=gs * nx, xa=g * nx, xb=g * nx, q=g * D * nu, fb=has_fb * g * nu, unew=g * nu,
                        st=(g * (D + 1) + 1) // 2)
            spans = sorted((L[k], L[k] + n) for k, n in need.items() if n > 0)
            assert all(a % 2 == 0 for a, _ in spans) and spans[0][0] == 0 and spans[-1][1] <= L["total"]
            assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
            if g == group:
                assert 8 * L["total"] <= max(target, one)
    assert big > 0  # (the sweep reaches shapes the setter refuses)
    assert emu.emu_delay_launch_group(6, 3, 2) == 32


def test_the_running_bound_covers_another_order_of_the_sum():
    """delay_ref's bound against the same prediction in longdouble: the rounding of D steps stays inside it, and it is not vacuous"""
    rng = np.random.default_rng(5)
    nx, nu, D = 6, 3, 8
    A, B, d = _model(rng, nx, nu, False)
    x, q = rng.standard_normal((BATCH, nx)), rng.standard_normal((BATCH, D, nu))
    got, err = delay_ref.predict((A, B, d), x, q, np.zeros((BATCH, D), dtype=np.int32))
    xl = x.astype(np.longdouble)
    for j in range(D):
        xl = np.einsum("brj,bj->br", A.astype(np.longdouble), xl) + np.einsum("brc,bc->br", B.astype(np.longdouble), q[:, j].astype(np.longdouble)) + d
    e = np.abs(got - xl).astype(np.float64)
    assert (e <= err).all() and err.max() < 1e-11 * max(1.0, np.abs(got).max())


# ---- memory errors on the host ----
def test_kernel_bodies_under_the_address_and_ub_sanitizers(tmp_path):
    """tests/emu/emu_delay_main.cpp -- (6, 3) and (3, 1), batch 5, groups 4 and 1, D 1, 2, 8, both kinds of model, with and without fallback
    controls, three walk orders -- as a stand-alone program built with -fsanitize=address,undefined; every array has exactly the elements
    the kernel may touch.  Exit status 0 and an empty stderr."""
    exe = str(tmp_path / "emu_delay_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(EMU, "emu_delay.cpp"), os.path.join(EMU, "emu_delay_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
