"""Steady-state targets (copra_batch_set_target, ABI 15) without a GPU: declared, exported, bound -- and the rule on the kernel's own phase
bodies (copra_amd/csrc/target_step.hpp), which compile on the host: tests/emu/emu_target.cpp walks the four phases thread by thread over a
NaN-filled image with the guard and the walk orders of tests/emu/emu_walk.h; this file compiles that harness itself (-ffp-contract=off).
The expectation is tests/target_ref.py: numpy's solve per instance, the extended-precision truth of tests/truth.py, and a restatement of the
elimination in the order the header writes down (the emulator, which rounds every product and sum, gives its bits).

The bound, per instance, as the issue sets it:  |z - z_true|_inf <= n^2 cond_inf(M) 2^-53 |z_true|_inf, cond from numpy; for a reference
row i in addition (n + 1) 2^-53 (|T_c| |z|)_i.  numpy's own float64 solve is asserted to stay inside the same bound on every input first.
The largest error / bound seen is printed (-s)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import target_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
NEW = ("copra_target_init", "copra_batch_set_target", "copra_batch_target_device", "copra_batch_target_status_device", "copra_batch_get_target",
       "copra_batch_get_cost_reference")
TARGET_FIELDS = ["struct_size", "nr", "H", "r", "steps", "offset", "per_instance", "n_costs", "cost_index", "cost_rows", "cost_map", "on_device"]
SHAPES = [(2, 1), (3, 3), (4, 2), (6, 3), (9, 3)]
VP, CI, LL, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong
N_HORIZON = 4  # (of the S_c = N and N + 1 cases: the kernel only repeats a block S_c times)


def _lib():
    from copra_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_capi.LIB_PATH)


# ---- surface ----
def test_header_declares_the_targets():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    end = code.index("} copra_target_t;")
    body = code[code.rindex("typedef struct {", 0, end):end]
    fields = []
    for m in re.finditer(r"\b(?:const\s+)?(?:long\s+long|double|int)\s*(?:\*\s*const\s*\*|\*)?\s*([^;]+);", body):
        fields += [n.strip().lstrip("*") for n in m.group(1).split(",")]
    assert fields == TARGET_FIELDS
    assert re.search(r"copra_batch_set_target\s*\(\s*copra_batch_t\s*\*\s*\w*\s*,\s*const\s+copra_target_t\s*\*\s*\w*\s*\)", code)
    assert re.search(r"copra_batch_get_target\s*\(\s*copra_batch_t\s*\*\s*\w*\s*,\s*double\s*\*\s*\w*\s*,\s*int\s*\*\s*\w*\s*\)", code)
    assert "ties to the LOWEST row" in text and "ASCENDING" in text  # (the orders are written down)
    order = open(os.path.join(ROOT, "copra_amd", "csrc", "target_step.hpp")).read()
    assert "ties go to the LOWEST row" in order and "for j = k + 1 .. n ascending" in order and "for j = i + 1 .. n - 1 ascending" in order


def test_library_exports_the_targets_with_abi_15():
    lib = _lib()
    for name in NEW:
        assert hasattr(lib, name), name
    lib.copra_abi_version.restype = CI
    assert lib.copra_abi_version() >= 15
    from copra_amd import _capi
    lib.copra_batch_set_target.restype = CI
    lib.copra_batch_set_target.argtypes = [VP, VP]
    lib.copra_batch_get_target.restype = CI
    lib.copra_batch_get_target.argtypes = [VP, VP, VP]
    for f in ("copra_batch_target_device", "copra_batch_target_status_device"):
        getattr(lib, f).restype = VP
        getattr(lib, f).argtypes = [VP]
    room = np.zeros(64)
    # (a NULL handle is refused before anything touches a device)
    assert lib.copra_batch_set_target(None, None) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_set_target(None, room.ctypes.data) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_get_target(None, room.ctypes.data, None) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_target_device(None) is None and lib.copra_batch_target_status_device(None) is None


def test_struct_size_and_binding():
    from copra_amd import BatchLMPC, _capi
    lib = _lib()
    assert [n for n, _ in _capi.Target._fields_] == TARGET_FIELDS
    t = _capi.Target()
    ctypes.memset(ctypes.byref(t), 0xff, ctypes.sizeof(t))
    lib.copra_target_init.restype = None
    lib.copra_target_init.argtypes = [ctypes.POINTER(_capi.Target)]
    lib.copra_target_init(ctypes.byref(t))
    assert t.struct_size == ctypes.sizeof(_capi.Target) == 80
    assert not any(bool(getattr(t, f)) for f in TARGET_FIELDS[1:])
    assert ctypes.sizeof(_capi.Score) == 96 and ctypes.sizeof(_capi.PlantStep) == 104 and ctypes.sizeof(_capi.Noise) == 48  # (the others keep theirs)
    for name in ("set_target", "target", "target_status", "cost_reference"):
        assert callable(getattr(BatchLMPC, name, None)), name
    assert isinstance(inspect.getattr_static(BatchLMPC, "target_ptr"), property)
    p = inspect.signature(BatchLMPC.set_target).parameters
    assert list(p)[1:] == ["outputs", "setpoint", "costs", "offset"] and p["offset"].default == 0


# ---- the kernel bodies on the host ----
class Run(ctypes.Structure):
    """EmuTarget of tests/emu/emu_target.h"""
    _fields_ = ([(n, CI) for n in ("batch", "nx", "nu", "group", "threads", "per_instance", "order", "vec2_mode")] + [("seed", U64)]
                + [(n, VP) for n in ("A", "B", "d", "H", "r")] + [("steps", LL), ("tau", LL), ("ncost", CI)]
                + [(n, VP) for n in ("cost_rows", "cost_blocks", "cost_map", "cost_out", "z", "status")]
                + [(n, CI) for n in ("lds_doubles", "vec2_used", "nan_left")])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_target") / "libemu_target.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(EMU, "emu_target.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_target_run.restype = CI
    lib.emu_target_run.argtypes = [ctypes.POINTER(Run)]
    lib.emu_target_image_bytes.restype = LL
    lib.emu_target_image_bytes.argtypes = [CI] * 3
    lib.emu_target_launch_group.argtypes = [CI] * 3
    lib.emu_target_layout.argtypes = [CI, CI, CI, CI, VP]
    lib.emu_target_lds_max.restype = LL
    return lib


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _even(v):
    return (v + 1) & ~1


def map_doubles(case):
    n = case["nx"] + case["nu"]
    return sum(_even(T.shape[0] * n) for T, _ in case["costs"])


def launch_group(emu, case):
    """the group the launch uses, asked of the emulator (target_group of target_step.hpp)"""
    return emu.emu_target_launch_group(case["nx"], case["nu"], map_doubles(case))


def workload_model(name, batch):
    """(A, B, d, H, step maps of its two costs) of one of the three shipped workloads; H picks the positions"""
    from copra_amd import workloads
    wl = getattr(workloads, name)(batch)
    nx, nu = wl["A"].shape[1], wl["B"].shape[2]
    H = np.eye(nx)[:nu]
    maps = [target_ref.step_map(c, nx, nu, wl["N"])[0] for c in wl["costs"]]
    return wl["A"], wl["B"], wl["d"], H, maps


WORKLOADS = ["com_preview", "jerk_preview", "kinematic_preview"]


def random_model(nx, nu, batch, rng):
    """well-conditioned systems: cond_inf(M) <= 1e6 asserted, a draw that misses is drawn again"""
    A, B, H = np.zeros((batch, nx, nx)), np.zeros((batch, nx, nu)), None
    while H is None:
        Hc = rng.standard_normal((nu, nx))
        H = Hc if np.linalg.cond(Hc) < 50 else None
    for i in range(batch):
        while True:
            A[i] = np.eye(nx) + 0.5 * rng.standard_normal((nx, nx))
            B[i] = rng.standard_normal((nx, nu))
            M, _ = target_ref.systems(A[i:i + 1], B[i:i + 1], np.zeros((1, nx)), H, np.zeros((1, nu)))
            if np.linalg.cond(M[0], np.inf) <= 1e6:
                break
    return A, B, 0.1 * rng.standard_normal((batch, nx)), H


def make_case(nx, nu, batch, model, rng, per=False, steps=1, costs=None, sentinel=-7.25):
    A, B, d, H = model
    n = nx + nu
    if costs is None:
        costs = [(rng.standard_normal((nx, n)), 1), (rng.standard_normal((nu, n)), 1)]
    sig = rng.standard_normal(((batch,) if per else ()) + (steps, nu))
    c = dict(nx=nx, nu=nu, batch=batch, A=np.array(A[:batch]), B=np.array(B[:batch]), d=np.array(d[:batch]), H=np.array(H), r=sig, per=per, steps=steps, costs=costs)
    c["z0"] = np.full((batch, n), sentinel)
    c["out0"] = [np.full((batch, S * T.shape[0]), sentinel + 1 + k) for k, (T, S) in enumerate(costs)]
    return c


def _shifted(a):
    """the same values one double off a 16-byte boundary"""
    room = np.zeros(a.size + 3)
    off = 1 if room.ctypes.data % 16 == 0 else 2
    view = room[off:off + a.size].reshape(a.shape)
    view[...] = a
    assert view.ctypes.data % 16 == 8
    return view


def _aligned(a):
    room = np.zeros(a.size + 3)
    off = 0 if room.ctypes.data % 16 == 0 else 1
    view = room[off:off + a.size].reshape(a.shape)
    view[...] = a
    assert view.ctypes.data % 16 == 0
    return view


def run(emu, c, tau=0, group=None, threads=None, order=0, seed=1, vec2_mode=-1, misalign=()):
    """one launch on the emulator from the case's initial z / references; (z, status, outs, info)"""
    group = launch_group(emu, c) if group is None else group
    threads = emu.emu_target_threads() if threads is None else threads
    place = lambda k, a: (_shifted(a) if k in misalign else _aligned(a))  # noqa: E731
    keep = dict(A=place("A", np.ascontiguousarray(np.swapaxes(c["A"], -1, -2))), B=place("B", np.ascontiguousarray(np.swapaxes(c["B"], -1, -2))),
                d=place("d", c["d"]), H=np.ascontiguousarray(c["H"].T), r=np.ascontiguousarray(c["r"]))
    z = place("z", c["z0"])
    status = np.full(c["batch"], -5, dtype=np.int32)
    outs = [place("out%d" % k, o) for k, o in enumerate(c["out0"])]
    maps = [np.ascontiguousarray(T.T) for T, _ in c["costs"]]
    nc = len(maps)
    rows = (CI * max(nc, 1))(*[T.shape[0] for T, _ in c["costs"]])
    blocks = (CI * max(nc, 1))(*[S for _, S in c["costs"]])
    mp = (VP * max(nc, 1))(*[m.ctypes.data for m in maps])
    op = (VP * max(nc, 1))(*[o.ctypes.data for o in outs])
    R = Run()
    R.batch, R.nx, R.nu, R.group, R.threads, R.per_instance, R.order, R.vec2_mode, R.seed = c["batch"], c["nx"], c["nu"], group, threads, int(c["per"]), order, vec2_mode, seed
    R.A, R.B, R.d, R.H, R.r = (keep[k].ctypes.data for k in ("A", "B", "d", "H", "r"))
    R.steps, R.tau, R.ncost = c["steps"], tau, nc
    R.cost_rows, R.cost_blocks = ctypes.cast(rows, VP), ctypes.cast(blocks, VP)
    R.cost_map, R.cost_out = ctypes.cast(mp, VP), ctypes.cast(op, VP)
    R.z, R.status = z.ctypes.data, status.ctypes.data
    assert emu.emu_target_run(ctypes.byref(R)) == 0  # (-2: the guard behind the image was touched)
    assert R.nan_left == 0  # (no NaN leaves the image for a good instance)
    return np.array(z), status, [np.array(o) for o in outs], dict(lds=R.lds_doubles, vec2=R.vec2_used, group=group)


WORST = {"z": 0.0, "p": 0.0, "numpy": 0.0}


def check(c, tau, z, status, outs, must_be_singular=()):
    """status against the restated rule; good instances within the bound of the truth (numpy's own solve first), references too; singular
    instances keep their bits; the emulator's bits are the restatement's"""
    r = target_ref.setpoint(c["r"], tau, 0, c["batch"])
    M, rhs = target_ref.systems(c["A"], c["B"], c["d"], c["H"], r)
    z_rule, st_rule = target_ref.gepp(M, rhs)
    assert np.array_equal(status, st_rule), (status, st_rule)
    for i in must_be_singular:
        assert status[i] == 1, i
    good = status == 0
    bad = ~good
    assert _same_bits(z[bad], c["z0"][bad])
    for k, o in enumerate(outs):
        assert _same_bits(o[bad], c["out0"][k][bad]), k
    if not good.any():
        return
    Mg, zt = M[good], target_ref.solve_true(M[good], rhs[good])
    bound = target_ref.z_bound(Mg, zt)
    assert (bound > 0).all() and np.isfinite(bound).all()
    e64 = np.abs(target_ref.solve64(Mg, rhs[good]) - zt).max(axis=1).astype(np.float64)
    assert (e64 <= bound).all(), (e64 / bound).max()  # numpy's own float64 solve stays inside the bound
    err = np.abs(z[good] - zt).max(axis=1).astype(np.float64)
    assert np.isfinite(z[good]).all() and (err <= bound).all(), (err / bound).max()
    WORST["numpy"], WORST["z"] = max(WORST["numpy"], float((e64 / bound).max())), max(WORST["z"], float((err / bound).max()))
    assert _same_bits(z[good], z_rule[good])  # (host arithmetic: the written order, bit for bit)
    for k, (T, S) in enumerate(c["costs"]):
        p, pb = target_ref.p_true_and_bound(T, Mg, zt)
        got = outs[k][good].reshape(int(good.sum()), S, T.shape[0])
        assert np.isfinite(got).all()
        for s in range(S):
            ep = np.abs(got[:, s, :] - p)
            assert (ep <= pb).all(), (k, s, (ep / pb).max())
            WORST["p"] = max(WORST["p"], float((ep / np.maximum(pb, 1e-300)).max()))
            assert _same_bits(np.ascontiguousarray(got[:, s, :]), target_ref.rows(T, z_rule[good]))


def batches_around(group):
    return [1, group - 1, group, group + 1, 2 * group + 1]


@pytest.mark.parametrize("name", WORKLOADS)
def test_the_three_workloads_around_the_group(emu, name):
    """A - I has a zero diagonal (CoM, jerk): the first pivot is a swap.  Batches 1, group - 1, group, group + 1, 2 group + 1"""
    A, B, d, H, maps = workload_model(name, 1)
    nx, nu = A.shape[1], B.shape[2]
    case0 = dict(nx=nx, nu=nu, costs=[(T, 1) for T in maps])
    group = launch_group(emu, case0)
    assert group % 64 == 0 and 64 <= group <= emu.emu_target_threads()
    rng = np.random.default_rng(5)
    for batch in batches_around(group):
        A, B, d, H, maps = workload_model(name, batch)
        if name != "kinematic_preview":
            assert (np.diagonal(A, axis1=1, axis2=2) == 1.0).all()  # (the zero diagonal of A - I)
        d = d + 0.004 * rng.uniform(-1, 1, d.shape)  # a load per instance
        c = make_case(nx, nu, batch, (A, B, d, H), rng, costs=[(T, 1) for T in maps])
        z, status, outs, info = run(emu, c)
        assert info["group"] == group and not status.any()
        check(c, 0, z, status, outs)
        M, _ = target_ref.systems(A, B, d, H, np.zeros((batch, nu)))
        print("%s: cond_inf(M) %.1f .. %.1f" % (name, target_ref.cond_inf(M).min(), target_ref.cond_inf(M).max()))
    print("largest error / bound so far: emulator z %.3g, references %.3g, numpy z %.3g" % (WORST["z"], WORST["p"], WORST["numpy"]))


@pytest.mark.parametrize("nx,nu", SHAPES)
def test_random_models_around_the_group(emu, nx, nu):
    """cond_inf(M) <= 1e6; shared and per-instance setpoints; a signal read below, at and past its end (held at the last block)"""
    rng = np.random.default_rng(100 * nx + nu)
    case0 = make_case(nx, nu, 1, random_model(nx, nu, 1, rng), rng)
    group = launch_group(emu, case0)
    model = random_model(nx, nu, 2 * group + 1, rng)
    for k, batch in enumerate(batches_around(group)):
        per = k % 2 == 1
        c = make_case(nx, nu, batch, model, rng, per=per, steps=3)
        for tau in (0, 2, 7):
            z, status, outs, _ = run(emu, c, tau=tau)
            check(c, tau, z, status, outs)
    print("largest error / bound so far: emulator z %.3g, references %.3g, numpy z %.3g" % (WORST["z"], WORST["p"], WORST["numpy"]))


def test_the_setpoint_block_follows_tau_and_the_offset(emu):
    """a 4-step signal: tau + offset 0 .. 3 read blocks 0 .. 3, beyond it the last; a launch at (tau, offset) is the launch at tau + offset"""
    rng = np.random.default_rng(3)
    nx, nu, batch = 6, 3, 5
    for per in (False, True):
        c = make_case(nx, nu, batch, random_model(nx, nu, batch, rng), rng, per=per, steps=4)
        seen = []
        for tau, block in ((0, 0), (1, 1), (3, 3), (4, 3), (9, 3)):
            assert target_ref.block_index(tau, 0, 4) == block
            z, status, outs, _ = run(emu, c, tau=tau)
            check(c, tau, z, status, outs)
            one = dict(c, r=c["r"][..., block:block + 1, :], steps=1)  # the same launch given that block alone
            z1, _, outs1, _ = run(emu, one, tau=0)
            assert _same_bits(z, z1) and all(_same_bits(a, b) for a, b in zip(outs, outs1))
            seen.append(z)
        assert _same_bits(seen[2], seen[3]) and _same_bits(seen[3], seen[4]) and not _same_bits(seen[0], seen[1])
        # offset > 0 is added to tau by the launch: (tau 1, offset 2) reads block 3
        assert target_ref.block_index(1, 2, 4) == 3 and target_ref.block_index(1, 5, 4) == 3


@pytest.mark.parametrize("ncost", [1, 2, 8])
def test_one_two_and_eight_driven_costs(emu, ncost):
    """S_c = 1, N and N + 1; odd r_c, so that an instance's block has an odd length and the 8-byte path runs; every block of a cost equal"""
    rng = np.random.default_rng(40 + ncost)
    nx, nu, batch, n = 6, 3, 7, 9
    model = random_model(nx, nu, batch, rng)
    shapes = [(6, 1), (3, N_HORIZON), (6, N_HORIZON + 1), (5, 1), (1, N_HORIZON + 1), (2, 1), (3, 1), (4, N_HORIZON)][:ncost]
    costs = [(rng.standard_normal((r, n)), S) for r, S in shapes]
    c = make_case(nx, nu, batch, model, rng, costs=costs)
    z, status, outs, info = run(emu, c)
    check(c, 0, z, status, outs)
    for k, (r, S) in enumerate(shapes):
        assert bool(info["vec2"] >> (2 + k) & 1) == ((r * S) % 2 == 0), k
        blocks = outs[k].reshape(batch, S, r)
        assert all(_same_bits(np.ascontiguousarray(blocks[:, s]), np.ascontiguousarray(blocks[:, 0])) for s in range(S))
    assert info["vec2"] & 1 and not info["vec2"] & 2  # (pairs loaded; n = 9 is odd: z leaves in single doubles)


@pytest.mark.parametrize("nx,nu", [(6, 3), (4, 2), (2, 1)])
def test_misaligned_arrays_give_the_bits_of_the_aligned_run(emu, nx, nu):
    rng = np.random.default_rng(9 * nx + nu)
    batch, n = 5, nx + nu
    c = make_case(nx, nu, batch, random_model(nx, nu, batch, rng), rng, costs=[(rng.standard_normal((nx, n)), 2), (rng.standard_normal((nu, n)), 2)])
    z, status, outs, info = run(emu, c)
    assert info["vec2"] & 1 and info["vec2"] & 4 and info["vec2"] & 8
    for which in ("A", "B", "d", "z", "out0", "out1"):
        z2, status2, outs2, info2 = run(emu, c, misalign=(which,))
        bit = dict(A=1, B=1, d=1, z=2, out0=4, out1=8)[which]
        assert not info2["vec2"] & bit, which
        assert _same_bits(z, z2) and np.array_equal(status, status2) and all(_same_bits(a, b) for a, b in zip(outs, outs2)), which
    z3, _, outs3, info3 = run(emu, c, vec2_mode=0)
    assert info3["vec2"] == 0 and _same_bits(z, z3) and all(_same_bits(a, b) for a, b in zip(outs, outs3))


def test_singular_instances_between_good_ones(emu):
    """a zero column of B, a NaN in d, an infinite entry of A -- and, for the whole batch, H rows that repeat: status 1, z and the references
    keep their bits; the neighbours are the bits of a run without them"""
    rng = np.random.default_rng(77)
    for nx, nu in ((6, 3), (4, 2), (9, 3)):
        batch, n = 70, nx + nu
        model = random_model(nx, nu, batch, rng)
        costs = [(rng.standard_normal((nx, n)), 1), (rng.standard_normal((nu, n)), 3)]
        c = make_case(nx, nu, batch, model, rng, per=True, steps=2, costs=costs)
        z, status, outs, _ = run(emu, c, tau=1)
        assert not status.any()
        s = dict(c, B=c["B"].copy(), d=c["d"].copy(), A=c["A"].copy())
        s["B"][3][:, nu - 1] = 0.0
        s["d"][64][nx - 1] = np.nan
        s["A"][66][0, 1] = np.inf
        zs, ss, os_, _ = run(emu, s, tau=1)
        check(s, 1, zs, ss, os_, must_be_singular=(3, 64, 66))
        keep = np.ones(batch, dtype=bool)
        keep[[3, 64, 66]] = False
        assert ss.sum() == 3 and _same_bits(zs[keep], z[keep]) and all(_same_bits(a[keep], b[keep]) for a, b in zip(os_, outs))
        # H with a repeated row: every instance is singular, nothing is stored
        if nu > 1:
            h = dict(c, H=c["H"].copy())
            h["H"][nu - 1] = h["H"][0]
            zh, sh, oh, _ = run(emu, h, tau=1)
            assert sh.all() and _same_bits(zh, c["z0"]) and all(_same_bits(a, b) for a, b in zip(oh, c["out0"]))


def test_every_walk_order_gives_the_same_bits(emu):
    """ascending, descending and three permutations, thread counts 1, 3, 64, 256, groups 64 and 128 with a partial last group: the same z,
    status and references bit for bit; the guard behind the image stays and no NaN leaves it (run() asserts both)"""
    rng = np.random.default_rng(11)
    for nx, nu in SHAPES:
        n = nx + nu
        batch = 131
        c = make_case(nx, nu, batch, random_model(nx, nu, batch, rng), rng, per=True, steps=2, costs=[(rng.standard_normal((3, n)), 2), (rng.standard_normal((2, n)), 1)])
        c["d"][5][0] = np.nan
        base = run(emu, c, tau=1, group=64, threads=64)
        for group, threads, order, seed in ((64, 64, 1, 1), (64, 256, 2, 1), (64, 3, 2, 2), (128, 256, 2, 3), (128, 1, 0, 1), (128, 64, 1, 1)):
            got = run(emu, c, tau=1, group=group, threads=threads, order=order, seed=seed)
            assert _same_bits(base[0], got[0]) and np.array_equal(base[1], got[1]) and all(_same_bits(a, b) for a, b in zip(base[2], got[2]))
        assert base[1].sum() == 1 and base[1][5] == 1


def test_the_launch_geometry(emu):
    """the group is a whole number of waves, at most the kernel's threads; the image is what the layout says, every part on 16 bytes; one
    wave's image fits the CU's LDS at least up to n = 12 with eight driven costs, and stops fitting beyond"""
    top = emu.emu_target_lds_max()
    out = (CI * 5)()
    for nx in range(1, 15):
        for nu in (1, 2, 3, 6):
            n = nx + nu
            for maps in (0, _even(nx * n) + _even(nu * n), 8 * _even(nx * n)):
                g = emu.emu_target_launch_group(nx, nu, maps)
                assert g in (64, 128, 256) and g <= emu.emu_target_threads()
                assert emu.emu_target_layout(nx, nu, g, maps, out) == 5
                oM, oH, oT, ost, total = list(out)
                assert oM == 0 and oH == n * (n + 1) * g and oT == oH + _even(nu * nx) and ost == oT + maps and total == ost + _even((g + 1) // 2)
                assert all(v % 2 == 0 for v in (oH, oT, ost, total))
                assert emu.emu_target_image_bytes(nx, nu, maps) == 8 * (n * (n + 1) * 64 + _even(nu * nx) + maps + 32)
                if g > 64:
                    assert 8 * total <= 64 * 1024
                if n <= 12:
                    assert emu.emu_target_image_bytes(nx, nu, maps) <= top, (nx, nu, maps)
    assert emu.emu_target_image_bytes(9, 3, 8 * _even(9 * 12)) <= top
    assert emu.emu_target_image_bytes(16, 4, 0) > top
    assert emu.emu_target_max_costs() == 8


def test_kernel_bodies_under_the_address_and_ub_sanitizers(tmp_path):
    """tests/emu/emu_target_main.cpp -- (6, 3), (9, 3) and (2, 1), batches around a group with a partial last group, shared and per-instance
    setpoints, one to eight costs with odd rows, singular instances, three walk orders -- as a stand-alone program built with
    -fsanitize=address,undefined; every array has exactly the elements the kernel may touch.  Exit status 0."""
    exe = str(tmp_path / "emu_target_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(EMU, "emu_target.cpp"), os.path.join(EMU, "emu_target_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
