"""Closed-loop scores (copra_batch_set_score, ABI 14) without a GPU: declared, exported, bound -- and the rule of the update and the order of the
summary on the kernels' own bodies (copra_amd/csrc/score_step.hpp), which compile on the host: tests/emu/emu_score.cpp walks the four phases
thread by thread over a NaN-filled image with the guard and the walk orders of tests/emu/emu_walk.h and applies the reduction's tree lane by
lane; this file compiles that harness itself (-ffp-contract=off).  The expectation is tests/score_ref.py.

The bound on the sums.  Both sides form e = x - x_ref and every violation v = lo - z | z - hi with ONE IEEE subtraction of the same operands:
e and v are the same bits on both sides and count as data.  A product behind jx then goes through at most 2 roundings (diagonal: (q e) e) or
nx + 2 (dense: the product Q[r,j] e_j, the nx additions of the row sum, the product with e_r), through the nx additions of the fold over
the rows and through one addition per tick into the record: k = 2 max(nx, nu) + 2 + T operations after T ticks covers jx, ju, viol_sum and a
tick's lx + lu (peak).  By the standard forward bound (Higham, Accuracy and Stability, 3.1 and 3.4 -- the form tests/test_closed_loop_abi.py
derives for plant_row) every computed field differs from the exact one by at most gamma_k S, gamma_k = k u / (1 - k u), u = 2^-53, S the sum
of the absolute values of the terms; two computations of the same field, in whatever order and with whatever contraction, by at most
2 gamma_k S.  viol_max is the largest of identical values: bit for bit.  On the host the emulator and the restatement round alike, so the
error printed here is 0; tests/test_score_gpu.py uses the same bound against the device.

The bound on the summary.  A record's value reaches the result through D merges: at most CHUNK / THREADS = 4 in its thread's fold, 6 in the
lane tree, 3 in the fold of the waves, and ceil(chunks / THREADS) + 6 + 3 in stage 2 (one more for a host merge of shards).  A merge forms
mean = mean_a + delta n_b / n with 4 roundings of quantities bounded by |mean_a| + |delta| <= 3 vmax, and the mean is a convex combination
of its inputs, so errors of the inputs are not amplified:  |mean - exact| <= E = 12 D u vmax / (1 - 12 D u).  m2 = m2_a + m2_b + delta^2
n_a n_b / n has 7 roundings per merge of non-negative quantities each bounded by the exact total M, and inherits delta's error 2 E: summed
over all merges, with sum n_a n_b / n <= sum min(n_a, n_b) <= n D and Cauchy-Schwarz,
  |m2 - exact| <= gamma_{7 D} M + 4 E sqrt(M n D) + 4 E^2 n D.
The exact values are numpy's longdouble mean and sum of squared deviations."""
import ctypes
import inspect
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import score_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
NEW = ("copra_score_init", "copra_batch_set_score", "copra_batch_score_reset", "copra_batch_score_device", "copra_batch_get_score",
       "copra_batch_score_summary")
SCORE_FIELDS = ["struct_size", "qx", "ru", "dense", "x_ref", "ref_steps", "x_lo", "x_hi", "u_lo", "u_hi", "tol", "per_instance", "on_device"]
RECORD_FIELDS = ["jx", "ju", "viol_sum", "viol_max", "peak", "ticks", "held", "replayed", "fallback", "violating", "first_violation"]
STAT_FIELDS = ["n", "mean", "m2", "min", "max", "argmin", "argmax"]
SUMMARY_FIELDS = ["jx", "ju", "viol_sum", "viol_max", "peak", "ticks", "held", "replayed", "fallback", "violating", "instances_violating", "instances_held"]
SHAPES = [(6, 3), (3, 1), (1, 1), (5, 2)]
BATCH = 5
VP, CI, LL, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong
U = 2.0 ** -53
HELD, FALLBACK = score_ref.HELD, score_ref.FALLBACK


def gamma(k):
    return k * U / (1.0 - k * U)


def sum_ops(nx, nu, ticks):
    return 2 * max(nx, nu) + 2 + ticks


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
    for m in re.finditer(r"\b(?:const\s+)?(?:long\s+long|double|int|copra_score_stat_t)\s*\*?\s*([^;]+);", body):
        out += [n.strip().lstrip("*") for n in m.group(1).split(",")]
    return out


def test_header_declares_the_scores():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert _struct_fields(code, "copra_score_t") == SCORE_FIELDS
    assert _struct_fields(code, "copra_score_record_t") == RECORD_FIELDS
    assert _struct_fields(code, "copra_score_stat_t") == STAT_FIELDS
    assert _struct_fields(code, "copra_score_summary_t") == SUMMARY_FIELDS
    assert re.search(r"copra_batch_set_score\s*\(\s*copra_batch_t\s*\*\s*\w*\s*,\s*const\s+copra_score_t\s*\*\s*\w*\s*\)", code)
    assert re.search(r"copra_batch_get_score\s*\(\s*copra_batch_t\s*\*\s*\w*\s*,\s*copra_score_record_t\s*\*\s*\w*\s*\)", code)
    assert "ASCENDING" in text and "lane l <- merge(lane l, lane l + off)" in text  # (the orders are written down)


def test_library_exports_the_scores_with_abi_14():
    lib = _lib()
    for name in NEW:
        assert hasattr(lib, name), name
    lib.copra_abi_version.restype = CI
    assert lib.copra_abi_version() >= 14
    from copra_amd import _capi
    for name in ("copra_batch_set_score", "copra_batch_get_score", "copra_batch_score_summary"):
        getattr(lib, name).restype = CI
        getattr(lib, name).argtypes = [VP, VP]
    lib.copra_batch_score_reset.restype = CI
    lib.copra_batch_score_reset.argtypes = [VP]
    lib.copra_batch_score_device.restype = VP
    lib.copra_batch_score_device.argtypes = [VP]
    room = np.zeros(64)
    # (a NULL handle is refused before anything touches a device)
    assert lib.copra_batch_set_score(None, None) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_set_score(None, room.ctypes.data) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_score_reset(None) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_get_score(None, room.ctypes.data) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_score_summary(None, room.ctypes.data) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_score_device(None) is None


def test_struct_sizes():
    from copra_amd import _capi
    lib = _lib()
    assert [n for n, _ in _capi.Score._fields_] == SCORE_FIELDS
    assert [n for n, _ in _capi.ScoreRecord._fields_] == RECORD_FIELDS
    assert [n for n, _ in _capi.ScoreStat._fields_] == STAT_FIELDS
    assert [n for n, _ in _capi.ScoreSummary._fields_] == SUMMARY_FIELDS
    assert ctypes.sizeof(_capi.ScoreRecord) == 64 == _capi.SCORE_RECORD_DTYPE.itemsize == score_ref.RECORD.itemsize
    assert list(_capi.SCORE_RECORD_DTYPE.names) == RECORD_FIELDS == list(score_ref.RECORD.names)
    assert ctypes.sizeof(_capi.ScoreStat) == 56 and ctypes.sizeof(_capi.ScoreSummary) == 5 * 56 + 7 * 8
    m = _capi.Score()
    ctypes.memset(ctypes.byref(m), 0xff, ctypes.sizeof(m))
    lib.copra_score_init.restype = None
    lib.copra_score_init.argtypes = [ctypes.POINTER(_capi.Score)]
    lib.copra_score_init(ctypes.byref(m))
    assert m.struct_size == ctypes.sizeof(_capi.Score) == 96
    assert not any(getattr(m, f) for f in SCORE_FIELDS[1:])
    # the step structs and the noise keep their sizes
    assert ctypes.sizeof(_capi.PlantStep) == 104
    assert ctypes.sizeof(_capi.PlantStepEx) == ctypes.sizeof(_capi.PlantStep) + 2 * ctypes.sizeof(VP)
    assert ctypes.sizeof(_capi.PlantStepObs) == ctypes.sizeof(_capi.PlantStepEx) + 7 * ctypes.sizeof(VP)
    assert ctypes.sizeof(_capi.Noise) == 48
    for init, struct in (("copra_plant_step_init", _capi.PlantStep), ("copra_plant_step_ex_init", _capi.PlantStepEx),
                         ("copra_plant_step_obs_init", _capi.PlantStepObs), ("copra_noise_init", _capi.Noise)):
        s = struct()
        getattr(lib, init).restype = None
        getattr(lib, init).argtypes = [VP]
        getattr(lib, init)(ctypes.byref(s))
        assert s.struct_size == ctypes.sizeof(struct), init


def test_python_binding_has_the_scores():
    from copra_amd import BatchLMPC, sharding
    for name in ("set_score", "reset_score", "score", "score_summary"):
        assert callable(getattr(BatchLMPC, name, None)), name
    assert isinstance(inspect.getattr_static(BatchLMPC, "score_ptr"), property)
    p = inspect.signature(BatchLMPC.set_score).parameters
    assert list(p)[1:] == ["state_weights", "control_weights", "state_ref", "state_limits", "control_limits", "tol"]
    assert all(p[k].default is None for k in list(p)[1:6]) and p["tol"].default == 0.0
    assert list(inspect.signature(sharding.merge_score_summaries).parameters) == ["summaries", "first_instances"]


# ---- the kernel bodies on the host ----
class Tick(ctypes.Structure):
    """EmuScoreTick of tests/emu/emu_score.h"""
    _fields_ = ([(n, CI) for n in ("batch", "nx", "nu", "group", "threads", "dense", "per_instance", "order", "vec2_mode")] + [("seed", U64)]
                + [(n, VP) for n in ("x", "u", "age", "qx", "ru", "x_ref")] + [("ref_steps", LL), ("tau", LL)]
                + [(n, VP) for n in ("x_lo", "x_hi", "u_lo", "u_hi")] + [("tol", ctypes.c_double), ("rec", VP), ("lds_doubles", CI), ("vec2_used", CI)])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_score") / "libemu_score.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(EMU, "emu_score.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.emu_score_tick.restype = CI
    lib.emu_score_tick.argtypes = [ctypes.POINTER(Tick)]
    lib.emu_score_reduce.restype = CI
    lib.emu_score_reduce.argtypes = [LL, VP, VP]
    lib.emu_score_image_bytes.restype = LL
    lib.emu_score_image_bytes.argtypes = [CI] * 3
    lib.emu_score_launch_group.argtypes = [CI] * 3
    lib.emu_score_layout.argtypes = [CI, CI, CI, VP, VP]
    return lib


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _case(nx, nu, dense, per, steps, seed, batch=BATCH, ages=(0, 2, FALLBACK, HELD, HELD)):
    """a measure in natural indexing, and three ticks' states, controls and ages: ages 0, 2, FALLBACK and HELD in one batch, NaN in the held
    instances' controls, infinite limits among the finite ones"""
    rng = np.random.default_rng(seed)
    lead = (batch,) if per else ()
    sym = lambda n: (lambda m: m @ np.swapaxes(m, -1, -2) + 0.1 * rng.standard_normal(lead + (n, n)))(rng.standard_normal(lead + (n, n)))  # noqa: E731
    c = dict(nx=nx, nu=nu, dense=dense, per=per, batch=batch)
    c["qx"] = sym(nx) if dense else rng.uniform(0.1, 2.0, lead + (nx,))
    c["ru"] = sym(nu) if dense else rng.uniform(0.1, 2.0, lead + (nu,))
    c["x_ref"] = rng.standard_normal(lead + (steps, nx))
    c["x_lo"], c["x_hi"] = rng.uniform(-1.5, -0.5, lead + (nx,)), rng.uniform(0.5, 1.5, lead + (nx,))
    c["u_lo"], c["u_hi"] = rng.uniform(-1.5, -0.5, lead + (nu,)), rng.uniform(0.5, 1.5, lead + (nu,))
    c["x_hi"][..., 0] = np.inf
    c["u_lo"][..., nu - 1] = -np.inf
    age = np.resize(np.asarray(ages, dtype=np.int32), batch)
    c["ticks"] = []
    for t in range(3):
        x, u = 1.5 * rng.standard_normal((batch, nx)), 1.5 * rng.standard_normal((batch, nu))
        a = np.roll(age, t).astype(np.int32)
        u[a == HELD] = np.nan
        c["ticks"].append((x, u, a))
    return c


MEASURE = ("qx", "ru", "x_ref", "x_lo", "x_hi", "u_lo", "u_hi")


def _abi(c, k):
    """array k of a case in the ABI's layout (dense weights column-major)"""
    a = c.get(k)
    if a is None:
        return None
    if k in ("qx", "ru") and c["dense"]:
        a = np.swapaxes(a, -1, -2)
    return np.ascontiguousarray(a, dtype=np.float64)


def _shifted(a):
    """the same values one double off a 16-byte boundary"""
    room = np.zeros(a.size + 3)
    off = 1 if room.ctypes.data % 16 == 0 else 2
    off = off if (room.ctypes.data + 8 * off) % 16 == 8 else off + 1
    view = room[off:off + a.size].reshape(a.shape)
    view[...] = a
    assert view.ctypes.data % 16 == 8
    return view


def run(emu, c, rec, t, tau, group, threads=64, order=0, seed=1, tol=0.25, misalign=None, vec2_mode=-1, drop=()):
    """tick t of case c on the emulator, rec updated in place; returns (image doubles, whether pairs were copied)"""
    x, u, age = c["ticks"][t]
    keep = {k: (None if k in drop else _abi(c, k)) for k in MEASURE}
    keep["x"], keep["u"] = np.ascontiguousarray(x), np.ascontiguousarray(u)
    if misalign:
        keep[misalign] = _shifted(keep[misalign])
    T = Tick()
    T.batch, T.nx, T.nu, T.group, T.threads, T.dense, T.per_instance, T.order, T.vec2_mode, T.seed = c["batch"], c["nx"], c["nu"], group, threads, int(c["dense"]), int(c["per"]), order, vec2_mode, seed
    T.x, T.u, T.age = keep["x"].ctypes.data, keep["u"].ctypes.data, age.ctypes.data
    for k in MEASURE:
        setattr(T, k, None if keep[k] is None else keep[k].ctypes.data)
    T.ref_steps, T.tau, T.tol, T.rec = c["x_ref"].shape[-2], tau, tol, rec.ctypes.data
    assert emu.emu_score_tick(ctypes.byref(T)) == 0  # (-2: the guard behind the image was touched)
    return T.lds_doubles, T.vec2_used


def ref_update(c, rec, t, tau, tol=0.25, drop=()):
    x, u, age = c["ticks"][t]
    kw = {k: (None if k in drop else c[k]) for k in MEASURE}
    return score_ref.update(rec, x, u, age, tau, tol=tol, dense=c["dense"], per_instance=c["per"], **kw)


def check_records(got, want, S, k, what, worst):
    """counters and viol_max exact; the sums within 2 gamma_k S; returns the largest error / bound seen"""
    for f in ("ticks", "held", "replayed", "fallback", "violating", "first_violation"):
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])
    assert _same_bits(got["viol_max"], want["viol_max"]), what
    for f in ("jx", "ju", "viol_sum", "peak"):
        bound = 2.0 * gamma(k) * S[f]
        err = np.abs(got[f] - want[f])
        assert np.isfinite(got[f]).all() and (err <= bound).all(), (what, f, err, bound)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def abs_sums(c, taus, drop=()):
    """S per field after the case's three ticks"""
    S = {f: np.zeros(c["batch"]) for f in ("jx", "ju", "viol_sum", "peak")}
    for t, tau in enumerate(taus):
        x, u, age = c["ticks"][t]
        kw = dict(qx=None if "qx" in drop else c["qx"], ru=None if "ru" in drop else c["ru"], x_ref=None if "x_ref" in drop else c["x_ref"])
        ax, au = score_ref.abs_terms(x, u, age, tau, dense=c["dense"], per_instance=c["per"], **kw)
        S["jx"] += ax
        S["ju"] += au
        S["peak"] = np.maximum(S["peak"], ax + au)
    return S


@pytest.mark.parametrize("group", [4, 1])
@pytest.mark.parametrize("nx,nu", SHAPES)
def test_three_ticks_equal_three_applications_of_the_rule(emu, nx, nu, group):
    """diagonal and dense, shared and per instance, ref_steps 1 and 4 with tau below, at and beyond the end, with and without each optional array;
    batch 5 at group 4 (a partial last group) and group 1"""
    worst, held_checked = 0.0, 0
    for dense, per, steps in itertools.product((False, True), (False, True), (1, 4)):
        c = _case(nx, nu, dense, per, steps, seed=1000 * nx + 100 * nu + 10 * dense + 2 * per + steps)
        drops = [()] + [(k,) for k in MEASURE] + [("x_lo", "x_hi", "u_lo", "u_hi")] if (dense, per) == (False, False) or steps == 4 else [()]
        for drop in drops:
            got, want = score_ref.zero_records(BATCH), score_ref.zero_records(BATCH)
            got["first_violation"] = 0
            taus = (2, 3, 7)  # below the end of a 4-step signal, at its last row, beyond it
            before = None
            for t, tau in enumerate(taus):
                held = c["ticks"][t][2] == HELD
                before = got["ju"][held].copy()
                run(emu, c, got, t, tau, group, drop=drop)
                ref_update(c, want, t, tau, drop=drop)
                assert _same_bits(got["ju"][held], before), (nx, nu, drop)  # a held instance's ju keeps its bits
                held_checked += int(held.sum())
            S = abs_sums(c, taus, drop)
            S["viol_sum"] = want["viol_sum"].copy()  # (non-negative terms: their sum is the sum of their absolute values)
            worst = check_records(got, want, S, sum_ops(nx, nu, 3), (nx, nu, group, dense, per, steps, drop), worst)
            assert (got["ticks"] == 3).all() and got["held"].sum() == 6 and got["replayed"].sum() == 3 and got["fallback"].sum() == 3
            if not set(drop) & {"x_lo", "x_hi"}:
                assert got["violating"].sum() > 0 and (got["first_violation"][got["violating"] > 0] >= 1).all()
            if drop == ("x_lo", "x_hi", "u_lo", "u_hi"):
                assert (got["violating"] == 0).all() and (got["viol_sum"] == 0).all() and (got["first_violation"] == 0).all()
            if "qx" in drop:
                assert (got["jx"] == 0).all()
    assert held_checked > 0
    print("(%d, %d) group %d: largest error / bound of the sums %.3g" % (nx, nu, group, worst))


def test_the_reference_row_follows_tau(emu):
    """a 4-step signal: tau 0 .. 3 read rows 0 .. 3, tau 9 the last; a constant goal never moves"""
    c = _case(6, 3, False, True, 4, seed=77)
    for tau, row in ((0, 0), (1, 1), (3, 3), (4, 3), (9, 3)):
        got, want = score_ref.zero_records(BATCH), score_ref.zero_records(BATCH)
        run(emu, c, got, 0, tau, 4)
        fixed = dict(c, x_ref=np.ascontiguousarray(c["x_ref"][:, row:row + 1]))
        ref_update(fixed, want, 0, 0)
        assert _same_bits(got, want), tau


def test_every_walk_order_gives_the_same_bits_and_no_nan_leaves(emu):
    """ascending, descending and three permutations, thread counts 1, 3, 64, 256, groups 1, 2, 4: the same records bit for bit; the guard
    behind the image stays (run() asserts the walker's return code); NaN reaches no field but through a NaN input"""
    for (nx, nu), dense, per in itertools.product(SHAPES, (False, True), (False, True)):
        c = _case(nx, nu, dense, per, 4, seed=5 + nx)
        first = None
        for group, threads, (order, seed) in itertools.product((4, 1, 2), (64, 1, 3, 256), ((0, 0), (1, 0), (2, 11), (2, 12), (2, 13))):
            rec = score_ref.zero_records(BATCH)
            for t in range(3):
                run(emu, c, rec, t, t + 2, group, threads=threads, order=order, seed=seed)
            first = rec if first is None else first
            assert _same_bits(rec, first), (nx, nu, dense, per, group, threads, order, seed)
        for f in score_ref.FIELDS:
            assert np.isfinite(first[f]).all(), f
    # ... and through a NaN input: a NaN state makes jx NaN for that instance alone, a NaN reference likewise
    c = _case(6, 3, False, True, 1, seed=3)
    c["ticks"][0][0][1, 2] = np.nan
    c["x_ref"][3, 0, 4] = np.nan
    rec = score_ref.zero_records(BATCH)
    run(emu, c, rec, 0, 0, 4)
    assert np.isnan(rec["jx"]).tolist() == [False, True, False, True, False]
    assert np.isfinite(rec["ju"]).all() and np.isfinite(rec["viol_sum"]).all() and np.isfinite(rec["viol_max"]).all()
    want = score_ref.zero_records(BATCH)
    ref_update(c, want, 0, 0)
    assert _same_bits(rec, want)


@pytest.mark.parametrize("nx,nu", SHAPES)
def test_one_misaligned_array_gives_the_bits_of_the_aligned_run(emu, nx, nu):
    for dense, per in itertools.product((False, True), (False, True)):
        c = _case(nx, nu, dense, per, 4, seed=9 * nx + nu)
        base = score_ref.zero_records(BATCH)
        _, wide = run(emu, c, base, 0, 2, 4)
        assert wide == 1  # (numpy's arrays start on 16 bytes, the group is even, row 2 of a signal starts on 16 bytes whatever nx)
        narrow = score_ref.zero_records(BATCH)
        assert run(emu, c, narrow, 0, 2, 4, vec2_mode=0)[1] == 0 and _same_bits(narrow, base)
        for k in ("x", "u") + MEASURE:
            rec = score_ref.zero_records(BATCH)
            _, used = run(emu, c, rec, 0, 2, 4, misalign=k)
            assert used == 0 and _same_bits(rec, base), (k, dense, per)
        odd = score_ref.zero_records(BATCH)
        assert run(emu, c, odd, 0, 2, 3)[1] == 0 and _same_bits(odd, base)  # an odd group: no pairs
    # a shared signal of odd nx: its odd rows start off 16 bytes -- the rule sees the ROW, not the array
    c = _case(5, 2, False, False, 4, seed=4)
    for tau, wide in ((0, 1), (1, 0), (2, 1)):
        assert run(emu, c, score_ref.zero_records(BATCH), 0, tau, 4)[1] == wide


def _layout(emu, nx, nu, group, flags):
    f = np.asarray(flags, dtype=np.int32)
    out = np.zeros(14, dtype=np.int32)
    assert emu.emu_score_layout(nx, nu, group, f.ctypes.data, out.ctypes.data) == 14
    return dict(zip(("x", "u", "age", "rec", "qx", "ru", "ref", "x_lo", "x_hi", "u_lo", "u_hi", "terms", "viol", "total"), out.tolist()))


def test_the_launch_geometry_swept(emu):
    """nx 1 .. 144, nu 1, 2, 3, 6, every combination of the layout's flags, at the launch's own group and at an odd one: every part starts on
    16 bytes, lies inside the image and overlaps no other; the group is 1 or even, at most 32, and fills the LDS target; the image of the
    launch never exceeds max(target, one instance's widest image)"""
    target, top, gmax = 24 * 1024, 160 * 1024, 32
    big = 0
    for nx, nu in itertools.product(list(range(1, 13)) + [16, 23, 38, 64, 77, 100, 130, 144], (1, 2, 3, 6)):
        for dense in (0, 1):
            one = emu.emu_score_image_bytes(nx, nu, dense)
            group = emu.emu_score_launch_group(nx, nu, dense)
            assert one == 8 * _layout(emu, nx, nu, 1, (dense, 1) + (1,) * 7)["total"]
            assert 1 <= group <= gmax and (group == 1 or group % 2 == 0)
            assert (group == 1 or group * one <= target) and (group == gmax or (group + 2) * one > target)
            big += one > top
            for per, rest in itertools.product((0, 1), itertools.product((0, 1), repeat=7)):
                for g in (group, 3):
                    L = _layout(emu, nx, nu, g, (dense, per) + rest)
                    gs = g if per else 1
                    need = dict(x=g * nx, u=g * nu, age=(g + 1) // 2, rec=8 * g, qx=rest[0] * gs * (nx * nx if dense else nx),
                                ru=rest[1] * gs * (nu * nu if dense else nu), ref=rest[2] * gs * nx, x_lo=rest[3] * gs * nx, x_hi=rest[4] * gs * nx,
                                u_lo=rest[5] * gs * nu, u_hi=rest[6] * gs * nu, terms=g * (nx + nu), viol=g * (nx + nu))
                    spans = sorted((L[k], L[k] + n) for k, n in need.items() if n > 0)
                    assert all(a % 2 == 0 for a, _ in spans) and spans[0][0] == 0 and spans[-1][1] <= L["total"]
                    assert all(spans[i][1] <= spans[i + 1][0] for i in range(len(spans) - 1))
                    if g == group:
                        assert 8 * L["total"] <= max(target, one)
    assert big > 0  # (the sweep reaches shapes the setter refuses)
    assert emu.emu_score_launch_group(6, 3, 0) == 32 and emu.emu_score_image_bytes(6, 3, 0) == 8 * _layout(emu, 6, 3, 1, (0, 1) + (1,) * 7)["total"]


# ---- the reduction ----
def _records(count, seed):
    """records with one NaN and one inf planted, a tie for the maximum, and an all-NaN field (peak)"""
    rng = np.random.default_rng(seed)
    rec = score_ref.zero_records(count)
    rec["jx"] = 10.0 + 0.3 * rng.standard_normal(count)
    rec["ju"] = rng.uniform(0.0, 5.0, count)
    rec["viol_sum"] = rng.uniform(0.0, 1.0, count) * (rng.uniform(size=count) < 0.4)
    rec["viol_max"] = 0.5 * rec["viol_sum"]
    rec["peak"] = np.nan
    rec["ticks"] = 9
    rec["held"] = rng.integers(0, 3, count) * (rng.uniform(size=count) < 0.3)
    rec["replayed"] = rng.integers(0, 4, count)
    rec["fallback"] = rng.integers(0, 2, count)
    rec["violating"] = (rec["viol_sum"] > 0) * rng.integers(1, 5, count)
    if count >= 3:
        rec["jx"][count // 2] = np.nan
        rec["ju"][count // 3] = np.inf
        top = rec["ju"][np.isfinite(rec["ju"])].max() + 1.0
        rec["ju"][[count - 1, 1]] = top  # a tie for the maximum: the lowest index wins
    return rec


def _emu_summary(emu, rec):
    out = np.zeros(42, dtype=np.int64)
    assert emu.emu_score_reduce(len(rec), rec.ctypes.data, out.ctypes.data) == 0
    s = {}
    for i, f in enumerate(score_ref.FIELDS):
        w = out[7 * i:7 * i + 7]
        d = w.view(np.float64)
        s[f] = dict(n=int(w[0]), mean=float(d[1]), m2=float(d[2]), min=float(d[3]), max=float(d[4]), argmin=int(w[5]), argmax=int(w[6]))
    s.update({k: int(out[35 + i]) for i, k in enumerate(score_ref.TOTALS)})
    return s


def _stat_bits(a):
    return (a["n"], np.float64(a["mean"]).tobytes(), np.float64(a["m2"]).tobytes(), np.float64(a["min"]).tobytes(), np.float64(a["max"]).tobytes(), a["argmin"], a["argmax"])


def summary_bounds(values, depth):
    """(E, the bound on m2) of the module's docstring for the finite ones of `values` after `depth` merges"""
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    if v.size == 0:
        return 0.0, 0.0
    n, _, M = score_ref.exact_stats(v)
    vmax, M = float(np.abs(v).max()), float(M)
    E = 12 * depth * U * vmax / (1 - 12 * depth * U)
    return E, gamma(7 * depth) * M + 4 * E * math.sqrt(M * n * depth) + 4 * E * E * n * depth


def merge_depth(count, extra=0):
    chunks = -(-count // score_ref.CHUNK)
    return score_ref.CHUNK // score_ref.THREADS + 9 + -(-chunks // score_ref.THREADS) + 9 + extra


def check_summary(s, rec, depth, worst=0.0):
    """counts, min, max and args exact against numpy; mean and m2 within the bound against longdouble; returns the largest error / bound"""
    for f in score_ref.FIELDS:
        v = rec[f]
        fin = np.isfinite(v)
        st = s[f]
        assert st["n"] == int(fin.sum()), f
        if st["n"] == 0:
            assert (st["mean"], st["m2"], st["min"], st["max"], st["argmin"], st["argmax"]) == (0.0, 0.0, np.inf, -np.inf, -1, -1), f
            continue
        idx = np.nonzero(fin)[0]
        assert st["min"] == v[idx].min() and st["max"] == v[idx].max(), f
        assert st["argmin"] == idx[np.argmin(v[idx])] and st["argmax"] == idx[np.argmax(v[idx])], f  # (numpy's arg: the first, the lowest index)
        n, mean, m2 = score_ref.exact_stats(v)
        E, B = summary_bounds(v, depth)
        e1, e2 = abs(float(np.longdouble(st["mean"]) - mean)), abs(float(np.longdouble(st["m2"]) - m2))
        assert e1 <= E and e2 <= B, (f, e1, E, e2, B)
        worst = max(worst, e1 / E if E else 0.0, e2 / B if B else 0.0)
    for k in score_ref.COUNTERS:
        assert s[k] == int(rec[k].astype(np.int64).sum()), k
    assert s["instances_violating"] == int((rec["violating"] != 0).sum()) and s["instances_held"] == int((rec["held"] != 0).sum())
    return worst


COUNTS = [1, 63, 64, 65, score_ref.CHUNK - 1, score_ref.CHUNK, score_ref.CHUNK + 1, 2 * score_ref.CHUNK + 1]


@pytest.mark.parametrize("count", COUNTS)
def test_the_emulated_tree_is_the_written_order(emu, count):
    """the tree applied lane by lane on the kernel's own merge == score_ref's restatement of the written order, bit for bit; both within the
    bound of numpy's longdouble mean and m2; counts, min, max, args exact; the all-NaN field has n == 0"""
    assert emu.emu_score_chunk() == score_ref.CHUNK and emu.emu_score_threads() == score_ref.THREADS
    rec = _records(count, seed=count)
    got, want = _emu_summary(emu, rec), score_ref.summary(rec)
    for f in score_ref.FIELDS:
        assert _stat_bits(got[f]) == _stat_bits(want[f]), (f, got[f], want[f])
    assert all(got[k] == want[k] for k in score_ref.TOTALS)
    worst = check_summary(got, rec, merge_depth(count))
    assert got["peak"]["n"] == 0
    if count >= 3:
        assert got["jx"]["n"] == count - 1 and got["ju"]["n"] == count - 1 and got["ju"]["argmax"] == 1
    again = _emu_summary(emu, rec)
    assert all(_stat_bits(got[f]) == _stat_bits(again[f]) for f in score_ref.FIELDS)
    print("%d records: largest error / bound of mean and m2 against longdouble %.3g" % (count, worst))


def test_an_empty_batch_and_a_shuffle(emu):
    s = _emu_summary(emu, score_ref.zero_records(0))
    assert s["jx"] == score_ref.stat_empty() and s["ticks"] == 0
    # the order is a function of the index: the same records in another order give other bits in general, the same counts and extremes
    rec = _records(700, seed=2)
    a, b = _emu_summary(emu, rec), _emu_summary(emu, rec[::-1].copy())
    assert a["jx"]["n"] == b["jx"]["n"] and a["jx"]["min"] == b["jx"]["min"] and a["jx"]["argmin"] == 699 - b["jx"]["argmin"]


def test_merge_score_summaries_of_two_halves(emu):
    """two halves cut at a chunk boundary, merged on the host with the same rule: every count, min, max and arg of the whole, mean and m2 within
    the bound (one merge deeper)"""
    from copra_amd import sharding
    count, cut = 2 * score_ref.CHUNK + 1, score_ref.CHUNK
    rec = _records(count, seed=8)
    whole = _emu_summary(emu, rec)
    parts = [_emu_summary(emu, np.ascontiguousarray(rec[:cut])), _emu_summary(emu, np.ascontiguousarray(rec[cut:]))]
    merged = sharding.merge_score_summaries(parts, [0, cut])
    for k in score_ref.TOTALS:
        assert merged[k] == whole[k], k
    for f in score_ref.FIELDS:
        for k in ("n", "min", "max", "argmin", "argmax"):
            assert merged[f][k] == whole[f][k], (f, k)
    worst = check_summary(merged, rec, merge_depth(count, 1))
    print("two halves merged: largest error / bound %.3g" % worst)
    # the host rule is the device's: merging with score_ref's rule gives the same bits
    for f in score_ref.FIELDS:
        a = dict(parts[1][f])
        a["argmin"], a["argmax"] = (a["argmin"] + cut if a["argmin"] >= 0 else -1), (a["argmax"] + cut if a["argmax"] >= 0 else -1)
        assert _stat_bits(score_ref.stat_merge(parts[0][f], a)) == _stat_bits(merged[f]), f
    assert sharding.merge_score_summaries([], [])["jx"]["n"] == 0
    with pytest.raises(ValueError):
        sharding.merge_score_summaries(parts, [0])


# ---- memory errors on the host ----
def test_kernel_bodies_under_the_address_and_ub_sanitizers(tmp_path):
    """tests/emu/emu_score_main.cpp -- (6, 3) and (3, 1), batch 5, groups 4 and 1, every kind of measure, three walk orders, and the reduction at
    its edge counts -- as a stand-alone program built with -fsanitize=address,undefined; every array has exactly the elements the kernel may
    touch.  Exit status 0 and an empty stderr."""
    exe = str(tmp_path / "emu_score_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(EMU, "emu_score.cpp"), os.path.join(EMU, "emu_score_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
