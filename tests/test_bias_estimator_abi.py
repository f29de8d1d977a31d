"""The disturbance estimator of the tick (copra_batch_set_bias_estimator, ABI 11) without a GPU: declared, exported, bound -- and the rule itself
on the phases of the plant-step kernel (copra_amd/csrc/plant_step.hpp), which compile on the host: tests/emu/emu_plant_bias.cpp walks them
thread by thread over a NaN-filled image, this file compiles that harness itself.

The expectation is a numpy.longdouble restatement of the rule in include/copra_hip.h (reference_bias).  x+ is compared with reference_step within
step_bound, both of tests/test_closed_loop_abi.py.  The bound on dhat+ is derived the same way -- every rounding of a partial sum is at most
2^-53 times the sum of the absolute values of its terms, products counted as one rounding more -- with u = 2^-53:

  x+ as computed differs from the exact x+ of the same inputs by at most       Ex = step_bound(nx, nu, Sx),   Sx = |dp| + |Ap||x| + |Bp||u| + |w|
  pred has the same chain without w:                                          Ep = step_bound(nx, nu, Sp),   Sp = |dhat| + |Am||x| + |Bm||u|
  e = fl(x+ - pred): one more rounding of a difference of size at most        Se = Sx + Sp:                  Ee = Ex + Ep + u Se
  dhat+ = dhat + sum_j L[r,j] e_j, n terms (n = nx dense, 1 diagonal): the errors of e pass through |L|, and the chain itself has n products
  and n additions -- counted as 2 (n + 1) roundings, as step_bound counts its own -- of partial sums of size at most |dhat| + |L| Se:
                                                                              bias_bound = |L| Ee + 2 (n + 1) u (|dhat| + |L| Se)
Nothing in it is fitted to what the kernel gives.  u_out, ages, held states and held estimates are copies: compared bit for bit."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from test_backup_plan_abi import BATCH, FRESH, _rule, _same_bits, _script
from test_closed_loop_abi import _case, _ptr, _run, reference_step, step_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
FALLBACK, HELD = -1, -2
NEW = ("copra_batch_set_bias_estimator", "copra_batch_set_bias", "copra_batch_bias_device", "copra_batch_get_bias")
LD = np.longdouble
U = 2.0 ** -53


def _lib():
    from copra_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_capi.LIB_PATH)


# ---- the rule, restated ----
def _per_instance(v, batch, ndim):
    v = np.asarray(v, dtype=LD)
    return np.broadcast_to(v, (batch,) + v.shape) if v.ndim == ndim else v


def reference_bias(Am, Bm, dhat, x, u, xplus, Sx, gain, dense):
    """dhat+ of the rule and its bound in numpy.longdouble.  Am (b, nx, nx), Bm (b, nx, nu) in natural indexing; xplus, Sx: the exact next
    state of the same inputs and its scale (reference_step); gain (nx,) / (b, nx) diagonal or (nx, nx) / (b, nx, nx) dense, natural indexing.
    Rows of instances that were held are meaningless: the caller masks them."""
    b, nx = x.shape
    nu = u.shape[1]
    Am, Bm, dhat, x, u = (np.asarray(v, dtype=LD) for v in (Am, Bm, dhat, x, u))
    pred = dhat + (Am * x[:, None, :]).sum(axis=2) + (Bm * u[:, None, :]).sum(axis=2)
    Sp = np.abs(dhat) + (np.abs(Am) * np.abs(x)[:, None, :]).sum(axis=2) + (np.abs(Bm) * np.abs(u)[:, None, :]).sum(axis=2)
    e = np.asarray(xplus, dtype=LD) - pred
    Se = np.asarray(Sx, dtype=LD) + Sp
    Ee = step_bound(nx, nu, Sx) + step_bound(nx, nu, Sp) + U * Se
    if dense:
        L = _per_instance(gain, b, 2)
        upd = (L * e[:, None, :]).sum(axis=2)
        absL = np.abs(L)
        bound = (absL * Ee[:, None, :]).sum(axis=2) + 2 * (nx + 1) * U * (np.abs(dhat) + (absL * Se[:, None, :]).sum(axis=2))
    else:
        l = _per_instance(gain, b, 1)
        upd = l * e
        bound = np.abs(l) * Ee + 2 * 2 * U * (np.abs(dhat) + np.abs(l) * Se)
    return dhat + upd, bound


def abi_gain(gain, dense):
    """natural indexing -> the ABI's column-major blocks"""
    g = np.asarray(gain, dtype=np.float64)
    return np.ascontiguousarray(np.swapaxes(g, -1, -2) if dense else g)


# ---- surface ----
def test_header_declares_the_estimator():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    assert re.search(r"\bcopra_plant_step_ex_init\s*\(\s*copra_plant_step_ex_t\s*\*", code)
    # the two outputs are appended to the plant step under a name of its own: copra_plant_step_t first, then d_out, d_hist, nothing else -- in
    # memory the struct of ABI 10 grown at its end; copra_plant_step_t itself keeps the fields (and the size) callers of ABI 10 compiled against
    end = code.index("} copra_plant_step_ex_t;")
    body = code[code.rindex("typedef struct {", 0, end):end]
    assert re.findall(r"(\w+)\s*;", body) == ["step", "d_out", "d_hist"]
    assert re.search(r"copra_plant_step_t\s+step\s*;", body) and re.search(r"double\s*\*\s*d_out\s*;", body) and re.search(r"double\s*\*\s*d_hist\s*;", body)
    assert code.index("} copra_plant_step_t;") < end
    assert "src/PreviewSystem.cpp:16-55" in text


def test_library_exports_the_estimator_with_abi_11():
    lib = _lib()
    for name in NEW:
        assert hasattr(lib, name), name
    lib.copra_abi_version.restype = ctypes.c_int
    assert lib.copra_abi_version() >= 11
    from copra_amd import _capi
    vp = ctypes.c_void_p
    lib.copra_batch_set_bias_estimator.restype = ctypes.c_int
    lib.copra_batch_set_bias_estimator.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.copra_batch_set_bias.restype = ctypes.c_int
    lib.copra_batch_set_bias.argtypes = [vp, vp, ctypes.c_int]
    lib.copra_batch_bias_device.restype = vp
    lib.copra_batch_bias_device.argtypes = [vp]
    lib.copra_batch_get_bias.restype = ctypes.c_int
    lib.copra_batch_get_bias.argtypes = [vp, vp]
    one = np.ones(4)
    # (a NULL handle is refused before anything touches a device)
    assert lib.copra_batch_set_bias_estimator(None, one.ctypes.data, 0, 0, 0) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_set_bias_estimator(None, None, 0, 0, 0) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_set_bias(None, one.ctypes.data, 0) == _capi.COPRA_ERR_ARG
    assert lib.copra_batch_get_bias(None, one.ctypes.data) == _capi.COPRA_ERR_ARG
    assert not lib.copra_batch_bias_device(None)


def test_plant_step_ex_init_sets_the_new_size():
    """the mirror of copra_plant_step_ex_t is the mirror of copra_plant_step_t with d_out, d_hist last; its init sets the new size and zeroes
    everything else, copra_plant_step_init keeps setting the size of copra_plant_step_t"""
    from copra_amd import _capi
    lib = _lib()
    assert hasattr(lib, "copra_plant_step_ex_init")
    old = [n for n, _ in _capi.PlantStep._fields_]
    names = [n for n, _ in _capi.PlantStepEx._fields_]
    assert names == old + ["d_out", "d_hist"]
    assert _capi.PlantStepEx.d_out.offset == ctypes.sizeof(_capi.PlantStep)  # grown at its end: no padding in between
    for n in old:
        assert getattr(_capi.PlantStepEx, n).offset == getattr(_capi.PlantStep, n).offset, n
    st = _capi.PlantStepEx()
    ctypes.memset(ctypes.byref(st), 0xff, ctypes.sizeof(st))
    lib.copra_plant_step_ex_init.restype = None
    lib.copra_plant_step_ex_init.argtypes = [ctypes.POINTER(_capi.PlantStepEx)]
    lib.copra_plant_step_ex_init(ctypes.byref(st))
    assert st.struct_size == ctypes.sizeof(_capi.PlantStepEx) == ctypes.sizeof(_capi.PlantStep) + 2 * ctypes.sizeof(ctypes.c_void_p)
    assert not st.d_out and not st.d_hist and not any((st.A, st.B, st.d, st.w, st.fallback_u, st.x_out, st.u_out, st.status_out, st.age_out, st.age_hist))
    assert st.shared == 0 and st.solve_every == 0
    small = _capi.PlantStep()
    lib.copra_plant_step_init.restype = None
    lib.copra_plant_step_init.argtypes = [ctypes.POINTER(_capi.PlantStep)]
    lib.copra_plant_step_init(ctypes.byref(small))
    assert small.struct_size == ctypes.sizeof(_capi.PlantStep)


def test_python_binding_has_the_estimator():
    import inspect
    from copra_amd import BatchLMPC
    for name in ("set_bias_estimator", "set_bias", "bias", "bias_ptr"):
        assert callable(getattr(BatchLMPC, name, None)), name
    assert inspect.signature(BatchLMPC.advance).parameters["d_out"].default is None
    ro = inspect.signature(BatchLMPC.rollout).parameters
    assert ro["d_hist"].default is None and ro["d_out"].default is None


# ---- the kernel bodies on the host ----
VP, CI = ctypes.c_void_p, ctypes.c_int
STEP_ARGS = [CI] * 7 + [VP] * 13 + [CI, CI] + [VP] * 3 + [CI] * 3 + [VP] * 5 + [CI]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_plant_bias") / "libemu_plant_bias.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(EMU, "emu_plant_bias.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.emu_plant_bias_step.restype = CI
    lib.emu_plant_bias_step.argtypes = STEP_ARGS
    lib.emu_plant_bias_lds_doubles.restype = CI
    lib.emu_plant_bias_est_doubles.restype = CI
    lib.emu_plant_launch_group.restype = CI
    lib.emu_plant_launch_group.argtypes = [CI] * 5
    return lib


@pytest.fixture(scope="module")
def emu_backup(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_plant_backup_ref") / "libemu_plant_backup.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(EMU, "emu_plant_backup.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.emu_plant_backup_step.restype = CI
    lib.emu_plant_backup_step.argtypes = [CI] * 7 + [VP] * 13 + [CI, CI] + [VP] * 3
    lib.emu_plant_backup_lds_doubles.restype = CI
    return lib


@pytest.fixture(scope="module")
def emu_abi9(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_plant_ref") / "libemu_plant.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(EMU, "emu_plant.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.emu_plant_step.restype = CI
    lib.emu_plant_step.argtypes = [CI] * 7 + [VP] * 13
    lib.emu_plant_lds_doubles.restype = CI
    return lib


def launch_group(emu, nx, nu, dense):
    """the group copra_hip_plant.hip launches with: plant_group(bias_image_bytes(nx, nu, dense)) of plant_step.hpp, asked of the emulator"""
    return emu.emu_plant_launch_group(1, nx, nu, 0, int(dense))


def _model(rng, batch, nx, nu, N=5, failed=0):
    """a controller's model, a state, the last solve's results (`failed` instances without a solution) and a fallback control"""
    status = np.zeros(batch, dtype=np.int32)
    bad = rng.choice(batch, failed, replace=False) if failed else np.zeros(0, dtype=int)
    status[bad] = rng.integers(1, 4, bad.size)
    control = rng.standard_normal((batch, nu * N))
    control[bad] = np.nan  # what the engine leaves in a failed instance
    return dict(Am=0.5 * rng.standard_normal((batch, nx, nx)), Bm=rng.standard_normal((batch, nx, nu)), dhat=rng.standard_normal((batch, nx)),
                x=rng.standard_normal((batch, nx)) * 10.0 ** rng.integers(-2, 2, (batch, 1)), w=0.01 * rng.standard_normal((batch, nx)),
                status=status, control=control, fb=rng.standard_normal((batch, nu)), N=N)


def _gain(rng, batch, nx, dense, per):
    lead = (batch,) if per else ()
    return rng.uniform(-1.0, 1.0, lead + ((nx, nx) if dense else (nx,)))


def _plant(rng, c, kind):
    """'own': a plant per instance, 'shared': one for the batch, 'none': the model with its estimates.  (A, B, d in natural indexing) or None"""
    batch, nx = c["x"].shape
    nu = c["fb"].shape[1]
    if kind == "none":
        return None
    lead = (batch,) if kind == "own" else ()
    return 0.5 * rng.standard_normal(lead + (nx, nx)), rng.standard_normal(lead + (nx, nu)), rng.standard_normal(lead + (nx,))


def _tick(emu, c, plant, gain, dense, per, with_w, with_fb, group, threads=256, vec2_mode=-1, backup=None):
    """one tick with the estimator on, in place; returns dict(x, dhat, x_out, u_out, d_out, s_out, a_out, vec2).  backup: (K, fresh, plan, next)"""
    batch, nx = c["x"].shape
    nu = c["fb"].shape[1]
    cm = lambda a: np.ascontiguousarray(np.swapaxes(a, -1, -2))  # noqa: E731  (the ABI's column-major blocks)
    Am, Bm = cm(c["Am"]), cm(c["Bm"])
    A, B, d, shared = None, None, None, 0
    if plant is not None:
        A, B, d = cm(plant[0]), cm(plant[1]), np.ascontiguousarray(plant[2])
        shared = int(plant[0].ndim == 2)
    G = abi_gain(gain, dense)
    x, dhat = c["x"].copy(), c["dhat"].copy()
    GUARD = -3.5
    d_out = np.full(batch * nx + 4, GUARD)
    dh_buf = np.full(batch * nx + 4, GUARD)
    dh_buf[:batch * nx] = dhat.ravel()
    x_out, u_out = np.full((batch, nx), np.nan), np.full((batch, nu), 7.0)
    s_out, a_out = np.full(batch, -1, dtype=np.int32), np.full(batch, -99, dtype=np.int32)
    vec2 = ctypes.c_int(-1)
    K, fresh, plan, nxt = backup if backup else (0, 1, None, None)
    rc = emu.emu_plant_bias_step(batch, nx, nu, c["N"], group, threads, shared, _ptr(A), _ptr(B), _ptr(d), _ptr(x), _ptr(c["w"] if with_w else None),
                                 _ptr(c["fb"] if with_fb else None), _ptr(c["status"]), _ptr(c["control"]), _ptr(x), _ptr(x_out), _ptr(u_out), _ptr(s_out),
                                 ctypes.addressof(vec2), K, fresh, _ptr(plan), _ptr(nxt), _ptr(a_out), 1, int(dense), int(not per), _ptr(Am), _ptr(Bm),
                                 _ptr(G), _ptr(dh_buf), _ptr(d_out), vec2_mode)
    assert rc == 0
    assert (d_out[batch * nx:] == GUARD).all() and (dh_buf[batch * nx:] == GUARD).all()
    return dict(x=x, dhat=dh_buf[:batch * nx].reshape(batch, nx).copy(), x_out=x_out, u_out=u_out, d_out=d_out[:batch * nx].reshape(batch, nx).copy(),
                s_out=s_out, a_out=a_out, vec2=vec2.value)


def _expect(c, plant, u, with_w, gain, dense):
    """(x+ exact, Sx, dhat+ exact, its bound) of one tick for the applied controls u"""
    if plant is None:
        plant = (c["Am"], c["Bm"], c["dhat"])
    ref, Sx = reference_step(plant[0], plant[1], plant[2], c["x"], u, c["w"] if with_w else None)
    dref, dbound = reference_bias(c["Am"], c["Bm"], c["dhat"], c["x"], u, ref, Sx, gain, dense)
    return ref, Sx, dref, dbound


def _check(got, c, ref, Sx, dref, dbound, moved, what):
    nx, nu = c["x"].shape[1], c["fb"].shape[1]
    assert not np.isnan(got["x"]).any() and not np.isnan(got["dhat"]).any(), what
    err = np.abs(got["x"][moved].astype(LD) - ref[moved])
    assert (err <= step_bound(nx, nu, Sx[moved])).all(), (what, float((err / step_bound(nx, nu, Sx[moved])).max()))
    derr = np.abs(got["dhat"][moved].astype(LD) - dref[moved])
    assert (derr <= dbound[moved]).all(), (what, float((derr / dbound[moved]).max()))
    assert _same_bits(got["x"][~moved], c["x"][~moved]), what  # held, bit for bit: the state ...
    assert _same_bits(got["dhat"][~moved], c["dhat"][~moved]), what  # ... and the estimate
    assert _same_bits(got["d_out"], got["dhat"]) and _same_bits(got["x_out"], got["x"]), what
    return float((derr / dbound[moved]).max()) if moved.any() else 0.0


@pytest.mark.parametrize("nx,nu", [(2, 1), (6, 3), (9, 3), (16, 4)])
def test_the_rule_on_the_kernel_bodies(emu, nx, nu):
    """item 1: x+ and dhat+ against the longdouble statement, within step_bound and bias_bound (derived above)"""
    runs, seen_vec2, worst = 0, set(), 0.0
    for batch in (1, 5, 37):
        rng = np.random.default_rng(1000 * nx + 10 * nu + batch)
        c = _model(rng, batch, nx, nu, failed=batch // 5)
        ok = c["status"] == 0
        u = np.where(ok[:, None], c["control"][:, :nu], c["fb"])
        for dense, per, kind in itertools.product((0, 1), (0, 1), ("own", "shared", "none")):
            gain, plant = _gain(rng, batch, nx, dense, per), _plant(rng, c, kind)
            for with_w in (False, True):
                ref, Sx, dref, dbound = _expect(c, plant, u, with_w, gain, dense)
                for group, vec2_mode in itertools.product(sorted({1, 4, launch_group(emu, nx, nu, dense)}), (-1, 0)):
                    what = (nx, nu, batch, dense, per, kind, with_w, group, vec2_mode)
                    got = _tick(emu, c, plant, gain, dense, per, with_w, True, group, vec2_mode=vec2_mode)
                    worst = max(worst, _check(got, c, ref, Sx, dref, dbound, np.ones(batch, dtype=bool), what))
                    assert _same_bits(got["u_out"], u) and np.array_equal(got["s_out"], c["status"]), what
                    assert got["vec2"] == (1 if vec2_mode == -1 and group % 2 == 0 else 0), what
                    seen_vec2.add(got["vec2"])
                    runs += 1
    print("nx %d nu %d: %d runs, max dhat err / bound = %.3f" % (nx, nu, runs, worst))
    assert seen_vec2 == {0, 1} and runs >= 3 * 12 * 2 * 2 * 2


def test_the_launch_group_leaves_a_partial_last_group(emu):
    """the cases above end in a partial last group at the launch's own group size, and that size is even"""
    for (nx, nu), dense in itertools.product([(2, 1), (6, 3), (9, 3), (16, 4)], (0, 1)):
        g = launch_group(emu, nx, nu, dense)
        assert g >= 2 and g % 2 == 0 and 37 % g != 0, (nx, nu, dense, g)


def test_held_instances_keep_state_and_estimate(emu):
    """item 2: no fallback -- a failed instance keeps x and dhat bit for bit, d_out is the old estimate, u_out NaN"""
    nx, nu, batch = 6, 3, 37
    rng = np.random.default_rng(7)
    c = _model(rng, batch, nx, nu, failed=9)
    ok = c["status"] == 0
    assert 0 < (~ok).sum() < batch
    u = np.where(ok[:, None], c["control"][:, :nu], 0.0)
    for dense, per, kind, group in itertools.product((0, 1), (0, 1), ("own", "none"), (1, 4, 16)):
        gain, plant = _gain(rng, batch, nx, dense, per), _plant(rng, c, kind)
        ref, Sx, dref, dbound = _expect(c, plant, u, True, gain, dense)
        got = _tick(emu, c, plant, gain, dense, per, True, False, group)
        _check(got, c, ref, Sx, dref, dbound, ok, (dense, per, kind, group))
        assert _same_bits(got["d_out"][~ok], c["dhat"][~ok])
        assert np.isnan(got["u_out"][~ok]).all() and _same_bits(got["u_out"][ok], c["control"][ok, :nu])
        assert (got["a_out"][ok] == 0).all() and (got["a_out"][~ok] == HELD).all()


def _play(emu, nx, nu, N, K, group, threads, dense, per, kind, with_w, with_fb, seed):
    """the five-tick script of tests/test_backup_plan_abi.py with the estimator on: the ages, and the estimate against the rule with the
    control the tick APPLIED (fresh, plan step, fallback) or kept (held)"""
    s = _script(nx, nu, N, 0, seed)
    rng = np.random.default_rng(seed + 1)
    gain = _gain(rng, BATCH, nx, dense, per)
    c = dict(Am=s["A"], Bm=s["B"], dhat=s["d"].copy(), x=s["x0"].copy(), fb=s["fb"], N=N)
    plant = _plant(rng, c, kind)
    plan_buf = np.full(BATCH * K * nu, np.nan)
    next_buf = np.zeros(BATCH, dtype=np.int32)
    want_plan, want_next = plan_buf.reshape(BATCH, K, nu).copy(), next_buf.copy()
    ages, moved_d = [], np.zeros(BATCH, dtype=bool)
    for t in range(len(FRESH)):
        u, age, want_plan, want_next = _rule(s, t, K, nu, with_fb, want_plan, want_next)
        moved = age != HELD
        c["w"], c["status"], c["control"] = s["w"][t], s["status"][t], s["control"][t]
        ref, Sx, dref, dbound = _expect(c, plant, np.where(moved[:, None], u, 0.0), with_w, gain, dense)
        got = _tick(emu, c, plant, gain, dense, per, with_w, with_fb, group, threads, backup=(K, FRESH[t], plan_buf, next_buf))
        what = (K, group, threads, dense, per, kind, with_w, with_fb, t)
        assert np.array_equal(got["a_out"], age), what
        assert _same_bits(got["u_out"], u), what
        assert _same_bits(plan_buf.reshape(BATCH, K, nu), want_plan) and np.array_equal(next_buf, want_next), what
        _check(got, c, ref, Sx, dref, dbound, moved, what)
        moved_d |= (got["dhat"] != c["dhat"]).any(axis=1)
        c["x"], c["dhat"] = got["x"], got["dhat"]
        ages.append(age)
    return np.stack(ages), moved_d


def test_backup_plan_and_fallback_ticks_move_the_estimate(emu):
    """item 3: (6, 3), K = 3: ages 0, 1 .. K, -1 and -2 all occur; the estimate follows the applied control on every one of them but -2"""
    nx, nu, N, K = 6, 3, 4, 3
    for dense, per, kind, with_w in itertools.product((0, 1), (0, 1), ("own", "none"), (False, True)):
        for group, threads in ((1, 64), (4, 3), (4, 64)):
            seen = set()
            for with_fb in (False, True):
                ages, moved_d = _play(emu, nx, nu, N, K, group, threads, dense, per, kind, with_w, with_fb, seed=11 + 2 * dense + per)
                assert set(ages.ravel().tolist()) == set(range(0, K + 1)) | {FALLBACK if with_fb else HELD}
                seen |= set(ages.ravel().tolist())
                if kind == "own":  # (instance 1 never solves: without a fallback its estimate never moves, with one it does)
                    assert moved_d[1] == with_fb and moved_d[[0, 2, 3, 4]].all()
            assert seen == set(range(-2, K + 1))


@pytest.mark.parametrize("nx,nu", [(2, 1), (6, 3), (16, 4)])
def test_estimator_off_is_the_tick_of_abi_10(emu, emu_abi9, emu_backup, nx, nu):
    """item 4: est = 0 through the new harness gives the bits of emu_plant.cpp / emu_plant_backup.cpp, and plant_lds(...).total is theirs"""
    batch = 77
    for shared, with_w, with_fb in itertools.product((False, True), (False, True), (False, True)):
        c = _case(nx, nu, batch, shared, seed=1000 * nx + nu + 7 * shared)
        A = np.ascontiguousarray(np.swapaxes(c["A"], -1, -2))
        B = np.ascontiguousarray(np.swapaxes(c["B"], -1, -2))
        for in_place, group in itertools.product((False, True), (1, 6, 32)):
            want = _run(emu_abi9, c, nx, nu, shared, with_w, with_fb, in_place, group)
            x0 = c["x0"].copy()
            nxt = x0 if in_place else np.full((batch, nx), np.nan)
            x_out, u_out = np.full((batch, nx), np.nan), np.full((batch, nu), 7.0)
            s_out, a_out = np.full(batch, -1, dtype=np.int32), np.full(batch, -99, dtype=np.int32)
            vec2 = ctypes.c_int(-1)
            rc = emu.emu_plant_bias_step(batch, nx, nu, c["N"], group, 256, int(shared), _ptr(A), _ptr(B), _ptr(c["d"]), _ptr(x0),
                                         _ptr(c["w"] if with_w else None), _ptr(c["fb"] if with_fb else None), _ptr(c["status"]), _ptr(c["control"]),
                                         _ptr(nxt), _ptr(x_out), _ptr(u_out), _ptr(s_out), ctypes.addressof(vec2), 0, 1, None, None, _ptr(a_out),
                                         0, 0, 0, None, None, None, None, None, -1)
            assert rc == 0
            for got, ref in zip((nxt, x_out, u_out, s_out), want[:4]):
                assert _same_bits(got, ref), (shared, with_w, with_fb, in_place, group)
            assert vec2.value == want[4]
    for group, shared, has_w in itertools.product((1, 6, 32), (0, 1), (0, 1)):
        assert emu.emu_plant_bias_lds_doubles(nx, nu, group, shared, has_w, 0) == emu_abi9.emu_plant_lds_doubles(nx, nu, group, shared, has_w)
        for backup in (0, 1):
            assert emu.emu_plant_bias_lds_doubles(nx, nu, group, shared, has_w, backup) == emu_backup.emu_plant_backup_lds_doubles(nx, nu, group, shared, has_w, backup)
            assert emu.emu_plant_bias_est_doubles(nx, nu, group, 0, has_w, backup, 1, 0, 1) > emu.emu_plant_bias_lds_doubles(nx, nu, group, 0, has_w, backup)


def test_estimator_off_plays_the_backup_script_bit_for_bit(emu, emu_backup):
    """item 4, with backup plans: the five-tick script at (6, 3), K = 3 through both harnesses on separate plan / next arrays"""
    nx, nu, N, K = 6, 3, 4, 3
    for shared, with_w, with_fb, group in itertools.product((0, 1), (False, True), (False, True), (1, 4)):
        s = _script(nx, nu, N, shared, seed=3 + shared)
        A = np.ascontiguousarray(np.swapaxes(s["A"], -1, -2))
        B = np.ascontiguousarray(np.swapaxes(s["B"], -1, -2))
        state = []
        for _ in range(2):
            state.append(dict(x=s["x0"].copy(), plan=np.full(BATCH * K * nu, np.nan), nxt=np.zeros(BATCH, dtype=np.int32)))
        for t in range(len(FRESH)):
            outs = []
            for which, st in enumerate(state):
                x_out, u_out = np.full((BATCH, nx), np.nan), np.full((BATCH, nu), 7.0)
                s_out, a_out = np.full(BATCH, -1, dtype=np.int32), np.full(BATCH, -99, dtype=np.int32)
                args = [BATCH, nx, nu, N, group, 64, shared, _ptr(A), _ptr(B), _ptr(s["d"]), _ptr(st["x"]), _ptr(s["w"][t] if with_w else None),
                        _ptr(s["fb"] if with_fb else None), _ptr(s["status"][t]), _ptr(s["control"][t]), _ptr(st["x"]), _ptr(x_out), _ptr(u_out), _ptr(s_out),
                        None, K, FRESH[t], _ptr(st["plan"]), _ptr(st["nxt"]), _ptr(a_out)]
                if which == 0:
                    assert emu_backup.emu_plant_backup_step(*args) == 0
                else:
                    assert emu.emu_plant_bias_step(*(args + [0, 0, 0, None, None, None, None, None, -1])) == 0
                outs.append((st["x"].copy(), x_out, u_out, s_out, a_out, st["plan"].copy(), st["nxt"].copy()))
            for a, b in zip(*outs):
                assert _same_bits(a, b), (shared, with_w, with_fb, group, t)


@pytest.mark.parametrize("nx,nu", [(2, 1), (6, 3), (16, 4)])
def test_deadbeat_after_one_tick(emu, nx, nu):
    """item 5: L = I, plant = model with d + c, no w: dhat+ = d + c exactly in exact arithmetic, within bias_bound as computed"""
    batch = 37
    rng = np.random.default_rng(50 + nx)
    c = _model(rng, batch, nx, nu)
    off = rng.standard_normal((batch, nx))
    plant = (c["Am"], c["Bm"], c["dhat"] + off)
    u = c["control"][:, :nu]
    target = plant[2].astype(LD)  # the plant's d as stored: dhat + (dp - dhat)
    for dense, gain in ((0, np.ones(nx)), (1, np.eye(nx))):
        ref, Sx, dref, dbound = _expect(c, plant, u, False, gain, dense)
        assert (np.abs(dref - target) <= 64 * np.finfo(LD).eps * (Sx + np.abs(dref))).all()  # (the statement itself is deadbeat)
        for group in (1, 4, launch_group(emu, nx, nu, dense)):
            got = _tick(emu, c, plant, gain, dense, 0, False, False, group)
            derr = np.abs(got["dhat"].astype(LD) - target)
            assert (derr <= dbound).all(), (dense, group, float((derr / dbound).max()))


# ---- memory errors on the host ----
def test_kernel_bodies_under_the_address_and_ub_sanitizers(tmp_path):
    """item 6: tests/emu/emu_plant_bias_main.cpp -- the backup script at (6, 3, 4), K = 3, batch 5, group 4 with the estimator on, plus a dense
    per-instance case at (9, 3), batch 7 -- as a stand-alone program built with -fsanitize=address,undefined; every array has exactly the
    elements the kernel may touch.  Exit status 0 and an empty stderr."""
    exe = str(tmp_path / "emu_plant_bias_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(EMU, "emu_plant_bias.cpp"), os.path.join(EMU, "emu_plant_bias_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "", r.stderr
