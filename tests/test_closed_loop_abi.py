"""The receding-horizon tick at the C ABI (copra_batch_advance / copra_batch_rollout, ABI 7) without a GPU: declared, exported, bound -- and
the arithmetic of the plant-step kernel (copra_amd/csrc/plant_step.hpp), whose two phases compile on the host: tests/emu/emu_plant.cpp walks
them thread by thread, this file compiles that harness itself.

The bound on a new state is derived, not measured: x+ is a sum of nx + nu + 2 terms (nx products with A, nu with B, d, w).  Whatever the order
of the sum and whether or not products are fused, every partial sum is bounded by S = |A||x0| + |B||u| + |d| + |w|, each of the at most
nx + nu + 1 additions and nx + nu products adds a relative error of at most 2^-53, so |x+ - exact| <= (nx + nu + 2) 2^-52 S entry-wise with room to
spare; the reference sum is evaluated in numpy.longdouble."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("copra_plant_step_init", "copra_batch_advance", "copra_batch_rollout", "copra_batch_x0_device", "copra_batch_get_x0")
SHAPES = [(2, 1), (6, 3), (9, 3), (12, 6), (16, 4)]


def _lib():
    from copra_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ctypes.CDLL(_capi.LIB_PATH)


def test_header_declares_the_tick():
    text = open(os.path.join(ROOT, "include", "copra_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
    end = code.index("} copra_plant_step_t;")
    body = code[code.rindex("typedef struct {", 0, end):end]
    for field in ("struct_size", "d", "shared", "w", "fallback_u", "x_out", "u_out", "status_out"):
        assert re.search(r"\b%s;" % field, body), field
    assert "include/PreviewSystem.h:52" in text and "include/LMPC.h:108" in text


def test_library_exports_the_tick_with_abi_7():
    lib = _lib()
    for name in NEW:
        assert hasattr(lib, name), name
    lib.copra_abi_version.restype = ctypes.c_int
    assert lib.copra_abi_version() >= 7


def test_plant_step_init_fills_the_size_of_the_mirror():
    from copra_amd import _capi
    lib = _lib()
    st = _capi.PlantStep()
    ctypes.memset(ctypes.byref(st), 0xff, ctypes.sizeof(st))
    lib.copra_plant_step_init.restype = None
    lib.copra_plant_step_init.argtypes = [ctypes.POINTER(_capi.PlantStep)]
    lib.copra_plant_step_init(ctypes.byref(st))
    assert st.struct_size == ctypes.sizeof(_capi.PlantStep)
    assert not any((st.A, st.B, st.d, st.w, st.fallback_u, st.x_out, st.u_out, st.status_out)) and st.shared == 0


def test_python_binding_has_the_tick():
    from copra_amd import BatchLMPC
    for name in ("advance", "rollout", "state", "state_ptr"):
        assert callable(getattr(BatchLMPC, name, None)), name


# ---- the kernel's arithmetic ----
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_plant") / "libemu_plant.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "emu", "emu_plant.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.emu_plant_step.restype = ctypes.c_int
    lib.emu_plant_step.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 13
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data


def _case(nx, nu, batch, shared, seed, N=5):
    rng = np.random.default_rng(seed)
    lead = () if shared else (batch,)
    A = rng.standard_normal(lead + (nx, nx))
    B = rng.standard_normal(lead + (nx, nu))
    d = rng.standard_normal(lead + (nx,))
    x0 = rng.standard_normal((batch, nx)) * 10.0 ** rng.integers(-3, 3, (batch, 1))
    w = 0.01 * rng.standard_normal((batch, nx))
    status = np.zeros(batch, dtype=np.int32)
    failed = rng.choice(batch, max(2, batch // 7), replace=False)
    status[failed] = rng.integers(1, 4, failed.size)  # (infeasible / not positive definite / iteration cap)
    control = rng.standard_normal((batch, nu * N))
    control[failed] = np.nan  # what the engine leaves in a failed instance
    fb = rng.standard_normal((batch, nu))
    return dict(A=A, B=B, d=d, x0=x0, w=w, status=status, control=control, fb=fb, N=N, failed=failed)


def _run(emu, c, nx, nu, shared, with_w, with_fb, in_place, group, threads=256):
    batch = c["x0"].shape[0]
    A = np.ascontiguousarray(np.swapaxes(c["A"], -1, -2))  # the ABI's column-major blocks
    B = np.ascontiguousarray(np.swapaxes(c["B"], -1, -2))
    x0 = c["x0"].copy()
    nxt = x0 if in_place else np.full((batch, nx), np.nan)
    x_out, u_out, s_out = np.full((batch, nx), np.nan), np.full((batch, nu), 7.0), np.full(batch, -1, dtype=np.int32)
    vec2 = ctypes.c_int(-1)
    rc = emu.emu_plant_step(batch, nx, nu, c["N"], group, threads, int(shared), _ptr(A), _ptr(B), _ptr(c["d"]), _ptr(x0), _ptr(c["w"] if with_w else None),
                            _ptr(c["fb"] if with_fb else None), _ptr(c["status"]), _ptr(c["control"]), _ptr(nxt), _ptr(x_out), _ptr(u_out), _ptr(s_out),
                            ctypes.addressof(vec2))
    assert rc == 0
    if not in_place:
        assert np.array_equal(x0, c["x0"])  # (the old state is only read)
    return nxt, x_out, u_out, s_out, vec2.value


def reference_step(A, B, d, x0, u, w):
    """x+ and the bound's scale S in numpy.longdouble; A (b, nx, nx) or (nx, nx) in natural indexing"""
    L = np.longdouble
    A, B, d, x0, u = (np.asarray(v, dtype=L) for v in (A, B, d, x0, u))
    w = np.zeros_like(x0) if w is None else np.asarray(w, dtype=L)
    if A.ndim == 2:
        A, B, d = (np.broadcast_to(v, (x0.shape[0],) + v.shape) for v in (A, B, d))
    ref = (A * x0[:, None, :]).sum(axis=2) + (B * u[:, None, :]).sum(axis=2) + d + w
    S = (np.abs(A) * np.abs(x0)[:, None, :]).sum(axis=2) + (np.abs(B) * np.abs(u)[:, None, :]).sum(axis=2) + np.abs(d) + np.abs(w)
    return ref, S


def step_bound(nx, nu, S):
    return (nx + nu + 2) * 2.0 ** -52 * S


@pytest.mark.parametrize("nx,nu", SHAPES)
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("with_w", [False, True])
@pytest.mark.parametrize("with_fb", [False, True])
def test_plant_step_arithmetic(emu, nx, nu, shared, with_w, with_fb):
    batch = 77  # (not a multiple of any group: the last workgroup is partial)
    c = _case(nx, nu, batch, shared, seed=1000 * nx + nu + 7 * shared)
    ok = c["status"] == 0
    u_used = np.where(ok[:, None], c["control"][:, :nu], c["fb"] if with_fb else 0.0)
    ref, S = reference_step(c["A"], c["B"], c["d"], c["x0"], u_used, c["w"] if with_w else None)
    moved = ok | with_fb
    seen_vec2 = set()
    for in_place in (False, True):
        for group in (1, 6, 32):
            nxt, x_out, u_out, s_out, vec2 = _run(emu, c, nx, nu, shared, with_w, with_fb, in_place, group)
            seen_vec2.add(vec2)
            assert not np.isnan(nxt).any()  # no NaN of a failed instance's control reaches a state
            err = np.abs(nxt[moved].astype(np.longdouble) - ref[moved])
            bound = step_bound(nx, nu, S[moved])
            print("nx %d nu %d shared %d w %d fallback %d in place %d group %d: max err / bound = %.3f" %
                  (nx, nu, shared, with_w, with_fb, in_place, group, float((err / bound).max())))
            assert (err <= bound).all()
            assert np.array_equal(nxt[~moved], c["x0"][~moved])  # held, bit for bit
            assert (~moved).sum() == (0 if with_fb else c["failed"].size)
            assert np.array_equal(x_out, nxt) and np.array_equal(s_out, c["status"])
            assert np.array_equal(u_out[ok], c["control"][ok, :nu])
            if with_fb:
                assert np.array_equal(u_out[~ok], c["fb"][~ok])
            else:
                assert np.isnan(u_out[~ok]).all()
    assert seen_vec2 == {0, 1}  # (both forms of the copy were walked: an odd group copies double by double)


def test_plant_step_reads_only_the_first_controls(emu):
    """control is read with stride nu N and only its first nu entries: NaN everywhere else changes nothing"""
    nx, nu = 6, 3
    c = _case(nx, nu, 40, False, seed=5)
    a = _run(emu, c, nx, nu, False, True, False, False, 32)
    c2 = dict(c, control=c["control"].copy())
    c2["control"][:, nu:] = np.nan
    b = _run(emu, c2, nx, nu, False, True, False, False, 32)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2], equal_nan=True)
