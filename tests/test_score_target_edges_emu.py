"""The cases of tests/launch_edge_cases.py on the kernels' own bodies on the host (tests/emu/emu_score.cpp, emu_target.cpp), AT THE LAUNCH'S
OWN GROUP AND THREAD COUNT, over the NaN-filled image with the guard behind it: here the answer is bit for bit -- the records equal
tests/score_ref.py, z and the references equal target_ref.gepp / rows.  tests/test_score_target_edges_gpu.py runs the same cases on the
device within the derived bounds: a case that passes here and fails there is a fault of the device side (divergent LDS addressing, the
dynamic-LDS opt-in, the grid arithmetic of launch_*, a contraction), not of the arithmetic.

The states, controls and ages a device rollout would give are replaced by launch_edge_cases.synthetic_history (the scenario's own model
under random controls, its two held instances held).  Every test asserts the property it is named for from the emulators' geometry
exports; the tables in the docstrings are the values at HEAD."""
import numpy as np
import pytest

import launch_edge_cases as lec
import score_ref
from test_score_abi import _same_bits, ref_update
from test_score_abi import run as score_run
from test_target_abi import check as target_check
from test_target_abi import run as target_run
from test_tick_edges_gpu import mixed


@pytest.fixture(scope="module")
def geo(tmp_path_factory):
    return lec.build_emulators(tmp_path_factory.mktemp("emu_edges"))


# ---- the score ----
def _score(geo, case, m=None, S=None):
    """the case's ticks on the emulator at the launch's group against score_ref, bit for bit; returns (records, geometry, pairs copied per tick)"""
    what = case["id"]
    n = lec.largest_nx(case["nx"], lec.score_property(geo, case), what)
    if S is None:
        S, m0 = lec.score_case(case, n)
        m = m0 if m is None else m
    G = lec.score_geometry(geo, m)
    hist = lec.synthetic_history(S, case["ticks"])
    mixed(hist["status_hist"])
    c = dict(m, batch=S["batch"], ticks=[(hist["x_hist"][t + 1], hist["u_hist"][t], hist["age_hist"][t]) for t in range(case["ticks"])])
    room, want = score_ref.zero_records(S["batch"] + 32), score_ref.zero_records(S["batch"])
    got = room[:S["batch"]]  # (a group of records behind the batch: a store that runs to `group` instead of the last group's count lands there)
    wide = []
    for t in range(case["ticks"]):
        lds, used = score_run(geo.score, c, got, t, t + 1, G["group"], threads=geo.score.emu_score_threads(), tol=m["tol"], drop=m["leave"])
        assert 8 * lds == G["bytes"], what  # (the image walked is the image the launch asks for)
        wide.append(used)
        ref_update(c, want, t, t + 1, tol=m["tol"], drop=m["leave"])
    got = got.copy()
    assert _same_bits(got, want), (what, [f for f in got.dtype.names if not _same_bits(got[f], want[f])])
    assert room[S["batch"]:].tobytes() == score_ref.zero_records(32).tobytes(), what
    assert (got["ticks"] == case["ticks"]).all() and (got["held"][list(S["held"])] == case["ticks"]).all()
    print("%s: nx %d, group %d, image %d bytes, %d workgroups" % (what, n, G["group"], G["bytes"], -(-S["batch"] // G["group"])))
    return got, G, wide


def _not_vacuous(got, m, what):
    """where the measure gives a field a source, the field moved"""
    g = lec.given(m)
    if g["qx"] is not None:
        assert (got["jx"] != 0).any(), what
    if any(g[k] is not None for k in lec.LIMITS):
        assert (got["violating"] > 0).any() and (got["viol_max"] > 0).any(), what


@pytest.mark.parametrize("case", lec.S1 + lec.S2 + lec.S3, ids=lambda c: c["id"])
def test_score_groups_and_big_images(geo, case):
    """S1 group 1 (every copy the scalar loop); S2 the launch's image above 48 KiB; S3 groups 4, 10 and 16 with more than one workgroup
    and a partial last one"""
    keeps = lec.score_property(geo, case)
    n = lec.largest_nx(case["nx"], keeps, case["id"])
    assert keeps(n)
    got, G, _ = _score(geo, case)
    _not_vacuous(got, lec.score_case(case, n)[1], case["id"])


@pytest.mark.parametrize("case", lec.S4, ids=lambda c: c["id"])
def test_a_shared_reference_of_odd_rows(geo, case):
    """batch nx is odd and so is nx: the rows of the shared 3-step signal start on 16 bytes only every other row; the same signal tiled per
    instance (the gather) gives the same bits"""
    S, m = lec.score_case(case)
    rows = lec.reference_rows(m, case["ticks"])
    assert (case["batch"] * case["nx"]) % 2 == 1 and {(r * case["nx"]) % 2 for r in rows} == {0, 1}
    got, _, wide = _score(geo, case, m, S)
    _not_vacuous(got, m, case["id"])
    assert all(not w for w, r in zip(wide, rows) if (r * case["nx"]) % 2)  # (an odd row: no pairs)
    per, _, _ = _score(geo, dict(case, per=True), lec.tiled(m, case["batch"]), S)
    assert _same_bits(got, per)


@pytest.mark.parametrize("case", lec.S5, ids=lambda c: c["id"])
def test_an_image_with_parts_absent(geo, case):
    """qx alone; the control box alone; dense qx and x_ref without limits: the fields that have no source stay 0"""
    S, m = lec.score_case(case)
    full = lec.score_geometry(geo, dict(m, leave=()))
    got, G, _ = _score(geo, case, m, S)
    assert G["bytes"] < full["bytes"]
    _not_vacuous(got, m, case["id"])
    g = lec.given(m)
    if g["qx"] is None:
        assert (got["jx"] == 0).all()
    if g["ru"] is None:
        assert (got["ju"] == 0).all()
    if all(g[k] is None for k in lec.LIMITS):
        assert all((got[f] == 0).all() for f in ("viol_sum", "viol_max", "violating", "first_violation"))
    if g["qx"] is None and g["ru"] is None:
        assert (got["peak"] == 0).all()


def test_the_first_dense_measure_that_does_not_fit(geo):
    """S6 on the host: the geometry's own limit -- the dense image of the first nx beyond it (141 at HEAD) is refused by the setter's rule,
    the diagonal one of the same nx fits, and one tick of it scores"""
    top = geo.target.emu_target_lds_max()
    bad = lec.first_beyond(geo, 1, 1, top)
    assert geo.score.emu_score_image_bytes(bad, 1, 0) <= top
    case = lec._s("S6 diagonal at nx %d" % bad, bad, 1, 5, 1, 1, False, False)
    got, G, _ = _score(geo, case)
    assert G["group"] >= 1 and (got["jx"] != 0).all()
    print("S6: dense nx %d is the first that does not fit (%d > %d bytes)" % (bad, geo.score.emu_score_image_bytes(bad, 1, 1), top))


# ---- the targets ----
def _target(geo, c, what, **kw):
    """the case on the emulator at the launch's group and thread count: test_target_abi.check (status the rule's, z and the references the
    bits of the restatement, singular instances untouched); returns (geometry, what the run reports)"""
    G = lec.target_geometry(geo, c)
    lec.target_preconditions(c, what)
    tau = c["offset"]  # (tick 0: the block is min(offset, steps - 1))
    z, status, outs, info = target_run(geo.target, c, tau=tau, group=G["group"], threads=geo.target.emu_target_threads(), **kw)
    target_check(c, tau, z, status, outs, must_be_singular=c["planted"])
    assert status.sum() == len(c["planted"])
    print("%s: group %d, one wave's image %d bytes, the launch's %d, %d workgroups" % (what, G["group"], G["bytes"], 8 * info["lds"], -(-c["batch"] // G["group"])))
    return G, info, (z, status, outs)


@pytest.mark.parametrize("case", lec.T1, ids=lambda c: c["id"])
def test_target_groups_with_lanes_that_disagree(geo, case):
    """groups 256, 128, 128 (odd n) and 64: two full workgroups and a partial one; singular instances at index 2, at index == group and at
    batch - 1; the lanes of a wave pick different pivot rows (target_preconditions)"""
    c = lec.target_of(case)
    G = lec.target_geometry(geo, c)
    assert c["batch"] == 2 * G["group"] + 1
    lec.plant(c, G["group"])
    _target(geo, c, case["id"])


@pytest.mark.parametrize("case", lec.T2, ids=lambda c: c["id"])
def test_the_largest_target_image_that_fits(geo, case):
    """n = 17: the largest image the setter accepts; n = 16: z leaves in pairs"""
    c = lec.target_of(case)
    G, info, _ = _target(geo, c, case["id"])
    n = c["nx"] + c["nu"]
    assert lec.KIB48 < G["bytes"] <= G["top"] and G["group"] == 64 and 8 * info["lds"] == G["bytes"]
    assert bool(info["vec2"] & 2) == (n % 2 == 0)
    if n % 2:  # the largest: one more state does not fit
        assert geo.target.emu_target_image_bytes(c["nx"] + 1, c["nu"], 0) > G["top"]


def test_eight_driven_costs_above_48_kib(geo):
    """T3: S_c = 1, N and N + 1, odd and even r_c S_c, the maps pushing the image of (6, 3) above 48 KiB; every block of a cost equal"""
    c, shapes = lec.eight_cost_case(geo)
    G, info, (z, status, outs) = _target(geo, c, "T3 eight costs")
    assert G["bytes"] > lec.KIB48 and len(shapes) == 8 and {s for _, s in shapes} == {1, c["N"], c["N"] + 1}
    assert {(r * s) % 2 for r, s in shapes} == {0, 1}
    for k, (r, s) in enumerate(shapes):
        assert bool(info["vec2"] >> (2 + k) & 1) == ((r * s) % 2 == 0), k
        blocks = outs[k].reshape(c["batch"], s, r)
        assert all(_same_bits(np.ascontiguousarray(blocks[:, j]), np.ascontiguousarray(blocks[:, 0])) for j in range(s))


@pytest.mark.parametrize("case", lec.T4, ids=lambda c: c["id"])
def test_target_inputs_off_16_bytes(geo, case):
    """A, B, d one double past a 16-byte boundary: the bits of the aligned run"""
    c = lec.target_of(case)
    _, info, base = _target(geo, c, case["id"])
    _, info2, off = _target(geo, c, case["id"] + " misaligned", misalign=("A", "B", "d"))
    assert info["vec2"] & 1 and not info2["vec2"] & 1
    assert _same_bits(base[0], off[0]) and np.array_equal(base[1], off[1]) and all(_same_bits(a, b) for a, b in zip(base[2], off[2]))
