"""The score and target kernels at their launch edges on the device: what launch_score (copra_hip_score.hip) and launch_target
(copra_hip_target.hip) decide at shapes no other GPU test reaches.  The cases are those of tests/launch_edge_cases.py, which
tests/test_score_target_edges_emu.py runs bit for bit on the kernels' own bodies on the host: a case that passes there and fails here is a
fault of the device side -- divergent LDS addressing, the dynamic-LDS opt-in, the grid arithmetic, a contraction of a product with the sum
behind it -- not of the arithmetic.

Score: test_score_gpu's _replay / _compare -- tests/score_ref.py over the device's OWN x_hist / u_hist / age_hist; counters and viol_max
exact, the sums within 2 gamma(k) S (tests/test_score_abi.py).  Targets: test_target_gpu's _check_targets -- the status of
target_ref.gepp, |z - z_true|_inf <= n^2 cond_inf(M) 2^-53 |z_true|_inf, a reference row in addition (n + 1) 2^-53 (|T| |z|)_i
(tests/test_target_abi.py), singular instances bit for bit; the conditions on the inputs (launch_edge_cases.target_preconditions) are
asserted on the reference before the device is looked at.  No solve is needed for the targets: set_target launches the kernel.

Every test asserts the property it is named for from the emulators' geometry exports (emu_score_launch_group, emu_score_layout,
emu_target_launch_group, emu_target_image_bytes, emu_target_lds_max); the values in the docstrings are those at HEAD.  The figures printed
(-s) are recorded in profiles/closed_loop/score_target_edges.txt."""
import numpy as np
import pytest

import launch_edge_cases as lec
import test_target_gpu as tg
from test_closed_loop_gpu import _engine
from test_score_gpu import _compare, _numpy, _replay, _set
from test_tick_edges_gpu import mixed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def geo(tmp_path_factory):
    return lec.build_emulators(tmp_path_factory.mktemp("emu_edges"))


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the score ----
def _creatable(geo, case):
    """(nx, scenario, measure, controller) at the largest nx' <= nx that keeps the case's property and that BatchLMPC accepts"""
    from copra_amd import _capi
    keeps = lec.score_property(geo, case)
    for n in range(case["nx"], 1, -1):
        if not keeps(n):
            break
        S, m = lec.score_case(case, n)
        try:
            eng = _engine(S["wl"])
            eng.solve()
        except _capi.CopraUnsupported as e:
            print("%s: nx %d refused (%s)" % (case["id"], n, e))
            continue
        if n != case["nx"]:
            print("%s: nx stepped down from %d to %d" % (case["id"], case["nx"], n))
        return n, S, m, eng
    raise AssertionError("%s: no creatable shape keeps the property" % case["id"])


def _score(geo, case, S, m, eng, what=None):
    """a rollout of the case's ticks with measure m: the records against score_ref over the device's own histories"""
    what = what or case["id"]
    G = lec.score_geometry(geo, m)
    g = lec.given(m)
    _set(eng, g)
    ticks = case["ticks"]
    hist = _numpy(eng.rollout(ticks, x_hist=True, u_hist=True, age_hist=True, status_hist=True, disturbances=np.ascontiguousarray(S["w_seq"][:ticks])))
    mixed(hist["status_hist"])
    got = eng.score()
    want, Sabs = _replay(hist, g)
    print("%s: nx %d, group %d, image %d bytes, %d workgroups" % (what, m["nx"], G["group"], G["bytes"], -(-S["batch"] // G["group"])))
    _compare(got, want, Sabs, ticks, what, nx=m["nx"], nu=m["nu"])
    assert (got["held"][list(S["held"])] == ticks).all() and got["held"].sum() == ticks * len(S["held"])
    return got, G


def _not_vacuous(got, m, what):
    """where the measure gives a field a source, the field moved"""
    g = lec.given(m)
    if g["qx"] is not None:
        assert (got["jx"] != 0).any(), what
    if any(g[k] is not None for k in lec.LIMITS):
        assert (got["violating"] > 0).any() and (got["viol_max"] > 0).any(), what


@pytest.mark.parametrize("case", lec.S1, ids=lambda c: c["id"])
def test_score_group_one(geo, case):
    """S1, dense per-instance weights at (40, 1), batch 5, three ticks: one instance per workgroup, every copy the scalar loop"""
    n, S, m, eng = _creatable(geo, case)
    assert lec.score_geometry(geo, m)["group"] == 1
    got, _ = _score(geo, case, S, m, eng)
    _not_vacuous(got, m, case["id"])


@pytest.mark.parametrize("case", lec.S2, ids=lambda c: c["id"])
def test_score_image_above_48_kib(geo, case):
    """S2, dense weights at (78, 1), N = 1, batch 5, two ticks, the measure shared and per instance: the launch opts in to more than 48 KiB
    of dynamic LDS"""
    n, S, m, eng = _creatable(geo, case)
    assert lec.score_geometry(geo, m)["bytes"] > lec.KIB48
    got, _ = _score(geo, case, S, m, eng)
    _not_vacuous(got, m, case["id"])


@pytest.mark.parametrize("case", lec.S3, ids=lambda c: c["id"])
def test_score_small_even_groups(geo, case):
    """S3, dense (23, 1) x 13, diagonal (40, 1) x 13, dense (9, 3) x 33: groups 4, 10 and 16, more than one workgroup and a partial last one"""
    n, S, m, eng = _creatable(geo, case)
    G = lec.score_geometry(geo, m)
    assert 2 <= G["group"] <= 16 and G["group"] % 2 == 0 and S["batch"] > G["group"] and S["batch"] % G["group"] != 0
    got, _ = _score(geo, case, S, m, eng)
    _not_vacuous(got, m, case["id"])


@pytest.mark.parametrize("case", lec.S4, ids=lambda c: c["id"])
def test_score_shared_reference_of_odd_rows(geo, case):
    """S4, (5, 2) and (9, 3), batch 13, a shared x_ref of 3 steps, six ticks: batch nx is odd and the reference row starts on 16 bytes only
    every other row -- those ticks copy double by double.  The same signal tiled per instance (every row gathered) gives bit-equal records"""
    S, m = lec.score_case(case)
    rows = lec.reference_rows(m, case["ticks"])
    assert (case["batch"] * case["nx"]) % 2 == 1 and {(r * case["nx"]) % 2 for r in rows} == {0, 1}
    got, _ = _score(geo, case, S, m, _engine(S["wl"]))
    _not_vacuous(got, m, case["id"])
    per, _ = _score(geo, case, S, lec.tiled(m, case["batch"]), _engine(S["wl"]), what=case["id"] + ", tiled per instance")
    assert _bits(got, per), [f for f in got.dtype.names if not _bits(got[f], per[f])]


@pytest.mark.parametrize("case", lec.S5, ids=lambda c: c["id"])
def test_score_image_with_parts_absent(geo, case):
    """S5, (5, 2), batch 13: qx alone; the control box alone; dense qx and x_ref with no limits -- the fields that have no source stay 0"""
    S, m = lec.score_case(case)
    assert lec.score_geometry(geo, m)["bytes"] < lec.score_geometry(geo, dict(m, leave=()))["bytes"]
    got, _ = _score(geo, case, S, m, _engine(S["wl"]))
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


def test_score_what_does_not_fit_is_refused(geo):
    """S6: dense weights at the first nx whose image passes the LDS limit (141 at HEAD), where a controller of that nx can be created:
    CopraUnsupported; the diagonal measure at the same nx is accepted and one tick scores"""
    from copra_amd import _capi
    top = geo.target.emu_target_lds_max()
    bad = lec.first_beyond(geo, 1, 1, top)
    assert geo.score.emu_score_image_bytes(bad, 1, 0) <= top
    case = lec._s("S6 diagonal at nx %d" % bad, bad, 1, 5, 1, 1, False, False)
    S, m = lec.score_case(case)
    try:
        eng = _engine(S["wl"])
        eng.solve()
    except _capi.CopraUnsupported as e:
        print("S6: dense nx %d is the first that does not fit, and no controller of that nx can be created (%s)" % (bad, e))
        return
    dense = lec.measure(bad, 1, None, True, seed=1)
    with pytest.raises(_capi.CopraUnsupported):
        _set(eng, dense)
    with pytest.raises(_capi.CopraRuntimeError):
        eng.score()  # (the refused call did not turn scoring on)
    print("S6: dense nx %d is refused (%d > %d bytes)" % (bad, geo.score.emu_score_image_bytes(bad, 1, 1), top))
    got, _ = _score(geo, case, S, m, eng)
    _not_vacuous(got, m, case["id"])


# ---- the targets ----
def _target(geo, c, what, eng=None):
    """set_target on a fresh controller of case c, checked by _check_targets; returns (geometry, z, references, controller)"""
    G = lec.target_geometry(geo, c)
    lec.target_preconditions(c, what)  # (on the reference alone, before the device is looked at)
    eng = _engine(c["wl"]) if eng is None else eng
    costs = list(range(len(c["maps"])))
    eng.set_target(c["H"], c["r"], costs, offset=c["offset"])
    tg.WORST["z"] = tg.WORST["p"] = 0.0  # (the figures printed are this case's own)
    print("%s: group %d, one wave's image %d bytes, %d workgroups" % (what, G["group"], G["bytes"], -(-c["batch"] // G["group"])))
    z, refs = tg._check_targets(eng, c["wl"], c["H"], c["r"], offset=c["offset"], what=what, singular=c["planted"], kept=(c["z0"], c["out0"]),
                                maps=c["maps"], costs=costs)
    for k, (T, s) in enumerate(c["costs"]):
        assert refs[k].shape == (c["batch"], s * T.shape[0]), (what, k)
    return G, z, refs, eng


@pytest.mark.parametrize("case", lec.T1, ids=lambda c: c["id"])
def test_target_groups_with_lanes_that_disagree(geo, case):
    """T1, (3, 2) x 513, (4, 2) x 257, (6, 1) x 257, (6, 3) x 129: groups 256, 128, 128 (odd n) and 64 -- two full workgroups and a partial
    one; per-instance setpoints (3 steps, offset 1) on the second and fourth; singular instances at index 2, at index == group and at
    batch - 1; the lanes of a wave pick different pivot rows"""
    c = lec.target_of(case)
    G = lec.target_geometry(geo, c)
    assert c["batch"] == 2 * G["group"] + 1 and G["group"] in (64, 128, 256)
    lec.plant(c, G["group"])
    _target(geo, c, case["id"])


@pytest.mark.parametrize("case", lec.T2, ids=lambda c: c["id"])
def test_target_largest_image_that_fits(geo, case):
    """T2, (14, 3) x 65 and (13, 3) x 65: n = 17 is the largest image the setter accepts (above 48 KiB, within the LDS limit: one more
    state does not fit); n = 16 takes the paired store of z"""
    c = lec.target_of(case)
    G = lec.target_geometry(geo, c)
    n = c["nx"] + c["nu"]
    assert lec.KIB48 < G["bytes"] <= G["top"] and G["group"] == 64 and c["batch"] > G["group"]
    if n % 2:
        assert geo.target.emu_target_image_bytes(c["nx"] + 1, c["nu"], 0) > G["top"]
    _target(geo, c, case["id"])


def test_target_eight_driven_costs_above_48_kib(geo):
    """T3, (6, 3) x 70, N = 2: eight driven costs with S_c = 1, N and N + 1 and odd and even r_c S_c; the maps push the image above 48 KiB;
    the S_c blocks of a cost are bit-equal"""
    c, shapes = lec.eight_cost_case(geo)
    assert len(shapes) == 8 and {s for _, s in shapes} == {1, c["N"], c["N"] + 1} and {(r * s) % 2 for r, s in shapes} == {0, 1}
    G, z, refs, _ = _target(geo, c, "T3 eight costs")
    assert G["bytes"] > lec.KIB48
    for k, (r, s) in enumerate(shapes):
        blocks = refs[k].reshape(c["batch"], s, r)
        assert all(_bits(np.ascontiguousarray(blocks[:, j]), np.ascontiguousarray(blocks[:, 0])) for j in range(s)), k


@pytest.mark.parametrize("case", lec.T4, ids=lambda c: c["id"])
def test_target_inputs_off_16_bytes(geo, case):
    """T4, (5, 2) and (6, 3), batch 14: set_system from CUDA views 8 bytes past a 16-byte boundary against tensors of their own, the same
    for H and the signal: z, status and the references bit-equal (and right: _check_targets on the aligned run)"""
    import torch
    c = lec.target_of(case)
    wl = c["wl"]
    arrays = dict(A=np.swapaxes(wl["A"], 1, 2), B=np.swapaxes(wl["B"], 1, 2), d=wl["d"], x0=wl["x0"], H=c["H"].T, r=c["r"])  # (the ABI's layout)
    outs = {}
    for mis in (False, True):
        t = {}
        for k, a in arrays.items():
            a = np.ascontiguousarray(a)
            room = torch.zeros(a.size + 2, dtype=torch.float64, device="cuda")
            off = 1 if mis else 0
            t[k] = room[off:off + a.size].view(a.shape)
            t[k].copy_(torch.from_numpy(a))
            assert t[k].is_contiguous() and t[k].data_ptr() % 16 == (8 if mis else 0)
        eng = _engine(wl)
        eng.set_target(t["H"], t["r"], [0, 1], offset=c["offset"])
        eng.set_system(t["A"], t["B"], t["d"], t["x0"])  # (used in place: the launch behind it reads the views)
        outs[mis] = (eng.target(), eng.target_status(), eng.cost_reference(0), eng.cost_reference(1))
        if not mis:
            _target(geo, c, case["id"], eng=eng)  # (set_target again, from host arrays: the same launch, checked)
            again = (eng.target(), eng.target_status(), eng.cost_reference(0), eng.cost_reference(1))
            assert all(_bits(a, b) for a, b in zip(outs[mis], again))
    assert not outs[False][1].any() and np.abs(outs[False][0]).max() > 0
    for a, b in zip(outs[False], outs[True]):
        assert _bits(a, b)
