"""Which build of a tier or of the one-instance-per-lane pass a controller gets (copra_amd/csrc/tier_builds.hpp: the lists and picks behind
select_fused_kernel, select_tier2_kernel, select_lane_kernel, select_lane_shared_kernel and select_shared_kernel of copra_hip.hip, and behind the
bodies the emulator runs), and which front end may run (copra_amd/csrc/front_end.hpp).

PICKS: one case per `return` of the five selectors as they stood before the lists existed (their if-chains, commit b5d0ec2: the line of
copra_hip.hip is the first field of a case), the expected entry written by hand from that line.  An entry is (kind, nx, nu, nh, rp, qr, srefs, spec),
the fields its list does not have zero.  Q = kFusedQ1Regs."""
import numpy as np
import pytest

import controller_cases as C

from copra_amd._capi import OPTIONS

Q = 5
W4_MOST = 160 * 1024 // (9 * 8)  # doubles of LDS: the most at which nine instances fit a CU (the _w4 threshold)


def _ric(nx, nu, nh, qr, srefs):
    return ("ric", nx, nu, nh, 6, qr, srefs, False)


def _plain(kind, nx=0, nu=0, nh=0, rp=0, qr=0, srefs=False, spec=False):
    return (kind, nx, nu, nh, rp, qr, srefs, spec)


HEAD = dict(nx=6, nu=3, N=20, rmax=6)
MASS = dict(nx=2, nu=1, N=10, rmax=2)
PICKS = []
# select_fused_kernel, lines 152-153: the run-time-horizon builds of ric_aot_shape, whenever the horizon is none of ric_aot_exact
for nx, nu in ((6, 3), (4, 2), (2, 1)):
    for srefs in (0, 1):
        for q in (Q, 0):
            PICKS.append((152 if srefs else 153, "first", dict(nx=nx, nu=nu, N=12, tri=1, ric=1, q1regs=q, stage_refs=srefs), _ric(nx, nu, 0, q, bool(srefs))))
# lines 161-163 (stage references) and 165-167: (6, 3) at the compiled horizons
for line, N in ((161, 10), (162, 15), (163, 20)):
    for q in (Q, 0):
        PICKS.append((line, "first", dict(nx=6, nu=3, N=N, tri=1, ric=1, q1regs=q, stage_refs=1), _ric(6, 3, N, q, True)))
        PICKS.append((line + 4, "first", dict(nx=6, nu=3, N=N, tri=1, ric=1, q1regs=q), _ric(6, 3, N, q, False)))
PICKS += [
    # line 167, its fall-through: a Riccati-factor layout on a shape the library holds no build of (copra_batch_specialise gave it: its own code object runs)
    (167, "first", dict(nx=5, nu=3, N=12, tri=1, ric=1, q1regs=Q), _ric(6, 3, 20, Q, False)),
    (169, "first", dict(HEAD, tri=1, q1regs=Q), _plain("tri", 6, 3, 20, 6, Q)),
    (170, "first", dict(HEAD, tri=1), _plain("tri", 6, 3, 20, 6, 0)),
    (172, "first", dict(HEAD, rfull=126, tri=1, q1regs=Q), _plain("tri", 6, 3, 20, 0, Q)),
    (172, "first", dict(HEAD, rfull=126, tri=1), _plain("tri", 6, 3, 20, 0, 0)),
    (173, "first", dict(nx=4, nu=2, N=20, rmax=4, tri=1), _plain("tri")),
    (173, "first", dict(MASS, tri=1), _plain("tri")),  # (the falling mass has no factor-only build of its own)
    (173, "first", dict(HEAD, rmax=7, tri=1), _plain("tri")),  # (more cost rows than the headline's build pads to)
    (175, "first", dict(HEAD, lds_total=W4_MOST), _plain("square", 6, 3, 20, 6)),  # (before the _w4 threshold)
    (176, "first", dict(MASS, lds_total=100), _plain("square", 2, 1, 10, 2)),
    (177, "first", dict(HEAD, rfull=126), _plain("square", 6, 3, 20, 0)),
    (178, "first", dict(nx=3, nu=1, N=8, rmax=3, lds_total=W4_MOST), _plain("w4")),
    (179, "first", dict(nx=3, nu=1, N=8, rmax=3, lds_total=W4_MOST + 1), _plain("square")),
    (179, "first", dict(MASS, rmax=3, lds_total=W4_MOST + 1), _plain("square")),
    # select_tier2_kernel
    (184, "second", dict(HEAD), _plain("second", 6, 3, 20, 6)),
    (185, "second", dict(MASS), _plain("second", 2, 1, 10, 2)),
    (186, "second", dict(HEAD, rfull=126), _plain("second", 6, 3, 20, 0)),
    (187, "second", dict(nx=6, nu=3, N=15, rmax=6, lds_total=100), _plain("second")),
    # select_lane_kernel, line 432, and select_lane_shared_kernel, line 439: no build for the shape
    (432, "lane", dict(nx=5, nu=3, N=12), None),
    (439, "lane_shared", dict(nx=5, nu=3, N=12), None),
    # select_shared_kernel
    (134, "shared", dict(HEAD, tri=1), _plain("shared_tri", 6, 3, 20)),
    (135, "shared", dict(MASS, tri=1, lds_total=100), _plain("shared_tri")),
    (138, "shared", dict(HEAD, lds_total=100), _plain("shared_first", 6, 3, 20)),
    (138, "shared", dict(HEAD, tri=1, tier2=1), _plain("shared_tier2", 6, 3, 20)),
    (140, "shared", dict(MASS, lds_total=100), _plain("shared_first", 2, 1, 10)),
    (140, "shared", dict(MASS, tier2=1), _plain("shared_tier2", 2, 1, 10)),
    (141, "shared", dict(nx=3, nu=1, N=8, lds_total=W4_MOST), _plain("shared_w4")),
    (142, "shared", dict(nx=3, nu=1, N=8, lds_total=W4_MOST + 1), _plain("shared_first")),
    (142, "shared", dict(nx=3, nu=1, N=8, lds_total=100, tier2=1), _plain("shared_tier2")),
]
# select_lane_kernel, lines 426-427, and select_lane_shared_kernel, lines 436-438
for line, (nx, nu) in ((436, (6, 3)), (437, (4, 2)), (438, (2, 1))):
    for spec in (0, 1):
        PICKS.append((line, "lane_shared", dict(nx=nx, nu=nu, N=9, lane_spec=spec), _plain("lane_shared", nx, nu, spec=bool(spec))))
        for srefs in (0, 1):
            PICKS.append((426 if spec else 427, "lane", dict(nx=nx, nu=nu, N=9, lane_spec=spec, stage_refs=srefs), _plain("lane", nx, nu, srefs=bool(srefs), spec=bool(spec))))

# entries no plan reaches: none -- every entry of every list is the expectation of a case above (test_every_entry_is_picked_and_none_twice)
UNREACHED = {}


@pytest.fixture(scope="module")
def emu():
    import pyemu
    pyemu.lib()
    return pyemu


def _entries(emu, list_):
    out, k = [], 0
    while emu.tier_build_entry(list_, k) is not None:
        out.append(emu.tier_build_entry(list_, k))
        k += 1
    return out


@pytest.mark.parametrize("line,list_,plan,want", PICKS, ids=["%s-%d-%d" % (c[1], c[0], k) for k, c in enumerate(PICKS)])
def test_pick_is_the_selectors_return(emu, line, list_, plan, want):
    assert emu.tier_build(list_, **plan) == want, (line, plan)


def test_use_specialised_zero_is_the_emulators_alone(emu):
    """the run-time-shape build for a shape that has a build of its own: a parameter of the emulator's call of the pick"""
    assert emu.tier_build("first", **HEAD, tri=1, q1regs=0, specialised=False) == _plain("tri")
    assert emu.tier_build("first", **HEAD, lds_total=W4_MOST + 1, specialised=False) == _plain("square")
    assert emu.tier_build("first", **MASS, lds_total=100, specialised=False) == _plain("w4")
    assert emu.tier_build("second", **HEAD, specialised=False) == _plain("second")
    assert emu.tier_build("first", nx=6, nu=3, N=20, tri=1, ric=1, q1regs=Q, specialised=False) == _ric(6, 3, 20, Q, False)  # (the tier has no such form)


def test_every_entry_is_picked_and_none_twice(emu):
    for list_ in emu.TIER_LISTS:
        entries = _entries(emu, list_)
        assert len(set(entries)) == len(entries) > 0, list_
        picked = {c[3] for c in PICKS if c[1] == list_ and c[3] is not None}
        assert picked | set(UNREACHED.get(list_, ())) == set(entries), (list_, set(entries) - picked)
    sizes = {list_: len(_entries(emu, list_)) for list_ in emu.TIER_LISTS}
    assert sizes == dict(first=34, second=4, lane=12, lane_shared=6, shared=9)  # (the instantiations the library held before the lists)
    # the emulator's stand-ins for what copra_batch_specialise compiles: none of them a build the library holds
    standins = [emu.tier_build_entry("first_standins", k) for k in range(20)] + [emu.tier_build_entry("lane_standins", k) for k in range(4)]
    assert {e[:4] for e in standins[:20]} == {("ric", 6, 3, 12), ("ric", 4, 2, 16), ("ric", 5, 3, 12), ("ric", 2, 1, 10), ("ric", 2, 1, 40)}
    assert {e[:3] for e in standins[20:]} == {("lane", 5, 3)} and emu.tier_build_entry("first_standins", 20) is None and emu.tier_build_entry("lane_standins", 4) is None
    assert len(set(standins)) == 24 and not set(standins) & set(_entries(emu, "first") + _entries(emu, "lane"))


# ---- end to end: what ran is what the pick names ----
def _full_size():
    from copra_amd import workloads
    from copra_amd.autospan import autospan_cost
    wl = workloads.com_preview(4, v_max=0.3, u_max=1.5, seed=9)
    wl["costs"] = [autospan_cost(dict(wl["costs"][0], p=np.tile(wl["costs"][0]["p"], 21))), wl["costs"][1]]
    return wl


def _tight(b=8):
    from copra_amd import workloads
    return workloads.com_preview(b, v_max=0.25, u_max=1.2)


def _cases():
    from copra_amd import workloads
    import cost_weights_cases as W
    tier = {"no_axis_solver": 1, "no_lane_pass": 1}  # (every instance through the first tier)
    second6 = _plain("second", 6, 3, 20, 6)
    return {
        "headline_behind_the_pass": (lambda: _tight(), {"no_axis_solver": 1}, {}, dict(first=_ric(6, 3, 20, Q, False), second=second6, lane=_plain("lane", 6, 3, spec=True))),
        "headline_stage_references": (lambda: W.tracking(8), tier, {}, dict(first=_ric(6, 3, 20, Q, True))),
        "planar_run_time_horizon": (lambda: C.planar_integrator(4, 2), tier, {}, dict(first=_ric(4, 2, 0, Q, False))),
        # (N = 48 is the smallest: a single-control system gets the Riccati-factor tier from 48 variables on -- plan_builder.hpp, build_plan)
        "falling_mass_run_time_horizon": (lambda: workloads.double_integrator(4, N=48), tier, {}, dict(first=_ric(2, 1, 0, Q, False))),
        "full_size_cost": (_full_size, {"no_stage_refs": 1, "no_step_rows": 1}, {}, dict(first=_plain("tri", 6, 3, 20, 0, Q))),
        "generic_w4": (lambda: C.generic(3, 1, 4), {}, {}, dict(first=_plain("w4"))),
        "generic_beyond_w4": (lambda: C.generic(5, 2, 20), {}, {}, dict(first=_plain("square"), second=_plain("second"))),
        "shared_records": (lambda: _tight(), {}, dict(shared=True), dict(first=_ric(6, 3, 20, Q, False), lane_shared=_plain("lane_shared", 6, 3, spec=True),
                                                                        shared_second=_plain("shared_tier2", 6, 3, 20))),
        "shared_plain": (lambda: _tight(), {"no_ric_shared": 1}, dict(shared=True), dict(shared=_plain("shared_tri", 6, 3, 20), shared_second=_plain("shared_tier2", 6, 3, 20))),
        "weights_reroute": (lambda: _tight(), tier, dict(weights=True), dict(first=_plain("square", 6, 3, 20, 6), second=second6)),
    }


CASES = ["headline_behind_the_pass", "headline_stage_references", "planar_run_time_horizon", "falling_mass_run_time_horizon", "full_size_cost",
         "generic_w4", "generic_beyond_w4", "shared_records", "shared_plain", "weights_reroute"]


@pytest.mark.parametrize("name", CASES)
def test_what_ran_is_what_the_pick_names(emu, monkeypatch, name):
    """small batches through emu_lmpc_solve / emu_lmpc_solve_shared: emu_last_tier_run reports these entries and no other launch"""
    import cost_weights_cases as W
    make, opts, how, want = _cases()[name]
    wl = make()
    for k, v in opts.items():
        monkeypatch.setitem(OPTIONS, k, v)
    if how.get("shared"):
        re = emu.lmpc_solve_shared(wl["A"][0], wl["B"][0], wl["d"][0], wl["x0"], wl["N"], wl["costs"], wl["cstrs"])
    else:
        cw = None
        if how.get("weights"):
            ws, _ = W.grouped_weights(wl, len(wl["x0"]), 5)
            cw = {t: w for t, w in enumerate(ws) if w is not None}
        re = emu.lmpc_solve(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], wl["costs"], wl["cstrs"], cost_weights=cw)
    assert (re["status"] == 0).all()
    ran = {k: v for k, v in emu.last_tier_run().items() if v is not None}
    assert ran == want
    if "second" in want or "shared_second" in want:
        assert re["overflowed"] > 0
