"""copra_amd/csrc/front_end.hpp on plans built by build_plan (through the emulator's emu_front_end): axis_solver_covers, lane_pass_covers and
weights_layout.  One case per `return false` of axis_solver_wanted and lane_pass_wanted as they stood in copra_hip.hip before the header existed
(commit b5d0ec2: the line is the first field of a case; expectations from that text), next to the same controller WITHOUT the one thing the line asks
about, which the front end covers.  What those lines ask of the handle -- AdaptState::axis_off and lane_off, prof_fine, lane_min_batch and
lane_batch_ok, packed, shared, the JIT handles -- stays in copra_hip.hip and has no plan to be tested on; line 532 (no build of the pass for the
shape) is tests/test_tier_builds.py's case 432."""
import numpy as np
import pytest

import controller_cases as C

from copra_amd._capi import OPTIONS


@pytest.fixture(scope="module")
def emu():
    import pyemu
    pyemu.lib()
    return pyemu


def _com(**kw):
    from copra_amd import workloads
    return workloads.com_preview(4, **kw)


def _coupled():
    return C.generic(5, 2, 12)


def _planar(N, tracking=False):
    wl = C.planar_integrator(4, N)
    if tracking:  # (a reference trajectory: FusedPlan::stage_refs)
        pf = np.tile(np.array([0.45, 0.3, 0.0, 0.0]), N + 1) * np.repeat(np.linspace(0, 1, N + 1), 4)
        wl["costs"] = [dict(kind="trajectory", M=np.kron(np.eye(N + 1), np.eye(4)), p=pf, weights=np.tile([10, 7, 1, 1.5], N + 1)), wl["costs"][1]]
    return wl


def _four_costs(wl):
    traj, ctrl = wl["costs"]  # (more cost terms than the pass and the Riccati-factor tier rebuild references for: lane_cref < 0)
    return dict(wl, costs=[traj, ctrl, dict(kind="target", M=np.eye(6)[:2], p=np.zeros(2), weights=[1.0, 1.0]), dict(kind="control", N=np.eye(3), p=np.zeros(3), weights=[1e-4] * 3)])


def _zero_weight():
    wl = _com()
    w0 = np.asarray(wl["costs"][0]["weights"], dtype=np.float64).copy()
    w0[4] = 0.0
    return dict(wl, costs=[dict(wl["costs"][0], weights=w0), wl["costs"][1]])


def _kinematic():
    from copra_amd import workloads
    return workloads.kinematic_preview(4)


def _jerk():
    from copra_amd import workloads
    return workloads.jerk_preview(4)


def _tracking():
    import cost_weights_cases as W
    return W.tracking(4)


def _initial_state():
    import fixtures as F
    pb = F.bounded_system("trajectory", N=12)
    return dict(A=np.tile(pb["A"], (2, 1, 1)), B=np.tile(pb["B"], (2, 1, 1)), x0=np.zeros((2, 2)), N=12, costs=pb["costs"], cstrs=pb["cstrs"])


def _limits(rows, nu, N):
    """per-instance right-hand sides of `rows` rows at every step and control bounds, for 4 instances"""
    return dict(row_rhs=np.full((4, rows * (N + 1)), 0.4), bounds=(np.full((4, nu * N), -1.0), np.full((4, nu * N), 1.0)))


COM_W = {0: np.ones((4, 6)), 1: np.ones((4, 3))}
IS = dict(R=10.0 * np.eye(2), r=np.array([0.1, -0.2]))
# name: (line of axis_solver_wanted | lane_pass_wanted, controller, options, inputs, axis covers, lane covers)
CASES = {
    "com": (None, _com, {}, {}, True, True),
    "axis_477_no_build_that_reads_weights": (477, _kinematic, {}, dict(cost_weights={0: np.ones((4, 3))}), False, False),
    "kinematic_without_weights": (None, _kinematic, {}, {}, True, True),
    "axis_481_weights_on_a_full_size_cost": (481, _tracking, {"no_stage_refs": 1}, dict(cost_weights={0: np.ones((4, 126))}), False, False),
    "axis_483_creation_weight_zero": (483, _zero_weight, {}, dict(cost_weights=COM_W), False, False),
    "creation_weight_zero_without_weights": (None, _zero_weight, {}, {}, True, True),
    "lane_524_weights": (524, _com, {}, dict(cost_weights=COM_W), True, False),
    "axis_486_no_axis_solver": (486, _com, {"no_axis_solver": 1}, {}, False, True),
    "axis_486_lane_525_no_lane_pass": (486, _com, {"no_lane_pass": 1}, {}, False, False),
    "axis_486_coupled_axes": (486, _coupled, {}, {}, False, True),
    "axis_488_lane_528_large": (488, lambda: _com(N=30), {}, {}, False, False),
    "axis_488_lane_528_initial_state": (488, _initial_state, {}, dict(initial_state=IS), False, False),
    "lane_528_no_tables_of_the_pass": (528, _jerk, {}, {}, True, False),
    "axis_491_lower_bounds_alone": (491, _com, {}, dict(bounds=(np.full((4, 60), -1.0), None)), False, True),
    "both_bounds": (None, _com, {}, dict(bounds=(np.full((4, 60), -1.0), np.full((4, 60), 1.0))), True, True),
    "axis_493_reference_of_no_cost": (493, _com, {}, dict(cost_refs={5: np.zeros((4, 6))}), False, True),
    "reference_of_the_first_cost": (None, _com, {}, dict(cost_refs={0: np.zeros((4, 6))}), True, True),
    "axis_497_stage_references_beyond_the_lanes_array": (497, lambda: _planar(31, True), {}, {}, False, True),
    "stage_references_within_it": (None, lambda: _planar(25, True), {}, {}, True, True),
    "planar_31": (None, lambda: _planar(31), {}, {}, True, True),
    "axis_499_no_build_for_the_horizon": (499, lambda: _planar(32), {}, {}, False, True),
    "lane_530_references_without_coefficients": (530, lambda: _four_costs(_com()), {}, dict(cost_refs={0: np.zeros((4, 6))}), False, False),
    "four_costs_without_references": (None, lambda: _four_costs(_com()), {}, {}, True, True),
    # (four cost terms: neither FusedPlan::lane_cref nor axis_cref -- also the second half of line 497's condition)
    "lane_531_stage_references_without_coefficients": (531, lambda: _four_costs(_tracking()), {}, {}, False, False),
    "stage_references_with_coefficients": (None, _tracking, {}, {}, True, True),
    # per-instance limits: only where BOTH builds the solver picks keep their tables in registers -- the others read the controller's limits
    # (front_end.hpp; line None: the rule is younger than the text the other lines are from)
    "limits_kinematic_second_chance_reads_lds": (None, _kinematic, {}, _limits(3, 3, 20), False, True),
    "limits_jerk_second_chance_reads_lds": (None, _jerk, {}, _limits(3, 3, 20), False, False),
    "limits_com_21_second_chance_reads_lds": (None, lambda: _com(N=21), {}, _limits(3, 3, 21), False, True),
    "limits_com_20_both_builds_in_registers": (None, _com, {}, _limits(3, 3, 20), True, True),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_covers(emu, monkeypatch, name):
    line, make, opts, inputs, axis, lane = CASES[name]
    wl = make()
    for k, v in opts.items():
        monkeypatch.setitem(OPTIONS, k, v)
    fe = emu.front_end(wl["A"], wl["B"], wl["N"], wl["costs"], wl["cstrs"], batch=len(wl["x0"]), **inputs)
    assert (fe["axis"], fe["lane"]) == (axis, lane), (line, fe)


# controller, options -> where weights_route sent it before front_end.hpp existed: `two_tier = dense && safe_two_tier && !lds_safe.ric; dense = false;
# layout = two_tier ? lds_safe : lds_full` (copra_hip.hip, lines 1744-1746)
@pytest.mark.parametrize("name", ["com", "short"])
def test_weights_layout(emu, monkeypatch, name):
    """weights_route, the part that is no state of the handle, against that text on the HostPlan's own fields (emu_front_end reports them): one controller that
    goes to lds_safe and one that goes to lds_full; and that layout is what a solve with weights then runs on"""
    monkeypatch.setitem(OPTIONS, "no_axis_solver", 1)
    wl = _com() if name == "com" else _com(N=5)  # (15 variables: the compact layout below the tier holds every column, so there is no safe tier)
    args = (wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], wl["costs"], wl["cstrs"])
    assert emu.lmpc_solve(*args)["riccati_factor"]
    fe = emu.front_end(wl["A"], wl["B"], wl["N"], wl["costs"], wl["cstrs"], batch=4)
    two_tier, dense, total, tri, ric, rcap = fe["reroute"]
    hp = fe["host_plan"]
    want_two_tier = bool(hp["dense"] and hp["safe_two_tier"] and not hp["lds_safe"][2])
    assert (bool(two_tier), bool(dense)) == (want_two_tier, False) and want_two_tier == (name == "com")
    assert (total, tri, ric, rcap) == (hp["lds_safe"] if want_two_tier else hp["lds_full"]) and not ric
    re = emu.lmpc_solve(*args, cost_weights={0: np.ones((4, 6)), 1: np.ones((4, 3))})
    assert not re["riccati_factor"] and (re["lds_bytes"], re["rcap"], re["factor_only"]) == (8 * total, rcap, bool(tri))


def test_weights_layout_routes_the_riccati_factor_tier_alone(emu):
    for make, inputs in ((_kinematic, {}), (lambda: _com(N=30), {}), (_initial_state, dict(initial_state=IS))):
        wl = make()
        assert emu.front_end(wl["A"], wl["B"], wl["N"], wl["costs"], wl["cstrs"], batch=len(wl["x0"]), **inputs)["reroute"] is None
