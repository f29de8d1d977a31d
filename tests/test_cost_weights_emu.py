"""Per-instance cost weights (copra_batch_set_cost_weights) on the kernel BODIES, run lane by lane on the CPU (tests/emu) against the oracle run
with each instance's own weights (tests/cost_weights_cases.py): the builds of the (instance, axis)-per-lane solver that rebuild their tables from
the instance's weights (lmpc_axis.hpp, WTS: the families first_w and list_w of axis_builds.hpp), the routing that keeps every kernel with the
creation weights in its tables away (copra_amd/csrc/front_end.hpp: axis_solver_covers, lane_pass_covers, weights_layout -- the library's and the emulator's),
and cost_weights(P, t, inst) of the generic bodies (lmpc_fused.hpp, islmpc_fused.hpp, lmpc_large.hpp).

Measures: RTOL = 1e-6 with the suite's floor of 1e-3.  Scattered weights (log-uniform over two decades per row) are compared norm-wise per instance
(cost_weights_cases.rel_inst, as tests/test_cost_weights_gpu.py argues); weights that equal or scale the creation weights uniformly entry by entry.

The emulator has no body of the packed forms (several instances per wavefront: packed_impl.inc is launched by the library only); their
weight indexing is covered on the device (tests/test_cost_weights_gpu.py::test_packed_kernels_with_instance_weights)."""
import os

import numpy as np
import pytest

from copra_amd._capi import OPTIONS, CopraUnsupported

import cost_weights_cases as W
import fixtures as F

AXIS = W.axis_cases()


@pytest.fixture(scope="module")
def emu():
    import pyemu
    pyemu.lib()
    return pyemu


def _solve(emu, wl, ws, two_slot=False, **kw):
    old = os.environ.pop("COPRA_EMU_AXIS_QMAX2", None)
    if two_slot:
        os.environ["COPRA_EMU_AXIS_QMAX2"] = "1"
    try:
        cw = None if ws is None else {t: w for t, w in enumerate(ws) if w is not None}
        re = emu.lmpc_solve(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], wl["costs"], wl["cstrs"], cost_weights=cw, **kw)
        re["axis"] = emu.last_axis_run()
        return re
    finally:
        os.environ.pop("COPRA_EMU_AXIS_QMAX2", None)
        if old is not None:
            os.environ["COPRA_EMU_AXIS_QMAX2"] = old


def _same_bits(a, b, sel=slice(None)):
    return all(np.array_equal(a[k][sel], b[k][sel], equal_nan=True) for k in W.KEYS)


# ---- the (instance, axis)-per-lane solver, WTS builds ----
@pytest.mark.parametrize("name", sorted(AXIS))
def test_axis_solver_weight_builds_against_the_oracle(emu, oracle, name):
    """the workloads of tests/test_axis_trip_bounds.py (85 instances: 4 waves and instances on spare lanes), two rows per axis and step, N = 12
    (the builds without the horizon compiled in) and axis-major state order, every instance with its own log-uniform weights on both costs:
    the first_w and list_w entries the case names ran, and statuses, both counters, U and X are the oracle's.  The tight cases leave instances
    to the second launch and to the tier; the two-slot mode of the loose workload to the second launch (sixteen slots there hold every active
    set that workload has, so none of it reaches the tier)."""
    wl, two_slot, builds, tight = AXIS[name]
    b = len(wl["x0"])
    ws, group = W.grouped_weights(wl, b, 5)
    re = _solve(emu, wl, ws, two_slot)
    ax = re["axis"]
    assert ax is not None and (ax["first"], ax["second"]) == builds
    nx, nu = wl["B"].shape[1], wl["B"].shape[2]
    assert emu.axis_build(nx, nu, wl["N"], True, builds[0][7], False, True, False) == builds[0]
    assert emu.axis_build(nx, nu, wl["N"], True, builds[0][7], False, True, True) == builds[1]
    assert re["lane_pass_finished"] > 0
    assert not re["riccati_factor"]  # (weights_route: the tier behind the solver is a generic one-wave kernel)
    if tight or two_slot:
        assert ax["listed_first"] > 0
    if tight:
        assert 0 < ax["listed_second"] < ax["listed_first"] and re["lane_pass_finished"] == b - ax["listed_second"]
    W.assert_matches(re, W.oracle_grouped(oracle, wl, ws, group))


@pytest.mark.parametrize("two_row", [False, True])
def test_reference_trajectory_cost_with_weights(emu, oracle, two_row):
    """weights next to a reference-trajectory cost (stage_refs: the builds without EXACT even at N = 20), the step's six weights repeated along
    the horizon: first_w (EXACT false, CT, RPA 1 and 2)"""
    wl = W.tracking(43, two_row=two_row)
    ws, group = W.tracking_weights(wl, 43, 31)
    re = _solve(emu, wl, ws)
    assert re["axis"] is not None and re["axis"]["first"] == ("first_w", 2, 3, 20, 6, False, True, 2 if two_row else 1)
    assert re["axis"]["second"] == ("list_w", 2, 3, 20, 16, False, True, 2)
    assert re["lane_pass_finished"] >= 41
    W.assert_matches(re, W.oracle_grouped(oracle, wl, ws, group))


def test_every_first_w_entry_is_picked_and_the_lds_list_w_entry_never(emu):
    """axis_builds.hpp: the four first_w entries are the picks of the cases above (checked here on the pick alone), and a controller that
    gets a first_w build -- all of them keep their tables in registers, CT -- gets the CT list_w entry: pick_axis_build prefers CT wherever
    axis_const holds, and without axis_const there is no first_w build, so axis_solver_wanted answers no before the second launch is picked.
    The list_w entry that reads its tables from LDS is picked only by a direct call with axis_const = false."""
    seen = set()
    for N in range(1, 21):
        for rpa in (0, 1, 2):
            for stage_refs in (False, True):
                first = emu.axis_build(6, 3, N, True, rpa, stage_refs, True, False)
                assert first is not None and first[0] == "first_w" and first[6]
                seen.add(first)
                assert emu.axis_build(6, 3, N, True, rpa, stage_refs, True, True) == ("list_w", 2, 3, 20, 16, False, True, 2)
                assert emu.axis_build(6, 3, N, False, rpa, stage_refs, True, False) is None  # -> the solver is not wanted at all
    assert seen == {("first_w", 2, 3, 20, 6, e, True, r) for e in (False, True) for r in (1, 2)}
    ran = {c[2][0] for c in AXIS.values()} | {("first_w", 2, 3, 20, 6, False, True, 1), ("first_w", 2, 3, 20, 6, False, True, 2)}
    assert ran == seen


@pytest.mark.parametrize("name", ["com_v06", "com_v06_two_slot", "com_v025", "com_v025_two_slot"])
def test_creation_weights_per_instance_give_the_bits_of_the_reference_rebuild(emu, monkeypatch, name):
    """per-instance weights EQUAL to the creation weights against per-instance references equal to the controller-wide ones (no weights): both
    lanes rebuild h and hN from the coefficients of FusedPlan::axis_cref; with w = w0 the weight code adds (1 - 1) / w0 ch ch' = 0 to H and
    scales the coefficients by w / w0 = 1 -- the same bits in U, X, status and iter.  The tier behind the solver is pinned to the generic
    one-wave kernel (no_ric) for both runs: what the solver does not finish is then solved by the same body too."""
    wl, two_slot, _, _ = AXIS[name]
    b = len(wl["x0"])
    monkeypatch.setitem(OPTIONS, "no_ric", 1)
    monkeypatch.setenv("COPRA_EMU_LANE_FILTER", "1")  # (the harness asks for a tier the pass can stand in front of: with no_ric it filters)
    ws = [np.tile(np.asarray(c["weights"], dtype=np.float64), (b, 1)) for c in wl["costs"]]
    refs = {0: np.tile(wl["costs"][0]["p"], (b, 1)), 1: np.tile(wl["costs"][1]["p"], (b, 1))}
    rw = _solve(emu, wl, ws, two_slot)
    rr = _solve(emu, wl, None, two_slot, cost_refs=refs)
    assert rw["axis"]["first"][0] == "first_w" and rr["axis"]["first"][0] == "first"
    assert rw["lane_pass_finished"] == rr["lane_pass_finished"] > 0
    assert _same_bits(rw, rr)


# ---- next to the other per-instance inputs ----
def test_weights_with_per_instance_references(emu, oracle):
    from copra_amd import workloads
    b = 44
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=31)
    ws, group = W.indexed_weights(wl, b)
    goals = wl["costs"][0]["p"][None, :] + 0.3 * np.random.default_rng(21).standard_normal((b, 6))
    re = _solve(emu, wl, ws, cost_refs={0: goals})
    assert re["axis"] is not None and re["lane_pass_finished"] >= b - 2
    ro = W.oracle_grouped(oracle, wl, ws, group, costs_of=lambda k, costs: [dict(costs[0], p=goals[k]), costs[1]])
    W.assert_matches(re, ro)


def test_weights_with_per_instance_limits(emu, oracle):
    """every instance its own velocity and actuator limits, constant along the horizon, next to its own weights"""
    from copra_amd import workloads
    rng = np.random.default_rng(33)
    b, inf = 47, np.inf
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=13)
    N = wl["N"]
    ws, group = W.indexed_weights(wl, b)
    vlim, ulim = 0.5 * rng.uniform(0.6, 1.3, b), 2.5 * rng.uniform(0.6, 1.3, b)
    rhs = np.repeat(vlim[:, None], 3 * (N + 1), axis=1)
    lo, hi = -np.repeat(ulim[:, None], 3 * N, axis=1), np.repeat(ulim[:, None], 3 * N, axis=1)
    re = _solve(emu, wl, ws, row_rhs=rhs, bounds=(lo, hi))
    assert re["axis"] is not None and re["lane_pass_finished"] >= b - 3

    def cstrs_of(k):
        up = np.full((N + 1, 6), inf)
        up[:, 3:] = vlim[k]
        return [dict(kind="trajectory_bound", lower=np.full(6 * (N + 1), -inf), upper=up.reshape(-1)), dict(kind="control_bound", lower=lo[k], upper=hi[k])]
    W.assert_matches(re, W.oracle_grouped(oracle, wl, ws, group, cstrs_of=cstrs_of))


# ---- indexing ----
@pytest.mark.parametrize("b", [1, 20, 21, 22, 64])
def test_every_lane_reads_its_own_instance_and_row(emu, oracle, b):
    """one instance, a wave short of one, exactly one wave (21 instances x 3 axes), one instance on the spare lanes, three waves and a spare:
    instance k's weights are a function of k and differ from row to row -- against the oracle instance by instance.  Swapping the weights of
    two instances changes the results of exactly those two."""
    from copra_amd import workloads
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=7)
    ws, group = W.indexed_weights(wl, b)
    re = _solve(emu, wl, ws)
    assert re["axis"] is not None and re["lane_pass_finished"] >= b - 1
    W.assert_matches(re, W.oracle_grouped(oracle, wl, ws, group), skip=0)
    if b > 1:
        i, j = (b - 1, b // 2)  # (b = 22: the instance on the spare lanes and one of the regular ones)
        sw = [w.copy() for w in ws]
        for w in sw:
            w[[i, j]] = w[[j, i]]
        rs = _solve(emu, wl, sw)
        others = np.ones(b, dtype=bool)
        others[[i, j]] = False
        assert _same_bits(re, rs, others)
        for k in (i, j):
            assert W.rel(rs["control"][k], re["control"][k]) > 100 * W.RTOL


# ---- routing ----
def test_zero_creation_weight_goes_to_the_generic_tier(emu, oracle):
    """a row created with weight zero and a non-zero weight per instance: the lane would divide by the creation weight -- axis_solver_wanted says
    no, the one-instance-per-lane pass is off while weights are set, the generic one-wave kernel solves every instance"""
    from copra_amd import workloads
    b = 24
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=3)
    w0 = np.asarray(wl["costs"][0]["weights"], dtype=np.float64).copy()
    w0[4] = 0.0
    wl["costs"] = [dict(wl["costs"][0], weights=w0), wl["costs"][1]]
    ws, group = W.indexed_weights(wl, b)
    ws[0][:, 4] = 0.5 + 0.1 * np.arange(b)
    base = _solve(emu, wl, None)
    assert base["axis"] is not None and base["lane_pass_finished"] > 0  # (without instance weights the zero row is no obstacle)
    re = _solve(emu, wl, ws)
    assert re["axis"] is None and max(re["lane_pass_finished"], 0) == 0 and not re["riccati_factor"]
    W.assert_matches(re, W.oracle_grouped(oracle, wl, ws, group))


@pytest.mark.parametrize("t", [0, 1])
def test_weights_on_one_cost_only(emu, oracle, t):
    from copra_amd import workloads
    b = 30
    wl = workloads.com_preview(b, v_max=0.4, u_max=2.0, seed=19)
    ws, group = W.indexed_weights(wl, b)
    ws[1 - t] = None
    re = _solve(emu, wl, ws)
    assert re["axis"] is not None and re["axis"]["first"][0] == "first_w" and re["lane_pass_finished"] >= b - 2
    W.assert_matches(re, W.oracle_grouped(oracle, wl, ws, group))


def test_weights_restored_to_none_give_the_bits_of_a_run_that_never_had_them(emu):
    from copra_amd import workloads
    b = 30
    wl = workloads.com_preview(b, v_max=0.4, u_max=2.0, seed=19)
    ws, _ = W.indexed_weights(wl, b)
    never = _solve(emu, wl, None)
    with_w = _solve(emu, wl, ws)
    assert W.rel(with_w["control"], never["control"]) > 100 * W.RTOL
    for restored in (_solve(emu, wl, None), _solve(emu, wl, [None, None])):
        assert restored["axis"]["first"][0] == "first" and restored["riccati_factor"] == never["riccati_factor"]
        assert _same_bits(restored, never)


def test_other_axis_shapes_leave_weights_to_the_generic_tier(emu, oracle):
    """a horizon of 21 has builds of the solver but none that reads weights: generic tier, the oracle's results"""
    from copra_amd import workloads
    b = 6
    wl = workloads.com_preview(b, N=21, v_max=0.5, u_max=2.5, seed=5)
    ws, group = W.indexed_weights(wl, b)
    assert _solve(emu, wl, None)["axis"] is not None
    re = _solve(emu, wl, ws)
    assert re["axis"] is None
    W.assert_matches(re, W.oracle_grouped(oracle, wl, ws, group))


def test_entry_points_that_cannot_honour_weights_refuse(emu):
    """the shared-model and the Riccati interior-point entry points of the emulator hold the creation weights in their model and stage plan, as
    the library's do: CopraUnsupported, and a dense (host-evaluated) cost has no weights the kernels read"""
    from copra_amd import workloads
    b = 4
    wl = workloads.com_preview(b)
    ws, _ = W.indexed_weights(wl, b)
    with pytest.raises(CopraUnsupported):
        emu.lmpc_solve_shared(wl["A"][0], wl["B"][0], wl["d"][0], wl["x0"], wl["N"], wl["costs"], wl["cstrs"], cost_weights={0: ws[0]})
    with pytest.raises(CopraUnsupported):
        emu.lmpc_solve_riccati(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], wl["costs"], wl["cstrs"], cost_weights={1: ws[1]})
    n = 3 * wl["N"]
    dense = dict(kind="dense", Q=1e-3 * np.eye(n), c=np.zeros(n))
    with pytest.raises(CopraUnsupported):
        emu.lmpc_solve(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], [wl["costs"][0], dense], wl["cstrs"], cost_weights={1: np.ones((b, n))})
    # ... and nothing of it is left behind for the next solve
    re = emu.lmpc_solve(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], wl["costs"], wl["cstrs"])
    assert emu.last_axis_run()["first"][0] == "first" and (re["status"] == 0).all()


def test_a_dense_cost_in_front_shifts_the_slot_not_the_weights(emu, oracle):
    """the user's cost index maps through cost_slot as the setter does: with a dense cost first, weights given for cost 1 reach kernel term 0"""
    from copra_amd import workloads
    b = 5
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=3)
    n = 3 * wl["N"]
    dense = dict(kind="dense", Q=1e-3 * np.eye(n), c=np.zeros(n))
    ws, _ = W.indexed_weights(wl, b)
    costs = [dense, wl["costs"][0], wl["costs"][1]]
    re = emu.lmpc_solve(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], costs, wl["cstrs"], cost_weights={1: ws[0], 2: ws[1]})
    for k in range(b):
        twin = dict(kind="control", N=np.eye(3), p=np.zeros(3), weights=[1e-3] * 3)  # (the oracle takes no dense cost: the same term, built in)
        ck = [twin, dict(wl["costs"][0], weights=ws[0][k]), dict(wl["costs"][1], weights=ws[1][k])]
        ro = oracle.lmpc_solve(wl["A"][k], wl["B"][k], wl["d"][k], wl["x0"][k], wl["N"], ck, wl["cstrs"])
        assert re["status"][k] == ro["status"] == 0 and tuple(re["iter"][k]) == tuple(ro["iter"])
        assert W.rel_inst(re["control"][k][None], ro["control"][None]) <= W.RTOL


# ---- the generic bodies: cost_weights(P, t, inst) ----
def test_one_wave_kernel_on_a_coupled_system(emu, oracle):
    """axes that are coupled through A: the lanes of the solver give every instance up, the generic one-wave kernel (lmpc_fused.hpp) evaluates
    the costs with the instance's weights"""
    from copra_amd import workloads
    b = 8
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=29)
    wl["A"][:, 3, 4] = 0.05
    wl["A"][:, 1, 5] = -0.02
    ws, group = W.indexed_weights(wl, b)
    re = _solve(emu, wl, ws)
    assert max(re["lane_pass_finished"], 0) == 0
    W.assert_matches(re, W.oracle_grouped(oracle, wl, ws, group), skip=0)


def test_initial_state_lmpc(emu, oracle):
    pb = F.bounded_system("trajectory", N=12)
    b = 6
    rng = np.random.default_rng(3)
    x0 = np.tile(pb["x0"], (b, 1))
    x0[:, 1] += rng.uniform(-0.5, 0.5, b)
    A, B, d = np.tile(pb["A"], (b, 1, 1)), np.tile(pb["B"], (b, 1, 1)), np.tile(pb["d"], (b, 1))
    ist = dict(R=10.0 * np.eye(2), r=np.array([0.1, -0.2]), x0lb=x0 - 0.05, x0ub=x0 + 0.05)
    wl = dict(A=A, B=B, d=d, x0=x0, N=12, costs=pb["costs"], cstrs=pb["cstrs"])
    ws, _ = W.indexed_weights(wl, b)
    re = _solve(emu, wl, ws, initial_state=ist)
    for k in range(b):
        costs = [dict(c, weights=w[k]) for c, w in zip(pb["costs"], ws)]
        ro = oracle.lmpc_solve(A[k], B[k], d[k], x0[k], 12, costs, pb["cstrs"], initial_state=dict(R=ist["R"], r=ist["r"], x0lb=x0[k] - 0.05, x0ub=x0[k] + 0.05))
        assert re["status"][k] == ro["status"] == 0 and tuple(re["iter"][k]) == tuple(ro["iter"])
        assert W.rel_inst(re["control"][k][None], ro["control"][None]) <= W.RTOL and W.rel_inst(re["x0_opt"][k][None], ro["x0_opt"][None]) <= W.RTOL


@pytest.mark.parametrize("initial_state", [False, True])
def test_workgroup_kernel(emu, oracle, initial_state):
    """N = 70: the workgroup-per-instance body (lmpc_large.hpp), as LMPC and as InitialStateLMPC; three instances walk through one workgroup"""
    pb = F.bounded_system("trajectory", N=70)
    b = 3
    x0 = np.tile(pb["x0"], (b, 1))
    x0[:, 1] += np.array([0.0, 0.2, -0.3])
    A, B, d = np.tile(pb["A"], (b, 1, 1)), np.tile(pb["B"], (b, 1, 1)), np.tile(pb["d"], (b, 1))
    ist = dict(R=10.0 * np.eye(2), r=np.array([0.1, -0.2]), x0lb=x0 - 0.05, x0ub=x0 + 0.05) if initial_state else None
    wl = dict(A=A, B=B, d=d, x0=x0, N=70, costs=pb["costs"], cstrs=pb["cstrs"])
    ws, _ = W.indexed_weights(wl, b)
    re = _solve(emu, wl, ws, initial_state=ist)
    for k in range(b):
        costs = [dict(c, weights=w[k]) for c, w in zip(pb["costs"], ws)]
        isk = dict(R=ist["R"], r=ist["r"], x0lb=x0[k] - 0.05, x0ub=x0[k] + 0.05) if initial_state else None
        ro = oracle.lmpc_solve(A[k], B[k], d[k], x0[k], 70, costs, pb["cstrs"], initial_state=isk)
        assert re["status"][k] == ro["status"] == 0 and tuple(re["iter"][k]) == tuple(ro["iter"])
        assert W.rel_inst(re["control"][k][None], ro["control"][None]) <= W.RTOL and W.rel_inst(re["trajectory"][k][None], ro["trajectory"][None]) <= W.RTOL
