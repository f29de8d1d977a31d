"""Per-instance cost weights (copra_batch_set_cost_weights, BatchLMPC.set_cost_weights) on the GPU, against the CPU oracle run with each
instance's own weights.  Full batches draw their weights from K = 64 distinct vectors, so that one oracle batch per group checks them all.

At the headline's shape the (instance, axis)-per-lane solver runs its builds that rebuild their tables from each instance's weights
(lmpc_axis.hpp, WTS).  Elsewhere the kernels that hold the creation weights in plan tables are routed away (include/copra_hip.h): the other
shapes of that solver, the one-instance-per-lane pass and the Riccati-factor tier give way to the generic one-wave kernels; the Riccati
interior-point solver and the shared-model mode refuse.  Every test asserts which of the two happened."""
import os
import subprocess

import numpy as np
import pytest

from copra_amd._capi import OPTIONS

import cost_weights_cases as W

pytestmark = pytest.mark.gpu

RTOL = W.RTOL
ABS_FLOOR = W.ABS_FLOOR
K = W.K
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b, floor=ABS_FLOOR):
    return np.nanmax(np.abs(a - b) / np.maximum(np.abs(b), floor))


def _engine(wl, batch, **kw):
    from copra_amd import BatchLMPC
    nx, nu = wl["B"].shape[1], wl["B"].shape[2]
    eng = BatchLMPC(nx, nu, wl["N"], batch, wl["costs"], wl["cstrs"], **kw)
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    return eng


# (inputs and measures shared with the CPU tests of the same paths: tests/cost_weights_cases.py)
_grouped_weights = W.grouped_weights
_oracle_grouped = W.oracle_grouped
_rel_inst = W.rel_inst


def _assert_matches(res, ref):
    assert np.array_equal(res["status"], ref["status"])
    assert np.array_equal(res["iter"], ref["iter"])
    ok = ref["status"] == 0
    assert ok.any()
    assert _rel_inst(res["control"][ok], ref["control"][ok]) <= RTOL
    assert _rel_inst(res["trajectory"][ok], ref["trajectory"][ok]) <= RTOL
    print("entry-wise (floor 1e-3): U %.2e, X %.2e" % (_rel(res["control"][ok], ref["control"][ok]), _rel(res["trajectory"][ok], ref["trajectory"][ok])))


def _solve_with_weights(oracle, wl, batch, seed=5, **kw):
    eng = _engine(wl, batch, **kw)
    ws, group = _grouped_weights(wl, batch, seed)
    for t, w in enumerate(ws):
        eng.set_cost_weights(t, w)
    eng.solve()
    res = eng.results()
    _assert_matches(res, _oracle_grouped(oracle, wl, ws, group))
    return eng, res


def test_condensed_qp_has_the_instance_weights(oracle):
    """dump_qp of several instances, the first and the last among them: Q and c as the oracle builds them with that instance's weights"""
    from copra_amd import workloads
    b = 256
    wl = workloads.com_preview(b)
    eng = _engine(wl, b)
    ws, _ = _grouped_weights(wl, b, 1)
    for t, w in enumerate(ws):
        eng.set_cost_weights(t, w)
    for k in (0, 1, 77, 200, b - 1):
        qp = eng.dump_qp(k)
        costs = [dict(c, weights=w[k]) for c, w in zip(wl["costs"], ws)]
        ref = oracle.lmpc_build(wl["A"][k], wl["B"][k], wl["d"][k], wl["x0"][k], wl["N"], costs, wl["cstrs"])
        assert np.abs(qp["Q"] - ref["Q"]).max() <= 1e-12 * np.abs(ref["Q"]).max()
        assert np.abs(qp["c"] - ref["c"]).max() <= 1e-12 * max(np.abs(ref["c"]).max(), 1e-300)


def test_headline_batch_with_instance_weights(oracle):
    """the headline shape at 65 536 instances, log-uniform weights on both costs: the (instance, axis)-per-lane solver's weight-reading build
    runs; every instance matches the oracle"""
    from copra_amd import workloads
    b = 65536
    wl = workloads.com_preview(b)
    eng, _ = _solve_with_weights(oracle, wl, b)
    assert eng.axis_solver_ran()


def test_tight_workload_with_instance_weights(oracle):
    """a tight workload: the (instance, axis)-per-lane solver and its second chance finish part of the batch, the first tier the rest"""
    from copra_amd import workloads
    b = 8192
    wl = workloads.com_preview(b, v_max=0.25)
    eng, _ = _solve_with_weights(oracle, wl, b, seed=7)
    ran, finished = eng.lane_pass_info()
    assert eng.axis_solver_ran() and 0 < finished < b
    eng.solve()  # (a second solve, after the engine adapted its layouts to the workload)
    ws, group = _grouped_weights(wl, b, 7)
    _assert_matches(eng.results(), _oracle_grouped(oracle, wl, ws, group))


@pytest.mark.parametrize("option", ["no_axis_solver", "no_ric"])
def test_pinned_tiers_with_instance_weights(oracle, monkeypatch, option):
    from copra_amd import workloads
    monkeypatch.setitem(OPTIONS, option, 1)
    b = 4096
    wl = workloads.com_preview(b)
    eng, _ = _solve_with_weights(oracle, wl, b, seed=11)
    assert eng.axis_solver_ran() == (option == "no_ric")  # (no_ric pins the tier behind the solver, not the solver)


def test_packed_kernels_with_instance_weights(oracle):
    """a small batch of a small problem: several instances share a wavefront"""
    from copra_amd import workloads
    b = 203
    wl = workloads.double_integrator(b, N=16)
    eng, _ = _solve_with_weights(oracle, wl, b, seed=13)
    assert eng.lanes_per_instance() == 16


def test_workgroup_kernel_with_instance_weights(oracle):
    """N = 70 (210 variables): the workgroup-per-instance Goldfarb-Idnani kernel -- under COPRA_SOLVER_DEFAULT, not the interior-point one"""
    from copra_amd import workloads
    b = 256
    wl = workloads.com_preview(b, N=70)
    eng, _ = _solve_with_weights(oracle, wl, b, seed=17)
    assert eng.lanes_per_instance() > 64
    assert eng.solver() == "quadprog_dense"


@pytest.mark.parametrize("shape", ["jerk", "kinematic", "com21"])
def test_axis_shapes_with_instance_weights(oracle, shape):
    """the other shapes the (instance, axis)-per-lane solver takes: three states per control, one state per control, a horizon of 21 --
    routed to the generic tier while per-instance weights are set"""
    from copra_amd import workloads
    b = 4096
    wl = {"jerk": lambda: workloads.jerk_preview(b), "kinematic": lambda: workloads.kinematic_preview(b),
          "com21": lambda: workloads.com_preview(b, N=21)}[shape]()
    eng, _ = _solve_with_weights(oracle, wl, b, seed=19)
    assert not eng.axis_solver_ran()


def test_initial_state_lmpc_with_instance_weights(oracle):
    """InitialStateLMPC within 64 variables: the one-wave InitialStateLMPC kernel reads the instance's weights"""
    import fixtures as F
    from copra_amd import BatchLMPC
    pb = F.bounded_system("trajectory", N=12)
    b = 128
    rng = np.random.default_rng(3)
    x0 = np.tile(pb["x0"], (b, 1))
    x0[:, 1] += rng.uniform(-0.5, 0.5, b)
    A, B, d = np.tile(pb["A"], (b, 1, 1)), np.tile(pb["B"], (b, 1, 1)), np.tile(pb["d"], (b, 1))
    ist = dict(R=10.0 * np.eye(2), r=np.array([0.1, -0.2]))
    eng = BatchLMPC(2, 1, 12, b, pb["costs"], pb["cstrs"], initial_state=ist)
    eng.set_system(A, B, d, x0)
    eng.set_initial_state_bounds(x0 - 0.05, x0 + 0.05)
    ws = [np.asarray(c["weights"], dtype=np.float64)[None, :] * np.exp(rng.uniform(np.log(0.1), np.log(10.0), (b, len(c["weights"]))))
          for c in pb["costs"]]
    for t, w in enumerate(ws):
        eng.set_cost_weights(t, w)
    eng.solve()
    res = eng.results()
    x0s = eng.initial_state()
    for k in range(0, b, 8):
        costs = [dict(c, weights=w[k]) for c, w in zip(pb["costs"], ws)]
        ro = oracle.lmpc_solve(A[k], B[k], d[k], x0[k], 12, costs, pb["cstrs"],
                               initial_state=dict(R=ist["R"], r=ist["r"], x0lb=x0[k] - 0.05, x0ub=x0[k] + 0.05))
        assert res["status"][k] == ro["status"]
        if ro["status"] == 0:
            assert _rel(res["control"][k], ro["control"]) <= RTOL
            assert _rel(x0s[k], ro["x0_opt"]) <= RTOL


def test_restore_and_in_place_tensor(oracle):
    """None restores the creation weights bit for bit; a device tensor is used in place: changing it changes the next solve"""
    import torch
    from copra_amd import workloads
    b = 4096
    wl = workloads.com_preview(b)
    eng = _engine(wl, b)
    eng.solve()
    eng.solve()  # (the second solve: after the engine's first look at its workload)
    base = eng.results()
    ran_before = eng.axis_solver_ran()
    ws, group = _grouped_weights(wl, b, 23)
    for t, w in enumerate(ws):
        eng.set_cost_weights(t, w)
    eng.solve()
    assert np.abs(eng.results()["control"] - base["control"]).max() > 1e-3  # the weights matter
    for t in range(len(ws)):
        eng.set_cost_weights(t, None)
    eng.solve()
    again = eng.results()
    assert eng.axis_solver_ran() == ran_before  # (the controller has its kernels back)
    for k in ("status", "iter", "control", "trajectory"):
        assert np.array_equal(again[k], base[k], equal_nan=k in ("control", "trajectory"))
    # device tensor, used in place
    wt = torch.tensor(ws[0], dtype=torch.float64, device="cuda")
    eng.set_cost_weights(0, wt)
    eng.solve()
    first = eng.results()
    ref = _oracle_grouped(oracle, wl, [ws[0], np.tile(wl["costs"][1]["weights"], (b, 1))], group)
    _assert_matches(first, ref)
    wt.mul_(4.0)
    torch.cuda.synchronize()
    eng.solve()
    second = eng.results()
    assert np.abs(second["control"] - first["control"]).max() > 1e-6
    ref = _oracle_grouped(oracle, wl, [4.0 * ws[0], np.tile(wl["costs"][1]["weights"], (b, 1))], group)
    _assert_matches(second, ref)
    # one vector for every instance
    eng.set_cost_weights(0, 2.0 * np.asarray(wl["costs"][0]["weights"]))
    eng.solve()
    r1 = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"],
                                 [dict(wl["costs"][0], weights=2.0 * np.asarray(wl["costs"][0]["weights"])), wl["costs"][1]], wl["cstrs"], nthreads=8)
    _assert_matches(eng.results(), r1)


def test_refusals_are_loud():
    from copra_amd import BatchLMPC, workloads
    from copra_amd._capi import CopraUnsupported
    # a forced Riccati interior-point solver: its stage plan holds the creation weights
    b = 64
    wl = workloads.com_preview(b, N=70)
    eng = _engine(wl, b)
    eng.select_solver("riccati_ipm")
    eng.set_cost_weights(0, np.tile(wl["costs"][0]["weights"], (b, 1)))
    with pytest.raises(CopraUnsupported):
        eng.solve()
    eng.set_cost_weights(0, None)
    eng.solve()  # (restored: the interior-point solver runs again)
    assert eng.solver() == "riccati_ipm"
    # a dense (host-evaluated) cost has no weights the kernels read
    wl = workloads.com_preview(b)
    n = 3 * wl["N"]
    dense = dict(kind="dense", Q=1e-3 * np.eye(n), c=np.zeros(n))
    eng = BatchLMPC(6, 3, wl["N"], b, [wl["costs"][0], dense], wl["cstrs"])
    with pytest.raises(CopraUnsupported):
        eng.set_cost_weights(1, np.ones((b, n)))


def test_shared_model_mode_refuses(oracle, monkeypatch):
    """shared-model mode (one factorised model for the batch) holds the creation weights: a solve with per-instance weights is refused.
    A controller whose shared model is written out per instance (the axis solver's case) solves as a batch, correctly."""
    from copra_amd import BatchLMPC, workloads
    from copra_amd._capi import CopraUnsupported
    b = 1024
    wl = workloads.com_preview(b)
    ws, group = _grouped_weights(wl, b, 29)
    for pin in (False, True):
        if pin:
            monkeypatch.setitem(OPTIONS, "no_axis_solver", 1)  # (the shared-model kernels proper)
        eng = BatchLMPC(6, 3, wl["N"], b, wl["costs"], wl["cstrs"])
        eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
        eng.set_x0(wl["x0"])
        if pin:
            with pytest.raises(CopraUnsupported):
                eng.set_cost_weights(0, ws[0])
            continue
        for t, w in enumerate(ws):
            eng.set_cost_weights(t, w)
        eng.solve()
        shared = dict(wl, A=np.tile(wl["A"][0], (b, 1, 1)), B=np.tile(wl["B"][0], (b, 1, 1)), d=np.tile(wl["d"][0], (b, 1)))
        _assert_matches(eng.results(), _oracle_grouped(oracle, shared, ws, group))


def test_pycopra_hands_new_weights_to_its_engine(oracle):
    """pycopra: cost.weights(w2) between solves goes to the engine that exists (no new engine) and the result is the oracle's with w2"""
    import fixtures as F
    from copra_amd import pycopra
    pb = F.bounded_system("trajectory", N=12)
    ps = pycopra.PreviewSystem(pb["A"], pb["B"], pb["d"], pb["x0"], 12)
    ctl = pycopra.LMPC(ps)
    costs = []
    for c in pb["costs"]:
        if c["kind"] == "trajectory":
            obj = pycopra.TrajectoryCost(c["M"], c["p"])
        else:
            obj = pycopra.ControlCost(c["N"], c["p"])
        obj.weights(np.asarray(c["weights"]))
        ctl.add_cost(obj)
        costs.append(obj)
    for k in pb["cstrs"]:  # (kept alive here: a piece only the controller refers to is dropped after the solve, LMPC.cpp:288-307)
        if k["kind"] == "trajectory_bound":
            costs.append(pycopra.TrajectoryBoundConstraint(k["lower"], k["upper"]))
        elif k["kind"] == "control_bound":
            costs.append(pycopra.ControlBoundConstraint(k["lower"], k["upper"]))
        ctl.add_constraint(costs[-1])
    assert ctl.solve()
    eng, builds = ctl._eng, ctl.handle_builds
    w2 = 3.0 * np.asarray(pb["costs"][0]["weights"], dtype=np.float64)
    w2[0] *= 0.1
    costs[0].weights(w2)
    assert ctl.solve()
    assert ctl._eng is eng and ctl.handle_builds == builds
    ref = oracle.lmpc_solve(pb["A"], pb["B"], pb["d"], pb["x0"], 12, [dict(pb["costs"][0], weights=w2)] + list(pb["costs"][1:]), pb["cstrs"])
    assert ref["status"] == 0
    assert _rel(ctl.control(), ref["control"]) <= RTOL
    assert _rel(ctl.trajectory(), ref["trajectory"]) <= RTOL


def test_cpp_mirror_hands_new_weights_to_its_handle(oracle):
    """C++ mirror (tests/cpp/test_weights.cpp): xCost->weights(w2) between solves -- same handle, and the oracle's result with w2"""
    from copra_amd import _capi
    import pyoracle
    _capi.build_library()
    src = os.path.join(ROOT, "tests", "cpp", "test_weights.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "test_weights")
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "copra_amd", "cpp", "include"), src, "-o", exe,
                           "-L", libdir, "-lcopra_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict(l.split(":", 1) for l in r.stdout.splitlines() if ":" in l)
    u = np.array([float(v) for v in lines["U"].split()])
    w2 = np.array([float(v) for v in lines["W2"].split()])
    pb = __import__("fixtures").bounded_system("trajectory", N=12)
    ref = pyoracle.lmpc_solve(pb["A"], pb["B"], pb["d"], pb["x0"], 12, [dict(pb["costs"][0], weights=w2)] + list(pb["costs"][1:]), pb["cstrs"])
    assert ref["status"] == 0
    assert _rel(u, ref["control"]) <= RTOL


# ---- weights next to the other per-instance inputs, on the other builds of the (instance, axis)-per-lane solver, on ragged batches ----
def _set_weights(eng, ws):
    for t, w in enumerate(ws):
        if w is not None:
            eng.set_cost_weights(t, w)


def test_weights_with_per_instance_references(oracle):
    from copra_amd import workloads
    b = 512
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=31)
    ws, group = _grouped_weights(wl, b, 37)
    goals = wl["costs"][0]["p"][None, :] + 0.3 * np.random.default_rng(21).standard_normal((K, 6))
    eng = _engine(wl, b)
    _set_weights(eng, ws)
    eng.set_cost_reference(0, goals[group])
    eng.solve()
    assert eng.axis_solver_ran()
    _assert_matches(eng.results(), _oracle_grouped(oracle, wl, ws, group, costs_of=lambda k, costs: [dict(costs[0], p=goals[group[k]]), costs[1]]))


def test_weights_with_per_instance_limits(oracle):
    """every instance its own velocity limit (a TrajectoryConstraint's right-hand side) and actuator limits, the same along the horizon"""
    from copra_amd import workloads
    b = 512
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=13)
    N = wl["N"]
    vsel = np.hstack([np.zeros((3, 3)), np.eye(3)])
    wl["cstrs"] = [dict(kind="trajectory", E=vsel, f=[0.5] * 3, ineq=True), wl["cstrs"][1]]
    ws, group = _grouped_weights(wl, b, 41)
    rng = np.random.default_rng(33)
    vlim, ulim = (0.5 * rng.uniform(0.6, 1.3, K))[group], (2.5 * rng.uniform(0.6, 1.3, K))[group]
    eng = _engine(wl, b)
    _set_weights(eng, ws)
    eng.set_constraint_rhs(0, np.repeat(vlim[:, None], 3, axis=1))
    eng.set_control_bounds(-np.repeat(ulim[:, None], 3 * N, axis=1), np.repeat(ulim[:, None], 3 * N, axis=1))
    eng.solve()
    assert eng.axis_solver_ran()
    cstrs_of = lambda k: [dict(wl["cstrs"][0], f=[vlim[k]] * 3), dict(kind="control_bound", lower=[-ulim[k]] * 3, upper=[ulim[k]] * 3)]
    _assert_matches(eng.results(), _oracle_grouped(oracle, wl, ws, group, cstrs_of=cstrs_of))


@pytest.mark.parametrize("two_row", [False, True])
def test_weights_with_a_reference_trajectory_cost(oracle, two_row):
    """a reference-trajectory cost whose weights repeat along the horizon: the builds without the horizon compiled in"""
    b = 512
    wl = W.tracking(b, two_row=two_row)
    ws, group = W.tracking_weights(wl, b, 31, groups=K)
    eng = _engine(wl, b)
    _set_weights(eng, ws)
    eng.solve()
    assert eng.axis_solver_ran()
    _assert_matches(eng.results(), _oracle_grouped(oracle, wl, ws, group))


def test_setter_errors_for_a_reference_trajectory_cost():
    """weights of a reference-trajectory cost that differ from step to step: COPRA_ERR_DOMAIN; device weights (not checked): COPRA_ERR_UNSUPPORTED"""
    import torch
    from copra_amd._capi import CopraDomainError, CopraUnsupported
    b = 8
    wl = W.tracking(b)
    ws, _ = W.tracking_weights(wl, b, 31)
    eng = _engine(wl, b)
    eng.set_cost_weights(0, ws[0])  # (repeating: accepted)
    bad = ws[0].copy()
    bad[3, 6 * 5 + 2] *= 1.5
    with pytest.raises(CopraDomainError):
        eng.set_cost_weights(0, bad)
    with pytest.raises(CopraUnsupported):
        eng.set_cost_weights(0, torch.tensor(ws[0], dtype=torch.float64, device="cuda"))
    eng.set_cost_weights(1, torch.tensor(ws[1], dtype=torch.float64, device="cuda"))  # (a per-step cost takes device weights)


@pytest.mark.parametrize("name", ["two_rows", "two_rows_N12", "N12", "axis_major"])
def test_other_weight_builds(oracle, name):
    """two rows per axis and step, N = 12 and axis-major state order (tests/cost_weights_cases.py: axis_cases) at a few waves"""
    from copra_amd import workloads
    b = 700
    wl = {"two_rows": lambda: W.two_rows(b), "two_rows_N12": lambda: W.two_rows(b, N=12),
          "N12": lambda: workloads.com_preview(b, N=12, v_max=0.35, u_max=1.8, seed=23),
          "axis_major": lambda: workloads.axis_major(workloads.com_preview(b, v_max=0.4, u_max=2.0, seed=17))}[name]()
    eng, _ = _solve_with_weights(oracle, wl, b, seed=43)
    ran, finished = eng.lane_pass_info()
    assert eng.axis_solver_ran() and finished > 0


@pytest.mark.parametrize("b", [1, 20, 21, 22, 64, 1000])
def test_ragged_batches_solved_twice(oracle, b):
    """one instance, a wave short of one, a full wave, an instance on the spare lanes, several waves: every instance's weights a function of its
    number, every row another factor -- solved twice (the second solve after the engine's look at its workload)"""
    from copra_amd import workloads
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=7)
    ws, group = W.indexed_weights(wl, b)
    if b > 64:  # (the factors grow with the instance's number: kept within the decade of the other tests)
        ws, group = W.indexed_weights(wl, 64)
        group = np.arange(b) % 64
        ws = [w[group] for w in ws]
    eng = _engine(wl, b)
    _set_weights(eng, ws)
    ref = _oracle_grouped(oracle, wl, ws, group)
    for _ in range(2):
        eng.solve()
        assert eng.axis_solver_ran()
        _assert_matches(eng.results(), ref)


def test_second_launch_alone(oracle):
    """a tight workload at 2048 instances: part of the batch ends in the solver's two launches, the rest in the tier -- on the first solve and
    after the engine adapted"""
    from copra_amd import workloads
    b = 2048
    wl = workloads.com_preview(b, v_max=0.25, u_max=1.2, seed=3)
    ws, group = _grouped_weights(wl, b, 47)
    eng = _engine(wl, b)
    _set_weights(eng, ws)
    ref = _oracle_grouped(oracle, wl, ws, group)
    for _ in range(2):
        eng.solve()
        ran, finished = eng.lane_pass_info()
        assert eng.axis_solver_ran() and 0 < finished < b
        _assert_matches(eng.results(), ref)


def _closed_loop(oracle, eng, wl, ws, group, ticks, w_seq, ref_of_tick=None):
    """rollout(ticks) against an oracle loop from the device's own states, with the same weights (and the reference window of the tick)"""
    hist = eng.rollout(ticks, disturbances=w_seq, x_hist=True, u_hist=True, status_hist=True)
    xh, uh, sh = (hist[k].cpu().numpy() for k in ("x_hist", "u_hist", "status_hist"))
    assert eng.axis_solver_ran()
    for t in range(ticks):
        step = dict(wl, x0=xh[t])
        costs_of = None if ref_of_tick is None else (lambda k, costs: [dict(costs[0], p=ref_of_tick(t, k)), costs[1]])
        ro = _oracle_grouped(oracle, step, ws, group, costs_of=costs_of)
        assert np.array_equal(sh[t], ro["status"]) and (sh[t] == 0).all(), t
        e = _rel_inst(uh[t], ro["control"][:, :3])
        print("tick %d: first control against the oracle, norm-wise %.2e" % (t, e))
        assert e <= RTOL, t
        xn = np.einsum("bij,bj->bi", wl["A"], xh[t]) + np.einsum("bij,bj->bi", wl["B"], uh[t]) + wl["d"] + w_seq[t]
        assert np.abs(xh[t + 1] - xn).max() <= 1e-12


def test_rollout_with_weights(oracle):
    from copra_amd import workloads
    import tracking_cases as tc
    b, ticks = 256, 5
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=51)
    ws, group = _grouped_weights(wl, b, 53, groups=8)
    eng = _engine(wl, b)
    _set_weights(eng, ws)
    _closed_loop(oracle, eng, wl, ws, group, ticks, tc.position_noise(ticks, b, 6, 3, seed=21))


def test_rollout_on_a_reference_schedule_with_weights(oracle):
    """the tracking controller of tests/tracking_cases.py, one schedule per instance, weights that repeat along the horizon"""
    import tracking_cases as tc
    b, ticks = 256, 5
    wl, signals = tc.tracking_workload(batch=b)
    N = wl["N"]
    sig = tc.group_of(b, True)
    ws, wgroup = W.tracking_weights(wl, b, 57, groups=2)
    group = 2 * sig + wgroup  # (instances that share signal and weights)
    eng = _engine(wl, b)
    _set_weights(eng, ws)
    eng.set_reference_schedule(0, np.ascontiguousarray(signals[sig]), tc.NX)
    _closed_loop(oracle, eng, wl, ws, group, ticks, tc.position_noise(ticks, b, 6, 3, seed=22),
                 ref_of_tick=lambda t, k: tc.window(signals[sig[k]], t, N + 1))


# ---- accuracy against the certified optimum ----
def _truth_distances(wl, ws, res, ref, picks):
    import truth
    dev = ora = 0.0
    for k in picks:
        costs = [dict(c, weights=w[k]) for c, w in zip(wl["costs"], ws)]
        t = truth.solve(wl["A"][k], wl["B"][k], wl["d"][k], wl["x0"][k], wl["N"], costs, wl["cstrs"], ref["control"][k])
        dev = max(dev, _rel(res["control"][k], t["control"]), _rel(res["trajectory"][k], t["trajectory"]))
        ora = max(ora, _rel(ref["control"][k], t["control"]), _rel(ref["trajectory"][k], t["trajectory"]))
    return dev, ora


@pytest.mark.parametrize("f0", [1e-4, 1.0, 1e4])
@pytest.mark.parametrize("f1", [1e-4, 1.0, 1e4])
def test_scaled_weights_against_the_certified_optimum(oracle, f0, f1):
    """weights at the creation weights x {1e-4, 1, 1e4} per cost, 64 instances: the device against the extended-precision certified optimum
    (tests/truth.py), entry by entry, next to the oracle's own distance on the same instances.  Bound: 10 x the oracle's distance or RTOL,
    whichever is larger -- the factor covers the cancellation in H0 + (w - w0) c c', whose error grows as eps w0 / w."""
    from copra_amd import workloads
    b = 64
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=61)
    ws = [np.tile(f * np.asarray(c["weights"], dtype=np.float64), (b, 1)) for f, c in zip((f0, f1), wl["costs"])]
    eng = _engine(wl, b)
    _set_weights(eng, ws)
    eng.solve()
    res = eng.results()
    ref = _oracle_grouped(oracle, wl, ws, np.zeros(b, dtype=int))
    assert eng.axis_solver_ran()
    assert np.array_equal(res["status"], ref["status"]) and (ref["status"] == 0).sum() >= b - 1
    dev, ora = _truth_distances(wl, ws, res, ref, np.nonzero(ref["status"] == 0)[0])
    print("weights x (%g, %g): distance from the certified optimum (entry-wise, floor 1e-3): device %.2e | oracle %.2e" % (f0, f1, dev, ora))
    assert dev <= max(10.0 * ora, RTOL), (dev, ora)


def test_zero_instance_weight_on_single_rows(oracle):
    """a zero weight per instance on one row whose creation weight is not zero (w / w0 = 0: the lane takes the row's whole term out of H):
    the oracle's statuses; results where the oracle itself is within RTOL of the certified optimum"""
    from copra_amd import workloads
    b = 64
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=67)
    ws = [np.tile(np.asarray(c["weights"], dtype=np.float64), (b, 1)) for c in wl["costs"]]
    for k in range(b):  # (instance k: row k % 6 of the trajectory cost)
        ws[0][k, k % 6] = 0.0
    group = np.arange(b) % 6
    eng = _engine(wl, b)
    _set_weights(eng, ws)
    eng.solve()
    res = eng.results()
    ref = _oracle_grouped(oracle, wl, ws, group)
    assert eng.axis_solver_ran()
    assert np.array_equal(res["status"], ref["status"])
    compared = 0
    for k in np.nonzero(ref["status"] == 0)[0]:
        dev, ora = _truth_distances(wl, ws, res, ref, [k])
        if ora <= RTOL:
            compared += 1
            assert _rel(res["control"][k], ref["control"][k]) <= RTOL and _rel(res["trajectory"][k], ref["trajectory"][k]) <= RTOL, (k, dev, ora)
    print("zero instance weights: %d of %d instances compared (oracle within RTOL of the certified optimum)" % (compared, b))
    assert compared >= b // 2
