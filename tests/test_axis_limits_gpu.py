"""Per-instance limits (copra_batch_set_constraint_rhs, copra_batch_set_control_bounds) on every shape of the (instance, axis)-per-lane solver, on the
device: the cases of tests/axis_limit_cases.py at batch 512, every instance against the oracle run with that instance's own limits, at the bars
of tests/test_gpu_parity.py -- equal statuses, U and X entry-wise within 1e-6 with the absolute floor 1e-3, iteration counters equal on all but
1 in 200 solved instances (ties of the most-violated-constraint rule).  The solver keeps a controller with limits set only where both its
launches keep their tables in registers (front_end.hpp): CoM at N = 20 here; the other shapes run the tiers, and used to return the optimum
for the controller-wide limits with status 0.  (The same cases on the CPU: tests/test_axis_limits_emu.py.)"""
import numpy as np
import pytest

import axis_limit_cases as AC

pytestmark = pytest.mark.gpu

BATCH = 512
RTOL = 1e-6
ABS_FLOOR = 1e-3


def _rel(a, b):
    return float(np.nanmax(np.abs(a - b) / np.maximum(np.abs(b), ABS_FLOOR)))  # (tests/test_gpu_parity.py::_rel)


def _against(res, ref, what, quad_of=None):
    """quad_of(k): the oracle's own statements of instance k in binary128 arithmetic -- an instance on which the device is further than RTOL from
    the oracle is held to RTOL of THAT, and the oracle must then be the one that is further than RTOL from it (at most 1 in 100 instances)"""
    assert np.array_equal(res["status"], ref["status"]), (what, np.nonzero(res["status"] != ref["status"])[0][:8])
    ok = ref["status"] == 0
    assert 4 * ok.sum() >= 3 * ok.size, what
    err = np.zeros(ok.size)
    for key in ("control", "trajectory"):
        err[ok] = np.maximum(err[ok], (np.abs(res[key][ok] - ref[key][ok]) / np.maximum(np.abs(ref[key][ok]), ABS_FLOOR)).max(axis=1))
    ndiff = int((res["iter"][ok] != ref["iter"][ok]).any(axis=1).sum())
    print("%s: %d of %d solved, against the oracle %.2e, iteration counters differ on %d" % (what, ok.sum(), ok.size, err.max(), ndiff))
    over = np.nonzero(err > RTOL)[0]
    if quad_of is not None and over.size:
        assert over.size * 100 <= ok.size, (what, over)
        for k in over:
            q = quad_of(k)
            dev = max(_rel(res[key][k], q[key]) for key in ("control", "trajectory"))
            ora = max(_rel(ref[key][k], q[key]) for key in ("control", "trajectory"))
            print("   instance %d: device %.2e and oracle %.2e from the oracle's statements in binary128" % (k, dev, ora))
            assert q["status"] == 0 and dev <= RTOL < ora, (what, k, dev, ora)
    else:
        assert err.max() <= RTOL, (what, err.max(), over[:8])
    assert ndiff * 200 <= ok.sum(), (what, ndiff)


def _engine(wl, batch=BATCH):
    from copra_amd import BatchLMPC
    nx, nu = wl["B"].shape[1], wl["B"].shape[2]
    eng = BatchLMPC(nx, nu, wl["N"], batch, wl["costs"], wl["cstrs"])
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    return eng


def _set_limits(eng, lim):
    if lim["rhs"] is not None:
        eng.set_constraint_rhs(0, lim["rhs"])
    if lim["lo"] is not None:
        eng.set_control_bounds(lim["lo"], lim["hi"])


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_case_against_the_oracle(oracle, name):
    case = AC.CASES[name]
    wl = AC.controller(name, BATCH)
    lim = AC.draw_case_limits(name, wl)
    ref = AC.oracle_by_instance(oracle, wl, lim)
    AC.check_inputs(name, wl, lim, ref)
    eng = _engine(wl)
    _set_limits(eng, lim)
    eng.solve()
    res = eng.results()
    ran = eng.axis_solver_ran()
    eng.close()
    assert ran == case.get("axis", False), name
    _against(res, ref, name)


def _other_limits(name, wl, seed):
    """another draw of the case's limits"""
    keep = AC.CASES[name]["seed"]
    AC.CASES[name]["seed"] = seed
    try:
        return AC.draw_case_limits(name, wl)
    finally:
        AC.CASES[name]["seed"] = keep


@pytest.mark.parametrize("name", ["jerk3_n20", "com_n20"])
def test_one_handle_without_limits_with_limits_and_with_others(oracle, name):
    """one controller through a solve without limits -- on the solver --, with limits, and with other limits: right every time; the solver
    keeps the CoM controller (both builds read an instance's limits) and leaves the jerk-controlled one to the tiers from the first limit on"""
    case = AC.CASES[name]
    wl = AC.controller(name, BATCH)
    eng = _engine(wl)
    eng.solve()
    assert eng.axis_solver_ran()
    _against(eng.results(), AC.oracle_by_instance(oracle, wl, None), name + ", no limits yet")
    first, second = AC.draw_case_limits(name, wl), _other_limits(name, wl, 977)
    assert np.abs(first["rhs"] - second["rhs"]).max() > 1e-2 and np.abs(first["hi"] - second["hi"]).max() > 1e-2
    for lim, what in ((first, "limits"), (second, "other limits")):
        _set_limits(eng, lim)
        eng.solve()
        assert eng.axis_solver_ran() == case.get("axis", False), (name, what)
        _against(eng.results(), AC.oracle_by_instance(oracle, wl, lim), "%s, %s" % (name, what))
    eng.close()


@pytest.mark.parametrize("order", ["model_first", "limits_first"])
def test_shared_model_with_limits(oracle, order):
    """copra_batch_set_shared_system on the jerk-controlled controller -- the model is written out per instance, because the solver would take it
     -- and per-instance limits, set after the model or before it: the tiers solve it, every instance against the oracle on
    the one model with its own limits"""
    name = "jerk3_n20"
    wl = AC.controller(name, BATCH)
    lim = AC.draw_case_limits(name, wl)
    from copra_amd import BatchLMPC
    eng = BatchLMPC(9, 3, wl["N"], BATCH, wl["costs"], wl["cstrs"])
    if order == "limits_first":
        _set_limits(eng, lim)
    eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
    eng.set_x0(wl["x0"])
    if order == "model_first":
        eng.solve()
        assert eng.axis_solver_ran()
        _against(eng.results(), AC.oracle_by_instance(oracle, wl, None, shared=True), "shared model, no limits yet")
        _set_limits(eng, lim)
    eng.solve()
    assert not eng.axis_solver_ran()
    _against(eng.results(), AC.oracle_by_instance(oracle, wl, lim, shared=True), "shared model with limits, " + order)
    eng.close()


def test_the_fleet_example_configuration(oracle):
    """what examples/jerk_fleet.py sets up, at batch 512: the jerk-controlled model with a goal, a velocity limit and a jerk limit per robot --
    one solve, every robot against the oracle.  The oracle itself is 1.4e-6 (entry-wise, floor 1e-3: an entry of 1.4e-4, absolute error 1.4e-9) from
    its own statements run in binary128 arithmetic on robot 82 of this draw, where the kernel bodies on the CPU are 4e-9 from them: such a robot
    is held to 1e-6 of the binary128 run instead (tests/test_gpu_parity.py does the same with its certified optimum)"""
    from copra_amd import BatchLMPC, workloads
    b, nx, nu = BATCH, 9, 3
    wl = workloads.jerk_preview(b, nu=3, N=20, v_max=0.5, j_max=15.0)
    N = wl["N"]
    rng = np.random.default_rng(0)
    Ev = np.hstack([np.zeros((3, 3)), np.eye(3), np.zeros((3, 3))])
    wl["cstrs"] = [dict(kind="trajectory", E=Ev, f=[0.5] * 3, ineq=True), wl["cstrs"][1]]
    eng = BatchLMPC(nx, nu, N, b, wl["costs"], wl["cstrs"])
    goals = np.tile(wl["costs"][0]["p"], (b, 1))
    goals[:, :3] += 0.3 * rng.standard_normal((b, 3))
    eng.set_cost_reference(0, goals)
    rhs = np.repeat((0.5 * rng.uniform(0.7, 1.3, b))[:, None], 3, axis=1)
    eng.set_constraint_rhs(0, rhs)
    jmax = 15.0 * rng.uniform(0.7, 1.3, b)
    lo, hi = -np.repeat(jmax[:, None], nu * N, axis=1), np.repeat(jmax[:, None], nu * N, axis=1)
    eng.set_control_bounds(lo, hi)
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    eng.solve()
    res = eng.results()
    ran = eng.axis_solver_ran()
    eng.close()
    lim = dict(rhs=rhs, lo=lo, hi=hi)
    costs_of = lambda k: [dict(wl["costs"][0], p=goals[k]), wl["costs"][1]]
    ref = AC.oracle_by_instance(oracle, wl, lim, costs_of=costs_of)
    assert not ran
    assert (ref["iter"][ref["status"] == 0, 0] >= 2).mean() >= 0.3  # (the limits matter)
    quad_of = lambda k: oracle.lmpc_solve_quad(wl["A"][k], wl["B"][k], wl["d"][k], wl["x0"][k], N, costs_of(k), AC.instance_cstrs(wl, lim, k))
    _against(res, ref, "the fleet example's configuration", quad_of=quad_of)
