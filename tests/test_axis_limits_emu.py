"""Per-instance limits (copra_batch_set_constraint_rhs, copra_batch_set_control_bounds) on every shape of the (instance, axis)-per-lane solver, on the
CPU: the kernel bodies through the emulator (tests/emu) against the oracle run instance by instance with that instance's own limits.

Only the solver's builds that keep their tables in registers (CT) read an instance's own limits (lmpc_axis.hpp); the others read the
controller's.  front_end.hpp (axis_solver_covers) therefore keeps the solver with limits set only where BOTH its launches are CT builds; every
other controller runs the lane pass and the tiers.  Before that rule asked for both builds, the solver returned the optimum for the
controller-wide limits with status 0 on every other shape: of the cases below com_n21, jerk3_n20, jerk3_n14_amax, jerk2_n9_amax, kinematic3_n20
and kinematic2_n29 (and the variants of jerk3_n20 that tighten a limit) fail on that rule.

The cases and the conditions on their inputs: tests/axis_limit_cases.py."""
import numpy as np
import pytest

import axis_limit_cases as AC
import random_controllers as RC

BATCH = 40


@pytest.fixture(scope="module")
def emu():
    import pyemu
    pyemu.lib()
    return pyemu


def _rel(a, b):
    return np.nanmax(np.abs(a - b) / (1.0 + np.abs(b)))  # (tests/test_emu_kernels.py::_rel)


def _against(re, ref, what):
    """statuses equal; where the oracle solved: both iteration counters equal, U and X within 1e-8 (the bar of test_emu_kernels.py::_axis_case)"""
    assert (re["status"] == ref["status"]).all(), (what, np.nonzero(re["status"] != ref["status"])[0])
    ok = ref["status"] == 0
    assert (re["iter"][ok] == ref["iter"][ok]).all(), (what, np.nonzero((re["iter"] != ref["iter"]).any(axis=1) & ok)[0])
    eu, ex = _rel(re["control"][ok], ref["control"][ok]), _rel(re["trajectory"][ok], ref["trajectory"][ok])
    assert eu <= 1e-8 and ex <= 1e-8, (what, eu, ex)


def _ran_with_limits(emu, covers):
    """what ran with limits set: the solver with both builds CT, or not the solver"""
    run = emu.last_axis_run()
    if run is None:
        assert not covers
        return
    assert covers and run["first"][6] and run["second"][6], run


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_case_against_the_oracle(emu, oracle, name):
    case = AC.CASES[name]
    wl = AC.controller(name, BATCH)
    lim = AC.draw_case_limits(name, wl)
    args = (wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], wl["costs"], wl["cstrs"])
    # without limits: the pair of builds the case is meant to hit
    plain = emu.lmpc_solve(*args)
    run = emu.last_axis_run()
    assert run is not None and (AC.strip(run["first"]), AC.strip(run["second"])) == case["pair"], (name, run)
    _against(plain, AC.oracle_by_instance(oracle, wl, None), name + " without limits")
    # with them
    ref = AC.oracle_by_instance(oracle, wl, lim)
    AC.check_inputs(name, wl, lim, ref)
    re = emu.lmpc_solve(*args, row_rhs=lim["row_rhs"], bounds=AC.bounds_arg(lim))
    _ran_with_limits(emu, case.get("axis", False))
    assert (emu.last_axis_run() is not None) == (case["pair"][0][4] and case["pair"][1][4])
    _against(re, ref, name)
    if case.get("change"):  # (the oracle's answers of instances 5 and 9 depend on the one limit that changes: the case tests what it says)
        flat = AC.draw_case_limits(name, wl)
        flat["hi"][5], flat["rhs"][9] = flat["hi"][5].max(), flat["rhs"][9].max()
        other = AC.oracle_by_instance(oracle, wl, flat)
        assert ref["status"][5] == 0 and ref["status"][9] == 0
        assert _rel(other["control"][5], ref["control"][5]) > 1e-6 and _rel(other["control"][9], ref["control"][9]) > 1e-6


# ---- the rule, swept over every shape and every kind of table the solver has builds for ----

def _shapes(emu):
    """every (nx, nu, N) the solver has builds for (axis_solver_nmax) at N = 4, nmax - 1 and nmax of each of its horizon classes"""
    out = []
    for nu in (1, 2, 3, 4):
        for nxa in (1, 2, 3, 4):
            for N in range(1, 34):
                b = emu.axis_build(nxa * nu, nu, N, False, 2, False, False, False)
                if b is not None and (N == 4 or N in (b[3] - 1, b[3])):
                    out.append((nxa * nu, nu, N))
    return out


def _shaped_controller(nx, nu, N, axis_const, rpa, stage_refs, batch=3):
    """a controller of the shape whose plan has these fields: the state limit as one row per axis and step; rpa 2: the lower limit as rows as
    well; not axis_const: control bounds that tighten along the horizon; stage_refs: a reference trajectory"""
    from copra_amd import workloads
    from controller_cases import planar_integrator
    nxa = nx // nu
    if nxa == 1:
        wl = workloads.kinematic_preview(batch, nu=nu, N=N)
    elif nxa == 3:
        wl = workloads.jerk_preview(batch, nu=nu, N=N)
    else:
        wl = workloads.com_preview(batch, N=N) if nu == 3 else planar_integrator(batch, N)
    up = np.asarray(wl["cstrs"][0]["upper"], dtype=float)
    sel = np.nonzero(np.isfinite(up))[0]
    E, f = np.eye(nx)[sel], up[sel]
    cstrs = [dict(kind="trajectory", E=E, f=f, ineq=True)]
    if rpa == 2:
        cstrs.append(dict(kind="trajectory", E=-E, f=f + 1.0, ineq=True))
    cb = wl["cstrs"][1]
    if not axis_const:
        ramp = np.repeat(np.linspace(1.0, 0.7, N), nu)
        cb = dict(kind="control_bound", lower=np.tile(cb["lower"], N) * ramp, upper=np.tile(cb["upper"], N) * ramp)
    cstrs.append(cb)
    costs = list(wl["costs"])
    if stage_refs:
        p = np.asarray(costs[0]["p"], dtype=float)[None, :] * np.linspace(0.5, 1.0, N + 1)[:, None]
        costs[0] = dict(kind="trajectory", M=np.kron(np.eye(N + 1), np.eye(nx)), p=p.reshape(-1), weights=np.tile(costs[0]["weights"], N + 1))
    return dict(wl, costs=costs, cstrs=cstrs), sel.size * (N + 1) * rpa


def test_the_rule_on_every_shape_and_table_kind(emu):
    """axis_solver_covers with per-instance limits is true exactly where the solver covers the controller without them and both builds it
    picks -- the first launch's and the second chance's -- exist and are CT; without limits its answer is what it was: the first launch has a
    build (reference trajectories: that also fit the lane's array)"""
    shapes = _shapes(emu)
    assert {(s[0] // s[1], s[1]) for s in shapes} == {(1, 2), (1, 3), (2, 2), (2, 3), (3, 2), (3, 3)} and len(shapes) >= 20
    kept = lost = 0
    for nx, nu, N in shapes:
        for axis_const in (False, True):
            for rpa in (1, 2):
                for stage_refs in (False, True):
                    what = (nx, nu, N, axis_const, rpa, stage_refs)
                    first = emu.axis_build(nx, nu, N, axis_const, rpa, stage_refs, False, False)
                    second = emu.axis_build(nx, nu, N, axis_const, rpa, stage_refs, False, True)
                    both_ct = first is not None and second is not None and first[6] and second[6]
                    assert first is not None and second is not None, what  # (every shape has a build of each launch for every kind of table)
                    wl, mgen = _shaped_controller(nx, nu, N, axis_const, rpa, stage_refs)
                    b = wl["x0"].shape[0]
                    fe = lambda **kw: emu.front_end(wl["A"], wl["B"], N, wl["costs"], wl["cstrs"], batch=b, **kw)["axis"]
                    plain = fe()
                    assert plain or stage_refs, what
                    if plain:  # the plan has the fields the controller was built for: a solve runs the builds picked for them
                        emu.lmpc_solve(wl["A"], wl["B"], wl["d"], wl["x0"], N, wl["costs"], wl["cstrs"])
                        run = emu.last_axis_run()
                        assert run is None or (run["first"], run["second"]) == (first, second), (what, run)
                        assert run is not None or nx == 2 * nu, what  # (chains of two states: the emulator runs the solver where the pass could run)
                    rhs, lo, hi = np.ones((b, mgen)), -np.ones((b, nu * N)), np.ones((b, nu * N))
                    for kw in (dict(row_rhs=rhs, bounds=(lo, hi)), dict(row_rhs=rhs), dict(bounds=(lo, hi))):
                        assert fe(**kw) == (plain and both_ct), (what, sorted(kw))
                    assert not fe(bounds=(lo, None)) and not fe(bounds=(None, hi)), what
                    # (every shape with a CT build of the second chance has CT builds of the first launch for the same rows: of the rule's two halves
                    #  only the second chance's decides today.  A build list that breaks this needs a case of its own in tests/axis_limit_cases.py)
                    assert first[6] or not second[6], what
                    kept += int(plain and both_ct)
                    lost += int(plain and not both_ct)
    assert kept >= 8 and lost >= 100, (kept, lost)  # (CT pairs: chains of two states at N <= 20, or two axes, with the same tables at every step)


# ---- random controllers on the solver's shapes ----

def _random_controller(kind, seed):
    make = dict(chain1=RC.make_chain1, chain3=RC.make_chain3, integrator=RC.make_integrator)[kind]
    s = seed
    while True:  # (the solver needs two axes: the next seed with them)
        c = make(s, 24)
        if c["nu"] >= 2:
            return c
        s += 1000


@pytest.mark.parametrize("kind", ["chain1", "chain3", "integrator"])
def test_random_controllers_with_limits(emu, oracle, kind):
    """12 random controllers of each of the solver's families of shapes (tests/random_controllers.py) with the limits draw_limits gives every
    instance, against the oracle instance by instance; what ran is the solver on CT builds or not the solver.  Over the 12 controllers the
    inputs meet the conditions of tests/axis_limit_cases.py: 3/4 of the instances solved, 30 % of those in two or more iterations"""
    solved = total = busy = ran_axis = nlimited = 0
    for seed in range(12):
        c = _random_controller(kind, seed)
        lim = RC.draw_limits(c, seed)
        b = c["x0"].shape[0]
        re = emu.lmpc_solve(c["A"], c["B"], c["d"], c["x0"], c["N"], c["costs"], c["cstrs"], row_rhs=lim["row_rhs"], bounds=lim["bounds"])
        run = emu.last_axis_run()
        limited = bool(lim["rhs"]) or lim["bounds"] is not None
        nlimited += int(limited)
        assert not limited or run is None or (run["first"][6] and run["second"][6]), (kind, seed, run)
        ran_axis += int(run is not None)
        for k in range(b):
            ro = oracle.lmpc_solve(c["A"][k], c["B"][k], c["d"][k], c["x0"][k], c["N"], c["costs"], RC.instance_cstrs(c, lim, k))
            what = (kind, seed, c["forms"], k)
            assert re["status"][k] == ro["status"], what
            total += 1
            if ro["status"] == 0:
                solved += 1
                busy += int(ro["iter"][0] >= 2)
                assert tuple(re["iter"][k]) == tuple(ro["iter"]), what
                assert _rel(re["control"][k], ro["control"]) <= 1e-8 and _rel(re["trajectory"][k], ro["trajectory"]) <= 1e-8, what
    assert 4 * solved >= 3 * total and busy >= 0.3 * solved and nlimited >= 10, (kind, solved, total, busy, nlimited)  # (a controller with a state bound alone has no limit to set)
    print("%s: %d of %d solved, %d in two or more iterations, %d of 12 controllers on the solver" % (kind, solved, total, busy, ran_axis))
