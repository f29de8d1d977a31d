"""The forward scan of the (instance, axis)-per-lane solver (lmpc_axis.hpp) carries its row-norm recurrences (G <- A G, and nrow or W) only as far
as the last stage at which some lane of the wave had a violated row: they are caught up, stage by stage, where the next violated row shows, and
a stage's rows and bounds sit behind one wave-uniform test.  Neither may move a bit: the emulated body against the oracle (the measure and the
bounds of tests/test_axis_trip_bounds.py) and against the arrays recorded from the body before the change (tests/golden/axis_scan_quiet.npz,
tests/golden/gen_axis_scan_quiet.py).  Every case asserts, on the oracle's unconstrained roll-out of its first wave, that its violated rows lie
where the case says (gen_axis_scan_quiet.premise).  (The same cases on the device: tests/test_axis_scan_quiet_gpu.py.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_axis_scan_quiet as G  # noqa: E402

CASES = G.cases()

# the builds a case is meant to run, as pyemu.axis_build reports them: (NXA, NMAX, EXACT, CT, RPA) of the first launch
BUILDS = {
    "terminal_only": (2, 20, True, True, 1),
    "row_and_bound": (2, 20, True, True, 1),
    "lds_isolated": (2, 20, False, False, 2),
    "second_slot_only": (2, 20, True, True, 2),
    "horizon_7": (2, 20, False, True, 1),
    "jerk_gap": (3, 20, False, True, 1),
    "kinematic_gap": (1, 20, False, False, 2),
}


@pytest.fixture(scope="module")
def golden():
    return np.load(G.PATH)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3))) if a.size else 0.0  # (tests/test_axis_trip_bounds.py::_rel)


def _oracle(oracle, wl):
    return oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], wl["costs"], wl["cstrs"], nthreads=4)


@pytest.mark.parametrize("name", G.EMU_CASES)
def test_scan_matches_the_oracle_and_the_recorded_bits(oracle, golden, name):
    wl = CASES[name]
    assert 42 <= wl["x0"].shape[0] <= 85
    ks = G.premise(name, G.rollout_pattern(oracle, wl), wl["N"])
    re = G.run(wl)
    run = re["axis_run"]
    assert run is not None, name
    first = run["first"]
    assert (first[1], first[3], first[5], first[6], first[7]) == BUILDS[name], (name, run)
    ro = _oracle(oracle, wl)
    ok = ro["status"] == 0
    eu, ex = _rel(re["control"][ok], ro["control"][ok]), _rel(re["trajectory"][ok], ro["trajectory"][ok])
    print("%s: rows violated at steps %r of the first wave's roll-out; %d of %d solved, %d finished by the solver, U %.2e and X %.2e from the oracle"
          % (name, ks, ok.sum(), ok.size, re["lane_pass_finished"], eu, ex))
    assert ok.sum() >= len(ok) - 1
    assert (re["status"] == ro["status"]).all()
    assert (re["iter"][ok] == ro["iter"][ok]).all()
    assert eu <= 1e-8 and ex <= 1e-8
    assert re["lane_pass_finished"] == int(golden[name + "/lane_pass_finished"]) > 0  # (the solver's lanes, not the tier, made these results)
    assert re["lane_pass_finished"] >= len(ok) - 3
    for k in G.KEYS:
        assert np.array_equal(re[k], golden[name + "/" + k]), (name, k)
    assert ro["iter"][:, 0].max() >= 3
