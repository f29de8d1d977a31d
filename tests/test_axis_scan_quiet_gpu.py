"""The forward scan of the (instance, axis)-per-lane solver (lmpc_axis.hpp) with its row norms caught up on demand and one wave-uniform test per
stage, compiled for the device: the cases of tests/golden/gen_axis_scan_quiet.py at their own sizes -- violated rows behind long gaps of clean
stages, at the terminal step alone, next to another lane's violated bound, in one row slot alone, on the builds that read their tables from LDS,
on a run-time horizon, on chains of one and three states -- and a batch of 3 x 21 + 1 instances, whose last instance runs on spare lanes.
Against the oracle: statuses and both iteration counters equal, U and X at the bars of tests/test_gpu_parity.py (entry-wise within 1e-6, absolute
floor 1e-3).  Against the arrays recorded from the emulated body before the scan changed (tests/golden/axis_scan_quiet.npz): statuses and counters
equal, U and X within 1e-9 (the compiler contracts multiply-adds on the device: not the same bits) -- the bars of
tests/test_gpu_parity.py::test_axis_trip_bounds_cases_on_the_device.  (The same cases on the CPU: tests/test_axis_scan_quiet_emu.py.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_axis_scan_quiet as G  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = 1e-6
ABS_FLOOR = 1e-3
CASES = G.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(G.PATH)


def _rel(a, b):
    return float(np.nanmax(np.abs(a - b) / np.maximum(np.abs(b), ABS_FLOOR))) if a.size else 0.0  # (tests/test_gpu_parity.py::_rel)


@pytest.mark.parametrize("name", G.EMU_CASES + ("spare_lane",))
def test_scan_on_the_device(oracle, golden, name):
    from copra_amd import BatchLMPC
    wl = CASES[name]
    b, nx, nu = wl["x0"].shape[0], wl["B"].shape[1], wl["B"].shape[2]
    ks = G.premise(name, G.rollout_pattern(oracle, wl), wl["N"])
    eng = BatchLMPC(nx, nu, wl["N"], b, wl["costs"], wl["cstrs"])
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    eng.solve()
    res = eng.results()
    ran, finished = eng.axis_solver_ran(), eng.lane_pass_info()[1]
    eng.close()
    assert ran, name
    ref = oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], wl["costs"], wl["cstrs"], nthreads=8)
    ok = ref["status"] == 0
    eu, ex = _rel(res["control"][ok], ref["control"][ok]), _rel(res["trajectory"][ok], ref["trajectory"][ok])
    gu, gx = _rel(res["control"][ok], golden[name + "/control"][ok]), _rel(res["trajectory"][ok], golden[name + "/trajectory"][ok])
    print("%s: rows violated at steps %r of the first wave's roll-out; %d of %d solved, %d finished by the solver; against the oracle U %.2e, X %.2e; "
          "against the emulated body's recorded arrays U %.2e, X %.2e" % (name, ks, ok.sum(), b, finished, eu, ex, gu, gx))
    assert ok.sum() >= b - 1, name
    assert np.array_equal(res["status"], ref["status"]), name
    assert np.array_equal(res["iter"][ok], ref["iter"][ok]), name
    assert eu <= RTOL and ex <= RTOL, (name, eu, ex)
    assert finished == int(golden[name + "/lane_pass_finished"]) > 0, name  # (the solver's lanes, not the tier, made these results)
    assert np.array_equal(res["status"], golden[name + "/status"]) and np.array_equal(res["iter"][ok], golden[name + "/iter"][ok]), name
    assert gu <= 1e-9 and gx <= 1e-9, (name, gu, gx)
