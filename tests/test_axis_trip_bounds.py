"""The trips of the (instance, axis)-per-lane solver (lmpc_axis.hpp) bound their small dense algebra -- the Cholesky of S, the two substitutions,
the loops over the slots -- by the wave's largest active set, and their scan looks at the bookkeeping of a candidate only where some lane has
one.  Neither may move a bit: the emulated body, in its normal mode and in the two-slot mode of the tests, against the oracle (the parity measure
of tests/test_emu_kernels.py) and against the arrays recorded from the body before the change (tests/golden/axis_trip_bounds.npz,
tests/golden/gen_axis_trip_bounds.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_axis_trip_bounds as G  # noqa: E402

CASES = G.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(G.PATH)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3))) if a.size else 0.0


def _oracle(oracle, wl):
    return oracle.lmpc_solve_batch(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], wl["costs"], wl["cstrs"], nthreads=4)


def _com_axis_counts(wl, ro, vmax, umax):
    """constraints active at the oracle's solution, per (instance, axis) of the CoM model: what a lane's active set ends with"""
    b, N = len(ro["status"]), wl["N"]
    X = ro["trajectory"].reshape(b, N + 1, 6)
    U = ro["control"].reshape(b, N, 3)
    return (X[:, :, 3:] >= vmax - 1e-9).sum(1) + (np.abs(U) >= umax - 1e-9).sum(1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_trips_match_the_oracle_and_the_recorded_bits(oracle, golden, name):
    wl, two_slot = CASES[name]
    re = G.run(wl, two_slot)
    ro = _oracle(oracle, wl)
    ok = ro["status"] == 0
    assert ok.sum() >= len(ok) - 1
    assert (re["status"] == ro["status"]).all()
    assert (re["iter"][ok] == ro["iter"][ok]).all()
    assert _rel(re["control"][ok], ro["control"][ok]) <= 1e-8 and _rel(re["trajectory"][ok], ro["trajectory"][ok]) <= 1e-8
    assert re["lane_pass_finished"] == int(golden[name + "/lane_pass_finished"]) > 0  # (the solver's lanes, not the tier, made these results)
    for k in G.KEYS:
        assert np.array_equal(re[k], golden[name + "/" + k]), (name, k)
    assert ro["iter"][:, 0].max() >= 3


def test_the_cases_mix_empty_partial_and_full_lanes_in_one_wave(oracle):
    """what the cases are chosen for, checked on the oracle's solutions: the first wave (21 instances x 3 axes) holds lanes without an active
    constraint, lanes with fewer than the wave's largest set and lanes that fill their slots -- two in the two-slot mode, six in the normal one --
    and an axis that outgrows them, whose instance ends in the list"""
    for name, qmax in (("com_v06_two_slot", 2), ("com_v025_two_slot", 2), ("com_v025", 6)):
        wl, two_slot = CASES[name]
        assert two_slot == (qmax == 2)
        vmax, umax = (0.6, 3.0) if "v06" in name else (0.25, 1.2)
        q = _com_axis_counts(wl, _oracle(oracle, wl), vmax, umax)[:21]
        assert (q == 0).any() and ((q > 0) & (q < qmax)).any() and (q == qmax).any(), (name, np.bincount(q.ravel()))
        if name != "com_v06_two_slot":
            assert (q > qmax).any(), (name, np.bincount(q.ravel()))
