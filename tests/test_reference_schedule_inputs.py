"""The inputs of tests/test_reference_schedule_gpu.py, checked where no GPU is needed: that test asserts statuses that are ALL ZERO at every tick
-- a condition on its inputs -- and that moving the window matters.  Here the oracle alone runs the same closed loops (same controllers, signals,
states, noise; tests/tracking_cases.py): it must solve every instance at every tick, and at the last tick its first control with the moved
window must differ from the one with the frozen window of tick 0 by more than 100 RTOL on at least half of the instances."""
import numpy as np
import pytest

import tracking_cases as tc


@pytest.mark.parametrize("per_instance", [False, True])
@pytest.mark.parametrize("shared_model", [False, True])
def test_oracle_tracks_every_instance_and_the_window_matters(oracle, per_instance, shared_model):
    wl, signals = tc.tracking_workload(shared_model=shared_model)
    N = wl["N"]
    groups = tc.group_of(tc.BATCH, per_instance)
    w_seq = tc.position_noise(tc.TICKS, tc.BATCH, tc.NX, 3, seed=21)
    xs, us, ss = tc.oracle_closed_loop(oracle, wl, signals, groups, w_seq, N + 1)
    assert (ss == 0).all()
    last = tc.TICKS - 1
    share = tc.moved_share(oracle, wl, xs[last], groups, [tc.window(s, last, N + 1) for s in signals], [tc.window(s, 0, N + 1) for s in signals], tc.NU)
    print("tracking, per instance %d, shared model %d: the moved window changes the first control of %.0f %% of the instances" % (per_instance, shared_model, 100 * share))
    assert share >= 0.5
    if per_instance:  # the four signals are distinct: so are the windows of every tick
        for t in range(tc.TICKS):
            wins = [tc.window(s, t, N + 1) for s in signals]
            assert all(not np.array_equal(wins[i], wins[j]) for i in range(4) for j in range(i))


def test_oracle_solves_the_integrators_with_a_moving_goal(oracle):
    wl, signals = tc.integrator_workload()
    N = wl["N"]
    groups = np.arange(tc.BATCH) % 2
    w_seq = tc.position_noise(tc.TICKS, tc.BATCH, 2, 1, seed=22)
    xs, us, ss = tc.oracle_closed_loop(oracle, wl, signals, groups, w_seq, 1, offset=N)
    assert (ss == 0).all()
    last = tc.TICKS - 1
    share = tc.moved_share(oracle, wl, xs[last], groups, [tc.window(s, last + N, 1) for s in signals], [tc.window(s, N, 1) for s in signals], 1)
    print("integrators: the moved goal changes the first control of %.0f %% of the instances" % (100 * share))
    assert share >= 0.5
