"""The inputs of tests/test_limit_schedule_gpu.py, checked where no GPU is needed: that test asserts statuses that are ALL ZERO at every tick and that
moving the limits matters -- conditions on its inputs.  Here the oracle alone runs the same closed loops (same controllers, signals, states, noise
seeds; tests/limit_cases.py): it must solve every instance at every tick; at the last tick its first control with the moved windows must differ from
the one with the frozen windows of tick 0 by more than 100 RTOL on at least half of the instances; a scheduled limit must be active (within 1e-9 of
its bound somewhere on the horizon) for at least 30 % of the instances; and preview on / off must give different first controls on at least 10 % of
the instances at some tick, or the flag would go untested."""
import numpy as np
import pytest

import limit_cases as lc
import tracking_cases as tc

# (workload, which limits move, noise seed): the closed loops of the GPU tests
LOOPS = [("com", ("v", "bounds"), 31), ("com", ("v",), 31), ("com", ("bounds",), 31), ("coupled", ("v", "bounds"), 32), ("integrator", ("bounds",), 33)]


def _workload(name):
    return lc.integrator_limits() if name == "integrator" else lc.com_limits(coupled=name == "coupled")


@pytest.fixture(scope="module")
def loops(oracle):
    """every loop once, shared by the tests below: (workload, use, per_instance, preview) -> (wl, sig, groups, x_hist, u_hist, status_hist, last solve)"""
    out = {}
    for name, use, seed in LOOPS:
        wl, sig = _workload(name)
        for per in (False, True):
            groups = lc.group_of(lc.BATCH, per)
            for preview in (True, False):
                out[(name, use, per, preview)] = (wl, sig, groups) + lc.oracle_closed_loop(oracle, wl, sig, groups, lc.noise(wl, seed), preview, use)
    return out


def test_oracle_solves_every_instance_at_every_tick(loops):
    for key, (wl, sig, groups, xs, us, ss, last) in loops.items():
        assert (ss == 0).all(), (key, [(t, int((ss[t] != 0).sum())) for t in range(lc.TICKS) if (ss[t] != 0).any()])


def test_moved_windows_matter_and_limits_are_active(oracle, loops):
    last = lc.TICKS - 1
    for (name, use, per, preview), (wl, sig, groups, xs, us, ss, ref) in loops.items():
        if use == ("v",) and not preview:
            continue  # (without preview the constraint schedule runs together with the bounds only: limit_cases.V_LIMITS says why)
        nu = wl["B"].shape[2]
        moved, frozen = lc.windows_at(wl, sig, last, preview, use), lc.windows_at(wl, sig, 0, preview, use)
        share = lc.moved_share(oracle, wl, xs[last], groups, moved, frozen, nu)
        active = lc.active_share(wl, ref, moved, groups)
        print("%s %s per instance %d preview %d: moved windows change the first control of %.0f %%, a scheduled limit is active for %.0f %%"
              % (name, "+".join(use), per, preview, 100 * share, 100 * active))
        assert share >= 0.5, (name, use, per, preview)
        assert active >= 0.3, (name, use, per, preview)


@pytest.mark.parametrize("name,use", [("com", ("v",)), ("coupled", ("v", "bounds")), ("integrator", ("bounds",))])
def test_the_preview_flag_matters(loops, name, use):
    for per in (False, True):
        on, off = loops[(name, use, per, True)][4], loops[(name, use, per, False)][4]
        share = max(float((tc.rel(on[t], off[t]).max(axis=1) > 100 * lc.RTOL).mean()) for t in range(lc.TICKS))
        print("%s %s per instance %d: preview on / off differ on up to %.0f %% of the instances" % (name, "+".join(use), per, 100 * share))
        assert share >= 0.1, (name, per)


def test_per_instance_signals_are_distinct():
    for wl, sig in (lc.com_limits(), lc.integrator_limits()):
        for key in ("v", "v_mild", "up"):
            if sig[key] is not None:
                assert all(not np.array_equal(sig[key][i], sig[key][j]) for i in range(lc.GROUPS) for j in range(i)), key
                assert (np.diff(sig[key], axis=1) <= 0).all()  # tightens monotonically, then holds
        assert sig["up"].shape[1] == lc.TICKS + 12 < lc.TICKS + wl["N"] + 1  # (the held tail is inside the horizon of the eight ticks)
