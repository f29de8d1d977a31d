"""The inputs of the per-instance cost-weight tests (tests/test_cost_weights_emu.py, tests/test_cost_weights_gpu.py), checked from the oracle
alone: those tests compare the instances the oracle SOLVED and may leave out one per case at the most -- a condition on their inputs --, and
their tight cases are meant to hold, in one wave, lanes without an active constraint, lanes with fewer than the six a lane of the first launch
has room for, and lanes with six or more (the second launch, the tier)."""
import numpy as np
import pytest

import cost_weights_cases as W

AXIS = W.axis_cases()


def _solved(ro):
    return int((ro["status"] == 0).sum())


@pytest.mark.parametrize("name", sorted(AXIS))
def test_the_oracle_solves_the_axis_cases_with_their_weights(oracle, name):
    wl, _, _, tight = AXIS[name]
    b = len(wl["x0"])
    ws, group = W.grouped_weights(wl, b, 5)
    ro = W.oracle_grouped(oracle, wl, ws, group)
    assert _solved(ro) >= b - 1
    assert ro["iter"][:, 0].max() >= 3  # (the constraints matter)
    if tight:
        q = W.com_axis_counts(wl, ro, 0.25, 1.2)[:21]  # (the first wave: 21 instances x 3 axes)
        print(name, "active constraints per lane of the first wave:", np.bincount(q.ravel()))
        assert (q == 0).any() and ((q > 0) & (q < 6)).any() and (q >= 6).any()


@pytest.mark.parametrize("what", ["references", "limits", "tracking", "tracking_two_rows", "indexed", "second_launch", "zero_rows", "other_builds"])
def test_the_oracle_solves_the_other_workloads(oracle, what):
    from copra_amd import workloads
    if what == "references":
        for b, groups in ((44, None), (512, W.K)):
            wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=31)
            ws, group = W.indexed_weights(wl, b) if groups is None else W.grouped_weights(wl, b, 37)
            goals = wl["costs"][0]["p"][None, :] + 0.3 * np.random.default_rng(21).standard_normal((b if groups is None else W.K, 6))
            pick = (lambda k: goals[k]) if groups is None else (lambda k: goals[group[k]])
            ro = W.oracle_grouped(oracle, wl, ws, group, costs_of=lambda k, costs: [dict(costs[0], p=pick(k)), costs[1]])
            assert _solved(ro) >= b - 1
    elif what == "limits":
        b = 512
        wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=13)
        vsel = np.hstack([np.zeros((3, 3)), np.eye(3)])
        wl["cstrs"] = [dict(kind="trajectory", E=vsel, f=[0.5] * 3, ineq=True), wl["cstrs"][1]]
        ws, group = W.grouped_weights(wl, b, 41)
        rng = np.random.default_rng(33)
        vlim, ulim = (0.5 * rng.uniform(0.6, 1.3, W.K))[group], (2.5 * rng.uniform(0.6, 1.3, W.K))[group]
        cstrs_of = lambda k: [dict(wl["cstrs"][0], f=[vlim[k]] * 3), dict(kind="control_bound", lower=[-ulim[k]] * 3, upper=[ulim[k]] * 3)]
        assert _solved(W.oracle_grouped(oracle, wl, ws, group, cstrs_of=cstrs_of)) >= b - 1
    elif what in ("tracking", "tracking_two_rows"):
        for b, groups in ((43, 8), (512, W.K)):
            wl = W.tracking(b, two_row=what == "tracking_two_rows")
            ws, group = W.tracking_weights(wl, b, 31, groups=groups)
            assert _solved(W.oracle_grouped(oracle, wl, ws, group)) >= b - 1
    elif what == "indexed":
        for b in (1, 20, 21, 22, 64):
            wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=7)
            ws, group = W.indexed_weights(wl, b)
            assert _solved(W.oracle_grouped(oracle, wl, ws, group)) == b
    elif what == "second_launch":
        b = 2048
        wl = workloads.com_preview(b, v_max=0.25, u_max=1.2, seed=3)
        ws, group = W.grouped_weights(wl, b, 47)
        ro = W.oracle_grouped(oracle, wl, ws, group)
        assert _solved(ro) >= b - 1
        q = W.com_axis_counts(wl, ro, 0.25, 1.2).max(axis=1)
        assert (q <= 6).any() and (q > 6).any()  # (instances the first launch finishes, instances it lists)
    elif what == "zero_rows":
        b = 64
        wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=67)
        ws = [np.tile(np.asarray(c["weights"], dtype=np.float64), (b, 1)) for c in wl["costs"]]
        for k in range(b):
            ws[0][k, k % 6] = 0.0
        assert _solved(W.oracle_grouped(oracle, wl, ws, np.arange(b) % 6)) >= b - 1
    else:
        b = 700
        for wl in (W.two_rows(b), W.two_rows(b, N=12), workloads.com_preview(b, N=12, v_max=0.35, u_max=1.8, seed=23),
                   workloads.axis_major(workloads.com_preview(b, v_max=0.4, u_max=2.0, seed=17))):
            ws, group = W.grouped_weights(wl, b, 43)
            assert _solved(W.oracle_grouped(oracle, wl, ws, group)) >= b - 1


@pytest.mark.parametrize("f0", [1e-4, 1.0, 1e4])
@pytest.mark.parametrize("f1", [1e-4, 1.0, 1e4])
def test_the_oracle_solves_the_scaled_weights(oracle, f0, f1):
    from copra_amd import workloads
    b = 64
    wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=61)
    ws = [np.tile(f * np.asarray(c["weights"], dtype=np.float64), (b, 1)) for f, c in zip((f0, f1), wl["costs"])]
    assert _solved(W.oracle_grouped(oracle, wl, ws, np.zeros(b, dtype=int))) >= b - 1


@pytest.mark.parametrize("tracking", [False, True])
def test_the_oracle_solves_every_tick_of_the_closed_loops(oracle, tracking):
    """the rollouts of the GPU tests, run by the oracle alone with the same weights, states and noise: status 0 on every instance at every tick"""
    from copra_amd import workloads
    import tracking_cases as tc
    b, ticks = 256, 5
    if tracking:
        wl, signals = tc.tracking_workload(batch=b)
        sig = tc.group_of(b, True)
        ws, wgroup = W.tracking_weights(wl, b, 57, groups=2)
        group = 2 * sig + wgroup
        w_seq = tc.position_noise(ticks, b, 6, 3, seed=22)
    else:
        wl = workloads.com_preview(b, v_max=0.5, u_max=2.5, seed=51)
        ws, group = W.grouped_weights(wl, b, 53, groups=8)
        w_seq = tc.position_noise(ticks, b, 6, 3, seed=21)
    x = wl["x0"].copy()
    for t in range(ticks):
        costs_of = (lambda k, costs: [dict(costs[0], p=tc.window(signals[sig[k]], t, wl["N"] + 1)), costs[1]]) if tracking else None
        ro = W.oracle_grouped(oracle, dict(wl, x0=x), ws, group, costs_of=costs_of)
        assert (ro["status"] == 0).all(), t
        x = np.einsum("bij,bj->bi", wl["A"], x) + np.einsum("bij,bj->bi", wl["B"], ro["control"][:, :3]) + wl["d"] + w_seq[t]
