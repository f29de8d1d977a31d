"""Cases and recorded results of tests/test_axis_scan_quiet_emu.py and tests/test_axis_scan_quiet_gpu.py: the forward scan of the (instance,
axis)-per-lane solver (lmpc_axis.hpp) advances its row-norm recurrences only where some lane of the wave has a violated row -- caught up stage
by stage from where they stopped -- and looks at a stage's rows and bounds behind ONE wave-uniform test.  The cases put the violated rows where
that can go wrong: behind long gaps of clean stages, at the terminal step alone, next to a violated bound of another lane, in the second row slot
alone, on the builds that read their tables from LDS, on a run-time horizon, on chains of one and three states.

    python tests/golden/gen_axis_scan_quiet.py          writes tests/golden/axis_scan_quiet.npz from the emulator of THIS tree

The arrays in the repository were recorded from the commit BEFORE the scan changed (its recurrences ran at every stage of every scan): the tests
ask for the same bits from the body as it is now.  Run it again only when a change is MEANT to move them.

Every case states its premise on the oracle's UNCONSTRAINED roll-out (rows and bounds lifted: what the solver's first scan looks at) of the
FIRST WAVE -- 64 / nu instances --: premise(name, pattern) raises where a case no longer puts its violated rows where it says."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests", "emu")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(HERE, "axis_scan_quiet.npz")
KEYS = ("control", "trajectory", "status", "iter")

# the isolated steps at which the full-size velocity limit of `lds_isolated` is tight
ISOLATED_STEPS = (2, 9, 15)
# ... and of the full-size position limit of `kinematic_gap`
KINEMATIC_STEPS = (3, 12)


def _vel_rows(nu, nxa):
    """selector of the velocities of a chain model with state i on axis i % nu (the second state of every chain)"""
    E = np.zeros((nu, nu * nxa))
    E[:, nu:2 * nu] = np.eye(nu)
    return E


def cases():
    """name -> workload"""
    from copra_amd import workloads
    out = {}
    # 1. rows violated right behind the start and at the terminal step alone: the recurrences are caught up over the whole horizon at once
    out["terminal_only"] = workloads.com_preview(85, v_max=0.30, u_max=1.5, seed=25)
    # 2. a violated row of one lane and a violated bound of another in the same stage
    out["row_and_bound"] = workloads.com_preview(85, v_max=0.30, u_max=0.6, seed=25)
    # 3. tables that change along the horizon (the builds that read them from LDS and keep W): the velocity limit as a full-size entry, loose
    #    everywhere but at ISOLATED_STEPS
    #    (42 instances: with these limits instance 60 of the same draw lies 3e-8 from the oracle, before the scan changed as after it)
    wl = workloads.com_preview(42, v_max=0.30, u_max=1.5, seed=25)
    N = wl["N"]
    f = np.full((N + 1, 3), 5.0)
    for k, lim in zip(ISOLATED_STEPS, (0.30, 0.06, 0.08)):
        f[k] = lim
    wl["cstrs"] = [dict(kind="trajectory", E=np.kron(np.eye(N + 1), _vel_rows(3, 2)), f=f.reshape(-1), ineq=True), wl["cstrs"][1]]
    out["lds_isolated"] = wl
    # 4. two rows per axis and step (RPA = 2): two velocity limits, the one tight on the first axis, the other on the second (5.0: never
    #    reached) -- stages where only the one, and stages where only the other slot has a violated row, whichever slot the plan gives which
    wl = workloads.com_preview(42, v_max=0.3, u_max=1.5, seed=9)
    inf = np.inf
    wl["cstrs"] = [dict(kind="trajectory_bound", lower=[-inf] * 6, upper=[inf, inf, inf, 0.2, 5.0, 5.0]),
                   dict(kind="trajectory", E=_vel_rows(3, 2), f=[5.0, 0.30, 5.0], ineq=True), wl["cstrs"][1]]
    out["second_slot_only"] = wl
    # 5. a run-time horizon: N = 7 on the build for N <= 20, a violated row at step N
    out["horizon_7"] = workloads.com_preview(63, N=7, v_max=0.30, u_max=1.5, seed=25)
    # 6. chains of three states, the tables in registers: limits on the positions a little above the goal -- the second axis overshoots it
    #    early in the horizon, the third ends above it at the last step, nothing between
    wl = workloads.jerk_preview(42, nu=3, N=20, seed=23, v_max=0.3, j_max=6.0)
    goal = np.asarray(wl["costs"][0]["p"], dtype=float)
    wl["x0"][:, 1:3] = np.minimum(wl["x0"][:, 1:3], goal[1:3] - [0.02, 0.05])  # (nobody starts at or next to a limit: such an instance may have no solution)
    wl["cstrs"] = [dict(kind="trajectory_bound", lower=[-inf] * 9, upper=[5.0, goal[1] + 0.012, goal[2] + 0.0015] + [inf] * 6), wl["cstrs"][1]]
    out["jerk_gap"] = wl
    #    chains of one state: the response of a first-order chain is monotone -- its violated rows are one run of steps whatever the limit --, so
    #    the position limit is a full-size entry, tight at two steps far apart (the builds that read their tables from LDS)
    wl = workloads.kinematic_preview(42)
    N = wl["N"]
    f = np.full((N + 1, 3), 5.0)
    f[KINEMATIC_STEPS[0]] = f[KINEMATIC_STEPS[1]] = 0.42
    wl["cstrs"] = [dict(kind="trajectory", E=np.eye(3 * (N + 1)), f=f.reshape(-1), ineq=True), wl["cstrs"][1]]
    out["kinematic_gap"] = wl
    # a batch of three full waves and one instance more: a spare lane takes part (GPU test only)
    out["spare_lane"] = workloads.com_preview(3 * 21 + 1, v_max=0.30, u_max=1.5, seed=25)
    return out


EMU_CASES = ("terminal_only", "row_and_bound", "lds_isolated", "second_slot_only", "horizon_7", "jerk_gap", "kinematic_gap")


def rollout_pattern(oracle, wl):
    """the oracle's unconstrained roll-out of the first wave against the workload's limits -> dict(rows: bool (row constraints, instances, N + 1,
    nu): row of that constraint at that step on that axis violated; bounds: bool (instances, N, nu))"""
    nx, nu, N = wl["B"].shape[1], wl["B"].shape[2], wl["N"]
    b = min(64 // nu, wl["x0"].shape[0])
    free = [dict(kind="control_bound", lower=[-np.inf] * nu, upper=[np.inf] * nu)]
    ro = oracle.lmpc_solve_batch(wl["A"][:b], wl["B"][:b], wl["d"][:b], wl["x0"][:b], N, wl["costs"], free, nthreads=4)
    assert (ro["status"] == 0).all()
    X = ro["trajectory"].reshape(b, N + 1, nx)
    U = ro["control"].reshape(b, N, nu)
    rows, bounds = [], np.zeros((b, N, nu), dtype=bool)
    for c in wl["cstrs"]:
        if c["kind"] == "control_bound":
            lo = np.broadcast_to(np.asarray(c["lower"], dtype=float).reshape(-1, nu), (N, nu))
            hi = np.broadcast_to(np.asarray(c["upper"], dtype=float).reshape(-1, nu), (N, nu))
            bounds |= (U > hi[None]) | (U < lo[None])
            continue
        v = np.zeros((b, N + 1, nu), dtype=bool)
        if c["kind"] == "trajectory_bound":
            up = np.asarray(c["upper"], dtype=float)
            assert np.isneginf(np.asarray(c["lower"], dtype=float)).all()
            for i in np.nonzero(np.isfinite(up))[0]:
                v[:, :, i % nu] |= X[:, :, i] > up[i]
        else:
            E, f = np.asarray(c["E"], dtype=float), np.asarray(c["f"], dtype=float)
            full = E.shape[1] != nx
            r = E.shape[0] // (N + 1) if full else E.shape[0]
            Es = E[:r, :nx]
            fs = f.reshape(N + 1, r) if full else np.tile(f, (N + 1, 1))
            for j in range(r):
                axis = np.nonzero(Es[j])[0][0] % nu
                v[:, :, axis] |= X @ Es[j] > fs[None, :, j]
        rows.append(v)
    return dict(rows=np.array(rows), bounds=bounds)


def _steps(v):
    """steps at which some lane of the wave is flagged"""
    return [int(k) for k in np.nonzero(v.reshape(v.shape[0], v.shape[1], -1).any(axis=(0, 2)))[0]]


def _longest_gap(steps):
    """the longest run of clean steps BETWEEN two flagged ones"""
    return max([b - a - 1 for a, b in zip(steps[:-1], steps[1:])], default=0)


def premise(name, pat, N):
    """what a case is there for, on the roll-out pattern of its first wave; raises where it does not hold"""
    rows, bounds = pat["rows"], pat["bounds"]
    anyrow = rows.any(axis=0)  # (instances, N + 1, nu)
    ks = _steps(anyrow)
    if name in ("terminal_only", "spare_lane"):
        assert ks and ks[-1] == N and len(ks) >= 2 and ks[-1] - ks[-2] - 1 >= 10, (name, ks)
    elif name == "row_and_bound":
        # (a stage at which some lane has a violated row and no violated bound, and ANOTHER lane a violated bound and no violated row)
        lanes_r, lanes_b = anyrow[:, :N].transpose(1, 0, 2).reshape(N, -1), bounds.transpose(1, 0, 2).reshape(N, -1)
        both = [k for k in range(N) if (lanes_r[k] & ~lanes_b[k]).any() and (lanes_b[k] & ~lanes_r[k]).any()]
        assert both, (name, ks, _steps(bounds))
    elif name == "lds_isolated":
        assert ks == list(ISOLATED_STEPS), (name, ks)
    elif name == "kinematic_gap":
        assert ks == list(KINEMATIC_STEPS) and _longest_gap(ks) >= 5, (name, ks)
    elif name == "second_slot_only":
        assert rows.shape[0] == 2
        k0, k1 = _steps(rows[0]), _steps(rows[1])
        assert set(k1) - set(k0) and set(k0) - set(k1), (name, k0, k1)
    elif name == "horizon_7":
        assert N == 7 and N in ks, (name, ks)
    elif name == "jerk_gap":
        assert _longest_gap(ks) >= 5, (name, ks)
    else:
        raise KeyError(name)
    return ks


def run(wl):
    """the emulator's results for a case, and what ran"""
    import pyemu
    re = pyemu.lmpc_solve(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], wl["costs"], wl["cstrs"])
    re["axis_run"] = pyemu.last_axis_run()
    return re


if __name__ == "__main__":
    rec = {}
    all_cases = cases()
    for name in EMU_CASES + ("spare_lane",):
        wl = all_cases[name]
        re = run(wl)
        for k in KEYS:
            rec[name + "/" + k] = re[k]
        rec[name + "/lane_pass_finished"] = np.int64(re["lane_pass_finished"])
        print("%-18s finished in the solver %d of %d, picks up to %d, builds %r" % (name, re["lane_pass_finished"], len(re["status"]),
                                                                                   re["iter"][:, 0].max(), re["axis_run"]))
    np.savez_compressed(PATH, **rec)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
