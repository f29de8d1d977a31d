"""Inputs and measures of the per-instance cost-weight tests (tests/test_cost_weights_emu.py and tests/test_cost_weights_inputs.py on the CPU,
tests/test_cost_weights_gpu.py on the GPU): the workloads, the weights an instance gets, and the oracle run with each instance's own weights.
The oracle takes controller-wide costs: instances that share their weights are solved together, one call per group."""
import numpy as np

from copra_amd import workloads

RTOL = 1e-6
ABS_FLOOR = 1e-3
K = 64
KEYS = ("control", "trajectory", "status", "iter")
TRACK_W = [10.0, 10.0, 10.0, 1.0, 1.0, 1.0]


def rel(a, b, floor=ABS_FLOOR):
    """the suite's measure: entry-wise relative error with an absolute floor"""
    return float(np.nanmax(np.abs(a - b) / np.maximum(np.abs(b), floor))) if np.size(a) else 0.0


def rel_inst(a, b, floor=ABS_FLOOR):
    """per instance (row), norm-wise: max_i |a_i - b_i| / max(max_i |b_i|, floor) -- the scattered weights (a ratio of up to 1e4 between
    the state and the control weights) leave the oracle's own Goldfarb-Idnani arithmetic that far from the optimum in its small entries;
    the parity suite's measure for comparisons set by the conditioning of the whole problem (tests/test_gpu_parity.py::_rel_vec)"""
    if not np.size(a):
        return 0.0
    return float(np.nanmax(np.nanmax(np.abs(a - b), axis=1) / np.maximum(np.nanmax(np.abs(b), axis=1), floor)))


def grouped_weights(wl, batch, seed, groups=K):
    """per cost: (batch, rows) weights, log-uniform in [0.1, 10] x the creation weights, drawn from `groups` vectors; and the group of each instance"""
    rng = np.random.default_rng(seed)
    group = rng.integers(0, groups, batch)
    ws = []
    for c in wl["costs"]:
        w0 = np.asarray(c["weights"], dtype=np.float64)
        table = w0[None, :] * np.exp(rng.uniform(np.log(0.1), np.log(10.0), (groups, w0.size)))
        ws.append(table[group])
    return ws, group


def indexed_weights(wl, batch):
    """weights that are a function of the instance's number k, every row r of every cost t with another factor: a lane that reads another
    instance's or another row's weight solves another problem.  Factors in [0.5, 4.2]."""
    k = np.arange(batch, dtype=np.float64)[:, None]
    ws = []
    for t, c in enumerate(wl["costs"]):
        w0 = np.asarray(c["weights"], dtype=np.float64)
        r = np.arange(w0.size, dtype=np.float64)[None, :]
        ws.append(w0[None, :] * (0.5 + 0.023 * k + 0.31 * r + 0.17 * t))
    return ws, np.arange(batch)


def oracle_grouped(oracle, wl, ws, group, costs_of=None, cstrs_of=None, **kw):
    """the oracle's results for every instance, one oracle batch per group of instances that share their weights.  costs_of(k, costs),
    cstrs_of(k): the costs (already with instance k's weights) and the constraints of the group whose first instance is k -- other per-instance
    inputs the group shares"""
    batch = group.size
    nx, nu, N = wl["B"].shape[1], wl["B"].shape[2], wl["N"]
    out = dict(control=np.full((batch, nu * N), np.nan), trajectory=np.full((batch, nx * (N + 1)), np.nan),
               status=np.zeros(batch, dtype=np.int32), iter=np.zeros((batch, 2), dtype=np.int32))
    for g in np.unique(group):
        idx = np.nonzero(group == g)[0]
        costs = [dict(c, weights=w[idx[0]]) if w is not None else c for c, w in zip(wl["costs"], ws)]
        if costs_of is not None:
            costs = costs_of(idx[0], costs)
        cstrs = wl["cstrs"] if cstrs_of is None else cstrs_of(idx[0])
        r = oracle.lmpc_solve_batch(wl["A"][idx], wl["B"][idx], wl["d"][idx], wl["x0"][idx], N, costs, cstrs, nthreads=8, **kw)
        for k in out:
            out[k][idx] = r[k]
    return out


def assert_matches(res, ref, skip=1):
    """statuses equal; on the instances the oracle solved (all but `skip` at the most) both iteration counters equal, U and X within RTOL
    norm-wise per instance.  Prints the entry-wise figures next to them."""
    assert np.array_equal(res["status"], ref["status"])
    ok = ref["status"] == 0
    assert ok.sum() >= max(len(ok) - skip, 1)
    assert np.array_equal(res["iter"][ok], ref["iter"][ok])
    u, x = rel_inst(res["control"][ok], ref["control"][ok]), rel_inst(res["trajectory"][ok], ref["trajectory"][ok])
    print("norm-wise U %.2e, X %.2e; entry-wise (floor 1e-3) U %.2e, X %.2e" % (u, x, rel(res["control"][ok], ref["control"][ok]), rel(res["trajectory"][ok], ref["trajectory"][ok])))
    assert u <= RTOL and x <= RTOL


# ---- the workloads of the (instance, axis)-per-lane solver's weight-reading builds (lmpc_axis.hpp, WTS) ----
def two_rows(batch=42, N=20):
    """two rows per axis and step, the same at every step: a lower velocity limit as rows next to the upper bound (the builds with RPA = 2;
    tests/golden/gen_axis_trip_bounds.py: com_two_rows)"""
    wl = workloads.com_preview(batch, N=N, v_max=0.3, u_max=1.5, seed=9)
    vsel = np.hstack([np.zeros((3, 3)), np.eye(3)])
    wl["cstrs"] = [wl["cstrs"][0], dict(kind="trajectory", E=-vsel, f=[0.3] * 3, ineq=True), wl["cstrs"][1]]
    return wl


def tracking(batch=43, N=20, two_row=False):
    """a reference-trajectory cost: a full-size TrajectoryCost whose reference changes along the horizon and whose weights repeat (the only
    form the weights of such a cost may take: copra_batch_set_cost_weights)"""
    wl = two_rows(batch, N) if two_row else workloads.com_preview(batch, N=N, v_max=0.5, u_max=2.5, seed=40 + N)
    ts = np.linspace(0.0, 1.0, N + 1)
    pos = workloads.COM_X_INIT[:3][None, :] + ts[:, None] * (workloads.COM_X_GOAL[:3] - workloads.COM_X_INIT[:3])[None, :]
    pf = np.hstack([pos, 0.05 * np.ones((N + 1, 3))]).reshape(-1)
    track = dict(kind="trajectory", M=np.kron(np.eye(N + 1), np.eye(6)), p=pf, weights=np.tile(TRACK_W, N + 1))
    wl["costs"] = [track, wl["costs"][1]]
    return wl


def tracking_weights(wl, batch, seed, groups=8):
    """weights of tracking(): the step's six of the reference-trajectory cost repeated along the horizon, the control cost's three"""
    N = wl["N"]
    step = dict(wl, costs=[dict(wl["costs"][0], weights=TRACK_W), wl["costs"][1]])
    ws, group = grouped_weights(step, batch, seed, groups)
    return [np.tile(ws[0], (1, N + 1)), ws[1]], group


# name -> (workload, two-slot mode of the emulator, (first_w, list_w) entries of axis_builds.hpp the controller gets, tight)
def axis_cases():
    FW = lambda exact, rpa: ("first_w", 2, 3, 20, 6, exact, True, rpa)
    LW = ("list_w", 2, 3, 20, 16, False, True, 2)
    out = {}
    out["com_v06"] = (workloads.com_preview(85, v_max=0.6, u_max=3.0, seed=25), False, (FW(True, 1), LW), False)
    out["com_v06_two_slot"] = (workloads.com_preview(85, v_max=0.6, u_max=3.0, seed=25), True, (FW(True, 1), LW), False)
    out["com_v025"] = (workloads.com_preview(85, v_max=0.25, u_max=1.2, seed=25), False, (FW(True, 1), LW), True)
    out["com_v025_two_slot"] = (workloads.com_preview(85, v_max=0.25, u_max=1.2, seed=25), True, (FW(True, 1), LW), True)
    out["two_rows"] = (two_rows(42), False, (FW(True, 2), LW), False)
    out["two_rows_N12"] = (two_rows(42, N=12), False, (FW(False, 2), LW), False)
    out["N12"] = (workloads.com_preview(44, N=12, v_max=0.35, u_max=1.8, seed=23), False, (FW(False, 1), LW), False)
    out["axis_major"] = (workloads.axis_major(workloads.com_preview(45, v_max=0.4, u_max=2.0, seed=17)), False, (FW(True, 1), LW), False)
    return out


def com_axis_counts(wl, ro, vmax, umax):
    """constraints active at the oracle's solution, per (instance, axis) of the CoM model: what a lane's active set ends with"""
    b, N = len(ro["status"]), wl["N"]
    X = ro["trajectory"].reshape(b, N + 1, 6)
    U = ro["control"].reshape(b, N, 3)
    return (X[:, :, 3:] >= vmax - 1e-9).sum(1) + (np.abs(U) >= umax - 1e-9).sum(1)
