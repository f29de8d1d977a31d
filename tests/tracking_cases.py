"""Inputs of the reference-schedule tests (tests/test_reference_schedule_inputs.py on the CPU, tests/test_reference_schedule_gpu.py on the GPU):
the tracking controller of examples/tracking.py -- com_preview(v_max = 0.6, u_max = 3.0) with a full-size TrajectoryCost that follows a circle --,
its reference signals, the window a tick sees and the oracle's closed loop.  The oracle takes controller-wide costs: instances that follow the
same signal are solved together, one call per group."""
import numpy as np

from copra_amd import workloads

BATCH, TICKS = 512, 8
NOISE = 0.002  # position noise of examples/tracking.py
RTOL = 1e-6
ABS_FLOOR = 1e-3
NX, NU = 6, 3
TRACK_W = [10.0, 10.0, 10.0, 1.0, 1.0, 1.0]
# four distinct signals for the per-instance runs: (angular speed, phase, offset in height)
SIGNALS = ((0.4, 0.0, 0.0), (0.8, 0.5, 0.004), (-0.6, 1.0, -0.004), (1.2, 2.0, 0.008))


def circle(steps, speed=0.4, phase=0.0, lift=0.0, T=0.117, radius=0.05):
    """examples/tracking.py::reference_window as a signal: positions on a circle of 5 cm around x_init at the height of x_goal (+ lift),
    velocities to match; (steps, 6)"""
    t = T * np.arange(steps)
    c = workloads.COM_X_INIT[:3] + np.array([0.0, 0.0, workloads.COM_X_GOAL[2] - workloads.COM_X_INIT[2] + lift])
    a = speed * t + phase
    pos = c[None, :] + radius * np.stack([np.cos(a), np.sin(a), 0.0 * t], axis=1)
    vel = radius * speed * np.stack([-np.sin(a), np.cos(a), 0.0 * t], axis=1)
    return np.hstack([pos, vel])


def window(sched, first, S):
    """blocks min(first + s, steps - 1), s = 0 .. S-1, of sched (..., steps, r), stacked: (..., S r)"""
    idx = np.minimum(first + np.arange(S), sched.shape[-2] - 1)
    return sched[..., idx, :].reshape(sched.shape[:-2] + (-1,))


def tracking_workload(batch=BATCH, steps=TICKS + 21, shared_model=False):
    """the controller of examples/tracking.py; costs[0] is the full-size TrajectoryCost, created with the window of tick 0 of SIGNALS[0]"""
    wl = workloads.com_preview(batch, v_max=0.6, u_max=3.0)
    N = wl["N"]
    if shared_model:
        wl["A"], wl["B"], wl["d"] = (np.ascontiguousarray(np.broadcast_to(wl[k][0], wl[k].shape)) for k in ("A", "B", "d"))
    signals = np.stack([circle(steps, *s) for s in SIGNALS])
    track = dict(kind="trajectory", M=np.kron(np.eye(N + 1), np.eye(NX)), p=window(signals[0], 0, N + 1), weights=np.tile(TRACK_W, N + 1))
    wl["costs"] = [track, wl["costs"][1]]
    return wl, signals


def group_of(batch, per_instance):
    """which of the signals an instance follows: all the first one, or the four in turn"""
    return (np.arange(batch) % len(SIGNALS)) if per_instance else np.zeros(batch, dtype=int)


def position_noise(ticks, batch, nx, npos, seed):
    w = np.zeros((ticks, batch, nx))
    w[:, :, :npos] = NOISE * np.random.default_rng(seed).standard_normal((ticks, batch, npos))
    return w


def oracle_tick(oracle, wl, x, groups, p_of_group, cost_index=0):
    """one solve of every instance from the states x, instances of group g with p_of_group[g] as the reference of cost `cost_index`"""
    batch = x.shape[0]
    out = None
    for g, p in enumerate(p_of_group):
        sel = np.nonzero(groups == g)[0]
        if sel.size == 0:
            continue
        costs = list(wl["costs"])
        costs[cost_index] = dict(costs[cost_index], p=np.asarray(p))
        ref = oracle.lmpc_solve_batch(wl["A"][sel], wl["B"][sel], wl["d"][sel], x[sel], wl["N"], costs, wl["cstrs"], nthreads=8)
        if out is None:
            out = {k: np.zeros((batch,) + v.shape[1:], dtype=v.dtype) for k, v in ref.items()}
        for k, v in ref.items():
            out[k][sel] = v
    return out


def rel(a, b, floor=ABS_FLOOR):
    """the suite's measure: entry-wise relative error with an absolute floor"""
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


def moved_share(oracle, wl, x, groups, moved, frozen, nu, cost_index=0):
    """share of the instances whose first control with the window `moved` differs from the one with the window `frozen` by more than 100 RTOL"""
    a = oracle_tick(oracle, wl, x, groups, moved, cost_index)
    b = oracle_tick(oracle, wl, x, groups, frozen, cost_index)
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    return float((rel(a["control"][:, :nu], b["control"][:, :nu]).max(axis=1) > 100 * RTOL).mean())


def oracle_closed_loop(oracle, wl, signals, groups, w_seq, S, offset=0, cost_index=0):
    """the oracle alone: solve with the window of the tick, apply the first control to the model, add the disturbance; (x_hist, u_hist, status_hist)"""
    nu = wl["B"].shape[2]
    x = wl["x0"].copy()
    xs, us, ss = [x.copy()], [], []
    for t in range(w_seq.shape[0]):
        ref = oracle_tick(oracle, wl, x, groups, [window(s, t + offset, S) for s in signals], cost_index)
        u = ref["control"][:, :nu]
        ok = ref["status"] == 0
        xn = np.einsum("bij,bj->bi", wl["A"], x) + np.einsum("bij,bj->bi", wl["B"], np.where(ok[:, None], u, 0.0)) + wl["d"] + w_seq[t]
        x = np.where(ok[:, None], xn, x)
        xs.append(x.copy()), us.append(u.copy()), ss.append(ref["status"].copy())
    return np.stack(xs), np.stack(us), np.stack(ss)


# ---- the packed small controller: a falling mass whose TargetCost follows a goal that moves (S = 1, offset = N) ----
def integrator_workload(batch=BATCH, steps=TICKS + 17):
    wl = workloads.double_integrator(batch, N=16)
    k = np.arange(steps)[:, None]
    signals = np.stack([np.array([0.0, -1.0]) - k * np.array([0.02, 0.25]), np.array([0.1, -1.2]) - k * np.array([0.04, 0.3])])
    return wl, signals
