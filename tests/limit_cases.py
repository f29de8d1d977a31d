"""Inputs of the limit-schedule tests (tests/test_limit_schedule_inputs.py on the CPU, tests/test_limit_schedule_gpu.py on the GPU): controllers
whose limits move during the closed loop -- a velocity limit written as a per-step TrajectoryConstraint (stacked rows, so that
copra_batch_set_constraint_schedule can move it) and the ControlBoundConstraint --, the limit signals, the window a tick sees and the oracle's
statement of a tick.  The oracle takes controller-wide constraints: the constraint becomes a FULL-SIZE TrajectoryConstraint
(E = kron(I_{N+1}, [0 I3])) with the window as f, the ControlBoundConstraint gets the window as full-size lower / upper, and instances that
follow the same signals are solved together, one call per group (as tests/tracking_cases.py does for references)."""
import numpy as np

import tracking_cases as tc
from copra_amd import workloads

BATCH, TICKS = tc.BATCH, tc.TICKS
RTOL, ABS_FLOOR = tc.RTOL, tc.ABS_FLOOR
GROUPS = 4
# com_limits / coupled_limits: V_MILD, U_LIMITS: (limit at block 0, limit held at the end, blocks of the linear descent, block where it
# starts), one tuple per group; every signal tightens monotonically and then holds.  The velocity limit includes x_0 (a TrajectoryConstraint does): a state above it
# is "no solution", and a state that RIDES the limit at step 1 is above it at the next tick by the rounding of the solve (seen with the
# oracle: 1e-13).  So no velocity signal may bind at step 1 before the last tick:
#   V_LIMITS  (wide limit, its last block, the levels of the blocks behind it: the last one is held) stays wide for the ticks of the loop and
#             falls steeply behind them: with preview the horizon of the later ticks sees the fall and brakes for it (the actuator can follow:
#             0.21 per step after the first, < u_max T = 3.0 x 0.08) -- the runs of the constraint schedule ALONE
#   V_MILD    tightens slowly above every velocity of the loop -- the runs together with the bound schedule, whose derated actuator could
#             not brake for V_LIMITS, and every run without preview, where the whole horizon sees the limit of the present tick
# The actuator limit binds at step 0 at every tick.  The numbers are tuned in tests/test_limit_schedule_inputs.py.
V_LIMITS = ((0.90, 7, (0.50, 0.29, 0.08, 0.0)), (0.92, 7, (0.52, 0.31, 0.10, 0.01)), (0.88, 7, (0.50, 0.29, 0.08, -0.01)), (0.94, 7, (0.54, 0.33, 0.12, 0.02)))
V_MILD = ((0.90, 0.75, 20, 0), (0.92, 0.77, 20, 0), (0.88, 0.74, 20, 0), (0.94, 0.78, 20, 0))
U_LIMITS = ((3.0, 0.7, 8, 0), (3.2, 0.8, 8, 0), (2.8, 0.6, 8, 0), (3.4, 0.9, 8, 0))
# integrator_limits: the upper bound of the thrust (the lower one stays -inf)
I_LIMITS = ((200.0, 120.0), (190.0, 110.0), (210.0, 130.0), (180.0, 100.0))


def ramp(steps, hi, lo, span, start=0):
    """hi up to block `start`, lo from block start + span on, linear in between: tightens monotonically, then holds; (steps,)"""
    return hi - (hi - lo) * np.clip(np.arange(steps) - start, 0, span) / float(span)


def window(sched, first, S, preview=True):
    """blocks min(first + s, steps - 1) -- preview -- or min(first, steps - 1), s = 0 .. S-1, of sched (..., steps, r), stacked: (..., S r)"""
    idx = np.minimum(first + (np.arange(S) if preview else np.zeros(S, dtype=int)), sched.shape[-2] - 1)
    return sched[..., idx, :].reshape(sched.shape[:-2] + (-1,))


def group_of(batch, per_instance):
    return (np.arange(batch) % GROUPS) if per_instance else np.zeros(batch, dtype=int)


def com_limits(batch=BATCH, coupled=False, steps=TICKS + 12):
    """workloads.com_preview with the velocity bound restated as a per-step TrajectoryConstraint (E = [0 I3], f = v_max: 3 rows, N + 1 steps)
    and the symmetric ControlBoundConstraint; coupled: one nonzero off-axis entry in every A (the axes are no longer decoupled: the lane pass
    and the tiers solve it, not the axis solver).  Returns the workload and the signals dict(v (4, steps, 3), lo (4, steps, 3), up)."""
    wl = workloads.com_preview(batch, v_max=V_MILD[0][0], u_max=U_LIMITS[0][0])
    if coupled:
        wl["A"] = wl["A"].copy()
        wl["A"][:, 0, 4] = 0.01
    E = np.hstack([np.zeros((3, 3)), np.eye(3)])
    wl["cstrs"] = [dict(kind="trajectory", E=E, f=[V_MILD[0][0]] * 3), wl["cstrs"][1]]

    def sig3(limits):
        return np.stack([np.repeat(ramp(steps, hi, lo, span, start)[:, None], 3, axis=1) for hi, lo, span, start in limits])

    def fall(hi, last, levels):
        sig = np.full(steps, levels[-1])
        sig[:last + 1] = hi
        sig[last + 1:last + 1 + len(levels)] = levels
        return np.repeat(sig[:, None], 3, axis=1)

    up = sig3(U_LIMITS)
    return wl, dict(v=np.stack([fall(*a) for a in V_LIMITS]), v_mild=sig3(V_MILD), lo=-up, up=up)


def integrator_limits(batch=BATCH, steps=TICKS + 12):
    """workloads.double_integrator(N = 16), the packed small controller: the upper thrust bound tightens, the lower one stays -inf"""
    wl = workloads.double_integrator(batch, N=16)
    span = TICKS + wl["N"]
    up = np.stack([ramp(steps, hi, lo, span)[:, None] for hi, lo in I_LIMITS])
    return wl, dict(v=None, v_mild=None, lo=np.full_like(up, -np.inf), up=up)


def vkey(preview, use):
    """the velocity signal a run takes (see V_LIMITS)"""
    return "v" if preview and "bounds" not in use else "v_mild"


def windows_at(wl, sig, t, preview=True, use=("v", "bounds"), offset=0):
    """what the oracle is given for tick t, one dict per group: v -- the full window of the velocity constraint (N + 1 blocks) --, lo / up -- of
    the bounds (N blocks); only the limits named in `use` move, the others keep their creation values (None)"""
    N = wl["N"]
    out = []
    for g in range(GROUPS):
        w = dict(v=None, lo=None, up=None)
        if "v" in use and sig["v"] is not None:
            w["v"] = window(sig[vkey(preview, use)][g], t + offset, N + 1, preview)
        if "bounds" in use:
            w["lo"], w["up"] = window(sig["lo"][g], t + offset, N, preview), window(sig["up"][g], t + offset, N, preview)
        out.append(w)
    return out


def oracle_cstrs(wl, w):
    """the controller's constraints with the windows w of one group stated the oracle's way"""
    N = wl["N"]
    cstrs = []
    for c in wl["cstrs"]:
        if c["kind"] == "trajectory" and w["v"] is not None:
            c = dict(kind="trajectory", E=np.kron(np.eye(N + 1), np.asarray(c["E"])), f=np.asarray(w["v"]))
        elif c["kind"] == "control_bound" and w["up"] is not None:
            c = dict(kind="control_bound", lower=np.asarray(w["lo"]), upper=np.asarray(w["up"]))
        cstrs.append(c)
    return cstrs


def oracle_tick(oracle, wl, x, groups, wins, p_of_group=None, cost_index=0):
    """one solve of every instance from the states x, instances of group g with the windows wins[g] (and p_of_group[g] as the reference of cost
    `cost_index`)"""
    batch = x.shape[0]
    out = None
    for g, w in enumerate(wins):
        sel = np.nonzero(groups == g)[0]
        if sel.size == 0:
            continue
        costs = list(wl["costs"])
        if p_of_group is not None:
            costs[cost_index] = dict(costs[cost_index], p=np.asarray(p_of_group[g]))
        ref = oracle.lmpc_solve_batch(wl["A"][sel], wl["B"][sel], wl["d"][sel], x[sel], wl["N"], costs, oracle_cstrs(wl, w), nthreads=8)
        if out is None:
            out = {k: np.zeros((batch,) + v.shape[1:], dtype=v.dtype) for k, v in ref.items()}
        for k, v in ref.items():
            out[k][sel] = v
    return out


def moved_share(oracle, wl, x, groups, moved, frozen, nu, p_moved=None, p_frozen=None):
    """tracking_cases.moved_share for limit windows: share of the instances whose first control with the windows `moved` differs from the one with
    the windows `frozen` by more than 100 RTOL"""
    a = oracle_tick(oracle, wl, x, groups, moved, p_moved)
    b = oracle_tick(oracle, wl, x, groups, frozen, p_frozen)
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    return float((tc.rel(a["control"][:, :nu], b["control"][:, :nu]).max(axis=1) > 100 * RTOL).mean())


def active_share(wl, ref, wins, groups, tol=1e-9):
    """share of the instances for which a scheduled limit is active somewhere on the horizon: within tol of its bound"""
    nx, nu, N = wl["B"].shape[1], wl["B"].shape[2], wl["N"]
    batch = ref["control"].shape[0]
    act = np.zeros(batch, dtype=bool)
    for g, w in enumerate(wins):
        sel = groups == g
        u = ref["control"][sel]
        if w["up"] is not None:
            act[sel] |= (np.abs(u - w["up"]) <= tol).any(axis=1) | (np.abs(u - w["lo"]) <= tol).any(axis=1)
        if w["v"] is not None:
            vel = ref["trajectory"][sel].reshape(-1, N + 1, nx)[:, :, nx - 3:].reshape(-1, 3 * (N + 1))
            act[sel] |= (np.abs(vel - w["v"]) <= tol).any(axis=1)
    return float(act.mean())


NOISE = 0.04  # position noise per tick: twenty times tests/tracking_cases.py's, so that the loop still works against its limits at the last tick


def noise(wl, seed):
    nx = wl["B"].shape[1]
    return (NOISE / tc.NOISE) * tc.position_noise(TICKS, wl["x0"].shape[0], nx, nx // 2, seed)


def oracle_closed_loop(oracle, wl, sig, groups, w_seq, preview=True, use=("v", "bounds")):
    """the oracle alone: solve with the windows of the tick, apply the first control to the model, add the disturbance; (x_hist, u_hist,
    status_hist, the last tick's solve)"""
    nu = wl["B"].shape[2]
    x = wl["x0"].copy()
    xs, us, ss = [x.copy()], [], []
    ref = None
    for t in range(w_seq.shape[0]):
        ref = oracle_tick(oracle, wl, x, groups, windows_at(wl, sig, t, preview, use))
        u = ref["control"][:, :nu]
        ok = ref["status"] == 0
        xn = np.einsum("bij,bj->bi", wl["A"], x) + np.einsum("bij,bj->bi", wl["B"], np.where(ok[:, None], u, 0.0)) + wl["d"] + w_seq[t]
        x = np.where(ok[:, None], xn, x)
        xs.append(x.copy()), us.append(u.copy()), ss.append(ref["status"].copy())
    return np.stack(xs), np.stack(us), np.stack(ss), ref
