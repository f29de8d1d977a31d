"""Inputs of the tests of per-instance limits (copra_batch_set_constraint_rhs, copra_batch_set_control_bounds) on the (instance, axis)-per-lane
solver (tests/test_axis_limits_emu.py on the CPU, tests/test_axis_limits_gpu.py on the GPU): one controller per pair of builds the solver picks
(copra_amd/csrc/axis_builds.hpp), the seeded limits of every instance, and the oracle's answer instance by instance with that instance's own
limits.

The builds that keep their tables in registers (CT) read an instance's own limits; the others read the controller's.  front_end.hpp therefore
keeps the solver only where BOTH launches -- the first and the second chance of what the first lists -- are CT builds.  A case names the pair
it is meant to hit, so that the tests notice when a controller drifts to another pair.

The state limit of a workload (an upper TrajectoryBoundConstraint) is restated as a TrajectoryConstraint E x_k <= f: the only form the C ABI
gives a per-instance right-hand side.  Per-step rows take one right-hand side per row and instance, the same at every step; the cases whose
right-hand side changes along the horizon state the constraint as a full-size entry (E = kron(I_{N+1}, E_step)), which takes one per row
and step."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from copra_amd import workloads

SCALE = (0.5, 0.9)  # every instance's limits: the workload's own times U(0.5, 0.9)
AXIS_QMAX = 6  # kAxisQmax (plan_builder.hpp): active constraints per lane of the first launch; an axis with more is listed to the second

# the builds as pyemu.axis_build reports them, without QMAX and EXACT: (family, NXA, NU, NMAX, CT, RPA)
REG, LDS = True, False


def _pair(nxa, nu, nmax, first_ct, rpa_first, list_ct):
    return ("first", nxa, nu, nmax, first_ct, rpa_first), ("list", nxa, nu, nmax, list_ct, 2)


def _jerk20(b):
    return workloads.jerk_preview(b, nu=3, N=20, v_max=0.3, j_max=6.0)


# name: make (batch -> workload), seed of the limit draw, the pair of builds, and the variant:
#   use     which limits are set: "rhs", "bounds" or both
#   scale   the range of the per-instance scale
#   change  instance 5 gets a tighter upper bound on one control of step 0, instance 9 a tighter right-hand side of one row of step 2
#           (the constraint as a full-size entry): limits that change along the horizon send the instance to the tier
#   axis    whether the solver keeps the controller with limits set: both builds CT
CASES = {
    "com_n20": dict(make=lambda b: workloads.com_preview(b, N=20, v_max=0.5, u_max=2.5), seed=101, pair=_pair(2, 3, 20, REG, 1, REG), axis=True),
    "com_n20_tight": dict(make=lambda b: workloads.com_preview(b, N=20, v_max=0.3, u_max=1.0), seed=102, pair=_pair(2, 3, 20, REG, 1, REG), axis=True,
                          lists=True),
    "com_n21": dict(make=lambda b: workloads.com_preview(b, N=21, v_max=0.4, u_max=2.0), seed=103, pair=_pair(2, 3, 21, REG, 1, LDS)),
    "jerk3_n20": dict(make=_jerk20, seed=104, pair=_pair(3, 3, 20, REG, 1, LDS)),
    "jerk3_n14_amax": dict(make=lambda b: workloads.jerk_preview(b, nu=3, N=14, v_max=0.3, j_max=6.0, a_max=2.0), seed=105,
                           pair=_pair(3, 3, 20, LDS, 2, LDS)),
    "jerk2_n9_amax": dict(make=lambda b: workloads.jerk_preview(b, nu=2, N=9, v_max=0.3, j_max=6.0, a_max=1.5), seed=106,
                          pair=_pair(3, 2, 20, LDS, 2, LDS)),
    "kinematic3_n20": dict(make=lambda b: workloads.kinematic_preview(b, nu=3, N=20), seed=107, pair=_pair(1, 3, 20, REG, 1, LDS)),
    "kinematic2_n29": dict(make=lambda b: workloads.kinematic_preview(b, nu=2, N=29), seed=108, pair=_pair(1, 2, 31, REG, 1, LDS)),
    "jerk3_n16_axis_major": dict(make=lambda b: workloads.axis_major(workloads.jerk_preview(b, nu=3, N=16, v_max=0.3, j_max=6.0)), seed=109,
                                 pair=_pair(3, 3, 20, REG, 1, LDS)),
    "jerk3_n20_rhs_only": dict(make=_jerk20, seed=116, pair=_pair(3, 3, 20, REG, 1, LDS), use=("rhs",)),
    "jerk3_n20_bounds_only": dict(make=_jerk20, seed=111, pair=_pair(3, 3, 20, REG, 1, LDS), use=("bounds",)),
    # (limits equal to the controller-wide ones: tighter ones for the whole controller, so that some axis outgrows a lane of the first launch)
    "jerk3_n20_scale_one": dict(make=lambda b: workloads.jerk_preview(b, nu=3, N=20, v_max=0.25, j_max=3.0), seed=112, pair=_pair(3, 3, 20, REG, 1, LDS),
                                scale=(1.0, 1.0)),
    "jerk3_n20_change": dict(make=_jerk20, seed=113, pair=_pair(3, 3, 20, REG, 1, LDS), change=True),
}


def controller(name, batch):
    """the case's workload with its state limit as rows E x_k <= f (full-size where the case changes a right-hand side along the horizon)"""
    case = CASES[name]
    wl = case["make"](batch)
    tb, cb = wl["cstrs"]
    assert tb["kind"] == "trajectory_bound" and cb["kind"] == "control_bound" and np.isneginf(np.asarray(tb["lower"], dtype=float)).all()
    up = np.asarray(tb["upper"], dtype=float)
    sel = np.nonzero(np.isfinite(up))[0]
    E, f = np.eye(up.size)[sel], up[sel]
    if case.get("change"):
        E, f = np.kron(np.eye(wl["N"] + 1), E), np.tile(f, wl["N"] + 1)
    return dict(wl, cstrs=[dict(kind="trajectory", E=E, f=f, ineq=True), cb])


def draw_case_limits(name, wl):
    """-> dict(rhs: (batch, rows of constraint 0) as copra_batch_set_constraint_rhs takes them, or None; row_rhs: the same in the stacked order
    of all rows (batch, mgen), as the emulator takes them; lo, hi: (batch, nu N), or None)"""
    case = CASES[name]
    use = case.get("use", ("rhs", "bounds"))
    rng = np.random.default_rng(case["seed"])
    batch, nu, N = wl["x0"].shape[0], wl["B"].shape[2], wl["N"]
    lo_s, hi_s = case.get("scale", SCALE)
    sf, su = rng.uniform(lo_s, hi_s, batch), rng.uniform(lo_s, hi_s, batch)
    f = np.asarray(wl["cstrs"][0]["f"], dtype=float)
    out = dict(rhs=None, row_rhs=None, lo=None, hi=None)
    if "rhs" in use:
        out["rhs"] = sf[:, None] * f[None, :]
    if "bounds" in use:
        out["lo"] = su[:, None] * np.tile(np.asarray(wl["cstrs"][1]["lower"], dtype=float), N)[None, :]
        out["hi"] = su[:, None] * np.tile(np.asarray(wl["cstrs"][1]["upper"], dtype=float), N)[None, :]
    if case.get("change"):
        r = f.size // (N + 1)
        out["hi"][5, nu * 0 + 1] *= 0.5  # (a bound and a row that are, or become, active: the tests check that the answers depend on them)
        out["rhs"][9, r * 2 + 2] *= 0.5
    if out["rhs"] is not None:  # (one general constraint: its rows are all the rows; a per-step entry repeats along the horizon)
        out["row_rhs"] = out["rhs"] if case.get("change") else np.tile(out["rhs"], (1, N + 1))
    return out


def bounds_arg(lim):
    return None if lim["lo"] is None else (lim["lo"], lim["hi"])


def instance_cstrs(wl, lim, k):
    """the controller's constraints with instance k's own limits, stated the oracle's way (it takes controller-wide constraints)"""
    c0, c1 = wl["cstrs"]
    if lim is not None and lim["rhs"] is not None:
        c0 = dict(c0, f=lim["rhs"][k])
    if lim is not None and lim["lo"] is not None:
        c1 = dict(kind="control_bound", lower=lim["lo"][k], upper=lim["hi"][k])
    return [c0, c1]


def oracle_by_instance(oracle, wl, lim, costs_of=None, shared=False, x0=None, nthreads=16):
    """the oracle's answer instance by instance, every instance with its own limits (and costs_of(k), and system 0 where `shared`), stacked like
    lmpc_solve_batch's: dict(status, iter, control, trajectory)"""
    x0 = wl["x0"] if x0 is None else x0

    def one(k):
        s = 0 if shared else k
        return oracle.lmpc_solve(wl["A"][s], wl["B"][s], wl["d"][s], x0[k], wl["N"], wl["costs"] if costs_of is None else costs_of(k),
                                 instance_cstrs(wl, lim, k))

    oracle.lib()
    with ThreadPoolExecutor(max_workers=nthreads) as pool:  # (the solves run outside the interpreter's lock)
        rows = list(pool.map(one, range(x0.shape[0])))
    return dict(status=np.array([r["status"] for r in rows], dtype=np.int32), iter=np.array([r["iter"] for r in rows], dtype=np.int32),
                control=np.stack([r["control"] for r in rows]), trajectory=np.stack([r["trajectory"] for r in rows]))


def listed_by_oracle(wl, lim, ref, tol=1e-9):
    """instances with more than AXIS_QMAX limits active on ONE axis at the oracle's solution: their active set outgrows a lane of the first
    launch, so the first launch lists them to the second (a lower bound on what it lists: a set can shrink again before the end)"""
    batch, nx, nu, N = wl["x0"].shape[0], wl["B"].shape[1], wl["B"].shape[2], wl["N"]
    E = np.asarray(wl["cstrs"][0]["E"], dtype=float)
    full = E.shape[1] != nx
    Es = E[:E.shape[0] // (N + 1), :nx] if full else E
    axis_of_row = np.array([np.nonzero(row)[0][0] for row in Es])  # (state index; its axis below)
    state_axis = _state_axes(wl)
    out = np.zeros(batch, dtype=bool)
    for k in np.nonzero(ref["status"] == 0)[0]:
        cs = instance_cstrs(wl, lim, k)
        x = ref["trajectory"][k].reshape(N + 1, nx)
        f = np.asarray(cs[0]["f"], dtype=float)
        f = f.reshape(N + 1, -1) if f.size == Es.shape[0] * (N + 1) else np.tile(f, (N + 1, 1))
        act_rows = np.abs(x @ Es.T - f) <= tol  # (N + 1, rows)
        u = ref["control"][k].reshape(N, nu)
        lo = np.broadcast_to(np.asarray(cs[1]["lower"], dtype=float).reshape(-1, nu), (N, nu))
        hi = np.broadcast_to(np.asarray(cs[1]["upper"], dtype=float).reshape(-1, nu), (N, nu))
        act_u = (np.abs(u - lo) <= tol) | (np.abs(u - hi) <= tol)
        per_axis = act_u.sum(axis=0)
        for j, s in enumerate(axis_of_row):
            per_axis[state_axis[s]] += act_rows[:, j].sum()
        out[k] = per_axis.max() > AXIS_QMAX
    return out


def _state_axes(wl):
    """axis of every state: the control whose chain it belongs to (state i on axis i % nu, or axis-major order)"""
    nx, nu = wl["B"].shape[1], wl["B"].shape[2]
    axis_major = "axis-major" in wl.get("name", "")
    return np.array([i // (nx // nu) if axis_major else i % nu for i in range(nx)])


def check_inputs(name, wl, lim, ref):
    """the conditions on a case's inputs, from the oracle alone: most instances are solved, the constraints matter, and where the second
    launch's build is another kind than the first's, somebody is listed to it"""
    case = CASES[name]
    ok = ref["status"] == 0
    assert 4 * ok.sum() >= 3 * ok.size, (name, int(ok.sum()), ok.size)
    assert (ref["iter"][ok, 0] >= 2).mean() >= 0.3, (name, float((ref["iter"][ok, 0] >= 2).mean()))
    first, second = case["pair"]
    if first[4] != second[4] or case.get("lists"):
        assert listed_by_oracle(wl, lim, ref).any(), name


def strip(build):
    """(family, NXA, NU, NMAX, QMAX, EXACT, CT, RPA) of pyemu -> (family, NXA, NU, NMAX, CT, RPA)"""
    return None if build is None else (build[0], build[1], build[2], build[3], build[6], build[7])
