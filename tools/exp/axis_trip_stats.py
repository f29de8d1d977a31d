"""What the (instance, axis)-per-lane solver's waves do on the CoM workload, counted on the CPU with the oracle: one chain (two states, one control)
per (instance, axis), solved on its own -- qpgen2's run on an instance is an interleaving of its axes' runs (lmpc_axis.hpp), the counters add up.

    python tools/exp/axis_trip_stats.py [instances] [v_max] [u_max] [seed]        default: the first 6300 instances (300 waves of 21) of the headline's batch

Prints: trips per lane (a trip = one pick of a lane = one pass of the active-set loop), trips per wave (the longest lane's), the kinds of the
constraints active at the solutions, and where the UNCONSTRAINED roll-out -- what the first scan looks at -- violates bounds and rows."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyoracle  # noqa: E402
from copra_amd import workloads  # noqa: E402


def axis_chains(wl):
    """the CoM workload axis by axis: a batch of batch x 3 chains, chain 3 i + c = axis c of instance i"""
    b, N = wl["x0"].shape[0], wl["N"]
    A, B = np.zeros((b, 3, 2, 2)), np.zeros((b, 3, 2, 1))
    d, x0 = np.zeros((b, 3, 2)), np.zeros((b, 3, 2))
    for c in range(3):
        ix = [c, 3 + c]
        A[:, c] = wl["A"][:, ix][:, :, ix]
        B[:, c, :, 0] = wl["B"][:, ix, c]
        d[:, c], x0[:, c] = wl["d"][:, ix], wl["x0"][:, ix]
    return A.reshape(-1, 2, 2), B.reshape(-1, 2, 1), d.reshape(-1, 2), x0.reshape(-1, 2), N


def main(argv):
    b = int(argv[1]) if len(argv) > 1 else 6300
    v_max = float(argv[2]) if len(argv) > 2 else 0.6
    u_max = float(argv[3]) if len(argv) > 3 else 3.0
    seed = int(argv[4]) if len(argv) > 4 else 1
    wl = workloads.com_preview(65536, seed=seed, v_max=v_max, u_max=u_max)
    wl = dict(wl, A=wl["A"][:b], B=wl["B"][:b], d=wl["d"][:b], x0=wl["x0"][:b])
    A, B, d, x0, N = axis_chains(wl)
    goal, w = np.asarray(wl["costs"][0]["p"], dtype=float), np.asarray(wl["costs"][0]["weights"], dtype=float)
    wu = np.asarray(wl["costs"][1]["weights"], dtype=float)
    picks = np.zeros((b, 3), dtype=int)
    act_u = np.zeros((b, 3), dtype=int)
    act_v = np.zeros((b, 3), dtype=int)
    roll_u = np.zeros((b, 3, N), dtype=bool)
    roll_v = np.zeros((b, 3, N + 1), dtype=bool)
    for c in range(3):  # (the goal and the weights differ from axis to axis: one oracle batch per axis)
        costs = [dict(kind="trajectory", M=np.eye(2), p=goal[[c, 3 + c]], weights=w[[c, 3 + c]]), dict(kind="control", N=np.eye(1), p=np.zeros(1), weights=wu[[c]])]
        cstrs = [dict(kind="trajectory_bound", lower=[-np.inf] * 2, upper=[np.inf, v_max]), dict(kind="control_bound", lower=[-u_max], upper=[u_max])]
        free = [dict(kind="control_bound", lower=[-np.inf], upper=[np.inf])]
        sel = slice(c, None, 3)
        r = pyoracle.lmpc_solve_batch(A[sel], B[sel], d[sel], x0[sel], N, costs, cstrs, nthreads=16)
        f = pyoracle.lmpc_solve_batch(A[sel], B[sel], d[sel], x0[sel], N, costs, free, nthreads=16)
        assert (r["status"] == 0).all() and (f["status"] == 0).all()
        picks[:, c] = r["iter"][:, 0] - 1  # (qpgen2 counts the pass that finds nothing violated)
        act_u[:, c] = (np.abs(r["control"]) >= u_max - 1e-9).sum(1)
        act_v[:, c] = (r["trajectory"].reshape(b, N + 1, 2)[:, :, 1] >= v_max - 1e-9).sum(1)
        roll_u[:, c] = np.abs(f["control"]) > u_max
        roll_v[:, c] = f["trajectory"].reshape(b, N + 1, 2)[:, :, 1] > v_max
    nchk = min(b, 2000)
    whole = pyoracle.lmpc_solve_batch(wl["A"][:nchk], wl["B"][:nchk], wl["d"][:nchk], wl["x0"][:nchk], N, wl["costs"], wl["cstrs"], nthreads=16)
    same = int(((whole["iter"][:, 0] - 1) == picks[:nchk].sum(1)).sum())
    print("CoM workload seed %d, v_max %.2f, u_max %.2f: %d instances, %d chains" % (seed, v_max, u_max, b, 3 * b))
    print("the whole instance's picks equal the sum over its axes on %d of %d instances checked" % (same, nchk))
    hist = np.bincount(picks.ravel())
    print("trips per lane: " + ", ".join("%d: %.1f %%" % (k, 100.0 * n / picks.size) for k, n in enumerate(hist)))
    nw = b // 21
    per_wave = picks[:21 * nw].reshape(nw, 63).max(1)
    print("trips per wave (21 instances, %d waves): mean %.2f; " % (nw, per_wave.mean()) + ", ".join("%d: %.0f %%" % (k, 100.0 * n / nw) for k, n in enumerate(np.bincount(per_wave))))
    print("scans per wave (the roll-out and one per trip): %.2f" % (1.0 + per_wave.mean()))
    print("active at the solutions: %d control bounds, %d velocity rows on %d axes (of %d)" % (act_u.sum(), act_v.sum(), int((act_v > 0).sum()), 3 * b))
    ru, rv = roll_u[:21 * nw].reshape(nw, 63, N), roll_v[:21 * nw].reshape(nw, 63, N + 1)
    print("roll-out, violated bounds by stage (waves with one): " + ", ".join("%d: %d" % (k, n) for k, n in enumerate(ru.any(1).sum(0)) if n))
    print("roll-out, violated rows by step (waves with one): " + ", ".join("%d: %d" % (k, n) for k, n in enumerate(rv.any(1).sum(0)) if n)
          + "; %.0f %% of the waves have one anywhere" % (100.0 * rv.any((1, 2)).mean()))


if __name__ == "__main__":
    main(sys.argv)
