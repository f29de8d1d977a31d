"""The fleet of examples/monte_carlo_scores.py, looked at tick by tick: the envelope of a Monte-Carlo run with no history leaving the device.

The scores answer "how did each robot do over the whole run".  A trace answers "how did the fleet look at tick t":

  set_trace(capacity=ticks, estimate_error=True, state_limits=(None, v_max))

and every tick of rollout() then reduces the batch into one slot on the device -- for every row of the plant's TRUE state, of the applied
control and of the observer's estimation error the number of robots counted, mean, spread, extremes and the robots that hold them; the
number of robots beyond the velocity limit; the numbers solved, replayed, on the fallback and held.  rollout() is asked for no x_hist, no
u_hist and no xhat_hist; trace() reads ticks x 960 bytes back.  A caller of the C ABI gets the same slots from copra_batch_get_trace
(tests/cpp/test_trace.cpp).  Traces pair with scores: both are on here, and neither changes a byte of the other.

    python examples/monte_carlo_envelope.py [batch] [ticks]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, workloads  # noqa: E402
from copra_amd.observer_design import kalman_gain  # noqa: E402

SIGMA_W = np.array([0.01, 0.01, 0.01, 0.005, 0.005, 0.005])
V_MAX = 0.6  # the velocity bound of workloads.com_preview: checked on the true state, which noise pushes across it


def closed_loop_trace(batch, ticks, seed, control_weight=1e-3, load=0.004, sensor_noise=0.01):
    """(trace, score summary) of one closed-loop run -- the scenario of examples/monte_carlo_scores.py::closed_loop_scores with a trace"""
    wl = workloads.com_preview(batch)
    nx, nu, ny, N = 6, 3, 3, wl["N"]
    costs = [dict(c) for c in wl["costs"]]
    costs[1]["weights"] = [control_weight] * nu
    rng = np.random.default_rng(0)
    eng = BatchLMPC(nx, nu, N, batch, costs, wl["cstrs"])
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    C = np.eye(nx)[:ny]
    G = np.zeros((nx, ny))
    G[3:] = np.eye(3)
    Lx, Ld = kalman_gain(wl["A"], C, 1e-4 * np.eye(nx), sensor_noise ** 2 * np.eye(ny) + 1e-4 * np.eye(ny), with_bias=True, Qd=1e-5 * np.eye(ny), Gd=G)
    eng.set_observer(C, Lx, Ld)
    xhat0 = wl["x0"].copy()
    xhat0[:, 3:] += 0.1 * rng.choice([-1.0, 1.0], (batch, 3))
    eng.set_x0(xhat0)
    c = np.zeros((batch, nx))
    c[:, 3:] = load * rng.uniform(-1.0, 1.0, (batch, 3))
    eng.set_noise(seed, process=SIGMA_W, sensor=np.full(ny, sensor_noise))
    goal = np.asarray(wl["costs"][0]["p"], dtype=np.float64)[:nx]
    upper = np.array([np.inf] * 3 + [V_MAX] * 3)
    eng.set_score(state_weights=[1.0, 1.0, 1.0, 0.0, 0.0, 0.0], control_weights=[1e-3] * nu, state_ref=goal, state_limits=(None, upper), tol=1e-9)
    eng.set_trace(ticks, estimate_error=True, state_limits=(None, upper), tol=1e-9)
    eng.rollout(ticks, plant=(wl["A"], wl["B"], wl["d"] + c), stream=torch.cuda.current_stream().cuda_stream)  # no history at all
    return eng.trace(), eng.score_summary(), eng.trace_info(), goal


def envelope(stat):
    """mean, standard deviation, min, max of one row's statistics at every tick"""
    n = np.maximum(stat["n"] - 1, 1)
    return stat["mean"], np.sqrt(stat["m2"] / n), stat["min"], stat["max"]


def run(batch=4096, ticks=60, seed=2026, row=0):
    tr, summary, info, goal = closed_loop_trace(batch, ticks, seed)
    mean, std, low, high = envelope(tr["x"][:, row])
    emean, estd, _, _ = envelope(tr["err"][:, 3 + row])
    lines = ["%d robots, %d ticks; position row %d (goal %.3g), the share beyond the velocity limit, the observer's velocity error" % (batch, ticks, row, goal[row])]
    for t in sorted({0, 1, 2, 5, 10, ticks // 2, ticks - 1}):
        if t >= ticks:
            continue
        h = tr["head"][t]
        lines.append("  tick %3d: %.4f +- %.4f in [%.4f (robot %d), %.4f (robot %d)]; %5.2f %% violating (largest excess %.3g); error %+.2e +- %.2e; held %d"
                     % (h["tick"], mean[t], std[t], low[t], tr["x"]["argmin"][t, row], high[t], tr["x"]["argmax"][t, row], 100.0 * h["violating"] / batch,
                        tr["viol"]["max"][t], emean[t], estd[t], h["held"]))
    lines.append("violating robot-ticks: %d from the trace, %d from the scores" % (int(tr["head"]["violating"].sum()), summary["violating"]))
    lines.append("bytes read back: %d (the trace) + 336 (the summary); x_hist, u_hist and xhat_hist would have taken %d"
                 % (info["recorded"] * info["slot_bytes"], 8 * batch * ((ticks + 1) * 6 + ticks * 3 + ticks * 6)))
    assert int(tr["head"]["violating"].sum()) == summary["violating"]  # (the trace's viol row and the score's vmax are one rule on one state)
    return lines


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    print("\n".join(run(b, k)))
