"""The Monte-Carlo comparison of examples/monte_carlo.py without any history: the tick keeps score.

The same fleet, the same two controller variants on common random numbers -- but the measure, per robot the sum over the ticks of
|position - goal|^2 + 1e-3 |u|^2, is handed to the library once:

  set_score(state_weights=[1, 1, 1, 0, 0, 0], control_weights=[1e-3] * 3, state_ref=goal, state_limits=(None, v_max))

and every tick of rollout() then updates one 64-byte record per robot on the device, against the plant's TRUE state.  rollout() is asked for
no x_hist and no u_hist; score() reads the records back (batch x 64 bytes) and score_summary() reduces them on the device to a few hundred
bytes -- mean, spread, worst robot, the share of robots that ever exceeded the velocity limit, the ticks held.  A caller of the C ABI gets the
same numbers from copra_batch_get_score / copra_batch_score_summary with no array library at all.

    python examples/monte_carlo_scores.py [batch] [ticks]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, workloads  # noqa: E402
from copra_amd.observer_design import kalman_gain  # noqa: E402

SIGMA_W = np.array([0.01, 0.01, 0.01, 0.005, 0.005, 0.005])
V_MAX = 0.6  # the velocity bound of workloads.com_preview: scored on the true state, which noise pushes across it


def closed_loop_scores(control_weight, batch, ticks, seed, load=0.004, sensor_noise=0.01):
    """(records, summary) of one closed-loop run -- the scenario of examples/monte_carlo.py::closed_loop_cost, line by line, up to the rollout"""
    wl = workloads.com_preview(batch)
    nx, nu, ny, N = 6, 3, 3, wl["N"]
    costs = [dict(c) for c in wl["costs"]]
    costs[1]["weights"] = [control_weight] * nu  # the variant
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
    eng.rollout(ticks, plant=(wl["A"], wl["B"], wl["d"] + c), stream=torch.cuda.current_stream().cuda_stream)  # no history at all
    return eng.score(), eng.score_summary()


def run(batch=4096, ticks=60, seed=2026):
    ra, sa = closed_loop_scores(1e-3, batch, ticks, seed)
    rb, sb = closed_loop_scores(1e-1, batch, ticks, seed)
    rc, _ = closed_loop_scores(1e-1, batch, ticks, seed + 1)  # the same variant on independent noise
    a, b, b_other = (r["jx"] + r["ju"] for r in (ra, rb, rc))
    diff, loose = b - a, b_other - a
    std = lambda s: float(np.sqrt(s["m2"] / max(s["n"] - 1, 1)))  # noqa: E731
    return dict(batch=batch, ticks=ticks, mean_cost_variant_a=float(a.mean()), mean_cost_variant_b=float(b.mean()),
                mean_difference=float(diff.mean()), difference_std_common_noise=float(diff.std(ddof=1)), difference_std_independent_noise=float(loose.std(ddof=1)),
                largest_per_robot_difference=float(np.abs(diff).max()), difference_of_the_first_robots=[round(float(v), 6) for v in diff[:6]],
                state_cost_a_from_the_summary="mean %.6g, std %.3g, worst %.6g (robot %d)" % (sa["jx"]["mean"], std(sa["jx"]), sa["jx"]["max"], sa["jx"]["argmax"]),
                state_cost_b_from_the_summary="mean %.6g, std %.3g, worst %.6g (robot %d)" % (sb["jx"]["mean"], std(sb["jx"]), sb["jx"]["max"], sb["jx"]["argmax"]),
                robots_over_the_velocity_limit="a: %d of %d, b: %d of %d (largest excess %.3g / %.3g)" % (sa["instances_violating"], batch, sb["instances_violating"], batch,
                                                                                                        sa["viol_max"]["max"], sb["viol_max"]["max"]),
                ticks_held="a: %d, b: %d" % (sa["held"], sb["held"]),
                bytes_read_back_per_run=batch * 64 + 336,
                bytes_the_histories_would_have_taken=8 * batch * ((ticks + 1) * 6 + ticks * 3))


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    for key, val in run(b, k).items():
        print("%-38s %s" % (key, val))
