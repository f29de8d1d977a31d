"""Monte-Carlo comparison of two controllers on common random numbers.

The fleet of examples/output_feedback.py -- positions measured with noise, an unknown constant load, a wrong first idea of the velocities --
is run twice, once per controller variant (here: two weights of the control cost).  Process and sensor noise are drawn ON THE DEVICE:

  set_noise(seed, process=sigma_w, sensor=sigma_v)   every tick draws w and v inside the plant-step kernel from a counter-based generator:
                                                     robot b at tick t gets the same draw in both runs, whatever the controller did before,
                                                     and no [ticks][batch][nx] array of noise exists anywhere.

Because both variants see the same noise, the per-robot DIFFERENCE of their closed-loop costs is free of the scatter that independent noise
would put into it -- how much that is depends on how much of the cost's scatter is noise, so the same difference on an independent seed is
printed beside it.  The whole run of a variant is ONE rollout().

    python examples/monte_carlo.py [batch] [ticks]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, workloads  # noqa: E402
from copra_amd.observer_design import kalman_gain  # noqa: E402

SIGMA_W = np.array([0.01, 0.01, 0.01, 0.005, 0.005, 0.005])


def closed_loop_cost(control_weight, batch, ticks, seed, load=0.004, sensor_noise=0.01):
    """per-robot cost of one closed-loop run: sum over the ticks of |position - goal|^2 + 1e-3 |u|^2 (the SAME measure for every variant)"""
    dev = torch.device("cuda:0")
    wl = workloads.com_preview(batch)
    nx, nu, ny, N = 6, 3, 3, wl["N"]
    costs = [dict(c) for c in wl["costs"]]
    costs[1]["weights"] = [control_weight] * nu  # the variant
    rng = np.random.default_rng(0)  # (the scenario -- loads, first estimates -- is the same for every variant and seed)
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
    eng.set_noise(seed, process=SIGMA_W, sensor=np.full(ny, sensor_noise))  # after set_observer: the sensor stream needs its ny
    hist = eng.rollout(ticks, plant=(wl["A"], wl["B"], wl["d"] + c), x_hist=True, u_hist=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert eng.noise_tick == ticks
    goal = torch.tensor(np.asarray(wl["costs"][0]["p"], dtype=np.float64)[:3], device=dev)
    u = torch.nan_to_num(hist["u_hist"])  # (a held robot applied nothing)
    return ((hist["x_hist"][1:, :, :3] - goal) ** 2).sum(dim=(0, 2)) + 1e-3 * (u ** 2).sum(dim=(0, 2))


def run(batch=4096, ticks=60, seed=2026):
    a = closed_loop_cost(1e-3, batch, ticks, seed)
    b = closed_loop_cost(1e-1, batch, ticks, seed)
    b_other = closed_loop_cost(1e-1, batch, ticks, seed + 1)  # the same variant on independent noise: what a comparison without a seed sees
    diff, loose = b - a, b_other - a
    return dict(batch=batch, ticks=ticks, mean_cost_variant_a=float(a.mean()), mean_cost_variant_b=float(b.mean()),
                mean_difference=float(diff.mean()), difference_std_common_noise=float(diff.std()), difference_std_independent_noise=float(loose.std()),
                largest_per_robot_difference=float(diff.abs().max()), difference_of_the_first_robots=[round(v, 6) for v in diff[:6].tolist()])


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    for key, val in run(b, k).items():
        print("%-34s %s" % (key, val))
