"""Output feedback: the controller never sees the state, only the positions.

Every robot of the CoM fleet has encoders on its three positions (ny = 3 of nx = 6) with a little noise, and carries a constant load its
model does not know (a push on the velocities at every tick).  The controller starts with a wrong idea of the velocities.

  set_observer(C, Lx, Ld)   after every tick the plant moves its OWN state; the outputs y = C xp+ + v are formed, and the estimate the next
                            solve reads is corrected by Lx (y - C xpred), the model's d by Ld (y - C xpred) -- on the device, inside the
                            plant-step kernel.  The gains are the steady-state Kalman filter's (observer_design.kalman_gain) for the model
                            augmented with a force-like disturbance on the velocities.

The whole run is ONE rollout(): the loop never returns to the host.  x_hist is the truth, xhat_hist what the controller believed.

    python examples/output_feedback.py [batch] [ticks]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, workloads  # noqa: E402
from copra_amd.observer_design import kalman_gain  # noqa: E402


def run(batch=4096, ticks=60, load=0.004, sensor_noise=0.002, seed=0):
    dev = torch.device("cuda:0")
    wl = workloads.com_preview(batch)
    nx, nu, ny, N = 6, 3, 3, wl["N"]
    rng = np.random.default_rng(seed)
    eng = BatchLMPC(nx, nu, N, batch, wl["costs"], wl["cstrs"])
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])  # the true start ...
    C = np.eye(nx)[:ny]  # positions only
    G = np.zeros((nx, ny))
    G[3:] = np.eye(3)  # the disturbance the observer looks for: a push on the velocities
    Lx, Ld = kalman_gain(wl["A"], C, 1e-4 * np.eye(nx), sensor_noise ** 2 * np.eye(ny) + 1e-4 * np.eye(ny), with_bias=True, Qd=1e-5 * np.eye(ny), Gd=G)
    eng.set_observer(C, Lx, Ld)  # ... becomes the plant's own state; one gain per robot (its sampling period is its own)
    xhat0 = wl["x0"].copy()
    xhat0[:, 3:] += 0.1 * rng.choice([-1.0, 1.0], (batch, 3))  # what the controller believes: velocities off by 0.1 m/s
    eng.set_x0(xhat0)
    c = np.zeros((batch, nx))
    c[:, 3:] = load * rng.uniform(-1.0, 1.0, (batch, 3))  # the load of each robot, constant over the run
    plant = (wl["A"], wl["B"], wl["d"] + c)
    gen = torch.Generator(device=dev).manual_seed(seed)
    v = sensor_noise * torch.randn(ticks, batch, ny, device=dev, generator=gen, dtype=torch.float64)
    hist = eng.rollout(ticks, plant=plant, noise=v, x_hist=True, xhat_hist=True, d_hist=True, status_hist=True,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    goal = torch.tensor(np.asarray(wl["costs"][0]["p"], dtype=np.float64)[:3], device=dev)
    truth, est, dh = hist["x_hist"], hist["xhat_hist"], hist["d_hist"]
    cd = torch.from_numpy(wl["d"] + c).to(dev)
    out = dict(batch=batch, ticks=ticks, failed_instance_ticks=int((hist["status_hist"] != 0).sum().item()))
    for name, t in (("first", 0), ("last", ticks - 1)):
        out["estimation_error_%s_tick" % name] = float((est[t] - truth[t + 1]).abs().mean().item())
        out["load_estimate_error_%s_tick" % name] = float((dh[t] - cd)[:, 3:].abs().mean().item())
        out["offset_from_goal_%s_tick" % name] = float((truth[t + 1][:, :3] - goal).norm(dim=1).mean().item())
    return out


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    for key, val in run(b, k).items():
        print("%-34s %s" % (key, val))
