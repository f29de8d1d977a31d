"""A constant load the model does not know: what the closed loop does about it.

Every robot of the CoM fleet carries a load of its own: its plant is the controller's model with a constant per-robot offset on d (a push on the
positions and the velocities at every tick).  The controller predicts with the d it was given, so

  without the estimator   every solve is wrong by the same amount at every tick and the robot settles beside its goal;
  with it                 set_bias_estimator(gain): after every tick the d of each robot's model moves by gain * (new state - the model's
                          prediction for the applied control), on the device, inside the plant-step kernel; the next solve reads it.  With
                          gain = 1 on every state and no noise the load is known after ONE tick; with noise a smaller gain averages.

Both runs are ONE rollout() each: the loop never returns to the host.  d_hist holds the estimates per tick.

    python examples/offset_free.py [batch] [ticks]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, workloads  # noqa: E402


def run(batch=4096, ticks=60, gain=None, load=0.004, noise=0.002, seed=0):
    dev = torch.device("cuda:0")
    wl = workloads.com_preview(batch)
    nx, nu, N = 6, 3, wl["N"]
    eng = BatchLMPC(nx, nu, N, batch, wl["costs"], wl["cstrs"])
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    rng = np.random.default_rng(seed)
    c = load * rng.uniform(-1.0, 1.0, (batch, nx))  # the load of each robot, constant over the run
    plant = (wl["A"], wl["B"], wl["d"] + c)  # numpy, natural indexing: copied to the device once
    if gain is not None:
        eng.set_bias_estimator(np.full(nx, float(gain)))  # one diagonal gain for the fleet
    gen = torch.Generator(device=dev).manual_seed(seed)
    w = torch.zeros((ticks, batch, nx), dtype=torch.float64, device=dev)
    w[:, :, :3] = noise * torch.randn(ticks, batch, 3, device=dev, generator=gen, dtype=torch.float64)
    hist = eng.rollout(ticks, plant=plant, disturbances=w, x_hist=True, status_hist=True, d_hist=gain is not None,
                       stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    goal = torch.tensor(np.asarray(wl["costs"][0]["p"], dtype=np.float64)[:3], device=dev)
    out = dict(batch=batch, ticks=ticks, gain=gain, failed_instance_ticks=int((hist["status_hist"] != 0).sum().item()),
               mean_distance_to_goal=float((hist["x_hist"][-1][:, :3] - goal).norm(dim=1).mean().item()))
    if gain is not None:
        err = eng.bias() - (wl["d"] + c)
        out["mean_abs_error_of_the_estimate"] = float(np.abs(err).mean())
        out["mean_abs_load"] = float(np.abs(c).mean())
    return out


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    print(run(b, k, gain=None))
    print(run(b, k, gain=0.5))
