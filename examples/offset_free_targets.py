"""A constant load, the estimator -- and the steady-state targets that make the loop offset-free.

The fleet of examples/offset_free.py with gain = 1: after one tick every robot's model knows its load.  That alone does not take the robot
to its goal: the workload pairs a TrajectoryCost towards the goal (with the goal's velocities) with a ControlCost whose reference is zero,
and under a constant load the equilibrium control is not zero -- the two costs pull against each other and the loop settles beside the goal
however good the estimate is.  The target calculator recomputes, per robot and per tick, the steady state (xs, us) that is consistent with
the model, its current d and the setpoint on the positions, and makes it the reference of both costs:

  as it is         set_bias_estimator(gain) alone;
  with targets     ... and set_target(outputs, setpoint, costs=[0, 1]): a kernel of its own behind every plant step, on the device.

Both runs are ONE rollout() each: the loop never returns to the host.

    python examples/offset_free_targets.py [batch] [ticks]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, workloads  # noqa: E402


def run(batch=4096, ticks=60, targets=False, gain=1.0, load=0.004, seed=0):
    wl = workloads.com_preview(batch)
    nx, nu, N = 6, 3, wl["N"]
    eng = BatchLMPC(nx, nu, N, batch, wl["costs"], wl["cstrs"])
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    rng = np.random.default_rng(seed)
    c = load * rng.uniform(-1.0, 1.0, (batch, nx))  # the load of each robot, constant over the run
    plant = (wl["A"], wl["B"], wl["d"] + c)
    eng.set_bias_estimator(np.full(nx, float(gain)))
    goal = np.asarray(wl["costs"][0]["p"], dtype=np.float64)[:3]
    if targets:
        eng.set_target(np.eye(nx)[:nu], goal, costs=[0, 1])  # the positions are the controlled outputs, the goal their setpoint
    hist = eng.rollout(ticks, plant=plant, x_hist=True, status_hist=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = torch.tensor(goal, device=hist["x_hist"].device)
    out = dict(batch=batch, ticks=ticks, targets=targets, failed_instance_ticks=int((hist["status_hist"] != 0).sum().item()),
               mean_distance_to_goal=float((hist["x_hist"][-1][:, :3] - g).norm(dim=1).mean().item()))
    if targets:
        out["singular_instances"] = int(eng.target_status().sum())
        out["mean_abs_steady_control"] = float(np.abs(eng.target()[:, nx:]).mean())
    return out


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    print(run(b, k, targets=False))
    print(run(b, k, targets=True))
