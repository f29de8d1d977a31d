"""A solve that fails for a few ticks: what the closed loop applies meanwhile.

The CoM fleet runs under a speed limit that follows a schedule WITHOUT preview (BatchLMPC.set_constraint_schedule(..., preview=False)): at tick
`drop` the limit falls from 0.9 to 0.3 for `dip` ticks and comes back.  The limit includes x_0, so every robot that is faster than 0.3 at that
moment has no solution until the limit is back -- an ordinary event, not an error.  What the tick does with such a robot:

  hold          its state is kept (nothing is applied: the loop pretends the robot stands still in time), or
  backup plan   set_backup_steps(3): it keeps applying u_1, u_2, u_3 of the last plan that did solve -- what every receding-horizon controller
                in use does -- and only a robot whose plan is used up is held.

Both runs are ONE rollout() each; age_hist says per robot and tick where the applied control came from (0: this tick's solve, j >= 1: step j of
the stored plan, -2: held).

    python examples/backup_plan.py [batch] [ticks]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, _capi, workloads  # noqa: E402


def run(batch=4096, ticks=30, backup_steps=0, drop=8, dip=3, noise=0.002, seed=0):
    dev = torch.device("cuda:0")
    wl = workloads.com_preview(batch, v_max=0.9, u_max=3.0)
    nx, nu, N = 6, 3, wl["N"]
    speed = dict(kind="trajectory", E=np.hstack([np.zeros((3, 3)), np.eye(3)]), f=[0.9] * 3)  # a constraint with stacked rows: a schedule can move it
    eng = BatchLMPC(nx, nu, N, batch, wl["costs"], [speed, wl["cstrs"][1]])
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    k = np.arange(ticks + 1)
    v_max = np.repeat(np.where((k >= drop) & (k < drop + dip), 0.3, 0.9)[:, None], 3, axis=1)
    eng.set_constraint_schedule(0, v_max, 3, preview=False)  # the limit of the present tick at every step of the horizon: nobody sees the dip coming
    eng.set_backup_steps(backup_steps)
    gen = torch.Generator(device=dev).manual_seed(seed)
    w = torch.zeros((ticks, batch, nx), dtype=torch.float64, device=dev)
    w[:, :, :3] = noise * torch.randn(ticks, batch, 3, device=dev, generator=gen, dtype=torch.float64)
    hist = eng.rollout(ticks, disturbances=w, x_hist=True, status_hist=True, age_hist=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    age, status = hist["age_hist"], hist["status_hist"]
    goal = torch.tensor(np.asarray(wl["costs"][0]["p"], dtype=np.float64)[:3], device=dev)
    return dict(batch=batch, ticks=ticks, backup_steps=backup_steps, limit_low_at_ticks=(drop, drop + dip),
                failed_instance_ticks=int((status != 0).sum().item()), held_instance_ticks=int((age == _capi.PLAN_HELD).sum().item()),
                played_from_a_plan=int((age >= 1).sum().item()),
                mean_distance_to_goal=float((hist["x_hist"][-1][:, :3] - goal).norm(dim=1).mean().item()))


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    print(run(b, k, backup_steps=0))
    print(run(b, k, backup_steps=3))
