"""Limits that MOVE during one rollout: a fleet whose actuators derate and whose speed limit tightens while the closed loop runs on the device.

The reference changes a limit by replacing the constraint object between solves; a host loop here would call set_control_bounds /
set_constraint_rhs every tick.  Instead the limit SIGNALS go to the controller once (BatchLMPC.set_control_bound_schedule,
set_constraint_schedule: one for the fleet, or one per robot) and rollout() enqueues ticks x (solve, plant step, next windows) on one stream.
The speed limit is a per-step TrajectoryConstraint (E = [0 I3], f = v_max): a constraint with stacked rows, which a schedule can move.  With
preview=True the horizon sees the future limits and brakes ahead of the corner; a limit that includes x_0 and falls below a robot's present
speed has no solution, so the signal stays above the speeds of the loop until the horizon has seen the corner coming.

    python examples/moving_limits.py [batch] [ticks]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, workloads  # noqa: E402


def run(batch=32768, ticks=50, per_robot=False, preview=True, noise=0.002, seed=0):
    dev = torch.device("cuda:0")
    wl = workloads.com_preview(batch, v_max=0.9, u_max=3.0)
    nx, nu, N = 6, 3, wl["N"]
    speed = dict(kind="trajectory", E=np.hstack([np.zeros((3, 3)), np.eye(3)]), f=[0.9] * 3)
    eng = BatchLMPC(nx, nu, N, batch, wl["costs"], [speed, wl["cstrs"][1]])
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    steps = ticks + N + 1
    k = np.arange(steps)
    u_max = np.repeat((3.0 - 2.0 * np.minimum(k, ticks) / ticks)[:, None], 3, axis=1)  # the actuators derate from 3.0 to 1.0 over the run
    v_max = np.repeat(np.where(k < ticks, 0.9, 0.3)[:, None], 3, axis=1)  # the corner behind the last tick: the horizon sees it N ticks ahead
    lo, up, vm = (torch.from_numpy(a).to(dev) for a in (-u_max, u_max, v_max))
    if per_robot:  # every robot its own signals, device tensors used in place
        gen = torch.Generator(device=dev).manual_seed(seed)
        scale = 1.0 + 0.1 * torch.rand(batch, 1, 1, device=dev, generator=gen, dtype=torch.float64)
        lo, up, vm = (scale * a[None, :, :] for a in (lo, up, vm))
        lo, up, vm = lo.contiguous(), up.contiguous(), vm.contiguous()
    eng.set_control_bound_schedule(lo, up, preview=preview)
    eng.set_constraint_schedule(0, vm, 3, preview=preview)
    w = torch.zeros((ticks, batch, nx), dtype=torch.float64, device=dev)
    w[:, :, :3] = noise * torch.randn(ticks, batch, 3, device=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hist = eng.rollout(ticks, disturbances=w, u_hist=True, status_hist=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    u_last = hist["u_hist"][-1].abs().max().item()
    return dict(batch=batch, ticks=ticks, per_robot_signals=per_robot, preview=preview, seconds=dt, solves_per_s=batch * ticks / dt,
                solved_every_tick=bool((hist["status_hist"] == 0).all().item()), largest_control_last_tick=u_last,
                actuator_limit_last_tick=float(u_max[ticks - 1, 0]) * (1.1 if per_robot else 1.0), schedule_tick=eng.schedule_tick())


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    run(b, 5)  # (module load, LDS opt-in, first-solve set-up: outside the figures below)
    print(run(b, k))
    print(run(b, k, per_robot=True))
    print(run(b, k, preview=False))
