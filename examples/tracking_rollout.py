"""Closed-loop TRACKING of a moving reference trajectory in ONE call: the controller of examples/tracking.py, driven by copra_batch_rollout.

examples/tracking.py returns to the host every tick: it builds the window of the reference that the horizon sees, hands it over
(copra_batch_set_cost_reference / _all), solves and moves the states with torch.  Here the whole reference SIGNAL goes to the controller once
(BatchLMPC.set_reference_schedule: one for the batch, or `per_instance=True` one per instance -- the shared signal plus the instance's own
offset in height); rollout() then enqueues ticks x (solve, plant step, next window) on one stream and the host is not needed again.

    python examples/tracking_rollout.py [batch] [ticks]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, workloads  # noqa: E402
from copra_amd.sharding import alloc_result_slab  # noqa: E402


def reference_signal(steps, T=0.117, speed=0.4):
    """examples/tracking.py::reference_window as one signal: block k is the state asked for at time k T; (steps, 6)"""
    t = T * np.arange(steps)
    c = workloads.COM_X_INIT[:3] + np.array([0.0, 0.0, workloads.COM_X_GOAL[2] - workloads.COM_X_INIT[2]])
    r, w = 0.05, speed
    pos = c[None, :] + r * np.stack([np.cos(w * t), np.sin(w * t), 0.0 * t], axis=1)
    vel = r * w * np.stack([-np.sin(w * t), np.cos(w * t), 0.0 * t], axis=1)
    return np.hstack([pos, vel])


def run(batch=32768, ticks=50, seed=0, noise=0.002, per_instance=False, shared_model=False):
    dev = torch.device("cuda:0")
    wl = workloads.com_preview(batch, v_max=0.6, u_max=3.0)
    nx, nu, N = 6, 3, wl["N"]
    signal = reference_signal(ticks + N + 1)
    track = dict(kind="trajectory", M=np.kron(np.eye(N + 1), np.eye(nx)), p=signal[:N + 1].reshape(-1),
                 weights=np.tile([10.0, 10.0, 10.0, 1.0, 1.0, 1.0], N + 1))
    eng = BatchLMPC(nx, nu, N, batch, [track, wl["costs"][1]], wl["cstrs"])
    slab, out = alloc_result_slab(batch, nu * N, nx * (N + 1), dev)
    eng.set_outputs(out["control"], out["trajectory"], out["status"], out["iter"])
    gen = torch.Generator(device=dev).manual_seed(seed)
    if shared_model:  # a fleet of identical plants: ONE model for the batch, only the states and the references differ
        eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
        eng.set_x0(wl["x0"])
    else:
        eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    sched = torch.from_numpy(signal).to(dev)
    if per_instance:  # every instance its own signal, a device tensor used in place
        phase = torch.rand(batch, 1, device=dev, generator=gen, dtype=torch.float64) * 0.01
        sched = sched[None, :, :].repeat(batch, 1, 1)
        sched[:, :, 2] += phase
    eng.set_reference_schedule(0, sched, nx)  # r = 6 rows per step, S = N + 1 steps in the window, offset 0
    w = torch.zeros((ticks, batch, nx), dtype=torch.float64, device=dev)
    w[:, :, :3] = noise * torch.randn(ticks, batch, 3, device=dev, generator=gen, dtype=torch.float64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.rollout(ticks, disturbances=w, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    x = torch.from_numpy(eng.state()).to(dev)
    goal = sched[..., ticks, :3]  # the block the state after `ticks` steps was asked to reach
    err = float((x[:, :3] - goal).norm(dim=1).mean().item())
    return dict(batch=batch, ticks=ticks, per_instance_schedules=per_instance, shared_model=shared_model, seconds=dt, solves_per_s=batch * ticks / dt,
                solved_last_tick=int((out["status"] == 0).sum().item()), schedule_tick=eng.schedule_tick(), mean_position_error_last_tick=err)


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    run(b, 5)  # (module load, LDS opt-in, first-solve set-up: outside the figures below)
    print(run(b, k))
    print(run(b, k, per_instance=True))
    print(run(b, k, per_instance=True, shared_model=True))  # (a fleet of identical plants, every one on its own path)
