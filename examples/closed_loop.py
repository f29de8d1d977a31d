"""The closed loops of examples/receding_horizon.py and examples/tracking.py on the engine's own tick: copra_batch_solve +
copra_batch_advance (BatchLMPC.advance) or, where nothing changes between ticks, ONE copra_batch_rollout call (BatchLMPC.rollout).

The plant update -- first control of the solve applied to the plant, a disturbance added, the result made the next initial state, an
instance whose QP failed keeping its state -- is one kernel of the library instead of five small torch kernels and a pointer hand-over; the
state lives in a buffer of the library and never visits the host.  Same workloads, same dictionaries as the two examples.

    python examples/closed_loop.py [batch] [ticks]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, workloads  # noqa: E402
from copra_amd.sharding import alloc_result_slab  # noqa: E402
from tracking import reference_window  # noqa: E402


def position_noise(ticks, batch, nx, noise, gen, dev):
    """(ticks, batch, nx): N(0, noise^2) on the three positions, nothing on the velocities (a state outside the velocity bound at step 0
    makes the QP infeasible: reference quirk Q5)"""
    w = torch.zeros((ticks, batch, nx), dtype=torch.float64, device=dev)
    w[:, :, :3] = noise * torch.randn(ticks, batch, 3, device=dev, generator=gen, dtype=torch.float64)
    return w


def run_receding_horizon(batch=16384, ticks=50, seed=0, noise=0.01, warm=False, v_max=0.6, u_max=3.0, rollout=True):
    """examples/receding_horizon.py::run -- a batch that shares one model; rollout=False: solve() + advance() per tick from Python"""
    dev = torch.device("cuda:0")
    wl = workloads.com_preview(batch, v_max=v_max, u_max=u_max)
    nx, nu, N = 6, 3, wl["N"]
    eng = BatchLMPC(nx, nu, N, batch, wl["costs"], wl["cstrs"])
    eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
    if warm:
        eng.set_warm_start(True)
    slab, out = alloc_result_slab(batch, nu * N, nx * (N + 1), dev)
    eng.set_outputs(out["control"], out["trajectory"], out["status"], out["iter"])
    eng.set_x0(torch.from_numpy(np.ascontiguousarray(wl["x0"])).to(dev))
    gen = torch.Generator(device=dev).manual_seed(seed)
    stream = torch.cuda.current_stream().cuda_stream
    goal = torch.tensor(workloads.COM_X_GOAL, device=dev)
    x = torch.empty((batch, nx), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w = position_noise(ticks, batch, nx, noise, gen, dev)  # (the disturbances of the whole run: part of the measured time)
    if rollout:
        eng.rollout(ticks, disturbances=w, x_out=x, stream=stream)
    else:
        for tick in range(ticks):
            eng.solve(stream)
            eng.advance(disturbance=w[tick], x_out=x if tick == ticks - 1 else None, stream=stream)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ok = int((out["status"] == 0).sum().item())
    dist = float((x[:, :3] - goal[:3]).norm(dim=1).mean().item())
    return dict(batch=batch, ticks=ticks, seconds=dt, ticks_per_s=ticks / dt, solves_per_s=batch * ticks / dt, solved_last_tick=ok,
                mean_distance_to_goal=dist, warm_start=warm, mean_iterations=None, mean_kernel_ms=None)


def run_tracking(batch=32768, ticks=50, seed=0, noise=0.002, per_instance=False, shared_model=False):
    """examples/tracking.py::run -- the window of the reference moves with set_cost_reference between advance() and solve()"""
    dev = torch.device("cuda:0")
    wl = workloads.com_preview(batch, v_max=0.6, u_max=3.0)
    nx, nu, N = 6, 3, wl["N"]
    track = dict(kind="trajectory", M=np.kron(np.eye(N + 1), np.eye(nx)), p=reference_window(0, N).reshape(-1),
                 weights=np.tile([10.0, 10.0, 10.0, 1.0, 1.0, 1.0], N + 1))
    eng = BatchLMPC(nx, nu, N, batch, [track, wl["costs"][1]], wl["cstrs"])
    slab, out = alloc_result_slab(batch, nu * N, nx * (N + 1), dev)
    eng.set_outputs(out["control"], out["trajectory"], out["status"], out["iter"])
    A, B, d = (torch.from_numpy(np.ascontiguousarray(np.swapaxes(wl[k], 1, 2) if wl[k].ndim == 3 else wl[k])).to(dev) for k in ("A", "B", "d"))
    x0 = torch.from_numpy(np.ascontiguousarray(wl["x0"])).to(dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    stream = torch.cuda.current_stream().cuda_stream
    if shared_model:
        eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
        eng.set_x0(x0)
    else:
        eng.set_system(A, B, d, x0)  # device tensors (column-major A, B), used in place; the states move into the library's buffer at the first tick
    own = torch.empty((batch, nx * (N + 1)), dtype=torch.float64, device=dev) if per_instance else None
    phase = torch.rand(batch, 1, device=dev, generator=gen, dtype=torch.float64) * 0.01 if per_instance else None
    x = torch.empty((batch, nx), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w = position_noise(ticks, batch, nx, noise, gen, dev)
    ref = None
    for tick in range(ticks):
        ref = torch.from_numpy(reference_window(tick, N).reshape(-1)).to(dev)
        if per_instance:
            own.copy_(ref[None, :].expand(batch, -1))
            own[:, 2::nx] += phase
            eng.set_cost_reference(0, own)
        else:
            eng.set_cost_reference(0, ref)
        eng.solve(stream)
        eng.advance(disturbance=w[tick], x_out=x if tick == ticks - 1 else None, stream=stream)
    err = float((x[:, :3] - ref[nx:nx + 3][None, :]).norm(dim=1).mean().item())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(batch=batch, ticks=ticks, per_instance_references=per_instance, shared_model=shared_model, seconds=dt, solves_per_s=batch * ticks / dt,
                solved_last_tick=int((out["status"] == 0).sum().item()), lane_pass=eng.lane_pass_info(), mean_position_error_last_tick=err)


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    run_receding_horizon(b, 5)  # (module load, LDS opt-in, first-solve set-up: outside the figures below)
    print(run_receding_horizon(b, k))
    print(run_receding_horizon(b, k, rollout=False))
    print(run_receding_horizon(b, k, warm=True))
    print(run_tracking(2 * b, k))
    print(run_tracking(2 * b, k, per_instance=True))
    print(run_tracking(2 * b, k, per_instance=True, shared_model=True))
