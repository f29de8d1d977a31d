"""An input delay of D ticks -- ignored, compensated, and absent.

In a real loop the solve, the bus and the drive take time: the command computed from the state at tick t reaches the plant at tick t + D.
The CoM fleet with D = 2, run three ways:

  naive         the delay sits in the plant and nobody compensates: the controller solves from the state it measures, and the command it
                issues is applied D ticks later.  Emulated with a delay-free handle whose result buffer gets, between solve() and
                advance(), the command issued D ticks ago in the place of the fresh one (a ring of tensors on the device);
  compensated   set_input_delay(D): the library queues the commands already issued and hands the solver the state PREDICTED for the time
                its command will act -- ONE rollout(), the loop never returns to the host;
  delay-free    D = 0, the loop of the other examples: what the compensated loop should look like, D ticks late.

Printed per run: the mean distance to the goal after the last tick, and from set_score the ticks and the robots that violated the velocity
bound (the workload's 0.6) on the true state.

    python examples/input_delay.py [batch] [ticks]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, workloads  # noqa: E402

D = 2
V_MAX = 0.6


def run(batch=4096, ticks=60, mode="compensated", noise=0.002, seed=0):
    wl = workloads.com_preview(batch, v_max=V_MAX)
    nx, nu, N = 6, 3, wl["N"]
    eng = BatchLMPC(nx, nu, N, batch, wl["costs"], wl["cstrs"])
    dev = torch.device("cuda:0")
    out = dict(control=torch.zeros((batch, nu * N), dtype=torch.float64, device=dev), trajectory=torch.zeros((batch, nx * (N + 1)), dtype=torch.float64, device=dev),
               status=torch.zeros(batch, dtype=torch.int32, device=dev), iter=torch.zeros((batch, 2), dtype=torch.int32, device=dev))
    eng.set_outputs(out["control"], out["trajectory"], out["status"], out["iter"])
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    goal = np.asarray(wl["costs"][0]["p"], dtype=np.float64)[:nx]
    inf = np.inf
    eng.set_score(state_weights=np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0]), state_ref=goal,
                  state_limits=(np.array([-inf] * 3 + [-V_MAX] * 3), np.array([inf] * 3 + [V_MAX] * 3)), tol=1e-6)
    gen = torch.Generator(device=dev).manual_seed(seed)
    w = torch.zeros((ticks, batch, nx), dtype=torch.float64, device=dev)
    w[:, :, :3] = noise * torch.randn(ticks, batch, 3, device=dev, generator=gen, dtype=torch.float64)
    stream = torch.cuda.current_stream().cuda_stream
    if mode == "compensated":
        eng.set_input_delay(D)
    if mode == "naive":
        ring = torch.zeros((D, batch, nu), dtype=torch.float64, device=dev)  # the commands on their way: zeros at first, as set_input_delay's
        ok = torch.ones((D, batch), dtype=torch.bool, device=dev)
        for t in range(ticks):
            eng.solve(stream)
            slot = t % D
            fresh, solved = out["control"][:, :nu].clone(), out["status"] == 0
            out["control"][:, :nu] = ring[slot]  # what reaches the plant now was issued D ticks ago
            out["status"].copy_(torch.where(ok[slot], 0, 1).to(torch.int32))
            ring[slot], ok[slot] = torch.where(solved[:, None], fresh, torch.zeros_like(fresh)), solved
            eng.advance(disturbance=w[t], stream=stream)
    else:
        eng.rollout(ticks, disturbances=w, stream=stream)
    torch.cuda.synchronize()
    x = eng.delay_state() if mode == "compensated" else eng.state()
    s = eng.score_summary()
    return dict(mode=mode, batch=batch, ticks=ticks, delay=0 if mode == "delay-free" else D,
                mean_distance_to_goal=float(np.linalg.norm(x[:, :3] - goal[:3], axis=1).mean()),
                violating_ticks=s["violating"], robots_that_violated=s["instances_violating"], largest_violation=s["viol_max"]["max"], held_ticks=s["held"])


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    for m in ("naive", "compensated", "delay-free"):
        print(run(b, k, m))
