"""Closed-loop tick rates: the plant update in torch (as examples/receding_horizon.py and examples/tracking.py do it) against the engine's
own tick (copra_batch_advance, copra_batch_rollout), on the CoM controller at the examples' sizes.

    python tools/bench_closed_loop.py [--ticks 200] [--reps 5] [--out profiles/closed_loop/tick_rates.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_closed_loop.py --trace 65536      (the advance kernel's own time)

Per size, `reps` alternating runs of
  (a) torch:   solve; pred = trajectory[:, nx:2nx].clone(); pred[:, :3] += noise * randn; x = where(status == 0, pred, x).contiguous(); set_x0 / set_system
  (b) advance: w = noise * randn for the whole run; per tick solve(); advance(disturbance=w[t])
  (c) rollout: w as in (b); ONE rollout(ticks, disturbances=w)
  (s) solver:  solve() alone, the state never moves -- the rate the ticks are compared with
on ONE controller each (created and warmed up outside the timed region, its state reset before every run).  16 384 instances share one model
(copra_batch_set_shared_system, noise 0.01: receding_horizon.py); 32 768 and 65 536 have per-instance systems (device tensors, noise 0.002:
tracking.py).  Medians and the spread (min .. max) of the runs are printed; host time around a final synchronisation.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from copra_amd import BatchLMPC, workloads  # noqa: E402
from copra_amd.sharding import alloc_result_slab  # noqa: E402

NX, NU = 6, 3


class Loop:
    def __init__(self, batch, shared):
        self.dev = torch.device("cuda:0")
        self.batch, self.shared = batch, shared
        self.noise = 0.01 if shared else 0.002
        wl = workloads.com_preview(batch)
        self.N = wl["N"]
        self.eng = BatchLMPC(NX, NU, self.N, batch, wl["costs"], wl["cstrs"])
        self.slab, self.out = alloc_result_slab(batch, NU * self.N, NX * (self.N + 1), self.dev)
        self.eng.set_outputs(self.out["control"], self.out["trajectory"], self.out["status"], self.out["iter"])
        self.A, self.B, self.d = (torch.from_numpy(np.ascontiguousarray(np.swapaxes(wl[k], 1, 2) if wl[k].ndim == 3 else wl[k])).to(self.dev)
                                  for k in ("A", "B", "d"))
        self.x_start = torch.from_numpy(np.ascontiguousarray(wl["x0"])).to(self.dev)
        if shared:
            self.eng.set_shared_system(wl["A"][0], wl["B"][0], wl["d"][0])
        self.gen = torch.Generator(device=self.dev).manual_seed(0)
        self.stream = torch.cuda.current_stream().cuda_stream

    def hand_over(self, x):
        if self.shared:
            self.eng.set_x0(x)
        else:
            self.eng.set_system(self.A, self.B, self.d, x)

    def disturbances(self, ticks):
        w = torch.zeros((ticks, self.batch, NX), dtype=torch.float64, device=self.dev)
        w[:, :, :3] = self.noise * torch.randn(ticks, self.batch, 3, device=self.dev, generator=self.gen, dtype=torch.float64)
        return w

    def run(self, variant, ticks):
        eng, out, stream = self.eng, self.out, self.stream
        x = self.x_start.clone()
        self.hand_over(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if variant == "torch":
            for _ in range(ticks):
                self.hand_over(x)
                eng.solve(stream)
                pred = out["trajectory"][:, NX:2 * NX].clone()
                pred[:, :3] += self.noise * torch.randn(self.batch, 3, device=self.dev, generator=self.gen, dtype=torch.float64)
                x = torch.where((out["status"] == 0)[:, None], pred, x).contiguous()
        elif variant == "advance":
            w = self.disturbances(ticks)
            for t in range(ticks):
                eng.solve(stream)
                eng.advance(disturbance=w[t], stream=stream)
        elif variant == "rollout":
            eng.rollout(ticks, disturbances=self.disturbances(ticks), stream=stream)
        else:
            for _ in range(ticks):
                eng.solve(stream)
        torch.cuda.synchronize()
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0, help="only `ticks` solve + advance ticks at this batch size (for a kernel trace)")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.trace:
        loop = Loop(args.trace, shared=args.trace <= 16384)
        loop.run("advance", 5)
        loop.run("advance", args.ticks)
        per = 8 * (NX * NX + NX * NU + NX) * (0 if loop.shared else 1) + 8 * (2 * NX + NU) + 4
        say("trace: %d ticks of solve + advance at %d instances; copra_plant_step_kernel reads %d B and writes %d B per instance and tick"
            % (args.ticks, args.trace, per, 8 * NX))
        return
    variants = ("torch", "advance", "rollout", "solver")
    say("closed-loop ticks, CoM controller (xDim 6, uDim 3, N 20), %d ticks per run, %d alternating runs; M solves/s: median (min .. max)" % (args.ticks, args.reps))
    for batch, shared in ((16384, True), (32768, False), (65536, False)):
        loops = {v: Loop(batch, shared) for v in variants}
        for v in variants:  # module load, LDS opt-in, first-solve set-up, the engine's adaptation
            loops[v].run(v, 10)
        rates = {v: [] for v in variants}
        for _ in range(args.reps):
            for v in variants:
                rates[v].append(batch * args.ticks / loops[v].run(v, args.ticks) / 1e6)
        say("batch %d, %s" % (batch, "one shared model" if shared else "per-instance systems"))
        for v in variants:
            r = rates[v]
            say("  %-8s %8.1f  (%8.1f .. %8.1f)" % (v, statistics.median(r), min(r), max(r)))
        spread = max(rates["torch"]) - min(rates["torch"])
        for v in ("advance", "rollout"):
            gain = statistics.median(rates[v]) - statistics.median(rates["torch"])
            say("  %s - torch = %+.1f M solves/s (spread of the torch runs: %.1f): %s" % (v, gain, spread, "faster" if gain > spread else "NOT faster beyond the spread"))
        say("  rollout / solver = %.2f" % (statistics.median(rates["rollout"]) / statistics.median(rates["solver"])))
        del loops
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
