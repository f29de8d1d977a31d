"""Tracking-loop rates: the host-driven loop that existed before reference schedules against ONE rollout on a schedule, on the tracking
controller of examples/tracking.py (the headline shape with a full-size TrajectoryCost that follows a circle).

    python tools/bench_tracking_loop.py [--ticks 200] [--reps 5] [--out profiles/closed_loop/tracking_rates.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_tracking_loop.py --trace 65536 [--per-instance]   (the window kernel's own time)

Per size and kind of schedule, `reps` alternating runs of
  (a) host:    per tick the window of the reference is built on the host and copied to the device (per-instance: written out per instance with
               torch, as examples/tracking.py does), set_cost_reference(0, window); solve(); advance(disturbance=w[t])
  (b) rollout: the signal handed over once (set_reference_schedule, a device tensor), per run schedule_seek(0) and ONE rollout(ticks, disturbances=w)
on ONE controller each (created and warmed up outside the timed region, state and tick counter reset before every run), per-instance systems
as device tensors, position noise 0.002.  Medians and the spread (min .. max) of the runs are printed; host time around a final synchronisation.
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
sys.path.insert(0, os.path.join(ROOT, "examples"))
from copra_amd import BatchLMPC, _capi, workloads  # noqa: E402
from copra_amd.sharding import alloc_result_slab  # noqa: E402
from tracking_rollout import reference_signal  # noqa: E402

NX, NU, NOISE = 6, 3, 0.002


class Loop:
    def __init__(self, batch, per_instance, ticks):
        self.dev = torch.device("cuda:0")
        self.batch, self.per_instance = batch, per_instance
        wl = workloads.com_preview(batch, v_max=0.6, u_max=3.0)
        self.N = N = wl["N"]
        self.signal = reference_signal(ticks + N + 1)
        track = dict(kind="trajectory", M=np.kron(np.eye(N + 1), np.eye(NX)), p=self.signal[:N + 1].reshape(-1),
                     weights=np.tile([10.0, 10.0, 10.0, 1.0, 1.0, 1.0], N + 1))
        self.eng = BatchLMPC(NX, NU, N, batch, [track, wl["costs"][1]], wl["cstrs"])
        self.slab, self.out = alloc_result_slab(batch, NU * N, NX * (N + 1), self.dev)
        self.eng.set_outputs(self.out["control"], self.out["trajectory"], self.out["status"], self.out["iter"])
        self.A, self.B, self.d = (torch.from_numpy(np.ascontiguousarray(np.swapaxes(wl[k], 1, 2) if wl[k].ndim == 3 else wl[k])).to(self.dev)
                                  for k in ("A", "B", "d"))
        self.x_start = torch.from_numpy(np.ascontiguousarray(wl["x0"])).to(self.dev)
        self.gen = torch.Generator(device=self.dev).manual_seed(0)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.phase = torch.rand(batch, 1, device=self.dev, generator=self.gen, dtype=torch.float64) * 0.01
        self.own = torch.empty((batch, NX * (N + 1)), dtype=torch.float64, device=self.dev) if per_instance else None
        self.sched = None

    def schedule(self):
        """the signal on the device, handed over once"""
        if self.sched is None:
            s = torch.from_numpy(self.signal).to(self.dev)
            if self.per_instance:
                s = s[None, :, :].repeat(self.batch, 1, 1)
                s[:, :, 2] += self.phase
            self.sched = s
            self.eng.set_reference_schedule(0, s, NX)
        return self.sched

    def disturbances(self, ticks):
        w = torch.zeros((ticks, self.batch, NX), dtype=torch.float64, device=self.dev)
        w[:, :, :3] = NOISE * torch.randn(ticks, self.batch, 3, device=self.dev, generator=self.gen, dtype=torch.float64)
        return w

    def run(self, variant, ticks):
        eng, stream, N = self.eng, self.stream, self.N
        x = self.x_start.clone()
        eng.set_system(self.A, self.B, self.d, x)
        w = self.disturbances(ticks)
        if variant == "rollout":
            self.schedule()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if variant == "host":
            for t in range(ticks):
                ref = torch.from_numpy(self.signal[t:t + N + 1].reshape(-1)).to(self.dev)
                if self.per_instance:
                    self.own.copy_(ref[None, :].expand(self.batch, -1))
                    self.own[:, 2::NX] += self.phase
                    eng.set_cost_reference(0, self.own)
                else:
                    eng.set_cost_reference(0, ref)
                eng.solve(stream)
                eng.advance(disturbance=w[t], stream=stream)
        else:
            eng.schedule_seek(0)
            eng.rollout(ticks, disturbances=w, stream=stream)
        torch.cuda.synchronize()
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", type=int, default=0, help="only one rollout of `ticks` ticks at this batch size (for a kernel trace)")
    ap.add_argument("--per-instance", action="store_true", help="with --trace: per-instance schedules")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.trace:
        loop = Loop(args.trace, args.per_instance, args.ticks)
        loop.run("rollout", 5)
        loop.run("rollout", args.ticks)
        W = 8 * NX * (loop.N + 1)
        say("trace: one rollout of %d ticks at %d instances, %s; copra_ref_window_kernel writes %d B per instance and tick (%.1f MB per tick) and reads %s"
            % (args.ticks, args.trace, "per-instance schedules" if args.per_instance else "one schedule", W, W * args.trace / 1e6,
               "as much" if args.per_instance else "%d B per workgroup" % W))
        return
    say("tracking loop, CoM controller (xDim 6, uDim 3, N 20) with a reference trajectory, %d ticks per run, %d alternating runs; M solves/s: median (min .. max)"
        % (args.ticks, args.reps))
    say("library source hash %s" % _capi.library_source_hash())
    for batch in (16384, 65536):
        for per_instance in (False, True):
            loops = {v: Loop(batch, per_instance, args.ticks) for v in ("host", "rollout")}
            for v, lp in loops.items():  # module load, LDS opt-in, first-solve set-up, the engine's adaptation
                lp.run(v, 10)
            rates = {v: [] for v in loops}
            for _ in range(args.reps):
                for v, lp in loops.items():
                    rates[v].append(batch * args.ticks / lp.run(v, args.ticks) / 1e6)
            say("batch %d, %s" % (batch, "per-instance schedules" if per_instance else "one schedule for the batch"))
            for v in loops:
                r = rates[v]
                say("  (%s) %-8s %8.1f  (%8.1f .. %8.1f)" % ("a" if v == "host" else "b", v, statistics.median(r), min(r), max(r)))
            a, b = statistics.median(rates["host"]), statistics.median(rates["rollout"])
            say("  rollout / host = %.3f: %s" % (b / a, "faster" if b > 1.02 * a else "within the 2 %% run-to-run spread" if b >= 0.98 * a else "SLOWER"))
            del loops
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
