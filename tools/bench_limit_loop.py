"""Moving-limit loop rates: the host-driven loop that existed before limit schedules against ONE rollout on limit schedules, on the headline
shape (CoM controller, xDim 6, uDim 3, N 20) with the velocity row as a TrajectoryConstraint and a ControlBoundConstraint.

    python tools/bench_limit_loop.py [--ticks 200] [--reps 5] [--out profiles/closed_loop/limit_rates.txt]

Per size, `reps` alternating runs of
  (a) host:    per tick set_control_bounds(window of the tick) and set_constraint_rhs(0, window of the tick) from host arrays, solve(),
               advance(disturbance=w[t]) -- on a controller created with the FULL-SIZE TrajectoryConstraint, which takes a right-hand side per step
  (b) rollout: the signals handed over once (set_control_bound_schedule, set_constraint_schedule: per-instance device tensors), per run
               schedule_seek(0) and ONE rollout(ticks, disturbances=w)
on ONE controller each (created and warmed up outside the timed region, state and tick counter reset before every run), per-instance systems
as device tensors, position noise 0.002, preview on.  Medians and the spread (min .. max) of the runs are printed; host time around a final
synchronisation.  The window kernel's own time: events around `ticks` calls of schedule_seek, which launch nothing but the windows.
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
from copra_amd import BatchLMPC, _capi, workloads  # noqa: E402

NX, NU, NOISE = 6, 3, 0.002


def signals(batch, steps, ticks):
    """per-instance limits: the actuator derates from 3.0 to 2.0, the speed limit tightens from 0.9 to 0.75 over the run"""
    k = np.minimum(np.arange(steps), ticks) / float(ticks)
    scale = 1.0 + 0.1 * (np.arange(batch) % 4)[:, None, None]
    up = scale * np.repeat((3.0 - 1.0 * k)[:, None], 3, axis=1)[None]
    v = scale * np.repeat((0.9 - 0.15 * k)[:, None], 3, axis=1)[None]
    return np.ascontiguousarray(up), np.ascontiguousarray(v)


class Loop:
    def __init__(self, batch, variant, ticks):
        self.dev = torch.device("cuda:0")
        self.batch, self.variant = batch, variant
        wl = workloads.com_preview(batch, v_max=0.9, u_max=3.0)
        self.N = N = wl["N"]
        E = np.hstack([np.zeros((3, 3)), np.eye(3)])
        if variant == "host":
            speed = dict(kind="trajectory", E=np.kron(np.eye(N + 1), E), f=[0.9] * (3 * (N + 1)))
        else:
            speed = dict(kind="trajectory", E=E, f=[0.9] * 3)
        self.eng = BatchLMPC(NX, NU, N, batch, wl["costs"], [speed, wl["cstrs"][1]])
        self.A, self.B, self.d = (torch.from_numpy(np.ascontiguousarray(np.swapaxes(wl[k], 1, 2) if wl[k].ndim == 3 else wl[k])).to(self.dev)
                                  for k in ("A", "B", "d"))
        self.x_start = torch.from_numpy(np.ascontiguousarray(wl["x0"])).to(self.dev)
        self.gen = torch.Generator(device=self.dev).manual_seed(0)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.up, self.v = signals(batch, ticks + N + 1, ticks)
        self.sched = None

    def schedules(self):
        if self.sched is None:
            up, v = torch.from_numpy(self.up).to(self.dev), torch.from_numpy(self.v).to(self.dev)
            self.sched = ((-up).contiguous(), up, v)
            self.eng.set_control_bound_schedule(self.sched[0], self.sched[1])
            self.eng.set_constraint_schedule(0, v, 3)

    def run(self, ticks):
        eng, stream, N = self.eng, self.stream, self.N
        eng.set_system(self.A, self.B, self.d, self.x_start.clone())
        w = torch.zeros((ticks, self.batch, NX), dtype=torch.float64, device=self.dev)
        w[:, :, :3] = NOISE * torch.randn(ticks, self.batch, 3, device=self.dev, generator=self.gen, dtype=torch.float64)
        if self.variant == "rollout":
            self.schedules()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if self.variant == "host":
            for t in range(ticks):
                up = self.up[:, t:t + N].reshape(self.batch, -1)
                eng.set_control_bounds(-up, up)
                eng.set_constraint_rhs(0, self.v[:, t:t + N + 1].reshape(self.batch, -1))
                eng.solve(stream)
                eng.advance(disturbance=w[t], stream=stream)
        else:
            eng.schedule_seek(0)
            eng.rollout(ticks, disturbances=w, stream=stream)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def window_kernel_seconds(self, ticks):
        """device time of one launch of the window kernel: events around `ticks` seeks (each launches the limit windows and nothing else)"""
        self.schedules()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for t in range(ticks):
            self.eng.schedule_seek(t)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3 / ticks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("moving-limit loop, CoM controller (xDim 6, uDim 3, N 20), velocity row as a TrajectoryConstraint + control bounds, per-instance limit signals, "
        "%d ticks per run, %d alternating runs; M solves/s: median (min .. max)" % (args.ticks, args.reps))
    say("library source hash %s" % _capi.library_source_hash())
    for batch in (65536, 16384):
        loops = {v: Loop(batch, v, args.ticks) for v in ("host", "rollout")}
        for lp in loops.values():  # module load, LDS opt-in, first-solve set-up, the engine's adaptation
            lp.run(10)
        rates = {v: [] for v in loops}
        for _ in range(args.reps):
            for v, lp in loops.items():
                rates[v].append(batch * args.ticks / lp.run(args.ticks) / 1e6)
        say("batch %d" % batch)
        for v in loops:
            r = rates[v]
            say("  (%s) %-8s %8.1f  (%8.1f .. %8.1f)" % ("a" if v == "host" else "b", v, statistics.median(r), min(r), max(r)))
        a, b = statistics.median(rates["host"]), statistics.median(rates["rollout"])
        say("  rollout / host = %.3f: %s" % (b / a, "faster" if b > 1.02 * a else "within the 2 %% run-to-run spread" if b >= 0.98 * a else "SLOWER"))
        wk = loops["rollout"].window_kernel_seconds(args.ticks)
        say("  copra_limit_window_kernel (3 windows, %d B written per instance): %.1f us per launch, launch gap included" % (8 * (2 * NU * loops["rollout"].N + 3 * (loops["rollout"].N + 1)), 1e6 * wk))
        del loops
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
