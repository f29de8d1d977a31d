"""What steady-state targets (copra_batch_set_target) cost the closed loop and what they replace, on the CoM controller at the sizes of
tools/bench_closed_loop.py, whose Loop (controller, result slab, disturbances, timing around a final synchronisation) is used as it is.

    python tools/bench_target_loop.py [--ticks 200] [--reps 5] [--parent DIR] [--out profiles/closed_loop/target_rates.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_target_loop.py --trace 65536 --variant targets   (the target kernel's own time)
    python tools/bench_target_loop.py --kernel-stats targets=CSV_OR_DB --out FILE  (appends that run's kernel times to FILE)

Per size (65 536 and 16 384 instances, per-instance systems, a plant of its own that carries a constant load per instance), `reps`
alternating runs of ONE rollout(ticks) each with
  nothing enabled                                                   -- the bar
  the estimator (gain 1, diagonal, shared)                          -- the loop the targets are added to
  the estimator and targets driving both costs                      -- the price of the targets: against the line above
and, with fewer ticks, the host-driven loop the feature replaces: per tick bias(), a batched numpy solve of the target systems and two
set_cost_reference.  One controller per variant, created and warmed up outside the timed region.  Rates are in M plant ticks/s
(instances x ticks / s).

--parent DIR: a checkout of the PARENT commit with its library built.  The bar on the path that never enables targets: `reps` runs of the
parent's rollout and `reps` of this tree's with nothing enabled, alternating, each in a process of its own (a process loads one build);
this tree's median may be lower than the parent's by at most the parent's own min .. max spread.  The exit status is 1 if it is not.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((65536, False), (16384, False))
NX, NU = 6, 3
VARIANTS = ("off", "estimator", "targets", "host")
HOST_TICKS = 20
# A, B, d read; z, the status and the two references written (the setpoint is shared): what the shapes give per instance and tick
ESTIMATE_BYTES = 8 * (NX * NX + NX * NU + NX) + 8 * (NX + NU) + 4 + 8 * (NX + NU)
LOAD = 0.004


def load_loop(root):
    """Loop of `root`'s tools/bench_closed_loop.py, which puts `root` in front of sys.path itself: the package of that tree is the one imported"""
    sys.path.insert(0, os.path.join(root, "tools"))
    from bench_closed_loop import Loop
    return Loop


def plant_of(loop):
    """the controller's model with a constant load per instance on d (torch tensors in ABI layout)"""
    import torch
    gen = torch.Generator(device=loop.dev).manual_seed(7)
    c = LOAD * (2.0 * torch.rand((loop.batch, NX), device=loop.dev, generator=gen, dtype=torch.float64) - 1.0)
    return loop.A, loop.B, (loop.d + c).contiguous()


def goal_of(loop):
    from copra_amd import workloads
    return np.asarray(workloads.COM_X_GOAL[:NU], dtype=np.float64)


def enable(loop, kind):
    loop.x_keep = loop.x_start.clone()  # (the estimator and the targets want a system in force)
    loop.hand_over(loop.x_keep)
    if kind in ("estimator", "targets", "host"):
        loop.eng.set_bias_estimator(np.ones(NX))
    if kind == "targets":
        loop.eng.set_target(np.eye(NX)[:NU], goal_of(loop), [0, 1])


def host_systems(loop):
    """what the host-driven loop keeps: the systems' matrices in natural indexing, the left-hand sides of its target problems"""
    A = np.swapaxes(loop.A.cpu().numpy(), 1, 2)
    B = np.swapaxes(loop.B.cpu().numpy(), 1, 2)
    b, n = loop.batch, NX + NU
    M = np.zeros((b, n, n))
    M[:, :NX, :NX] = A - np.eye(NX)
    M[:, :NX, NX:] = B
    M[:, NX:, :NX] = np.eye(NX)[:NU]
    return M


def timed_rollout(loop, ticks, kind="off", feature=True, M=None):
    """one rollout from the start state; feature False: nothing of the feature is called (a tree without it); returns seconds"""
    import torch
    x = loop.x_start.clone()
    loop.hand_over(x)
    w = loop.disturbances(ticks)
    plant = loop.plant if hasattr(loop, "plant") else (loop.A, loop.B, loop.d)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if kind == "host" and feature:
        goal = np.tile(goal_of(loop), (loop.batch, 1))
        for t in range(ticks):
            rhs = np.concatenate([-loop.eng.bias(), goal], axis=1)
            z = np.linalg.solve(M, rhs[:, :, None])[:, :, 0]
            loop.eng.set_cost_reference(0, np.ascontiguousarray(z[:, :NX]))
            loop.eng.set_cost_reference(1, np.ascontiguousarray(z[:, NX:]))
            loop.eng.solve(loop.stream)
            loop.eng.advance(plant=plant, disturbance=w[t], stream=loop.stream)
    else:
        loop.eng.rollout(ticks, plant=plant, disturbances=w, stream=loop.stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_times(pairs, say):
    """the project's kernels out of rocprofv3's output, one file per variant -- a *_kernel_stats.csv, or the run's *_results.db where the
    profiler writes a database: calls and the average time of each per launch"""
    import csv
    import sqlite3
    say("kernel times at 65 536 instances, per-instance systems and a plant of its own, from separate rocprofv3 --kernel-trace --stats runs of --trace "
        "(us per launch, calls); what its bytes and a launch boundary give for copra_target_kernel: 1.5 - 1.9 us plus %d B per instance:" % ESTIMATE_BYTES)
    for pair in pairs:
        kind, path = pair.split("=", 1)
        if path.endswith(".db"):
            with sqlite3.connect(path) as db:
                rows = [(n, a, c) for n, c, a in db.execute("select name, count(*), avg(end - start) from kernels group by name order by 3 desc") if "copra_" in n]
        else:
            with open(path, newline="") as fh:
                rows = [(r["Name"], float(r["AverageNs"]), r["Calls"]) for r in csv.DictReader(fh) if "copra_" in r["Name"]]
        say("  variant: %s" % kind)
        for name, avg, calls in rows:
            say("    %-52s %8.1f  x %s" % (name.replace("void ", "").split("(")[0], avg / 1e3, calls))


def child(args):
    """one timed run in this process, nothing of the feature called: prints the rate"""
    Loop = load_loop(args.child)
    batch, shared = SIZES[args.size]
    loop = Loop(batch, shared)
    timed_rollout(loop, 10, feature=False)
    print("RATE %.6f" % (batch * args.ticks / timed_rollout(loop, args.ticks, feature=False) / 1e6), flush=True)


def against_parent(args, say):
    ok = True
    for size, (batch, shared) in enumerate(SIZES):
        rates = {args.parent: [], ROOT: []}
        for rep in range(args.reps):
            for root in ((args.parent, ROOT) if rep % 2 == 0 else (ROOT, args.parent)):  # (neither tree always runs behind the other)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--size", str(size), "--ticks", str(args.ticks)],
                                     check=True, capture_output=True, text=True, timeout=600).stdout
                rates[root].append(float([ln for ln in out.splitlines() if ln.startswith("RATE ")][-1].split()[1]))
        p, o = rates[args.parent], rates[ROOT]
        spread = max(p) - min(p)
        lower = statistics.median(p) - statistics.median(o)
        good = lower <= spread
        ok = ok and good
        say("batch %d, per-instance systems, the controller's model as the plant: rollout, one process per run" % batch)
        say("  parent            %8.1f  (%8.1f .. %8.1f)   spread %.1f" % (statistics.median(p), min(p), max(p), spread))
        say("  never enabled     %8.1f  (%8.1f .. %8.1f)" % (statistics.median(o), min(o), max(o)))
        say("  parent - this tree = %+.1f M ticks/s: %s" % (lower, "within the parent's spread" if good else "LOWER than the parent by more than its spread"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built: the bar on the path that never enables targets")
    ap.add_argument("--trace", type=int, default=0, help="only `ticks` ticks of one rollout at this batch size (for a kernel trace)")
    ap.add_argument("--variant", choices=VARIANTS[:3], default="targets", help="with --trace: the variant")
    ap.add_argument("--kernel-stats", nargs="+", default=None, metavar="VARIANT=FILE",
                    help="no run: append the kernel times of these rocprofv3 *_kernel_stats.csv files (one per --variant of a --trace run) to --out")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--size", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.kernel_stats:
        kernel_times(args.kernel_stats, say)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        return 0
    if args.trace:
        Loop = load_loop(ROOT)
        loop = Loop(args.trace, shared=False)
        loop.plant = plant_of(loop)
        enable(loop, args.variant)
        timed_rollout(loop, 5, args.variant)
        timed_rollout(loop, args.ticks, args.variant)
        say("trace: %d + 5 ticks of one rollout at %d instances, per-instance systems and a plant of its own, variant: %s" % (args.ticks, args.trace, args.variant))
        return 0
    import torch
    ok = True
    say("steady-state targets, CoM controller (xDim 6, uDim 3, N 20), %d ticks per run, %d alternating runs; M plant ticks/s: median (min .. max)"
        % (args.ticks, args.reps))
    if args.parent:
        ok = against_parent(args, say)  # (first: no process of this tool has the device open while the children run)
    Loop = load_loop(ROOT)
    names = {"off": "nothing enabled", "estimator": "estimator (gain 1)", "targets": "estimator and targets, two driven costs",
             "host": "host-driven targets (%d ticks per run)" % HOST_TICKS}
    for batch, shared in SIZES:
        rates = {k: [] for k in VARIANTS}
        loops, M = {}, None
        for k in VARIANTS:
            loops[k] = Loop(batch, shared)
            loops[k].plant = plant_of(loops[k])
            enable(loops[k], k)
            if k == "host":
                M = host_systems(loops[k])
            timed_rollout(loops[k], 10 if k != "host" else 2, k, M=M)  # module load, LDS opt-in, first-solve set-up, the engine's adaptation
        for _ in range(args.reps):
            for k in VARIANTS:
                ticks = args.ticks if k != "host" else HOST_TICKS
                rates[k].append(batch * ticks / timed_rollout(loops[k], ticks, k, M=M) / 1e6)
        say("batch %d, per-instance systems, a plant of its own under a constant load" % batch)
        for k in VARIANTS:
            r = rates[k]
            say("  %-42s %8.1f  (%8.1f .. %8.1f)" % (names[k], statistics.median(r), min(r), max(r)))
        med = {k: statistics.median(rates[k]) for k in VARIANTS}
        say("  targets / estimator alone = %.3f  (estimator alone: spread %.1f)" % (med["targets"] / med["estimator"], max(rates["estimator"]) - min(rates["estimator"])))
        say("  targets / nothing enabled = %.3f" % (med["targets"] / med["off"]))
        say("  targets on the device / host-driven = %.1f" % (med["targets"] / med["host"]))
        del loops
        torch.cuda.empty_cache()
    say("the target kernel's traffic per instance and tick, from the shapes: A %d B, B %d B, d %d B read; z %d B, the status 4 B and the two references "
        "%d B written = %d B" % (8 * NX * NX, 8 * NX * NU, 8 * NX, 8 * (NX + NU), 8 * (NX + NU), ESTIMATE_BYTES))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
