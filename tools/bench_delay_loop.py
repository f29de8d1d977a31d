"""What input delay (copra_batch_set_input_delay) costs the closed loop and what it replaces, on the CoM controller at the sizes of
tools/bench_closed_loop.py, whose Loop (controller, result slab, disturbances, timing around a final synchronisation) is used as it is.

    python tools/bench_delay_loop.py [--ticks 200] [--reps 5] [--parent DIR] [--out profiles/closed_loop/delay_rates.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_delay_loop.py --trace 65536 --variant delay   (the delay kernel's own time)
    python tools/bench_delay_loop.py --kernel-stats delay=CSV_OR_DB --out FILE  (appends that run's kernel times to FILE)

Per size (65 536 and 16 384 instances, per-instance systems, the controller's model as the plant), `reps` alternating runs of ONE
rollout(ticks) each with
  nothing enabled                       -- the bar
  input delay, D = 2                    -- the price of the queue and the predictor: against the line above
and, with fewer ticks, the host-driven loop the feature replaces: per tick the state is read back, the popped command applied and the
prediction formed in numpy (tests/delay_ref.py), set_x0, solve, and the controls read back for the queue.  One controller per variant,
created and warmed up outside the timed region.  Rates are in M plant ticks/s (instances x ticks / s).

--parent DIR: a checkout of the PARENT commit with its library built.  The bar on the path that never enables delay: `reps` runs of the
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
NX, NU, D = 6, 3, 2
VARIANTS = ("off", "delay", "host")
HOST_TICKS = 10
# A, B, d, xnow, the queue block and the new command read; the command, its status and the prediction written: per instance and tick
READ_BYTES = 8 * (NX * NX + NX * NU + NX + NX + D * NU + NU) + 4 * (D + 1)
WRITE_BYTES = 8 * (NU + NX) + 4
PLANT_BYTES = 8 * (NX * NX + NX * NU + NX + NX + NX + NU) + 4 + 8 * NX  # (the plant step with a w: what it reads, and the new state)


def load_loop(root):
    """Loop of `root`'s tools/bench_closed_loop.py, which puts `root` in front of sys.path itself: the package of that tree is the one imported"""
    sys.path.insert(0, os.path.join(root, "tools"))
    from bench_closed_loop import Loop
    return Loop


def enable(loop, kind):
    loop.x_keep = loop.x_start.clone()  # (delay wants a system and an x0 in force)
    loop.hand_over(loop.x_keep)
    if kind == "delay":
        loop.eng.set_input_delay(D)


def timed_rollout(loop, ticks, kind="off", feature=True):
    """one rollout from the start state; feature False: nothing of the feature is called (a tree without it); returns seconds"""
    import torch
    x = loop.x_start.clone()
    loop.hand_over(x)  # (delay on: xnow <- x, the queue is kept, the prediction formed again)
    w = loop.disturbances(ticks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if kind == "host" and feature:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import delay_ref
        model = tuple(np.swapaxes(m.cpu().numpy(), 1, 2) if m.dim() == 3 else m.cpu().numpy() for m in (loop.A, loop.B, loop.d))
        ref = delay_ref.DelayLoop(D, x.cpu().numpy(), NU)
        wh = w.cpu().numpy()
        for t in range(ticks):
            loop.eng.set_x0(ref.x0)
            loop.eng.solve(loop.stream)
            torch.cuda.synchronize()
            ref.tick(model, model, loop.out["control"].cpu().numpy(), loop.out["status"].cpu().numpy(), None, wh[t])
    else:
        loop.eng.rollout(ticks, disturbances=w, stream=loop.stream)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_times(pairs, say):
    """the project's kernels out of rocprofv3's output, one file per variant -- a *_kernel_stats.csv, or the run's *_results.db where the
    profiler writes a database: calls and the average time of each per launch"""
    import csv
    import sqlite3
    say("kernel times at 65 536 instances, per-instance systems, from separate rocprofv3 --kernel-trace --stats runs of --trace (us per launch, calls); "
        "per instance copra_delay_kernel moves %d B, the plant step %d B:" % (READ_BYTES + WRITE_BYTES, PLANT_BYTES))
    for pair in pairs:
        kind, path = pair.split("=", 1)
        if path.endswith(".db"):
            with sqlite3.connect(path) as db:
                tables = [r[0] for r in db.execute("select name from sqlite_master where type in ('table', 'view') and name like 'kernels%'")]
                rows = [(n, a, c) for n, c, a in db.execute("select name, count(*), avg(end - start) from %s group by name order by 3 desc" % tables[0]) if "copra_" in n]
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
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built: the bar on the path that never enables delay")
    ap.add_argument("--trace", type=int, default=0, help="only `ticks` ticks of one rollout at this batch size (for a kernel trace)")
    ap.add_argument("--variant", choices=VARIANTS[:2], default="delay", help="with --trace: the variant")
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
        enable(loop, args.variant)
        timed_rollout(loop, 5, args.variant)
        timed_rollout(loop, args.ticks, args.variant)
        say("trace: %d + 5 ticks of one rollout at %d instances, per-instance systems, variant: %s" % (args.ticks, args.trace, args.variant))
        return 0
    import torch
    ok = True
    say("input delay, CoM controller (xDim 6, uDim 3, N 20), D = %d, %d ticks per run, %d alternating runs; M plant ticks/s: median (min .. max)"
        % (D, args.ticks, args.reps))
    if args.parent:
        ok = against_parent(args, say)  # (first: no process of this tool has the device open while the children run)
    Loop = load_loop(ROOT)
    names = {"off": "nothing enabled", "delay": "input delay, D = %d" % D, "host": "host-driven delay (%d ticks per run)" % HOST_TICKS}
    for batch, shared in SIZES:
        rates = {k: [] for k in VARIANTS}
        loops = {}
        for k in VARIANTS:
            loops[k] = Loop(batch, shared)
            enable(loops[k], k)
            timed_rollout(loops[k], 10 if k != "host" else 2, k)  # module load, LDS opt-in, first-solve set-up, the engine's adaptation
        for _ in range(args.reps):
            for k in VARIANTS:
                ticks = args.ticks if k != "host" else HOST_TICKS
                rates[k].append(batch * ticks / timed_rollout(loops[k], ticks, k) / 1e6)
        say("batch %d, per-instance systems, the controller's model as the plant" % batch)
        for k in VARIANTS:
            r = rates[k]
            say("  %-42s %8.1f  (%8.1f .. %8.1f)" % (names[k], statistics.median(r), min(r), max(r)))
        med = {k: statistics.median(rates[k]) for k in VARIANTS}
        say("  delay / nothing enabled = %.3f  (nothing enabled: spread %.1f)" % (med["delay"] / med["off"], max(rates["off"]) - min(rates["off"])))
        say("  delay on the device / host-driven = %.1f" % (med["delay"] / med["host"]))
        del loops
        torch.cuda.empty_cache()
    say("the delay kernel's traffic per instance and tick, from the shapes: %d B read (A, B, d, xnow, the queue block, the new command, the "
        "statuses), %d B written (the command, its status, the prediction) = %d B; the plant step's: %d B"
        % (READ_BYTES, WRITE_BYTES, READ_BYTES + WRITE_BYTES, PLANT_BYTES))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
