"""What backup plans cost the closed loop (copra_batch_set_backup_steps), on the CoM controller at the sizes of tools/bench_closed_loop.py, whose
Loop (controller, result slab, disturbances, timing around a final synchronisation) is used as it is.

    python tools/bench_backup_loop.py [--ticks 200] [--reps 5] [--parent DIR] [--out profiles/closed_loop/backup_rates.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_backup_loop.py --trace 65536 --steps 3   (the plant step's own time; --steps 0 beside it)

Per size (16 384 instances on one shared model, 65 536 with per-instance systems), `reps` alternating runs of ONE rollout(ticks) each with
  K = 0, 1, 3, N - 1 at a solve every tick, and K = 3 with a solve every 2nd and every 4th tick (solve_every)
on one controller per variant, created and warmed up outside the timed region; set_backup_steps(K) starts the episode of every run.  Rates are in
M plant ticks/s (instances x ticks / s): with solve_every = k the controller solves k times less often -- a capability, the rate is no speed-up
of the solver.  Nothing fails in these runs: every tick with a solve stores K nu doubles per instance, no plan is read except between solves.

--parent DIR: a checkout of the PARENT commit with its library built.  The bar on the off path: `reps` runs of the parent's rollout and `reps` of
this tree's with K = 0, alternating, each in a process of its own (a process loads one build); this tree's median may be lower than the parent's
by at most the parent's own min .. max spread.  The exit status is 1 if it is not.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((16384, True), (65536, False))


def load_loop(root):
    """Loop of `root`'s tools/bench_closed_loop.py, which puts `root` in front of sys.path itself: the package of that tree is the one imported"""
    sys.path.insert(0, os.path.join(root, "tools"))
    from bench_closed_loop import Loop
    return Loop


def timed_rollout(loop, ticks, steps=None, every=1):
    """Loop.run("rollout", ticks) with the backup arguments; steps None: nothing of the feature is called (a tree without it)"""
    import torch
    x = loop.x_start.clone()
    loop.hand_over(x)
    kw = {}
    if steps is not None:
        loop.eng.set_backup_steps(steps)
        kw = dict(solve_every=every)
    w = loop.disturbances(ticks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.eng.rollout(ticks, disturbances=w, stream=loop.stream, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def child(args):
    """one timed run in this process: prints the rate"""
    Loop = load_loop(args.child)
    batch, shared = SIZES[args.size]
    loop = Loop(batch, shared)
    steps = 0 if os.path.abspath(args.child) == ROOT else None  # (the parent has no setter: its loop is untouched)
    timed_rollout(loop, 10, steps)
    print("RATE %.6f" % (batch * args.ticks / timed_rollout(loop, args.ticks, steps) / 1e6), flush=True)


def against_parent(args, say):
    ok = True
    for size, (batch, shared) in enumerate(SIZES):
        rates = {args.parent: [], ROOT: []}
        for _ in range(args.reps):
            for root in (args.parent, ROOT):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--size", str(size), "--ticks", str(args.ticks)],
                                     check=True, capture_output=True, text=True, timeout=600).stdout
                rates[root].append(float([ln for ln in out.splitlines() if ln.startswith("RATE ")][-1].split()[1]))
        p, o = rates[args.parent], rates[ROOT]
        spread = max(p) - min(p)
        lower = statistics.median(p) - statistics.median(o)
        good = lower <= spread
        ok = ok and good
        say("batch %d, %s: rollout, one process per run" % (batch, "one shared model" if shared else "per-instance systems"))
        say("  parent        %8.1f  (%8.1f .. %8.1f)   spread %.1f" % (statistics.median(p), min(p), max(p), spread))
        say("  K = 0         %8.1f  (%8.1f .. %8.1f)" % (statistics.median(o), min(o), max(o)))
        say("  parent - K = 0 = %+.1f M ticks/s: %s" % (lower, "within the parent's spread" if good else "LOWER than the parent by more than its spread"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built: the bar on the off path")
    ap.add_argument("--trace", type=int, default=0, help="only `ticks` ticks of one rollout at this batch size (for a kernel trace)")
    ap.add_argument("--steps", type=int, default=0, help="with --trace: K")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--size", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.trace:
        Loop = load_loop(ROOT)
        loop = Loop(args.trace, shared=args.trace <= 16384)
        timed_rollout(loop, 5, args.steps)
        timed_rollout(loop, args.ticks, args.steps)
        say("trace: %d + 5 ticks of one rollout at %d instances, K = %d" % (args.ticks, args.trace, args.steps))
        return 0
    ok = True
    say("backup plans in the closed loop, CoM controller (xDim 6, uDim 3, N 20), %d ticks per run, %d alternating runs; M plant ticks/s: median (min .. max)"
        % (args.ticks, args.reps))
    if args.parent:
        ok = against_parent(args, say)  # (first: no process of this tool has the device open while the children run)
    Loop = load_loop(ROOT)
    for batch, shared in SIZES:
        variants = [("K = 0", 0, 1), ("K = 1", 1, 1), ("K = 3", 3, 1), ("K = N - 1", None, 1), ("K = 3, a solve every 2nd tick", 3, 2),
                    ("K = 3, a solve every 4th tick", 3, 4)]
        loops = [Loop(batch, shared) for _ in variants]
        N = loops[0].N
        variants = [(name, N - 1 if K is None else K, every) for name, K, every in variants]
        for loop, (_, K, every) in zip(loops, variants):  # module load, LDS opt-in, first-solve set-up, the engine's adaptation
            timed_rollout(loop, 10, K, every)
        rates = [[] for _ in variants]
        for _ in range(args.reps):
            for r, loop, (_, K, every) in zip(rates, loops, variants):
                r.append(batch * args.ticks / timed_rollout(loop, args.ticks, K, every) / 1e6)
        say("batch %d, %s" % (batch, "one shared model" if shared else "per-instance systems"))
        for r, (name, _, every) in zip(rates, variants):
            say("  %-30s %8.1f  (%8.1f .. %8.1f)%s" % (name, statistics.median(r), min(r), max(r),
                                                       "" if every == 1 else "   %d solves in %d ticks" % ((args.ticks + every - 1) // every, args.ticks)))
        base = statistics.median(rates[0])
        for r, (name, _, every) in zip(rates[1:4], variants[1:4]):
            say("  %s / K = 0 = %.3f" % (name, statistics.median(r) / base))
        del loops
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
