"""What the disturbance estimator costs the closed loop (copra_batch_set_bias_estimator), on the CoM controller at the sizes of
tools/bench_closed_loop.py, whose Loop (controller, result slab, disturbances, timing around a final synchronisation) is used as it is.

    python tools/bench_bias_loop.py [--ticks 200] [--reps 5] [--parent DIR] [--out profiles/closed_loop/bias_rates.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_bias_loop.py --trace 65536 --gain dense   (the plant step's own time; --gain off beside it)
    python tools/bench_bias_loop.py --kernel-stats off=CSV diagonal=CSV dense=CSV --out FILE        (appends those runs' kernel times to FILE)

Per size (16 384 and 65 536 instances), `reps` alternating runs of ONE rollout(ticks) each with
  the estimator never enabled | a diagonal gain shared by the batch | a dense gain per instance
on one controller per variant, created and warmed up outside the timed region; set_system starts the episode of every run (with the estimator
on, the estimates restart from its d).  The estimator needs per-instance systems: its variants use them at both sizes, and at 16 384 the
off variant is also reported for one shared model (the size as tools/bench_closed_loop.py runs it).  The estimator's variants, and the off
variant they are compared with, are given a plant of its own per instance (the model's arrays): the estimates then stay at the plant's d plus
filtered noise, and the loop solves what the off variant solves.  With no plant the plant is the model with its estimates, e = w, and a gain
turns the noise into a random walk of the plant -- a harder closed loop, nothing the kernel costs.  Rates are in M plant ticks/s
(instances x ticks / s).  Beside them, the bytes per instance and tick the estimator adds to the plant step's traffic, from the shapes.

--parent DIR: a checkout of the PARENT commit with its library built.  The bar on the off path: `reps` runs of the parent's rollout and `reps` of
this tree's with the estimator never enabled, alternating, each in a process of its own (a process loads one build); this tree's median may be
lower than the parent's by at most the parent's own min .. max spread.  The exit status is 1 if it is not.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((16384, True), (65536, False))
NX, NU = 6, 3
GAINS = ("off", "diagonal", "dense")


def load_loop(root):
    """Loop of `root`'s tools/bench_closed_loop.py, which puts `root` in front of sys.path itself: the package of that tree is the one imported"""
    sys.path.insert(0, os.path.join(root, "tools"))
    from bench_closed_loop import Loop
    return Loop


def make_gain(loop, kind):
    """a torch tensor in ABI layout, used in place: (nx,) shared and diagonal, or (batch, nx, nx) dense per instance"""
    import torch
    if kind == "diagonal":
        return torch.full((NX,), 0.5, dtype=torch.float64, device=loop.dev)
    g = 0.5 * torch.eye(NX, dtype=torch.float64, device=loop.dev) + 0.01
    return g.expand(loop.batch, NX, NX).contiguous()


def timed_rollout(loop, ticks, gain=None, own_plant=False):
    """Loop.run("rollout", ticks); gain None: nothing of the feature is called (a tree without it, or the estimator never enabled);
    own_plant: the model's arrays handed over as a plant of its own (device tensors in ABI layout, used in place)"""
    import torch
    x = loop.x_start.clone()
    loop.hand_over(x)  # (estimator on: the estimates restart from the model's d)
    if gain is not None:
        loop.eng.set_bias_estimator(gain)
    w = loop.disturbances(ticks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kw = dict(plant=(loop.A, loop.B, loop.d)) if own_plant else {}
    loop.eng.rollout(ticks, disturbances=w, stream=loop.stream, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def extra_bytes(kind, d_out=False, own_plant=False):
    """doubles the estimator adds per instance and tick, as bytes: dhat read and written, d_out, a plant of its own, a per-instance gain"""
    n = 2 * NX + (NX if d_out else 0) + (NX * NX + NX * NU if own_plant else 0) + (NX * NX if kind == "dense" else 0)
    return 8 * n


def kernel_times(pairs, say):
    """the project's kernels out of rocprofv3's *_kernel_stats.csv files, one per gain: calls and the average time of each per launch"""
    import csv
    say("kernel times at 65 536 instances, per-instance systems and a plant of its own, from separate rocprofv3 --kernel-trace --stats runs of --trace "
        "(us per launch, calls):")
    for pair in pairs:
        gain, path = pair.split("=", 1)
        with open(path, newline="") as fh:
            rows = [r for r in csv.DictReader(fh) if "copra_" in r["Name"]]
        say("  gain: %s" % gain)
        for r in rows:
            name = r["Name"].replace("void ", "").split("(")[0]
            say("    %-52s %8.1f  x %s" % (name, float(r["AverageNs"]) / 1e3, r["Calls"]))


def child(args):
    """one timed run in this process: prints the rate"""
    Loop = load_loop(args.child)
    batch, shared = SIZES[args.size]
    loop = Loop(batch, shared)
    timed_rollout(loop, 10)
    print("RATE %.6f" % (batch * args.ticks / timed_rollout(loop, args.ticks) / 1e6), flush=True)


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
        say("  parent            %8.1f  (%8.1f .. %8.1f)   spread %.1f" % (statistics.median(p), min(p), max(p), spread))
        say("  estimator off     %8.1f  (%8.1f .. %8.1f)" % (statistics.median(o), min(o), max(o)))
        say("  parent - off = %+.1f M ticks/s: %s" % (lower, "within the parent's spread" if good else "LOWER than the parent by more than its spread"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built: the bar on the off path")
    ap.add_argument("--trace", type=int, default=0, help="only `ticks` ticks of one rollout at this batch size, per-instance systems (for a kernel trace)")
    ap.add_argument("--gain", choices=GAINS, default="off", help="with --trace: the estimator's gain")
    ap.add_argument("--kernel-stats", nargs="+", default=None, metavar="GAIN=CSV",
                    help="no run: append the kernel times of these rocprofv3 *_kernel_stats.csv files (one per --gain of a --trace run) to --out")
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
        gain = None if args.gain == "off" else make_gain(loop, args.gain)
        timed_rollout(loop, 5, gain, True)
        timed_rollout(loop, args.ticks, gain, True)
        say("trace: %d + 5 ticks of one rollout at %d instances, per-instance systems and a plant of its own, gain: %s" % (args.ticks, args.trace, args.gain))
        return 0
    ok = True
    say("disturbance estimator in the closed loop, CoM controller (xDim 6, uDim 3, N 20), %d ticks per run, %d alternating runs; M plant ticks/s: median (min .. max)"
        % (args.ticks, args.reps))
    if args.parent:
        ok = against_parent(args, say)  # (first: no process of this tool has the device open while the children run)
    Loop = load_loop(ROOT)
    for batch, shared in SIZES:
        # (name, gain, one shared model, a plant of its own)
        variants = [("estimator off", None, False, False), ("estimator off, own plant", None, False, True),
                    ("diagonal gain, shared, own plant", "diagonal", False, True), ("dense gain per instance, own plant", "dense", False, True)]
        if shared:
            variants.insert(0, ("estimator off, one shared model", None, True, False))
        loops = [Loop(batch, v[2]) for v in variants]
        gains = [None if v[1] is None else make_gain(loop, v[1]) for loop, v in zip(loops, variants)]
        for loop, gain, v in zip(loops, gains, variants):  # module load, LDS opt-in, first-solve set-up, the engine's adaptation
            timed_rollout(loop, 10, gain, v[3])
        rates = [[] for _ in variants]
        for _ in range(args.reps):
            for r, loop, gain, v in zip(rates, loops, gains, variants):
                r.append(batch * args.ticks / timed_rollout(loop, args.ticks, gain, v[3]) / 1e6)
        say("batch %d, per-instance systems%s" % (batch, " unless said otherwise" if shared else ""))
        for r, v in zip(rates, variants):
            say("  %-36s %8.1f  (%8.1f .. %8.1f)%s" % (v[0], statistics.median(r), min(r), max(r),
                                                       "" if v[1] is None else "   + %d B per instance and tick" % extra_bytes(v[1], own_plant=True)))
        base = statistics.median(rates[-3])
        for r, v in zip(rates[-2:], variants[-2:]):
            say("  %s / estimator off, own plant = %.3f" % (v[0], statistics.median(r) / base))
        del loops, gains
    say("bytes the estimator adds to the plant step per instance and tick, from the shapes (8 B per double): dhat read and written 2 nx = %d B; "
        "+ nx = %d B with d_out; + nx^2 + nx nu = %d B with a plant of its own per instance; + nx^2 = %d B (dense) or nx = %d B (diagonal) with "
        "a gain per instance" % (8 * 2 * NX, 8 * NX, 8 * (NX * NX + NX * NU), 8 * NX * NX, 8 * NX))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
