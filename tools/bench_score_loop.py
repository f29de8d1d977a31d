"""What closed-loop scores (copra_batch_set_score) cost the closed loop and what they replace, on the CoM controller at the sizes of
tools/bench_closed_loop.py, whose Loop (controller, result slab, disturbances, timing around a final synchronisation) is used as it is.

    python tools/bench_score_loop.py [--ticks 200] [--reps 5] [--parent DIR] [--out profiles/closed_loop/score_rates.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_score_loop.py --trace 65536 --measure dense   (the score kernel's own time, and the summary's)
    python tools/bench_score_loop.py --kernel-stats diagonal=CSV dense=CSV --out FILE        (appends those runs' kernel times to FILE)

Per size (65 536 and 16 384 instances, per-instance systems, a plant of its own), `reps` alternating runs of ONE rollout(ticks) each with
  scoring never enabled, no histories                              -- the bar
  a diagonal measure shared by the batch, no histories             -- the price of the score: against the line above
  a dense measure per instance, no histories
  x_hist + u_hist, reduced with torch as examples/monte_carlo.py   -- what the feature replaces
on one controller per variant, created and warmed up outside the timed region.  The scored runs end with score_summary(), the history run
with its torch reduction: both are inside the timed region.  Rates are in M plant ticks/s (instances x ticks / s).  Beside them the peak
of the device memory each run takes while it runs (torch's allocator: the histories and the temporaries of their reduction; the disturbances
every variant is given are left out) and what the library itself holds for the scores (from the shapes).

--parent DIR: a checkout of the PARENT commit with its library built.  The bar on the path that never scores: `reps` runs of the parent's
rollout and `reps` of this tree's with scoring never enabled, alternating, each in a process of its own (a process loads one build); this
tree's median may be lower than the parent's by at most the parent's own min .. max spread.  The exit status is 1 if it is not.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((65536, False), (16384, False))
NX, NU = 6, 3
MEASURES = ("off", "diagonal", "dense", "histories")
ESTIMATE_BYTES = 8 * NX + 8 * NU + 4 + 64 + 64  # x, u, age and the record read, the record written: what the issue of the feature estimated


def load_loop(root):
    """Loop of `root`'s tools/bench_closed_loop.py, which puts `root` in front of sys.path itself: the package of that tree is the one imported"""
    sys.path.insert(0, os.path.join(root, "tools"))
    from bench_closed_loop import Loop
    return Loop


def set_measure(loop, kind):
    """torch tensors in ABI layout, used in place: shared and diagonal, or dense per instance (with limits and a goal either way)"""
    import torch
    dev, b = loop.dev, loop.batch
    f = lambda *a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    inf = float("inf")
    qx, ru = f(1, 1, 1, 0, 0, 0), f(1e-3, 1e-3, 1e-3)
    goal, lo, hi, ulo, uhi = f(0.5, 0.5, 0.5, 0, 0, 0), f(-inf, -inf, -inf, -0.6, -0.6, -0.6), f(inf, inf, inf, 0.6, 0.6, 0.6), f(-3, -3, -3), f(3, 3, 3)
    if kind == "dense":
        per = lambda t: t.expand((b,) + tuple(t.shape)).contiguous()  # noqa: E731
        qx, ru = per(torch.diag(qx) + 0.01), per(torch.diag(ru) + 1e-5)
        goal, lo, hi, ulo, uhi = per(goal[None, :]), per(lo), per(hi), per(ulo), per(uhi)
    loop.eng.set_score(qx, ru, goal, (lo, hi), (ulo, uhi), tol=1e-9)


def timed_rollout(loop, ticks, kind="off", scores=True):
    """one rollout from the start state; scores False: nothing of the feature is called (a tree without it); returns (seconds, the peak of
    the device memory the run took from torch's allocator: histories and the temporaries of their reduction)"""
    import torch
    x = loop.x_start.clone()
    loop.hand_over(x)
    if scores and kind in ("diagonal", "dense"):
        loop.eng.reset_score()
    w = loop.disturbances(ticks)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    kw = dict(plant=(loop.A, loop.B, loop.d), disturbances=w, stream=loop.stream)
    if kind == "histories":
        hist = loop.eng.rollout(ticks, x_hist=True, u_hist=True, **kw)
        u = torch.nan_to_num(hist["u_hist"])
        cost = ((hist["x_hist"][1:, :, :3] - 0.5) ** 2).sum(dim=(0, 2)) + 1e-3 * (u ** 2).sum(dim=(0, 2))
        keep = (float(cost.mean()), float(cost.std()), float(cost.max()))
    else:
        loop.eng.rollout(ticks, **kw)
        keep = loop.eng.score_summary() if scores and kind != "off" else None
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del keep
    return dt, torch.cuda.max_memory_allocated() - before


def kernel_times(pairs, say):
    """the project's kernels out of rocprofv3's *_kernel_stats.csv files, one per measure: calls and the average time of each per launch"""
    import csv
    say("kernel times at 65 536 instances, per-instance systems and a plant of its own, from separate rocprofv3 --kernel-trace --stats runs of --trace "
        "(us per launch, calls); the estimate for copra_score_kernel was a launch boundary of 1.5 - 1.9 us plus %d B per instance:" % ESTIMATE_BYTES)
    for pair in pairs:
        kind, path = pair.split("=", 1)
        with open(path, newline="") as fh:
            rows = [r for r in csv.DictReader(fh) if "copra_" in r["Name"]]
        say("  measure: %s" % kind)
        for r in rows:
            name = r["Name"].replace("void ", "").split("(")[0]
            say("    %-52s %8.1f  x %s" % (name, float(r["AverageNs"]) / 1e3, r["Calls"]))


def child(args):
    """one timed run in this process, nothing of the feature called: prints the rate"""
    Loop = load_loop(args.child)
    batch, shared = SIZES[args.size]
    loop = Loop(batch, shared)
    timed_rollout(loop, 10, scores=False)
    print("RATE %.6f" % (batch * args.ticks / timed_rollout(loop, args.ticks, scores=False)[0] / 1e6), flush=True)


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
        say("batch %d, per-instance systems, a plant of its own: rollout, one process per run" % batch)
        say("  parent            %8.1f  (%8.1f .. %8.1f)   spread %.1f" % (statistics.median(p), min(p), max(p), spread))
        say("  never scoring     %8.1f  (%8.1f .. %8.1f)" % (statistics.median(o), min(o), max(o)))
        say("  parent - this tree = %+.1f M ticks/s: %s" % (lower, "within the parent's spread" if good else "LOWER than the parent by more than its spread"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built: the bar on the path that never scores")
    ap.add_argument("--trace", type=int, default=0, help="only `ticks` ticks of one rollout and one summary at this batch size (for a kernel trace)")
    ap.add_argument("--measure", choices=MEASURES[:3], default="diagonal", help="with --trace: the measure")
    ap.add_argument("--kernel-stats", nargs="+", default=None, metavar="MEASURE=CSV",
                    help="no run: append the kernel times of these rocprofv3 *_kernel_stats.csv files (one per --measure of a --trace run) to --out")
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
        if args.measure != "off":
            set_measure(loop, args.measure)
        timed_rollout(loop, 5, args.measure)
        timed_rollout(loop, args.ticks, args.measure)
        say("trace: %d + 5 ticks of one rollout and two summaries at %d instances, per-instance systems and a plant of its own, measure: %s"
            % (args.ticks, args.trace, args.measure))
        return 0
    import torch
    ok = True
    say("closed-loop scores, CoM controller (xDim 6, uDim 3, N 20), %d ticks per run, %d alternating runs; M plant ticks/s: median (min .. max)"
        % (args.ticks, args.reps))
    if args.parent:
        ok = against_parent(args, say)  # (first: no process of this tool has the device open while the children run)
    Loop = load_loop(ROOT)
    names = {"off": "scoring never enabled, no histories", "diagonal": "diagonal measure, shared, no histories",
             "dense": "dense measure per instance, no histories", "histories": "x_hist + u_hist, reduced with torch"}
    for batch, shared in SIZES:
        rates, mem = {k: [] for k in MEASURES}, {k: 0 for k in MEASURES}
        loops = {}
        for k in MEASURES:
            loops[k] = Loop(batch, shared)
            if k in ("diagonal", "dense"):
                set_measure(loops[k], k)
            timed_rollout(loops[k], 10, k)  # module load, LDS opt-in, first-solve set-up, the engine's adaptation
        for _ in range(args.reps):
            for k in MEASURES:
                dt, peak = timed_rollout(loops[k], args.ticks, k)
                rates[k].append(batch * args.ticks / dt / 1e6)
                mem[k] = max(mem[k], peak)
        say("batch %d, per-instance systems, a plant of its own" % batch)
        for k in MEASURES:
            r = rates[k]
            say("  %-42s %8.1f  (%8.1f .. %8.1f)   peak memory of a run %8.1f MB" % (names[k], statistics.median(r), min(r), max(r), mem[k] / 1e6))
        base = statistics.median(rates["off"])
        spread = max(rates["off"]) - min(rates["off"])
        for k in ("diagonal", "dense"):
            say("  %s / never enabled = %.3f  (never enabled: spread %.1f)" % (names[k], statistics.median(rates[k]) / base, spread))
        for k in ("diagonal", "dense"):
            say("  %s / histories = %.3f" % (names[k], statistics.median(rates[k]) / statistics.median(rates["histories"])))
        say("  histories of %d ticks: %.1f MB; what the library holds for the scores (records, u and age where the caller asks for none): %.1f MB"
            % (args.ticks, 8e-6 * batch * ((args.ticks + 1) * NX + args.ticks * NU), 1e-6 * batch * (64 + 8 * NU + 4)))
        del loops
        torch.cuda.empty_cache()
    say("the score kernel's traffic per instance and tick, from the shapes: x %d B, u %d B, age 4 B, the record read and written 2 x 64 B = %d B; a measure "
        "per instance adds its own arrays (dense: (nx^2 + nu^2 + 3 nx + 2 nu) x 8 = %d B)" % (8 * NX, 8 * NU, ESTIMATE_BYTES, 8 * (NX * NX + NU * NU + 3 * NX + 2 * NU)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
