"""What ensemble traces (copra_batch_set_trace) cost the closed loop and what they replace, on the CoM controller at the sizes of
tools/bench_closed_loop.py, whose Loop (controller, result slab, disturbances, timing around a final synchronisation) is used as it is.

    python tools/bench_trace_loop.py [--ticks 200] [--reps 5] [--parent DIR] [--out profiles/closed_loop/trace_rates.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_trace_loop.py --trace 65536 --what all     (the two kernels' own times)
    python tools/bench_trace_loop.py --kernel-stats all=CSV --out FILE                    (appends that run's kernel times to FILE)

Per size (65 536 and 16 384 instances, per-instance systems, a plant of its own), `reps` alternating runs of ONE rollout(ticks) each with
  tracing never enabled, no histories                                    -- the bar
  a trace of x and u (9 rows), no histories                              -- the price of the trace: against the line above
  a trace of x, u, err and viol with limits (16 rows), no histories      -- (without an observer the err rows are empty on every tick)
  the observer simulating the plant, tracing never enabled               -- the bar of the line below
  the observer, a trace of x, u, err and viol (16 rows)                  -- the err rows live: the estimates are read as well
  x_hist + u_hist + age_hist, the same statistics per tick in torch      -- what the feature replaces
on one controller per variant, created and warmed up outside the timed region.  The traced runs end with trace() -- the copy of the slots to
the host --, the history run with its torch reduction: both are inside the timed region.  Rates are in M plant ticks/s (instances x ticks /
s).  Beside them the peak of the device memory each run takes while it runs (torch's allocator: the histories and the temporaries of their
reduction; the disturbances every variant is given are left out) and what the library itself holds for the trace (from the shapes).

--parent DIR: a checkout of the PARENT commit with its library built.  The bar on the path that never traces: `reps` runs of the parent's
rollout and `reps` of this tree's with tracing never enabled, alternating, each in a process of its own (a process loads one build); this
tree's median may differ from the parent's, in either direction, by at most the parent's own min .. max spread.  The exit status is 1 if it
does not.
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
VARIANTS = ("off", "xu", "all", "obs_off", "obs_all", "histories")
NAMES = {"off": "tracing never enabled, no histories", "xu": "trace of x, u (9 rows)", "all": "trace of x, u, err, viol (16 rows; err empty)",
         "obs_off": "observer, tracing never enabled", "obs_all": "observer, trace of x, u, err, viol (16 rows)",
         "histories": "x_hist + u_hist + age_hist, reduced per tick in torch"}
HELD = -2


def load_loop(root):
    """Loop of `root`'s tools/bench_closed_loop.py, which puts `root` in front of sys.path itself: the package of that tree is the one imported"""
    sys.path.insert(0, os.path.join(root, "tools"))
    from bench_closed_loop import Loop
    return Loop


def prepare(loop, kind, ticks):
    """the observer and the trace of variant `kind`, limits as torch tensors used in place"""
    import numpy as np
    import torch
    if kind.startswith("obs"):
        loop.first_x = loop.x_start.clone()  # (the observer wants a system and a state in force; the tensor is used in place: kept)
        loop.hand_over(loop.first_x)
        C = np.eye(NX)[:3]
        Lx = np.zeros((NX, 3))
        Lx[:3], Lx[3:] = 0.4 * np.eye(3), 0.2 * np.eye(3)
        loop.eng.set_observer(C, Lx)
    f = lambda *a: torch.tensor(a, dtype=torch.float64, device=loop.dev)  # noqa: E731
    inf = float("inf")
    if kind == "xu":
        loop.eng.set_trace(ticks)
    elif kind in ("all", "obs_all"):
        loop.eng.set_trace(ticks, estimate_error=True, state_limits=(f(-inf, -inf, -inf, -0.6, -0.6, -0.6), f(inf, inf, inf, 0.6, 0.6, 0.6)),
                           control_limits=(f(-3, -3, -3), f(3, 3, 3)), tol=1e-9)


def torch_statistics(hist):
    """the trace's statistics of every tick from the histories: x and u rows (a held instance has no u), counts of the ages"""
    import torch
    x, u, age = hist["x_hist"][1:], hist["u_hist"], hist["age_hist"]
    live = (age != HELD)[:, :, None]
    n = live.sum(dim=1).clamp(min=1)
    uz = torch.where(live, u, torch.zeros_like(u))
    um = uz.sum(dim=1) / n
    out = [x.mean(dim=1), x.var(dim=1), x.amin(dim=1), x.amax(dim=1), x.argmin(dim=1), x.argmax(dim=1), um, (torch.where(live, (u - um[:, None]) ** 2, torch.zeros_like(u))).sum(dim=1),
           torch.where(live, u, torch.full_like(u, float("inf"))).amin(dim=1), torch.where(live, u, torch.full_like(u, -float("inf"))).amax(dim=1),
           (age == 0).sum(dim=1), (age >= 1).sum(dim=1), (age == HELD).sum(dim=1)]
    return [t.cpu() for t in out]


def timed_rollout(loop, ticks, kind="off", traces=True):
    """one rollout from the start state; traces False: nothing of the feature is called (a tree without it); returns (seconds, the peak of
    the device memory the run took from torch's allocator: histories and the temporaries of their reduction)"""
    import torch
    x = loop.x_start.clone()
    loop.hand_over(x)
    if traces and kind.startswith("obs"):
        loop.eng.set_plant_state(loop.x_start)
    if traces and kind in ("xu", "all", "obs_all"):
        loop.eng.reset_trace()
    w = loop.disturbances(ticks)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    kw = dict(plant=(loop.A, loop.B, loop.d), disturbances=w, stream=loop.stream)
    if kind == "histories":
        keep = torch_statistics(loop.eng.rollout(ticks, x_hist=True, u_hist=True, age_hist=True, **kw))
    else:
        loop.eng.rollout(ticks, **kw)
        keep = loop.eng.trace() if traces and kind in ("xu", "all", "obs_all") else None
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if keep is not None and kind != "histories":
        assert len(keep["head"]) == ticks
    del keep
    return dt, torch.cuda.max_memory_allocated() - before


def kernel_times(pairs, say, ticks_bytes):
    """the project's kernels out of rocprofv3's *_kernel_stats.csv files, one per variant: calls and the average time of each per launch"""
    import csv
    say("kernel times at 65 536 instances, per-instance systems and a plant of its own, from a separate rocprofv3 --kernel-trace --stats --output-format csv run of --trace "
        "(us per launch, calls); stage 1 of the trace reads %.1f MB per tick (x, u and the ages; %.1f MB with the estimates), which the device's %.0f TB/s "
        "would move in %.1f us, and the two launches add a boundary of 1.5 - 1.9 us each:" % (ticks_bytes[0] / 1e6, ticks_bytes[1] / 1e6, 8.0, ticks_bytes[0] / 8e6))
    for pair in pairs:
        kind, path = pair.split("=", 1)
        with open(path, newline="") as fh:
            rows = [r for r in csv.DictReader(fh) if "copra_" in r["Name"]]
        say("  variant: %s" % kind)
        for r in rows:
            name = r["Name"].replace("void ", "").split("(")[0]
            say("    %-52s %8.1f  x %s" % (name, float(r["AverageNs"]) / 1e3, r["Calls"]))


def child(args):
    """one timed run in this process, nothing of the feature called: prints the rate"""
    Loop = load_loop(args.child)
    batch, shared = SIZES[args.size]
    loop = Loop(batch, shared)
    timed_rollout(loop, 10, traces=False)
    print("RATE %.6f" % (batch * args.ticks / timed_rollout(loop, args.ticks, traces=False)[0] / 1e6), flush=True)


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
        good = abs(lower) <= spread
        ok = ok and good
        say("batch %d, per-instance systems, a plant of its own: rollout, one process per run" % batch)
        say("  parent            %8.1f  (%8.1f .. %8.1f)   spread %.1f" % (statistics.median(p), min(p), max(p), spread))
        say("  never tracing     %8.1f  (%8.1f .. %8.1f)" % (statistics.median(o), min(o), max(o)))
        say("  parent - this tree = %+.1f M ticks/s: %s" % (lower, "within the parent's spread" if good else "apart by MORE than the parent's spread"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built: the bar on the path that never traces")
    ap.add_argument("--trace", type=int, default=0, help="only `ticks` ticks of one rollout at this batch size (for a kernel trace)")
    ap.add_argument("--what", choices=VARIANTS[:5], default="all", help="with --trace: the variant")
    ap.add_argument("--kernel-stats", nargs="+", default=None, metavar="VARIANT=CSV",
                    help="no run: append the kernel times of these rocprofv3 *_kernel_stats.csv files (one per --what of a --trace run) to --out")
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
        b = SIZES[0][0]
        kernel_times(args.kernel_stats, say, (b * (8 * NX + 8 * NU + 4), b * (16 * NX + 8 * NU + 4)))
        if args.out:
            with open(args.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        return 0
    if args.trace:
        Loop = load_loop(ROOT)
        loop = Loop(args.trace, shared=False)
        prepare(loop, args.what, args.ticks)
        timed_rollout(loop, 5, args.what)
        timed_rollout(loop, args.ticks, args.what)
        say("trace: %d + 5 ticks of one rollout at %d instances, per-instance systems and a plant of its own, variant: %s" % (args.ticks, args.trace, args.what))
        return 0
    import torch
    ok = True
    say("ensemble traces, CoM controller (xDim 6, uDim 3, N 20), %d ticks per run, %d alternating runs; M plant ticks/s: median (min .. max)"
        % (args.ticks, args.reps))
    if args.parent:
        ok = against_parent(args, say)  # (first: no process of this tool has the device open while the children run)
    Loop = load_loop(ROOT)
    for batch, shared in SIZES:
        rates, mem = {k: [] for k in VARIANTS}, {k: 0 for k in VARIANTS}
        loops = {}
        for k in VARIANTS:
            loops[k] = Loop(batch, shared)
            prepare(loops[k], k, args.ticks)
            timed_rollout(loops[k], 10, k)  # module load, LDS opt-in, first-solve set-up, the engine's adaptation
        for _ in range(args.reps):
            for k in VARIANTS:
                dt, peak = timed_rollout(loops[k], args.ticks, k)
                rates[k].append(batch * args.ticks / dt / 1e6)
                mem[k] = max(mem[k], peak)
        say("batch %d, per-instance systems, a plant of its own" % batch)
        for k in VARIANTS:
            r = rates[k]
            say("  %-56s %8.1f  (%8.1f .. %8.1f)   peak memory of a run %8.1f MB" % (NAMES[k], statistics.median(r), min(r), max(r), mem[k] / 1e6))
        med = {k: statistics.median(rates[k]) for k in VARIANTS}
        say("  x, u / never enabled = %.3f;  16 rows / never enabled = %.3f  (never enabled: spread %.1f)"
            % (med["xu"] / med["off"], med["all"] / med["off"], max(rates["off"]) - min(rates["off"])))
        say("  observer: 16 rows with live err rows / never enabled = %.3f  (never enabled: spread %.1f)"
            % (med["obs_all"] / med["obs_off"], max(rates["obs_off"]) - min(rates["obs_off"])))
        say("  x, u / histories = %.3f;  16 rows / histories = %.3f" % (med["xu"] / med["histories"], med["all"] / med["histories"]))
        chunks = -(-batch // 1024)
        say("  histories of %d ticks: %.1f MB; what the library holds for a trace of 16 rows (slots, the partials of a tick, u and age where nobody asks for "
            "them): %.3f MB, of which the slots are %.1f KB"
            % (args.ticks, 1e-6 * batch * (8 * (args.ticks + 1) * NX + 8 * args.ticks * NU + 4 * args.ticks),
               1e-6 * ((args.ticks + chunks) * (64 + 56 * 16) + batch * (8 * NU + 4)), 1e-3 * args.ticks * (64 + 56 * 16)))
        del loops
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
