"""What trace quantiles (copra_batch_set_trace_quantiles) cost the closed loop and what they replace, on the CoM controller at the sizes of
tools/bench_closed_loop.py, whose Loop is used as it is; the variants, the timed rollout and the comparison with a parent checkout are those
of tools/bench_trace_loop.py.

    python tools/bench_trace_quant_loop.py [--ticks 200] [--reps 5] [--parent DIR] [--out profiles/closed_loop/trace_quant_rates.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_trace_quant_loop.py --trace 65536 --what all --levels 3
    python tools/bench_trace_quant_loop.py --kernel-stats all/3=CSV --out FILE            (appends that run's kernel times to FILE)

Per size (65 536 and 16 384 instances, per-instance systems, a plant of its own), `reps` alternating runs of ONE rollout(ticks) each with
  a trace of x and u (9 rows) without quantiles, with 3 levels (0.05, 0.5, 0.95) and with 8 levels
  a trace of x, u, err and viol with limits (16 rows) likewise
  x_hist + u_hist, torch.sort along the batch and the index picked per level       -- what the feature replaces
on one controller per variant, created and warmed up outside the timed region.  The traced runs end with trace() and trace_quantiles() --
the copies to the host --, the history run with its sort: both are inside the timed region.  Rates are in M plant ticks/s (instances x
ticks / s).  Beside them the peak of the device memory a run takes from torch's allocator and the bytes of the quantile buffer,
capacity x rows x levels x 8.

--parent DIR: a checkout of the PARENT commit with its library built: the bar on the path that never traces, as in tools/bench_trace_loop.py.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_trace_loop as base  # noqa: E402

SIZES, NX, NU = base.SIZES, base.NX, base.NU
LEVELS = {0: None, 3: [0.05, 0.5, 0.95], 8: [0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0]}
VARIANTS = [(what, nq) for what in ("xu", "all") for nq in (0, 3, 8)]
ROWS = {"xu": 9, "all": 16}


def prepare(loop, what, nq, ticks):
    base.prepare(loop, what, ticks)
    if nq:
        loop.eng.set_trace_quantiles(LEVELS[nq])


def timed(loop, ticks, what, nq):
    """one rollout from the start state, read-outs inside the timed region: (seconds, peak of torch's allocator)"""
    import torch
    x = loop.x_start.clone()
    loop.hand_over(x)
    loop.eng.reset_trace()
    w = loop.disturbances(ticks)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    loop.eng.rollout(ticks, plant=(loop.A, loop.B, loop.d), disturbances=w, stream=loop.stream)
    keep = loop.eng.trace()
    band = loop.eng.trace_quantiles() if nq else None
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert len(keep["head"]) == ticks and (band is None or band["x"].shape == (ticks, NX, nq))
    return dt, torch.cuda.max_memory_allocated() - before


def torch_quantiles(hist, levels):
    """the x and u rows' order statistics of every tick by torch.sort along the batch (NaN, a held instance's u, sorts last and is counted out)"""
    import torch
    out = []
    for v in (hist["x_hist"][1:], hist["u_hist"]):
        s, _ = torch.sort(v, dim=1)
        n = torch.isfinite(v).sum(dim=1, keepdim=True)
        for p in levels:
            k = (torch.ceil(p * n.double()).long() - 1).clamp(min=0)
            k = torch.minimum(k, (n - 1).clamp(min=0))
            out.append(torch.gather(s, 1, k).cpu())
    return out


def timed_histories(loop, ticks, levels):
    import torch
    x = loop.x_start.clone()
    loop.hand_over(x)
    w = loop.disturbances(ticks)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    keep = torch_quantiles(loop.eng.rollout(ticks, x_hist=True, u_hist=True, plant=(loop.A, loop.B, loop.d), disturbances=w, stream=loop.stream), levels)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del keep
    return dt, torch.cuda.max_memory_allocated() - before


def kernel_times(pairs, say):
    import csv
    say("kernel times at 65 536 instances, per-instance systems and a plant of its own, from a separate rocprofv3 --kernel-trace --stats --output-format csv run of --trace "
        "(us per launch, calls); the quantile kernel is one workgroup of 1024 threads per row:")
    for pair in pairs:
        kind, path = pair.split("=", 1)
        with open(path, newline="") as fh:
            rows = [r for r in csv.DictReader(fh) if "copra_" in r["Name"]]
        say("  variant (rows / levels): %s" % kind)
        for r in rows:
            say("    %-52s %8.1f  x %s" % (r["Name"].replace("void ", "").split("(")[0], float(r["AverageNs"]) / 1e3, r["Calls"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built: the bar on the path that never traces")
    ap.add_argument("--sizes", type=int, nargs="+", default=None, help="only these batch sizes")
    ap.add_argument("--trace", type=int, default=0, help="only `ticks` ticks of one rollout at this batch size (for a kernel trace)")
    ap.add_argument("--what", choices=("xu", "all"), default="all", help="with --trace: the trace")
    ap.add_argument("--levels", type=int, choices=(0, 3, 8), default=3, help="with --trace: the number of levels")
    ap.add_argument("--kernel-stats", nargs="+", default=None, metavar="VARIANT=CSV", help="no run: append the kernel times of these rocprofv3 *_kernel_stats.csv files to --out")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--size", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return base.child(args)
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
    Loop = base.load_loop(ROOT)
    if args.trace:
        loop = Loop(args.trace, shared=False)
        prepare(loop, args.what, args.levels, args.ticks)
        timed(loop, 5, args.what, args.levels)
        timed(loop, args.ticks, args.what, args.levels)
        say("trace: %d + 5 ticks of one rollout at %d instances, variant: %s with %d levels" % (args.ticks, args.trace, args.what, args.levels))
        return 0
    import torch
    ok = True
    say("trace quantiles, CoM controller (xDim 6, uDim 3, N 20), %d ticks per run, %d alternating runs; M plant ticks/s: median (min .. max)" % (args.ticks, args.reps))
    if args.parent:
        ok = base.against_parent(args, say)  # (first: no process of this tool has the device open while the children run)
    for batch, shared in SIZES:
        if args.sizes and batch not in args.sizes:
            continue
        rates, mem, loops = {v: [] for v in VARIANTS}, {v: 0 for v in VARIANTS}, {}
        for v in VARIANTS:
            loops[v] = Loop(batch, shared)
            prepare(loops[v], v[0], v[1], args.ticks)
            timed(loops[v], 10, *v)
        hist_loop, hist_rates, hist_mem = Loop(batch, shared), [], 0
        timed_histories(hist_loop, 10, LEVELS[3])
        for _ in range(args.reps):
            for v in VARIANTS:
                dt, peak = timed(loops[v], args.ticks, *v)
                rates[v].append(batch * args.ticks / dt / 1e6)
                mem[v] = max(mem[v], peak)
            dt, peak = timed_histories(hist_loop, args.ticks, LEVELS[3])
            hist_rates.append(batch * args.ticks / dt / 1e6)
            hist_mem = max(hist_mem, peak)
        say("batch %d, per-instance systems, a plant of its own" % batch)
        for what, nq in VARIANTS:
            r = rates[(what, nq)]
            say("  trace of %2d rows, %d levels %s %8.1f  (%8.1f .. %8.1f)   peak memory of a run %8.1f MB   quantile buffer %7.1f KB"
                % (ROWS[what], nq, " " * 24, statistics.median(r), min(r), max(r), mem[(what, nq)] / 1e6, 1e-3 * args.ticks * ROWS[what] * nq * 8))
        say("  x_hist + u_hist, torch.sort along the batch, 3 levels %8.1f  (%8.1f .. %8.1f)   peak memory of a run %8.1f MB"
            % (statistics.median(hist_rates), min(hist_rates), max(hist_rates), hist_mem / 1e6))
        med = {v: statistics.median(rates[v]) for v in VARIANTS}
        for what in ("xu", "all"):
            say("  %2d rows: 3 levels / no quantiles = %.3f;  8 levels / no quantiles = %.3f  (no quantiles: spread %.1f)"
                % (ROWS[what], med[(what, 3)] / med[(what, 0)], med[(what, 8)] / med[(what, 0)], max(rates[(what, 0)]) - min(rates[(what, 0)])))
        say("  9 rows with 3 levels / torch.sort of the histories = %.3f;  the key buffer the setter takes: %.1f MB (9 rows), %.1f MB (16 rows)"
            % (med[("xu", 3)] / statistics.median(hist_rates), 9 * batch * 8e-6, 16 * batch * 8e-6))
        del loops, hist_loop
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
