"""What output feedback costs the closed loop (copra_batch_set_observer), on the CoM controller at the sizes of tools/bench_closed_loop.py,
whose Loop (controller, result slab, disturbances, timing around a final synchronisation) is used as it is.

    python tools/bench_observer_loop.py [--ticks 200] [--reps 5] [--parent DIR] [--out profiles/closed_loop/observer_rates.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_observer_loop.py --trace 65536 --gains each --ld   (the plant step's own time)
    python tools/bench_observer_loop.py --kernel-stats off=CSV shared=CSV each+ld=CSV --out FILE      (appends those runs' kernel times to FILE)

Per size (16 384 and 65 536 instances, per-instance systems: the observer needs them), `reps` alternating runs of ONE rollout(ticks) each with
  the observer never enabled | positions measured (ny = 3), gains shared by the batch or one per instance, each with and without Ld
on one controller per variant, created and warmed up outside the timed region; set_system and set_plant_state start the episode of every run.
Every variant is given a plant of its own per instance (the model's arrays), as in tools/bench_bias_loop.py.  Rates are in M plant ticks/s
(instances x ticks / s).  Beside them, the bytes per instance and tick the observer adds to the plant step's traffic, from the shapes.

Against the host-driven loop on the same build: per tick that loop solves, applies the plant on the device (advance, observer off), reads the
state back, runs the observer in numpy and calls set_x0 and set_bias -- the round trip the observer in the tick removes.

--parent DIR: a checkout of the PARENT commit with its library built.  The bar on the off path: `reps` runs of the parent's rollout and `reps`
of this tree's with the observer never enabled, alternating, each in a process of its own (a process loads one build); this tree's median may
be lower than the parent's by at most the parent's own min .. max spread.  The exit status is 1 if it is not.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (16384, 65536)
NX, NU, NY = 6, 3, 3
VARIANTS = (("observer off", None, False), ("shared gains", "shared", False), ("shared gains, Ld", "shared", True),
            ("gains per instance", "each", False), ("gains per instance, Ld", "each", True))


def load_loop(root):
    """Loop of `root`'s tools/bench_closed_loop.py, which puts `root` in front of sys.path itself: the package of that tree is the one imported"""
    sys.path.insert(0, os.path.join(root, "tools"))
    from bench_closed_loop import Loop
    return Loop


def make_observer(loop, kind, with_ld):
    """(C, Lx, Ld) as torch tensors in ABI layout (column-major blocks: C (.., nx, ny), gains (.., ny, nx)), used in place"""
    import torch
    C = torch.zeros((NX, NY), dtype=torch.float64, device=loop.dev)
    C[:NY, :NY] = torch.eye(NY, dtype=torch.float64, device=loop.dev)
    Lx = torch.zeros((NY, NX), dtype=torch.float64, device=loop.dev)
    Lx[:, :NY] = 0.45 * torch.eye(NY, dtype=torch.float64, device=loop.dev)
    Lx[:, NY:] = 0.8 * torch.eye(NY, dtype=torch.float64, device=loop.dev)
    Ld = torch.zeros((NY, NX), dtype=torch.float64, device=loop.dev)
    Ld[:, NY:] = 0.07 * torch.eye(NY, dtype=torch.float64, device=loop.dev)
    if kind == "each":
        C, Lx, Ld = (m.expand(loop.batch, *m.shape).contiguous() for m in (C, Lx, Ld))
    return C, Lx, (Ld if with_ld else None)


def sensor_noise(loop, ticks):
    import torch
    return 0.002 * torch.randn(ticks, loop.batch, NY, device=loop.dev, generator=loop.gen, dtype=torch.float64)


def timed_rollout(loop, ticks, obs=None):
    """Loop.run("rollout", ticks) with a plant of its own; obs None: nothing of the feature is called (a tree without it, or the observer never
    enabled)"""
    import torch
    x = loop.x_start.clone()
    loop.hand_over(x)  # (observer on with Ld: the estimates restart from the model's d)
    kw = dict(plant=(loop.A, loop.B, loop.d))
    if obs is not None:
        loop.eng.set_observer(*obs)
        loop.eng.set_plant_state(loop.x_start)
        kw["noise"] = sensor_noise(loop, ticks)
    w = loop.disturbances(ticks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.eng.rollout(ticks, disturbances=w, stream=loop.stream, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def timed_host_loop(loop, ticks, with_ld):
    """the loop a user of ABI 11 runs for output feedback: the plant on the device, the observer on the host, every tick"""
    import numpy as np
    import torch
    x = loop.x_start.clone()
    loop.hand_over(x)
    A, B = (np.swapaxes(m.cpu().numpy(), 1, 2) for m in (loop.A, loop.B))
    dhat = loop.d.cpu().numpy().copy()
    if with_ld:
        loop.eng.set_bias_estimator(np.zeros(NX))  # (the library's buffer of estimates, which set_bias writes; a zero gain: the host estimates)
    xhat = loop.x_start.cpu().numpy().copy()
    w = loop.disturbances(ticks)
    v = sensor_noise(loop, ticks).cpu().numpy()
    Lx = np.zeros((NX, NY))
    Lx[:NY], Lx[NY:] = 0.45 * np.eye(NY), 0.8 * np.eye(NY)
    Ld = np.zeros((NX, NY))
    Ld[NY:] = 0.07 * np.eye(NY)
    xp = loop.x_start.clone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(ticks):
        loop.eng.solve(loop.stream)
        loop.eng.set_x0(xp)  # the plant moves its own state: the tick applies the control of the solve to it ...
        out = loop.eng.advance(plant=(loop.A, loop.B, loop.d), disturbance=w[t], u_out=True, x_out=True, stream=loop.stream)
        xp = out["x_out"]
        y = xp[:, :NY].cpu().numpy() + v[t]  # ... and the host reads the outputs back,
        u = np.nan_to_num(out["u_out"].cpu().numpy())
        xpred = np.einsum("bij,bj->bi", A, xhat) + np.einsum("bij,bj->bi", B, u) + dhat
        inn = y - xpred[:, :NY]
        xhat = xpred + inn @ Lx.T  # runs the observer
        loop.eng.set_x0(xhat)  # and hands the estimates over
        if with_ld:
            dhat = dhat + inn @ Ld.T
            loop.eng.set_bias(dhat)
    torch.cuda.synchronize()
    if with_ld:
        loop.eng.set_bias_estimator(None)
    return time.perf_counter() - t0


def extra_bytes(kind, with_ld):
    """doubles the observer adds per instance and tick to the tick with a plant of its own, as bytes: the model beside the plant, xhat read and
    written, v read; dhat written with Ld; C, Lx (and Ld) per instance"""
    n = NX * NX + NX * NU + NX + 2 * NX + NY + (NX if with_ld else 0)
    if kind == "each":
        n += (3 if with_ld else 2) * NX * NY
    return 8 * n


def kernel_times(pairs, say):
    """the project's kernels out of rocprofv3's *_kernel_stats.csv files, one per variant: calls and the average time of each per launch"""
    import csv
    say("kernel times at 65 536 instances, per-instance systems and a plant of its own, from separate rocprofv3 --kernel-trace --stats runs of --trace "
        "(us per launch, calls); the disturbance estimator's plant step takes 28.8 (diagonal) / 32.7 (dense) us there:")
    for pair in pairs:
        name, path = pair.split("=", 1)
        with open(path, newline="") as fh:
            rows = [r for r in csv.DictReader(fh) if "copra_" in r["Name"]]
        say("  variant: %s" % name)
        for r in rows:
            kernel = r["Name"].replace("void ", "").split("(")[0]
            say("    %-52s %8.1f  x %s" % (kernel, float(r["AverageNs"]) / 1e3, r["Calls"]))


def child(args):
    """one timed run in this process: prints the rate"""
    Loop = load_loop(args.child)
    batch = SIZES[args.size]
    loop = Loop(batch, False)
    timed_rollout(loop, 10)
    print("RATE %.6f" % (batch * args.ticks / timed_rollout(loop, args.ticks) / 1e6), flush=True)


def against_parent(args, say):
    ok = True
    for size, batch in enumerate(SIZES):
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
        say("batch %d, per-instance systems, a plant of its own: rollout, one process per run" % batch)
        say("  parent            %8.1f  (%8.1f .. %8.1f)   spread %.1f" % (statistics.median(p), min(p), max(p), spread))
        say("  observer off      %8.1f  (%8.1f .. %8.1f)" % (statistics.median(o), min(o), max(o)))
        say("  parent - off = %+.1f M ticks/s: %s" % (lower, "within the parent's spread" if good else "LOWER than the parent by more than its spread"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-ticks", type=int, default=20, help="ticks of the host-driven loop per run (it is slow)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built: the bar on the off path")
    ap.add_argument("--trace", type=int, default=0, help="only `ticks` ticks of one rollout at this batch size (for a kernel trace)")
    ap.add_argument("--gains", choices=("off", "shared", "each"), default="off", help="with --trace: the observer's gains")
    ap.add_argument("--ld", action="store_true", help="with --trace: with Ld")
    ap.add_argument("--kernel-stats", nargs="+", default=None, metavar="VARIANT=CSV",
                    help="no run: append the kernel times of these rocprofv3 *_kernel_stats.csv files (one per --trace run) to --out")
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
        loop = load_loop(ROOT)(args.trace, False)
        obs = None if args.gains == "off" else make_observer(loop, args.gains, args.ld)
        timed_rollout(loop, 5, obs)
        timed_rollout(loop, args.ticks, obs)
        say("trace: %d + 5 ticks of one rollout at %d instances, a plant of its own, gains: %s%s" % (args.ticks, args.trace, args.gains, ", Ld" if args.ld else ""))
        return 0
    ok = True
    say("output feedback in the closed loop, CoM controller (xDim 6, uDim 3, N 20), positions measured (ny 3), %d ticks per run, %d alternating runs; "
        "M plant ticks/s: median (min .. max)" % (args.ticks, args.reps))
    if args.parent:
        ok = against_parent(args, say)  # (first: no process of this tool has the device open while the children run)
    Loop = load_loop(ROOT)
    for batch in SIZES:
        loops = [Loop(batch, False) for _ in VARIANTS]
        obs = [None if v[1] is None else make_observer(loop, v[1], v[2]) for loop, v in zip(loops, VARIANTS)]
        for loop, o in zip(loops, obs):  # module load, LDS opt-in, first-solve set-up, the engine's adaptation
            timed_rollout(loop, 10, o)
        rates = [[] for _ in VARIANTS]
        for _ in range(args.reps):
            for r, loop, o in zip(rates, loops, obs):
                r.append(batch * args.ticks / timed_rollout(loop, args.ticks, o) / 1e6)
        say("batch %d, per-instance systems, a plant of its own" % batch)
        for r, v in zip(rates, VARIANTS):
            say("  %-28s %8.1f  (%8.1f .. %8.1f)%s" % (v[0], statistics.median(r), min(r), max(r),
                                                       "" if v[1] is None else "   + %d B per instance and tick" % extra_bytes(v[1], v[2])))
        base = statistics.median(rates[0])
        for r, v in zip(rates[1:], VARIANTS[1:]):
            say("  %s / observer off = %.3f" % (v[0], statistics.median(r) / base))
        del loops[1:], obs
        host = loops[0]
        for with_ld, on in ((False, rates[1]), (True, rates[2])):
            timed_host_loop(host, 3, with_ld)
            h = [batch * args.host_ticks / timed_host_loop(host, args.host_ticks, with_ld) / 1e6 for _ in range(args.reps)]
            say("  host-driven loop%s        %8.1f  (%8.1f .. %8.1f)   observer in the tick / host-driven = %.1f"
                % (", Ld" if with_ld else "    ", statistics.median(h), min(h), max(h), statistics.median(on) / statistics.median(h)))
        del loops, host
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
