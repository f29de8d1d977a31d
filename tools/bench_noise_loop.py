"""What drawing the noise on the device costs the closed loop (copra_batch_set_noise), on the CoM controller at the sizes of
tools/bench_closed_loop.py, whose Loop (controller, result slab, timing around a final synchronisation) is used as it is, for the plain tick
and for the observer loop of tools/bench_observer_loop.py (positions measured, gains shared by the batch, Ld).

    python tools/bench_noise_loop.py [--ticks 200] [--reps 5] [--parent DIR] [--out profiles/closed_loop/noise_rates.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_noise_loop.py --trace 65536 --noise device [--observer]
    python tools/bench_noise_loop.py --kernel-stats "plain, explicit"=CSV "plain, device"=CSV ... --out FILE      (appends the kernel times)

(a) --parent DIR: a checkout of the PARENT commit with its library built.  `reps` runs of the parent's rollout and `reps` of this tree's with
    noise never enabled, alternating, each in a process of its own (a process loads one build), for both loops; this tree's median may be
    lower than the parent's by at most the parent's own min .. max spread.  The exit status is 1 if it is not.
(b) per size and loop, `reps` alternating runs of ONE rollout(ticks) each with
      explicit arrays: w_seq (and v_seq) = sigma * torch.randn, generated outside the timed region | device noise of the same sigma
    on one controller per variant, warmed up outside the timed region.  Rates in M plant ticks/s (instances x ticks / s).  No threshold.
(c) the device memory each variant holds for its noise.
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
SIGMA_W = (0.002, 0.002, 0.002, 0.0005, 0.0005, 0.0005)
SIGMA_V = (0.002, 0.002, 0.002)
SEED = 2026


def load(root):
    """Loop and the observer of `root`'s tools, which put `root` in front of sys.path themselves: the package of that tree is the one imported"""
    sys.path.insert(0, os.path.join(root, "tools"))
    from bench_closed_loop import Loop
    from bench_observer_loop import make_observer
    return Loop, make_observer


def explicit(loop, ticks, sigma):
    import torch
    s = torch.tensor(sigma, dtype=torch.float64, device=loop.dev)
    return s * torch.randn(ticks, loop.batch, len(sigma), device=loop.dev, generator=loop.gen, dtype=torch.float64)


def timed_rollout(loop, ticks, obs=None, noise="off"):
    """one rollout with a plant of its own.  noise "off": nothing of the feature is called (a tree without it, or noise never enabled);
    "explicit": w_seq / v_seq from torch.randn; "device": copra_batch_set_noise"""
    import numpy as np
    import torch
    loop.hand_over(loop.x_start.clone())
    kw = dict(plant=(loop.A, loop.B, loop.d))
    if obs is not None:
        loop.eng.set_observer(*obs)
        loop.eng.set_plant_state(loop.x_start)
    if noise == "explicit":
        kw["disturbances"] = explicit(loop, ticks, SIGMA_W)
        if obs is not None:
            kw["noise"] = explicit(loop, ticks, SIGMA_V)
    elif noise == "device":
        loop.eng.set_noise(SEED, process=np.array(SIGMA_W), sensor=np.array(SIGMA_V) if obs is not None else None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.eng.rollout(ticks, stream=loop.stream, **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def noise_bytes(batch, ticks, observer, noise):
    """device memory held for the noise of one rollout"""
    rows = NX + (NY if observer else 0)
    return 8 * rows * (ticks * batch if noise == "explicit" else 1)


def kernel_times(pairs, say):
    """the project's kernels out of rocprofv3's *_kernel_stats.csv files, one per variant: calls and the average time of each per launch"""
    import csv
    say("kernel times at 65 536 instances, per-instance systems and a plant of its own, from separate rocprofv3 --kernel-trace --stats runs of --trace "
        "(us per launch, calls):")
    for pair in pairs:
        name, path = pair.split("=", 1)
        with open(path, newline="") as fh:
            rows = [r for r in csv.DictReader(fh) if "copra_plant" in r["Name"] or "copra_noise" in r["Name"]]
        say("  variant: %s" % name)
        for r in rows:
            kernel = r["Name"].replace("void ", "").split("(")[0]
            say("    %-60s %8.1f  x %s" % (kernel, float(r["AverageNs"]) / 1e3, r["Calls"]))


def child(args):
    """one timed run in this process, noise never enabled: prints the rate"""
    Loop, make_observer = load(args.child)
    batch = SIZES[args.size]
    loop = Loop(batch, False)
    obs = make_observer(loop, "shared", True) if args.observer else None
    timed_rollout(loop, 10, obs)
    print("RATE %.6f" % (batch * args.ticks / timed_rollout(loop, args.ticks, obs) / 1e6), flush=True)


def against_parent(args, say):
    ok = True
    for size, batch in enumerate(SIZES):
        for observer in (False, True):
            rates = {args.parent: [], ROOT: []}
            for _ in range(args.reps):
                for root in (args.parent, ROOT):
                    cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--size", str(size), "--ticks", str(args.ticks)]
                    out = subprocess.run(cmd + (["--observer"] if observer else []), check=True, capture_output=True, text=True, timeout=600).stdout
                    rates[root].append(float([ln for ln in out.splitlines() if ln.startswith("RATE ")][-1].split()[1]))
            p, o = rates[args.parent], rates[ROOT]
            spread = max(p) - min(p)
            lower = statistics.median(p) - statistics.median(o)
            good = lower <= spread
            ok = ok and good
            say("(a) batch %d, %s, noise never enabled: rollout, one process per run" % (batch, "observer loop" if observer else "plain tick"))
            say("  parent            %8.1f  (%8.1f .. %8.1f)   spread %.1f" % (statistics.median(p), min(p), max(p), spread))
            say("  this tree         %8.1f  (%8.1f .. %8.1f)" % (statistics.median(o), min(o), max(o)))
            say("  parent - this tree = %+.1f M ticks/s: %s" % (lower, "within the parent's spread" if good else "LOWER than the parent by more than its spread"))
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit, its library built: the bar on the path with noise never enabled")
    ap.add_argument("--trace", type=int, default=0, help="only `ticks` ticks of one rollout at this batch size (for a kernel trace)")
    ap.add_argument("--noise", choices=("off", "explicit", "device"), default="off", help="with --trace: where the noise comes from")
    ap.add_argument("--observer", action="store_true", help="with --trace: the observer loop")
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
        Loop, make_observer = load(ROOT)
        loop = Loop(args.trace, False)
        obs = make_observer(loop, "shared", True) if args.observer else None
        timed_rollout(loop, 5, obs, args.noise)
        timed_rollout(loop, args.ticks, obs, args.noise)
        say("trace: %d + 5 ticks of one rollout at %d instances, a plant of its own, %s, noise: %s"
            % (args.ticks, args.trace, "observer loop" if args.observer else "plain tick", args.noise))
        return 0
    ok = True
    say("noise drawn on the device in the closed loop, CoM controller (xDim 6, uDim 3, N 20), %d ticks per run, %d alternating runs; "
        "M plant ticks/s: median (min .. max)" % (args.ticks, args.reps))
    if args.parent:
        ok = against_parent(args, say)  # (first: no process of this tool has the device open while the children run)
    Loop, make_observer = load(ROOT)
    variants = [(observer, noise) for observer in (False, True) for noise in ("explicit", "device")]
    for batch in SIZES:
        loops = [Loop(batch, False) for _ in variants]
        obs = [make_observer(loop, "shared", True) if v[0] else None for loop, v in zip(loops, variants)]
        for loop, o, v in zip(loops, obs, variants):  # module load, LDS opt-in, first-solve set-up, the engine's adaptation
            timed_rollout(loop, 10, o, v[1])
        rates = [[] for _ in variants]
        for _ in range(args.reps):
            for r, loop, o, v in zip(rates, loops, obs, variants):
                r.append(batch * args.ticks / timed_rollout(loop, args.ticks, o, v[1]) / 1e6)
        say("(b), (c) batch %d, per-instance systems, a plant of its own; the explicit arrays are generated outside the timed region" % batch)
        for r, v in zip(rates, variants):
            say("  %-14s %-9s %8.1f  (%8.1f .. %8.1f)   holds %d B for its noise"
                % ("observer loop," if v[0] else "plain tick,", v[1], statistics.median(r), min(r), max(r), noise_bytes(batch, args.ticks, v[0], v[1])))
        for i in (0, 2):
            say("  %s device / explicit = %.3f" % ("observer loop:" if variants[i][0] else "plain tick:", statistics.median(rates[i + 1]) / statistics.median(rates[i])))
        del loops, obs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
