"""Random controllers on the shapes of the (instance, axis)-per-lane solver (tests/random_controllers.py: make_integrator, make_chain3, make_chain1; now and then
in axis-major state order, with a goal per instance, with cost weights per instance) through the CPU wave emulator of the kernel bodies against the oracle: statuses, iteration
counters, U and X.   python tests/fuzz/fuzz_axis_emulator.py [--limits] [first_seed [count [batch]]]
--limits: every instance its own right-hand sides and control bounds as well (random_controllers.draw_limits: the solver keeps the controller only where
both its builds read them, pyemu.last_axis_run() says whether it did)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "emu"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pyemu  # noqa: E402
import pyoracle  # noqa: E402
import random_controllers as RC  # noqa: E402


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3))) if a.size else 0.0


argv = [a for a in sys.argv[1:] if a != "--limits"]
with_limits = "--limits" in sys.argv[1:]
first = int(argv[0]) if len(argv) > 0 else 0
count = int(argv[1]) if len(argv) > 1 else 60
b = int(argv[2]) if len(argv) > 2 else 24
nbad = ntie = naxis = 0
for seed in range(first, first + count):
    rng = np.random.default_rng([seed, 5])
    c = RC.make_chain3(seed, b) if seed % 4 == 0 else RC.make_chain1(seed, b) if seed % 4 == 2 else RC.make_integrator(seed, b)
    if c["nu"] == 1:
        continue
    what = list(c["forms"])
    refs = None
    plain_goal = c["costs"][0]["kind"] == "trajectory" and np.asarray(c["costs"][0]["p"]).size == c["nx"]
    if plain_goal and rng.random() < 0.4:
        refs = {0: np.tile(c["costs"][0]["p"], (b, 1)) + 0.1 * rng.standard_normal((b, c["nx"]))}
        what.append("own goals")
    # weights per instance on a third of the controllers: log-uniform in [0.1, 10] x the creation weights, row by row (the headline's shape runs the
    # solver's weight-reading builds, the other shapes and zero creation weights the generic tier: pyemu.last_axis_run() says which)
    wts = None
    if rng.random() < 0.33:
        wts = {t: np.asarray(cs["weights"], dtype=float)[None, :] * np.exp(rng.uniform(np.log(0.1), np.log(10.0), (b, np.size(cs["weights"]))))
               for t, cs in enumerate(c["costs"]) if cs.get("weights") is not None and cs["kind"] != "dense"
               and np.size(cs["weights"]) == np.size(cs["p"]) and np.size(cs["p"]) in (c["nx"], c["nu"])}
        what.append("own weights on %s" % sorted(wts))
    lim = RC.draw_limits(c, seed) if with_limits else dict(rhs={}, bounds=None, row_rhs=None)
    re = pyemu.lmpc_solve(c["A"], c["B"], c["d"], c["x0"], c["N"], c["costs"], c["cstrs"], cost_refs=refs, cost_weights=wts, row_rhs=lim["row_rhs"],
                          bounds=lim["bounds"])
    run = pyemu.last_axis_run()
    if with_limits:
        what.append("own limits (%s%s), %s" % ("rhs " if lim["rhs"] else "", "bounds" if lim["bounds"] else "", "solver" if run else "tiers"))
        if run and (lim["rhs"] or lim["bounds"]) and not (run["first"][6] and run["second"][6]):
            what.append("A BUILD THAT DOES NOT READ THEM")
            nbad += 1
    if wts:
        what.append("builds %s" % (run["first"][0] if run else "generic"))
    bad = tie = 0
    worst = 0.0
    for k in range(b):
        costs = c["costs"] if refs is None else [dict(c["costs"][0], p=refs[0][k])] + c["costs"][1:]
        if wts:
            costs = [dict(cs, weights=wts[t][k]) if t in wts else cs for t, cs in enumerate(costs)]
        ro = pyoracle.lmpc_solve(c["A"][k], c["B"][k], c["d"][k], c["x0"][k], c["N"], costs, RC.instance_cstrs(c, lim, k))
        if re["status"][k] != ro["status"]:
            bad += 1
            continue
        if ro["status"] != 0:
            continue
        tie += int(tuple(re["iter"][k]) != tuple(ro["iter"]))
        if wts:  # (scattered weights: norm-wise per instance, tests/cost_weights_cases.py::rel_inst)
            worst = max(worst, np.abs(re["control"][k] - ro["control"]).max() / max(np.abs(ro["control"]).max(), 1e-3),
                        np.abs(re["trajectory"][k] - ro["trajectory"]).max() / max(np.abs(ro["trajectory"]).max(), 1e-3))
        else:
            worst = max(worst, rel(re["control"][k], ro["control"]), rel(re["trajectory"][k], ro["trajectory"]))
    axis = re.get("lane_pass_finished", 0)
    naxis += int(axis > 0)
    flag = "   <<<<<<" if bad or worst > 1e-6 else ("   < counters" if tie else "")
    nbad += int(bool(bad or worst > 1e-6))
    ntie += tie
    print("%4d (%d, %d, %d) %s: ended in the pass / solver %d of %d, status differ %d, counters differ %d, rel %.1e%s" % (seed, c["nx"], c["nu"], c["N"], what, axis, b, bad, tie, worst, flag), flush=True)
print("controllers with a status or value mismatch: %d; instances with other counters: %d; controllers that ran a per-lane kernel: %d" % (nbad, ntie, naxis))
