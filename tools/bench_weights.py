"""Per-instance cost weights (copra_batch_set_cost_weights) at the headline shape: solves/s at batch 65 536 with per-instance weights, next to
the rate without them, with per-instance goals and with the (instance, axis)-per-lane solver switched off -- all in the same run -- and the
C++ mirror's solve after CostFunction::weights(...) with the setter and with a new handle (tests/cpp/test_weights.cpp measure).
Prints one JSON line.  Usage: python tools/bench_weights.py [--batch 65536] [--steps 20] [--warmup 8]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rate(wl, b, steps, warmup, setup=None, **opts):
    import torch
    from copra_amd import BatchLMPC, _capi
    saved = dict(_capi.OPTIONS)
    _capi.OPTIONS.update(opts)
    try:
        eng = BatchLMPC(6, 3, wl["N"], b, wl["costs"], wl["cstrs"])
    finally:
        _capi.OPTIONS.clear()
        _capi.OPTIONS.update(saved)
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    keep = setup(eng, torch) if setup else None
    for _ in range(warmup):
        eng.solve()
    eng.synchronize()
    ts = []
    for _ in range(steps):
        eng.solve()
        eng.synchronize()
        ts.append(eng.last_solve_seconds())
    ran = eng.axis_solver_ran()
    ok = float((eng.results()["status"] == 0).mean())
    eng.close()
    del keep
    ms = float(np.median(ts)) * 1e3
    return dict(ms=round(ms, 4), msolves_per_s=round(b / ms * 1e-3, 1), axis_solver=bool(ran), solved_share=ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    a = ap.parse_args()
    from copra_amd import workloads
    b = a.batch
    wl = workloads.com_preview(b)
    rng = np.random.default_rng(5)
    group = rng.integers(0, 64, b)
    ws = [np.asarray(c["weights"], dtype=np.float64)[None, :] * np.exp(rng.uniform(np.log(0.1), np.log(10.0), (64, len(c["weights"]))))[group]
          for c in wl["costs"]]
    goals = workloads.COM_X_GOAL[None, :] + 0.05 * rng.standard_normal((b, 6))

    def own_weights(eng, torch):
        dev = [torch.from_numpy(np.ascontiguousarray(w)).cuda() for w in ws]
        for t, w in enumerate(dev):
            eng.set_cost_weights(t, w)
        return dev

    def own_goals(eng, torch):
        g = torch.from_numpy(np.ascontiguousarray(goals)).cuda()
        eng.set_cost_reference(0, g)
        return g

    out = dict(batch=b, shape="com_preview nx=6 nu=3 N=20")
    out["plain"] = _rate(wl, b, a.steps, a.warmup)
    out["own_goals"] = _rate(wl, b, a.steps, a.warmup, own_goals)
    out["own_weights"] = _rate(wl, b, a.steps, a.warmup, own_weights)
    out["plain_no_axis_solver"] = _rate(wl, b, a.steps, a.warmup, no_axis_solver=1)
    # the C++ mirror: one solve after weights(...), setter vs a new handle
    from copra_amd import _capi
    exe = os.path.join(ROOT, "tests", "cpp", "test_weights")
    libdir = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "copra_amd", "cpp", "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_weights.cpp"), "-o", exe, "-L", libdir, "-lcopra_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, "measure"], capture_output=True, text=True, timeout=600)
    for line in r.stdout.splitlines():
        if line.startswith("measure_"):
            k, v = line.split(":")
            out["cpp_" + k] = float(v)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
