"""Cases and recorded results of tests/test_axis_trip_bounds.py: the emulated body of the (instance, axis)-per-lane solver (lmpc_axis.hpp) in its
normal mode and in the tests' two-slot mode (COPRA_EMU_AXIS_QMAX2), on the workloads whose waves mix lanes without an active constraint, lanes
with fewer than the wave's largest active set and lanes that fill their slots.

    python tests/golden/gen_axis_trip_bounds.py          writes tests/golden/axis_trip_bounds.npz from the emulator of THIS tree

The arrays in the repository were recorded from the commit BEFORE the small dense algebra of a trip was bounded by the wave's largest active
set: the test asks for the same bits from the body as it is now.  Run it again only when a change is MEANT to move them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests", "emu")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(HERE, "axis_trip_bounds.npz")
KEYS = ("control", "trajectory", "status", "iter")


def cases():
    """name -> (workload, two-slot mode)"""
    from copra_amd import workloads
    out = {}
    out["com_v06"] = (workloads.com_preview(85, v_max=0.6, u_max=3.0, seed=25), False)
    out["com_v06_two_slot"] = (workloads.com_preview(85, v_max=0.6, u_max=3.0, seed=25), True)
    out["com_v025"] = (workloads.com_preview(85, v_max=0.25, u_max=1.2, seed=25), False)
    out["com_v025_two_slot"] = (workloads.com_preview(85, v_max=0.25, u_max=1.2, seed=25), True)
    out["jerk"] = (workloads.jerk_preview(42, nu=3, N=20, seed=23, v_max=0.3, j_max=6.0), False)
    out["jerk_two_slot"] = (workloads.jerk_preview(42, nu=3, N=20, seed=23, v_max=0.3, j_max=6.0), True)
    out["kinematic"] = (workloads.kinematic_preview(42), False)
    out["kinematic_two_slot"] = (workloads.kinematic_preview(42), True)
    # two rows per axis and step, the same at every step: a lower velocity limit as rows next to the upper bound (the builds with RPA = 2)
    wl = workloads.com_preview(42, v_max=0.3, u_max=1.5, seed=9)
    vsel = np.hstack([np.zeros((3, 3)), np.eye(3)])
    wl["cstrs"] = [wl["cstrs"][0], dict(kind="trajectory", E=-vsel, f=[0.3] * 3, ineq=True), wl["cstrs"][1]]
    out["com_two_rows"] = (wl, False)
    out["com_two_rows_two_slot"] = (wl, True)
    return out


def run(wl, two_slot):
    """the emulator's results for a case (the mode is an environment variable the harness reads at every solve)"""
    import pyemu
    old = os.environ.pop("COPRA_EMU_AXIS_QMAX2", None)
    if two_slot:
        os.environ["COPRA_EMU_AXIS_QMAX2"] = "1"
    try:
        return pyemu.lmpc_solve(wl["A"], wl["B"], wl["d"], wl["x0"], wl["N"], wl["costs"], wl["cstrs"])
    finally:
        os.environ.pop("COPRA_EMU_AXIS_QMAX2", None)
        if old is not None:
            os.environ["COPRA_EMU_AXIS_QMAX2"] = old


if __name__ == "__main__":
    rec = {}
    for name, (wl, two_slot) in cases().items():
        re = run(wl, two_slot)
        for k in KEYS:
            rec[name + "/" + k] = re[k]
        rec[name + "/lane_pass_finished"] = np.int64(re["lane_pass_finished"])
        print("%-24s finished in the solver %d of %d, picks up to %d" % (name, re["lane_pass_finished"], len(re["status"]), re["iter"][:, 0].max()))
    np.savez_compressed(PATH, **rec)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
