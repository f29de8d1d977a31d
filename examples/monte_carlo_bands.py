"""The fleet of examples/monte_carlo_envelope.py with percentile bands: where 5 %, 50 % and 95 % of the robots lie at tick t.

Mean +- spread is a band for a Gaussian row.  The violation row -- zero for most of the fleet -- is none, a velocity against its bound is
none, and the extremes are one robot each.

  set_trace(capacity=ticks, state_limits=(None, v_max))
  set_trace_quantiles([0.05, 0.5, 0.95])

and every tick of rollout() then also selects, on the device, the exact order statistics of every row of the slot: an element of the data
per row and level, k = min(n - 1, max(0, ceil(p n) - 1)) of the n finite values (numpy's method="inverted_cdf").  rollout() is asked for no
x_hist and no u_hist; trace_quantiles() reads ticks x rows x 3 doubles back.  A caller of the C ABI gets the same buffer from
copra_batch_get_trace_quantiles (tests/cpp/test_trace_quant.cpp).

    python examples/monte_carlo_bands.py [batch] [ticks]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from copra_amd import BatchLMPC, workloads  # noqa: E402
from copra_amd.observer_design import kalman_gain  # noqa: E402

SIGMA_W = np.array([0.01, 0.01, 0.01, 0.005, 0.005, 0.005])
V_MAX = 0.6  # the velocity bound of workloads.com_preview: checked on the true state, which noise pushes across it
LEVELS = (0.05, 0.5, 0.95)


def closed_loop_bands(batch, ticks, seed, load=0.004, sensor_noise=0.01):
    """(trace, quantiles) of one closed-loop run -- the scenario of examples/monte_carlo_envelope.py::closed_loop_trace with quantiles"""
    wl = workloads.com_preview(batch)
    nx, nu, ny, N = 6, 3, 3, wl["N"]
    rng = np.random.default_rng(0)
    eng = BatchLMPC(nx, nu, N, batch, wl["costs"], wl["cstrs"])
    eng.set_system(wl["A"], wl["B"], wl["d"], wl["x0"])
    C = np.eye(nx)[:ny]
    G = np.zeros((nx, ny))
    G[3:] = np.eye(3)
    Lx, Ld = kalman_gain(wl["A"], C, 1e-4 * np.eye(nx), sensor_noise ** 2 * np.eye(ny) + 1e-4 * np.eye(ny), with_bias=True, Qd=1e-5 * np.eye(ny), Gd=G)
    eng.set_observer(C, Lx, Ld)
    xhat0 = wl["x0"].copy()
    xhat0[:, 3:] += 0.1 * rng.choice([-1.0, 1.0], (batch, 3))
    eng.set_x0(xhat0)
    c = np.zeros((batch, nx))
    c[:, 3:] = load * rng.uniform(-1.0, 1.0, (batch, 3))
    eng.set_noise(seed, process=SIGMA_W, sensor=np.full(ny, sensor_noise))
    upper = np.array([np.inf] * 3 + [V_MAX] * 3)
    eng.set_trace(ticks, state_limits=(None, upper), tol=1e-9)
    eng.set_trace_quantiles(LEVELS)
    eng.rollout(ticks, plant=(wl["A"], wl["B"], wl["d"] + c), stream=torch.cuda.current_stream().cuda_stream)  # no history at all
    return eng.trace(), eng.trace_quantiles()


def run(batch=4096, ticks=60, seed=2026, row=0):
    tr, q = closed_loop_bands(batch, ticks, seed)
    stat = tr["x"][:, row]
    std = np.sqrt(stat["m2"] / np.maximum(stat["n"] - 1, 1))
    lines = ["%d robots, %d ticks; position row %d and the largest violation of the velocity limit: mean +- spread beside the 5 / 50 / 95 %% band" % (batch, ticks, row)]
    for t in sorted({0, 1, 2, 5, 10, ticks // 2, ticks - 1}):
        if t >= ticks:
            continue
        p, v = q["x"][t, row], q["viol"][t]
        lines.append("  tick %3d: position %.4f +- %.4f, band [%.4f, %.4f, %.4f]; violation mean %.2e, band [%.2e, %.2e, %.2e], %5.2f %% violating"
                     % (tr["head"]["tick"][t], stat["mean"][t], std[t], p[0], p[1], p[2], tr["viol"]["mean"][t], v[0], v[1], v[2], 100.0 * tr["head"]["violating"][t] / batch))
    lines.append("bytes read back for the bands: %d; x_hist and u_hist would have taken %d" % (q["x"].nbytes + q["u"].nbytes + q["viol"].nbytes, 8 * batch * ((ticks + 1) * 6 + ticks * 3)))
    assert (q["x"][:, :, 0] <= q["x"][:, :, 1]).all() and (q["x"][:, :, 1] <= q["x"][:, :, 2]).all()
    assert (tr["x"]["min"] <= q["x"][:, :, 0]).all() and (q["x"][:, :, 2] <= tr["x"]["max"]).all()
    return lines


if __name__ == "__main__":
    b = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    print("\n".join(run(b, k)))
