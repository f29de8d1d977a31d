"""Controllers that several test modules build (no test of its own): a planar point mass and a generic coupled system."""
import numpy as np


def planar_integrator(b, N, seed=1, v_max=0.4, u_max=1.5, T=0.1):
    """(nx, nu) = (4, 2): a point mass in the plane, bounds on both velocities and both controls (the two axes differ in weights,
    bounds and goal: with identical axes the most-violated-constraint rule meets exact ties, which rounding breaks differently
    in the device's factor and in the CPU path's -- same optimum, other iteration counts)"""
    rng = np.random.default_rng(seed)
    A = np.tile(np.block([[np.eye(2), T * np.eye(2)], [np.zeros((2, 2)), np.eye(2)]]), (b, 1, 1))
    B = np.tile(np.vstack([0.5 * T * T * np.eye(2), T * np.eye(2)]), (b, 1, 1))
    A[:, 0, 2] *= rng.uniform(0.8, 1.2, b)  # (per-instance systems)
    d = np.zeros((b, 4))
    x0 = np.hstack([rng.normal(0, 0.2, (b, 2)), rng.uniform(-0.2, 0.2, (b, 2))])
    inf = np.inf
    costs = [dict(kind="trajectory", M=np.eye(4), p=np.array([0.45, 0.3, 0.0, 0.0]), weights=[10, 7, 1, 1.5]),
             dict(kind="control", N=np.eye(2), p=np.zeros(2), weights=[1e-3, 2e-3])]
    cstrs = [dict(kind="trajectory_bound", lower=[-inf] * 4, upper=[inf, inf, v_max, 0.85 * v_max]),
             dict(kind="control_bound", lower=[-u_max, -0.9 * u_max], upper=[u_max, 0.8 * u_max])]
    return dict(A=A, B=B, d=d, x0=x0, N=N, costs=costs, cstrs=cstrs)


def generic(nx, nu, N, b=3):
    rng = np.random.default_rng(18)
    A = np.tile(np.eye(nx) + 0.05 * rng.standard_normal((nx, nx)), (b, 1, 1))
    B = np.tile(0.3 * rng.standard_normal((nx, nu)), (b, 1, 1))
    costs = [dict(kind="trajectory", M=np.eye(nx), p=np.zeros(nx), weights=np.ones(nx)), dict(kind="control", N=np.eye(nu), p=np.zeros(nu), weights=[1e-2] * nu)]
    return dict(A=A, B=B, d=np.zeros((b, nx)), x0=rng.standard_normal((b, nx)), N=N, costs=costs, cstrs=[dict(kind="control_bound", lower=[-0.5] * nu, upper=[0.5] * nu)])
