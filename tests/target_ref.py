"""The expectation of the steady-state targets (copra_batch_set_target, ABI 15; copra_amd/csrc/target_step.hpp) in numpy, natural indexing:
the systems M z = rhs, numpy's own solve, the extended-precision truth (tests/truth.py), the bound of the issue, and a restatement of the
kernel's elimination in the order its header writes down -- which decides what `singular` means, operation by operation.

  M = [[A - I, B], [H, 0]],  rhs = [-d, r],  z = [xs, us];  p_c = tile(T_c z, S_c)
  bound on z:  |z - z_true|_inf <= n^2 cond_inf(M) 2^-53 |z_true|_inf
  bound on a reference row i:  sum_j |T_ij| (bound on z)  +  (n + 1) 2^-53 (|T| |z_true|)_i"""
import numpy as np

import truth

U = 2.0 ** -53


def block_index(tau, offset, steps):
    return min(int(tau) + int(offset), int(steps) - 1)


def setpoint(signal, tau, offset, batch):
    """the block r of every instance, (batch, nu): signal of shape (nu,), (steps, nu) or (batch, steps, nu)"""
    s = np.asarray(signal, dtype=np.float64)
    if s.ndim == 1:
        s = s[None, :]
    if s.ndim == 2:
        return np.broadcast_to(s[block_index(tau, offset, s.shape[0])], (batch, s.shape[1])).copy()
    return s[:, block_index(tau, offset, s.shape[1]), :].copy()


def systems(A, B, d, H, r):
    """M (batch, n, n) and rhs (batch, n) exactly as the kernel forms them: A - I is one subtraction on the diagonal, -d a sign"""
    A, B, d, H, r = (np.asarray(a, dtype=np.float64) for a in (A, B, d, H, r))
    b, nx, nu = A.shape[0], A.shape[1], B.shape[2]
    n = nx + nu
    M = np.zeros((b, n, n))
    M[:, :nx, :nx] = A - np.eye(nx)
    M[:, :nx, nx:] = B
    M[:, nx:, :nx] = H
    rhs = np.concatenate([-d, r], axis=1)
    return M, rhs


def gepp(M, rhs):
    """the kernel's elimination restated (float64, every product and every sum rounded): z (batch, n) and the status (batch,)"""
    M = np.array(M, dtype=np.float64)
    b, n, _ = M.shape
    W = np.concatenate([M, np.asarray(rhs, dtype=np.float64)[:, :, None]], axis=2)  # the augmented rows
    with np.errstate(all="ignore"):
        amax = np.zeros(b)
        for j in range(n):
            for i in range(n):
                a = np.abs(W[:, i, j])
                amax = np.where(a > amax, a, amax)
        finite = np.isfinite(W).all(axis=(1, 2))
        tol = (float(n) * 2.0 ** -52) * amax
        singular = ~finite
        ar = np.arange(b)
        for k in range(n):
            p = np.full(b, k)
            best = np.abs(W[:, k, k])
            for i in range(k + 1, n):
                a = np.abs(W[:, i, k])
                win = a > best
                best = np.where(win, a, best)
                p = np.where(win, i, p)
            singular |= ~(best > tol)
            top, low = W[ar, k, k:].copy(), W[ar, p, k:].copy()
            W[ar, k, k:] = low
            W[ar, p, k:] = top
            piv = W[:, k, k]
            for i in range(k + 1, n):
                f = W[:, i, k] / piv
                W[:, i, k + 1:] = W[:, i, k + 1:] - f[:, None] * W[:, k, k + 1:]
        z = np.zeros((b, n))
        for i in range(n - 1, -1, -1):
            acc = W[:, i, n].copy()
            for j in range(i + 1, n):
                acc = acc - W[:, i, j] * z[:, j]
            z[:, i] = acc / W[:, i, i]
    return z, singular.astype(np.int32)


def rows(T, z):
    """T z in the kernel's order: ascending from 0.0"""
    T = np.asarray(T, dtype=np.float64)
    acc = np.zeros((z.shape[0], T.shape[0]))
    for j in range(T.shape[1]):
        acc = acc + T[None, :, j] * z[:, j:j + 1]
    return acc


def solve64(M, rhs):
    """numpy's own float64 solve per instance"""
    return np.stack([np.linalg.solve(M[i], rhs[i]) for i in range(M.shape[0])])


def solve_true(M, rhs):
    """the solution in extended precision (truth.lu_solve) with one step of refinement there, as longdouble"""
    LD = truth.LD
    out = np.zeros(rhs.shape, dtype=LD)
    for i in range(M.shape[0]):
        Ml, bl = M[i].astype(LD), rhs[i].astype(LD)
        z = truth.lu_solve(Ml, bl).reshape(-1)
        z = z + truth.lu_solve(Ml, bl - Ml @ z).reshape(-1)
        out[i] = z
    return out


def cond_inf(M):
    return np.array([np.linalg.cond(M[i], np.inf) for i in range(M.shape[0])])


def z_bound(M, z_true):
    """(batch,): n^2 cond_inf(M) 2^-53 |z_true|_inf"""
    n = M.shape[1]
    return n * n * cond_inf(M) * U * np.abs(np.asarray(z_true, dtype=np.float64)).max(axis=1)


def p_true_and_bound(T, M, z_true):
    """T z_true as float64 (batch, r) and the bound on every row"""
    T = np.asarray(T, dtype=np.float64)
    n = M.shape[1]
    zt = np.asarray(z_true)
    p = np.asarray(zt @ T.T.astype(zt.dtype), dtype=np.float64)
    bz = z_bound(M, z_true)
    bound = np.abs(T).sum(axis=1)[None, :] * bz[:, None] + (n + 1) * U * (np.abs(np.asarray(zt, dtype=np.float64)) @ np.abs(T).T)
    return p, bound


def step_map(cost, nx, nu, N):
    """T_c = [M_c N_c] of the STEP form of a cost dict (kind, M, N) and r_c: a per-step entry as it is, a full-size entry's first block"""
    M = None if cost.get("M") is None else np.atleast_2d(np.asarray(cost["M"], dtype=np.float64))
    Nm = None if cost.get("N") is None else np.atleast_2d(np.asarray(cost["N"], dtype=np.float64))
    R = (M if M is not None else Nm).shape[0]
    r = R
    if M is not None and M.shape[1] != nx:
        r = R // (N + 1 if cost["kind"] == "trajectory" else N)
    elif Nm is not None and Nm.shape[1] != nu:
        r = R // N
    T = np.zeros((r, nx + nu))
    if M is not None:
        T[:, :nx] = M[:r, :nx]
    if Nm is not None:
        T[:, nx:] = Nm[:r, :nu]
    return T, r
