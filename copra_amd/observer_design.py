"""Gains for the state observer of the tick (BatchLMPC.set_observer, copra_batch_set_observer): the steady-state Kalman filter, batched numpy.

The tick runs the filter in its current (predictor-corrector) form,
    xpred = A xhat + B u + dhat;   inn = y - C xpred;   xhat+ = xpred + Lx inn;   dhat+ = dhat + Ld inn
so the gains are those of the PRIOR covariance P, the fixed point of the filter Riccati recursion
    K = P C' (C P C' + Rv)^-1;   P <- A (P - K C P) A' + Qw
and Lx = K.  With with_bias the model is augmented with an integrating disturbance delta that enters the state through Gd, d = Gd delta:
    [x; delta]+ = [[A, Gd], [0, I]] [x; delta] + [w; w_d],   y = [C, 0] [x; delta]
whose gain splits into Lx (its first nx rows) and Ld = Gd K_delta, the gain on d itself.  Pure host code: numpy only."""
import numpy as np


def _stack(M, lead, shape, name):
    M = np.asarray(M, dtype=np.float64)
    if M.shape[-2:] != shape:
        raise ValueError("kalman_gain: %s must be %s, got %s" % (name, shape, M.shape[-2:]))
    return np.broadcast_to(M, lead + shape)


def kalman_gain(A, C, Qw, Rv, with_bias=False, Qd=None, Gd=None, tol=1e-13, max_iter=20000, return_info=False):
    """Steady-state gains of the Kalman filter in the form the tick uses.  A (.., nx, nx), C (.., ny, nx), Qw (.., nx, nx), Rv (.., ny, ny) in
    natural indexing; leading dimensions broadcast (one system, or a batch of them).  Returns Lx (.., nx, ny); with with_bias (Lx, Ld), both
    (.., nx, ny), for the model augmented with the disturbance d = Gd delta: Gd (.., nx, nd) defaults to the identity (a disturbance on every
    state), Qd (.., nd, nd), the covariance of delta's random walk, to the identity scaled to the mean diagonal of Qw.  return_info appends a
    dict(P, A, C, Q, iterations): the fixed point and the (augmented) system it belongs to.
    Raises ValueError where the recursion does not converge within max_iter iterations or leaves the positive definite cone -- an unobservable
    pair (C = 0), or more disturbance states than outputs (nd > ny is never observable: ask for fewer through Gd)."""
    A = np.asarray(A, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    nx, ny = A.shape[-1], C.shape[-2]
    if A.shape[-2:] != (nx, nx) or C.shape[-1] != nx:
        raise ValueError("kalman_gain: A must be (.., nx, nx) and C (.., ny, nx)")
    lead = np.broadcast_shapes(A.shape[:-2], C.shape[:-2], np.shape(Qw)[:-2], np.shape(Rv)[:-2])
    A, C = _stack(A, lead, (nx, nx), "A"), _stack(C, lead, (ny, nx), "C")
    Q, R = _stack(Qw, lead, (nx, nx), "Qw"), _stack(Rv, lead, (ny, ny), "Rv")
    nd = 0
    if with_bias:
        G = np.eye(nx) if Gd is None else np.asarray(Gd, dtype=np.float64)
        nd = G.shape[-1]
        if nd > ny:
            raise ValueError("kalman_gain: %d disturbance states are not observable from %d outputs (give Gd with at most %d columns)" % (nd, ny, ny))
        G = _stack(G, lead, (nx, nd), "Gd")
        Qdd = _stack(np.eye(nd) * float(np.mean(np.diagonal(Q, axis1=-2, axis2=-1))) if Qd is None else Qd, lead, (nd, nd), "Qd")
        n = nx + nd
        Aa = np.zeros(lead + (n, n))
        Aa[..., :nx, :nx], Aa[..., :nx, nx:], Aa[..., nx:, nx:] = A, G, np.eye(nd)
        Ca = np.zeros(lead + (ny, n))
        Ca[..., :nx] = C
        Qa = np.zeros(lead + (n, n))
        Qa[..., :nx, :nx], Qa[..., nx:, nx:] = Q, Qdd
        A, C, Q = Aa, Ca, Qa
    At, Ct = np.swapaxes(A, -1, -2), np.swapaxes(C, -1, -2)
    P = Q.copy()
    K = None
    for it in range(1, max_iter + 1):
        S = C @ P @ Ct + R
        K = np.swapaxes(np.linalg.solve(np.swapaxes(S, -1, -2), C @ np.swapaxes(P, -1, -2)), -1, -2)  # P C' S^-1
        Pn = A @ (P - K @ C @ P) @ At + Q
        Pn = 0.5 * (Pn + np.swapaxes(Pn, -1, -2))
        scale = np.abs(Pn).max(axis=(-1, -2), keepdims=True)
        if not np.isfinite(scale).all():
            raise ValueError("kalman_gain: the Riccati recursion diverged (the pair (A, C) is not detectable)")
        done = (np.abs(Pn - P) <= tol * scale).all()
        P = Pn
        if done:
            break
    else:
        raise ValueError("kalman_gain: the Riccati recursion did not converge in %d iterations (an unobservable pair?)" % max_iter)
    S = C @ P @ Ct + R
    K = np.swapaxes(np.linalg.solve(np.swapaxes(S, -1, -2), C @ np.swapaxes(P, -1, -2)), -1, -2)
    # a fixed point of a pair that is not detectable can still be reached (C = 0 with a stable A): the observer must contract on its own
    rho = np.abs(np.linalg.eigvals((np.eye(A.shape[-1]) - K @ C) @ A)).max(axis=-1)
    if (rho >= 1.0).any():
        raise ValueError("kalman_gain: the error dynamics (I - L C) A are not stable (spectral radius %.6g): the pair (A, C) is not detectable" % float(np.max(rho)))
    info = dict(P=P, A=A, C=C, Q=Q, iterations=it)
    if not with_bias:
        return (K, info) if return_info else K
    Lx, Ld = K[..., :nx, :], G @ K[..., nx:, :]
    return (Lx, Ld, info) if return_info else (Lx, Ld)
