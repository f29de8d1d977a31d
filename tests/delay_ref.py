"""Input delay in the tick (copra_batch_set_input_delay, ABI 16) restated in numpy: the queue, its pop and push, the prediction with its three
cases per entry, the resets -- the rule include/copra_hip.h writes down, in natural indexing (A[b, r, j], B[b, r, c]).  Pure: numpy only,
used by tests/test_delay_abi.py (against the kernel's phase bodies on the host, bit for bit: every product and every sum is rounded, and the
row sum is formed in the order of plant_row) and by tests/test_delay_gpu.py (against the device, within the running bound below).

The queue is kept OLDEST FIRST, q[b, j], j = 0 the command the next tick applies; the library's ring holds entry j in slot (head + j) % D
(to_ring / from_ring).  The command of a failed solve is NaN: it is never applied and never read.

The running rounding bound of a prediction.  One step forms, per row, a sum of k = nx + nu + 1 terms (d_r, the nx products of A, the nu
products of B; k + 1 = nx + nu + 2 covers the products' own roundings): by Higham, Accuracy and Stability, 3.1 and 3.4, in any order of
summation and with or without fused multiply-add the computed row differs from the exact one of the same inputs by at most
gamma (|A||x| + |B||u| + |d|), gamma = k u / (1 - k u) with k = nx + nu + 2 and u = 2^-53.  An error err_j of the input state is carried on
by |A| err_j:   err_0 = 0,   err_{j+1} = |A| err_j + gamma (|A||x_j| + |B||u_j| + |d|);   an entry that holds the state keeps err."""
import numpy as np

OK = 0
FALLBACK, HELD = -1, -2  # COPRA_PLAN_FALLBACK, COPRA_PLAN_HELD
U = 2.0 ** -53


def gamma(nx, nu):
    k = nx + nu + 2
    return k * U / (1.0 - k * U)


def model_of(A, B, d, batch):
    """(A [b, nx, nx], B [b, nx, nu], d [b, nx]) of a model given per instance or once for the batch"""
    A, B, d = (np.asarray(m, dtype=np.float64) for m in (A, B, d))
    if A.ndim == 2:
        A, B, d = (np.broadcast_to(m, (batch,) + m.shape) for m in (A, B, d))
    return A, B, d


def row_sums(A, B, d, x, u, w=None):
    """A x + B u + d (+ w) for every instance, each row in the order of plant_row: d_r, then the columns of A ascending, then those of B,
    then w_r; every product and every sum rounded"""
    acc = np.array(d, dtype=np.float64, copy=True)
    for j in range(A.shape[-1]):
        acc = acc + A[:, :, j] * x[:, j:j + 1]
    for c in range(B.shape[-1]):
        acc = acc + B[:, :, c] * u[:, c:c + 1]
    if w is not None:
        acc = acc + w
    return acc


def plant_step(plant, x, control, status, fallback_u=None, w=None):
    """one plant step of the tick (K = 0): (x+, u_out, age).  control [b, nu] (a failed instance's is not looked at), status [b]"""
    A, B, d = model_of(*plant, batch=x.shape[0])
    ok = np.asarray(status) == OK
    u = np.where(ok[:, None], np.where(ok[:, None], control, 0.0), np.nan if fallback_u is None else fallback_u)
    moved = ok | (fallback_u is not None)
    xn = row_sums(A, B, d, x, np.where(moved[:, None], u, 0.0), w)
    xn = np.where(moved[:, None], xn, x)
    age = np.where(ok, 0, FALLBACK if fallback_u is not None else HELD).astype(np.int32)
    return xn, u, age


def predict(model, xnow, q, qs, fallback_u=None):
    """(x0, err): the prediction from xnow over the D pending entries q [b, D, nu], qs [b, D], oldest first, with `model` and no w, and its
    running rounding bound"""
    b, nx = xnow.shape
    A, B, d = model_of(*model, batch=b)
    g = gamma(nx, q.shape[-1])
    x, err = np.array(xnow, dtype=np.float64, copy=True), np.zeros((b, nx))
    aA, aB, ad = np.abs(A), np.abs(B), np.abs(d)
    for j in range(q.shape[1]):
        ok = qs[:, j] == OK
        moved = ok | (fallback_u is not None)
        u = np.where(ok[:, None], np.where(ok[:, None], q[:, j], 0.0), 0.0 if fallback_u is None else fallback_u)
        xn = row_sums(A, B, d, x, u)
        en = np.einsum("brj,bj->br", aA, err) + g * (np.einsum("brj,bj->br", aA, np.abs(x)) + np.einsum("brc,bc->br", aB, np.abs(u)) + ad)
        x = np.where(moved[:, None], xn, x)
        err = np.where(moved[:, None], en, err)
    return x, err


def predict_exact(model, xnow, q, qs, fallback_u=None):
    """(x0, err) as predict(), every step in numpy.longdouble: the value a float64 computation of whatever order is held to, within err"""
    LD = np.longdouble
    b, nx = xnow.shape
    A, B, d = (np.asarray(m, dtype=LD) for m in model_of(*model, batch=b))
    g = gamma(nx, q.shape[-1])
    x, err = np.asarray(xnow, dtype=LD).copy(), np.zeros((b, nx), dtype=LD)
    aA, aB, ad = np.abs(A), np.abs(B), np.abs(d)
    mv = lambda M, v: (M * v[:, None, :]).sum(axis=2)  # noqa: E731
    for j in range(q.shape[1]):
        ok = qs[:, j] == OK
        moved = ok | (fallback_u is not None)
        u = np.where(ok[:, None], np.where(ok[:, None], q[:, j], 0.0), 0.0 if fallback_u is None else fallback_u).astype(LD)
        xn = mv(A, x) + mv(B, u) + d
        en = mv(aA, err) + g * (mv(aA, np.abs(x)) + mv(aB, np.abs(u)) + ad)
        x = np.where(moved[:, None], xn, x)
        err = np.where(moved[:, None], en, err)
    return x, err.astype(np.float64)


def to_ring(q, qs, head):
    """(ring [b, D, nu], ring statuses [D, b]) of a queue kept oldest first: entry j sits in slot (head + j) % D"""
    D = q.shape[1]
    ring, rs = np.empty_like(q), np.empty((D, q.shape[0]), dtype=np.int32)
    for j in range(D):
        ring[:, (head + j) % D] = q[:, j]
        rs[(head + j) % D] = qs[:, j]
    return np.ascontiguousarray(ring), rs


def from_ring(ring, rs, head):
    D = ring.shape[1]
    q, qs = np.empty_like(ring), np.empty((ring.shape[0], D), dtype=np.int32)
    for j in range(D):
        q[:, j] = ring[:, (head + j) % D]
        qs[:, j] = rs[(head + j) % D]
    return q, qs


class DelayLoop:
    """The state the library keeps and its tick.  D = 0 is delay off: tick() is the plant step on x0 itself."""

    def __init__(self, D, x0, nu, u_init=None):
        self.nu = nu
        self.xnow = np.array(x0, dtype=np.float64, copy=True)
        self.x0 = self.xnow.copy()  # what the next solve reads
        self.err = np.zeros_like(self.xnow)  # the running bound of x0
        self.reset(D, u_init)

    def reset(self, D, u_init=None):
        """the setter: every slot holds u_init with status OK; xnow stays"""
        b = self.xnow.shape[0]
        self.D = D
        u0 = np.zeros((b, self.nu)) if u_init is None else np.asarray(u_init, dtype=np.float64)
        self.q = np.repeat(u0[:, None, :], D, axis=1)
        self.qs = np.zeros((b, D), dtype=np.int32)
        self.head = 0

    def repredict(self, model, fallback_u=None):
        """set_x0 / set_bias / set_system: the queue is kept, the prediction formed again"""
        if self.D == 0:
            self.x0, self.err = self.xnow.copy(), np.zeros_like(self.xnow)
        else:
            self.x0, self.err = predict(model, self.xnow, self.q, self.qs, fallback_u)
        return self.x0

    def set_state(self, x, model):
        self.xnow = np.array(x, dtype=np.float64, copy=True)
        return self.repredict(model)

    def push(self, control, status):
        """the oldest entry leaves, the last solve's command becomes the newest (NaN where its solve failed: never loaded)"""
        ok = np.asarray(status) == OK
        new = np.where(ok[:, None], np.where(ok[:, None], control, 0.0), np.nan)
        self.q = np.concatenate([self.q[:, 1:], new[:, None, :]], axis=1)
        self.qs = np.concatenate([self.qs[:, 1:], np.asarray(status, dtype=np.int32)[:, None]], axis=1)
        self.head = (self.head + 1) % self.D

    def tick(self, plant, model, control, status, fallback_u=None, w=None):
        """one copra_batch_advance: (x_out, u_out, status_out, age_out) of the command that reached the plant; afterwards xnow, the queue and
        x0 (the prediction) are those of the next tick"""
        control = np.asarray(control, dtype=np.float64)[:, :self.nu]
        status = np.asarray(status, dtype=np.int32)
        if self.D == 0:
            xn, u, age = plant_step(plant, self.xnow, control, status, fallback_u, w)
            self.xnow, self.x0, self.err = xn, xn.copy(), np.zeros_like(xn)
            return xn, u, status.copy(), age
        s_app = self.qs[:, 0].copy()
        xn, u, age = plant_step(plant, self.xnow, self.q[:, 0], s_app, fallback_u, w)
        self.xnow = xn
        self.push(control, status)
        self.x0, self.err = predict(model, self.xnow, self.q, self.qs, fallback_u)
        return xn, u, s_app, age
