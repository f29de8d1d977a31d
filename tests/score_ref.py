"""Closed-loop scores (copra_batch_set_score, ABI 14) restated in numpy: the rule of one tick's update of the records and the merge rule and
order of the summary, in the orders include/copra_hip.h writes down.  Every product and every sum is rounded once, rows in ascending order,
sums from 0.0 -- the emulator (tests/emu/emu_score.cpp, -ffp-contract=off) gives these bits."""
import numpy as np

HELD, FALLBACK = -2, -1
RECORD = np.dtype([("jx", "f8"), ("ju", "f8"), ("viol_sum", "f8"), ("viol_max", "f8"), ("peak", "f8"), ("ticks", "i4"), ("held", "i4"),
                   ("replayed", "i4"), ("fallback", "i4"), ("violating", "i4"), ("first_violation", "i4")])
FIELDS = ("jx", "ju", "viol_sum", "viol_max", "peak")
COUNTERS = ("ticks", "held", "replayed", "fallback", "violating")
CHUNK, THREADS = 1024, 256
assert RECORD.itemsize == 64


def zero_records(batch):
    return np.zeros(batch, dtype=RECORD)


def _pick(a, b, per):
    return None if a is None else (a[b] if per else a)


def _viol(z, lo, hi):
    v = 0.0
    if lo is not None and lo - z > v:
        v = lo - z
    if hi is not None and z - hi > v:
        v = z - hi
    return v


def _quad(w, e, dense):
    """the terms of e' W e, one per row"""
    n = e.shape[0]
    out = np.zeros(n)
    for r in range(n):
        if dense:  # W in natural indexing: W[r, j]
            acc = 0.0
            for j in range(n):
                acc = acc + w[r, j] * e[j]
            out[r] = e[r] * acc
        else:
            out[r] = (w[r] * e[r]) * e[r]
    return out


def update(rec, x, u, age, tau, qx=None, ru=None, x_ref=None, x_lo=None, x_hi=None, u_lo=None, u_hi=None, tol=0.0, dense=False, per_instance=False):
    """one tick: rec (RECORD array) updated in place.  x (batch, nx) the true state after the tick, u (batch, nu), age (batch,), tau the schedule
    tick after the tick.  Weights in natural indexing ((nx,) | (nx, nx), with a leading batch axis when per_instance); x_ref ([batch,] steps, nx)."""
    with np.errstate(invalid="ignore", over="ignore"):
        batch, nx = x.shape
        nu = u.shape[1]
        for b in range(batch):
            ref = None
            if x_ref is not None:
                sig = x_ref[b] if per_instance else x_ref
                ref = sig[min(tau, sig.shape[0] - 1)]
            e = x[b] - ref if ref is not None else x[b].copy()
            held = age[b] == HELD
            cx = _quad(_pick(qx, b, per_instance), e, dense) if qx is not None else np.zeros(nx)
            cu = _quad(_pick(ru, b, per_instance), u[b], dense) if (ru is not None and not held) else np.zeros(nu)
            lo, hi = _pick(x_lo, b, per_instance), _pick(x_hi, b, per_instance)
            v = [_viol(x[b, r], None if lo is None else lo[r], None if hi is None else hi[r]) for r in range(nx)]
            if not held:
                lo, hi = _pick(u_lo, b, per_instance), _pick(u_hi, b, per_instance)
                v += [_viol(u[b, c], None if lo is None else lo[c], None if hi is None else hi[c]) for c in range(nu)]
            lx = lu = vs = vmax = 0.0
            for t in cx:
                lx = lx + t
            for t in cu:
                lu = lu + t
            for t in v:
                vs = vs + t
                if t > vmax:
                    vmax = t
            R = rec[b]
            lsum = lx + lu
            R["jx"] += lx
            if not held:
                R["ju"] += lu
            R["viol_sum"] += vs
            if vmax > R["viol_max"]:
                R["viol_max"] = vmax
            if lsum > R["peak"]:
                R["peak"] = lsum
            R["ticks"] += 1
            R["held"] += int(held)
            R["replayed"] += int(age[b] >= 1)
            R["fallback"] += int(age[b] == FALLBACK)
            if vmax > tol:
                R["violating"] += 1
                if R["first_violation"] == 0:
                    R["first_violation"] = R["ticks"]
    return rec


def abs_terms(x, u, age, tau, qx=None, ru=None, x_ref=None, dense=False, per_instance=False):
    """per instance: the sum of the absolute values of every product behind lx and lu (what the forward error bound multiplies)"""
    batch, nx = x.shape
    ax, au = np.zeros(batch), np.zeros(batch)
    with np.errstate(invalid="ignore"):
        for b in range(batch):
            ref = 0.0
            if x_ref is not None:
                sig = x_ref[b] if per_instance else x_ref
                ref = sig[min(tau, sig.shape[0] - 1)]
            e = np.abs(x[b] - ref)
            if qx is not None:
                w = np.abs(_pick(qx, b, per_instance))
                ax[b] = e @ w @ e if dense else (w * e * e).sum()
            if ru is not None and age[b] != HELD:
                w, a = np.abs(_pick(ru, b, per_instance)), np.abs(u[b])
                au[b] = a @ w @ a if dense else (w * a * a).sum()
    return ax, au


# ---- the summary ----
def stat_empty():
    return dict(n=0, mean=0.0, m2=0.0, min=np.inf, max=-np.inf, argmin=-1, argmax=-1)


def stat_one(v, index):
    if not np.isfinite(v):
        return stat_empty()
    v = float(v)
    return dict(n=1, mean=v, m2=0.0, min=v, max=v, argmin=int(index), argmax=int(index))


def stat_merge(a, b):
    """the pairwise update: a, then b"""
    if b["n"] == 0:
        return dict(a)
    if a["n"] == 0:
        return dict(b)
    na, nb, n = np.float64(a["n"]), np.float64(b["n"]), np.float64(a["n"] + b["n"])
    delta = np.float64(b["mean"]) - np.float64(a["mean"])
    with np.errstate(over="ignore", invalid="ignore"):
        mean = np.float64(a["mean"]) + delta * nb / n
        m2 = np.float64(a["m2"]) + np.float64(b["m2"]) + delta * delta * na * nb / n
    bmin = b["min"] < a["min"] or (b["min"] == a["min"] and b["argmin"] < a["argmin"])
    bmax = b["max"] > a["max"] or (b["max"] == a["max"] and b["argmax"] < a["argmax"])
    return dict(n=a["n"] + b["n"], mean=float(mean), m2=float(m2), min=b["min"] if bmin else a["min"], max=b["max"] if bmax else a["max"],
                argmin=b["argmin"] if bmin else a["argmin"], argmax=b["argmax"] if bmax else a["argmax"])


TOTALS = COUNTERS + ("instances_violating", "instances_held")


def summary_empty():
    s = {f: stat_empty() for f in FIELDS}
    s.update({k: 0 for k in TOTALS})
    return s


def summary_of(r, index):
    s = {f: stat_one(r[f], index) for f in FIELDS}
    s.update({k: int(r[k]) for k in COUNTERS})
    s["instances_violating"], s["instances_held"] = int(r["violating"] != 0), int(r["held"] != 0)
    return s


def summary_merge(a, b):
    s = {f: stat_merge(a[f], b[f]) for f in FIELDS}
    s.update({k: a[k] + b[k] for k in TOTALS})
    return s


def _workgroup(items):
    """THREADS threads: thread t folds items t, t + THREADS, ... from the empty summary; the lane tree of every wave; the fold of the waves"""
    lane = []
    for t in range(THREADS):
        acc = summary_empty()
        for it in items[t::THREADS]:
            acc = summary_merge(acc, it)
        lane.append(acc)
    for w in range(THREADS // 64):
        off = 32
        while off >= 1:
            for l in range(64 - off):
                lane[64 * w + l] = summary_merge(lane[64 * w + l], lane[64 * w + l + off])
            off //= 2
    acc = lane[0]
    for w in range(1, THREADS // 64):
        acc = summary_merge(acc, lane[64 * w])
    return acc


def summary(rec):
    """the summary of the records in the written order: chunks of CHUNK records, then one workgroup over the partials"""
    if len(rec) == 0:
        return summary_empty()
    parts = []
    for c in range(0, len(rec), CHUNK):
        parts.append(_workgroup([summary_of(rec[i], i) for i in range(c, min(c + CHUNK, len(rec)))]))
    return _workgroup(parts)


def exact_stats(values):
    """n, mean and m2 of the finite values in numpy's longdouble, and the sum of squares (for the bound)"""
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)].astype(np.longdouble)
    if v.size == 0:
        return 0, np.longdouble(0), np.longdouble(0)
    mean = v.sum() / v.size
    return int(v.size), mean, ((v - mean) ** 2).sum()
