"""Ensemble traces (copra_batch_set_trace, ABI 17) restated in numpy: the layout of a slot, the head counts, the vmax rule and the reduction of every
row in the order include/copra_hip.h writes down -- the summary's, with "record i" read as "instance i's value of row r".  The merge rule, the
chunk and the thread count are score_ref's; the emulator (tests/emu/emu_trace.cpp, -ffp-contract=off) gives these bits."""
import numpy as np

import score_ref
from score_ref import CHUNK, FALLBACK, HELD, THREADS, stat_empty, stat_merge, stat_one

X, U, ERR = 1, 2, 4
HEAD = np.dtype([(n, "i8") for n in ("tick", "tau", "solved", "replayed", "fallback", "held", "violating", "reserved")])
STAT = np.dtype([("n", "i8"), ("mean", "f8"), ("m2", "f8"), ("min", "f8"), ("max", "f8"), ("argmin", "i8"), ("argmax", "i8")])
COUNTS = ("solved", "replayed", "fallback", "held", "violating")
assert HEAD.itemsize == 64 and STAT.itemsize == 56


def rows_of(what, nx, nu, limits):
    return (nx if what & X else 0) + (nu if what & U else 0) + (nx if what & ERR else 0) + (1 if limits else 0)


def slot_dtype(rows):
    return np.dtype([("head", HEAD), ("stat", STAT, (rows,))])


def vmax(x, u, age, x_lo=None, x_hi=None, u_lo=None, u_hi=None):
    """per instance: the largest of max(0, lo_r - z_r, z_r - hi_r) over the rows of x, then of u (held: no u rows); `>` from 0.0"""
    out = np.zeros(x.shape[0])
    for b in range(x.shape[0]):
        v = 0.0
        if x_lo is not None or x_hi is not None:
            for r in range(x.shape[1]):
                t = score_ref._viol(x[b, r], None if x_lo is None else x_lo[r], None if x_hi is None else x_hi[r])
                if t > v:
                    v = t
        if (u_lo is not None or u_hi is not None) and age[b] != HELD:
            for c in range(u.shape[1]):
                t = score_ref._viol(u[b, c], None if u_lo is None else u_lo[c], None if u_hi is None else u_hi[c])
                if t > v:
                    v = t
        out[b] = v
    return out


def values(what, x, u, age, est=None, x_lo=None, x_hi=None, u_lo=None, u_hi=None):
    """(rows, batch): every instance's value of every row of the slot, NaN where it has none"""
    batch, nx = x.shape
    out = []
    if what & X:
        out += [x[:, r] for r in range(nx)]
    if what & U:
        held = age == HELD
        out += [np.where(held, np.nan, u[:, c]) for c in range(u.shape[1])]
    if what & ERR:
        out += [(est[:, r] - x[:, r]) if est is not None else np.full(batch, np.nan) for r in range(nx)]
    if any(a is not None for a in (x_lo, x_hi, u_lo, u_hi)):
        out.append(vmax(x, u, age, x_lo, x_hi, u_lo, u_hi))
    return np.asarray(out, dtype=np.float64).reshape(len(out), batch)


def _workgroup(items, empty, merge):
    """THREADS threads: thread t folds items t, t + THREADS, ... from the empty one; the lane tree of every wave; the fold of the waves"""
    lane = []
    for t in range(THREADS):
        acc = empty()
        for it in items[t::THREADS]:
            acc = merge(acc, it)
        lane.append(acc)
    for w in range(THREADS // 64):
        off = 32
        while off >= 1:
            for l in range(64 - off):
                lane[64 * w + l] = merge(lane[64 * w + l], lane[64 * w + l + off])
            off //= 2
    acc = lane[0]
    for w in range(1, THREADS // 64):
        acc = merge(acc, lane[64 * w])
    return acc


def reduce_parts(parts, empty=stat_empty, merge=stat_merge):
    """stage 2: one workgroup over the partials"""
    return _workgroup(list(parts), empty, merge)


def reduce_row(v):
    """one row over the batch: chunks of CHUNK instances, then one workgroup over the partials"""
    parts = [_workgroup([stat_one(v[i], i) for i in range(c, min(c + CHUNK, len(v)))], stat_empty, stat_merge) for c in range(0, len(v), CHUNK)]
    return reduce_parts(parts)


def counts(age, vm=None, tol=0.0):
    age = np.asarray(age)
    return dict(solved=int((age == 0).sum()), replayed=int((age >= 1).sum()), fallback=int((age == FALLBACK).sum()), held=int((age == HELD).sum()),
                violating=0 if vm is None else int((vm > tol).sum()))


def slot(tick, tau, what, x, u, age, est=None, x_lo=None, x_hi=None, u_lo=None, u_hi=None, tol=0.0):
    """the slot of one recorded tick, a 0-d structured array of slot_dtype(rows)"""
    limits = any(a is not None for a in (x_lo, x_hi, u_lo, u_hi))
    with np.errstate(invalid="ignore", over="ignore"):
        vals = values(what, x, u, age, est, x_lo, x_hi, u_lo, u_hi)
    out = np.zeros((), dtype=slot_dtype(vals.shape[0]))
    c = counts(age, vals[-1] if limits else None, tol)
    out["head"]["tick"], out["head"]["tau"] = tick, tau
    for k in COUNTS:
        out["head"][k] = c[k]
    for r in range(vals.shape[0]):
        s = reduce_row(vals[r])
        for f in STAT.names:
            out["stat"][r][f] = s[f]
    return out


def check_stat(st, v, bounds, what=""):
    """one statistic against the values it was reduced from: n, min, max and the args exact (numpy's arg: the first, the lowest index), mean
    and m2 within bounds(finite values) = (E, B) of numpy's longdouble; returns the largest error / bound"""
    v = np.asarray(v, dtype=np.float64)
    fin = np.isfinite(v)
    assert int(st["n"]) == int(fin.sum()), (what, st, int(fin.sum()))
    if not fin.any():
        assert (float(st["mean"]), float(st["m2"]), float(st["min"]), float(st["max"]), int(st["argmin"]), int(st["argmax"])) == (0.0, 0.0, np.inf, -np.inf, -1, -1), (what, st)
        return 0.0
    idx = np.nonzero(fin)[0]
    assert float(st["min"]) == v[idx].min() and float(st["max"]) == v[idx].max(), (what, st)
    assert int(st["argmin"]) == idx[np.argmin(v[idx])] and int(st["argmax"]) == idx[np.argmax(v[idx])], (what, st)
    _, mean, m2 = score_ref.exact_stats(v)
    E, B = bounds(v)
    e1, e2 = abs(float(np.longdouble(st["mean"]) - mean)), abs(float(np.longdouble(st["m2"]) - m2))
    assert e1 <= E and e2 <= B, (what, e1, E, e2, B)
    return max(e1 / E if E else 0.0, e2 / B if B else 0.0)


def recorded_ticks(ticks, every, capacity):
    """(the ticks t < ticks that a trace records, the number it misses)"""
    every = every or 1
    want = [t for t in range(ticks) if t % every == 0]
    return want[:capacity], max(0, len(want) - capacity)
