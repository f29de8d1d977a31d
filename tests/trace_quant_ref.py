"""Trace quantiles (copra_batch_set_trace_quantiles, ABI 18) restated in numpy: the rule include/copra_hip.h writes down -- the key of a value's 64
bits, the stable sort of a row's finite values by it, the rank k = min(n - 1, max(0, ceil(p * n) - 1)) and the quiet NaN of an empty row.  An
order statistic is an element of the data, so everything that follows the rule gives these bytes; the rows' values come from
tests/trace_ref.py (values).  self_check() holds the rule against numpy's own quantile, method="inverted_cdf"."""
import math

import numpy as np

QUANT_MAX = 8
NAN_BITS = np.uint64(0x7FF8000000000000)


def keys(v):
    """the sort key of every value's bits b: b ^ (b >> 63 ? ~0 : 1 << 63)"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63) != 0, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(1) << np.uint64(63))


def rank(p, n):
    """the 0-based rank of level p among n > 0 values: one FP64 multiply, then ceil"""
    c = math.ceil(float(np.float64(p) * np.float64(n)))
    return min(n - 1, max(0, c - 1))


def row(v, levels):
    """the quantiles of one row as uint64 bits, (len(levels),)"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    fin = v[np.isfinite(v)]
    out = np.full(len(levels), NAN_BITS, dtype=np.uint64)
    if fin.size:
        order = fin[np.argsort(keys(fin), kind="stable")]
        for q, p in enumerate(levels):
            out[q] = order[rank(p, fin.size)].view(np.uint64)
    return out


def rows(vals, levels):
    """(rows, batch) values -> (rows, nq) float64 whose BYTES are the rule's (compare with tobytes(): a NaN is not equal to itself)"""
    return np.stack([row(v, levels) for v in vals]).view(np.float64).reshape(len(vals), len(levels))


def self_check(seed=0, cases=200):
    """the rule against np.quantile(..., method="inverted_cdf") on random rows, with +-0, denormals, +-1e308 and non-finite entries mixed in"""
    rng = np.random.default_rng(seed)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 1e308, -1e308, 2.2250738585072014e-308])
    levels = [0.0, 1.0, 0.5, 1.0 / 3.0, 1e-9, 0.999, 0.05, 0.95]
    for _ in range(cases):
        n = int(rng.integers(1, 400))
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)
        pick = rng.random(n) < 0.1
        v[pick] = rng.choice(special, int(pick.sum()))
        bad = rng.random(n) < 0.05
        w = v.copy()
        w[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf]), int(bad.sum()))
        got = row(w, levels).view(np.float64)
        fin = w[np.isfinite(w)]
        if fin.size == 0:
            assert (row(w, levels) == NAN_BITS).all()
            continue
        want = np.quantile(fin, levels, method="inverted_cdf")
        assert np.array_equal(got, want), (n, got, want)  # (numerically: numpy's sort does not order -0.0 and +0.0)
        assert got[0] == fin.min() and got[1] == fin.max()
    return True
