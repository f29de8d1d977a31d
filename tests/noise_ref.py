"""The noise of the tick (copra_batch_set_noise, include/copra_hip.h) restated in numpy: Philox4x32-10 vectorised on uint64, then the
Box-Muller transform with the C library's log, cos and sin.  The 32-bit words are exact; the normals of a correct implementation differ from
these only through log, sin and cos (about 2 ulp each, |rad| <= 8.5): below 1e-14 for sigma = 1, the tests allow 1e-13 sigma."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)
S32 = np.uint64(32)
TOL = 1e-13  # absolute, times sigma


def philox(counter, key):
    """Philox4x32-10: counter (..., 4), key (..., 2), integers below 2^32 -> (..., 4) uint64 words below 2^32"""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1)


def words(seed, gi, s, j, t):
    """the generator's words for pair j of stream s of global instance gi at noise tick t (all broadcastable integers; seed, t below 2^64)"""
    seed, gi, s, j, t = np.broadcast_arrays(*(np.asarray(a, dtype=np.uint64) for a in (seed, gi, s, j, t)))
    counter = np.stack([gi & MASK, (s << np.uint64(16)) | j, t & MASK, t >> S32], axis=-1)
    return philox(counter, np.stack([seed & MASK, seed >> S32], axis=-1))


def normals(seed, first_instance, batch, rows, t, s):
    """n [batch][rows] of stream s (0: process, 1: sensor) at noise tick t"""
    pairs = (rows + 1) // 2
    gi = np.uint64(first_instance) + np.arange(batch, dtype=np.uint64)
    o = words(np.uint64(seed), gi[:, None], np.uint64(s), np.arange(pairs, dtype=np.uint64)[None, :], np.uint64(t))
    u1 = (((o[..., 0] << S32 | o[..., 1]) >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52
    u2 = (((o[..., 2] << S32 | o[..., 3]) >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    n = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1).reshape(batch, 2 * pairs)
    return np.ascontiguousarray(n[:, :rows])


def terms(seed, first_instance, batch, sigma, t, s):
    """sigma n: sigma (rows,) or (batch, rows)"""
    sigma = np.asarray(sigma, dtype=np.float64)
    return sigma * normals(seed, first_instance, batch, sigma.shape[-1], t, s)
