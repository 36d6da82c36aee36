"""The dropout masks of the training route restated in numpy from the contract in include/beat_this_amd.h (the section on
bt_train_dropout): Philox4x32-10 over (group, site, stream) counters under the seed as key, keep iff word >= floor(p 2^32).
Used by tests/test_dropout_rng.py (against bt_dropout_mask_host) and tests/test_gpu_dropout.py (the fp64 truth's masks)."""
import numpy as np

ATTN_P, ATTN_OUT, FF_HIDDEN, FF_OUT = range(4)
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays of one shape (or scalars), key: two Python ints -> four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """floor(p 2^32) in double, p as the fp32 value the library receives"""
    return int(np.floor(float(np.float32(p)) * 4294967296.0))


def _words(groups, site, seed, stream):
    """uint32 [..., 4]: the four words of every group"""
    g = np.asarray(groups, dtype=np.uint64)
    ctr = [g & MASK32, np.uint64(site << 24) | (g >> S32), np.uint64(stream & 0xFFFFFFFF), np.uint64((stream >> 32) & 0xFFFFFFFF)]
    ctr = [np.broadcast_to(v, g.shape) for v in ctr]
    return np.stack(philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)), axis=-1)


def mask(p, seed, stream, site, B, T, dim, hidden=0):
    """uint8, 1 = kept: [B, dim / 32, T, T] (query by key) for ATTN_P, [B T, dim or hidden] for the row sites"""
    thr = threshold(p)
    if site == ATTN_P:
        H, G = dim // 32, (T + 3) // 4
        rows = np.arange(B * H * T, dtype=np.uint64)                      # (b H + h) T + q
        groups = rows[:, None] * np.uint64(G) + np.arange(G, dtype=np.uint64)[None, :]
        w = _words(groups, site, seed, stream).reshape(B * H * T, 4 * G)[:, :T]   # word k mod 4 of group k / 4
        return (w >= thr).astype(np.uint8).reshape(B, H, T, T)
    n = hidden if site == FF_HIDDEN else dim
    groups = np.arange(B * T * n // 4, dtype=np.uint64)                   # row (n / 4) + col / 4
    return (_words(groups, site, seed, stream).reshape(B * T, n) >= thr).astype(np.uint8)
