"""An independent numpy (fp64) restatement of the reference's losses (beat_this/model/loss.py) and their gradients, written
with explicit windows: no max-pooling library call, no autograd.  Rows are the last axis.

The rules it restates: the logits' window of frame t is [t - tol, t + tol] and its maximum is the FIRST index holding it
(the pooling only moves on a strictly greater value), except that a NaN takes the window (the last NaN, as torch's CPU
max_pool1d); the targets' window is [t - 2 tol, t + 2 tol]; the output frames are [2 tol, T - 2 tol); the BCE is torch's
with pos_weight; the mean is over all output frames, whatever the weights."""
import numpy as np


def window_argmax(x, lo, hi):
    """first index of the maximum of x[lo .. hi] (inclusive); a NaN wins (the last one)"""
    best, arg = x[lo], lo
    for i in range(lo + 1, hi + 1):
        if x[i] > best or np.isnan(x[i]):
            best, arg = x[i], i
    return arg


def bce(x, y, pw):
    """torch's binary_cross_entropy_with_logits element with pos_weight, and d/dx"""
    if np.isnan(x):
        return np.nan, np.nan
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(-abs(x))
        loss = (1 - y) * x + (1 + (pw - 1) * y) * (np.log1p(e) + max(-x, 0.0))
        sig = 1 / (1 + e) if x >= 0 else e / (1 + e)
        d = (pw * y + 1 - y) * sig - pw * y
    return loss, d


def row_terms(kind, tol, pw, x, y, m):
    """one row -> (sum of weighted terms, output frames, d(sum)/dx per frame)"""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    m = np.ones_like(y) if m is None else np.asarray(m, np.float64)
    T = x.size
    h = 0 if kind == "masked" else 2 * tol
    grad = np.zeros(T)
    total = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(h, T - h):
            if kind == "masked":
                l, d = bce(x[t], y[t], pw)
                total += l * m[t]
                grad[t] += d * m[t]
                continue
            a = window_argmax(x, t - tol, t + tol)
            S = np.max(y[t - 2 * tol:t + 2 * tol + 1])
            l, d = bce(x[a], y[t], pw)
            if kind == "shift_tolerant":
                w = (y[t] + (1 - S)) * m[t]
                total += l * w
                grad[a] += d * w
            else:
                l2, d2 = bce(x[a], S, pw)
                total += l * y[t] * m[t] + l2 * (1 - S) * m[t]
                grad[a] += d * y[t] * m[t] + d2 * (1 - S) * m[t]
    return total, T - 2 * h, grad


def loss(kind, tol, pw, x, y, m=None):
    """the loss over rows on the last axis -> (mean, d mean / dx of x's shape)"""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    shape = x.shape
    X, Y = x.reshape(-1, shape[-1] if x.ndim else 1), y.reshape(-1, shape[-1] if x.ndim else 1)
    M = None if m is None else np.broadcast_to(np.asarray(m, np.float64), shape).reshape(X.shape)
    total, count, grads = 0.0, 0, []
    for r in range(X.shape[0]):
        s, n, g = row_terms(kind, tol, pw, X[r], Y[r], None if M is None else M[r])
        total += s
        count += n
        grads.append(g)
    return total / count, (np.stack(grads) / count).reshape(shape)


def fuzz_rows(seed, n_rows, soft_frac=0.3, tol=3, max_len=700):
    """seeded rows (logits, targets, mask) of random lengths >= 1 + 4 tol: beat-like binary targets, some soft, with ties and
    masked stretches"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n_rows):
        T = int(rng.integers(1 + 4 * tol, max_len))
        x = rng.normal(0, 4, T).astype(np.float32)
        if i % 7 == 3:
            x = np.round(x / 3).astype(np.float32) * 3   # plateaus: ties inside windows
        y = np.zeros(T, np.float32)
        period = int(rng.integers(10, 40))
        y[int(rng.integers(0, period))::period] = 1
        if rng.random() < soft_frac:
            y = (y * 0.9 + 0.05).astype(np.float32)
        m = (rng.random(T) < 0.9).astype(np.float32) if i % 3 else np.ones(T, np.float32)
        rows.append((x, y, m))
    return rows
