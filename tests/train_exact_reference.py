""""Selection attention": inputs on which the three attention sweeps of the training route (csrc/train.hip, csrc/train_mixed.inc)
have to be right bit for bit, on the fp32 route and on the 16-mixed one, with and without dropout.

Softmax is exact when every probability is a power of two or zero.  Per (sequence, head) the T tokens are partitioned into key
classes of 1, 2 or 4 tokens; every class has a code, a pair of the 32 dimensions of its own; a key is 32 on its class's two
dimensions, a query 64 on the two dimensions of the class it selects, both 0 elsewhere.  A score is then 4096 (the selected
class), 2048 (one shared dimension) or 0: powers of two, so score * QK_SCALE_LOG2E is exact in fp32 (it has to be: the kernels
are compiled with multiply-add contraction, and fma(s, c, -lse) equals the rounded form only when s c is exact).  Neighbouring
levels are 522 apart in log2 units, so everything but the selected class has probability exp2(-522) = 0 and a running maximum's
rescale is 0 as well: P = 1 / n over the n keys of the class and exactly zero elsewhere, l = n, lse = 4096 c + log2 n.  With v
integers in [-2, 2], dO integers in [-1, 1] and a p = 0.5 mask (1 / (1 - p) = 2) every value downstream is a dyadic rational with
few bits: O, delta, dP, dS = P (dP - delta), dV = (P m c)^T dO, and dQ = dS K, dK = dS^T Q before their one multiplication by
QK_SCALE, which the expectation does in numpy's float32.

Here: the generator, the fp64 expectation, two numpy emulations of the device's orders of operation (sequential keys with a
per-key running maximum in fp32; tiles of 32 with P and dS rounded to fp16, in both directions) that have to reproduce the
expectation bit for bit -- which is what makes a device mismatch mean a kernel error rather than a property of the inputs --
and three mutants of the tiled emulation that have to miss it.  tests/test_train_exact_reference.py runs all of it without a
GPU; tests/test_gpu_train_exact.py hands the same cases to bt_train_attention.
"""
import ctypes as C

import numpy as np

QK_SCALE = np.float32(0.17677669529663687)
QK_SCALE_LOG2E = np.float32(0.2550348616841918)
CASES = ((1, 1, 64), (1, 31, 64), (1, 32, 64), (1, 33, 64), (1, 63, 64), (1, 64, 64), (3, 65, 64), (2, 97, 192), (1, 130, 64),
         (2, 200, 192))   # (B, T, dim)
DROP_P = 0.5
# (seed, stream) of the dropout variants; one stream beyond 32 bits
DROPS = ((0x5EED_0000_0000_0017, 3), (11, 0x1_0000_0007), (0xFFFF_FFFF_FFFF_FFF1, 0xABCD_EF01_2345))
MUTANTS = ("swap_two_keys_of_a_tile", "mask_word_of_the_next_key", "drop_the_last_key")
PAIRS = np.array([(i, j) for i in range(32) for j in range(i + 1, 32)])   # the 496 codes
f32, f64, f16 = np.float32, np.float64, np.float16


def host_mask(seed, stream, B, T, dim):
    """bt_dropout_mask_host(BT_DROP_ATTN_P) at p = 0.5: uint8 [B, H, T, T], query by key, 1 = kept"""
    from beat_this_amd import _lib as L

    out = np.zeros((B, dim // 32, T, T), dtype=np.uint8)
    d = L.TrainDropout(p=DROP_P, seed=seed, stream=stream)
    L.check(L.lib().bt_dropout_mask_host(C.byref(d), L.DROP_ATTN_P, B, T, dim, 0, out.ctypes.data))
    return out


def exact32(x, what):
    """x (float64) as float32, asserting that nothing is lost"""
    y = x.astype(f32)
    assert np.array_equal(y.astype(f64), x), f"{what} is not exact in fp32"
    return y


class Case:
    """One (B, T, dim) case: inputs q, k, v, dO [B, H, T, 32] (fp64 holding small integers), kc / qc [B, H, T] the key class
    of a token and the class its query selects, size [B, H, T] = n of the selected class, mask [B, H, T, T] or None, and the
    expectation: O, dq, dk, dv [B, H, T, 32], lse, delta [B, H, T] as float32."""

    def __init__(self, B, T, dim, seed, mask=None):
        self.B, self.T, self.dim, self.H, self.seed, self.mask = B, T, dim, dim // 32, seed, mask
        self.c = 2.0 if mask is not None else 1.0
        for attempt in range(50):
            self.draw(np.random.default_rng([seed, attempt]))
            if self.expect():
                self.attempt = attempt
                return
        raise AssertionError(f"no draw of case {(B, T, dim, seed)} met the fp16 preconditions")

    def draw(self, rng):
        B, H, T = self.B, self.H, self.T
        self.kc, self.qc = np.zeros((B, H, T), dtype=np.int64), np.zeros((B, H, T), dtype=np.int64)
        self.q, self.k = np.zeros((B, H, T, 32)), np.zeros((B, H, T, 32))
        for b in range(B):
            for h in range(H):
                sizes, left = [], T
                while left:
                    s = min(int(rng.choice((1, 2, 4))), left)
                    sizes.append(2 if s == 3 else s)                     # (a truncated last class of 3 becomes 2 + 1)
                    left -= sizes[-1]
                n_cls = len(sizes)
                self.kc[b, h, rng.permutation(T)] = np.repeat(np.arange(n_cls), sizes)
                # every class is selected by at least one query (so that every key has a gradient), the others at random; a
                # token's query class is drawn without looking at its key class
                self.qc[b, h] = rng.permutation(np.concatenate([np.arange(n_cls), rng.integers(0, n_cls, T - n_cls)]))
                code = PAIRS[rng.permutation(len(PAIRS))[:n_cls]]   # afresh per head and per sequence
                for t in range(T):
                    self.k[b, h, t, code[self.kc[b, h, t]]] = 32.0
                    self.q[b, h, t, code[self.qc[b, h, t]]] = 64.0
        self.v = rng.integers(-2, 3, size=(B, H, T, 32)).astype(f64)
        self.dO = rng.integers(-1, 2, size=(B, H, T, 32)).astype(f64)
        if T > 1:   # distinct per row: a value taken from another row shows
            for x in (self.v, self.dO):
                assert len(np.unique(x.reshape(-1, 32), axis=0)) == B * H * T

    def expect(self):
        """the fp64 expectation; False when a redraw is needed (dS or the masked, scaled P not exact in fp16)"""
        sel = self.kc[:, :, None, :] == self.qc[:, :, :, None]            # [B, H, q, k]
        self.size = sel.sum(-1)
        assert np.isin(self.size, (1, 2, 4)).all()
        s = self.q @ self.k.transpose(0, 1, 3, 2)
        assert np.isin(s, (0.0, 2048.0, 4096.0)).all() and np.array_equal(s == 4096.0, sel)
        P = sel / self.size[..., None]
        mc = self.c * (self.mask.astype(f64) if self.mask is not None else 1.0)
        Pm = P * mc
        O = Pm @ self.v
        top = f64(f32(4096.0) * QK_SCALE_LOG2E)
        assert top == 4096.0 * f64(QK_SCALE_LOG2E)                        # the scaled score is exact in fp32
        lse = top + np.log2(self.size)
        delta = (self.dO * O).sum(-1)
        dP = (self.dO @ self.v.transpose(0, 1, 3, 2)) * mc
        dS = P * (dP - delta[..., None])
        if not (np.array_equal(dS.astype(f16).astype(f64), dS) and np.array_equal(Pm.astype(f16).astype(f64), Pm)):
            return False
        self.P, self.Pm, self.dS = P, Pm, dS
        self.O, self.lse, self.delta = exact32(O, "O"), exact32(lse, "lse"), exact32(delta, "delta")
        self.dv = exact32(Pm.transpose(0, 1, 3, 2) @ self.dO, "dV")
        self.dq = exact32(dS @ self.k, "dS K") * QK_SCALE                  # (one rounding, in float32)
        self.dk = exact32(dS.transpose(0, 1, 3, 2) @ self.q, "dS^T Q") * QK_SCALE
        return True

    # ---- the device's layouts ----
    def rows(self, x):
        """[B, H, T, w] -> [B T, H w] (head h in columns w h)"""
        B, H, T, w = x.shape
        return np.ascontiguousarray(x.transpose(0, 2, 1, 3).reshape(B * T, H * w)).astype(f32)

    def qkv(self):
        return np.concatenate([self.rows(self.q), self.rows(self.k), self.rows(self.v)], axis=1)

    def dqkv(self):
        return np.concatenate([self.rows(self.dq), self.rows(self.dk), self.rows(self.dv)], axis=1)

    def per_row(self, x):
        """[B, H, T] -> [B T, H]"""
        return self.rows(x[..., None])

    def unrows(self, x, w=32):
        """[B T, H w] -> [B, H, T, w]"""
        return x.reshape(self.B, self.T, self.H, w).transpose(0, 2, 1, 3)

    def describe(self, name, got, want):
        """None, or the first differing (b, head, row, column) of a [B, H, T, w] tensor with the class structure around it"""
        g, w = (pos_zero(np.ascontiguousarray(x, dtype=f32)).view(np.uint32) for x in (got, want))
        bad = np.argwhere(g != w)
        if not len(bad):
            return None
        b, h, t, d = (int(i) for i in bad[0])
        kc, qc = self.kc[b, h], self.qc[b, h]
        return (f"{name}: {len(bad)} of {g.size} elements differ, the first at (b, head, row, column) = {(b, h, t, d)}: got "
                f"{got[b, h, t, d]!r}, want {want[b, h, t, d]!r}.  Token {t} has key class {kc[t]} (keys {np.flatnonzero(kc == kc[t]).tolist()}, "
                f"selected by queries {np.flatnonzero(qc == kc[t]).tolist()}) and selects class {qc[t]} (keys "
                f"{np.flatnonzero(kc == qc[t]).tolist()}); T = {self.T}, dropout {'on' if self.mask is not None else 'off'}"
                + (f", kept keys of query {t}: {np.flatnonzero(self.mask[b, h, t]).tolist()}" if self.mask is not None else ""))


def make_case(B, T, dim, drop=None):
    """drop: None or (seed, stream) of a p = 0.5 mask"""
    mask = None if drop is None else host_mask(drop[0], drop[1], B, T, dim)
    return Case(B, T, dim, 7000 + 10 * T + B, mask)


def fma_sub(s, c, ls):
    """fma(s, c, -ls) in fp32: the product and the difference are exact in fp64 here, one rounding at the end"""
    return (s.astype(f64) * f64(c) - ls.astype(f64)).astype(f32)


def dots(a, b):
    """a b^T of small integers: exact whatever the order, so fp64 and a checked cast"""
    return exact32(a @ b.T, "a product of the inputs")


# ---- emulation 1: the fp32 route's order (csrc/train.hip): one key (query) at a time, everything in fp32 ----------------------------
def emulate_sequential(case):
    """-> dict O, lse, dq, dk, dv of float32 arrays shaped like the expectation's"""
    B, H, T = case.B, case.H, case.T
    out = {n: np.zeros((B, H, T, 32), dtype=f32) for n in ("O", "dq", "dk", "dv")}
    out["lse"] = np.zeros((B, H, T), dtype=f32)
    c = f32(case.c)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for b in range(B):
            for h in range(H):
                q, k, v, dO = (x[b, h].astype(f32) for x in (case.q, case.k, case.v, case.dO))
                kept = np.ones((T, T), dtype=bool) if case.mask is None else case.mask[b, h].astype(bool)
                ls, dl = case.lse[b, h], case.delta[b, h]
                S, G = dots(q, k), dots(dO, v)                            # [query, key]
                # forward: per-key running maximum
                mx, l, acc = np.full(T, -np.inf, dtype=f32), np.zeros(T, dtype=f32), np.zeros((T, 32), dtype=f32)
                for j in range(T):
                    s = S[:, j] * QK_SCALE_LOG2E
                    up = s > mx
                    corr = np.where(up, np.exp2(mx - s), f32(1.0)).astype(f32)
                    l, acc, mx = l * corr, acc * corr[:, None], np.where(up, s, mx)
                    p = np.exp2(s - mx).astype(f32)
                    l = l + p
                    acc = acc + np.where(kept[:, j], p, f32(0.0))[:, None] * v[j][None, :]
                out["O"][b, h] = acc * (c / l)[:, None]
                out["lse"][b, h] = mx + np.log2(l).astype(f32)
                # dQ: keys ascending
                acc = np.zeros((T, 32), dtype=f32)
                for j in range(T):
                    p = np.exp2(fma_sub(S[:, j], QK_SCALE_LOG2E, ls)).astype(f32)
                    ds = p * (np.where(kept[:, j], G[:, j] * c, f32(0.0)) - dl)
                    acc = acc + ds[:, None] * k[j][None, :]
                out["dq"][b, h] = acc * QK_SCALE
                # dK / dV: queries ascending
                dk, dv = np.zeros((T, 32), dtype=f32), np.zeros((T, 32), dtype=f32)
                for i in range(T):
                    p = np.exp2(fma_sub(S[i, :], QK_SCALE_LOG2E, ls[i])).astype(f32)
                    pm = np.where(kept[i, :], p * c, f32(0.0))
                    ds = p * (np.where(kept[i, :], G[i, :] * c, f32(0.0)) - dl[i])
                    dv = dv + pm[:, None] * dO[i][None, :]
                    dk = dk + ds[:, None] * q[i][None, :]
                out["dk"][b, h], out["dv"][b, h] = dk * QK_SCALE, dv
    return out


# ---- emulation 2: the mixed route's order (csrc/train_mixed.inc): tiles of 32, P and dS rounded to fp16, both directions ----------
def r16(x):
    return x.astype(f16).astype(f32)


def mfma(acc, a, b, what):
    """acc + a^T b on the MFMA: fp16 operands (a, b hold fp16 values), fp32 accumulation; the operands here make every partial
    sum exact, whatever the unit's internal order -- checked"""
    return exact32(acc.astype(f64) + a.astype(f64).T @ b.astype(f64), what)


def emulate_tiled(case, mutant=None):
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(f"unknown mutant {mutant!r}")
    B, H, T, XB = case.B, case.H, case.T, 32
    out = {n: np.zeros((B, H, T, 32), dtype=f32) for n in ("O", "dq", "dk", "dv")}
    out["lse"] = np.zeros((B, H, T), dtype=f32)
    c = f32(case.c)
    n_keys = T - 1 if mutant == "drop_the_last_key" else T                # (the last key of the last, ragged tile)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for b in range(B):
            for h in range(H):
                q, k, v, dO = (r16(x[b, h].astype(f32)) for x in (case.q, case.k, case.v, case.dO))
                kept = np.ones((T, T), dtype=bool) if case.mask is None else case.mask[b, h].astype(bool)
                if mutant == "mask_word_of_the_next_key":
                    kept = np.roll(kept, -1, axis=1)
                ls, dl = case.lse[b, h], case.delta[b, h]
                S, G = dots(q, k), dots(dO, v)                            # [query, key]: the first products, fp32 accumulators
                order = np.arange(T)                                      # the k order of the transposed images
                if mutant == "swap_two_keys_of_a_tile":                   # two keys of tile 0 that belong to different classes
                    other = int(np.flatnonzero(case.kc[b, h, :XB] != case.kc[b, h, 0])[0])
                    order[[0, other]] = order[[other, 0]]
                # forward, keys in tiles: running maximum per tile, l in two halves (the lane halves' keys), P relative to it
                mx, acc = np.full(T, -np.inf, dtype=f32), np.zeros((T, 32), dtype=f32)
                l = np.zeros((2, T), dtype=f32)
                for k0 in range(0, T, XB):
                    sc = np.full((T, XB), -np.inf, dtype=f32)
                    nk = max(0, min(XB, n_keys - k0))
                    sc[:, :nk] = S[:, k0:k0 + nk] * QK_SCALE_LOG2E
                    mnew = np.maximum(mx, sc.max(axis=1))
                    corr = np.exp2(mx - mnew).astype(f32)
                    mx, l, acc = mnew, l * corr[None, :], acc * corr[:, None]
                    p = np.exp2(sc - mx[:, None]).astype(f32)
                    for i in range(16):                                   # register i of lane half g: its key of the tile
                        for g in range(2):
                            l[g] = l[g] + p[:, (i & 3) + 8 * (i >> 2) + 4 * g]
                    nv = min(XB, T - k0)
                    pm = np.where(kept[:, k0:k0 + nv], p[:, :nv] * c, f32(0.0))
                    acc = mfma(acc, r16(pm).T, v[order[k0:k0 + nv]], "O's accumulator")
                lsum = l[0] + l[1]
                out["O"][b, h] = acc * (f32(1.0) / lsum)[:, None]
                out["lse"][b, h] = mx + np.log2(lsum).astype(f32)
                # dQ: key tiles ascending
                acc = np.zeros((T, 32), dtype=f32)
                for k0 in range(0, T, XB):
                    nv = min(XB, T - k0)
                    nk = max(0, min(XB, n_keys - k0))
                    p = np.zeros((T, nv), dtype=f32)
                    p[:, :nk] = np.exp2(fma_sub(S[:, k0:k0 + nk], QK_SCALE_LOG2E, ls[:, None]))
                    d = np.where(kept[:, k0:k0 + nv], G[:, k0:k0 + nv] * c, f32(0.0))
                    ds = p * (d - dl[:, None])
                    acc = mfma(acc, r16(ds).T, k[order[k0:k0 + nv]], "dQ's accumulator")
                out["dq"][b, h] = acc * QK_SCALE
                # dK / dV: query tiles ascending (the key on the lane)
                dk, dv = np.zeros((T, 32), dtype=f32), np.zeros((T, 32), dtype=f32)
                for q0 in range(0, T, XB):
                    nq = min(XB, T - q0)
                    p = np.exp2(fma_sub(S[q0:q0 + nq, :], QK_SCALE_LOG2E, ls[q0:q0 + nq, None])).astype(f32)
                    p[:, n_keys:] = 0.0
                    kp = kept[q0:q0 + nq, :]
                    pm = np.where(kp, p * c, f32(0.0))
                    ds = p * (np.where(kp, G[q0:q0 + nq, :] * c, f32(0.0)) - dl[q0:q0 + nq, None])
                    dv = mfma(dv, r16(pm), dO[q0:q0 + nq], "dV's accumulator")
                    dk = mfma(dk, r16(ds), q[q0:q0 + nq], "dK's accumulator")
                out["dk"][b, h], out["dv"][b, h] = dk * QK_SCALE, dv
    return out


def expectation(case):
    return dict(O=case.O, lse=case.lse, dq=case.dq, dk=case.dk, dv=case.dv)


def pos_zero(x):
    """-0 -> +0, every other value as it is.  The sign of an exact zero is the one thing here that depends on the order of the
    operations: a negative accumulator times a rescale of exactly 0 is -0, and -0 survives adding products that are -0 too (a
    dropped key's 0 times a negative v), so the fp32 route, the mixed route and a plain matrix product may each hold another
    zero where the value is 0."""
    return x + f32(0.0)


def same_bits(a, b):
    """the same bits, but for the sign of a zero (pos_zero)"""
    a, b = pos_zero(np.ascontiguousarray(a, dtype=f32)), pos_zero(np.ascontiguousarray(b, dtype=f32))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
