"""Inputs on which the inference attention kernels (csrc/attn.hip, csrc/attn2.hip with its two generated loops) have to be right
bit for bit, in every arithmetic they run in ("The inference attention pinned the same way").  Three families, all of operands that are small integers or
powers of two -- exact in fp16, in bfloat16 and as hi + lo with lo = 0 -- and whose scores q . k ARE the base-2 exponents (q
arrives pre-scaled at every entry: neither attn.hip nor attn2.hip multiplies a score by anything):

selection   "selection attention" as in tests/train_exact_reference.py.  Per (sequence, head) the L keys are partitioned into
            classes of 1, 2 or 4, placed by a random permutation; a class's code is a triple of the 32 dimensions; a key is 5 on
            its class's dimensions, a query 32 on those of the class it selects.  A score is 160 times the number of shared
            dimensions: 480 on the selected class, at most 320 elsewhere.  Levels are 160 octaves apart, so every probability
            but the selected class's is exp2(-160 or less) = 0 in fp32 already (and a running maximum's rescale is 0 too): nothing
            of the 1500 other keys reaches an accumulator, in any order.  P is one power of two on the n selected keys,
            O = gate . mean of v over them, v integers in [-2, 2].  A query whose selected keys lie outside the kernel's
            reference blocks overflows the fast pass (exp2(160 - shift) = inf) and takes the kernel's other route: the SAFE
            re-run of the half kernels, the fix-up launch of the x3 / P16 ones.
graded      the fast pass's ordinary case: up to 32 classes of n_sel keys on ONE dimension each (key 2, query 2: score 4), every
            other key 0 (score 0).  Relative to score 0 a row sums to 16 n_sel + (L - n_sel) = 16 (n_sel + k) for
            L = n_sel + 16 k, a power of two for the (n_sel, k) used; O = gate (16 sum_sel v + sum_other v) / that, one exact
            dyadic rational.  Later keys score 4 octaves above the reference point without overflowing anything.
uniform     the count of keys: q = 0, every score 0, every probability the same power of two, v[j, d] = c_d +- 2^-4 alternating
            and zero-sum over the L keys (odd L: key 0 holds c_d itself).  O = gate c_d exactly; one key too many or too few
            moves it by c_d / (L +- 1).

Here: the generator with its fp64 expectation, three emulations of the kernels' orders of operation that have to reproduce the
expectation bit for bit (which is what makes a device mismatch mean a kernel error, not a property of the inputs), five mutants
that have to miss it, and describe() for the failure messages.  The one step the emulations do NOT restate is the final
acc x (gate / l): they divide exactly.  On a power-of-two row sum (selection, graded) the device's reciprocal is exact as well;
on the uniform family's L 2^-s it is not, which is why fp32 rows of that family carry a derived bound instead
(tests/test_gpu_attn_exact.py).  tests/test_attn_exact_reference.py runs all of it without a GPU."""
import itertools

import numpy as np
import torch

f32, f64, f16 = np.float32, np.float64, np.float16

Q_SEL, K_SEL = 32.0, 5.0            # selection: 32 x 5 = 160 octaves per shared dimension
TOP = 3 * Q_SEL * K_SEL             # 480: far from the ~1e6 "hopeless scores" that raise the range flag (test_gpu_x3.py)
Q_GR, K_GR = 2.0, 2.0               # graded: score 4
TRIPLES = np.array(list(itertools.combinations(range(32), 3)))   # the 4960 codes
C_UNI = (1.75, 1.875, 3.5, 3.75, 7.0, 7.5)   # [1.75, 2) 2^e: c +- 2^-4 has at most 7 significant bits (bfloat16 holds 8)
D_UNI = 2.0 ** -4

SELECTION = ((1, 1, 1), (2, 31, 1), (1, 32, 2), (2, 33, 1), (1, 63, 1), (1, 64, 1), (2, 65, 1), (1, 96, 1), (1, 127, 1), (1, 128, 2),
             (2, 129, 1), (1, 250, 1), (1, 257, 1), (1, 1012, 1), (1, 1499, 1), (2, 1500, 2))           # (n_seq, L, heads)
GRADED = ((1, 1, 17), (2, 2, 34), (1, 3, 49), (4, 4, 68), (3, 5, 83), (8, 8, 136), (1, 15, 241), (16, 16, 272), (3, 61, 979),
          (37, 91, 1493), (35, 93, 1523))                                                                # (n_sel, k, L)
UNIFORM = (1, 33, 64, 65, 129, 257, 1500)                                                                # L
ROWMAP = (2, 129, 1)   # the selection case that also goes through the time-direction row map (as B = 1, F = 2)
MUTANTS = ("drop_the_last_key", "count_a_padding_slot", "swap_two_keys_of_a_block", "skip_the_rescale", "gate_of_the_next_head")
FORMATS = ("half", "f32", "hl32", "hi")   # half rows | out_f32 = 1 | hl32 rows (hi + lo) | the hi halves of out_f32 = 2 rows


def gate_of(s, h, t):
    """1, 0.5 or 0.25: exact, and never the same on neighbouring heads"""
    return 2.0 ** -((s + h + t) % 3)


class Case:
    """q, k, v [S, H, L, 32] and gates [S, H, L] (float64 holding exact values), kc [S, H, L] the class of a key (-1: none), qc
    the class a query selects (-1: none), want [S, H, L, 32] the exact output, fast_half / fast_x3 [S, H, L] whether the query
    itself stays in the fast pass of the half kernels (reference point: key block 0) / of the x3 and P16 kernels (the first
    two key blocks and the query's own)."""

    def __init__(self, family, n_seq, L, heads, n_sel=0):
        self.family, self.S, self.L, self.H, self.n_sel = family, n_seq, L, heads, n_sel
        self.id = f"{family}-{n_seq}x{L}x{heads}"
        rng = np.random.default_rng([{"selection": 1, "graded": 2, "uniform": 3}[family], n_seq, L, heads])
        S, H = n_seq, heads
        self.q, self.k, self.v = (np.zeros((S, H, L, 32)) for _ in range(3))
        self.kc, self.qc = np.full((S, H, L), -1, dtype=np.int64), np.full((S, H, L), -1, dtype=np.int64)
        self.gates = np.array([[[gate_of(s, h, t) for t in range(L)] for h in range(H)] for s in range(S)])
        getattr(self, "draw_" + family)(rng)
        for x in (self.q, self.k, self.v):   # exact in fp16 and in bfloat16
            assert np.array_equal(x.astype(f16).astype(f64), x)
            assert np.array_equal(torch.from_numpy(x).to(torch.bfloat16).double().numpy(), x)
        self.expect()

    # ---- the three families ----
    def draw_selection(self, rng):
        L = self.L
        alone = list(dict.fromkeys((L - 1, 32 * ((L - 1) // 32))))   # the last real key, the first key of the last block
        for s in range(self.S):
            for h in range(self.H):
                if s == 0 and h == 0 and self.S * self.H > 1:
                    sizes = [1] * L        # the first pair of a case that has several: every key the sole selected key of a query
                else:                      # elsewhere those two keys are classes of their own, the rest is drawn
                    sizes, left = [1] * len(alone), L - len(alone)
                    while left:
                        n = min(int(rng.choice((1, 2, 4))), left)
                        sizes.append(2 if n == 3 else n)
                        left -= sizes[-1]
                n_cls = len(sizes)
                perm = rng.permutation(L)
                for i, pos in enumerate(alone):
                    j = int(np.flatnonzero(perm == pos)[0])
                    perm[[i, j]] = perm[[j, i]]
                self.kc[s, h, perm] = np.repeat(np.arange(n_cls), sizes)
                for pos in alone:
                    assert (self.kc[s, h] == self.kc[s, h, pos]).sum() == 1
                # every class is selected by at least one query, the others at random
                self.qc[s, h] = rng.permutation(np.concatenate([np.arange(n_cls), rng.integers(0, n_cls, L - n_cls)]))
                code = TRIPLES[rng.permutation(len(TRIPLES))[:n_cls]]
                for t in range(L):
                    self.k[s, h, t, code[self.kc[s, h, t]]] = K_SEL
                    self.q[s, h, t, code[self.qc[s, h, t]]] = Q_SEL
        self.draw_v(rng)

    def draw_graded(self, rng):
        L, n = self.L, self.n_sel
        n_cls = min(32, max(1, (L - 1) // n))       # (at least one key stays in the background)
        for s in range(self.S):
            for h in range(self.H):
                perm = rng.permutation(L)
                self.kc[s, h, perm[:n_cls * n]] = np.repeat(np.arange(n_cls), n)
                self.qc[s, h] = rng.permutation(np.concatenate([np.arange(n_cls), rng.integers(0, n_cls, L - n_cls)]))
                dim = rng.permutation(32)[:n_cls]   # a class's one dimension
                for t in range(L):
                    if self.kc[s, h, t] >= 0:
                        self.k[s, h, t, dim[self.kc[s, h, t]]] = K_GR
                    self.q[s, h, t, dim[self.qc[s, h, t]]] = Q_GR
        self.draw_v(rng)

    def draw_v(self, rng):
        for attempt in range(50):
            self.v = rng.integers(-2, 3, size=self.v.shape).astype(f64)
            if self.L == 1 or len(np.unique(self.v.reshape(-1, 32), axis=0)) == self.S * self.H * self.L:
                return                              # distinct rows: a value taken from another key shows
        raise AssertionError("no draw of v with distinct rows")

    def draw_uniform(self, rng):
        L = self.L
        self.kc[:] = np.arange(L)                   # (no classes: every key stands for itself)
        self.c = np.zeros((self.S, self.H, 32))
        j = np.arange(L)
        for s in range(self.S):
            for h in range(self.H):
                for d in range(32):
                    self.c[s, h, d] = C_UNI[(d + h + s) % len(C_UNI)] * (-1.0 if (d // 3 + h) % 2 else 1.0)
                    off = np.where((j + d) % 2 == 0, D_UNI, -D_UNI)
                    if L % 2:
                        off[0] = 0.0                # (key 0 and not the last one: dropping the last key still shows)
                    assert off.sum() == 0.0
                    self.v[s, h, :, d] = self.c[s, h, d] + off

    def expect(self):
        s = self.q @ self.k.transpose(0, 1, 3, 2)                        # [S, H, query, key], exact
        sel = (self.kc[:, :, None, :] == self.qc[:, :, :, None]) & (self.qc[:, :, :, None] >= 0)
        self.sel, self.scores = sel, s
        g = self.gates[..., None]
        if self.family == "selection":
            assert s.max() == TOP and np.array_equal(s == TOP, sel) and s[~sel].max(initial=0.0) <= TOP - Q_SEL * K_SEL
            size = sel.sum(-1, keepdims=True)
            assert np.isin(size, (1, 2, 4)).all()
            self.want = g * ((sel / size) @ self.v)
        elif self.family == "graded":
            assert np.array_equal(s == Q_GR * K_GR, sel) and np.isin(s, (0.0, Q_GR * K_GR)).all() and (sel.sum(-1) == self.n_sel).all()
            total = 16.0 * self.n_sel + (self.L - self.n_sel)
            assert total == 2.0 ** round(np.log2(total))                  # a power of two: the division is exact
            self.want = g * ((sel * 15.0 + 1.0) @ self.v) / total
        else:
            assert not s.any() and not sel.any()
            self.want = g * (self.v.sum(axis=2, keepdims=True) / self.L)
            assert np.array_equal(self.want, g * self.c[:, :, None, :])      # gate c_d, exactly
        assert np.array_equal(self.want.astype(f32).astype(f64), self.want), "the expectation is not exact in fp32"
        key = np.arange(self.L)
        if self.family == "selection":
            own = key[:, None] // 32 == key[None, :] // 32
            self.fast_half = (sel & (key < 32)).any(-1)
            self.fast_x3 = (sel & ((key < 64)[None, :] | own)).any(-1)
        else:
            self.fast_half = self.fast_x3 = np.ones((self.S, self.H, self.L), dtype=bool)

    # ---- the device's layouts ----
    def rows(self, x):
        """[S, H, L, w] -> [S L, H w]: the rows a launch without a row map writes, and the q | k | v columns bt_attention reads"""
        S, H, L, w = x.shape
        return np.ascontiguousarray(x.transpose(0, 2, 1, 3).reshape(S * L, H * w))

    def unrows(self, x):
        """[S L, H 32] -> [S, H, L, 32]"""
        return np.asarray(x).reshape(self.S, self.L, self.H, 32).transpose(0, 2, 1, 3)

    def pairs(self, x):
        """[S, H, L, ...] -> [S H, L, ...]: the (sequence, head) pairs of the fragment-major operands"""
        return x.reshape((self.S * self.H,) + x.shape[2:])

    def describe(self, name, got, want, rule=None, tol=0.0):
        """None, or the first differing (sequence, head, query, column) of a [S, H, L, 32] output with what the query selects and
        the pass its kernel is expected to take (rule: "half" / "x3" / None for the kernels that have one pass only); tol: the
        absolute difference allowed per element (0: the same bits but for the sign of a zero)"""
        g, w = (np.ascontiguousarray(x, dtype=f64) + 0.0 for x in (got, want))   # (+ 0.0: the sign of a zero does not count)
        with np.errstate(invalid="ignore"):
            bad = np.argwhere(~(np.abs(g - w) <= tol))                            # (a NaN differs from everything)
        if not len(bad):
            return None
        s, h, t, d = (int(i) for i in bad[0])
        keys = np.flatnonzero(self.sel[s, h, t]).tolist()
        fast = {None: None, "half": self.fast_half, "x3": self.fast_x3}[rule]
        if fast is None:
            route = "one pass (online softmax)"
        elif fast[s, h, t]:
            group = fast[s, h, t // 128 * 128:t // 128 * 128 + 128].all()
            route = "the fast pass" + ("" if rule == "x3" or group else ", but its 128-query workgroup re-runs in the SAFE pass")
        else:
            route = "the SAFE re-run of its workgroup" if rule == "half" else "the fix-up launch"
        return (f"{name} [{self.id}]: {len(bad)} of {g.size} elements differ, the first at (sequence, head, query, column) = {(s, h, t, d)}: "
                f"got {g[s, h, t, d]!r}, want {w[s, h, t, d]!r}.  Query {t} (gate {self.gates[s, h, t]}) selects class {self.qc[s, h, t]}: "
                f"keys {keys} (key blocks {sorted({j // 32 for j in keys})}) of L = {self.L} ({(self.L + 31) // 32} blocks, {self.L % 32 or 32} "
                f"keys in the last); expected route: {route}")


_cache = {}


def make(family, *shape):
    """the one Case of a (family, shape): selection (n_seq, L, heads) | graded (n_sel, k, L) | uniform (L,)"""
    key = (family,) + tuple(shape)
    if key not in _cache:
        if family == "selection":
            _cache[key] = Case(family, *shape)
        elif family == "graded":
            n_sel, k, L = shape
            assert L == n_sel + 16 * k
            _cache[key] = Case(family, 1, L, 1 + (k % 2), n_sel=n_sel)   # (heads 1 or 2)
        else:
            _cache[key] = Case(family, 1, shape[0], 1 if shape[0] >= 1000 else 2)
    return _cache[key]


def all_cases():
    return [make("selection", *s) for s in SELECTION] + [make("graded", *s) for s in GRADED] + [make("uniform", L) for L in UNIFORM]


# ---- output formats ---------------------------------------------------------------------------------------------------------------
def r_half(x, half):
    """x rounded to the half type ("f16" / "bf16", the latter through torch's bfloat16), as float64"""
    x = np.ascontiguousarray(x, dtype=f32)
    with np.errstate(over="ignore"):
        return x.astype(f16).astype(f64) if half == "f16" else torch.from_numpy(x).to(torch.bfloat16).double().numpy()


def round_out(x, fmt, half="f16"):
    """an fp32-valued result as the kernel stores it in ``fmt`` (FORMATS), as float64"""
    x32 = np.ascontiguousarray(x, dtype=f32)
    if fmt == "f32":
        return x32.astype(f64)
    if fmt == "half":
        return r_half(x32, half)
    hi = r_half(x32, "f16")
    if fmt == "hi":
        return hi
    with np.errstate(invalid="ignore"):
        return hi + r_half((x32.astype(f64) - hi).astype(f32), "f16")   # hl32: hi + lo


def same(a, b):
    """the same values, but for the sign of a zero; NaN equals nothing"""
    return a.shape == b.shape and bool(np.all((np.asarray(a, dtype=f64) + 0.0) == (np.asarray(b, dtype=f64) + 0.0)))


# ---- emulations ---------------------------------------------------------------------------------------------------------------------
def exp2_32(x):
    """exp2 of integral exponents as fp32: exact, 0 below 2^-149, inf from 2^128"""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(np.asarray(x, dtype=f64)).astype(f32)


def _pair_inputs(case, s, h, mutant):
    """-> S [L, slots] (scores, slot = key position padded to whole blocks; padding slots hold K = 0, i.e. score 0), V [slots, 32],
    n_keys (slots from here on are masked), gate [L] -- with the mutant's change applied"""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(f"unknown mutant {mutant!r}")
    L = case.L
    slots = (L + 31) // 32 * 32
    S, V = np.zeros((L, slots)), np.zeros((slots, 32))
    S[:, :L], V[:L] = case.scores[s, h], case.v[s, h]
    n_keys = L
    if mutant == "drop_the_last_key":
        n_keys = L - 1
    elif mutant == "count_a_padding_slot" and L % 32:
        n_keys = L + 1                                                   # (a whole last block has no padding slot to count)
    elif mutant == "swap_two_keys_of_a_block":                          # V of two keys of block 0 that belong to different classes
        other = np.flatnonzero(case.kc[s, h, :32] != case.kc[s, h, 0])
        if len(other):
            V[[0, int(other[0])]] = V[[int(other[0]), 0]]
    hg = (h + 1) % case.H if mutant == "gate_of_the_next_head" else h
    return S, V, n_keys, case.gates[s, hg]


def _normalise(acc, l, gate):
    """acc gate / l by exact division, rounded once to fp32 (the module docstring says why)"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (acc.astype(f64) * gate[:, None] / l.astype(f64)[:, None]).astype(f32)


def _madd(acc, p, v):
    """acc + p v on the matrix pipe, fp32 accumulators (every partial sum of these inputs is exact in fp32 whatever the order)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc.astype(f64) + p.astype(f64) @ v).astype(f32)


def emulate_online(case, mutant=None):
    """(a) csrc/attn.hip: online softmax in fp32, one key at a time -> (O [S, H, L, 32] float32, None)"""
    out = np.zeros((case.S, case.H, case.L, 32), dtype=f32)
    for s in range(case.S):
        for h in range(case.H):
            S, V, n_keys, gate = _pair_inputs(case, s, h, mutant)
            L = case.L
            m, l, acc = np.full(L, -1e30, dtype=f32), np.zeros(L, dtype=f32), np.zeros((L, 32), dtype=f32)
            for j in range(n_keys):
                sc = S[:, j].astype(f32)
                m_new = np.maximum(m, sc)
                alpha = exp2_32(m - m_new)
                l = l * alpha
                if mutant != "skip_the_rescale":
                    acc = acc * alpha[:, None]
                m = m_new
                p = exp2_32(sc - m)
                l = l + p
                acc = _madd(acc, p[:, None], V[j][None, :])
            out[s, h] = _normalise(acc, l, gate)
    return out, None


def emulate_half(case, half="f16", mutant=None):
    """(b) the half kernels of csrc/attn2.hip: key blocks of 32, probabilities relative to the maximum over key block 0 minus the
    shift (4 octaves for fp16, none for bfloat16) and rounded to the half type, row sums from the rounded values; a row sum that
    is not below 1e30 re-runs the 128 queries of its workgroup as a classic online softmax over the blocks (SAFE)
    -> (O, rerun [S, H, L]: whether the query's workgroup re-ran)"""
    shift = 4.0 if half == "f16" else 0.0
    out = np.zeros((case.S, case.H, case.L, 32), dtype=f32)
    rerun = np.zeros((case.S, case.H, case.L), dtype=bool)
    for s in range(case.S):
        for h in range(case.H):
            S, V, n_keys, gate = _pair_inputs(case, s, h, mutant)
            L, slots = case.L, S.shape[1]
            live = np.arange(slots) < n_keys
            ref = np.where(live[:32], S[:, :32], -1e30).max(axis=1)
            l, acc = np.zeros(L, dtype=f32), np.zeros((L, 32), dtype=f32)
            for b0 in range(0, slots, 32):
                p = np.where(live[b0:b0 + 32], r_half(exp2_32(S[:, b0:b0 + 32] - ref[:, None] - shift), half), 0.0)
                if case.family != "selection" and half == "f16":
                    assert (p[p > 0] >= 2.0 ** -14).all(), "a subnormal fp16 probability"
                with np.errstate(over="ignore"):
                    l = (l.astype(f64) + p.sum(axis=1)).astype(f32)
                acc = _madd(acc, p, V[b0:b0 + 32])
            over = ~(l < f32(1e30))
            group = np.repeat(np.add.reduceat(over, np.arange(0, L, 128)) > 0, 128)[:L]
            # the SAFE pass, for everybody; taken where the workgroup re-ran
            m, l2, acc2 = np.full(L, -1e30, dtype=f32), np.zeros(L, dtype=f32), np.zeros((L, 32), dtype=f32)
            for b0 in range(0, slots, 32):
                sc = np.where(live[b0:b0 + 32], S[:, b0:b0 + 32], -1e30).astype(f32)
                m_new = np.maximum(m, sc.max(axis=1))
                alpha = exp2_32(m - m_new)
                l2 = l2 * alpha
                if mutant != "skip_the_rescale":
                    acc2 = acc2 * alpha[:, None]
                m = m_new
                p = r_half(exp2_32(sc - m[:, None]), half)
                l2 = (l2.astype(f64) + p.sum(axis=1)).astype(f32)
                acc2 = _madd(acc2, p, V[b0:b0 + 32])
            out[s, h] = np.where(group[:, None], _normalise(acc2, l2, gate), _normalise(acc, l, gate))
            rerun[s, h] = group
    return out, rerun


def emulate_p16(case, mutant=None):
    """(c) the P16 rule as _attn_ref_p16 of test_gpu_x3.py states it: reference point = the maximum over the first two key blocks
    and the query's own block, rounded up to a whole octave, plus 3; a query whose row maximum lies 15.99 or more above it is
    computed again (by the fix-up launch: two sweeps, no rescale) on ceil(row maximum) - 14; probabilities rounded to fp16, row
    sums from the rounded values.  The three-term x3 kernels take the same reference points and the same hand-over (their
    probabilities are hi + lo halves: on these inputs lo = 0, the same numbers) -> (O, rerun [S, H, L])"""
    out = np.zeros((case.S, case.H, case.L, 32), dtype=f32)
    rerun = np.zeros((case.S, case.H, case.L), dtype=bool)
    for s in range(case.S):
        for h in range(case.H):
            S, V, n_keys, gate = _pair_inputs(case, s, h, mutant)
            L, slots = case.L, S.shape[1]
            live = np.arange(slots) < n_keys
            own = np.arange(L)[:, None] // 32 == np.arange(slots)[None, :] // 32
            lead = np.arange(slots)[None, :] < 64
            m = np.ceil(np.where((own | lead) & live, S, -1e30).max(axis=1)) + 3.0
            top = np.where(live, S, -1e30).max(axis=1)
            over = (top - m) >= 15.99
            with np.errstate(over="ignore"):   # the device's own test: the fast pass's row sum is not below 65504
                fast_sum = np.where(live, r_half(exp2_32(S - m[:, None]), "f16"), 0.0).sum(axis=1)
            assert np.array_equal(over, ~(fast_sum < 65504.0)) or n_keys == 0
            m = np.where(over, np.ceil(top) - 14.0, m)
            l, acc = np.zeros(L, dtype=f32), np.zeros((L, 32), dtype=f32)
            for b0 in range(0, slots, 32):
                p = np.where(live[b0:b0 + 32], r_half(exp2_32(S[:, b0:b0 + 32] - m[:, None]), "f16"), 0.0)
                if case.family != "selection":
                    assert (p[p > 0] >= 2.0 ** -14).all(), "a subnormal fp16 probability"
                l = (l.astype(f64) + p.sum(axis=1)).astype(f32)
                acc = _madd(acc, p, V[b0:b0 + 32])
            out[s, h] = _normalise(acc, l, gate)
            rerun[s, h] = over
    return out, rerun


EMULATIONS = {"online": lambda c, m=None: emulate_online(c, m), "half_f16": lambda c, m=None: emulate_half(c, "f16", m),
              "half_bf16": lambda c, m=None: emulate_half(c, "bf16", m), "p16": lambda c, m=None: emulate_p16(c, m)}
# the formats each arithmetic is stored in (and, for round_out, in which half type)
STORED = {"online": (("f32", "f16"), ("half", "f16"), ("half", "bf16")), "half_f16": (("half", "f16"),), "half_bf16": (("half", "bf16"),),
          "p16": (("hl32", "f16"), ("f32", "f16"), ("hi", "f16"))}
# skip_the_rescale is a mutant of a running maximum: of (a) and of (b)'s SAFE re-run.  The fix-up launch behind (c) takes the row
# maxima in a sweep of their own and has no rescale to skip.
APPLIES = {m: ("online", "half_f16", "half_bf16", "p16") for m in MUTANTS}
APPLIES["skip_the_rescale"] = ("online", "half_f16", "half_bf16")


# ---- which mutant is caught where ------------------------------------------------------------------------------------------------
BITS = {("f32", "f16"): 24, ("hl32", "f16"): 22, ("half", "f16"): 11, ("hi", "f16"): 11, ("half", "bf16"): 8}   # significand bits


def claims(mutant, emulation, case, fmt, half):
    """True: this (case, output format) catches the mutant, and tests/test_gpu_attn_exact.py relies on it; False: it cannot (the
    mutant computes the same numbers, or its change provably rounds back); None: rounding decides, nothing is claimed.
    T is a graded row's sum 16 (n_sel + k); p the significand bits of the format; a change of more than one part in 2^(p - 1) of
    an element always reaches its stored value, one of less than one part in 2^(p + 1) never does on the uniform family, whose
    expected values c_d are representable."""
    p, L, fam = BITS[(fmt, half)], case.L, case.family
    wide = p >= 22                                   # fp32 and hl32 rows hold every expected value with bits to spare
    T = 16 * case.n_sel + (L - case.n_sel)
    if emulation not in APPLIES[mutant]:
        return None
    if mutant == "drop_the_last_key":
        if fam == "selection" or L == 1:
            return True                              # the last key is the only one of its class: a query is left with nothing
        if fam == "graded":
            return True if wide or T < 2 ** (p - 1) else None          # every element moves by 1 / (T - 1) of itself at least
        # uniform: the mean moves by 2^-4 / (L - 1), half an ulp of c = 1.75 is 2^-p
        return True if wide or L - 1 < 2 ** (p - 4) else (False if L - 1 > 2 ** (p - 4) else None)
    if mutant == "count_a_padding_slot":
        if L % 32 == 0 or fam == "selection":
            return False                             # no slot to count / a score of 0 is 480 octaves down: probability 0
        if fam == "graded":
            return True if wide or T + 1 < 2 ** (p - 1) else None      # every element shrinks by 1 / (T + 1) of itself
        # uniform: c L / (L + 1); half an ulp of c is between c 2^-p / 1.875 and c 2^-p / 1.75
        return True if wide or L + 1 < 1.75 * 2 ** p else (False if L + 1 > 1.875 * 2 ** p else None)
    if mutant == "swap_two_keys_of_a_block":
        if fam == "uniform" or L == 1:
            return False                             # equal probabilities: the sum does not care which v sits where
        if fam == "selection":
            return True
        return True if wide or T < 2 ** (p - 1) else None              # 15 (v_a - v_b) / T for the queries of a's class
    if mutant == "skip_the_rescale":
        if fam == "uniform" or L == 1:
            return False                             # the maximum never rises over a non-empty accumulator
        if emulation == "online":
            return True if fam == "selection" or wide or T < 2 ** (p - 1) else None
        if fam == "graded":
            return False                             # (b) has a running maximum in its SAFE re-run only: graded never gets there
        return L > 32                                # selection: a re-run needs a selected key beyond block 0
    if mutant == "gate_of_the_next_head":
        return case.H > 1                            # neighbouring heads' gates differ by a factor of 2 or 4
    raise ValueError(mutant)
