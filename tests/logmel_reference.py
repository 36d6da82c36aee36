"""What the tests of csrc/logmel.hip measure with (tests/test_logmel_reference.py on the CPU, tests/test_gpu_logmel_spec.py on
the device).  The float64 truth is oracle.beat_this_oracle.logmel(x.double(), torch.float64); this module adds

  * unit(x): for every element of the output, the size of ONE fp32 rounding of this operation, so that an error is counted in
    roundings wherever it falls -- a loud band, an empty band of a pure tone or a track of 2^-30 alike:

        b[f, m] = 1000 W[m] u (S[f] / 32) / (1 + 1000 mel64[f, m])  +  u (1 + out64[f, m]),       u = 2^-24

    W[m] is the column sum of the filterbank, S[f] the 2-norm of frame f after reflect padding and windowing.  An fp32 FFT
    leaves an error of O(u S) in a bin whatever that bin holds (Parseval: the rounding of every butterfly is spread over all
    bins), the mel sum scales it by at most W[m], the logarithm by 1 / (1 + 1000 mel); the second term is the rounding of the
    final logarithm itself (and of 1 + y in front of it).  r(out, x) = max |out - out64| / b is the one error measure.
  * twin(x, tables, mutate): an fp32 numpy restatement of the kernel's DATAFLOW -- reflect index map, window product, even +
    i odd packing, three radix-8 stages with tw1 / tw2 in the kernel's index order (n = 64 a + 8 b + c, k = p + 8 q + 64 r),
    the split step with tw3, 1 / 32, the banded mel sum over mel_start / mel_len / mel_w, log(1 + 1000 acc) -- and six
    single-entry mutations of it.  It says how large r is for a correct fp32 evaluation that is not the reference's, and how
    large for each kind of wrong one.  (It does not reproduce the butterflies' addition order or FMA contraction.)
  * CASES: the named signals both test modules run."""
import functools
import math

import numpy as np
import torch

from oracle import beat_this_oracle as O

U = 2.0 ** -24
N_FFT, HOP, PAD = O.N_FFT, O.HOP, O.N_FFT // 2


# ---- truth, unit and the error measure ----------------------------------------------------------------------------------------
def as_f32(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)) if not torch.is_tensor(x) else x.detach().cpu().float()


def truth(x):
    """float64 (frames, 128) of the fp32 samples x"""
    return O.logmel(as_f32(x).double(), torch.float64)


@functools.lru_cache(maxsize=None)
def filter_sums():
    """W[m]: column sums of the filterbank the reference multiplies by, float64 [128]"""
    return O.mel_filterbank(torch.float64).sum(0)


def frame_norms(x):
    """S[f]: 2-norm of frame f after reflect padding and windowing, float64 [frames]"""
    xd = as_f32(x).double()
    xp = torch.nn.functional.pad(xd[None, None, :], (PAD, PAD), mode="reflect")[0, 0]
    win = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64)
    return (xp.unfold(0, N_FFT, HOP) * win).norm(dim=1)


def unit(x, out64=None):
    """float64 (frames, 128): one fp32 rounding of the log-mel of x, element by element (module docstring)"""
    out64 = truth(x) if out64 is None else out64
    y = torch.expm1(out64)                                                # 1000 mel64
    return 1000.0 * filter_sums()[None, :] * U * (frame_norms(x)[:, None] / 32.0) / (1.0 + y) + U * (1.0 + out64)


def r_map(out, x):
    """|out - out64| / b, float64 (frames, 128); a non-finite output counts as infinitely wrong"""
    out64 = truth(x)
    out = torch.as_tensor(np.asarray(out)).double() if not torch.is_tensor(out) else out.detach().cpu().double()
    assert out.shape == out64.shape, (tuple(out.shape), tuple(out64.shape))
    e = (out - out64).abs() / unit(x, out64)
    return torch.where(torch.isfinite(out), e, torch.full_like(e, math.inf))


def r(out, x):
    return float(r_map(out, x).max())


def r_ref(x):
    """the reference's own fp32 arithmetic against float64"""
    return r(O.logmel(as_f32(x), torch.float32), x)


# ---- the twin -----------------------------------------------------------------------------------------------------------------
MUTATIONS = ("tw1", "tw2", "tw3", "tap", "reflect", "frame")
MUT_TW1 = 3 * 8 + 5                 # tw1[b = 3][p = 5]
MUT_TW2 = 64 + 3 * 64 + 37          # tw2[c = 3][m = 37]
MUT_TW3_BIN = 300                   # tw3[300]: only X[300] reads it
MUT_TAP_FILTER = 90                 # the last tap of filter 90


def reflect_index(j, n):
    """sample index of position j of the reflect-padded track (center=True, pad_mode="reflect"): one reflection per side"""
    j = np.where(j < 0, -j, j)
    return np.where(j >= n, 2 * (n - 1) - j, j)


def frame_indices(n, mutate=None):
    """int64 (frames, 1024): the sample each position of each frame reads"""
    frames = 1 + n // HOP
    s0 = np.arange(frames, dtype=np.int64)[:, None] * HOP - (PAD - 1 if mutate == "frame" else PAD)
    j = s0 + np.arange(N_FFT, dtype=np.int64)[None, :]
    if mutate == "reflect":
        j = np.where(j < 0, -j - 1, j)
    return reflect_index(j, n)


@functools.lru_cache(maxsize=None)
def _dft8():
    a = np.arange(8)
    ang = -2.0 * np.pi * np.outer(a, a) / 8.0
    return (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64)


def twin(x, tables, mutate=None):
    """fp32 (frames, 128); ``tables`` = beat_this_amd.tables.logmel_tables()"""
    assert mutate is None or mutate in MUTATIONS
    x = as_f32(x).numpy()
    tw = tables["twiddle"].astype(np.float32).copy()
    mel_w = tables["mel_w"].astype(np.float32).copy()
    start, length = tables["mel_start"].astype(np.int64), tables["mel_len"].astype(np.int64)
    if mutate == "tw1":
        tw[MUT_TW1, 1] = -tw[MUT_TW1, 1]
    elif mutate == "tw2":
        tw[MUT_TW2, 1] = -tw[MUT_TW2, 1]
    elif mutate == "tw3":
        tw[576 + MUT_TW3_BIN, 1] = -tw[576 + MUT_TW3_BIN, 1]
    elif mutate == "tap":
        mel_w[MUT_TAP_FILTER, length[MUT_TAP_FILTER] - 1] = 0.0
    twc = (tw[:, 0] + 1j * tw[:, 1]).astype(np.complex64)
    tw1 = twc[:64].reshape(8, 8)                       # [b][p]
    tw2 = twc[64:576].reshape(8, 8, 8)                 # [c][q][p]   (m = p + 8 q)
    tw3 = tw[576:]                                     # [k] (cos, -sin)
    D = _dft8()

    fr = x[frame_indices(len(x), mutate)] * tables["window"].astype(np.float32)[None, :]
    z = (fr[:, 0::2] + 1j * fr[:, 1::2]).astype(np.complex64).reshape(-1, 8, 8, 8)       # [f][a][b][c], n = 64 a + 8 b + c
    s1 = np.einsum("pa,fabc->fpbc", D, z) * tw1.T[None, :, :, None]                      # [f][p][b][c]
    s2 = np.einsum("qb,fpbc->fqpc", D, s1) * tw2.transpose(1, 2, 0)[None]                # [f][q][p][c]
    Z = np.einsum("rc,fqpc->frqp", D, s2).astype(np.complex64).reshape(-1, 512)          # k = p + 8 q + 64 r

    k = np.arange(513)
    A, B = Z[:, k & 511], Z[:, (512 - k) & 511]
    a, b, c, d = A.real, A.imag, B.real, B.imag
    half = np.float32(0.5)
    er, ei, orr, oi = half * (a + c), half * (b - d), half * (a - c), half * (b + d)
    tx, ty = tw3[None, :, 0], tw3[None, :, 1]
    xr = er + (tx * oi + ty * orr)
    xi = ei - (tx * orr - ty * oi)
    mag = np.zeros((Z.shape[0], 513 + 32), dtype=np.float32)
    mag[:, :513] = np.sqrt(xr * xr + xi * xi) * np.float32(0.03125)

    acc = np.zeros((Z.shape[0], 128), dtype=np.float32)
    for i in range(int(length.max())):
        acc = acc + mag[:, start + i] * np.where(i < length, mel_w[:, i], np.float32(0.0))[None, :]
    out = np.log(np.float32(1.0) + np.float32(1000.0) * acc)
    assert out.dtype == np.float32
    return out


# ---- the signals --------------------------------------------------------------------------------------------------------------
N_CASE = 4410
# 513 is the shortest track; around the multiples of 441 the frame count changes; at 953 and 1394 the kernel's interior test
# (s0 >= 0 and s0 + 1024 <= N) first holds for frame 1 and frame 2; from 513 to 952 frame 1 reflects at both ends
LENGTHS = (513, 514, 881, 882, 883, 952, 953, 954, 1023, 1024, 1025, 1322, 1323, 1324, 1393, 1394, 1395, 1764, 1835, 1836)


def gauss(n, seed, sigma):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g, dtype=torch.float64) * sigma).float()


def tone(n, bin_, amp=0.5, phase=0.0):
    """amp sin(2 pi bin n / 1024 + phase), rounded to fp32"""
    return (amp * torch.sin(2.0 * math.pi * bin_ * torch.arange(n, dtype=torch.float64) / N_FFT + phase)).float()


def chirp(n, f0=20.0, f1=11000.0):
    t = torch.arange(n, dtype=torch.float64) / O.SAMPLE_RATE
    T = n / O.SAMPLE_RATE
    return (0.5 * torch.sin(2.0 * math.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / T))).float()


def impulse(n, at):
    x = torch.zeros(n, dtype=torch.float32)
    x[at] = 1.0
    return x


def length_track(n):
    """noise plus a tone, n samples (the tracks of LENGTHS)"""
    return gauss(n, 7000 + n, 0.1) + tone(n, 37.3, 0.3, 0.4)


CASES = {
    "noise_0.1": lambda: gauss(N_CASE, 11, 0.1),
    "noise_1e-6": lambda: gauss(N_CASE, 12, 1e-6),
    "noise_2^-30": lambda: gauss(N_CASE, 13, 2.0 ** -30),
    "noise_1e4": lambda: gauss(N_CASE, 14, 1e4),
    "tone_1": lambda: tone(N_CASE, 1),
    "tone_7": lambda: tone(N_CASE, 7),
    "tone_100.5": lambda: tone(N_CASE, 100.5),
    "tone_300": lambda: tone(N_CASE, 300),
    "tone_400": lambda: tone(N_CASE, 400),
    "tone_511": lambda: tone(N_CASE, 511),
    "dc_0.25": lambda: torch.full((N_CASE,), 0.25, dtype=torch.float32),
    "alternating_0.5": lambda: 0.5 * (1.0 - 2.0 * (torch.arange(N_CASE) % 2)).float(),
    "chirp": lambda: chirp(N_CASE),
    "impulse_2000": lambda: impulse(N_CASE, 2000),
    "tone_100_noise_1e-3": lambda: tone(N_CASE, 100) + gauss(N_CASE, 15, 1e-3),
    **{f"length_{n}": functools.partial(length_track, n) for n in LENGTHS},
}


@functools.lru_cache(maxsize=None)
def case(name):
    """the fp32 samples of CASES[name] (computed once; do not write into them)"""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def r_ref_worst():
    """R_REF: the worst r of the reference's own fp32 arithmetic over CASES.  The gate of every tolerance comparison is
    GATE = 3 R_REF: the kernel has three things the reference has not -- another FFT factorisation with fp32 table twiddles,
    FMA contraction, 1-ulp hardware sqrt and log -- and each adds a term no larger than the one already there."""
    return max(r_ref(case(name)) for name in CASES)


def gate():
    return 3.0 * r_ref_worst()
