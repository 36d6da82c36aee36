"""Plain numpy statements of the two resamplers (csrc/frontend.hip: bt_resample; csrc/stretch.hip: bt_resample_ratio) and the
tools that measure them against their SPECIFICATION instead of against a second copy of their design: sine tones, a
least-squares gain fit at the known output frequency, and the filter's frequency response by direct summation.

Specification (beat_this_amd/tables.py): linear phase with no delay, flat up to 0.913 x the lower Nyquist frequency, nothing
from 1.0 x the lower Nyquist frequency on; "flat" and "nothing" are 1e-6 (-120 dB).  Nothing here reads the design constants of
tables.py: the filter comes in as an argument, the pass and stop bands below are the specification's.

numpy only.  Shared by tests/test_resample_spec.py (CPU) and tests/test_gpu_resample_spec.py (device)."""
from math import ceil, gcd, sqrt

import numpy as np

OUT_RATE = 22050
RATES = (8000, 11025, 16000, 32000, 44100, 48000, 66150, 88200, 96000, 110250, 176400, 192000, 352800, 22051)
PASS_END, STOP_BEGIN = 0.913, 1.0          # x the lower Nyquist frequency
SPEC = 1e-6                                # pass-band gain error and stop-band gain: -120 dB
PASS_TONES = (0.031, 0.47, 0.913)          # x the lower Nyquist frequency
STOP_TONES = (1.003, 1.37, 1.9)            # likewise; used where the tone is below the input's Nyquist frequency
TONE_PHASE, TONE_AMP = 0.7, 0.5
RATIO_STEPS = {"0.25": 0.25, "-5st": 2.0 ** (-5 / 12), "1": 1.0, "+6st": 2.0 ** (6 / 12), "2": 2.0, "4": 4.0}
RATIO_N_IN = 60000


def up_down(sr, out_rate=OUT_RATE):
    g = gcd(int(sr), out_rate)
    return out_rate // g, int(sr) // g


def n_out_of(sr):
    """outputs of the tone tests: three 2048-output decimator workgroups and a ragged 7 (25 workgroups of resample_kernel);
    at 22051 Hz enough for tap indices m down + half beyond 2^31 (from output 97 400 on)"""
    return 100003 if sr == 22051 else 6151


def n_in_for(n_out, up, down):
    """the shortest input with ceil(n_in up / down) >= n_out"""
    return -(-n_out * down // up)


def tone_fractions(lo_over_hi):
    """(pass-band, stop-band) tone frequencies as fractions of the lower Nyquist frequency; lo_over_hi = input Nyquist / lower
    Nyquist (down / up, or the ratio resampler's step): a stop-band tone has to exist in the input"""
    return PASS_TONES, tuple(f for f in STOP_TONES if f < lo_over_hi)


# ---- the operations ----------------------------------------------------------------------------------------------------------
def polyphase(x, up, down, h, half, ms, dtype=np.float64):
    """y[m] = sum_k x[k] h[m down + half - k up] for the outputs ``ms``, x = 0 outside 0 .. len(x) - 1, h = 0 outside
    0 .. 2 half; products and the running sum (ascending k) in ``dtype``"""
    dtype = np.dtype(dtype).type
    x = np.asarray(x).astype(dtype)
    h = np.asarray(h).astype(dtype)
    assert len(h) == 2 * half + 1
    ms = np.asarray(ms, dtype=np.int64)
    c = ms * down + half                                   # h index of x[0]'s tap
    k_lo = -(-(c - 2 * half) // up)                        # smallest k with c - k up <= 2 half (may be negative)
    acc = np.zeros(len(ms), dtype)
    for o in range(2 * half // up + 1):
        k = k_lo + o
        t = c - k * up
        ok = (k >= 0) & (k < len(x)) & (t >= 0) & (t <= 2 * half)
        prod = (x[np.clip(k, 0, len(x) - 1)] * h[np.clip(t, 0, 2 * half)]).astype(dtype)
        acc = (acc + np.where(ok, prod, dtype(0))).astype(dtype)
    return acc


def ratio(x, step, ms, table, P, Z, dtype=np.float64):
    """y[m] = c sum_j x[j] h(c (m step - j)), c = 1 / step for step > 1 and 1 otherwise, over the j within Z / c of m step;
    h(t) read from the one-sided ``table`` (h(i / P), i = 0 .. P Z) by linear interpolation at |t| P.  The position and the
    table argument are float64 (as in the kernel); the interpolation weight, products and the running sum (ascending j) are
    ``dtype``."""
    dtype = np.dtype(dtype).type
    x = np.asarray(x).astype(dtype)
    tab = np.asarray(table).astype(dtype)
    assert len(tab) == P * Z + 1
    step = float(step)
    c = 1.0 / step if step > 1.0 else 1.0
    pos = np.asarray(ms, dtype=np.float64) * step
    reach = Z / c
    j_lo = np.ceil(pos - reach).astype(np.int64)
    acc = np.zeros(len(pos), dtype)
    for o in range(int(np.floor(2.0 * reach)) + 1):
        j = j_lo + o
        u = np.abs(c * (pos - j)) * P
        ok = (u < P * Z) & (j >= 0) & (j < len(x))
        i = np.minimum(u.astype(np.int64), P * Z - 1)
        f = (u - i).astype(dtype)
        hv = (tab[i] + (f * (tab[i + 1] - tab[i]).astype(dtype)).astype(dtype)).astype(dtype)
        prod = (x[np.clip(j, 0, len(x) - 1)] * hv).astype(dtype)
        acc = (acc + np.where(ok, prod, dtype(0))).astype(dtype)
    return (acc * dtype(c)).astype(dtype)


# ---- tones and their measurement ----------------------------------------------------------------------------------------------
def tone(n, f_cycles_per_sample, phase=TONE_PHASE, amp=TONE_AMP):
    """float64 amp sin(2 pi f k + phase), k = 0 .. n - 1"""
    return amp * np.sin(2.0 * np.pi * ((f_cycles_per_sample * np.arange(n, dtype=np.float64)) % 1.0) + phase)


def fit_matrix(ms, f_out):
    th = 2.0 * np.pi * ((f_out * np.asarray(ms, dtype=np.float64)) % 1.0)
    return np.stack([np.sin(th), np.cos(th)], 1)


def fit_gain(y, ms, f_out, phase=TONE_PHASE, amp=TONE_AMP):
    """complex gain G of y[ms] = Im(G amp e^{i (2 pi f_out m + phase)}) by least squares: |G| is the magnitude response, arg G
    the phase error; the ideal resampler has G = 1.  ``y`` holds the outputs ``ms`` only."""
    (a, b), *_ = np.linalg.lstsq(fit_matrix(ms, f_out), np.asarray(y, dtype=np.float64), rcond=None)
    return complex(a, b) / (amp * np.exp(1j * phase))


def interior(n_out, half, down):
    """the outputs of the rational resampler whose taps all fall on real input: ceil(half / down) + 2 away from both ends"""
    margin = -(-half // down) + 2
    return np.arange(margin, n_out - margin, dtype=np.int64)


def interior_ratio(n_out, step, crossings=116):
    margin = int(ceil(crossings * max(1.0, 1.0 / step))) + 2
    return np.arange(margin, n_out - margin, dtype=np.int64)


def response(h, up, freqs):
    """|sum_n h[n] e^{-2 pi i f n}| / up in float64, f in cycles per sample of the rate the filter runs at.  The sum is taken
    directly (no FFT); n = a B + b splits the exponential into two factors, so that a long filter costs one matrix product."""
    h = np.asarray(h, dtype=np.float64)
    f = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    B = int(ceil(sqrt(len(h))))
    A = -(-len(h) // B)
    H = np.zeros(A * B)
    H[:len(h)] = h
    H = H.reshape(A, B)
    out = np.empty(len(f), dtype=np.complex128)
    for lo in range(0, len(f), 1024):
        fc = f[lo:lo + 1024]
        pb = 2.0 * np.pi * ((fc[None, :] * np.arange(B, dtype=np.float64)[:, None]) % 1.0)
        pa = 2.0 * np.pi * ((fc[None, :] * (B * np.arange(A, dtype=np.float64))[:, None]) % 1.0)
        inner = H @ np.cos(pb) - 1j * (H @ np.sin(pb))               # [A, F]: sum over b
        out[lo:lo + 1024] = (inner * np.exp(-1j * pa)).sum(0)
    return np.abs(out) / up


def db(v):
    """20 log10 v, or None where nothing was measured (no stop-band tone fits below the input's Nyquist frequency)"""
    return None if v is None else 20.0 * np.log10(max(float(v), 1e-300))


# ---- the tone cases, shared by the CPU and the device tests -----------------------------------------------------------------
def _tones(n_in, ms, nyq_in, out_per_in, lo_over_hi, run):
    """run(x fp32, ms) -> the outputs ``ms``.  -> (worst |G - 1| over the pass-band tones, worst stop-band |y| / amplitude or
    None without a stop-band tone, worst condition number of the fit); nyq_in: the lower Nyquist frequency in cycles per
    input sample, out_per_in: output frequency / input frequency (cycles per sample each)"""
    passes, stops = tone_fractions(lo_over_hi)
    g_err, s_max, cond = 0.0, None, 0.0
    for frac in passes:
        f_in = frac * nyq_in
        y = run(tone(n_in, f_in).astype(np.float32), ms)
        g_err = max(g_err, abs(fit_gain(y, ms, f_in * out_per_in) - 1.0))
        cond = max(cond, float(np.linalg.cond(fit_matrix(ms, f_in * out_per_in))))
    for frac in stops:
        y = run(tone(n_in, frac * nyq_in).astype(np.float32), ms)
        s_max = max(s_max or 0.0, float(np.max(np.abs(y))) / TONE_AMP)
    return g_err, s_max, cond


def rational_tones(up, down, half, n_out, run):
    ms = interior(n_out, half, down)
    assert len(ms) > 0.9 * n_out
    return _tones(n_in_for(n_out, up, down), ms, 0.5 * min(1.0, up / down), down / up, down / up, run)


def ratio_tones(step, run, crossings=116):
    n_out = int(RATIO_N_IN / step)
    ms = interior_ratio(n_out, step, crossings)
    assert len(ms) > 0.9 * n_out
    return _tones(RATIO_N_IN, ms, 0.5 * min(1.0, 1.0 / step), step, step, run)
