"""Numpy twin of csrc/stretch.hip, written from the contract in include/beat_this_amd.h (bt_stretch, bt_resample_ratio):
the phase-vocoder time stretch with identity phase locking and the arbitrary-ratio Kaiser-sinc resampler.

``dtype=np.float64`` is the reference the device is held to.  ``dtype=np.float32`` is the same algorithm with every
floating-point value in float32 (window, FFTs, magnitudes, phases, synthesis, overlap-add); its distance from the fp64
mode is the yardstick ``e_ref`` of the tests (ten times the reference's own fp32 error).  The phase
arithmetic is uint32 in both modes, and the positions of the resampler are fp64 in both, as the contract demands.
"""
import numpy as np
import scipy.fft

N_FFT, HS, BINS = 2048, 512, 1025


def out_len(n_in, L):
    return int(np.floor(n_in * float(L) + 0.5))


def n_frames(m_out):
    return -(-m_out // HS) + 1


def _window(dtype):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dtype)


def _frames(x, centres, win):
    """windowed frames centred at ``centres`` (zero outside the signal): (len(centres), 2048)"""
    idx = centres[:, None] - N_FFT // 2 + np.arange(N_FFT)[None, :]
    ok = (idx >= 0) & (idx < len(x))
    return np.where(ok, x[np.clip(idx, 0, len(x) - 1)], 0).astype(win.dtype) * win[None, :]


def _q(z, dtype):
    """phase in 32-bit fixed-point turns, q(0) = 0"""
    turns = np.arctan2(z.imag.astype(dtype), z.real.astype(dtype)) * dtype(1.0 / (2.0 * np.pi))
    q = np.rint(turns.astype(dtype) * dtype(4294967296.0)).astype(np.int64)
    q[(z.real == 0) & (z.imag == 0)] = 0
    return (q & 0xFFFFFFFF).astype(np.uint32)


def peaks_of(mag):
    """boolean (frames, bins): the peak rule of the contract"""
    m = mag
    pk = m > 0
    pk[:, 1:] &= m[:, 1:] > m[:, :-1]
    pk[:, 2:] &= m[:, 2:] > m[:, :-2]
    pk[:, :-1] &= m[:, :-1] >= m[:, 1:]
    pk[:, :-2] &= m[:, :-2] >= m[:, 2:]
    return pk


def owners_of(pk):
    """(frames, bins) int: the peak that owns every bin (itself in a frame without a peak)"""
    F, K = pk.shape
    k = np.arange(K)
    own = np.tile(k, (F, 1))
    for n in range(F):
        p = np.nonzero(pk[n])[0]
        if len(p) == 0:
            continue
        j = np.searchsorted(p, k, side="left")            # first peak >= k
        lo = p[np.clip(j - 1, 0, len(p) - 1)]
        hi = p[np.clip(j, 0, len(p) - 1)]
        o = np.where(k <= (lo + hi) // 2, lo, hi)
        o = np.where(j == 0, p[0], o)
        o = np.where(j == len(p), p[-1], o)
        own[n] = o
    return own


def analysis(x, L, dtype=np.float64):
    """-> mag (F, 1025) dtype, q1 (F, 1025) uint32, d (F, 1025) uint32 (d[0] = q1[0]), M"""
    dtype = np.dtype(dtype).type
    x = np.asarray(x, dtype=np.float32)
    M = out_len(len(x), L)
    F = n_frames(M)
    a = np.floor(np.arange(F, dtype=np.float64) * HS / float(L) + 0.5).astype(np.int64)
    win = _window(dtype)
    X1 = scipy.fft.rfft(_frames(x, a, win), axis=1)
    X0 = scipy.fft.rfft(_frames(x, a - HS, win), axis=1)
    assert X1.dtype == (np.complex64 if dtype is np.float32 else np.complex128)
    mag = np.sqrt(X1.real * X1.real + X1.imag * X1.imag).astype(dtype)
    q1, q0 = _q(X1, dtype), _q(X0, dtype)
    d = q1 - q0
    d[0] = q1[0]
    return mag, q1, d, M


def stretch(x, L, dtype=np.float64, details=False):
    """x (N,) -> (floor(N L + 0.5),) ``dtype``"""
    if not (0.5 <= L <= 2.0):
        raise ValueError("length factor outside [0.5, 2]")
    dtype = np.dtype(dtype).type
    mag, q1, d, M = analysis(x, L, dtype)
    F = mag.shape[0]
    S = np.cumsum(d.astype(np.uint64), axis=0).astype(np.uint32)          # (mod 2^32: uint64 wraps consistently)
    own = owners_of(peaks_of(mag.copy()))
    rows = np.arange(F)[:, None]
    phi = S[rows, own] + q1 - q1[rows, own]                                # uint32 arithmetic
    ang = phi.astype(np.int32).astype(dtype) * dtype(2.0 ** -31) * dtype(np.pi)
    Y = (mag * np.cos(ang)).astype(dtype) + 1j * (mag * np.sin(ang)).astype(dtype)
    Y[:, 0] = Y[:, 0].real
    Y[:, -1] = Y[:, -1].real
    Y = Y.astype(np.complex64 if dtype is np.float32 else np.complex128)
    win = _window(dtype)
    y = (scipy.fft.irfft(Y, n=N_FFT, axis=1).astype(dtype) * win[None, :]).astype(dtype)
    w2 = (win * win).astype(dtype)
    out = np.zeros(M, dtype)
    norm = np.zeros(M, dtype)
    m = np.arange(M)
    top = (m + N_FFT // 2) // HS
    for j in (3, 2, 1, 0):                                                 # ascending frame index
        n = top - j
        i = m + N_FFT // 2 - n * HS
        ok = (n >= 0) & (n < F)
        nn = np.clip(n, 0, F - 1)
        out = (out + np.where(ok, y[nn, i], 0).astype(dtype)).astype(dtype)
        norm = (norm + np.where(ok, w2[i], 0).astype(dtype)).astype(dtype)
    res = (out / norm).astype(dtype)
    if details:
        return res, dict(mag=mag, q1=q1, S=S, own=own)
    return res


# ---- the resampler ---------------------------------------------------------------------------------------------------
def resample_ratio(x, step, n_out, table, taps_per_crossing, crossings, dtype=np.float64):
    """y[m] = c sum_j x[j] h(c (m step - j)), c = min(1, 1 / step); h read from ``table`` (one side, h(i / P) for
    i = 0 .. P Z) by linear interpolation; positions in fp64; taps in ascending j"""
    dtype = np.dtype(dtype).type
    x = np.asarray(x, dtype=np.float32)
    P, Z = int(taps_per_crossing), int(crossings)
    tab = np.asarray(table, dtype=np.float32)
    assert len(tab) == P * Z + 1
    step = float(step)
    c = min(1.0, 1.0 / step)
    pos = np.arange(n_out, dtype=np.float64) * step
    reach = Z / c
    j_lo = np.ceil(pos - reach).astype(np.int64)
    n_taps = int(np.floor(2 * reach)) + 1
    acc = np.zeros(n_out, dtype)
    for o in range(n_taps):
        j = j_lo + o
        u = np.abs(c * (pos - j)) * P
        inside = (u < P * Z) & (j >= 0) & (j < len(x))
        u = np.minimum(u, P * Z - 0.5)
        i = np.floor(u).astype(np.int64)
        f = (u - i).astype(dtype)
        h = (tab[i].astype(dtype) + f * (tab[i + 1].astype(dtype) - tab[i].astype(dtype))).astype(dtype)
        xv = np.where(inside, x[np.clip(j, 0, len(x) - 1)], 0).astype(dtype)
        acc = (acc + (xv * h).astype(dtype)).astype(dtype)
    return (acc * dtype(c)).astype(dtype)


def resample_rational(x, up, down, h, half, n_out):
    """fp64 twin of the existing rational resampler (bt_resample): y[m] = sum_j x[j] h[m down - j up + half]"""
    x = np.asarray(x, dtype=np.float64)
    m = np.arange(n_out, dtype=np.int64)
    acc = np.zeros(n_out)
    j_lo = -(-(m * down - half) // up)
    n_taps = (2 * half) // up + 1
    for o in range(n_taps):
        j = j_lo + o
        t = m * down - j * up + half
        ok = (t >= 0) & (t <= 2 * half) & (j >= 0) & (j < len(x))
        acc += np.where(ok, x[np.clip(j, 0, len(x) - 1)] * h[np.clip(t, 0, 2 * half)], 0)
    return acc


def pitch_shift(x, semitones, table, taps_per_crossing, crossings, dtype=np.float64):
    r = 2.0 ** (semitones / 12.0)
    y = stretch(x, r, dtype)
    return resample_ratio(y, r, len(x), table, taps_per_crossing, crossings, dtype)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- signals and properties shared by the CPU and the GPU tests ------------------------------------------------------------
SR = 44100
SINE_HZ = 1000.0            # 46.44 bins of 44100 / 2048 Hz: neither on a bin nor half-way between two
CLICKS = (5000, 14000, 23000)


def sine(n, f=SINE_HZ):
    return (0.5 * np.sin(2 * np.pi * f * np.arange(n) / SR)).astype(np.float32)


def click_train(n=30000):
    x = np.zeros(n, np.float32)
    x[list(CLICKS)] = 0.8
    return x


def peak_bin(y):
    return int(np.argmax(np.abs(np.fft.rfft(np.asarray(y, np.float64)))))


def assert_sine_stretched(y, n_in, L):
    """the length is floor(N L + 0.5) and the largest bin of a whole-signal FFT is within one bin of the sine's"""
    assert len(y) == int(np.floor(n_in * L + 0.5))
    assert abs(peak_bin(y) - SINE_HZ * len(y) / SR) <= 1.0


def assert_sine_shifted(y, n_in, semitones):
    assert len(y) == n_in
    assert abs(peak_bin(y) - SINE_HZ * 2.0 ** (semitones / 12.0) * n_in / SR) <= 1.0


def assert_clicks_confined(y, L):
    """every sample farther than (n_fft / 2) (1 + L) from every stretched click position is exactly zero: a frame whose
    analysis window holds no click has magnitudes of 0 and synthesises zeros"""
    m = np.arange(len(y))
    far = np.ones(len(y), bool)
    for c in CLICKS:
        far &= np.abs(m - c * L) > (N_FFT // 2) * (1 + L)
    assert far.sum() > 0
    assert np.all(np.asarray(y)[far] == 0)


def click_centroid_offsets(y, L):
    """per click: energy centroid of the output around c L, minus c L (samples)"""
    y = np.asarray(y, np.float64)
    out = []
    for c in CLICKS:
        lo, hi = max(0, int(c * L - 3100)), min(len(y), int(c * L + 3100))
        e = y[lo:hi] ** 2
        out.append(float((np.arange(lo, hi) * e).sum() / e.sum() - c * L))
    return out


def test_signal(n, seed, sr=44100):
    """a few off-bin sinusoids + a click train + noise 40 dB below the sinusoids' power, fp32, peak below 1"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = np.zeros(n)
    for f, a in ((233.7, 0.30), (1012.3, 0.22), (3307.9, 0.15), (7411.1, 0.08)):
        x += a * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    sig_rms = np.sqrt(np.mean(x * x)) if n else 1.0
    x[int(rng.integers(100, 600))::4801] += 0.2
    x += rng.standard_normal(n) * sig_rms * 0.01
    return x.astype(np.float32)
