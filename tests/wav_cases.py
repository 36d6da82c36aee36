"""A small WAV writer and the sample sets of the PCM decode tests (test_wav_probe.py, test_pcm_host.py, test_gpu_pcm.py,
test_gpu_files.py): the six sample formats of csrc/pcm.hip, any channel count, optional extra chunks in front of ``data``
(an odd-sized one with its pad byte among them) and the extensible header.  Not a test."""
import struct

import numpy as np

FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64")          # in the order of BT_PCM_*
SAMPLE_BYTES = dict(u8=1, s16=2, s24=3, s32=4, f32=4, f64=8)
INT_RANGE = dict(u8=(0, 255), s16=(-2 ** 15, 2 ** 15 - 1), s24=(-2 ** 23, 2 ** 23 - 1), s32=(-2 ** 31, 2 ** 31 - 1))
CHANNELS = (1, 2, 3, 6, 7)                                   # ... plus 8 for the integer formats
FRAME_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 4099)
GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def channel_grid():
    """(format, channels) of the decode tests: all six formats x {1, 2, 3, 6, 7}, plus 8 for the integer formats"""
    return [(f, c) for f in FORMATS for c in CHANNELS + ((8,) if f in INT_RANGE else ())]


def is_float(fmt):
    return fmt in ("f32", "f64")


def payload(fmt, samples) -> bytes:
    """(frames, channels) samples (integers: the values v of the contract, u8 as 0 .. 255; floats: the samples) -> the
    interleaved little-endian bytes of the data chunk"""
    a = np.asarray(samples)
    if fmt == "u8":
        return a.astype(np.uint8).tobytes()
    if fmt == "s16":
        return a.astype("<i2").tobytes()
    if fmt == "s24":
        return a.astype("<i4").reshape(-1, 1).view(np.uint8)[:, :3].tobytes()
    if fmt == "s32":
        return a.astype("<i4").tobytes()
    return a.astype("<f4" if fmt == "f32" else "<f8").tobytes()


def fmt_chunk(fmt, channels, rate, extensible=False, valid_bits=None, tag=None) -> bytes:
    bits = 8 * SAMPLE_BYTES[fmt]
    align = channels * SAMPLE_BYTES[fmt]
    base_tag = 3 if is_float(fmt) else 1
    if tag is not None:
        base_tag = tag
    if not extensible:
        return struct.pack("<HHIIHH", base_tag, channels, rate, rate * align, align, bits)
    return (struct.pack("<HHIIHH", 0xFFFE, channels, rate, rate * align, align, bits)
            + struct.pack("<HHI", 22, bits if valid_bits is None else valid_bits, (1 << channels) - 1)
            + struct.pack("<H", base_tag) + GUID_TAIL)


def chunk(cid: bytes, body: bytes) -> bytes:
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def wav_bytes(fmt, samples, rate=22050, extra=(), extensible=False, valid_bits=None, tag=None, magic=b"RIFF", form=b"WAVE",
              data_size=None, trailer=b"") -> bytes:
    """A whole file.  ``extra``: (id, body) chunks between ``fmt `` and ``data``; ``data_size``: the size the data chunk CLAIMS
    (default: its real size); ``trailer``: chunks behind ``data``."""
    a = np.asarray(samples)
    a = a.reshape(len(a), -1)
    data = payload(fmt, a)
    body = form + chunk(b"fmt ", fmt_chunk(fmt, a.shape[1], rate, extensible, valid_bits, tag))
    for cid, b in extra:
        body += chunk(cid, b)
    body += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data + (b"\0" if len(data) & 1 else b"")
    body += trailer
    return magic + struct.pack("<I", len(body)) + body


def write_wav(path, fmt, samples, **kw):
    with open(path, "wb") as f:
        f.write(wav_bytes(fmt, samples, **kw))
    return path


def data_offset(fmt, extra=(), extensible=False) -> int:
    """where ``wav_bytes`` puts the first sample"""
    n = 12 + 8 + (40 if extensible else 16)
    for _, b in extra:
        n += 8 + len(b) + (len(b) & 1)
    return n + 8


EXTRA_VARIANTS = {
    "plain": dict(),
    "list": dict(extra=((b"LIST", b"INFOISFT" + struct.pack("<I", 6) + b"tests\0"),)),
    "odd": dict(extra=((b"fact", struct.pack("<I", 7)), (b"junk", b"abcde"))),          # a 5-byte chunk: one pad byte
    "extensible": dict(extensible=True),
    "extensible_odd": dict(extensible=True, extra=((b"bext", b"x" * 13), (b"LIST", b"INFO"))),
}


def int_samples(fmt, channels, n_frames, seed=0):
    """Seeded integers over the format's whole range.  The first frames hold the edge values -- min, min + 1, -1, 0, 1, max
    in every channel, then min and max alternating over the channels -- and a stretch of frames near both ends of the range,
    so that channel sums need more than 24 bits (s24, s32 at 2, 3, 6, 8 channels)."""
    lo, hi = INT_RANGE[fmt]
    mid = 128 if fmt == "u8" else 0
    rng = np.random.default_rng([seed, FORMATS.index(fmt), channels, n_frames])
    a = rng.integers(lo, hi + 1, (n_frames, channels), dtype=np.int64)
    edges = [lo, lo + 1, mid - 1, mid, mid + 1, hi]
    rows = [np.full(channels, e) for e in edges]
    rows.append(np.where(np.arange(channels) % 2 == 0, lo, hi))
    rows.append(np.where(np.arange(channels) % 2 == 0, hi, lo + 1))
    for k in range(8):     # all channels within 2^10 of an end: the sum of C such values has log2(C) more bits than one
        rows.append((hi if k % 2 else lo) + (-1 if k % 2 else 1) * (rng.integers(0, 1024, channels) % (hi - lo + 1)))
    rows = np.array(rows[:n_frames], dtype=np.int64).reshape(-1, channels)
    a[:len(rows)] = np.clip(rows, lo, hi)
    return a


def float_samples(fmt, channels, n_frames, seed=0):
    """Seeded floats whose magnitudes are spread over 16 decades ACROSS the channels of a frame (the summation order shows at
    3 .. 7 channels).  The first frames hold the special values: +-0 (all channels, and mixed), fp32 / fp64 subnormals, values
    whose mean rounds to an fp32 subnormal and to the largest finite fp32, +-inf (alone, and both in a frame), NaN."""
    dt = np.float32 if fmt == "f32" else np.float64
    rng = np.random.default_rng([seed, FORMATS.index(fmt), channels, n_frames])
    a = (rng.standard_normal((n_frames, channels)) * 10.0 ** rng.integers(-8, 9, (n_frames, channels))).astype(dt)
    tiny32, big32 = np.float32(1e-45), np.finfo(np.float32).max
    C = channels
    rows = [np.full(C, -0.0), np.full(C, 0.0), np.where(np.arange(C) % 2 == 0, -0.0, 0.0), np.where(np.arange(C) % 2 == 0, 0.0, -0.0),
            np.full(C, tiny32), np.full(C, -tiny32), np.full(C, np.float32(1.1754942e-38)),                 # fp32 subnormals
            np.full(C, np.float32(3e-39)) * np.arange(1, C + 1), np.full(C, np.float32(-2e-40)) * np.arange(1, C + 1),
            np.full(C, float(big32)), np.full(C, -float(big32)),
            np.where(np.arange(C) == 0, 1.0, -1.0) * 1e-3, np.full(C, 1.0) / 3.0]
    if fmt == "f64":
        rows += [np.full(C, 5e-324), np.full(C, -5e-324), np.full(C, 2.2e-308) / np.arange(1, C + 1),    # fp64 subnormals
                 np.full(C, 1.4e-45 * 0.5), np.full(C, 1.4012984643e-45 * 1.5), np.full(C, -7.006492321624085e-46),   # ties / near-ties at the smallest fp32 subnormal
                 np.full(C, 1.17549435e-38 * 0.999999), np.full(C, 3.4028234663852886e38), np.full(C, 3.4028235e38 * (1 + 2e-8)),
                 np.full(C, 3.40282356779733e38), np.full(C, 1e39), np.full(C, -1e300)]                     # round to max / to inf
    rows += [np.where(np.arange(C) == C - 1, np.inf, 1.0), np.where(np.arange(C) == 0, -np.inf, 1.0),
             np.where(np.arange(C) % 2 == 0, np.inf, -np.inf), np.where(np.arange(C) == C // 2, np.nan, 1.0), np.full(C, np.nan)]
    with np.errstate(over="ignore"):
        rows = np.array(rows[:n_frames], dtype=np.float64).reshape(-1, C).astype(dt)
    if C >= 3:   # a large value, its negative, then small ones: what is left of the small ones depends on the order of the sum
        big = (10.0 ** rng.integers(8, 17, n_frames) * (1 + rng.random(n_frames))).astype(dt)
        sel = np.arange(n_frames) % 8 == 5
        a[sel, 0], a[sel, 1] = big[sel], -big[sel]
    a[:len(rows)] = rows
    return a


def samples(fmt, channels, n_frames, seed=0):
    return (float_samples if is_float(fmt) else int_samples)(fmt, channels, n_frames, seed)


def numpy_reference(fmt, samples_) -> np.ndarray:
    """What ``load_audio`` + the mono mix + the fp32 conversion give for these samples, computed from the samples (not from a
    file): float64 values as scipy's branch of load_audio makes them, numpy's ``mean(1)`` for more than one channel."""
    a = np.asarray(samples_)
    a = a.reshape(len(a), -1)
    if fmt == "u8":
        sig = (a.astype(np.float64) - 128.0) / 128.0
    elif fmt in INT_RANGE:
        sig = a.astype(np.float64) / float(-INT_RANGE[fmt][0])
    else:
        sig = a.astype(np.float64)
    if sig.shape[1] == 1:
        sig = sig[:, 0]
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(sig.mean(1) if sig.ndim == 2 else sig, dtype=np.float32)


def same_bits(got, want):
    """None, or a message: raw 32-bit patterns equal, the sign of zero included; a NaN is compared as a NaN"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return f"shapes {got.shape} != {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.where(gn | wn, gn != wn, got.view(np.uint32) != want.view(np.uint32))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        return (f"{int(bad.sum())} of {bad.size} samples differ, first at {i}: got {got[i]!r} (0x{int(got.view(np.uint32)[i]):08X}), "
                f"want {want[i]!r} (0x{int(want.view(np.uint32)[i]):08X})")
    return None
