"""The host twin of the PCM decoder (bt_pcm_decode_host, csrc/pcm.hip) against what the file path computes today: the
float64 signal of ``load_audio``, numpy's channel mean and the fp32 conversion -- on the raw 32-bit patterns.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import wav_cases as W


def _lib():
    from beat_this_amd import _lib as L

    L.build()
    return L


def host_decode(L, raw: bytes, offset: int, fmt: str, channels: int, n_frames: int) -> np.ndarray:
    """bt_pcm_decode_host on the payload at ``offset`` of ``raw`` (so at whatever alignment the file gives it)"""
    buf = np.frombuffer(raw, dtype=np.uint8)
    out = np.full(n_frames + 2, 123.0, dtype=np.float32)   # (one float on each side must stay)
    rc = L.lib().bt_pcm_decode_host(buf.ctypes.data + offset, W.FORMATS.index(fmt), channels, n_frames, out.ctypes.data + 4)
    L.check(rc)
    assert out[0] == 123.0 and out[-1] == 123.0
    return out[1:-1].copy()


def todays_waveform(path) -> np.ndarray:
    from beat_this_amd.preprocessing import load_audio

    sig, _ = load_audio(path)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(sig.mean(1) if sig.ndim == 2 else sig, dtype=np.float32)


@pytest.mark.parametrize("fmt,channels", W.channel_grid())
def test_host_twin_matches_load_audio_and_the_numpy_mean(fmt, channels, tmp_path):
    from beat_this_amd import wav

    L = _lib()
    variants = list(W.EXTRA_VARIANTS.values())
    for k, n in enumerate(W.FRAME_COUNTS):
        s = W.samples(fmt, channels, n, seed=k)
        path = W.write_wav(tmp_path / f"{fmt}_{channels}_{n}.wav", fmt, s, **variants[k % len(variants)])
        info = wav.probe(path)
        assert info is not None and (info.format, info.channels, info.n_frames) == (W.FORMATS.index(fmt), channels, n)
        got = host_decode(L, path.read_bytes(), info.data_offset, fmt, channels, n)
        want = todays_waveform(path)
        assert W.same_bits(got, want) is None, (fmt, channels, n, W.same_bits(got, want))
        assert W.same_bits(W.numpy_reference(fmt, s), want) is None   # (the sample-level reference the GPU tests share)


def test_sample_sets_reach_their_edge_cases():
    """the sets hold what they promise: integer extremes and sums beyond 24 bits, float specials, a summation-order case"""
    for fmt in ("s24", "s32"):
        for ch in (2, 3, 6, 8):
            s = W.int_samples(fmt, ch, 64)
            lo, hi = W.INT_RANGE[fmt]
            assert (s == lo).any() and (s == hi).any() and (s == 0).any() and (s == -1).any()
            assert np.abs(s.sum(1)).max() > (hi + 1) * ch * 0.99 and np.abs(s.sum(1)).max() >= 2 ** 24
    for fmt in ("f32", "f64"):
        for ch in (3, 7):
            s = W.float_samples(fmt, ch, 4099).astype(np.float64)
            assert np.isnan(s).any() and np.isposinf(s).any() and np.isneginf(s).any() and np.signbit(s[s == 0]).any()
            ref = W.numpy_reference(fmt, s.astype(np.float32 if fmt == "f32" else np.float64))
            with np.errstate(all="ignore"):
                rev = np.ascontiguousarray(s[:, ::-1]).mean(1).astype(np.float32)     # the same sum, right to left
                sub = np.abs(ref[np.isfinite(ref)])
            assert W.same_bits(rev, ref) is not None, "the summation order does not show in this sample set"
            assert ((sub > 0) & (sub < np.finfo(np.float32).tiny)).any(), "no fp32 subnormal result"
    s = W.float_samples("f64", 1, 64)
    ref = W.numpy_reference("f64", s)
    assert (np.abs(ref) == np.finfo(np.float32).max).any() and np.isinf(ref[np.isfinite(s[:, 0])]).any()


def test_zero_sign_is_numpys():
    """-0.0 in every channel: a mono file keeps it, a channel mean (numpy's sum starts at +0.0) gives +0.0"""
    L = _lib()
    for fmt in ("f32", "f64"):
        for ch in (1, 2, 7):
            s = np.full((5, ch), -0.0)
            got = host_decode(L, W.payload(fmt, s), 0, fmt, ch, 5)
            assert np.signbit(got).all() if ch == 1 else not np.signbit(got).any()
            assert W.same_bits(got, W.numpy_reference(fmt, s)) is None


def test_argument_errors():
    L = _lib()
    lib = L.lib()
    src = np.zeros(256, dtype=np.uint8)
    out = np.zeros(16, dtype=np.float32)
    s, o = src.ctypes.data, out.ctypes.data
    assert lib.bt_pcm_decode_host(s, 1, 2, 4, o) == L.BT_OK
    assert lib.bt_pcm_decode_host(s, 1, 2, 0, o) == L.BT_OK             # a track of 0 frames is legal
    for bad in [(None, 1, 2, 4, o), (s, 1, 2, 4, None), (s, -1, 2, 4, o), (s, 6, 2, 4, o), (s, 1, 0, 4, o), (s, 1, 9, 4, o),
                (s, 3, 9, 4, o), (s, 4, 8, 4, o), (s, 5, 8, 4, o), (s, 1, 2, -1, o)]:
        assert lib.bt_pcm_decode_host(*bad) == L.BT_ERR_ARG, bad
        with pytest.raises(ValueError):
            L.check(L.BT_ERR_ARG)
    assert lib.bt_pcm_decode_host(s, 3, 8, 4, o) == L.BT_OK             # 8 channels: the integer formats only
    # the device entry points refuse the same things before any launch (no GPU is touched: this runs without one)
    for bad in [(None, None, 1, 2, 4, o), (None, s, 1, 2, 4, None), (None, s, 6, 2, 4, o), (None, s, -1, 2, 4, o),
                (None, s, 1, 0, 4, o), (None, s, 1, 9, 4, o), (None, s, 4, 8, 4, o), (None, s, 1, 2, -1, o)]:
        assert lib.bt_pcm_decode(*bad) == L.BT_ERR_ARG, bad
    for bad in [(None, None, 1, 4), (None, s, -1, 4), (None, s, 1, -4), (None, s, L.PCM_MAX_TRACKS + 1, 4)]:
        assert lib.bt_pcm_decode_batch(*bad) == L.BT_ERR_ARG, bad
    assert C.sizeof(L.PcmSpan) == 32
