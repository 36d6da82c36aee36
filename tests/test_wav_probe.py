"""wav.probe: the header walk of the device decode route.  What it accepts, scipy.io.wavfile reads with the same offset,
frame count and sample type; everything else is None (= "use load_audio as before").  No GPU needed."""
import struct
import warnings

import numpy as np
import pytest

import wav_cases as W

SCIPY_DTYPE = dict(u8=np.uint8, s16=np.int16, s24=np.int32, s32=np.int32, f32=np.float32, f64=np.float64)


def _scipy(path):
    from scipy.io import wavfile

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (WavFileWarning: chunks it does not know)
        return wavfile.read(str(path))


@pytest.mark.parametrize("variant", sorted(W.EXTRA_VARIANTS))
@pytest.mark.parametrize("fmt", W.FORMATS)
def test_probe_agrees_with_scipy(fmt, variant, tmp_path):
    from beat_this_amd import wav

    kw = W.EXTRA_VARIANTS[variant]
    for channels, n, rate in ((1, 37, 22050), (2, 100, 44100), (3, 5, 48000), (7, 64, 8000)):
        s = W.samples(fmt, channels, n, seed=3)
        path = W.write_wav(tmp_path / f"{channels}.wav", fmt, s, rate=rate, **kw)
        info = wav.probe(path)
        assert info == wav.PcmInfo(W.FORMATS.index(fmt), channels, rate, W.data_offset(fmt, **kw), n)
        assert info.frame_bytes == channels * W.SAMPLE_BYTES[fmt] and info.data_bytes == n * info.frame_bytes
        sr, data = _scipy(path)
        assert sr == info.sample_rate and data.dtype == SCIPY_DTYPE[fmt]
        assert data.shape == ((n,) if channels == 1 else (n, channels))
        # the bytes at the probed offset ARE scipy's samples
        raw = path.read_bytes()[info.data_offset: info.data_offset + info.data_bytes]
        assert raw == W.payload(fmt, s)
        mine = np.frombuffer(raw, dtype=np.uint8)
        if fmt == "s24":
            mine = np.concatenate([np.zeros((n * channels, 1), np.uint8), mine.reshape(-1, 3)], 1).reshape(-1).view("<i4")
        else:
            mine = mine.view(np.dtype(SCIPY_DTYPE[fmt]).newbyteorder("<"))
        assert np.array_equal(mine.view(np.uint8), np.ascontiguousarray(data).reshape(-1).view(np.uint8))
        lo, nbytes, pay = info.raw_span
        assert lo % 16 == 0 and nbytes % 16 == 0 and lo + pay == info.data_offset and pay < 16
        assert lo + nbytes >= info.data_offset + info.data_bytes > lo + nbytes - 16


def test_read_raw_reads_the_windows_unconverted(tmp_path):
    from beat_this_amd import wav

    s = W.samples("s24", 2, 1001, seed=1)
    path = W.write_wav(tmp_path / "a.wav", "s24", s, **W.EXTRA_VARIANTS["odd"], trailer=W.chunk(b"LIST", b"x" * 40))
    info = wav.probe(path)
    lo, nbytes, pay = info.raw_span
    buf = np.full(nbytes + 5, 0xAB, dtype=np.uint8)
    assert wav.read_raw(info, path, buf) == pay
    assert buf[:nbytes].tobytes() == path.read_bytes()[lo: lo + nbytes] and (buf[nbytes:] == 0xAB).all()
    # a file that ends inside the last window: the payload is there, the rest of the buffer is left alone
    path2 = W.write_wav(tmp_path / "b.wav", "s24", s[:7])
    info2 = wav.probe(path2)
    lo, nbytes, pay = info2.raw_span
    buf = np.full(nbytes, 0xAB, dtype=np.uint8)
    assert wav.read_raw(info2, path2, buf) == pay
    assert buf[pay: pay + info2.data_bytes].tobytes() == W.payload("s24", s[:7])
    with pytest.raises(ValueError):
        wav.read_raw(info, path, np.zeros(16, dtype=np.uint8))
    path.write_bytes(path.read_bytes()[: info.data_offset + 100])   # the file shrank after the probe
    with pytest.raises(OSError):
        wav.read_raw(info, path, np.zeros(info.raw_span[1], dtype=np.uint8))


def _declined(tmp_path):
    s16 = W.samples("s16", 2, 50)
    good = W.wav_bytes("s16", s16)
    off = W.data_offset("s16")
    cases = {
        "not_riff": b"JUNK" + good[4:],
        "not_wave": good[:8] + b"AVI " + good[12:],
        "rifx": W.wav_bytes("s16", s16, magic=b"RIFX"),
        "rf64": W.wav_bytes("s16", s16, magic=b"RF64"),
        "bw64": W.wav_bytes("s16", s16, magic=b"BW64"),
        "tag_adpcm": W.wav_bytes("s16", s16, tag=2),
        "tag_alaw": W.wav_bytes("u8", W.samples("u8", 1, 50), tag=6),
        "tag_mp3": W.wav_bytes("s16", s16, tag=0x55),
        "extensible_other_guid": W.wav_bytes("s16", s16, extensible=True).replace(W.GUID_TAIL, b"\1" + W.GUID_TAIL[1:]),
        "extensible_tag_adpcm": W.wav_bytes("s16", s16, extensible=True, tag=2),
        "valid_bits_12_of_16": W.wav_bytes("s16", s16, extensible=True, valid_bits=12),
        "valid_bits_20_of_24": W.wav_bytes("s24", W.samples("s24", 2, 50), extensible=True, valid_bits=20),
        "valid_bits_7_of_8": W.wav_bytes("u8", W.samples("u8", 1, 50), extensible=True, valid_bits=7),
        "int_9_channels": W.wav_bytes("s16", W.samples("s16", 9, 50)),
        "float_8_channels": W.wav_bytes("f32", W.samples("f32", 8, 50)),
        "data_size_0": W.wav_bytes("s16", s16, data_size=0),
        "data_exceeds_file": W.wav_bytes("s16", s16, data_size=4 * 50 + 4),
        "data_streamed_size": W.wav_bytes("s16", s16, data_size=0xFFFFFFFF),
        "data_not_whole_frames": W.wav_bytes("s16", s16, data_size=4 * 50 - 2),
        "truncated_in_data": good[:off + 77],
        "truncated_in_fmt": good[:30],
        "truncated_before_data": good[:off - 8],
        "ten_bytes": good[:10],
        "empty": b"",
        "no_fmt": good[:12] + good[off - 8:],
    }
    # containers the decoder does not have: 12-bit in 16 (a block align that does not fit), 16-bit float, 48-bit
    for name, bits in (("bits_12", 12), ("bits_48", 48)):
        b = bytearray(good)
        struct.pack_into("<H", b, 34, bits)
        cases[name] = bytes(b)
    b = bytearray(W.wav_bytes("s16", s16, tag=3))   # IEEE float, 16 bits
    cases["float_16"] = bytes(b)
    b = bytearray(good)
    struct.pack_into("<H", b, 32, 6)                # block align 6 for 2 x 16 bits
    cases["block_align"] = bytes(b)
    paths = {}
    for name, data in cases.items():
        p = tmp_path / f"{name}.wav"
        p.write_bytes(data)
        paths[name] = p
    (tmp_path / "dir.wav").mkdir()
    paths["directory"] = tmp_path / "dir.wav"
    paths["missing"] = tmp_path / "nothing_here.wav"
    return paths


def test_probe_declines_what_it_does_not_fully_recognise(tmp_path):
    from beat_this_amd import wav

    good = W.write_wav(tmp_path / "good.wav", "s16", W.samples("s16", 2, 50))
    assert wav.probe(good) is not None and wav.probe(str(good)) is not None
    for name, p in _declined(tmp_path).items():
        assert wav.probe(p) is None, name
    assert wav.probe(None) is None and wav.probe(12.5) is None   # never raises
