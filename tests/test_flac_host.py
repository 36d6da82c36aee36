"""The host side of the FLAC decoder (csrc/flac.hip over csrc/flac_bits.h): bt_flac_probe_host, bt_flac_decode_host and
``beat_this_amd.flac.probe`` on the case table of flac_cases.py -- the writer's integers, the MD5 of STREAMINFO, the numpy
statement of the contract, the WAV identity, the statuses of the rejected streams -- and the parser under sanitizers as a
stand-alone program.  No GPU needed."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import flac_cases as F
import wav_cases as W
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "flac_rfc_example1.flac")
SENTINEL = 123.0


def _lib():
    from beat_this_amd import _lib as L

    L.build()
    return L


def c_probe(L, data: bytes):
    info = L.FlacInfo()
    buf = np.frombuffer(data, dtype=np.uint8)
    return info if L.lib().bt_flac_probe_host(buf.ctypes.data, len(data), C.byref(info)) == 1 else None


def host_decode(L, data: bytes, info=None, want_pcm=True):
    """bt_flac_decode_host -> (status, fp32 output with a sentinel float on each side still in place, interleaved integers)"""
    info = info or c_probe(L, data)
    assert info is not None
    buf = np.frombuffer(data, dtype=np.uint8)
    n, ch = info.total_samples, info.channels
    out = np.full(n + 2, SENTINEL, dtype=np.float32)
    pcm = np.full((n, ch), -7, dtype=np.int32)
    st = L.FlacStatus()
    L.check(L.lib().bt_flac_decode_host(buf.ctypes.data, C.byref(info), out.ctypes.data + 4, pcm.ctypes.data if want_pcm else None, C.byref(st)))
    assert out[0] == SENTINEL and out[-1] == SENTINEL
    return st, out[1:-1], pcm


def test_known_answer_file():
    """RFC 9639's one-frame example: two verbatim subframes with 2 and 4 wasted bits"""
    L = _lib()
    data = open(GOLDEN, "rb").read()
    assert hashlib.sha256(data).hexdigest()[:8] and len(data) == 57
    info = c_probe(L, data)
    assert (info.sample_rate, info.channels, info.bps, info.total_samples, info.first_frame, info.blocking) == (44100, 2, 16, 1, 42, 0)
    st, out, pcm = host_decode(L, data)
    assert (st.code, st.n_frames, st.n_samples, st.where) == (F.OK, 1, 1, 57)
    assert pcm.tolist() == [[25588, 10416]]
    assert hashlib.md5(pcm.astype("<i2").tobytes()).digest() == bytes(info.md5)
    assert out.view(np.uint32)[0] == np.float32((25588 + 10416) / 32768 / 2).view(np.uint32)
    assert F.crc8(data[42:48]) == 0xBF == data[48] and F.crc16(data[42:55]) == 0xAA9A


@pytest.mark.parametrize("case", F.valid(), ids=lambda c: c.name)
def test_every_case_decodes_to_the_writers_integers(case):
    L = _lib()
    info = c_probe(L, case.data)
    assert info is not None
    assert (info.sample_rate, info.channels, info.bps, info.total_samples, info.first_frame, info.n_bytes) == \
        (case.rate, case.channels, case.bps, len(case.pcm), case.first_frame, len(case.data))
    st, out, pcm = host_decode(L, case.data, info)
    assert (st.code, st.n_frames, st.n_samples) == (F.OK, case.n_frames, len(case.pcm)), (st.code, st.n_frames, st.n_samples, st.where)
    assert st.where == case.audio_end
    assert np.array_equal(pcm, case.pcm)
    assert F.pcm_md5(pcm, case.bps) == bytes(info.md5)
    assert W.same_bits(out, case.reference()) is None, W.same_bits(out, case.reference())
    # the output does not depend on whether the integers were asked for
    _, out2, _ = host_decode(L, case.data, info, want_pcm=False)
    assert np.array_equal(out2.view(np.uint32), out.view(np.uint32))
    # a FLAC file and a WAV file that hold the same integers decode to the same bits
    fmt = {8: "u8", 16: "s16", 24: "s24"}.get(case.bps)
    if fmt:
        raw = W.payload(fmt, case.pcm + (128 if fmt == "u8" else 0))
        wav = np.empty(len(case.pcm), dtype=np.float32)
        buf = np.frombuffer(raw, dtype=np.uint8)
        L.check(L.lib().bt_pcm_decode_host(buf.ctypes.data, W.FORMATS.index(fmt), case.channels, len(case.pcm), wav.ctypes.data))
        assert W.same_bits(out, wav) is None


@pytest.mark.parametrize("case", F.rejected(), ids=lambda c: c.name)
def test_rejected_cases_return_their_status_and_write_nothing(case):
    L = _lib()
    st, out, pcm = host_decode(L, case.data)
    assert st.code == case.status, (st.code, st.n_frames, st.where)
    assert st.where == case.where
    if getattr(case, "good_frames", None) is not None:
        assert (st.n_frames, st.n_samples) == (case.good_frames, 192 * case.good_frames)
    assert (out == SENTINEL).all() and (pcm == -7).all()


def test_the_table_holds_what_it_promises():
    names = {c.name for c in F.valid()}
    assert {"types", "lpc_grid", "wide_accumulator", "side_25_bits", "rice", "escapes", "block_sizes", "block_65535", "many_frames",
            "metadata", "id3_and_trailing", "frame_as_payload", "good_crc8_bad_crc16"} <= names
    by = {c.name: c for c in F.valid()}
    assert by["many_frames"].n_frames == 2100 and by["block_65535"].pcm.shape[0] == 65535 + 7
    assert max(abs(by["side_25_bits"].pcm[:, 0] - by["side_25_bits"].pcm[:, 1])) == (1 << 24) - 1     # a signed side of 25 bits
    # the payload of the false-frame case really is a frame: the parser accepts it where it lies
    c = by["frame_as_payload"]
    inner = F.write_frame(F.tone(40, 1, 8, 40), 8, 8000, 1, False, subframes=[dict(type="fixed", order=1)])
    assert c.data.count(inner) == 1 and c.data.index(inner) > c.first_frame
    assert len(F.mutations()) > 100


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return p


def test_python_probe_agrees_with_the_library_and_declines_the_rest(tmp_path):
    from beat_this_amd import flac

    L = _lib()
    for case in F.valid() + F.rejected():
        got = flac.probe(_write(tmp_path, "x.flac", case.data))
        want = c_probe(L, case.data)
        assert got is not None and want is not None, case.name
        for k in ("sample_rate", "channels", "bps", "blocking", "min_block", "max_block", "total_samples", "first_frame", "n_bytes"):
            assert getattr(got, k) == getattr(want, k), (case.name, k)
        assert got.md5 == bytes(want.md5) and bytes(got.c_info()) == bytes(want)
    md5 = bytes(16)
    frame = F.write_frame(np.zeros((16, 1)), 16, 44100, 0, False)

    def stream(info, head=b"fLaC"):
        return head + F.metadata([(0, info)]) + frame
    declined = {
        "ogg": b"OggS\0\2" + bytes(20) + b"\x7fFLAC\1\0\0\1" + stream(F.streaminfo(16, 16, 44100, 1, 16, 16, md5)),
        "total_0": stream(F.streaminfo(16, 16, 44100, 1, 16, 0, md5)),
        "bps_32": stream(F.streaminfo(16, 16, 44100, 1, 32, 16, md5)),
        "bps_25": stream(F.streaminfo(16, 16, 44100, 1, 25, 16, md5)),
        "no_marker": stream(F.streaminfo(16, 16, 44100, 1, 16, 16, md5), head=b"fLaX"),
        "no_sync": b"fLaC" + F.metadata([(0, F.streaminfo(16, 16, 44100, 1, 16, 16, md5))]) + b"\0\0\0\0",
        "metadata_past_the_end": b"fLaC" + F.metadata([(0, F.streaminfo(16, 16, 44100, 1, 16, 16, md5)), (1, bytes(50))])[:-20],
        "streaminfo_not_first": b"fLaC" + F.metadata([(1, bytes(8)), (0, F.streaminfo(16, 16, 44100, 1, 16, 16, md5))]) + frame,
        "empty": b"",
    }
    for name, data in declined.items():
        assert flac.probe(_write(tmp_path, name + ".flac", data)) is None, name
        assert c_probe(L, data) is None, name
    ok = stream(F.streaminfo(16, 16, 44100, 1, 16, 16, md5))
    assert flac.probe(_write(tmp_path, "ok.flac", ok)) is not None and c_probe(L, ok) is not None
    assert flac.probe(tmp_path / "missing.flac") is None
    # no WAV file is taken for a FLAC stream
    for k, (fmt, ch) in enumerate(W.channel_grid()):
        p = W.write_wav(tmp_path / "w.wav", fmt, W.samples(fmt, ch, 65, seed=k), **list(W.EXTRA_VARIANTS.values())[k % 5])
        assert flac.probe(p) is None


def test_argument_errors_and_the_workspace_query():
    L = _lib()
    lib = L.lib()
    case = F.valid()[0]
    info = c_probe(L, case.data)
    buf = np.frombuffer(case.data, dtype=np.uint8)
    out = np.zeros(len(case.pcm), dtype=np.float32)
    st = L.FlacStatus()
    s, o = buf.ctypes.data, out.ctypes.data
    assert lib.bt_flac_decode_host(s, C.byref(info), o, None, C.byref(st)) == L.BT_OK
    for bad in [(None, C.byref(info), o, None, C.byref(st)), (s, None, o, None, C.byref(st)), (s, C.byref(info), None, None, C.byref(st)),
                (s, C.byref(info), o, None, None)]:
        assert lib.bt_flac_decode_host(*bad) == L.BT_ERR_ARG
    ws = lib.bt_flac_workspace_bytes(C.byref(info))
    assert ws >= 4 * info.channels * info.total_samples + 32 * ((info.n_bytes - info.first_frame) // 8 + 64) and ws % 16 == 0
    for field, value in (("channels", 9), ("bps", 25), ("bps", 3), ("total_samples", 0), ("first_frame", info.n_bytes), ("max_block", 0),
                         ("n_bytes", 1 << 31), ("total_samples", 1 << 31)):
        bad = L.FlacInfo.from_buffer_copy(bytes(info))
        setattr(bad, field, value)
        assert lib.bt_flac_workspace_bytes(C.byref(bad)) == 0, field
        if field != "n_bytes" and value != 1 << 31:
            assert lib.bt_flac_decode_host(s, C.byref(bad), o, None, C.byref(st)) == L.BT_ERR_ARG, field
    assert lib.bt_flac_workspace_bytes(None) == 0
    assert lib.bt_flac_probe_host(None, 10, C.byref(info)) == 0 and lib.bt_flac_probe_host(s, len(case.data), None) == 0
    # the device entry points refuse before any launch (no GPU is touched: this runs without one)
    span = L.FlacSpan(1 << 20, 1 << 21, 1 << 22, ws, 1 << 23, info)
    short = L.FlacSpan(1 << 20, 1 << 21, 1 << 22, ws - 256, 1 << 23, info)
    assert lib.bt_flac_decode_batch(None, C.byref(short), 1 << 24, 1) == L.BT_ERR_WORKSPACE
    assert lib.bt_flac_decode(None, 1 << 20, C.byref(info), 1 << 21, 1 << 22, ws - 256, 1 << 23) == L.BT_ERR_WORKSPACE
    assert lib.bt_flac_decode(None, 1 << 20, C.byref(info), (1 << 21) + 4, 1 << 22, ws, 1 << 23) == L.BT_ERR_ARG
    assert lib.bt_flac_decode(None, None, C.byref(info), 1 << 21, 1 << 22, ws, 1 << 23) == L.BT_ERR_ARG
    assert lib.bt_flac_decode_batch(None, None, 1 << 24, 1) == L.BT_ERR_ARG
    assert lib.bt_flac_decode_batch(None, C.byref(span), 1 << 24, -1) == L.BT_ERR_ARG
    assert lib.bt_flac_decode_batch(None, C.byref(span), 1 << 24, L.FLAC_MAX_TRACKS + 1) == L.BT_ERR_ARG
    assert lib.bt_flac_decode_batch(None, C.byref(span), 1 << 24, 0) == L.BT_OK
    assert (C.sizeof(L.FlacInfo), C.sizeof(L.FlacStatus), C.sizeof(L.FlacSpan)) == (64, 24, 104)


def test_header_binding_and_library_agree_on_the_exports():
    L = _lib()
    header = open(os.path.join(ROOT, "include", "beat_this_amd.h")).read()
    declared = {n for n in re.findall(r"\b(bt_flac_[a-z_0-9]+)\s*\(", header)}
    want = {"bt_flac_probe_host", "bt_flac_decode_host", "bt_flac_workspace_bytes", "bt_flac_decode_batch", "bt_flac_decode"}
    assert declared == want == {n for n in L.EXPORTS if n.startswith("bt_flac_")}
    for n in want:
        assert hasattr(L.lib(), n)
    for name, value in re.findall(r"^#define BT_FLAC_(\w+) (\d+)", header, re.M):
        assert getattr(L, "FLAC_" + name) == int(value), name
    assert "flac.hip" in L.SOURCES and "-ffp-contract=off" in L.FLAGS_BY_SOURCE["flac.hip"] and "flac_bits.h" in L.HEADERS
    assert re.search(r"#define BT_ABI_VERSION 600\b", header)


def test_parser_under_sanitizers(tmp_path):
    """tools/flac_sanitize.cpp -- the shared parser with a main of its own -- built with -fsanitize=address,undefined and run
    as a child process over the whole table: valid, false-frame and rejected cases, seeded byte flips, truncations"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    one = tmp_path / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    if cxx is None or subprocess.run([cxx, *flags, str(one), "-o", str(tmp_path / "one")], capture_output=True).returncode \
            or subprocess.run([str(tmp_path / "one")], capture_output=True).returncode:
        pytest.skip("a one-line program built with -fsanitize=address,undefined does not link and run here")
    exe = tmp_path / "flac_sanitize"
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tools", "flac_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = {}
    for c in F.valid() + F.rejected():
        files[c.name] = c.data
        if len(c.data) < 5000:
            for cut in (1, 2, 3, 7, len(c.data) - c.first_frame - 1, len(c.data) - c.first_frame + 3):
                files[f"{c.name}_cut{cut}"] = c.data[: len(c.data) - cut]
    files.update(F.mutations())
    files["rfc_example"] = open(GOLDEN, "rb").read()
    paths = [str(_write(tmp_path, f"{k:04d}.flac", d)) for k, d in enumerate(files.values())]
    r = subprocess.run([str(exe), *paths], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    assert len(lines) == len(paths)
    status = {name: (int(l[1]), int(l[2])) for name, l in zip(files, lines)}
    for c in F.valid():
        assert status[c.name] == (1, F.OK), c.name
    for c in F.rejected():
        assert status[c.name] == (1, c.status), c.name
