"""The PCM decode kernel (csrc/pcm.hip) on the MI355X against its host twin, on the raw 32-bit patterns: every format and
channel count, frame counts around the per-thread (4) and per-workgroup (1024) units, every source alignment 0 .. 15, poisoned
memory around every payload and every output, guard bands around the output buffer.  One ragged launch carries a whole case
(bt_pcm_decode_batch), so a case is a few launches."""
import ctypes as C

import numpy as np
import pytest
import torch

import wav_cases as W
from gpu_util import POISONS, Guarded, assert_intact, dev

pytestmark = pytest.mark.gpu

THREAD, BLOCK = 4, 1024     # BT_PCM_THREAD_FRAMES, BT_PCM_BLOCK_FRAMES
ALIGN_COUNTS = (1, 5, 65, 257, 1025, 4099)      # these frame counts run at all 16 source alignments


def _frame_counts():
    """FRAME_COUNTS, and one value on each side of every multiple of 4 and of 1024 up to two workgroups (and the multiples)"""
    ns = set(W.FRAME_COUNTS)
    for unit in (THREAD, BLOCK):
        for m in range(unit, 2 * BLOCK + 1, unit):
            ns |= {m - 1, m, m + 1}
    return sorted(ns)


def _L():
    from beat_this_amd import _lib

    assert _lib.PCM_THREAD_FRAMES == THREAD and _lib.PCM_BLOCK_FRAMES == BLOCK
    return _lib


def _twin(L, fmt, ch, n, data: bytes) -> np.ndarray:
    out = np.empty(max(n, 1), dtype=np.float32)
    buf = np.frombuffer(data + b"\0", dtype=np.uint8)
    L.check(L.lib().bt_pcm_decode_host(buf.ctypes.data, W.FORMATS.index(fmt), ch, n, out.ctypes.data))
    return out[:n]


class Case:
    """tracks [(fmt, channels, n_frames, source alignment)] laid out for one ragged launch: every payload at its alignment
    inside a slot of one source buffer, with at least 16 bytes of the poison before and after it; every output at a 16-byte
    aligned offset of one guarded buffer, with 4 poisoned floats behind it"""

    def __init__(self, L, tracks, seed=0):
        self.L, self.tracks = L, tracks
        self.data = [W.payload(f, W.samples(f, c, n, seed=seed + k)) if n else b"" for k, (f, c, n, _) in enumerate(tracks)]
        self.want = [_twin(L, f, c, n, d) for (f, c, n, _), d in zip(tracks, self.data)]
        self.src_off, self.out_off = [], []
        s = o = 0
        for (f, c, n, a), d in zip(tracks, self.data):
            s += 16
            self.src_off.append(s + a)
            s = (s + a + len(d) + 15) // 16 * 16 + 16
            self.out_off.append(o)
            o += (n + 3) // 4 * 4 + 4
        self.src_bytes, self.out_floats = s + 16, o

    def source(self, poison):
        host = np.full(self.src_bytes, poison, dtype=np.uint8)
        for off, d in zip(self.src_off, self.data):
            host[off: off + len(d)] = np.frombuffer(d, dtype=np.uint8)
        t = torch.from_numpy(host).to(dev())
        assert t.data_ptr() % 16 == 0
        return t

    def table(self, src, out):
        tab = np.zeros((len(self.tracks), 4), dtype=np.int64)
        for k, (f, c, n, _) in enumerate(self.tracks):
            tab[k] = (src.data_ptr() + self.src_off[k], n, out.ptr() + 4 * self.out_off[k], W.FORMATS.index(f) | (c << 32))
        return torch.from_numpy(tab).to(dev())

    def run(self, poison, single=()):
        """the launch with ``poison`` around every payload and in every output byte -> the whole output buffer (numpy); the
        tracks ``single`` (indices) are decoded again by bt_pcm_decode into a second buffer, which must come out the same"""
        L = self.L
        src = self.source(poison)
        out = Guarded((self.out_floats,), torch.float32).fill(poison)
        tab = self.table(src, out)
        n_max = max(n for _, _, n, _ in self.tracks)
        L.check(L.lib().bt_pcm_decode_batch(L.stream_ptr(dev()), tab.data_ptr(), len(self.tracks), n_max))
        torch.cuda.synchronize()
        assert_intact(("pcm output", out))
        got = out.t.cpu().numpy().copy()
        written = np.zeros(self.out_floats, dtype=bool)
        for k, (f, c, n, a) in enumerate(self.tracks):
            o = self.out_off[k]
            written[o: o + n] = True
            msg = W.same_bits(got[o: o + n], self.want[k])
            assert msg is None, f"{f} x{c}, {n} frames, source alignment {a}, poison 0x{poison:02X}: {msg}"
        untouched = got.view(np.uint8).reshape(-1, 4)[~written]
        assert (untouched == poison).all(), "a float outside a track's n_frames was written"
        if len(single):
            out1 = Guarded((self.out_floats,), torch.float32).fill(poison)
            for k in single:
                f, c, n, _ = self.tracks[k]
                L.check(L.lib().bt_pcm_decode(L.stream_ptr(dev()), src.data_ptr() + self.src_off[k], W.FORMATS.index(f), c, n,
                                              out1.ptr() + 4 * self.out_off[k]))
            torch.cuda.synchronize()
            assert_intact(("pcm output (single)", out1))
            got1 = out1.t.cpu().numpy()
            sel = np.zeros(self.out_floats, dtype=bool)
            for k in single:
                sel[self.out_off[k]: self.out_off[k] + self.tracks[k][2]] = True
            assert np.array_equal(got1.view(np.uint32)[sel], got.view(np.uint32)[sel]), "bt_pcm_decode differs from the batch"
            assert (got1.view(np.uint8).reshape(-1, 4)[~sel] == poison).all()
        return got


@pytest.mark.parametrize("fmt,channels", W.channel_grid())
def test_device_matches_the_twin_at_every_count_and_alignment(fmt, channels):
    L = _L()
    tracks = [(fmt, channels, n, (5 * i + 3) % 16) for i, n in enumerate(_frame_counts())]
    first_aligned = len(tracks)
    tracks += [(fmt, channels, n, a) for n in ALIGN_COUNTS for a in range(16)]
    case = Case(L, tracks)
    single = list(range(first_aligned, len(tracks))) + list(range(0, first_aligned, 97))
    outs = [case.run(p, single if p == POISONS[0] else ()) for p in POISONS]
    # the bytes around a payload do not reach the result: the two runs agree wherever a track was written
    # (elsewhere each holds its own poison), and a third run repeats the first bit for bit
    mask = outs[0].view(np.uint32) != outs[1].view(np.uint32)
    written = np.zeros(case.out_floats, dtype=bool)
    for k, t in enumerate(tracks):
        written[case.out_off[k]: case.out_off[k] + t[2]] = True
    assert not (mask & written).any()
    assert np.array_equal(case.run(POISONS[0]).view(np.uint32), outs[0].view(np.uint32))


def test_one_ragged_launch_with_every_format_and_an_empty_track():
    L = _L()
    grid = W.channel_grid()
    tracks = [(f, c, (37 * k * k + 11 * k + 1) % 3001 + 1, (3 * k) % 16) for k, (f, c) in enumerate(grid)]
    tracks.insert(len(tracks) // 2, ("s24", 2, 0, 7))          # a track of 0 frames in the middle
    tracks.append(("s16", 2, 300_001, 12))                     # the largest: a few hundred thousand frames
    tracks.append(("f64", 7, 0, 0))
    case = Case(L, tracks, seed=100)
    a = case.run(POISONS[0], single=[0, len(tracks) // 2, len(tracks) - 2])
    b = case.run(POISONS[1])
    written = np.zeros(case.out_floats, dtype=bool)
    for k, t in enumerate(tracks):
        written[case.out_off[k]: case.out_off[k] + t[2]] = True
    assert np.array_equal(a.view(np.uint32)[written], b.view(np.uint32)[written])


def test_table_entries_outside_the_contract_write_nothing():
    """the host cannot check a device table: the kernel skips an entry with an unknown format or channel count"""
    L = _L()
    case = Case(L, [("s16", 2, 100, 3), ("f32", 3, 50, 1), ("u8", 1, 9, 0)])
    src = case.source(POISONS[0])
    out = Guarded((case.out_floats,), torch.float32).fill(POISONS[0])
    tab = case.table(src, out).cpu().numpy().copy()
    tab[0, 3] = 6 | (2 << 32)        # unknown format
    tab[1, 3] = 4 | (8 << 32)        # 8 channels of f32
    d_tab = torch.from_numpy(tab).to(dev())
    L.check(L.lib().bt_pcm_decode_batch(L.stream_ptr(dev()), d_tab.data_ptr(), 3, 100))
    torch.cuda.synchronize()
    assert_intact(("pcm output", out))
    got = out.t.cpu().numpy()
    o = case.out_off[2]
    assert W.same_bits(got[o: o + 9], case.want[2]) is None
    assert (got.view(np.uint8)[: 4 * o] == POISONS[0]).all()
    # and the argument checks happen before any launch
    assert L.lib().bt_pcm_decode_batch(L.stream_ptr(dev()), None, 1, 4) == L.BT_ERR_ARG
    assert L.lib().bt_pcm_decode_batch(L.stream_ptr(dev()), d_tab.data_ptr(), L.PCM_MAX_TRACKS + 1, 4) == L.BT_ERR_ARG
    assert L.lib().bt_pcm_decode(L.stream_ptr(dev()), src.data_ptr(), 1, 2, 4, out.ptr() + 4) == L.BT_ERR_ARG   # d_out not 16-byte aligned
    assert L.lib().bt_pcm_decode_batch(L.stream_ptr(dev()), d_tab.data_ptr(), 0, 0) == L.BT_OK
    assert C.sizeof(L.PcmSpan) == 32
