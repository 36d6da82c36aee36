"""The FLAC decode kernels (csrc/flac.hip) on the MI355X against the host twin, bit for bit in output and status: every case
of flac_cases.py alone and in one ragged batch, twice, with the source, the output and the workspace in guarded buffers
poisoned with both patterns -- exactly n_samples floats are written, nothing outside a track's workspace, the bands stay
intact.  The rejected streams go to the device only after the host twin -- the same parser text -- has rejected them."""
import ctypes as C

import numpy as np
import pytest
import torch

import flac_cases as F
import wav_cases as W
from gpu_util import POISONS, Guarded, assert_intact, dev

pytestmark = pytest.mark.gpu

GAP = 256     # poisoned bytes between two tracks' workspaces


def _L():
    from beat_this_amd import _lib

    return _lib


def _probe(L, data):
    info = L.FlacInfo()
    buf = np.frombuffer(data, dtype=np.uint8)
    assert L.lib().bt_flac_probe_host(buf.ctypes.data, len(data), C.byref(info)) == 1
    return info


def _twin(L, data, info):
    """-> (status tuple, output or None where the status is not OK)"""
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.full(info.total_samples, 123.0, dtype=np.float32)
    st = L.FlacStatus()
    L.check(L.lib().bt_flac_decode_host(buf.ctypes.data, C.byref(info), out.ctypes.data, None, C.byref(st)))
    if st.code != F.OK:
        assert (out == 123.0).all()
    return (st.code, st.n_frames, st.n_samples, st.where), (out if st.code == F.OK else None)


class Batch:
    """streams [(name, bytes)] laid out for one ragged call: every file at its own alignment inside one guarded source
    buffer with at least 16 poisoned bytes around it, every output at a 16-byte aligned offset of one guarded buffer with 4
    poisoned floats behind it, every workspace in one guarded buffer with GAP poisoned bytes behind it"""

    def __init__(self, L, streams):
        self.L, self.names = L, [n for n, _ in streams]
        self.data = [d for _, d in streams]
        self.info = [_probe(L, d) for d in self.data]
        self.twin = [_twin(L, d, i) for d, i in zip(self.data, self.info)]     # (the host first: see the module docstring)
        self.ws_n = [L.lib().bt_flac_workspace_bytes(C.byref(i)) for i in self.info]
        assert all(n > 0 and n % 16 == 0 for n in self.ws_n)
        self.src_off, self.out_off, self.ws_off = [], [], []
        s = o = w = 0
        for k, (d, i) in enumerate(zip(self.data, self.info)):
            s += 16
            self.src_off.append(s + (5 * k + 3) % 16)
            s = (self.src_off[-1] + len(d) + 15) // 16 * 16 + 16
            self.out_off.append(o)
            o += (i.total_samples + 3) // 4 * 4 + 4
            self.ws_off.append(w)
            w += self.ws_n[k] + GAP
        self.src_bytes, self.out_floats, self.ws_bytes = s + 16, o, w

    def buffers(self, poison):
        host = np.full(self.src_bytes, poison, dtype=np.uint8)
        for off, d in zip(self.src_off, self.data):
            host[off: off + len(d)] = np.frombuffer(d, dtype=np.uint8)
        self.src_host = host
        src = Guarded((self.src_bytes,), torch.uint8).fill(poison, torch.from_numpy(host).to(dev()))
        out = Guarded((self.out_floats,), torch.float32).fill(poison)
        ws = Guarded((self.ws_bytes,), torch.uint8).fill(poison)
        status = torch.full((len(self.data), 3), -1, dtype=torch.int64, device=dev())
        return src, out, ws, status

    def spans(self, src, out, ws, status, short=0):
        L = self.L
        spans = (L.FlacSpan * len(self.data))()
        for k, i in enumerate(self.info):
            spans[k] = L.FlacSpan(src.ptr() + self.src_off[k], out.ptr() + 4 * self.out_off[k], ws.ptr() + self.ws_off[k],
                                  self.ws_n[k] - short, status.data_ptr() + 24 * k, i)
        return spans

    def check(self, poison, src, out, ws, status, which, what):
        """bands, gaps, statuses and outputs of the tracks ``which`` after a run; every other float and workspace byte must
        still hold the poison -> the whole output buffer"""
        torch.cuda.synchronize()
        assert_intact((what + ": source", src), (what + ": output", out), (what + ": workspace", ws))
        assert np.array_equal(src.t.cpu().numpy(), self.src_host), f"{what}: the source was written"
        got = out.t.cpu().numpy().copy()
        st64 = status.cpu().numpy()
        st = st64.view(np.int32).reshape(len(self.data), 6)
        wsb = ws.t.cpu().numpy()
        written = np.zeros(self.out_floats, dtype=bool)
        ws_used = np.zeros(self.ws_bytes, dtype=bool)
        for k in which:
            want_st, want = self.twin[k]
            got_st = (int(st[k, 0]), int(st[k, 1]), int(st64[k, 1]), int(st64[k, 2]))
            assert got_st == want_st, f"{what}: {self.names[k]}: status {got_st}, the host twin's {want_st}"
            ws_used[self.ws_off[k]: self.ws_off[k] + self.ws_n[k]] = True
            if want is not None:
                o = self.out_off[k]
                written[o: o + len(want)] = True
                msg = W.same_bits(got[o: o + len(want)], want)
                assert msg is None, f"{what}: {self.names[k]}, poison 0x{poison:02X}: {msg}"
        assert (got.view(np.uint8).reshape(-1, 4)[~written] == poison).all(), f"{what}: a float outside a track's n_samples was written"
        assert (wsb[~ws_used] == poison).all(), f"{what}: a byte outside a track's workspace was written"
        for k in range(len(self.data)):
            if k not in which:
                assert (st64[k] == -1).all()
        return got

    def run_batch(self, poison):
        L = self.L
        src, out, ws, status = self.buffers(poison)
        spans = self.spans(src, out, ws, status)
        d_spans = torch.from_numpy(np.frombuffer(bytes(spans), dtype=np.uint8).copy()).to(dev())
        L.check(L.lib().bt_flac_decode_batch(L.stream_ptr(dev()), spans, d_spans.data_ptr(), len(self.data)))
        return self.check(poison, src, out, ws, status, range(len(self.data)), "batch")

    def run_singles(self, poison, which):
        L = self.L
        src, out, ws, status = self.buffers(poison)
        spans = self.spans(src, out, ws, status)
        for k in which:
            sp = spans[k]
            L.check(L.lib().bt_flac_decode(L.stream_ptr(dev()), sp.d_src, C.byref(self.info[k]), sp.d_out, sp.d_ws, sp.ws_bytes, sp.d_status))
        return self.check(poison, src, out, ws, status, list(which), "single")


@pytest.fixture(scope="module")
def valid_batch():
    golden = open(__file__.replace("test_gpu_flac.py", "golden/flac_rfc_example1.flac"), "rb").read()
    return Batch(_L(), [("rfc_example", golden)] + [(c.name, c.data) for c in F.valid()])


def test_known_answer_and_every_case_in_one_ragged_batch_twice(valid_batch):
    b = valid_batch
    assert all(st[0] == F.OK for st, _ in b.twin)
    assert b.twin[0][0] == (F.OK, 1, 1, 57) and b.twin[0][1].view(np.uint32)[0] == np.float32((25588 + 10416) / 32768 / 2).view(np.uint32)
    first = b.run_batch(POISONS[0])
    again = b.run_batch(POISONS[0])
    other = b.run_batch(POISONS[1])
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))          # two runs are identical
    same = first.view(np.uint32) == other.view(np.uint32)                          # ... and no poison reaches a result
    for k, i in enumerate(b.info):
        assert same[b.out_off[k]: b.out_off[k] + i.total_samples].all(), b.names[k]
    assert (~same).sum() == b.out_floats - sum(i.total_samples for i in b.info)


def test_every_case_alone_equals_the_batch(valid_batch):
    b = valid_batch
    batch = b.run_batch(POISONS[1])
    half = len(b.data) // 2
    a = b.run_singles(POISONS[1], range(0, half))
    c = b.run_singles(POISONS[1], range(half, len(b.data)))
    for k, i in enumerate(b.info):
        got = (a if k < half else c)[b.out_off[k]: b.out_off[k] + i.total_samples]
        assert np.array_equal(got.view(np.uint32), batch[b.out_off[k]: b.out_off[k] + i.total_samples].view(np.uint32)), b.names[k]


def test_flac_and_wav_of_the_same_integers_decode_to_the_same_bits(valid_batch):
    b = valid_batch
    L = b.L
    out = b.run_batch(POISONS[0])
    by = {c.name: c for c in F.valid()}
    for name in ("stereo_modes", "wide_accumulator", "bps_8", "channels_8", "frame_as_payload"):
        case = by[name]
        k = b.names.index(name)
        fmt = {8: "u8", 16: "s16", 24: "s24"}[case.bps]
        raw = torch.from_numpy(np.frombuffer(W.payload(fmt, case.pcm + (128 if fmt == "u8" else 0)) + bytes(16), dtype=np.uint8).copy()).to(dev())
        wav = torch.empty((len(case.pcm) + 3) // 4 * 4, dtype=torch.float32, device=dev())
        L.check(L.lib().bt_pcm_decode(L.stream_ptr(dev()), raw.data_ptr(), W.FORMATS.index(fmt), case.channels, len(case.pcm), wav.data_ptr()))
        got = out[b.out_off[k]: b.out_off[k] + len(case.pcm)]
        assert W.same_bits(got, wav.cpu().numpy()[: len(case.pcm)]) is None, name
        assert W.same_bits(got, case.reference()) is None, name


def test_a_workspace_256_bytes_short_is_refused_before_any_launch(valid_batch):
    b = valid_batch
    L = b.L
    src, out, ws, status = b.buffers(POISONS[0])
    spans = b.spans(src, out, ws, status)
    short = b.spans(src, out, ws, status, short=256)
    mixed = (L.FlacSpan * len(b.data))(*spans)
    mixed[len(b.data) - 1] = short[len(b.data) - 1]          # only the last track's workspace is too small
    d_spans = torch.from_numpy(np.frombuffer(bytes(mixed), dtype=np.uint8).copy()).to(dev())
    assert L.lib().bt_flac_decode_batch(L.stream_ptr(dev()), mixed, d_spans.data_ptr(), len(b.data)) == L.BT_ERR_WORKSPACE
    sp = short[3]
    assert L.lib().bt_flac_decode(L.stream_ptr(dev()), sp.d_src, C.byref(b.info[3]), sp.d_out, sp.d_ws, sp.ws_bytes, sp.d_status) == L.BT_ERR_WORKSPACE
    with pytest.raises(RuntimeError):
        L.check(L.BT_ERR_WORKSPACE)
    b.check(POISONS[0], src, out, ws, status, [], "refused")     # nothing ran: every byte still holds the poison


def test_rejected_streams_set_their_status_and_write_no_sample():
    L = _L()
    cases = F.rejected()
    b = Batch(L, [(c.name, c.data) for c in cases])
    for c, (st, out) in zip(cases, b.twin):      # the shared parser rejected each of them on the host, cleanly
        assert st[0] == c.status and st[3] == c.where and out is None, c.name
    for poison in POISONS:
        b.run_batch(poison)                      # statuses equal the twin's, no float written, bands and gaps intact
    b.run_singles(POISONS[0], range(len(cases)))
    # a good track between two rejected ones is not disturbed
    good = F.valid()[0]
    m = Batch(L, [(cases[0].name, cases[0].data), (good.name, good.data), (cases[4].name, cases[4].data)])
    m.run_batch(POISONS[1])


def test_more_candidates_than_the_workspace_provides_for_is_a_status():
    """a valid stream followed by 1 000 six-byte frame headers with good CRC-8s: n / 6 candidates in a workspace for
    n / 8 + 64.  The host twin, which never searches, decodes the stream; the device reports BT_FLAC_CANDIDATES, writes no
    sample and stays inside its workspace."""
    L = _L()
    x = F.tone(192, 1, 16, 60)
    head = bytes([0xFF, 0xF8, 0x10, 0x08, 0x00])
    head += bytes([F.crc8(head)])
    few = F.build("few_headers", x, 16, 44100, [dict(n=192)], trailing=head * 20)
    many = F.build("many_headers", x, 16, 44100, [dict(n=192)], trailing=head * 1000)
    b = Batch(L, [(few.name, few.data), (many.name, many.data)])
    assert b.twin[0][0][0] == F.OK and b.twin[1][0][0] == F.OK
    n = len(many.data) - many.first_frame
    assert 1000 > n // 8 + 64
    b.twin[1] = ((F.CANDIDATES, 0, 0, many.first_frame), None)       # (the one place where the device says more than the twin)
    b.run_batch(POISONS[0])
    b.run_batch(POISONS[1])
