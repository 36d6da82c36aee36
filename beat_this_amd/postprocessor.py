"""``Postprocessor`` -- drop-in for beat_this.model.postprocessor.Postprocessor
(postprocessor.py:9-173).  "minimal": the peak mask (x == maxpool7(x) and x > 0) and the
ordered index compaction run in one HIP kernel per call; the handful of surviving indices
go to the host where deduplicate_peaks / nearest-beat snapping / unique run in C++
(bt_postprocess_host, float64 like numpy).  No thread pool.  Logits that live in host memory (the
reference accepts CPU tensors, postprocessor.py:58-83) get the same peak mask from the library's host entry
point (bt_peaks_host).  ``ragged`` (extension) post-processes many tracks stored back to back with one launch
and one device-to-host copy.  "dbn": madmom's DBNDownBeatTrackingProcessor with the reference's arguments, restated in the
library (csrc/dbn.hip: the Viterbi of every track and bar length in one launch; bt_dbn_host for host logits); madmom is
never imported."""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np
import torch

from . import _lib

_PIN_LOCK = threading.Lock()


def _host_post(bidx: np.ndarray, didx: np.ndarray, fps: float):
    bidx = np.ascontiguousarray(bidx, dtype=np.int32)
    didx = np.ascontiguousarray(didx, dtype=np.int32)
    beats = np.empty(max(len(bidx), 1), dtype=np.float64)
    downs = np.empty(max(len(didx), 1), dtype=np.float64)
    nb, nd = C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.lib().bt_postprocess_host(bidx.ctypes.data, len(bidx), didx.ctypes.data, len(didx), float(fps),
                                              beats.ctypes.data, C.byref(nb), downs.ctypes.data, C.byref(nd)))
    return beats[: nb.value].copy(), downs[: nd.value].copy()


def deduplicate_peaks(peaks, width=1) -> np.ndarray:
    """Groups of adjacent peak frame indices that are each not more than ``width`` frames apart (from the group's running mean)
    replaced by their mean -- the reference's public helper (postprocessor.py:176-197), on the library's host entry point."""
    idx = np.ascontiguousarray(np.fromiter(map(int, peaks), dtype=np.int64), dtype=np.int32)
    out = np.empty(max(len(idx), 1), dtype=np.float64)
    m = C.c_int32(0)
    _lib.check(_lib.lib().bt_deduplicate_peaks_host(idx.ctypes.data, len(idx), float(width), out.ctypes.data, C.byref(m)))
    return out[: m.value].copy()


class PendingBeats:
    """Handle of an enqueued post-processing call (``Postprocessor.ragged_async``); ``result()`` -> [(beats, downbeats)] per
    track.  ``result()`` waits for ``done`` (the device-to-host copy into the pinned buffer ``host``), turns the buffer into
    the result with ``decode``, gives the buffer back to ``owner``'s pool and keeps the result.  ``out``: a result known
    already (an empty batch, a host-side post-processor); ``keep``: device buffers the copy reads from."""

    def __init__(self, out=None, host=None, done=None, decode=None, owner=None, keep=None):
        self._out, self._host, self._done, self._decode, self._owner, self._keep = out, host, done, decode, owner, keep

    def result(self):
        if self._out is None:
            self._done.synchronize()
            try:
                self._out = self._decode(self._host.numpy())
            finally:
                self._owner._return_pinned(self._host)
                self._host = self._keep = None
        return self._out


def _no_tracks(n: int) -> PendingBeats:
    return PendingBeats([(np.zeros(0), np.zeros(0)) for _ in range(n)])


# DBNDownBeatTrackingProcessor(beats_per_bar=[3, 4], min_bpm=55.0, max_bpm=215.0, fps=fps, transition_lambda=100)
# (postprocessor.py:31-37) with madmom's defaults for the rest
DBN_PARAMS = dict(beats_per_bar=(3, 4), min_bpm=55.0, max_bpm=215.0, num_tempi=60, transition_lambda=100.0,
                  observation_lambda=16.0, threshold=0.05)


def dbn_tables(fps: float, **kw) -> np.ndarray:
    """The library's DBN tables (bt_dbn_tables, layout in include/beat_this_amd.h) as a uint8 host array; a parameter
    set the kernel cannot run raises ValueError."""
    p = dict(DBN_PARAMS, **kw)
    beats = np.ascontiguousarray(p["beats_per_bar"], dtype=np.int32)
    size = C.c_size_t(0)
    lib = _lib.lib()
    args = (float(fps), float(p["min_bpm"]), float(p["max_bpm"]), int(p["num_tempi"]), float(p["transition_lambda"]),
            float(p["observation_lambda"]), float(p["threshold"]), beats.ctypes.data, len(beats))
    _lib.check(lib.bt_dbn_tables(*args, None, C.byref(size)))
    blob = np.zeros(size.value, dtype=np.uint8)
    _lib.check(lib.bt_dbn_tables(*args, blob.ctypes.data, C.byref(size)))
    return blob


class DBN:
    """``Postprocessor.dbn``: the callable madmom's processor is -- act (T, 2) float64 -> (N, 2) rows (beat time,
    beat number in the bar) -- on the library's host decoder."""

    def __init__(self, tables: np.ndarray, fps: float):
        self.tables, self.fps = tables, fps

    def __call__(self, act):
        act = np.ascontiguousarray(act, dtype=np.float64)
        if act.ndim != 2 or act.shape[1] != 2:
            raise ValueError(f"expected a (T, 2) activation, got shape {act.shape}")
        rows = np.zeros((max(len(act), 1), 2), dtype=np.int32)
        n = C.c_int32(0)
        _lib.check(_lib.lib().bt_dbn_host_act(self.tables.ctypes.data, act.ctypes.data, len(act), rows.ctypes.data, C.byref(n)))
        return _dbn_rows(rows[: n.value], self.fps)


def _dbn_rows(rows: np.ndarray, fps: float) -> np.ndarray:
    """(frame, beat number) int32 rows -> madmom's output: float64 (frame / fps, beat number)"""
    return np.vstack((rows[:, 0].astype(np.int64) / float(fps), rows[:, 1].astype(np.float64))).T


def _split_rows(out: np.ndarray, fps: float):
    res = _dbn_rows(out, fps)
    return res[:, 0].copy(), res[res[:, 1] == 1][:, 0].copy()


_DBN_LOCK = threading.Lock()


class Postprocessor:
    def __init__(self, type: str = "minimal", fps: int = 50):
        assert type in ["minimal", "dbn"]
        self.type = type
        self.fps = fps
        if type == "dbn":
            self._dbn_tables = dbn_tables(fps)
            self._dbn_dev = {}   # device -> uploaded tables
            self.dbn = DBN(self._dbn_tables, fps)

    def __call__(self, beat: torch.Tensor, downbeat: torch.Tensor, padding_mask: torch.Tensor | None = None):
        batched = beat.ndim != 1
        if not batched:
            beat, downbeat = beat.unsqueeze(0), downbeat.unsqueeze(0)
            padding_mask = None if padding_mask is None else padding_mask.unsqueeze(0)
        if self.type == "minimal":
            pb, pd = self.postp_minimal(beat, downbeat, padding_mask)
        else:
            pb, pd = self.postp_dbn(beat, downbeat, padding_mask)
        return (pb, pd) if batched else (pb[0], pd[0])

    def postp_minimal(self, beat, downbeat, padding_mask=None):
        B, T = beat.shape
        if (B == 1 and padding_mask is None and beat.is_cuda and beat.dtype == downbeat.dtype == torch.float32 and beat.is_contiguous()
                and downbeat.is_contiguous() and beat.untyped_storage().data_ptr() == downbeat.untyped_storage().data_ptr()
                and downbeat.data_ptr() == beat.data_ptr() + 4 * T):
            logits = torch.as_strided(beat, (1, 2, T), (2 * T, T, 1))   # (the two rows of one buffer, as split_predict_aggregate leaves them: no copy)
        else:
            logits = torch.stack([beat, downbeat], 1).to(torch.float32)  # (B, 2, T)
        if padding_mask is not None:
            logits = logits.masked_fill(~padding_mask.bool().unsqueeze(1), -1000.0)
        logits = logits.contiguous()
        if not logits.is_cuda:  # host logits: the library's host peak mask, same definition
            idx_h = np.zeros((B * 2, max(T, 1)), dtype=np.int32)
            cnt_h = np.zeros(B * 2, dtype=np.int32)
            flat = logits.view(B * 2, T).numpy()
            for a in range(B * 2):
                c = C.c_int32(0)
                _lib.check(_lib.lib().bt_peaks_host(flat[a].ctypes.data, T, idx_h[a].ctypes.data, C.byref(c)))
                cnt_h[a] = c.value
        else:
            # indices and counts travel in ONE buffer -> one device-to-host copy, one synchronisation
            buf = torch.empty((B * 2 * T + B * 2,), dtype=torch.int32, device=beat.device)
            with torch.cuda.device(beat.device):
                _lib.check(_lib.lib().bt_peaks(_lib.stream_ptr(beat.device), logits.data_ptr(), T, B * 2, buf.data_ptr(),
                                               buf[B * 2 * T:].data_ptr()))
            host = buf.cpu().numpy()
            cnt_h, idx_h = host[B * 2 * T:], host[: B * 2 * T].reshape(B * 2, T)
        out_b, out_d = [], []
        for b in range(B):
            frames_b = idx_h[2 * b, : cnt_h[2 * b]]
            frames_d = idx_h[2 * b + 1, : cnt_h[2 * b + 1]]
            if padding_mask is not None:
                # reference truncates masked frames before nonzero(); indices shift accordingly
                m = padding_mask[b].bool().cpu().numpy()
                remap = np.cumsum(m) - 1
                frames_b, frames_d = remap[frames_b], remap[frames_d]
            bt, dt = _host_post(frames_b, frames_d, self.fps)
            out_b.append(bt)
            out_d.append(dt)
        return tuple(out_b), tuple(out_d)

    def ragged(self, beat: torch.Tensor, downbeat: torch.Tensor, frame_off):
        """Extension: "minimal" post-processing of many tracks stored back to back (track k = frames
        ``frame_off[k]:frame_off[k+1]`` of the 1-D ``beat`` / ``downbeat`` device tensors) -> [(beats, downbeats)]:
        one peak-picking launch and one device-to-host copy for all tracks, then the C++ host step per track."""
        return self.ragged_async(beat, downbeat, frame_off).result()

    def ragged_async(self, beat: torch.Tensor, downbeat: torch.Tensor, frame_off) -> "PendingBeats":
        """``ragged`` split in two: everything up to the (asynchronous, pinned-memory) device-to-host copy is enqueued
        now; ``.result()`` waits for that copy and runs the host step.  A caller with several batches enqueues batch
        i + 1 before collecting batch i, so the GPU never idles during the host step."""
        if self.type == "dbn":
            return self._dbn_ragged_async(beat, downbeat, frame_off)
        assert self.type == "minimal"
        _lib.require_gpu(beat, "beat logits")
        frame_off = np.asarray(frame_off, dtype=np.int64)
        n = len(frame_off) - 1
        total = int(frame_off[-1])
        if n == 0 or total == 0:
            return _no_tracks(n)
        dev = beat.device
        b1, d1 = beat.reshape(-1), downbeat.reshape(-1)
        if (b1.dtype == d1.dtype == torch.float32 and b1.is_contiguous() and d1.is_contiguous() and b1.numel() == total
                and b1.untyped_storage().data_ptr() == d1.untyped_storage().data_ptr()
                and d1.data_ptr() == b1.data_ptr() + 4 * total):
            logits = b1   # (the batched forward writes both rows into one buffer: bt_peaks_batch addresses them by offset)
        else:
            logits = torch.cat([b1.float(), d1.float()])   # [2 * total]
        lens = (frame_off[1:] - frame_off[:-1]).astype(np.int32)
        spans = np.empty((2 * n, 2), dtype=np.int32)     # array 2 k = beat of track k, 2 k + 1 = its downbeat
        spans[0::2, 0], spans[1::2, 0] = frame_off[:-1], total + frame_off[:-1]
        spans[0::2, 1] = spans[1::2, 1] = lens
        size = 2 * total + 2 * n
        buf = torch.empty((size,), dtype=torch.int32, device=dev)   # [indices | counts]
        with torch.cuda.device(dev):
            d_spans = _lib.upload(spans, dev)
            _lib.check(_lib.lib().bt_peaks_batch(_lib.stream_ptr(dev), logits.data_ptr(), d_spans.data_ptr(), 2 * n,
                                                 buf.data_ptr(), buf[2 * total:].data_ptr()))
            host = self._pinned(size)
            host[:size].copy_(buf, non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))

        def decode(h):   # [indices | counts]: the peak frames of track k start at its first frame
            cnt = h[2 * total:]
            return [_host_post(h[lo: lo + cnt[2 * k]], h[total + lo: total + lo + cnt[2 * k + 1]], self.fps)
                    for k, lo in enumerate(map(int, frame_off[:-1]))]
        return PendingBeats(host=host[:size], done=done, decode=decode, owner=self, keep=(buf, logits, d_spans))

    def _pinned(self, size: int) -> torch.Tensor:
        """A pinned host buffer of at least ``size`` int32 (pool of returned buffers: page-locking costs ~a millisecond)."""
        with _PIN_LOCK:   # (one Postprocessor may serve several host threads)
            pool = self.__dict__.setdefault("_pin_pool", [])
            for i, t in enumerate(pool):
                if t.numel() >= size:
                    return pool.pop(i)
        return torch.empty((max(size, 1 << 16),), dtype=torch.int32, pin_memory=True)

    def _return_pinned(self, t: torch.Tensor) -> None:
        """Give a buffer of ``_pinned`` (or a view of one) back to the pool."""
        with _PIN_LOCK:
            self.__dict__.setdefault("_pin_pool", []).append(t if t._base is None else t._base)

    def postp_dbn(self, beat, downbeat, padding_mask=None):
        B = beat.shape[0]
        if beat.is_cuda:
            # unpad by the mask (a gather) and decode all tracks with one launch triple
            if padding_mask is None:
                b1, d1 = beat.reshape(-1), downbeat.reshape(-1)
                frame_off = np.arange(B + 1, dtype=np.int64) * beat.shape[1]
            else:
                m = padding_mask.bool().to(beat.device)
                b1, d1 = beat[m], downbeat[m]
                frame_off = np.concatenate([[0], np.cumsum(padding_mask.bool().sum(1).cpu().numpy())]).astype(np.int64)
            out = self._dbn_ragged_async(b1, d1, frame_off).result()
            return tuple(o[0] for o in out), tuple(o[1] for o in out)
        out_b, out_d = [], []
        for b in range(B):
            lb, ld = beat[b], downbeat[b]
            if padding_mask is not None:
                m = padding_mask[b].bool()
                lb, ld = lb[m], ld[m]
            lb = np.ascontiguousarray(lb.double().numpy())
            ld = np.ascontiguousarray(ld.double().numpy())
            rows = np.zeros((max(len(lb), 1), 2), dtype=np.int32)
            n = C.c_int32(0)
            _lib.check(_lib.lib().bt_dbn_host(self._dbn_tables.ctypes.data, lb.ctypes.data, ld.ctypes.data, len(lb),
                                              rows.ctypes.data, C.byref(n)))
            bt, dt = _split_rows(rows[: n.value], self.fps)
            out_b.append(bt)
            out_d.append(dt)
        return tuple(out_b), tuple(out_d)

    def _dbn_device_tables(self, dev) -> torch.Tensor:
        with _DBN_LOCK:
            t = self._dbn_dev.get(dev)
            if t is None:
                t = self._dbn_dev[dev] = torch.from_numpy(self._dbn_tables).to(dev)
            return t

    def _dbn_ragged_async(self, beat, downbeat, frame_off) -> PendingBeats:
        """DBN decode of the tracks ``frame_off[k]:frame_off[k+1]`` of the 1-D device tensors: one bt_dbn_decode (three
        launches) and one device-to-host copy of [row counts | rows]."""
        _lib.require_gpu(beat, "beat logits")
        frame_off = np.asarray(frame_off, dtype=np.int64)
        n = len(frame_off) - 1
        total = int(frame_off[-1])
        if n == 0 or total == 0:
            return _no_tracks(n)
        dev = beat.device
        b1, d1 = beat.reshape(-1), downbeat.reshape(-1)
        f64 = b1.dtype == torch.float64 or d1.dtype == torch.float64
        dt = torch.float64 if f64 else torch.float32
        if (b1.dtype == d1.dtype == dt and b1.is_contiguous() and d1.is_contiguous() and b1.numel() == total
                and b1.untyped_storage().data_ptr() == d1.untyped_storage().data_ptr()
                and d1.data_ptr() == b1.data_ptr() + b1.element_size() * total):
            logits = b1   # (the batched forward writes both rows into one buffer)
        else:
            logits = torch.cat([b1.to(dt), d1.to(dt)])   # (fp16 / bf16 -> fp32 is exact, as is the reference's .double())
        spans = np.empty((n, 4), dtype=np.int32)
        spans[:, 0] = frame_off[:-1]
        spans[:, 1] = total + frame_off[:-1]
        spans[:, 2] = frame_off[1:] - frame_off[:-1]
        spans[:, 3] = frame_off[:-1]
        lib = _lib.lib()
        tables = self._dbn_tables.ctypes.data
        size = n + 2 * total
        with torch.cuda.device(dev):
            d_tab = self._dbn_device_tables(dev)
            ws = torch.empty((lib.bt_dbn_workspace_bytes(tables, n, total),), dtype=torch.uint8, device=dev)
            buf = torch.empty((size,), dtype=torch.int32, device=dev)
            d_spans = _lib.upload(spans, dev)
            _lib.check(lib.bt_dbn_decode(_lib.stream_ptr(dev), tables, d_tab.data_ptr(), logits.data_ptr(), int(f64),
                                         d_spans.data_ptr(), n, total, buf.data_ptr(), ws.data_ptr(), ws.numel()))
            host = self._pinned(size)
            host[:size].copy_(buf, non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))

        def decode(h):   # [row counts | rows]: the (frame, beat number) rows of track k start at row frame_off[k]
            return [_split_rows(h[n + 2 * lo: n + 2 * lo + 2 * int(h[k])].reshape(-1, 2), self.fps)
                    for k, lo in enumerate(map(int, frame_off[:-1]))]
        return PendingBeats(host=host[:size], done=done, decode=decode, owner=self, keep=(buf, logits, d_spans, ws))
