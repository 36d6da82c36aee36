"""Inference API -- drop-in for beat_this/inference.py (same names, signatures, return types,
exceptions), backed by the HIP kernels of libbeat_this_amd.so.

Differences that matter for speed, not for results:
  * ``split_predict_aggregate`` runs ALL chunks of a piece as one batch (the reference loops
    batch-1, inference.py:215); chunk gathering and keep_first aggregation are GPU kernels.
  * ``Spect2Frames.spect2frames_many`` (extension) batches the chunks of several pieces, and
    shards them over torch.distributed ranks (RCCL) when a process group is initialised.
  * ``Audio2Beats.many`` / ``Audio2Frames.signal2spect_many`` / ``Spect2Frames.spect2frames_batch`` (extensions):
    a whole list of tracks per call -- ONE launch per stage (resample, log-mel, chunk gather, forward slices,
    aggregation, peak picking) and ONE device-to-host copy for all tracks.
  * ``File2Beats.many`` / ``many_async`` / ``Audio2Frames.files2waves`` (extensions) and ``device_decode=True`` (opt-in): PCM
    WAV files go to the GPU as the bytes they are and are decoded there (csrc/pcm.hip: the channel mean in fp64 exactly as
    numpy computes it, so the waveform has the bits of ``load_audio`` + ``mean(1)``), and so do FLAC files (csrc/flac.hip:
    frame search, Rice and LPC decode on the device, the same channel mean); a file neither ``wav.probe`` nor ``flac.probe``
    fully recognises takes ``load_audio`` as before.

Precision (the ``float16`` argument of the inference classes):
  * ``False`` (the reference's default): fp32 activations and fp32-class results -- framewise logits within 1e-3 of the
    reference's CPU fp32 path (measured 1e-5 .. 2e-5), identical beats -- with every product of the forward on three fp16
    MFMAs over hi + lo operand halves (BT_PREC_F32X3; ``BeatThis.fp32_split_gemms``).  A batch whose operands leave the
    fp16 range of a hi half is detected and repeated on the exact fp32 MFMA path (``Engine.last_fallbacks``).
  * ``True``: the reference's float16 autocast -- fp16 MFMA operands, fp32 accumulation; not under the 1e-3 gate.
  * ``"exact"``: every product on exact fp32 MFMAs (``v_mfma_f32_32x32x2_f32``), a third of the default's speed.

Limits of the drop-in (there is no CPU implementation in this package):
  * ``device`` must be a ROCm GPU; the default is "cuda" (the reference's default "cpu" raises here, in ``__init__``);
  * the resampler is a Kaiser-windowed-sinc polyphase FIR built to libsoxr's HQ specification, not libsoxr.
"""
from __future__ import annotations

import inspect
import threading

import numpy as np
import torch

from . import _lib
from .model import BeatThis
from .pack import Engine
from .postprocessor import PendingBeats, Postprocessor, _host_post
from .preprocessing import LogMelSpect, load_audio
from .utils import replace_state_dict_key, save_beat_tsv

CHECKPOINT_URL = "https://cloud.cp.jku.at/public.php/dav/files/7ik4RrBKTS273gp"
MAX_CHUNKS_PER_LAUNCH = 96  # workspace is ~70 MB (fp32) / ~45 MB (half) per chunk; larger batches are split into equal slices
CONCURRENT_STREAMS = 2      # forward slices of a big batch run on this many streams (1 = everything on the caller's stream)
CONCURRENT_SLICE_CHUNKS = 32  # ... from this many chunks on
_SIDE_STREAMS: dict = {}


def _side_streams(main, n):
    """The ``n`` side streams of a batch issued on the stream ``main``: every caller stream has its own, so host threads on
    their own streams never share one -- nor the workspace the engine keeps per stream."""
    key = (main, n)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = [torch.cuda.Stream(main.device) for _ in range(n)]
    return _SIDE_STREAMS[key]


def _copy_stream(dev):
    key = (torch.device(dev).index, "copy")
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(dev)
    return _SIDE_STREAMS[key]


READ_THREADS = 4   # host threads that read files into pinned buffers (files2waves); never sized from the machine's CPU count
_READ_POOL = None
_RAW_POOL: list = []        # [(pinned uint8 tensor, event of the upload that last read it)]
_RAW_POOL_MAX = 16
_RAW_LOCK = threading.Lock()


def _read_pool():
    global _READ_POOL
    if _READ_POOL is None:
        from concurrent.futures import ThreadPoolExecutor

        _READ_POOL = ThreadPoolExecutor(max_workers=READ_THREADS, thread_name_prefix="bt-read")
    return _READ_POOL


def _raw_pinned(nbytes: int) -> torch.Tensor:
    """A pinned uint8 host buffer of at least ``nbytes`` for a file's raw bytes (page-locking 50 MB costs milliseconds: buffers
    are pooled).  A buffer of the pool is handed out once the upload that last read it has run."""
    with _RAW_LOCK:
        fits = [i for i, (t, _) in enumerate(_RAW_POOL) if t.numel() >= nbytes]
        entry = _RAW_POOL.pop(min(fits, key=lambda i: _RAW_POOL[i][0].numel())) if fits else None
    if entry is None:
        return torch.empty((max(nbytes, 1 << 16),), dtype=torch.uint8, pin_memory=True)
    if entry[1] is not None:
        entry[1].synchronize()
    return entry[0]


def _return_raw(bufs, event) -> None:
    with _RAW_LOCK:
        for t in bufs:
            if len(_RAW_POOL) >= _RAW_POOL_MAX:   # (drop the smallest: the pool keeps what the longest files need)
                _RAW_POOL.sort(key=lambda e: e[0].numel())
                _RAW_POOL.pop(0)
            _RAW_POOL.append((t, event))


def _host_mono(signal) -> np.ndarray:
    """``load_audio``'s signal -> the mono fp32 waveform of ``signal2spect`` (inference.py:269-277): numpy's channel mean"""
    if signal.ndim == 2:
        signal = signal.mean(1)
    elif signal.ndim != 1:
        raise ValueError(f"Expected 1D or 2D signal, got shape {signal.shape}")
    return np.ascontiguousarray(signal, dtype=np.float32)


def load_checkpoint(checkpoint_path, device="cpu") -> dict:
    """Local file, short name or URL -> checkpoint dict (inference.py:16-53)."""
    try:
        return torch.load(checkpoint_path, map_location=device, weights_only=True)
    except FileNotFoundError:
        try:
            if str(checkpoint_path).startswith(("https://", "http://")):
                url, file_name = checkpoint_path, None
            else:
                url, file_name = f"{CHECKPOINT_URL}/{checkpoint_path}.ckpt", f"beat_this-{checkpoint_path}.ckpt"
            return torch.hub.load_state_dict_from_url(url, file_name=file_name, map_location=device)
        except Exception:
            raise ValueError("Could not load the checkpoint given the provided name", checkpoint_path)


def averaged_checkpoint(ckpt) -> dict:
    """A checkpoint of a run with weight averaging (``fit(ema_decay=...)``) -> a checkpoint dict whose ``state_dict`` is the
    averaged one (``ema_state_dict``: the averaged parameters, the live buffers), for ``load_model``, the inference classes and
    ``evaluate``.  ``ckpt``: a loaded dict, or what ``load_checkpoint`` takes.  The other entries are shared with the input."""
    ckpt = ckpt if isinstance(ckpt, dict) else load_checkpoint(ckpt, "cpu")
    if "ema_state_dict" not in ckpt:
        raise ValueError("the checkpoint has no 'ema_state_dict': it was not written by a run with weight averaging (ema_decay)")
    out = {k: v for k, v in ckpt.items() if k != "ema_state_dict"}
    out["state_dict"] = ckpt["ema_state_dict"]
    return out


def _gpu_device(device) -> torch.device:
    """The device argument of the inference classes: a ROCm GPU, or a clear error right away."""
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError(
            f"beat_this_amd runs on ROCm GPUs only (got device='{dev}'): this package has no CPU implementation. "
            "Pass device='cuda' (the default here) or 'cuda:N'.")
    return dev


def load_model(checkpoint_path="final0", device="cpu") -> BeatThis:
    """BeatThis in eval mode on ``device`` (inference.py:56-87).  ``checkpoint_path`` may also be
    an already loaded checkpoint dict, or None for a randomly initialised model."""
    if checkpoint_path is not None:
        ckpt = checkpoint_path if isinstance(checkpoint_path, dict) else load_checkpoint(checkpoint_path, "cpu")
        accepted = set(inspect.signature(BeatThis).parameters)
        hparams = {k: v for k, v in ckpt["hyper_parameters"].items() if k in accepted}
        model = BeatThis(**hparams)
        model.load_state_dict(replace_state_dict_key(dict(ckpt["state_dict"]), "model.", ""))
    else:
        model = BeatThis()
    return model.to(device).eval()


def zeropad(spect: torch.Tensor, left: int = 0, right: int = 0):
    if left == 0 and right == 0:
        return spect
    return torch.nn.functional.pad(spect, (0, 0, left, right), "constant", 0)


def chunk_starts(n_frames: int, chunk_size: int, border_size: int = 6, avoid_short_end: bool = True) -> np.ndarray:
    """Start frames of split_piece (inference.py:120-125)."""
    starts = np.arange(-border_size, n_frames - border_size, chunk_size - 2 * border_size)
    if avoid_short_end and n_frames > chunk_size - 2 * border_size:
        starts[-1] = n_frames - (chunk_size - border_size)
    return starts


def chunk_length(n_frames: int, chunk_size: int, border_size: int) -> int:
    """All chunks of a piece have this many frames (short pieces give one shorter chunk)."""
    return chunk_size if n_frames > chunk_size - 2 * border_size else n_frames + 2 * border_size


def split_piece(spect: torch.Tensor, chunk_size: int, border_size: int = 6, avoid_short_end: bool = True):
    """List of zero-padded chunks + their starts (inference.py:100-135); torch glue for callers
    that want the chunks themselves -- the fast path below gathers them on the GPU instead."""
    n = len(spect)
    starts = chunk_starts(n, chunk_size, border_size, avoid_short_end)
    chunks = [zeropad(spect[max(s, 0): min(s + chunk_size, n)], left=max(0, -s),
                      right=max(0, min(border_size, s + chunk_size - n))) for s in map(int, starts)]
    return chunks, starts


def aggregate_prediction(pred_chunks, starts, full_size, chunk_size, border_size, overlap_mode, device):
    """Reference-compatible aggregation of per-chunk dicts (inference.py:138-185)."""
    if border_size > 0:
        pred_chunks = [{k: p[k][border_size:-border_size] for k in ("beat", "downbeat")} for p in pred_chunks]
    beat = torch.full((full_size,), -1000.0, device=device)
    down = torch.full((full_size,), -1000.0, device=device)
    order = list(zip(starts, pred_chunks))
    if overlap_mode == "keep_first":
        order.reverse()
    for start, p in order:
        beat[start + border_size: start + chunk_size - border_size] = p["beat"]
        down[start + border_size: start + chunk_size - border_size] = p["downbeat"]
    return beat, down


def _gather_chunks(spect: torch.Tensor, starts: np.ndarray, T: int):
    B = len(starts)
    d_starts = torch.as_tensor(np.asarray(starts, dtype=np.int32), device=spect.device)
    chunks = torch.empty((B, T, 128), dtype=torch.float32, device=spect.device)
    with torch.cuda.device(spect.device):
        _lib.check(_lib.lib().bt_split_chunks(_lib.stream_ptr(spect.device), spect.data_ptr(), spect.shape[0],
                                              d_starts.data_ptr(), B, T, chunks.data_ptr()))
    return chunks, d_starts


USE_GRAPHS = True   # single-file path: the forward of up to Engine.GRAPH_MAX_CHUNKS chunks is replayed as one hipGraph
USE_ONE_CALL = True  # Audio2Beats.__call__: one track = ONE library call (bt_audio2beats_enqueue), no Python between the stages
ONE_CALL_MAX_CHUNKS = 96   # longer tracks (> 47 minutes) take the sliced path


def _graphed_forward(model, spect: torch.Tensor, starts: np.ndarray, T: int, prec):
    """The chunks of one piece through a captured forward (pack.Engine.graph_forward): the chunk gather writes straight into
    the graph's input buffer and the aggregation reads the graph's logits -- no launches from the host but three, no copies.
    -> (beat, downbeat, device starts), or None when the model is not a BeatThis on its fused path, the piece is too long or
    graphs are off.  The range flag of BT_PREC_F32X3 is looked at now: if it fired, the piece runs on the exact path instead."""
    if not USE_GRAPHS or not isinstance(model, BeatThis) or len(starts) > Engine.GRAPH_MAX_CHUNKS or _model_hooked(model):
        return None
    eng = model.engine()
    entry = eng.graph_forward(len(starts), T, prec)
    if entry is None:
        return None
    dev = spect.device
    with torch.cuda.device(dev):
        d_starts = _lib.upload(np.asarray(starts, dtype=np.int32), dev)
        _lib.check(_lib.lib().bt_split_chunks(_lib.stream_ptr(dev), spect.data_ptr(), spect.shape[0], d_starts.data_ptr(), len(starts), T,
                                              entry.x.data_ptr()))
        entry.replay()
        if prec == _lib.PREC_F32X3 and int(entry.flag.item()) != 0:
            eng._count_fallback()   # (operands beyond the fp16 range)
            return _chunk_logits(model, spect, starts, T, _lib.PREC_F32, None)
    return entry.beat, entry.down, d_starts


def _model_hooked(model) -> bool:
    from .model import _hooked_below

    return _hooked_below(model) or bool(model._forward_hooks or model._forward_pre_hooks)


def _run_batched(model, chunks: torch.Tensor, prec=None, checks=None):
    """model over (B,T,128) in equal slices of at most MAX_CHUNKS_PER_LAUNCH -> beat, downbeat (B,T).  A BeatThis without
    hooks runs at ``prec`` with ``checks`` (BeatThis._run); any other model through its forward."""
    B = chunks.shape[0]
    step = -(-B // max(1, -(-B // MAX_CHUNKS_PER_LAUNCH)))
    if isinstance(model, BeatThis) and not _model_hooked(model):
        outs = [model._run(chunks[i: i + step], 0, 2, prec=prec, checks=checks) for i in range(0, B, step)]
    else:
        outs = [(o["beat"], o["downbeat"]) for o in (model(chunks[i: i + step]) for i in range(0, B, step))]
    if len(outs) == 1:
        return outs[0]
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


def _chunk_logits(model, spect: torch.Tensor, starts: np.ndarray, T: int, prec, checks):
    """The chunks of one piece gathered and run through ``model`` (_run_batched) -> (beat, downbeat, device starts)."""
    chunks, d_starts = _gather_chunks(spect, starts, T)
    cb, cd = _run_batched(model, chunks, prec, checks)
    return cb.float().contiguous(), cd.float().contiguous(), d_starts


def _model_precision(model):
    """BT_PREC_* a BeatThis runs at now (autocast, ``fp32_split_gemms``); None for any other model."""
    return model._precision() if isinstance(model, BeatThis) else None


def split_predict_aggregate(spect: torch.Tensor, chunk_size: int, border_size: int, overlap_mode: str,
                            model) -> dict:
    """Chunk a (T,128) piece, predict, aggregate (inference.py:188-230).  ``model`` is any callable
    (B,T,128) -> {"beat": (B,T), "downbeat": (B,T)}; all chunks go through it as ONE batch."""
    return _split_predict(spect, chunk_size, border_size, overlap_mode, model, _model_precision(model), None)


def _split_predict(spect, chunk_size, border_size, overlap_mode, model, prec, checks) -> dict:
    """``split_predict_aggregate`` at precision ``prec`` (_model_precision); ``checks``: see Engine.forward_stages (a piece
    whose range flags are collected does not take the captured forward, which looks at its flag at once)."""
    _lib.require_gpu(spect, "spectrogram")
    if spect.dim() != 2 or spect.shape[1] != 128:
        raise ValueError(f"expected a (frames, 128) spectrogram, got {tuple(spect.shape)}")
    spect = spect.to(torch.float32).contiguous()
    n = spect.shape[0]
    if n == 0:  # no chunks: the reference returns empty (full_size = 0) tensors, inference.py:172-173
        empty = torch.empty((0,), dtype=torch.float32, device=spect.device)
        return {"beat": empty, "downbeat": empty.clone()}
    starts = chunk_starts(n, chunk_size, border_size)
    T = chunk_length(n, chunk_size, border_size)
    fast = _graphed_forward(model, spect, starts, T, prec) if overlap_mode == "keep_first" and checks is None else None
    cb, cd, d_starts = fast if fast is not None else _chunk_logits(model, spect, starts, T, prec, checks)
    if overlap_mode != "keep_first":  # "keep_last": reference-compatible torch glue
        preds = [{"beat": cb[i], "downbeat": cd[i]} for i in range(len(starts))]
        beat, down = aggregate_prediction(preds, starts, n, chunk_size, border_size, overlap_mode, spect.device)
        return {"beat": beat, "downbeat": down}
    both = torch.empty((2, n), dtype=torch.float32, device=spect.device)   # (adjacent rows: the peak picker takes them as they lie)
    beat, down = both[0], both[1]
    with torch.cuda.device(spect.device):
        _lib.check(_lib.lib().bt_aggregate(_lib.stream_ptr(spect.device), cb.data_ptr(), cd.data_ptr(),
                                           d_starts.data_ptr(), len(starts), T, border_size, n, beat.data_ptr(),
                                           down.data_ptr()))
    return {"beat": beat, "downbeat": down}


def _precision_mode(float16) -> str:
    """The ``float16`` argument of the inference classes -> "half" | "f32x3" | "exact" (module docstring)."""
    if isinstance(float16, str):
        mode = {"f32x3": "f32x3", "exact": "exact", "fp32": "exact", "f32": "exact", "half": "half", "fp16": "half",
                "float16": "half"}.get(float16.lower())
        if mode is None:
            raise ValueError(f"unknown precision float16={float16!r}: use False (fp32-class results, the default), True "
                             "(fp16 autocast) or 'exact' (exact fp32 MFMAs)")
        return mode
    return "half" if float16 else "f32x3"


class Spect2Frames:
    """Framewise beat/downbeat logits from a spectrogram (inference.py:233-257)."""

    def __init__(self, checkpoint_path="final0", device="cuda", float16=False):
        super().__init__()
        self.device = _gpu_device(device)
        mode = _precision_mode(float16)
        self.float16 = mode == "half"
        # what ``float16=False`` means here: hi + lo fp16 operands (BT_PREC_F32X3, the default of BeatThis itself) or exact fp32
        # MFMAs ("exact").  ``model.fp32_split_gemms`` is the switch; a model assigned to ``.model`` keeps the value its owner
        # gave it (a model shared by two objects is not flipped by the second one) -- except that an object created with
        # float16="exact" turns it off on the models it is given, since that is what it was asked for.
        self.fp32_mode = "exact" if mode == "exact" or _lib.lib().bt_half_is_bf16() else "f32x3"
        self.model = load_model(checkpoint_path, self.device)

    @property
    def model(self):
        return self._model

    @model.setter
    def model(self, m):
        if isinstance(m, BeatThis) and self.fp32_mode == "exact":
            m.fp32_split_gemms = False
        self._model = m

    def spect2frames(self, spect):
        with torch.inference_mode():
            with torch.autocast(enabled=self.float16, device_type=self.device.type):
                pred = split_predict_aggregate(spect=spect, chunk_size=1500, overlap_mode="keep_first",
                                               border_size=6, model=self.model)
        return pred["beat"].float(), pred["downbeat"].float()

    def spect2frames_many(self, spects, group=None):
        """Extension: several (T_i,128) pieces at once.  Chunks of all pieces form one batch; with an
        initialised torch.distributed group the batch is block-partitioned over the ranks, every
        rank computes its share, and ONE all_gather (RCCL over xGMI) returns all chunk logits to
        every rank.  Returns a list of (beat, downbeat) like repeated ``spect2frames`` calls."""
        from .parallel import forward_chunks_sharded

        with torch.inference_mode():
            with torch.autocast(enabled=self.float16, device_type=self.device.type):
                return forward_chunks_sharded(self.model, spects, 1500, 6, group)

    def spect2frames_batch(self, spect: torch.Tensor, frame_off, checks=None):
        """Extension: the pieces ``spect[frame_off[k]:frame_off[k+1]]`` of one concatenated (frames, 128) spectrogram
        -> (beat, downbeat) logits concatenated the same way.  One chunk-gather launch per forward slice, one aggregation
        launch for all pieces (same chunking / keep_first arithmetic as ``spect2frames``, inference.py:188-230).
        ``checks``: see ``batch_predict_aggregate``."""
        with torch.inference_mode():
            with torch.autocast(enabled=self.float16, device_type=self.device.type):
                return batch_predict_aggregate(spect, frame_off, 1500, 6, self.model, checks=checks)

    def __call__(self, spect):
        return self.spect2frames(spect)


class Audio2Frames(Spect2Frames):
    """Framewise logits from an audio signal (inference.py:260-281)."""

    def __init__(self, checkpoint_path="final0", device="cuda", float16=False):
        super().__init__(checkpoint_path, device, float16)
        self.spect = LogMelSpect(device=self.device)

    def signal2spect(self, signal, sr):
        if signal.ndim == 2:
            signal = signal.mean(1)
        elif signal.ndim != 1:
            raise ValueError(f"Expected 1D or 2D signal, got shape {signal.shape}")
        if isinstance(signal, torch.Tensor):   # (a waveform decoded on the device: File2Beats(device_decode=True))
            signal = signal.to(device=self.device, dtype=torch.float32)
        else:
            signal = torch.tensor(signal, dtype=torch.float32, device=self.device)
        if sr != 22050:
            signal = resample_gpu(signal, sr, 22050)
        return self.spect(signal)

    def signal2spect_many(self, signals, sr):
        """Extension: a list of waveforms (numpy (N,) / (N, C) or torch tensors on the host or the device, all at sample rate ``sr``) ->
        (spect, frame_off): ONE (sum of frames, 128) spectrogram tensor with the tracks back to back and the int64 numpy
        array of their first rows (length n + 1).  Mono mix as in ``signal2spect``; resampling and the log-mel run as one
        launch each for all tracks (bt_resample_batch / bt_logmel_batch)."""
        import ctypes as C
        from math import gcd

        dev = self.device
        for sig in signals:
            if sig.ndim not in (1, 2):
                raise ValueError(f"Expected 1D or 2D signal, got shape {tuple(sig.shape)}")
        # Host buffers: PINNED tensors go up on a copy stream of their own (the caller's stream waits for one event), so the
        # upload of batch i + 1 overlaps the kernels of batch i when batches are submitted ahead (many_async); anything else
        # is copied the ordinary, synchronous way.
        cur = torch.cuda.current_stream(dev)
        pinned = [isinstance(sig, torch.Tensor) and sig.device.type == "cpu" and sig.is_pinned() for sig in signals]
        waves = [None] * len(signals)
        if any(pinned):
            copy = _copy_stream(dev)
            with torch.cuda.stream(copy):
                for k, sig in enumerate(signals):
                    if pinned[k]:
                        waves[k] = sig.to(dev, non_blocking=True)
                        waves[k].record_stream(cur)
            ev = torch.cuda.Event()
            ev.record(copy)
            cur.wait_event(ev)
        for k, sig in enumerate(signals):
            w = waves[k]
            if w is None:
                w = sig.to(dev) if isinstance(sig, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(sig)).to(dev)
            if w.dim() == 2:   # mono mix in the signal's own type (float64 for float64 / integer input), like numpy's mean(1)
                w = (w if w.dtype in (torch.float32, torch.float64) else w.to(torch.float64)).mean(1)   # in the reference (inference.py:270-271)
            waves[k] = w.to(torch.float32).contiguous()
        n = len(waves)
        if n == 0:
            return torch.empty((0, 128), dtype=torch.float32, device=dev), np.zeros(1, dtype=np.int64)
        sr = int(sr)
        g = gcd(sr, 22050)
        up, down = 22050 // g, sr // g
        n_in = np.array([w.shape[0] for w in waves], dtype=np.int64)
        n22 = n_in if up == down else -(-n_in * up // down)
        if int(n22.min()) <= 512:
            raise ValueError("signal too short: reflect padding needs more than 512 samples")
        n_fr = 1 + n22 // 441
        s_off = np.concatenate([[0], np.cumsum(n22)]).astype(np.int64)
        frame_off = np.concatenate([[0], np.cumsum(n_fr)]).astype(np.int64)
        lib, st = _lib.lib(), _lib.stream_ptr(dev)
        table = np.zeros((2, n, 4), dtype=np.int64)
        with torch.cuda.device(dev):
            if up != down:
                buf22 = torch.empty(int(s_off[-1]), dtype=torch.float32, device=dev)
                table[0, :, 0] = [w.data_ptr() for w in waves]
                table[0, :, 1], table[0, :, 2], table[0, :, 3] = n_in, s_off[:-1], n22
                table[1, :, 0] = buf22.data_ptr() + 4 * s_off[:-1]
            else:
                table[1, :, 0] = [w.data_ptr() for w in waves]
            table[1, :, 1], table[1, :, 2], table[1, :, 3] = n22, frame_off[:-1], n_fr
            d_table = _lib.upload(table, dev)
            if up != down:
                h, half = _resample_filter(up, down, dev)
                _lib.check(lib.bt_resample_batch(st, d_table[0].data_ptr(), n, int(n22.max()), up, down, h.data_ptr(), half,
                                                 buf22.data_ptr()))
            spect = torch.empty((int(frame_off[-1]), 128), dtype=torch.float32, device=dev)
            if self.spect.device != dev:
                self.spect.to(dev)
            _lib.check(lib.bt_logmel_batch(st, C.byref(self.spect._get_tables()), d_table[1].data_ptr(), n, int(n_fr.max()),
                                           spect.data_ptr()))
        return spect, frame_off

    def files2waves(self, paths):
        """Extension: audio files -> [(mono fp32 waveform on the device, sample rate)] in the order of ``paths``.  PCM WAV
        files (``wav.probe``) are read as they are into pooled pinned buffers -- by up to READ_THREADS host threads that do
        nothing else; only the calling thread touches the GPU --, uploaded on the copy stream and decoded by ONE
        bt_pcm_decode_batch launch: bit for bit the waveform ``load_audio`` + ``mean(1)`` + the fp32 conversion give on the
        host.  FLAC files inside the device decoder's subset (``flac.probe``) go up whole and are decoded -- frame search,
        Rice, LPC, channel mean -- by ONE bt_flac_decode_batch call (csrc/flac.hip); that call reads the tracks' statuses back:
        one small copy and one synchronisation per batch.  Any other file, and a FLAC track whose status is not OK, takes
        exactly the host route (and raises what ``load_audio`` raises)."""
        from . import flac, wav

        dev = self.device
        paths = list(paths)
        out = [None] * len(paths)
        infos = [wav.probe(p) for p in paths]
        flacs = [(k, flac.probe(p)) for k, p in enumerate(paths) if infos[k] is None]
        flacs = [(k, i) for k, i in flacs if i is not None]
        if flacs:
            for (k, _), w in zip(flacs, self._flac2waves([(paths[k], i) for k, i in flacs])):
                out[k] = w
        idx = [k for k, i in enumerate(infos) if i is not None]
        bufs = [_raw_pinned(infos[k].raw_span[1]) for k in idx]        # (allocated here, by the caller; the threads only fill them)
        if len(idx) > 1:
            jobs = [_read_pool().submit(wav.read_raw, infos[k], paths[k], b) for k, b in zip(idx, bufs)]
        else:
            jobs = [_Done(wav.read_raw, infos[k], paths[k], b) for k, b in zip(idx, bufs)]
        ok, pay = [], {}
        for k, b, job in zip(idx, bufs, jobs):
            try:
                pay[k] = job.result()
                ok.append((k, b))
            except OSError:      # (the file changed under us: let load_audio say what it says today)
                infos[k] = None
        if ok:
            cur = torch.cuda.current_stream(dev)
            copy = _copy_stream(dev)
            with torch.cuda.device(dev):
                raws = []
                with torch.cuda.stream(copy):
                    for k, b in ok:
                        d = b[: infos[k].raw_span[1]].to(dev, non_blocking=True)
                        d.record_stream(cur)
                        raws.append(d)
                ev = torch.cuda.Event()
                ev.record(copy)
                cur.wait_event(ev)
                n_fr = np.array([infos[k].n_frames for k, _ in ok], dtype=np.int64)
                off = np.concatenate([[0], np.cumsum((n_fr + 3) // 4 * 4)])       # every track 16-byte aligned
                big = torch.empty(int(off[-1]), dtype=torch.float32, device=dev)
                table = np.zeros((len(ok), 4), dtype=np.int64)                    # bt_pcm_span
                table[:, 0] = [d.data_ptr() + pay[k] for d, (k, _) in zip(raws, ok)]
                table[:, 1] = n_fr
                table[:, 2] = big.data_ptr() + 4 * off[:-1]
                table[:, 3] = [infos[k].format | (infos[k].channels << 32) for k, _ in ok]
                d_table = _lib.upload(table, dev)
                _lib.check(_lib.lib().bt_pcm_decode_batch(_lib.stream_ptr(dev), d_table.data_ptr(), len(ok), int(n_fr.max())))
            _return_raw(bufs, ev)
            for j, (k, _) in enumerate(ok):
                out[k] = (big[int(off[j]): int(off[j]) + int(n_fr[j])], infos[k].sample_rate)
        else:
            _return_raw(bufs, None)
        for k, p in enumerate(paths):
            if out[k] is None:
                signal, sr = load_audio(p)
                out[k] = (torch.from_numpy(_host_mono(signal)).to(dev), sr)
        return out

    def _flac2waves(self, items):
        """[(path, flac.FlacInfo)] -> [(mono fp32 waveform on the device, sample rate), or None for a track whose file could
        not be read or whose status is not OK].  The files go up as they are (pooled pinned buffers, the copy stream); one
        bt_flac_decode_batch call (bt_flac_decode for a single track: no device table) finds and decodes the frames of all
        of them; then the statuses are read back -- one small copy and one synchronisation per call."""
        import ctypes as C

        from . import flac

        dev = self.device
        result = [None] * len(items)
        bufs = [_raw_pinned(i.n_bytes) for _, i in items]
        if len(items) > 1:
            jobs = [_read_pool().submit(flac.read_raw, i, p, b) for (p, i), b in zip(items, bufs)]
        else:
            jobs = [_Done(flac.read_raw, i, p, b) for (p, i), b in zip(items, bufs)]
        ok = []
        for j, job in enumerate(jobs):
            try:
                job.result()
                ok.append(j)
            except OSError:      # (the file changed under us: let load_audio say what it says today)
                pass
        ev = None
        if ok:
            lib = _lib.lib()
            cur = torch.cuda.current_stream(dev)
            copy = _copy_stream(dev)
            with torch.cuda.device(dev):
                raws = []
                with torch.cuda.stream(copy):
                    for j in ok:
                        d = bufs[j][: items[j][1].n_bytes].to(dev, non_blocking=True)
                        d.record_stream(cur)
                        raws.append(d)
                ev = torch.cuda.Event()
                ev.record(copy)
                cur.wait_event(ev)
                infos = [items[j][1].c_info() for j in ok]
                n = np.array([i.total_samples for i in infos], dtype=np.int64)
                off = np.concatenate([[0], np.cumsum((n + 3) // 4 * 4)])          # every track 16-byte aligned
                ws_n = np.array([lib.bt_flac_workspace_bytes(C.byref(i)) for i in infos], dtype=np.int64)
                ws_off = np.concatenate([[0], np.cumsum((ws_n + 255) // 256 * 256)])
                big = torch.empty(int(off[-1]), dtype=torch.float32, device=dev)
                ws = torch.empty(int(ws_off[-1]), dtype=torch.uint8, device=dev)
                status = torch.empty((len(ok), 3), dtype=torch.int64, device=dev)   # bt_flac_status
                spans = (_lib.FlacSpan * len(ok))()
                for t, (d, i) in enumerate(zip(raws, infos)):
                    spans[t] = _lib.FlacSpan(d.data_ptr(), big.data_ptr() + 4 * int(off[t]), ws.data_ptr() + int(ws_off[t]), int(ws_n[t]),
                                             status.data_ptr() + 24 * t, i)
                if len(ok) == 1:
                    sp = spans[0]
                    _lib.check(lib.bt_flac_decode(_lib.stream_ptr(dev), sp.d_src, C.byref(infos[0]), sp.d_out, sp.d_ws, sp.ws_bytes, sp.d_status))
                else:
                    d_table = _lib.upload(np.frombuffer(bytes(spans), dtype=np.uint8), dev)
                    _lib.check(lib.bt_flac_decode_batch(_lib.stream_ptr(dev), spans, d_table.data_ptr(), len(ok)))
                codes = status.view(torch.int32)[:, 0].cpu().numpy()                # (the synchronisation)
            for t, j in enumerate(ok):
                if codes[t] == _lib.FLAC_OK:
                    result[j] = (big[int(off[t]): int(off[t]) + int(n[t])], infos[t].sample_rate)
        _return_raw(bufs, ev)
        return result

    def file2wave(self, path):
        """One PCM WAV file -> (mono fp32 waveform on the device, sample rate) by bt_pcm_decode, or None where ``wav.probe``
        declines the file (the caller then decodes it on the host, as before).  No device table, no second stream: this is
        the latency path of ``File2Beats(device_decode=True)``.  A FLAC file ``flac.probe`` takes is decoded by
        bt_flac_decode (``_flac2waves``: its status is read back, one synchronisation); None as well where that status is
        not OK."""
        from . import flac, wav

        info = wav.probe(path)
        if info is None:
            finfo = flac.probe(path)
            return None if finfo is None else self._flac2waves([(path, finfo)])[0]
        dev = self.device
        buf = _raw_pinned(info.raw_span[1])
        ev = None
        try:
            try:
                pay = wav.read_raw(info, path, buf)
            except OSError:
                return None
            with torch.cuda.device(dev):
                raw = buf[: info.raw_span[1]].to(dev, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
                wave = torch.empty(info.n_frames, dtype=torch.float32, device=dev)
                _lib.check(_lib.lib().bt_pcm_decode(_lib.stream_ptr(dev), raw.data_ptr() + pay, info.format, info.channels,
                                                    info.n_frames, wave.data_ptr()))
        finally:
            _return_raw([buf], ev)
        return wave, info.sample_rate

    def many(self, signals, sr):
        """Extension: [(beat_logits, downbeat_logits)] for a list of waveforms, batched per stage."""
        spect, frame_off = self.signal2spect_many(signals, sr)
        beat, down = self.spect2frames_batch(spect, frame_off)
        return [(beat[frame_off[k]: frame_off[k + 1]], down[frame_off[k]: frame_off[k + 1]]) for k in range(len(signals))]

    def __call__(self, signal, sr):
        return self.spect2frames(self.signal2spect(signal, sr))


class Audio2Beats(Audio2Frames):
    """Beat and downbeat times in seconds from an audio signal (inference.py:284-303)."""

    def __init__(self, checkpoint_path="final0", device="cuda", float16=False, dbn=False):
        super().__init__(checkpoint_path, device, float16)
        self.frames2beats = Postprocessor(type="dbn" if dbn else "minimal")

    def __call__(self, signal, sr):
        out = self._one_call(signal, sr) if USE_ONE_CALL else None
        if out is not None:
            return out
        beat_logits, downbeat_logits = super().__call__(signal, sr)
        return self.frames2beats(beat_logits, downbeat_logits)

    def _one_call(self, signal, sr):
        """``__call__`` as ONE library call (bt_audio2beats_enqueue, include/beat_this_amd.h): the mono mix and the upload of the
        waveform happen here like in ``signal2spect`` (inference.py:269-277), then resampler, log-mel, chunk gather, the forward
        (a hipGraph the library captures itself), aggregation, peak picking and the device-to-host copy of the peak frames are
        enqueued by the library in one go -- round 5's path came back to Python five times per file, and the GPU waited each time
        (profiles/r05_latency_trace.txt).  Same kernels in the same order: bit-identical to the stage-by-stage path (tested).
        -> (beats, downbeats), or None where the call does not apply (DBN post-processing, a model that is not a plain BeatThis,
        hooks, a replaced ``self.spect``, very long tracks) and the caller takes the ordinary path."""
        import ctypes as C
        from math import gcd

        model = self.model
        if (self.frames2beats.type != "minimal" or not isinstance(model, BeatThis) or _model_hooked(model)
                or type(self.spect) is not LogMelSpect or model.device != self.device):
            return None
        signal = np.asarray(signal) if not isinstance(signal, torch.Tensor) else signal
        if signal.ndim == 2:
            signal = signal.mean(1)
        elif signal.ndim != 1:
            raise ValueError(f"Expected 1D or 2D signal, got shape {signal.shape}")
        dev = self.device
        sr = int(sr)
        g = gcd(sr, 22050)
        up, down = 22050 // g, sr // g
        eng = model.engine()
        n_in = int(signal.shape[0])
        if eng.profiling or n_in == 0:
            return None
        with torch.inference_mode(), torch.autocast(enabled=self.float16, device_type=dev.type):
            first = model._precision()
        lib = _lib.lib()
        # BT_PREC_F32X3: if an operand left the fp16 range of a hi part, the exact fp32 path repeats the call
        for prec in (first, _lib.PREC_F32):
            plan = _lib.A2BPlan()
            _lib.check(lib.bt_audio2beats_plan(eng._h, n_in, up, down, prec, C.byref(plan)))
            if plan.B > ONE_CALL_MAX_CHUNKS:
                return None
            eng.ensure_positions(plan.T)
            host = self.frames2beats._pinned(plan.result_words)
            try:
                with torch.cuda.device(dev):
                    # (from_numpy + one H2D copy: torch.tensor(array, device=...) copies the 5 MB of a 30 s file on the host first)
                    wave = torch.from_numpy(np.ascontiguousarray(signal, dtype=np.float32)).to(dev) \
                        if not isinstance(signal, torch.Tensor) else signal.to(dev, torch.float32).contiguous()
                    if self.spect.device != dev:
                        self.spect.to(dev)
                    h, half = _resample_filter(up, down, dev) if up != down else (None, 0)
                    ws = eng._a2b_workspace(plan.ws_bytes)
                    _lib.check(lib.bt_audio2beats_enqueue(eng._h, _lib.stream_ptr(dev), prec, C.byref(self.spect._get_tables()),
                                                          wave.data_ptr(), n_in, up, down, _lib.ptr(h), half, ws.data_ptr(),
                                                          ws.numel(), host.data_ptr(), int(USE_GRAPHS and plan.T == Engine.GRAPH_T)))
                    torch.cuda.current_stream(dev).synchronize()
                res = host.numpy()
                n = int(plan.n_frames)
                nb, nd = int(res[2 * n]), int(res[2 * n + 1])
                if int(res[2 * n + 2]) == 0:   # (the range flag)
                    return _host_post(res[:nb], res[n: n + nd], self.frames2beats.fps)
            finally:
                self.frames2beats._return_pinned(host)
            eng._count_fallback()
        return None

    def many(self, signals, sr):
        """Extension: [(beats, downbeats)] (seconds, float64 arrays as ``__call__`` returns them) for a list of waveforms
        at sample rate ``sr``: every GPU stage is one launch for all tracks and the peak indices of all tracks come back in
        one device-to-host copy (``Postprocessor.ragged``)."""
        return self.many_async(signals, sr).result()

    def many_async(self, signals, sr):
        """``many`` without the final wait: all GPU work and the device-to-host copy of the peak indices are enqueued;
        ``.result()`` of the returned handle waits for the copy and runs the host step.  Submitting batch i + 1 before
        collecting batch i keeps the GPU busy during the host step (bench.py does).  ``.logits``: the batch's framewise
        logits (beat, downbeat, frame_off), concatenated."""
        spect, frame_off = self.signal2spect_many(signals, sr)
        return self._frames2beats_async(spect, frame_off)

    def _frames2beats_async(self, spect, frame_off, prec=None):
        """``many_async`` from the spectrogram on, at precision ``prec`` (None: the model's, read once here)."""
        post = self.frames2beats
        on_device = post.type == "minimal" or (isinstance(post, Postprocessor) and post.type == "dbn")
        with torch.inference_mode(), torch.autocast(enabled=self.float16, device_type=self.device.type):
            if prec is None:
                prec = _model_precision(self.model)
            # float16="f32x3" with a post-processor on the device: the range flags of the forwards are collected, not waited
            # for; ``result()`` looks at them once the batch's device-to-host copy has arrived and repeats the batch on the
            # exact fp32 path if one fired.  A DBN-type post-processor of another kind runs on the host right away and needs
            # final logits: checks=None, the flags are looked at -- and the batch repeated if one fired -- before it sees them.
            checks = [] if on_device and prec == _lib.PREC_F32X3 else None
            beat, down = _batch_predict(spect, frame_off, 1500, 6, self.model, prec, checks)
        if on_device:
            pending = post.ragged_async(beat, down, frame_off)
        else:
            pending = PendingBeats([post(beat[frame_off[k]: frame_off[k + 1]], down[frame_off[k]: frame_off[k + 1]])
                                    for k in range(len(frame_off) - 1)])
        pending.logits = (beat, down, frame_off)
        if checks:
            return _GuardedPending(pending, self.model.engine(), checks,
                                   lambda: self._frames2beats_async(spect, frame_off, _lib.PREC_F32))
        return pending


class _GuardedPending:
    """A pending ``many_async`` result of the BT_PREC_F32X3 path: ``result()`` also evaluates the forwards' range flags
    (they arrived with / before the peak indices) and repeats the batch on the exact path when one fired."""

    def __init__(self, inner, eng, checks, redo):
        self.inner, self.eng, self.checks, self.redo = inner, eng, checks, redo
        self.logits = inner.logits

    def result(self):
        out = self.inner.result()
        if self.checks and self.eng.range_exceeded(self.checks):
            self.inner = self.redo()           # (the exact path: no flags of its own)
            self.logits = self.inner.logits    # ... and its logits replace the overflowed ones
            out = self.inner.result()
        self.checks = self.redo = None   # (the repeat holds the batch's spectrogram)
        return out


class _Done:
    """a call made right away, with the ``result()`` of a future (one file needs no thread)"""

    def __init__(self, fn, *args):
        try:
            self._out, self._exc = fn(*args), None
        except Exception as e:
            self._out, self._exc = None, e

    def result(self):
        if self._exc is not None:
            raise self._exc
        return self._out


class PendingFiles:
    """Handle of ``File2Beats.many_async``: ``result()`` -> [(beats, downbeats)] in the order of the paths; ``logits``: the
    batch's framewise logits (beat, downbeat, frame_off), concatenated in that order."""

    def __init__(self, n, groups):
        self._n, self._groups = n, groups      # groups: [(indices into the paths, pending result of that sample rate)]

    def result(self):
        out = [None] * self._n
        for idx, pending in self._groups:
            for k, r in zip(idx, pending.result()):
                out[k] = r
        return out

    @property
    def logits(self):
        if len(self._groups) == 1:             # (one sample rate: the tracks lie in the order of the paths already)
            return self._groups[0][1].logits
        parts = [None] * self._n
        for idx, pending in self._groups:
            beat, down, off = pending.logits
            for j, k in enumerate(idx):
                parts[k] = (beat[off[j]: off[j + 1]], down[off[j]: off[j + 1]])
        frame_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64)
        if not parts:                          # (no paths)
            return torch.empty(0), torch.empty(0), frame_off
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), frame_off


class File2Beats(Audio2Beats):
    def __init__(self, checkpoint_path="final0", device="cuda", float16=False, dbn=False, device_decode=False):
        super().__init__(checkpoint_path, device, float16, dbn)
        # opt-in: ``__call__`` decodes PCM WAV files on the GPU (``file2wave``).  Off, ``__call__`` is the reference's body.
        # (Where load_audio goes through torchaudio, s32 and f64 samples are rounded to fp32 BEFORE the mono mix there, and
        # the device route may differ from it in the last bit of the waveform: INTEGRATION.md.)
        self.device_decode = bool(device_decode)

    def __call__(self, audio_path):
        if self.device_decode:
            wave = self.file2wave(audio_path)
            if wave is not None:
                return super().__call__(*wave)
        signal, sr = load_audio(audio_path)
        return super().__call__(signal, sr)

    def many(self, paths):
        """Extension: [(beats, downbeats)] for a list of audio files, in the order of ``paths``: ``files2waves`` (PCM WAV
        files decoded on the GPU by one launch), then ``Audio2Beats.many``'s stages once per distinct sample rate."""
        return self.many_async(paths).result()

    def many_async(self, paths):
        """``many`` without the final wait (see ``Audio2Beats.many_async``): the files are read, uploaded and decoded, all
        GPU work is enqueued; ``.result()`` of the returned handle waits and runs the host step, ``.logits`` are the batch's
        framewise logits.  Submitting batch i + 1 before collecting batch i overlaps its file reads with batch i's GPU work."""
        waves = self.files2waves(paths)
        by_rate: dict = {}
        for k, (_, sr) in enumerate(waves):
            by_rate.setdefault(int(sr), []).append(k)
        groups = [(idx, Audio2Beats.many_async(self, [waves[k][0] for k in idx], sr)) for sr, idx in by_rate.items()]
        return PendingFiles(len(waves), groups)


class File2File(File2Beats):
    def __call__(self, audio_path, output_path):
        downbeats, beats = super().__call__(audio_path)  # (sic) argument naming as in inference.py:313-315
        save_beat_tsv(downbeats, beats, output_path)


_RESAMPLE_FILTERS: dict = {}


def _resample_filter(up: int, down: int, device):
    from . import tables

    key = (up, down, torch.device(device))
    if key not in _RESAMPLE_FILTERS:
        h, half = tables.resample_filter(up, down)
        _RESAMPLE_FILTERS[key] = (torch.from_numpy(h.astype(np.float32)).to(device), half)
    return _RESAMPLE_FILTERS[key]


def batch_predict_aggregate(spect: torch.Tensor, frame_off, chunk_size: int, border_size: int, model, checks=None):
    """``split_predict_aggregate`` (keep_first) for several pieces stored back to back in ``spect`` (rows
    ``frame_off[k]:frame_off[k+1]``): -> (beat, downbeat), concatenated like the input.  Pieces longer than
    ``chunk_size - 2 border_size`` frames share one chunk table: their chunks are gathered slice by slice
    (MAX_CHUNKS_PER_LAUNCH) straight into the model and aggregated by one launch; shorter pieces (one odd-length chunk
    each) go through ``split_predict_aggregate`` one by one.
    A ``BeatThis`` with ``fp32_split_gemms`` (BT_PREC_F32X3) runs its forwards without waiting for their range flags: with
    ``checks=None`` the flags are looked at before returning and the batch is repeated on the exact fp32 path if one fired;
    a caller that passes a list gets the flags appended instead (Engine.forward_stages) and evaluates them itself with
    ``model.engine().range_exceeded`` (``Audio2Beats.many_async``)."""
    return _batch_predict(spect, frame_off, chunk_size, border_size, model, _model_precision(model), checks)


def _batch_predict(spect, frame_off, chunk_size, border_size, model, prec, checks):
    """``batch_predict_aggregate`` at precision ``prec`` (_model_precision)."""
    if prec != _lib.PREC_F32X3:
        checks = None   # (no range flags: nothing to collect)
    elif checks is None:
        flags = []
        out = _batch_predict(spect, frame_off, chunk_size, border_size, model, prec, flags)
        if not model.engine().range_exceeded(flags):
            return out
        prec = _lib.PREC_F32   # (the batch again, on the exact path)
    _lib.require_gpu(spect, "spectrogram")
    if spect.dim() != 2 or spect.shape[1] != 128:
        raise ValueError(f"expected a (frames, 128) spectrogram, got {tuple(spect.shape)}")
    spect = spect.to(torch.float32).contiguous()
    dev = spect.device
    frame_off = np.asarray(frame_off, dtype=np.int64)
    total = int(frame_off[-1])
    both = torch.empty((2, total), dtype=torch.float32, device=dev)   # (one buffer: the peak picker takes it without a concatenation)
    beat, down = both[0], both[1]
    rows, pieces = [], []
    for k in range(len(frame_off) - 1):
        lo, hi = int(frame_off[k]), int(frame_off[k + 1])
        n = hi - lo
        if n == 0:
            continue
        if n <= chunk_size - 2 * border_size:  # a single (n + 2 border)-frame chunk
            r = _split_predict(spect[lo:hi], chunk_size, border_size, "keep_first", model, prec, checks)
            beat[lo:hi], down[lo:hi] = r["beat"], r["downbeat"]
            continue
        c0 = len(rows)
        rows += [(lo + int(st), lo, hi, 0) for st in chunk_starts(n, chunk_size, border_size)]
        pieces.append((lo, hi, c0, len(rows)))
    if not rows:
        return beat, down
    if total + chunk_size >= 2 ** 31:
        raise ValueError("batch too long for 32-bit frame indices: split the track list")
    B = len(rows)
    tab = _lib.upload(np.concatenate([np.asarray(rows, dtype=np.int32).reshape(-1), np.asarray(pieces, dtype=np.int32).reshape(-1)]), dev)
    d_rows, d_pieces = tab[: 4 * B], tab[4 * B:]
    cb = torch.empty((B, chunk_size), dtype=torch.float32, device=dev)
    cd = torch.empty((B, chunk_size), dtype=torch.float32, device=dev)
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    # Equal slices of at most MAX_CHUNKS_PER_LAUNCH chunks; from CONCURRENT_SLICE_CHUNKS chunks on, at least two of them
    # on two streams: a launch rarely fills its last round of workgroups (the layer tail of 33 chunks is 387 workgroups
    # on 256 CUs), and the other slice's kernels take the idle CUs.  Each stream has its own chunk buffer and workspace.
    n_slices = -(-B // MAX_CHUNKS_PER_LAUNCH)
    if B >= CONCURRENT_SLICE_CHUNKS and CONCURRENT_STREAMS > 1:
        n_slices = max(n_slices, CONCURRENT_STREAMS)
    step = -(-B // n_slices)                 # (66 chunks -> 33 + 33, not 64 + 2)
    with torch.cuda.device(dev):
        main = torch.cuda.current_stream(dev)
        side = _side_streams(main, min(n_slices, CONCURRENT_STREAMS)) if n_slices > 1 and CONCURRENT_STREAMS > 1 else [main]
        if side[0] is not main:
            ready = torch.cuda.Event()
            ready.record(main)
        for j, i in enumerate(range(0, B, step)):
            nb = min(step, B - i)
            st_ = side[j % len(side)]
            with torch.cuda.stream(st_):
                if st_ is not main:
                    st_.wait_event(ready)
                chunks = torch.empty((nb, chunk_size, 128), dtype=torch.float32, device=dev)
                _lib.check(lib.bt_split_chunks_batch(_lib.stream_ptr(dev), spect.data_ptr(), d_rows[4 * i:].data_ptr(), nb,
                                                     chunk_size, chunks.data_ptr()))
                if isinstance(model, BeatThis) and not _model_hooked(model):
                    model._run(chunks, 0, 2, out=(cb[i: i + nb], cd[i: i + nb]), prec=prec, checks=checks)   # logits straight into their rows
                else:
                    r = model(chunks)
                    cb[i: i + nb], cd[i: i + nb] = r["beat"], r["downbeat"]
        for st_ in side:
            if st_ is not main:
                main.wait_stream(st_)
        st = _lib.stream_ptr(dev)
        max_frames = max(hi - lo for lo, hi, _, _ in pieces)
        _lib.check(lib.bt_aggregate_batch(st, cb.data_ptr(), cd.data_ptr(), d_rows.data_ptr(), d_pieces.data_ptr(),
                                          len(pieces), max_frames, chunk_size, border_size, beat.data_ptr(),
                                          down.data_ptr()))
    return beat, down


def resample_gpu(signal: torch.Tensor, in_rate: int, out_rate: int) -> torch.Tensor:
    """1-D fp32 device waveform at ``in_rate`` -> ``out_rate`` on the GPU (csrc/frontend.hip: resample_kernel), the
    MI355X replacement of the reference's host ``soxr.resample`` (inference.py:274-275).  Polyphase
    Kaiser-windowed-sinc FIR designed to libsoxr's HQ specification (tables.resample_filter: flat to 91.3 % of the lower
    Nyquist frequency, 125 dB rejection from 100 %); like every non-libsoxr resampler it is not bit-compatible with soxr:
    parity is defined from the 22.05 kHz waveform onwards."""
    from math import gcd

    _lib.require_gpu(signal, "waveform")
    if signal.dim() != 1:
        raise ValueError(f"expected a 1-D waveform, got shape {tuple(signal.shape)}")
    in_rate, out_rate = int(in_rate), int(out_rate)
    g = gcd(in_rate, out_rate)
    up, down = out_rate // g, in_rate // g
    if up == down:
        return signal
    h, half = _resample_filter(up, down, signal.device)
    x = signal.to(torch.float32).contiguous()
    n_in = x.shape[0]
    n_out = -(-n_in * up // down)
    y = torch.empty(n_out, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().bt_resample(_lib.stream_ptr(x.device), x.data_ptr(), n_in, up, down, h.data_ptr(), half,
                                          y.data_ptr(), n_out))
    return y
