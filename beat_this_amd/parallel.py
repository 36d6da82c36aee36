"""Multi-GPU sharding of the chunk batch: one process per GPU, torch.distributed (backend
"nccl" = RCCL over xGMI on ROCm; "gloo" in the CPU tests).

The reference has no in-process multi-GPU path (README.md:53-56 runs N independent CLI
processes).  Chunks are independent forwards (inference.py:215), so the path shards with a
single exchange: weights replicated, the global chunk list block-partitioned over ranks, one
``all_gather`` of the per-chunk logits (2 x 1500 fp32 = 12 KB per chunk), then every rank
holds everything needed for aggregation + post-processing.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.distributed as dist

from . import inference as inf


def partition(n_items: int, world: int, rank: int):
    """Contiguous block partition with equal (padded) block size: (lo, hi, per_rank)."""
    per = (n_items + world - 1) // world if n_items else 0
    lo = min(rank * per, n_items)
    hi = min(lo + per, n_items)
    return lo, hi, per


def _hip_aggregate(cb, cd, starts, T, border, n):
    from . import _lib

    dev = cb.device
    d_starts = torch.as_tensor(np.asarray(starts, dtype=np.int32), device=dev)
    beat = torch.empty((n,), dtype=torch.float32, device=dev)
    down = torch.empty((n,), dtype=torch.float32, device=dev)
    cb, cd = cb.contiguous(), cd.contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().bt_aggregate(_lib.stream_ptr(dev), cb.data_ptr(), cd.data_ptr(), d_starts.data_ptr(),
                                           len(starts), T, border, n, beat.data_ptr(), down.data_ptr()))
    return beat, down


def _hip_gather(spect, starts, T):
    return inf._gather_chunks(spect, np.asarray(starts), T)[0]


def forward_chunks_sharded(model, spects, chunk_size=1500, border=6, group=None, gather=_hip_gather,
                           aggregate=_hip_aggregate, run=None):
    """[(T_i,128)] -> [(beat_i, downbeat_i)], chunks of all full-length pieces sharded over the
    ranks of ``group`` (or run locally when torch.distributed is not initialised)."""
    run = run or inf._run_batched
    distributed = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if distributed else 1
    rank = dist.get_rank(group) if distributed else 0
    spects = [s.to(torch.float32).contiguous() for s in spects]
    plan = []   # (piece, start) for every full-length chunk, in piece order
    meta = []
    for i, s in enumerate(spects):
        n = s.shape[0]
        starts = inf.chunk_starts(n, chunk_size, border)
        T = inf.chunk_length(n, chunk_size, border)
        meta.append((n, starts, T))
        if T == chunk_size:
            plan += [(i, int(st)) for st in starts]
    results = [None] * len(spects)
    # short pieces: a single (n+12)-frame chunk each, cheap -> computed redundantly on every rank
    for i, (n, starts, T) in enumerate(meta):
        if T != chunk_size:
            cb, cd = run(model, gather(spects[i], starts, T))
            results[i] = aggregate(cb.float(), cd.float(), starts, T, border, n)
    if plan:
        dev = spects[0].device
        lo, hi, per = partition(len(plan), world, rank)
        mine = plan[lo:hi]
        parts = []
        j = 0
        while j < len(mine):  # consecutive chunks of one piece are gathered by one kernel launch
            k = j
            while k < len(mine) and mine[k][0] == mine[j][0]:
                k += 1
            parts.append(gather(spects[mine[j][0]], [st for _, st in mine[j:k]], chunk_size))
            j = k
        local = torch.zeros((per, 2, chunk_size), dtype=torch.float32, device=dev)
        if parts:
            chunks = parts[0] if len(parts) == 1 else torch.cat(parts)
            cb, cd = run(model, chunks)
            local[: hi - lo, 0] = cb.float()
            local[: hi - lo, 1] = cd.float()
        if distributed:   # (also in a world of one: the collective path is the same code on 1 and N ranks)
            full = torch.empty((world * per, 2, chunk_size), dtype=torch.float32, device=dev)
            dist.all_gather_into_tensor(full, local, group=group)
        else:
            full = local
        pos = 0
        for i, (n, starts, T) in enumerate(meta):
            if T == chunk_size:
                seg = full[pos: pos + len(starts)]
                results[i] = aggregate(seg[:, 0].contiguous(), seg[:, 1].contiguous(), starts, T, border, n)
                pos += len(starts)
    return results


def track_frames(n_samples: int, sr: int) -> int:
    """Spectrogram rows of an ``n_samples`` track at sample rate ``sr`` (resampled to 22.05 kHz, hop 441, centred)."""
    from math import gcd

    g = gcd(int(sr), 22050)
    up, down = 22050 // g, int(sr) // g
    n22 = n_samples if up == down else -(-n_samples * up // down)
    return 1 + n22 // 441


def audio2frames_sharded(signals, sr, frames_fn, group=None, device=None):
    """Track-level sharding of ``Audio2Frames.many`` (README.md:53-56 runs N independent CLI processes over a file set; this
    is the in-process form): every rank holds the same list of waveforms, computes the block ``partition`` gives it with
    ``frames_fn(sub_list) -> (beat_cat, downbeat_cat, frame_off)`` (e.g. ``lambda s: a2f.spect2frames_batch(
    *a2f.signal2spect_many(s, sr))`` plus the offsets), and ONE ``all_gather_into_tensor`` of the zero-padded framewise
    logits (2 x frames fp32 per rank: 120 KB per 5-minute track) returns every track's logits to every rank.
    -> [(beat, downbeat)] in the order of ``signals``."""
    distributed = dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if distributed else 1
    rank = dist.get_rank(group) if distributed else 0
    n = len(signals)
    frames = [track_frames(s.shape[0], sr) for s in signals]
    lo, hi, per = partition(n, world, rank)
    blocks = [partition(n, world, r)[:2] for r in range(world)]
    width = max([sum(frames[a:b]) for a, b in blocks] + [1])
    mine = signals[lo:hi]
    if mine:
        beat, down, off = frames_fn(mine)
        dev = beat.device
    else:
        # (an empty block -- fewer tracks than ranks -- still takes part in the collective, on the device the backend moves:
        # a CPU tensor handed to an RCCL group errors out or hangs the other ranks)
        if device is not None:
            dev = torch.device(device)
        elif distributed and dist.get_backend(group) == "nccl":
            dev = torch.device("cuda", torch.cuda.current_device())
        else:
            dev = torch.device("cpu")
        beat = down = torch.zeros(0, device=dev)
    local = torch.zeros((2, width), dtype=torch.float32, device=dev)
    local[0, : beat.shape[0]], local[1, : down.shape[0]] = beat.float(), down.float()
    if distributed:
        full = torch.empty((world * 2, width), dtype=torch.float32, device=dev)  # (concatenation along dim 0)
        dist.all_gather_into_tensor(full, local, group=group)
        full = full.view(world, 2, width)
    else:
        full = local[None]
    out = []
    for r, (a, b) in enumerate(blocks):
        pos = 0
        for k in range(a, b):
            out.append((full[r, 0, pos: pos + frames[k]], full[r, 1, pos: pos + frames[k]]))
            pos += frames[k]
    return out


# ---- data-parallel training: the gradient exchange -------------------------------------------------------
def grad_rank_sum_host(parts: np.ndarray, world: int, n: int, stride: int | None = None, out: np.ndarray | None = None):
    """bt_grad_rank_sum_host on a flat fp32 array holding ``world`` parts of ``n`` elements, ``stride`` elements apart (default
    ``n``) -> ``out`` (a new array, or the one given; ``out is parts`` sums in place over rank 0's part)"""
    from . import _lib

    stride = n if stride is None else stride
    if parts.dtype != np.float32 or not parts.flags.c_contiguous or parts.size < ((world - 1) * stride + n if world >= 1 else 0):
        raise ValueError("parts must be a contiguous float32 array that holds every part")
    if out is None:
        out = np.empty(max(n, 0), np.float32)
    _lib.check(_lib.lib().bt_grad_rank_sum_host(parts.ctypes.data, stride, world, n, out.ctypes.data))
    return out


def segment_length(total: int, world: int) -> int:
    """Elements per rank's segment of a flat buffer of ``total``: ceil(total / world), rounded up to a multiple of 4"""
    return (-(-int(total) // int(world)) + 3) // 4 * 4


class GradientExchange:
    """The one gradient exchange of a data-parallel optimiser step.  The flat gradient buffer (``total`` fp32 elements) is the
    head of a store of ``world * per`` elements, ``per = segment_length(total, world)``; the tail padding is zero and stays
    zero.  ``reduce_(flat)``: one ``all_to_all_single`` hands every rank all ranks' copies of its segment, ``bt_grad_rank_sum``
    adds them IN RANK ORDER (csrc/reduce.hip), one ``all_gather_into_tensor`` returns the summed segments to every rank's
    store.  The traffic is a ring all-reduce's; the result is the same on every rank and is, bit for bit, what autograd's
    in-place accumulation of the ranks' gradients in rank order would have left -- whatever algorithm RCCL picks, because the
    collectives only move data.

    ``self.flat`` is the buffer to accumulate into (``AdamW`` makes it its gradient buffer, so nothing is staged); a foreign
    ``flat`` handed to ``reduce_`` is copied in and out, one extra pass each way.  ``staged=True``: the collectives go through
    host copies (gloo, development runs whose ranks share one GPU); the sum still runs on the GPU."""

    def __init__(self, group, total: int, device, staged: bool = False):
        from . import _lib

        self.group, self.total, self.device, self.staged = group, int(total), torch.device(device), bool(staged)
        self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        if not 1 <= self.world <= _lib.REDUCE_MAX_WORLD:
            raise ValueError(f"a gradient exchange over {self.world} ranks: at most {_lib.REDUCE_MAX_WORLD} are supported")
        self.per = segment_length(self.total, self.world)
        self.store = torch.zeros(self.world * self.per, dtype=torch.float32, device=self.device)
        self.flat = self.store[:self.total]
        self._recv = torch.zeros_like(self.store)   # row r: rank r's copy of this rank's segment

    def _collect(self) -> None:
        if self.staged:
            recv = torch.empty(self.store.shape, dtype=torch.float32)
            dist.all_to_all_single(recv, self.store.cpu(), group=self.group)
            self._recv.copy_(recv)
        else:
            dist.all_to_all_single(self._recv, self.store, group=self.group)

    def _distribute(self, segment: torch.Tensor) -> None:
        if self.staged:
            full = torch.empty(self.store.shape, dtype=torch.float32)
            dist.all_gather_into_tensor(full, segment.cpu(), group=self.group)
            self.store.copy_(full)
        else:
            dist.all_gather_into_tensor(self.store, segment, group=self.group)

    @torch.no_grad()
    def reduce_(self, flat: torch.Tensor) -> torch.Tensor:
        """``flat`` (``total`` fp32 elements on the device) becomes the rank-ordered sum of all ranks' ``flat``; every rank of
        the group calls it, in the same order"""
        from . import _lib

        own = flat.data_ptr() == self.store.data_ptr()
        if flat.numel() != self.total or flat.dtype != torch.float32 or flat.device != self.store.device or not flat.is_contiguous():
            raise ValueError(f"reduce_ takes a contiguous float32 tensor of {self.total} elements on {self.device}")
        if not own:
            self.flat.copy_(flat)
        self._collect()
        with torch.cuda.device(self.device):   # in place over row 0, which is then this rank's summed segment
            _lib.check(_lib.lib().bt_grad_rank_sum(_lib.stream_ptr(self.device), self._recv.data_ptr(), self.per, self.world, self.per,
                                                   self._recv.data_ptr()))
        self._distribute(self._recv[:self.per])
        if not own:
            flat.copy_(self.flat)
        return flat
