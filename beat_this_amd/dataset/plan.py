"""The planner of training batches: every random decision of the reference's ``BeatTrackingDataset.__getitem__`` drawn from
``np.random`` with the reference's calls in the reference's order, written into the three tables csrc/data.hip reads
(include/beat_this_amd.h: bt_train_item, bt_train_op, bt_train_part), and the two ways to run them: ``run_host``
(bt_train_batch_host on numpy arrays) and ``run_device`` (bt_train_batch, one launch).  The order of the draws for one item:

1. ``randint(2)`` when both pitch and tempo are enabled;
2. the pitch ``randint(min, max + 1)``, or the tempo ``choice(arange(min, max + 1, stride))``;
3. ``randint(0, longer)`` for the start of the excerpt (a piece longer than train_length, not deterministic);
4. ``randint(min_count, max_count + 1)`` masks;
5. per mask its length ``randint(min_len, max_len + 1)`` in frames, then its start ``randint(0, n - length)``;
6. for a permute mask the number of parts ``randint(min_parts, max_parts + 1)``, clamped to length + 1, the cut positions
   ``choice(length, parts - 1, replace=False)`` (sorted afterwards) and the new order ``permutation(parts)``."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from .. import _lib

ZERO, PERMUTE = 0, 1          # BT_MASK_*
F32, F16 = 0, 1               # BT_LOSS_F32 / BT_LOSS_F16: the element types of the store and of the spectrogram output
WIDTH = 128
_KINDS = {"zero": ZERO, "permute": PERMUTE}

ITEM = np.dtype({"names": ["row", "ann_begin", "ann_end", "n", "start_frame", "op_begin", "op_end", "has_downbeats", "reserved"],
                 "formats": ["<i8", "<i8", "<i8", "<i4", "<i4", "<i4", "<i4", "<i4", "<i4"],
                 "offsets": [0, 8, 16, 24, 28, 32, 36, 40, 44], "itemsize": 48})
OP = np.dtype({"names": ["start", "length", "kind", "part_begin", "part_end"], "formats": ["<i4"] * 5,
               "offsets": [0, 4, 8, 12, 16], "itemsize": 20})
PART = np.dtype({"names": ["new_off", "old_off"], "formats": ["<i4", "<i4"], "offsets": [0, 4], "itemsize": 8})

# one mask operation on frames [start, start + length) of an excerpt; parts (permute): (new offset, old offset, frames) of
# every non-empty part in the new order
MaskOp = namedtuple("MaskOp", "start length kind parts")
# one item of a batch: the store row its excerpt starts at, its frames, where the excerpt starts in the piece, its mask
# operations, its range in the annotation arrays, whether its dataset annotates downbeats
ItemPlan = namedtuple("ItemPlan", "row n start_frame ops ann_begin ann_end has_downbeats")

_checked = False


def _check_layout():
    """the numpy dtypes above against the library's structs (once)"""
    global _checked
    if _checked:
        return
    sizes = (C.c_int32 * 10)()
    _lib.lib().bt_train_batch_struct_sizes(sizes)
    mine = [ITEM.itemsize, OP.itemsize, PART.itemsize, ITEM.fields["ann_begin"][1], ITEM.fields["n"][1],
            ITEM.fields["op_begin"][1], ITEM.fields["has_downbeats"][1], OP.fields["kind"][1], OP.fields["part_begin"][1],
            PART.fields["old_off"][1]]
    ctypes_sizes = [C.sizeof(_lib.TrainItem), C.sizeof(_lib.TrainOp), C.sizeof(_lib.TrainPart)]
    if list(sizes) != mine or ctypes_sizes != mine[:3]:
        raise ImportError(f"bt_train_item / _op / _part layouts differ between the library {list(sizes)} and the binding {mine}")
    _checked = True


# ---- the draws ------------------------------------------------------------------------------------------------------------------
def draw_pitch(params) -> int:
    return np.random.randint(params["min"], params["max"] + 1)


def tempo_choices(params):
    return np.arange(params["min"], params["max"] + 1, params["stride"])


def draw_tempo(params):
    return np.random.choice(tempo_choices(params))


def stretched(beat_time, percentage):
    """beat times after a tempo change of ``percentage`` percent (the reference's expression, so the same bits)"""
    return beat_time / (1.0 + percentage / 100)


def draw_variant(augmentations):
    """-> (file name suffix, tempo percentage): the precomputed variant of a piece this item uses"""
    both = "pitch" in augmentations and "tempo" in augmentations
    if "pitch" in augmentations and (not both or np.random.randint(2) == 0):
        semitones = draw_pitch(augmentations["pitch"])
        return (f"_ps{semitones}" if semitones else ""), 0
    if "tempo" in augmentations:
        percentage = draw_tempo(augmentations["tempo"])
        return (f"_ts{percentage}" if percentage else ""), int(percentage)
    return "", 0


def variant_suffixes(augmentations):
    out = [""]
    for method, params in augmentations.items():
        if method == "pitch":
            out += [f"_ps{s}" for s in range(params["min"], params["max"] + 1) if s]
        elif method == "tempo":
            out += [f"_ts{p}" for p in range(params["min"], params["max"] + 1, params["stride"]) if p]
    return out


def draw_mask_op(length, start, kind, min_parts, max_parts) -> MaskOp:
    if kind not in _KINDS:
        raise ValueError(f"Unsupported mask operation: {kind}")
    if kind == "zero":
        return MaskOp(start, length, ZERO, ())
    count = min(np.random.randint(min_parts, max_parts + 1), length + 1)
    cuts = np.random.choice(length, count - 1, replace=False)
    cuts.sort()
    order = np.random.permutation(count)
    bounds = [0, *cuts.tolist(), length]
    parts, new = [], 0
    for j in order.tolist():
        size = bounds[j + 1] - bounds[j]
        if size:
            parts.append((new, bounds[j], size))
            new += size
    return MaskOp(start, length, PERMUTE, tuple(parts))


def plan_mask(n, params, fps):
    """the mask operations of one excerpt of n frames, in the order the reference applies them"""
    count = np.random.randint(params["min_count"], params["max_count"] + 1)
    min_len, max_len = int(params["min_len"] * fps), int(params["max_len"] * fps)
    ops = []
    for _ in range(count):
        length = np.random.randint(min_len, max_len + 1)
        start = np.random.randint(0, n - length)   # (ValueError "low >= high" for a mask not shorter than the excerpt)
        ops.append(draw_mask_op(length, start, params["kind"], params.get("min_parts"), params.get("max_parts")))
    return ops


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def tables(plans):
    """[ItemPlan] -> (items, ops, parts) as arrays of the three struct dtypes"""
    items = np.zeros(len(plans), ITEM)
    ops, parts = [], []
    for b, p in enumerate(plans):
        first = len(ops)
        for op in p.ops:
            ops.append((op.start, op.length, op.kind, len(parts), len(parts) + len(op.parts)))
            parts.extend((new, old) for new, old, _ in op.parts)
        items[b] = (p.row, p.ann_begin, p.ann_end, p.n, p.start_frame, first, len(ops), int(bool(p.has_downbeats)), 0)
    return items, np.array(ops, OP) if ops else np.zeros(0, OP), np.array(parts, PART) if parts else np.zeros(0, PART)


def _np_dtype_code(dtype, what):
    if dtype == np.float16:
        return F16
    if dtype == np.float32:
        return F32
    raise ValueError(f"{what} must be float16 or float32, not {dtype}")


def _p(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def run_host(store, plans, L, ann_time, ann_value, fps, spect_dtype=None, want_spect=True, want_targets=True):
    """bt_train_batch_host: ``store`` a C-contiguous (rows, 128) float16 / float32 array.  -> dict of numpy arrays: spect
    (B, L, 128) of spect_dtype (default: the store's), truth_beat / truth_downbeat / padding_mask (B, L) bool, downbeat_mask
    (B,) bool"""
    _check_layout()
    if store.ndim != 2 or store.shape[1] != WIDTH:
        raise ValueError(f"expected a (frames, {WIDTH}) spectrogram, got {store.shape}")
    if not store.flags.c_contiguous:
        store = np.ascontiguousarray(store)
    spect_dtype = np.dtype(store.dtype if spect_dtype is None else spect_dtype)
    items, ops, parts = tables(plans)
    B = len(plans)
    out = {}
    if want_spect:
        out["spect"] = np.empty((B, L, WIDTH), spect_dtype)
    if want_targets:
        for k in ("truth_beat", "truth_downbeat", "padding_mask"):
            out[k] = np.empty((B, L), np.uint8)
        out["downbeat_mask"] = np.empty(B, np.uint8)
    ann_time = np.ascontiguousarray(ann_time, np.float64)
    ann_value = np.ascontiguousarray(ann_value, np.int32)
    _lib.check(_lib.lib().bt_train_batch_host(
        _p(store), _np_dtype_code(store.dtype, "the spectrogram store"), store.shape[0], items.ctypes.data, B, L, _p(ops),
        ops.size, _p(parts), parts.size, _p(ann_time), _p(ann_value), ann_time.size, float(fps), _p(out.get("spect")),
        _np_dtype_code(spect_dtype, "the spectrogram output"), _p(out.get("truth_beat")), _p(out.get("truth_downbeat")),
        _p(out.get("padding_mask")), _p(out.get("downbeat_mask"))))
    return {k: (v if k == "spect" else v.view(np.bool_)) for k, v in out.items()}


def check_tables(items, ops, parts, store_rows, L, n_ann):
    """what bt_train_batch_host checks before it runs, for tables that go to the device (which cannot refuse them)"""
    n, row = items["n"].astype(np.int64), items["row"]
    if ((n < 0) | (n > L) | (row < 0) | (row + n > store_rows)).any():
        raise ValueError("a batch item reaches outside the spectrogram store or the batch length")
    if ((items["ann_begin"] < 0) | (items["ann_end"] < items["ann_begin"]) | (items["ann_end"] > n_ann)).any():
        raise ValueError("a batch item's annotation range lies outside the annotation arrays")
    for it in items:
        o = ops[it["op_begin"]:it["op_end"]]
        if ((o["start"] < 0) | (o["length"] < 0) | (o["start"].astype(np.int64) + o["length"] > it["n"])).any():
            raise ValueError("a mask operation reaches outside its excerpt")
    if parts.size and ((ops["part_begin"] < 0) | (ops["part_end"] > parts.size)).any():
        raise ValueError("a mask operation's parts lie outside the parts table")


def run_device(stream_device, store, store_rows, store_code, plans, L, d_ann_time, d_ann_value, n_ann, fps, out):
    """bt_train_batch: ONE upload of the three tables (one pinned block) and ONE launch on the current stream.  ``store`` a
    device tensor; ``out``: dict of device tensors to fill, any of spect (float32 / float16), truth_beat, truth_downbeat,
    padding_mask, downbeat_mask (bool or uint8)."""
    import torch

    _check_layout()
    items, ops, parts = tables(plans)
    check_tables(items, ops, parts, store_rows, L, n_ann)
    raw = [items.view(np.uint8).reshape(-1), ops.view(np.uint8).reshape(-1), parts.view(np.uint8).reshape(-1)]
    starts, total = [], 0
    for r in raw:
        starts.append(total)
        total += (r.size + 15) // 16 * 16
    block = np.zeros(max(total, 16), np.uint8)
    for s, r in zip(starts, raw):
        block[s:s + r.size] = r
    d_block = _lib.upload(block, stream_device)
    base = d_block.data_ptr()
    spect = out.get("spect")
    if spect is not None and spect.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"the spectrogram output must be float32 or float16, not {spect.dtype}")
    for k, t in out.items():
        _lib.require_gpu(t, k)
        want = (len(plans), L, WIDTH) if k == "spect" else (len(plans),) if k == "downbeat_mask" else (len(plans), L)
        if tuple(t.shape) != want or not t.is_contiguous() or (k != "spect" and t.element_size() != 1):
            raise ValueError(f"out['{k}'] must be a contiguous {want} tensor" + ("" if k == "spect" else " of one-byte elements"))
    _lib.check(_lib.lib().bt_train_batch(
        _lib.stream_ptr(stream_device), _lib.ptr(store), store_code, store_rows, base + starts[0], len(plans), L,
        base + starts[1] if ops.size else None, ops.size, base + starts[2] if parts.size else None, parts.size,
        _lib.ptr(d_ann_time) if n_ann else None, _lib.ptr(d_ann_value) if n_ann else None, n_ann, float(fps), _lib.ptr(spect),
        F16 if spect is not None and spect.dtype == torch.float16 else F32, _lib.ptr(out.get("truth_beat")),
        _lib.ptr(out.get("truth_downbeat")), _lib.ptr(out.get("padding_mask")), _lib.ptr(out.get("downbeat_mask"))))
    return out


def apply_ops_(spect, ops):
    """mask operations in place on one (frames, 128) spectrogram: numpy array or CPU tensor through the host twin, CUDA
    tensor through the kernel (one scratch copy, then the gather)"""
    import torch

    n = len(spect)
    plan = [ItemPlan(0, n, 0, ops, 0, 0, False)]
    if isinstance(spect, torch.Tensor) and spect.is_cuda:
        if spect.dim() != 2 or spect.shape[1] != WIDTH or spect.dtype not in (torch.float32, torch.float16) or not spect.is_contiguous():
            raise ValueError(f"expected a contiguous (frames, {WIDTH}) float32 / float16 spectrogram, got {tuple(spect.shape)} {spect.dtype}")
        if n:
            run_device(spect.device, spect.clone(), n, F16 if spect.dtype == torch.float16 else F32, plan, n, None, None, 0, 1.0,
                       {"spect": spect.view(1, n, WIDTH)})
        return spect
    a = spect.numpy() if isinstance(spect, torch.Tensor) else spect
    if a.ndim != 2 or a.shape[1] != WIDTH:
        raise ValueError(f"expected a (frames, {WIDTH}) spectrogram, got {a.shape}")
    if n:
        a[...] = run_host(a.copy(), plan, n, np.zeros(0), np.zeros(0, np.int32), 1.0, want_targets=False)["spect"][0]
    return spect
