#!/usr/bin/env python
"""Training batches per second at the training shape: 8 excerpts of 1500 frames with the mask augmentation of the reference's
train.py, from a seeded synthetic set of float16 pieces (--pieces of 3000 .. 9000 frames, one bundle).  Four legs:

  resident:  ds.batch with the store in device memory (planning on the host + one upload of the tables + one launch), host
             clock around --batches batches ending in a synchronise; next to it the kernel alone (device events around
             bt_train_batch with the tables already planned);
  staged:    ds.batch with resident=False (the excerpts go through pinned memory);
  host:      the library's host twin, ds[i] for 8 items, no collate or upload;
  numpy:     the restated numpy item (tests/dataset_reference.py: slicing, in-place masks, np.round targets) for 8 items, then
             torch's default_collate, pin_memory and the upload -- what a DataLoader without workers does per batch.

    python tools/data_speed.py [--batches 200] [--pieces 64] [--json out.json]

Prints one JSON line.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, L, FPS = 8, 1500, 50


def build_folder(root, pieces, seed=1):
    rng = np.random.default_rng(seed)
    ann = os.path.join(root, "annotations", "speed")
    os.makedirs(os.path.join(ann, "annotations", "beats"))
    json.dump({"has_downbeats": True}, open(os.path.join(ann, "info.json"), "w"))
    members, names = {}, []
    for i in range(pieces):
        frames = int(rng.integers(3000, 9001))
        times = np.cumsum(rng.uniform(0.35, 0.65, frames // 20))
        with open(os.path.join(ann, "annotations", "beats", f"p{i:03d}.beats"), "w") as f:
            f.write("".join(f"{t:.4f}\t{k % 4 + 1}\n" for k, t in enumerate(times[times < frames / FPS])))
        members[f"p{i:03d}/track"] = rng.standard_normal((frames, 128)).astype(np.float16)
        names.append(f"speed/p{i:03d}")
    os.makedirs(os.path.join(root, "audio", "spectrograms"))
    np.savez(os.path.join(root, "audio", "spectrograms", "speed.npz"), **members)
    return names


def timed(fn, batches, rng, n_items):
    """batches per second of fn(indices), host clock, the window ends in a device synchronise"""
    for _ in range(5):
        fn(rng.integers(0, n_items, B))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
        fn(rng.integers(0, n_items, B))
    torch.cuda.synchronize()
    return batches / (time.perf_counter() - t0)


def kernel_ms(ds, reps, rng):
    """device events around bt_train_batch alone: the plans are made and their tables uploaded outside the window"""
    from beat_this_amd import _lib
    from beat_this_amd.dataset import plan as P

    ds.batch([0])
    dev = ds.device
    planned = [ds._plan(int(i)) for i in rng.integers(0, len(ds), B)]
    plans = [P.ItemPlan(ds._rows[path] + start, n, start, ops, *item["ann"][pct][:2], True) for item, path, start, n, ops, pct in planned]
    items, ops, parts = P.tables(plans)
    d = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev) for a in (items, ops, parts)]
    out = {"spect": torch.empty((B, L, 128), dtype=torch.float32, device=dev)}
    for k in ("truth_beat", "truth_downbeat", "padding_mask"):
        out[k] = torch.empty((B, L), dtype=torch.bool, device=dev)
    out["downbeat_mask"] = torch.empty(B, dtype=torch.bool, device=dev)

    def call():
        _lib.check(_lib.lib().bt_train_batch(
            _lib.stream_ptr(dev), ds._store[0].data_ptr(), P.F16, ds._store_rows, d[0].data_ptr(), B, L, _lib.ptr(d[1]), ops.size,
            _lib.ptr(d[2]), parts.size, ds._d_ann[0].data_ptr(), ds._d_ann[1].data_ptr(), ds._ann_time.size, float(FPS),
            out["spect"].data_ptr(), P.F32, out["truth_beat"].data_ptr(), out["truth_downbeat"].data_ptr(),
            out["padding_mask"].data_ptr(), out["downbeat_mask"].data_ptr()))

    for _ in range(10):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def numpy_batch(ds, indices, mask):
    """the restated numpy path for one batch: items, collate, pin, upload"""
    import dataset_reference as R
    from beat_this_amd.dataset import plan as P

    items = []
    for i in indices:
        item = ds.items[int(i)]
        spect = ds._get_spect(item)
        start = np.random.randint(0, len(spect) - L)
        ops = [tuple(op) for op in P.plan_mask(L, mask, FPS)]
        s, beat, down, pad = R.item(spect, start, L, L, ops, item["beat_time"], item["beat_value"], FPS)
        items.append({"spect": s, "truth_beat": beat, "truth_downbeat": down, "padding_mask": pad,
                      "downbeat_mask": torch.as_tensor(True)})
    batch = torch.utils.data.default_collate(items)
    return {k: v.pin_memory().to(ds.device, non_blocking=True) for k, v in batch.items()}


def main():
    import dataset_reference as R
    from beat_this_amd.dataset import BeatTrackingDataset

    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--pieces", type=int, default=64)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/data_speed.py measures on a GPU"
    mask = R.MASK_PERMUTE
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "frames": L, "batches": args.batches}
    with tempfile.TemporaryDirectory() as tmp:
        names = build_folder(tmp, args.pieces)
        kw = dict(spect_fps=FPS, train_length=L, augmentations={"mask": mask}, device="cuda")
        resident = BeatTrackingDataset(names, tmp, resident=True, **kw)
        staged = BeatTrackingDataset(names, tmp, resident=False, **kw)
        res["store_mib"] = round(resident.store_bytes() / 2 ** 20, 1)
        rng = np.random.default_rng(0)
        np.random.seed(0)
        res["resident_batches_per_s"] = round(timed(resident.batch, args.batches, rng, len(names)), 1)
        res["kernel_ms_median"], res["kernel_ms_min"] = (round(x, 4) for x in kernel_ms(resident, 50, rng))
        res["staged_batches_per_s"] = round(timed(staged.batch, args.batches, rng, len(names)), 1)
        res["host_twin_batches_per_s"] = round(timed(lambda idx: [resident[int(i)] for i in idx], max(args.batches // 4, 5), rng,
                                                     len(names)), 1)
        res["numpy_collate_upload_batches_per_s"] = round(timed(lambda idx: numpy_batch(resident, idx, mask),
                                                                max(args.batches // 4, 5), rng, len(names)), 1)
    # bytes the kernel moves per batch: float16 rows in, float32 rows and three byte planes out
    res["kernel_mib_per_batch"] = round(B * L * (128 * 2 + 128 * 4 + 3) / 2 ** 20, 2)
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
