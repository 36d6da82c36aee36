#!/usr/bin/env python
"""Record tests/golden/dataset_reference.npz: the reference's own dataset.py / augment.py (beat_this/dataset) run over the
seeded synthetic data folder of tests/dataset_reference.py, which this tool writes to a temporary directory and the tests
rebuild from the same seed (no spectrogram is committed).  Lightning is not needed: a stub ``pytorch_lightning`` module
stands in for the one base class the reference's data module derives from.

Per case of tests/dataset_reference.py and np.random seed: start_frame, spect_path, dataset, the two framewise truths, the
padding and downbeat masks, the truth_orig_* bytes, column 0 of the item's spectrogram (the synthetic spectrograms hold their
row number there) and a sha256 of the whole spectrogram.  Also: the item lists, dataset sizes and positive weights of the
data module's setups, the test items, and the dataset sizes under length-based oversampling.  No test runs this.

    python tools/make_dataset_golden.py /path/to/reference/checkout [out.npz]
"""
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dataset_reference as R  # noqa: E402


def load_reference(ref_root):
    stub = types.ModuleType("pytorch_lightning")

    class LightningDataModule:
        def __init__(self):
            pass

        def save_hyperparameters(self, *args, **kwargs):
            pass

    stub.LightningDataModule = LightningDataModule
    sys.modules["pytorch_lightning"] = stub
    sys.path.insert(0, ref_root)
    import beat_this.dataset.dataset as ref

    return ref


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def main(argv):
    ref = load_reference(argv[0])
    out = argv[1] if len(argv) > 1 else os.path.join(ROOT, "tests", "golden", "dataset_reference.npz")
    arrays, meta = {}, {"cases": {}, "setups": {}, "oversampling": {}}
    with tempfile.TemporaryDirectory() as tmp:
        folder = Path(R.build_data_folder(tmp))
        for name, (items, kwargs, index) in R.CASES.items():
            ds = quiet(ref.BeatTrackingDataset, items, folder, spect_fps=R.FPS, **kwargs)
            for seed in R.SEEDS:
                np.random.seed(seed)
                item = ds[index]
                key = f"{name}.{seed}"
                spect = np.ascontiguousarray(item["spect"])
                meta["cases"][key] = dict(start_frame=int(item["start_frame"]), spect_path=item["spect_path"],
                                          dataset=item["dataset"], downbeat_mask=bool(item["downbeat_mask"]),
                                          spect_dtype=str(spect.dtype), spect_shape=list(spect.shape),
                                          sha256=hashlib.sha256(spect.tobytes()).hexdigest())
                arrays[key + ".truth_beat"] = item["truth_beat"]
                arrays[key + ".truth_downbeat"] = item["truth_downbeat"]
                arrays[key + ".padding_mask"] = item["padding_mask"]
                arrays[key + ".col0"] = spect[:, 0].astype(np.float16)
                arrays[key + ".truth_orig_beat"] = np.frombuffer(item["truth_orig_beat"], np.uint8)
                arrays[key + ".truth_orig_downbeat"] = np.frombuffer(item["truth_orig_downbeat"], np.uint8)
        for name, kwargs in R.SETUPS.items():
            dm = ref.BeatDataModule(folder, train_length=R.TRAIN_LENGTH, spect_fps=R.FPS, num_workers=0, **kwargs)
            quiet(dm.setup, "fit")
            quiet(dm.setup, "test")
            meta["setups"][name] = dict(train_items=dm.train_items, val_items=dm.val_items, test_items=dm.test_items,
                                        train_len=len(dm.train_dataset), val_len=len(dm.val_dataset),
                                        test_len=len(dm.test_dataset), positive_weights=dm.get_train_positive_weights(),
                                        train_datasets=[item["dataset"] for item in dm.train_dataset.items])
        for factor in R.OVERSAMPLING:
            ds = quiet(ref.BeatTrackingDataset, R.ALPHA, folder, spect_fps=R.FPS, train_length=R.TRAIN_LENGTH,
                       length_based_oversampling_factor=factor)
            meta["oversampling"][str(factor)] = dict(length=len(ds), frames=[int(ds.get_frame_count(i)) for i in range(len(ds))],
                                                     beats=[int(ds.get_beat_count(i)) for i in range(len(ds))],
                                                     downbeats=[int(ds.get_downbeat_count(i)) for i in range(len(ds))])
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(out, **arrays)
    print(f"wrote {out}: {len(meta['cases'])} items, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
