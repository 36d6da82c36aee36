"""The reference's beat_this/dataset/dataset.py on the GPU: ``BeatTrackingDataset`` keeps the spectrograms of its items in
device memory as they are stored (the float16 ``.npz`` bundles, mapped without a copy by ``SpectBundle``) and builds a
whole training batch -- excerpts, mask augmentation, framewise targets, masks -- in one launch of csrc/data.hip;
``BeatDataModule`` is the reference's data module without Lightning.  DESIGN.md section 12.

``ds[i]`` still gives the reference's item (numpy arrays, from the library's host twin), so a torch ``DataLoader`` works as
before; ``ds.batch(indices)`` gives the collated batch on the device.  Under ``np.random.seed(k)`` both give what the
reference's dataset gives under the same seed (plan.py has the order of the draws)."""
from __future__ import annotations

import concurrent.futures
import itertools
import json
import re
import warnings
from pathlib import Path

import numpy as np
import torch

from ..bundle import SpectBundle
from . import plan as P
from .augment import precomputed_augmentation_filenames

_SUPPORTED = {"mask", "pitch", "tempo"}


class BeatTrackingDataset(torch.utils.data.Dataset):
    """Spectrogram excerpts with beat / downbeat targets, for training or evaluation.

    item_names: names like "gtzan/gtzan_rock_00099"; data_folder: holds audio/spectrograms (``<dataset>.npz`` bundles or
    loose ``<item>/track*.npy`` files) and annotations; spect_fps: frames per second; train_length: frames per excerpt
    (None: whole pieces); deterministic: the middle excerpt instead of a random one; augmentations: dict with any of "tempo",
    "pitch", "mask"; length_based_oversampling_factor: repeat long pieces (0: off).
    device: where ``batch`` builds its batches.  resident: True keeps every spectrogram the items can use in device memory,
    False uploads only each batch's excerpts (through pinned memory), "auto" decides by the free device memory when the
    first batch is built."""

    def __init__(self, item_names, data_folder, spect_fps=50, train_length=1500, deterministic=False, augmentations={},
                 length_based_oversampling_factor=0, device="cuda", resident="auto"):
        if not set(augmentations) <= _SUPPORTED:
            raise ValueError(f"Unsupported augmentations: {augmentations.keys()}")
        if resident not in ("auto", True, False):
            raise ValueError(f"resident must be 'auto', True or False, not {resident!r}")
        data_folder = Path(data_folder)
        self.spect_basepath = data_folder / "audio" / "spectrograms"
        self.annotation_basepath = data_folder / "annotations"
        self.fps = spect_fps
        self.train_length = train_length
        self.deterministic = deterministic
        self.augmentations = augmentations
        self.length_based_oversampling_factor = length_based_oversampling_factor
        self.device = torch.device(device)
        self.resident = resident
        datasets = sorted({name.split("/", 1)[0] for name in item_names})
        self.dataset_info = {}
        for dataset in datasets:
            with open(self.annotation_basepath / dataset / "info.json") as f:
                self.dataset_info[dataset] = json.load(f)
        self.spects = {}
        for dataset in datasets:
            bundle = (self.spect_basepath / dataset).with_suffix(".npz")
            if bundle.exists():
                self.spects[dataset] = SpectBundle(bundle)
        self._loose = {}
        with concurrent.futures.ThreadPoolExecutor() as pool:
            items = [item for item in pool.map(self._load_dataset_item, item_names) if item is not None]
        self._index_members(items)
        self._index_annotations(items)
        if length_based_oversampling_factor and train_length is not None:
            repeated = []
            for item in items:
                factor = np.round(length_based_oversampling_factor * len(self._get_spect(item)) / train_length).astype(int)
                repeated.extend(itertools.repeat(item, max(factor, 1)))
            print(f"Training set oversampled from {len(items)} to {len(repeated)} excerpts.")
            items = repeated
        self.items = items
        self._store = None          # (the device tensor, or None in the staged mode,) once the first batch was built
        self._d_ann = None

    # ---- loading ----------------------------------------------------------------------------------------------------------------
    def _load_dataset_item(self, item_name):
        dataset, stem = item_name.split("/", 1)
        for filename in precomputed_augmentation_filenames(self.augmentations):
            if f"{stem}/{filename[:-4]}" not in self.spects.get(dataset, ()) and \
                    not (self.spect_basepath / item_name / filename).exists():
                print(f"Skipping {item_name} because not all necessary spectrograms are there.")
                return None
        annotation = np.loadtxt(self.annotation_basepath / dataset / "annotations" / "beats" / (stem + ".beats"))
        if annotation.ndim == 2:
            beat_time, beat_value = annotation[:, 0], annotation[:, 1].astype(int)
        else:
            beat_time, beat_value = annotation, np.zeros_like(annotation, dtype=np.int32)
        has_downbeats = self.dataset_info[dataset]["has_downbeats"]
        if has_downbeats and annotation.ndim != 2:
            print(f"Skipping {item_name} because it has {annotation.ndim} columns but downbeat is supposed to be there.")
            return None
        beat_time = np.atleast_1d(beat_time)
        beat_value = np.atleast_1d(beat_value)
        if not np.isfinite(beat_time).all() or (np.diff(beat_time) < 0).any():
            raise ValueError(f"{item_name}: the beat annotations are not finite and ascending (the framewise targets are "
                             "found by bisection, as the reference finds them with searchsorted)")
        if dataset == "rwc":   # the sections of RWC count as datasets of their own
            dataset = "rwc_" + stem.split("_", 2)[1]
        return {"spect_path": Path(item_name) / "track.npy", "beat_time": beat_time, "beat_value": beat_value,
                "downbeat_mask": has_downbeats, "dataset": dataset}

    def _member(self, path):
        """the (frames, 128) array stored under ``<dataset>/<stem>/<file>.npy``: a view into the dataset's bundle, or the
        loose file mapped read-only"""
        path = str(path)
        dataset, name = path.split("/", 1)
        try:
            return self.spects[dataset][name[:-4]]
        except KeyError:
            if path not in self._loose:
                self._loose[path] = np.load(self.spect_basepath / path, mmap_mode="r")
            return self._loose[path]

    def _get_spect(self, item):
        return self._member(item["spect_path"])

    def _index_members(self, items):
        """every spectrogram the items can ask for, in a fixed order with its first row in the store; one dtype, 128 bins"""
        self._rows, self._store_rows, self._store_dtype = {}, 0, None
        for item in items:
            for filename in precomputed_augmentation_filenames(self.augmentations):
                path = str(item["spect_path"].with_name(filename))
                if path in self._rows:
                    continue
                a = self._member(path)
                if a.ndim != 2 or a.shape[1] != P.WIDTH:
                    raise ValueError(f"{path}: expected a (frames, {P.WIDTH}) spectrogram, got {a.shape}")
                if a.dtype not in (np.float16, np.float32):
                    raise ValueError(f"{path}: spectrograms must be float16 or float32, not {a.dtype}")
                if self._store_dtype is None:
                    self._store_dtype = a.dtype
                elif a.dtype != self._store_dtype:
                    raise ValueError(f"{path} is {a.dtype}, earlier spectrograms are {self._store_dtype}: mixed dtypes cannot "
                                     "share one store")
                self._rows[path] = self._store_rows
                self._store_rows += a.shape[0]

    def _index_annotations(self, items):
        """the annotation arrays the kernel reads: per item its beat times as annotated and, with tempo augmentation, one
        stretched copy per tempo (computed here with the reference's expression, so host and device read the same bits)"""
        percentages = [0]
        if "tempo" in self.augmentations:
            percentages += [p for p in P.tempo_choices(self.augmentations["tempo"]) if p]
        times, values, total = [], [], 0
        for item in items:
            item["ann"] = {}
            for p in percentages:
                t = item["beat_time"] if not p else P.stretched(item["beat_time"], p)
                item["ann"][int(p)] = (total, total + len(t), t)
                times.append(t)
                values.append(item["beat_value"])
                total += len(t)
        self._ann_time = np.concatenate(times).astype(np.float64) if times else np.zeros(0)
        self._ann_value = np.concatenate(values).astype(np.int32) if values else np.zeros(0, np.int32)

    # ---- the reference's queries ----------------------------------------------------------------------------------------------------
    def get_frame_count(self, index):
        """number of frames of the given item"""
        return len(self._get_spect(self.items[index]))

    def get_beat_count(self, index):
        """number of beats (downbeats included) of the given item"""
        return len(self.items[index]["beat_time"])

    def get_downbeat_count(self, index):
        """number of downbeats of the given item"""
        return (self.items[index]["beat_value"] == 1).sum()

    def __len__(self):
        return len(self.items)

    # ---- planning -----------------------------------------------------------------------------------------------------------------
    def _plan(self, index):
        """every random decision of one item -> (item, member path, start_frame, frames, mask ops, tempo percentage)"""
        item = self.items[index]
        suffix, percentage = P.draw_variant(self.augmentations)
        path = item["spect_path"].with_name(f"track{suffix}.npy")
        length = len(self._member(path))
        longer = length - self.train_length if self.train_length is not None else 0
        if longer > 0:
            start = longer // 2 if self.deterministic else np.random.randint(0, longer)
            n = self.train_length
        else:
            start, n = 0, length
        ops = P.plan_mask(n, self.augmentations["mask"], self.fps) if "mask" in self.augmentations else []
        return item, str(path), start, n, ops, percentage

    def _truth_orig(self, item, percentage, start, n):
        """the annotations inside the excerpt in seconds from its start, as bytes (sequences of different lengths collate as
        byte strings)"""
        beat = item["ann"][percentage][2]
        down = beat[item["beat_value"] == 1]
        lo, hi = start / self.fps, (start + n) / self.fps
        return tuple((t[(t >= lo) & (t < hi)] - lo).tobytes() for t in (beat, down))

    def __getitem__(self, index):
        if not isinstance(index, (int, np.integer)):
            return [self[i] for i in index]
        item, path, start, n, ops, percentage = self._plan(index)
        L = self.train_length if self.train_length is not None else n
        a0, a1, _ = item["ann"][percentage]
        plan = P.ItemPlan(start, n, start, ops, a0, a1, item["downbeat_mask"])
        r = P.run_host(self._member(path), [plan], L, self._ann_time, self._ann_value, self.fps)
        orig_beat, orig_down = self._truth_orig(item, percentage, start, n)
        return {"spect": r["spect"][0], "spect_path": path, "dataset": item["dataset"], "start_frame": start,
                "truth_beat": r["truth_beat"][0], "truth_downbeat": r["truth_downbeat"][0],
                "downbeat_mask": torch.as_tensor(item["downbeat_mask"]), "padding_mask": r["padding_mask"][0],
                "truth_orig_beat": orig_beat, "truth_orig_downbeat": orig_down}

    # ---- device batches -----------------------------------------------------------------------------------------------------------
    def store_bytes(self):
        return self._store_rows * P.WIDTH * (np.dtype(self._store_dtype).itemsize if self._store_dtype is not None else 0)

    def _ensure_store(self):
        if self._store is not None:
            return
        if self.device.type != "cuda":
            raise RuntimeError(f"beat_this_amd builds batches on ROCm GPUs only, not on '{self.device}' (ds[i] gives host items)")
        resident = self.resident
        if resident == "auto":   # leave a fifth of what is free to the model and its activations
            resident = self.store_bytes() <= 0.8 * torch.cuda.mem_get_info(self.device)[0]
        store = None
        if resident and self._store_rows:
            store = torch.empty((self._store_rows, P.WIDTH), dtype=torch.from_numpy(np.zeros(0, self._store_dtype)).dtype,
                                device=self.device)
            with warnings.catch_warnings():   # read-only mappings: the tensors are only the sources of the uploads
                warnings.simplefilter("ignore", UserWarning)
                for path, row in self._rows.items():
                    a = np.ascontiguousarray(self._member(path))
                    store[row:row + len(a)].copy_(torch.from_numpy(a))
        self._d_ann = (torch.from_numpy(self._ann_time).to(self.device), torch.from_numpy(self._ann_value).to(self.device))
        self.is_resident = bool(resident)
        self._store = (store,)

    def plan_batch(self, indices):
        """The host-side draws of a batch, item by item in the order of ``indices``: what ``batch`` draws when it is not
        handed a plan.  Touches no device; advances numpy's generator exactly as building the batch would."""
        return [self._plan(int(i)) for i in indices]

    def batch(self, indices, out=None, spect_dtype=torch.float32, planned=None):
        """The collated batch of ``ds[i] for i in indices`` on the device, from ONE launch: spect (B, L, 128) of
        ``spect_dtype`` (float32 or float16), truth_beat / truth_downbeat / padding_mask (B, L) and downbeat_mask (B,) as
        torch.bool; truth_orig_beat / truth_orig_downbeat, dataset, spect_path and start_frame as lists with one entry per
        item.  ``out``: a dict with tensors to fill instead of new ones (any of the five device entries).  With
        train_length None all items must have the same number of frames.  ``planned``: the ``plan_batch(indices)`` of this
        batch, drawn earlier (nothing is drawn here then)."""
        self._ensure_store()
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("an empty batch")
        if planned is None:
            planned = self.plan_batch(indices)
        elif len(planned) != len(indices):
            raise ValueError(f"a plan of {len(planned)} items for a batch of {len(indices)}")
        L = self.train_length if self.train_length is not None else planned[0][3]
        if any(p[3] > L or (self.train_length is None and p[3] != L) for p in planned):
            raise ValueError("train_length=None batches whole pieces: they must have the same number of frames "
                             f"(got {[p[3] for p in planned]})")
        store = self._store[0]
        store_rows = self._store_rows
        if store is None:   # staged: only the excerpts travel, through pinned memory
            excerpts = [self._member(path)[start:start + n] for _, path, start, n, _, _ in planned]
            firsts = np.cumsum([0] + [len(e) for e in excerpts])
            store_rows = int(firsts[-1])
            host = np.concatenate(excerpts) if store_rows else np.zeros((0, P.WIDTH), self._store_dtype)
            store = torch.from_numpy(host).pin_memory().to(self.device, non_blocking=True)
            rows = firsts[:-1].tolist()
        else:
            rows = [self._rows[path] + start for _, path, start, _, _, _ in planned]
        plans = [P.ItemPlan(row, n, start, ops, *item["ann"][percentage][:2], item["downbeat_mask"])
                 for row, (item, _, start, n, ops, percentage) in zip(rows, planned)]
        B = len(plans)
        given = dict(out or {})
        dev = self.device
        t = {"spect": given.get("spect", None)}
        if t["spect"] is None:
            t["spect"] = torch.empty((B, L, P.WIDTH), dtype=spect_dtype, device=dev)
        for k in ("truth_beat", "truth_downbeat", "padding_mask", "downbeat_mask"):
            t[k] = given[k] if given.get(k) is not None else \
                torch.empty((B,) if k == "downbeat_mask" else (B, L), dtype=torch.bool, device=dev)
        P.run_device(dev, store, store_rows, P.F16 if self._store_dtype == np.float16 else P.F32, plans, L, self._d_ann[0],
                     self._d_ann[1], self._ann_time.size, self.fps, t)
        orig = [self._truth_orig(item, percentage, start, n) for item, _, start, n, _, percentage in planned]
        return {"spect": t["spect"], "spect_path": [p[1] for p in planned], "dataset": [p[0]["dataset"] for p in planned],
                "start_frame": [int(p[2]) for p in planned], "truth_beat": t["truth_beat"],
                "truth_downbeat": t["truth_downbeat"], "downbeat_mask": t["downbeat_mask"], "padding_mask": t["padding_mask"],
                "truth_orig_beat": [o[0] for o in orig], "truth_orig_downbeat": [o[1] for o in orig]}


class BatchLoader:
    """What the data module's ``*_dataloader()`` return: an iterable of ``dataset.batch(...)`` device batches.  ``shuffle``
    draws ONE ``np.random.permutation(len(dataset))`` when an iteration starts: the order is this class's own, not that of
    torch's RandomSampler, so an epoch visits the items in another order than the reference's DataLoader under the same
    seed (the items themselves follow the reference's draws)."""

    def __init__(self, dataset, batch_size=1, shuffle=False, drop_last=False, spect_dtype=torch.float32):
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, batch_size, shuffle, drop_last
        self.spect_dtype = spect_dtype

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        n = len(self.dataset)
        order = np.random.permutation(n) if self.shuffle else np.arange(n)
        for i in range(len(self)):
            yield self.dataset.batch(order[i * self.batch_size:(i + 1) * self.batch_size], spect_dtype=self.spect_dtype)

    def shard(self, rank: int, world: int) -> "ShardedBatchLoader":
        """This loader for rank ``rank`` of ``world`` data-parallel ranks: the same global sequence of batches, of which the
        rank builds every ``world``-th (``ShardedBatchLoader``)."""
        return ShardedBatchLoader(self, rank, world)


class ShardedBatchLoader:
    """A ``BatchLoader`` seen from one of ``world`` data-parallel ranks.  Every rank draws what the unsharded loader draws, in
    its order -- the permutation when an iteration starts, then every batch's plan (``BeatTrackingDataset.plan_batch``) -- so
    numpy's generator is in the single-process state on every rank after every batch.  Global batch ``j`` belongs to rank
    ``j % world``; only its owner builds it.  Iterating yields ``(j, batch)`` for the owned batches; ``len()`` is the GLOBAL
    number of batches."""

    def __init__(self, loader: BatchLoader, rank: int, world: int):
        rank, world = int(rank), int(world)
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"rank {rank} of a world of {world}")
        self.loader, self.rank, self.world = loader, rank, world

    def __len__(self):
        return len(self.loader)

    def _planned(self):
        """(j, owner, indices, planned) for every global batch; the draws happen as the iteration advances"""
        lo = self.loader
        n = len(lo.dataset)
        order = np.random.permutation(n) if lo.shuffle else np.arange(n)
        for j in range(len(lo)):
            indices = order[j * lo.batch_size:(j + 1) * lo.batch_size]
            yield j, j % self.world, indices, lo.dataset.plan_batch(indices)

    def iter_plans(self):
        """Host only: ``(j, owner, planned)`` for every global batch, in order, with all of an iteration's draws and no
        device work (what the rank would build is the entries with ``owner == rank``)."""
        for j, owner, _, planned in self._planned():
            yield j, owner, planned

    def __iter__(self):
        lo = self.loader
        for j, owner, indices, planned in self._planned():
            if owner == self.rank:
                yield j, lo.dataset.batch(indices, spect_dtype=lo.spect_dtype, planned=planned)


# the training sets of "Modeling Beats and Downbeats with a Time-Frequency Transformer" (Hung et al.)
_HUNG_PREFIXES = ("hainsworth/", "ballroom/", "hjdb/", "beatles/", "rwc/rwc_popular", "simac/", "smc/", "harmonix/")


class BeatDataModule:
    """The reference's data module as a plain class (no Lightning): cross-validation or single train / val / test splits
    over ``data_dir``.

    batch_size, train_length, augmentations, spect_fps, length_based_oversampling_factor: as in BeatTrackingDataset;
    num_workers: accepted and ignored (there are no worker processes: a batch is one kernel launch); test_dataset: the
    dataset held out for testing; hung_data: restrict training to the datasets of Hung et al.; no_val: train on train + val
    (validation still runs, on data seen in training); fold: cross-validation fold to validate on (None: the single split);
    predict_datasplit: "test", "train" or "val" -- whole pieces of that split for prediction."""

    def __init__(self, data_dir, batch_size=8, train_length=1500, num_workers=20,
                 augmentations={"pitch": {"min": -5, "max": 6}, "tempo": {"min": -20, "max": 20, "stride": 4}},
                 test_dataset="gtzan", hung_data=False, no_val=False, spect_fps=50, length_based_oversampling_factor=0,
                 fold=None, predict_datasplit="test", device="cuda", resident="auto"):
        if not set(augmentations.keys()).issubset(_SUPPORTED):
            raise ValueError(f"Unsupported augmentations: {augmentations.keys()}")
        self.initialized = {}
        self.data_dir = Path(data_dir)
        self.batch_size, self.train_length, self.num_workers = batch_size, train_length, num_workers
        self.augmentations = augmentations
        self.test_set_name = test_dataset
        self.hung_data, self.no_val = hung_data, no_val
        self.spect_fps = spect_fps
        self.length_based_oversampling_factor = length_based_oversampling_factor
        self.fold = fold
        self.predict_datasplit = predict_datasplit
        self.device, self.resident = device, resident

    @staticmethod
    def _read_split(path):
        """[(piece, part)] of a tab-separated split file; parts are integers when every one of them is (the fold files)"""
        rows = [line.rstrip("\r\n").split("\t") for line in open(path) if line.strip()]
        pieces, parts = [r[0] for r in rows], [r[1] if len(r) > 1 else "" for r in rows]
        try:
            parts = [int(p) for p in parts]
        except ValueError:
            pass
        return list(zip(pieces, parts))

    def _dataset(self, items, **kw):
        return BeatTrackingDataset(items, data_folder=self.data_dir, spect_fps=self.spect_fps, device=self.device,
                                   resident=self.resident, **kw)

    def setup(self, stage):
        if self.initialized.get(stage, False):
            return
        annotation_dir = self.data_dir / "annotations"
        if stage in ("fit", "validate"):
            self.val_items, self.train_items = [], []
            split_file = "8-folds.split" if self.fold is not None else "single.split"
            for dataset_dir in annotation_dir.iterdir():
                if not dataset_dir.is_dir() or not (dataset_dir / split_file).exists() or dataset_dir.name == self.test_set_name:
                    continue
                for piece, part in self._read_split(dataset_dir / split_file):
                    name = f"{dataset_dir.name}/{piece}"
                    if self.fold is not None:   # cross-validation: the given fold validates, the others train
                        (self.val_items if part == self.fold else self.train_items).append(name)
                    elif part == "val":
                        self.val_items.append(name)
                    elif part == "train":
                        self.train_items.append(name)
            if self.no_val:
                self.train_items.extend(self.val_items)
            if self.hung_data:
                # (as in the reference, the list ends in an EMPTY alternative: the pattern matches every item)
                pattern = re.compile("^(" + "|".join(_HUNG_PREFIXES) + "|).*$")
                self.train_items = [item for item in self.train_items if pattern.match(item)]
            self.val_items.sort()
            self.train_items.sort()
            self.val_dataset = self._dataset(self.val_items, deterministic=True, augmentations={}, train_length=self.train_length)
            print("Validation set:", len(self.val_dataset), "items from:", *sorted({i.split("/", 1)[0] for i in self.val_items}))
            self.initialized["validate"] = True
        if stage == "fit":
            self.train_dataset = self._dataset(self.train_items, deterministic=False, augmentations=self.augmentations,
                                               train_length=self.train_length,
                                               length_based_oversampling_factor=self.length_based_oversampling_factor)
            print("Training set:", len(self.train_dataset), "items from:", *sorted({i.split("/", 1)[0] for i in self.train_items}))
            self.initialized["fit"] = True
        if stage == "test":
            beats_dir = annotation_dir / self.test_set_name / "annotations" / "beats"
            self.test_items = sorted(f"{self.test_set_name}/{f.stem}" for f in beats_dir.glob("*.beats"))
            self.test_dataset = self._dataset(self.test_items, deterministic=True, augmentations={}, train_length=None)
            print("Test set:", len(self.test_dataset), "items from:", self.test_set_name)
            self.initialized["test"] = True
        if stage == "predict":
            if self.predict_datasplit == "test":
                self.setup("test")
                self.predict_dataset = self.test_dataset
            else:
                if self.predict_datasplit == "train":
                    self.setup("fit")
                    items = self.train_items
                elif self.predict_datasplit == "val":
                    self.setup("validate")
                    items = self.val_items
                self.predict_dataset = self._dataset(items, deterministic=True, augmentations={}, train_length=None)

    def train_dataloader(self):
        return BatchLoader(self.train_dataset, batch_size=self.batch_size, shuffle=True, drop_last=True)

    def val_dataloader(self):
        """(the middle excerpt of long pieces only, as in the reference)"""
        return BatchLoader(self.val_dataset, batch_size=self.batch_size)

    def test_dataloader(self):
        return BatchLoader(self.test_dataset, batch_size=1)

    def predict_dataloader(self):
        return BatchLoader(self.predict_dataset, batch_size=1)

    def get_train_positive_weights(self, widen_target_mask=3):
        """Negative over positive targets of the training set, per target kind, with ``widen_target_mask`` frames on each
        side of a positive one counted as neither (3: seven frames per annotation)."""
        ds = self.train_dataset
        frames = [len(ds._get_spect(item)) for item in ds.items]
        all_frames = sum(frames)
        all_frames_db = sum(f for f, item in zip(frames, ds.items) if item["downbeat_mask"])
        beats = sum(len(item["beat_value"]) for item in ds.items)
        downbeats = sum((item["beat_value"] == 1).sum() for item in ds.items if item["downbeat_mask"])
        ignored = widen_target_mask * 2 + 1
        return {"beat": int(np.round((all_frames - beats * ignored) / beats)),
                "downbeat": int(np.round((all_frames_db - downbeats * ignored) / downbeats))}
