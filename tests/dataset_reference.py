"""What tests/test_dataset.py and tests/test_gpu_dataset.py share: the seeded synthetic data folder (also what
tools/make_dataset_golden.py runs the reference over -- no spectrogram is committed), the list of recorded cases, and a plain
numpy restatement of one training item: the mask operations applied one after the other in place, the framewise targets by
np.round and comparisons."""
import json
import os

import numpy as np

DATA_SEED = 20240
FPS = 50
TRAIN_LENGTH = 150
PITCH = {"min": -5, "max": 6}
TEMPO = {"min": -20, "max": 20, "stride": 4}
MASK_PERMUTE = {"kind": "permute", "min_count": 1, "max_count": 6, "min_len": 0.1, "max_len": 2, "min_parts": 5, "max_parts": 9}
MASK_ZERO = dict(MASK_PERMUTE, kind="zero")
MASK_TINY = dict(MASK_PERMUTE, min_len=0.04, max_len=0.06)   # 2 .. 3 frames: 5 .. 9 parts are clamped to length + 1
MASK_SHORT = dict(MASK_PERMUTE, max_len=1)                   # masks that fit a piece of 97 frames
SEEDS = (0, 2, 5, 7)   # np.random seeds per case: no shift, a positive one, two negative ones

# piece -> (dataset, frames, bundle or loose files, every precomputed variant or the plain track only)
PIECES = {
    "a_long": ("alpha", 400, "bundle", True),
    "a_exact": ("alpha", TRAIN_LENGTH, "bundle", True),
    "a_plus1": ("alpha", TRAIN_LENGTH + 1, "bundle", True),
    "a_short": ("alpha", 97, "bundle", True),
    "a_plain": ("alpha", 260, "bundle", False),
    "b_one": ("beta", 300, "loose", True),
    "b_two": ("beta", 220, "loose", False),
    "rwc_popular_001": ("rwc", 333, "bundle", True),
    "rwc_jazz_002": ("rwc", 180, "bundle", True),
    "g_1": ("gtzan", 210, "bundle", False),
    "g_2": ("gtzan", 175, "bundle", False),
}
HAS_DOWNBEATS = {"alpha": True, "beta": False, "rwc": True, "gtzan": True}
SINGLE_SPLIT = {"a_long": "train", "a_exact": "val", "a_plus1": "train", "a_short": "train", "a_plain": "val", "b_one": "train",
                "b_two": "val", "rwc_popular_001": "train", "rwc_jazz_002": "val", "g_1": "train", "g_2": "val"}

ALPHA = ["alpha/a_long", "alpha/a_exact", "alpha/a_plus1", "alpha/a_short"]
# name -> (item names, dataset arguments, index of the item)
CASES = {
    "longer": (ALPHA, dict(train_length=TRAIN_LENGTH), 0),
    "exact": (ALPHA, dict(train_length=TRAIN_LENGTH), 1),
    "plus1": (ALPHA, dict(train_length=TRAIN_LENGTH), 2),
    "shorter_padded": (ALPHA, dict(train_length=TRAIN_LENGTH), 3),
    "deterministic": (ALPHA, dict(train_length=TRAIN_LENGTH, deterministic=True), 0),
    "deterministic_plus1": (ALPHA, dict(train_length=TRAIN_LENGTH, deterministic=True), 2),
    "whole_piece": (ALPHA, dict(train_length=None), 0),
    "pitch": (ALPHA, dict(train_length=TRAIN_LENGTH, augmentations={"pitch": PITCH}), 0),
    "tempo": (ALPHA, dict(train_length=TRAIN_LENGTH, augmentations={"tempo": TEMPO}), 0),
    "pitch_tempo": (ALPHA, dict(train_length=TRAIN_LENGTH, augmentations={"pitch": PITCH, "tempo": TEMPO}), 0),
    "pitch_tempo_short": (ALPHA, dict(train_length=TRAIN_LENGTH, augmentations={"tempo": TEMPO, "pitch": PITCH}), 3),
    "mask_permute": (ALPHA, dict(train_length=TRAIN_LENGTH, augmentations={"mask": MASK_PERMUTE}), 0),
    "mask_permute_short": (ALPHA, dict(train_length=TRAIN_LENGTH, augmentations={"mask": MASK_SHORT}), 3),
    "mask_zero": (ALPHA, dict(train_length=TRAIN_LENGTH, augmentations={"mask": MASK_ZERO}), 2),
    "mask_clamped_parts": (ALPHA, dict(train_length=TRAIN_LENGTH, augmentations={"mask": MASK_TINY}), 0),
    "everything": (ALPHA, dict(train_length=TRAIN_LENGTH, augmentations={"pitch": PITCH, "tempo": TEMPO, "mask": MASK_PERMUTE}), 0),
    "one_column_no_downbeats": (["beta/b_one", "beta/b_two"], dict(train_length=TRAIN_LENGTH), 0),
    "no_downbeats_tempo": (["beta/b_one"], dict(train_length=TRAIN_LENGTH, augmentations={"tempo": TEMPO}), 0),
    "rwc_stem": (["rwc/rwc_popular_001", "rwc/rwc_jazz_002"], dict(train_length=TRAIN_LENGTH), 1),
}
# BeatDataModule arguments of the recorded setups
SETUPS = {"single": {}, "fold2": {"fold": 2}, "no_val": {"no_val": True}, "hung": {"hung_data": True}}
OVERSAMPLING = (0.65, 2)


def variant_lengths(frames):
    """suffix -> frames of every precomputed variant of a piece (a tempo change of p percent shortens it by 1 + p / 100)"""
    out = {"": frames}
    for s in range(PITCH["min"], PITCH["max"] + 1):
        if s:
            out[f"_ps{s}"] = frames
    for p in range(TEMPO["min"], TEMPO["max"] + 1, TEMPO["stride"]):
        if p:
            out[f"_ts{p}"] = int(round(frames / (1 + p / 100)))
    return out


def spectrogram(rng, frames):
    """float16 (frames, 128): column 0 holds the row number (exact in float16 up to 2048), the rest seeded values"""
    a = rng.standard_normal((frames, 128)).astype(np.float16)
    a[:, 0] = np.arange(frames)
    return a


def build_data_folder(root, seed=DATA_SEED):
    """write the synthetic data folder (annotations, splits, float16 bundles and loose files) under ``root``"""
    rng = np.random.default_rng(seed)
    bundles = {}
    for fold, (piece, (dataset, frames, kind, all_variants)) in enumerate(PIECES.items()):
        ann_dir = os.path.join(root, "annotations", dataset)
        os.makedirs(os.path.join(ann_dir, "annotations", "beats"), exist_ok=True)
        with open(os.path.join(ann_dir, "info.json"), "w") as f:
            json.dump({"has_downbeats": HAS_DOWNBEATS[dataset]}, f)
        with open(os.path.join(ann_dir, "single.split"), "a") as f:
            f.write(f"{piece}\t{SINGLE_SPLIT[piece]}\n")
        with open(os.path.join(ann_dir, "8-folds.split"), "a") as f:
            f.write(f"{piece}\t{fold % 8}\n")
        times = np.cumsum(rng.uniform(0.31, 0.62, 2 * frames // 25 + 4)) - 0.2
        times = times[(times > 0.0) & (times < (frames + 10) / FPS)]
        with open(os.path.join(ann_dir, "annotations", "beats", piece + ".beats"), "w") as f:
            for i, t in enumerate(times):
                f.write(f"{t:.6f}\n" if not HAS_DOWNBEATS[dataset] else f"{t:.6f}\t{i % 4 + 1}\n")
        for suffix, n in variant_lengths(frames).items():
            if suffix and not all_variants:
                continue
            a = spectrogram(rng, n)
            if kind == "bundle":
                bundles.setdefault(dataset, {})[f"{piece}/track{suffix}"] = a
            else:
                os.makedirs(os.path.join(root, "audio", "spectrograms", dataset, piece), exist_ok=True)
                np.save(os.path.join(root, "audio", "spectrograms", dataset, piece, f"track{suffix}.npy"), a)
    for dataset, members in bundles.items():
        os.makedirs(os.path.join(root, "audio", "spectrograms"), exist_ok=True)
        np.savez(os.path.join(root, "audio", "spectrograms", dataset + ".npz"), **members)
    return root


# ---- one item, restated in numpy --------------------------------------------------------------------------------------------------
def apply_ops(excerpt, ops):
    """mask operations in their order, in place: (start, length, kind 0 zero / 1 permute, parts [(new offset, old offset,
    frames)])"""
    for start, length, kind, parts in ops:
        window = excerpt[start:start + length]
        if kind == 0:
            window[:] = 0
        else:
            old = window.copy()
            for new, src, size in parts:
                window[new:new + size] = old[src:src + size]
    return excerpt


def item(spect, start, n, L, ops, beat_time, beat_value, fps=FPS, out_dtype=None):
    """-> spect (L, 128), truth_beat, truth_downbeat, padding_mask (L,) bool of one item: frames [start, start + n) of
    ``spect``, masked, padded with zeros to L"""
    out = np.zeros((L, spect.shape[1]), out_dtype or spect.dtype)
    out[:n] = apply_ops(np.array(spect[start:start + n]), ops).astype(out.dtype)
    frame = np.round(np.asarray(beat_time, np.float64) * fps) - start
    keep = (frame >= 0) & (frame < n)
    beat, down = np.zeros(L, bool), np.zeros(L, bool)
    beat[frame[keep].astype(np.int64)] = True
    down[frame[keep & (np.asarray(beat_value) == 1)].astype(np.int64)] = True
    return out, beat, down, np.arange(L) < n


def random_ops(rng, n):
    """overlapping zero and permute operations on an excerpt of n frames, in the restatement's form"""
    ops = []
    for _ in range(int(rng.integers(0, 7))):
        length = int(rng.integers(0, n))
        start = int(rng.integers(0, n - length))
        if rng.random() < 0.3:
            ops.append((start, length, 0, ()))
            continue
        count = min(int(rng.integers(1, 10)), length + 1)
        cuts = np.sort(rng.choice(length, count - 1, replace=False)) if length else np.zeros(0, np.int64)
        bounds = [0, *cuts.tolist(), length]
        parts, new = [], 0
        for j in rng.permutation(count).tolist():
            if bounds[j + 1] > bounds[j]:
                parts.append((new, bounds[j], bounds[j + 1] - bounds[j]))
                new += bounds[j + 1] - bounds[j]
        ops.append((start, length, 1, tuple(parts)))
    return ops
