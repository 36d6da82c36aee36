"""The reference's beat_this/dataset/augment.py restated on this package's training-batch kernel.

The pitch / tempo helpers choose among PRECOMPUTED spectrograms and rescale the annotations; they are host code on a few
numbers.  The mask augmentation is different here: ``plan_mask`` draws the reference's random decisions (the same
``np.random`` calls in the same order, so a seed gives the reference's result) into a list of operations, and the frames are
moved by csrc/data.hip as a gather -- ``augment_mask_`` on a CUDA tensor is one scratch copy and one launch, on a numpy array
(or a CPU tensor) it runs the library's bit-identical host twin.  Spectrograms are (frames, 128), float16 or float32.

``number_of_precomputed_augmentations`` of the reference is left out on purpose: it unpacks ``augmentations.values()`` into
(method, params) pairs, which fails for every dict the other functions accept (the values are the parameter dicts), so it has
no behaviour to mirror.  ``len(precomputed_augmentation_filenames(augmentations))`` is the count it was meant to give."""
from __future__ import annotations

import numpy as np

from . import plan as P


def augment_pitchtempo(item, augmentations):
    """One randomly chosen pitch shift or tempo change: the item with its ``spect_path`` (and, for tempo, its ``beat_time``)
    replaced.  With both kinds enabled a coin picks one of them."""
    pitch, tempo = augmentations.get("pitch"), augmentations.get("tempo")
    if "pitch" in augmentations and "tempo" in augmentations:
        return augment_pitch(item, pitch) if np.random.randint(2) == 0 else augment_tempo(item, tempo)
    if "pitch" in augmentations:
        return augment_pitch(item, pitch)
    if "tempo" in augmentations:
        return augment_tempo(item, tempo)
    return item


def augment_pitch(item, pitch_params):
    semitones = P.draw_pitch(pitch_params)
    return shift_annotations(shift_filename(item, semitones), semitones)


def augment_tempo(item, tempo_params):
    percentage = P.draw_tempo(tempo_params)
    return stretch_annotations(stretch_filename(item, percentage), percentage)


def stretch_annotations(item, percentage):
    """beat times of a piece whose TEMPO changed by ``percentage`` percent"""
    if not percentage:
        return item
    return {**item, "beat_time": P.stretched(item["beat_time"], percentage)}


def shift_annotations(item, semitones):
    """(a pitch shift moves no beat)"""
    return item


def _renamed(item, suffix):
    path = item["spect_path"]
    return {**item, "spect_path": path.with_stem(path.stem + suffix) if suffix else path}


def stretch_filename(item, percentage):
    return _renamed(item, f"_ts{percentage}" if percentage else "")


def shift_filename(item, semitones):
    return _renamed(item, f"_ps{semitones}" if semitones else "")


def precomputed_augmentation_filenames(augmentations, ext="npy"):
    """File names of every precomputed variant the augmentations can choose: the unmodified track first, then per key of
    ``augmentations`` in its order the pitch shifts min .. max and the tempo changes min .. max by stride (0 left out)."""
    return [f"track{suffix}.{ext}" for suffix in P.variant_suffixes(augmentations)]


def apply_mask_excerpt(excerpt, kind, min_parts, max_parts):
    """One mask operation in place on ``excerpt`` (numpy array or torch tensor, frames first): "zero" clears it, "permute"
    cuts it at randomly chosen frames into min_parts .. max_parts parts (at most one more than it has frames) and reorders
    them randomly."""
    op = P.draw_mask_op(len(excerpt), 0, kind, min_parts, max_parts)
    if op.kind == P.ZERO:
        excerpt[:] = 0
        return
    source = np.concatenate([np.arange(old, old + size) for _, old, size in op.parts] or [np.zeros(0, np.int64)])
    if isinstance(excerpt, np.ndarray):
        excerpt[:] = excerpt[source]
    else:
        import torch

        excerpt[:] = excerpt[torch.as_tensor(source, device=excerpt.device)]


def augment_mask_(spect, augmentations: dict, fps: int):
    """Apply the "mask" augmentation in place and return ``spect``: min_count .. max_count times, a stretch of min_len ..
    max_len seconds at a random position is zeroed (kind "zero") or cut into min_parts .. max_parts parts that are reordered
    (kind "permute").  Without a "mask" key nothing happens.  A mask not shorter than the spectrogram raises ValueError."""
    if "mask" not in augmentations:
        return spect
    ops = P.plan_mask(len(spect), augmentations["mask"], fps)
    P.apply_ops_(spect, ops)
    return spect
