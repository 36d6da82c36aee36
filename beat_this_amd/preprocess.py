"""Build training bundles from audio on the GPU: the reference's launch_scripts/preprocess_audio.py restated.

    python -m beat_this_amd.preprocess --orig_audio_paths data/audio_paths.csv --pitch_shift -5:6 --time_stretch 20:4

Flags, defaults and what ends up on disk are the reference's: per track ``<data>/audio/spectrograms/<dataset>/<stem>/`` with
``track.npy`` and the variants ``track_ps<k>.npy`` (pitch moved by k semitones) and ``track_ts<p>.npy`` (tempo changed by p
percent: the audio is 1 / (1 + p / 100) as long, which is what ``dataset.augment.stretch_annotations`` assumes), float16
(frames, 128) log-mel spectrograms at 50 frames per second, and one uncompressed ``<dataset>.npz`` per dataset with the members
``<stem>/<file>`` in the order of ``precomputed_augmentation_filenames`` (``gtzan`` without variants).

What differs is how the variants are made.  The reference writes 23 intermediate WAV files per track with pedalboard (Rubber
Band) and reads them back; here nothing intermediate is written: the mono signal goes to the device once, is brought to
44.1 kHz by the rational resampler, stretched or shifted there by csrc/stretch.hip (a phase vocoder with identity phase
locking, defined in include/beat_this_amd.h -- NOT Rubber Band: the variants sound alike, their samples differ), halved to
22.05 kHz and turned into the log-mel spectrogram.  ``track.npy`` is exactly ``Audio2Frames.signal2spect`` of the file.
A track's variants run back to back on one stream; their results travel to pinned host memory behind them and ONE writer
thread saves them while the device works on the next track.
"""
from __future__ import annotations

import argparse
import csv
import re
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from zipfile import ZIP_STORED, ZipFile

import numpy as np
import torch

from . import _lib
from .dataset.augment import precomputed_augmentation_filenames
from .inference import resample_gpu
from .preprocessing import LogMelSpect, load_audio, pitch_shift, time_stretch

OUT_SR, AUG_SR = 22050, 44100
SKIPPED_STEMS = ("gtzan_speech", "gtzan_music_")


def ints(value):
    """``"LOW:HIGH"`` / ``"MAX:STRIDE"`` -> tuple of ints; an empty string switches the augmentation off (None)"""
    return tuple(int(v) for v in value.split(":")) if value else None


def augmentations_of(pitch, stretch) -> dict:
    """the augmentation dictionary (``dataset.augment``'s format) of ``--pitch_shift`` / ``--time_stretch`` tuples"""
    aug = {}
    if pitch:
        aug["pitch"] = {"min": pitch[0], "max": pitch[1]}
    if stretch:
        aug["tempo"] = {"min": -stretch[0], "max": stretch[0], "stride": stretch[1] if len(stretch) > 1 else 1}
    return aug


def read_audio_paths(path) -> dict:
    """rows ``dataset_name,audio_dir`` -> {dataset_name: audio_dir}"""
    with open(path, newline="") as f:
        return {row[0].strip(): row[1].strip() for row in csv.reader(f) if len(row) >= 2 and row[0].strip()}


def save_spectrogram(path: Path, spect: np.ndarray) -> None:
    try:
        np.save(path, np.asarray(spect, dtype=np.float16))
    except BaseException:
        path.unlink(missing_ok=True)   # no half-written files
        raise


def variant_of(name: str):
    """``track_ps-3.npy`` -> ("pitch", -3); ``track_ts8.npy`` -> ("tempo", 8); ``track.npy`` -> (None, 0)"""
    stem = Path(name).stem
    if "_ps" in stem:
        return "pitch", int(stem.split("_ps")[1])
    if "_ts" in stem:
        return "tempo", int(stem.split("_ts")[1])
    return None, 0


def length_factor(name: str) -> float:
    """how much longer the 44.1 kHz signal gets inside the stretcher for this file (a pitch shift is undone by its resampler)"""
    kind, amount = variant_of(name)
    return 2.0 ** (amount / 12.0) if kind == "pitch" else 1.0 / (1.0 + amount / 100.0) if kind == "tempo" else 0.0


def max_stretched_length(n: int, sr: int, names) -> int:
    """the longest signal, in or out, that the stretcher sees for these files of an n-sample track at ``sr`` (0: no variant)"""
    n44 = -(-n * AUG_SR // sr)
    return max([int(n44 * max(length_factor(name), 1.0)) + 1 for name in names if variant_of(name)[0]] or [0])


class Preprocessor:
    def __init__(self, data_dir="data", pitch=(-5, 6), stretch=(20, 4), device="cuda", verbose=False):
        self.audio_dir = Path(data_dir) / "audio"
        self.spect_dir = self.audio_dir / "spectrograms"
        self.annotation_dir = Path(data_dir) / "annotations"
        if not self.annotation_dir.exists():
            raise RuntimeError(f"{self.annotation_dir} missing: the beat annotations decide which pieces are processed")
        self.augmentations = augmentations_of(pitch, stretch)
        self.device = torch.device(device)
        self.logmel = LogMelSpect(device=self.device)
        self.verbose = verbose
        self.written = 0

    def filenames(self, dataset_name):
        return precomputed_augmentation_filenames({} if dataset_name == "gtzan" else self.augmentations)

    def spectrograms(self, signal: np.ndarray, sr: int, names):
        """mono float signal -> {file name: (frames, 128) float16 device tensor}, everything enqueued on the current stream"""
        out = {}
        x = torch.tensor(signal, dtype=torch.float32, device=self.device)
        if "track.npy" in names:   # (Audio2Frames.signal2spect)
            out["track.npy"] = self.logmel(resample_gpu(x, sr, OUT_SR) if sr != OUT_SR else x).to(torch.float16)
        if any(n != "track.npy" for n in names):
            x44 = resample_gpu(x, sr, AUG_SR) if sr != AUG_SR else x
            for name in names:
                kind, amount = variant_of(name)
                if kind is None:
                    continue
                y = pitch_shift(x44, amount) if kind == "pitch" else time_stretch(x44, 1.0 + amount / 100.0)
                out[name] = self.logmel(resample_gpu(y, AUG_SR, OUT_SR)).to(torch.float16)
        return out

    def process_file(self, dataset_name, audio_path: Path, writer):
        """-> None (skipped) or the future of the track's file writes"""
        beat_path = self.annotation_dir / dataset_name / "annotations" / "beats" / (audio_path.stem + ".beats")
        if not beat_path.exists():
            print(f"{audio_path}: no annotations ({beat_path} is missing), piece left out")
            return None
        folder = self.spect_dir / dataset_name / audio_path.stem
        todo = [n for n in self.filenames(dataset_name) if not (folder / n).exists()]
        if not todo:
            if self.verbose:
                print(f"{folder}: complete, nothing to do")
            return None
        try:
            signal, sr = load_audio(audio_path)
        except Exception as e:
            print(f"{audio_path}: cannot be decoded ({e}), piece left out")
            return None
        if signal.ndim != 1:
            signal = signal.mean(1)
        longest = max_stretched_length(len(signal), int(sr), todo)
        if longest > _lib.STRETCH_MAX_SAMPLES:
            print(f"{audio_path} is too long for its variants ({longest} samples at {AUG_SR} Hz, the limit is "
                  f"{_lib.STRETCH_MAX_SAMPLES}): piece left out")
            return None
        folder.mkdir(parents=True, exist_ok=True)
        if self.verbose:
            print(f"Computing {len(todo)} spectrograms in {folder}")
        with torch.cuda.device(self.device):
            dev = self.spectrograms(signal, int(sr), todo)
            host = {n: torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True) for n, t in dev.items()}
            done = torch.cuda.Event()
            done.record()

        def write():
            done.synchronize()
            for n, t in host.items():
                save_spectrogram(folder / n, t.numpy())
            return len(host)

        return writer.submit(write)

    def run(self, audio_dirs: dict):
        print("Computing spectrograms ...")
        processed, pending = 0, None
        with ThreadPoolExecutor(max_workers=1) as writer:   # (one thread: the disk, not the CPU count, is what it waits for)
            for dataset_name, audio_dir in audio_dirs.items():
                for audio_path in sorted(Path(audio_dir).iterdir()):
                    if audio_path.stem[:12] in SKIPPED_STEMS or not audio_path.is_file():
                        continue
                    fut = self.process_file(dataset_name, audio_path, writer)
                    if pending is not None:   # (at most one track's results wait in pinned memory)
                        self.written += pending.result()
                        processed += 1
                    pending = fut
            if pending is not None:
                self.written += pending.result()
                processed += 1
        print(f"{processed} pieces done, {self.written} spectrograms written to {self.spect_dir}")

    def create_bundles(self):
        print("Writing one bundle per dataset ...")
        if not self.spect_dir.exists():
            return
        for spect_dir in sorted(c for c in self.spect_dir.iterdir() if c.is_dir()):
            create_npz(spect_dir, spect_dir.with_suffix(".npz"), self.filenames(spect_dir.name), self.verbose)


def create_npz(spect_dir: Path, npz_file: Path, filenames, verbose=False) -> bool:
    """the spectrograms of one dataset as one uncompressed .npz, members ``<stem>/<file>``; an existing bundle is kept"""
    if npz_file.exists():
        if verbose:
            print(f"{npz_file}: kept as it is")
        return False
    try:
        with ZipFile(npz_file, "w", compression=ZIP_STORED) as z:
            for piece in sorted(d for d in spect_dir.iterdir() if d.is_dir()):
                for name in filenames:
                    z.write(piece / name, arcname=f"{piece.name}/{name}")
    except BaseException:
        npz_file.unlink(missing_ok=True)
        raise
    return True


def main(argv=None) -> int:
    parser = argparse.ArgumentParser(prog="python -m beat_this_amd.preprocess", description=__doc__.split("\n\n")[0])
    parser.add_argument("--orig_audio_paths", type=str, default="data/audio_paths.csv",
                        help="CSV file with one row `dataset_name,audio_dir` per dataset (default: %(default)s)")
    parser.add_argument("--pitch_shift", metavar="LOW:HIGH", type=str, default="-5:6",
                        help="lowest and highest pitch shift in semitones, both included; \"\" for none (default: %(default)s)")
    parser.add_argument("--time_stretch", metavar="MAX:STRIDE", type=str, default="20:4",
                        help="largest tempo change in percent, either way, and the step between changes; \"\" for none (default: %(default)s)")
    parser.add_argument("--data-dir", type=str, default="data",
                        help="directory holding annotations/ and receiving audio/spectrograms/ (default: %(default)s)")
    parser.add_argument("--verbose", action="store_true", help="say what is computed and what is skipped")
    # (`--pitch_shift -5:6`: argparse takes a value that starts with a minus sign and is no number for an option)
    argv, joined = list(sys.argv[1:] if argv is None else argv), []
    for a in argv:
        if joined and joined[-1] in ("--pitch_shift", "--time_stretch") and re.fullmatch(r"-?\d+(:-?\d+)*", a):
            joined[-1] += "=" + a
        else:
            joined.append(a)
    args = parser.parse_args(joined)
    pre = Preprocessor(args.data_dir, ints(args.pitch_shift), ints(args.time_stretch), verbose=args.verbose)
    pre.run(read_audio_paths(args.orig_audio_paths))
    pre.create_bundles()
    return 0


if __name__ == "__main__":
    sys.exit(main())
