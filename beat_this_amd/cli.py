#!/usr/bin/env python3
"""Command line front end with the option surface of the reference's ``beat_this`` console script
(beat_this/cli.py:22-191): same positional inputs and flags, same output-path rules, same ``.beats`` TSV and
``--activations`` ``.npy`` outputs -- running on the MI355X kernels.  SURVEY.md section 8(f3).

Differences: ``--gpu -1`` (CPU) is refused, there is no CPU path in this package; with a ROCm device present
``--gpu N`` selects ``cuda:N`` exactly like the reference.

Extensions, both opt-in: ``--device-decode`` decodes PCM WAV and FLAC files on the GPU (csrc/pcm.hip, csrc/flac.hip; any other file
is decoded as before), ``--batch N`` processes up to N files per batch through ``File2Beats.many_async``.  Without them the loop below is
the reference's.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

OPTIONS = (
    # flags, kwargs  (help texts paraphrase the reference's --help)
    (("--model",), dict(type=str, default="final0", help="checkpoint name, path or URL (default: %(default)s)")),
    (("--output", "-o"), dict(type=str, default=None,
                              help="output file (single input) or output directory (several inputs); default: next "
                                   "to each input, see --suffix / --append")),
    (("--suffix", "-s"), dict(type=str, default=".beats", help="output suffix (default: %(default)s)")),
    (("--append",), dict(action="store_true", help="append the suffix instead of replacing the input's suffix")),
    (("--skip-existing",), dict(action="store_true", help="do not overwrite existing outputs")),
    (("--touch-first",), dict(action="store_true",
                              help="create the (empty) output before processing: with --skip-existing several "
                                   "processes can share one file set")),
    (("--dbn",), dict(default=False, action=argparse.BooleanOptionalAction, help="madmom DBN post-processing")),
    (("--gpu",), dict(type=int, default=0, help="index of the GPU to use (default: %(default)s)")),
    (("--float16",), dict(action="store_true", help="half-precision path: fp16 MFMA operands, fp32 accumulation (float16=True of the Python API)")),
    (("--activations",), dict(action="store_true", help="also save the raw logits as .npy")),
    # extensions (absent from the parsed arguments unless given: ``run``'s defaults are today's behaviour)
    (("--device-decode",), dict(action="store_true", default=argparse.SUPPRESS,
                                help="decode PCM WAV and FLAC files on the GPU (any other file is decoded as before)")),
    (("--batch",), dict(type=int, default=argparse.SUPPRESS, metavar="N",
                        help="process up to N files per batch: files of batch i + 1 are read while batch i computes (default: 1)")),
)
BATCH_MAX_BYTES = 1 << 30     # file bytes per batch (two batches are in flight: their PCM bytes sit in pinned host memory)
BATCH_MAX_FRAMES = 1 << 22    # 50 fps frames per batch (23 hours; a 2 GiB spectrogram): far below the 32-bit limit of a batch


def get_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Detect beats and downbeats in audio files (Beat This!, MI355X kernels).")
    parser.add_argument("inputs", type=str, nargs="+", help="audio files and/or directories of audio files")
    for flags, kwargs in OPTIONS:
        parser.add_argument(*flags, **kwargs)
    return parser


def derive_output_path(input_path: Path, suffix: str, append: bool, output: Path | None = None,
                       parent: Path | None = None) -> Path:
    """Where the result of ``input_path`` goes (cli.py:94-112): next to the input, or under ``output`` keeping
    the path relative to the directory ``parent`` given on the command line; the suffix replaces the input's
    suffix unless ``append``."""
    if output is None:
        target = input_path
    else:
        target = output / (input_path.relative_to(parent) if parent is not None else input_path.name)
    return target.parent / (target.name + suffix) if append else target.with_suffix(suffix)


def collect_tasks(inputs, output, suffix, append, skip_existing):
    """[(audio file, output file)] for files and (recursively) directories, cli.py:163-176."""
    tasks = []
    for item in inputs:
        if item.is_dir():
            for fn in sorted(item.rglob("*")):
                if fn.is_dir() or fn.name.endswith(suffix):
                    continue
                dest = derive_output_path(fn, suffix, append, output, parent=item)
                if skip_existing and dest.exists():
                    continue
                tasks.append((fn, dest))
        else:
            tasks.append((item, derive_output_path(item, suffix, append, output)))
    return tasks


def batch_cost(audiofile: Path):
    """(file bytes, an upper estimate of the 50 fps frames) of one input, for the caps of a batch: exact for a PCM WAV file,
    the decoded PCM bytes for a FLAC file the device decodes; for anything else 50 frames per kilobyte (an 8 kbit/s stream), so that the byte cap bounds the frames as well"""
    from . import flac, wav

    info = wav.probe(audiofile)
    if info is not None:
        return info.data_bytes, 50 * info.n_frames // info.sample_rate + 2
    info = flac.probe(audiofile)
    if info is not None:      # (the bytes it decodes to, not the file's: the workspace holds the decoded integers)
        return info.decoded_bytes, 50 * info.total_samples // info.sample_rate + 2
    try:
        size = audiofile.stat().st_size
    except OSError:
        size = 0
    return size, size // 20 + 2


def cut_batches(items, batch: int, max_bytes: int = BATCH_MAX_BYTES, max_frames: int = BATCH_MAX_FRAMES):
    """``items``: an iterable of (item, bytes, frames) -> consecutive runs [item], as a generator that takes an item only when
    its batch is being formed: at most ``batch`` files, ``max_bytes`` and ``max_frames`` per run; a single file above a cap
    goes alone."""
    cur, nb, nf = [], 0, 0
    for item, b, f in items:
        if cur and (len(cur) >= batch or nb + b > max_bytes or nf + f > max_frames):
            yield cur
            cur, nb, nf = [], 0, 0
        cur.append(item)
        nb, nf = nb + b, nf + f
    if cur:
        yield cur


def run(inputs, model, output, suffix, append, skip_existing, touch_first, dbn, gpu, float16, activations,
        device_decode=False, batch=1):
    from .inference import File2File, load_audio
    from .utils import save_beat_tsv

    if gpu < 0 or not torch.cuda.is_available():
        raise SystemExit("beat_this_amd needs a ROCm GPU (there is no CPU path in this package)")
    if batch < 1:
        raise SystemExit("--batch needs a positive number of files")
    file2file = File2File(model, torch.device(f"cuda:{gpu}"), float16, dbn, **({"device_decode": True} if device_decode else {}))

    def process(audiofile: Path, outfile: Path):
        if not activations:
            return file2file(audiofile, outfile)
        wave = file2file.file2wave(audiofile) if device_decode else None
        signal, sr = wave if wave is not None else load_audio(audiofile)
        beat_logits, downbeat_logits = file2file.spect2frames(file2file.signal2spect(signal, sr))
        np.save(outfile.with_suffix(".npy"), np.vstack([beat_logits.cpu().numpy(), downbeat_logits.cpu().numpy()]))
        beats, downbeats = file2file.frames2beats(beat_logits, downbeat_logits)
        save_beat_tsv(beats, downbeats, outfile)

    inputs = [Path(p) for p in inputs]
    output = Path(output) if output is not None else None
    if len(inputs) == 1 and not inputs[0].is_dir():  # single file: --output may name the file itself
        dest = output if output is not None and not output.is_dir() else derive_output_path(inputs[0], suffix, append, output)
        process(inputs[0], dest)
        return
    tasks = collect_tasks(inputs, output, suffix, append, skip_existing)
    try:
        import tqdm
        tasks = tqdm.tqdm(tasks)
    except ImportError:
        pass

    def claim(dest: Path) -> bool:
        if touch_first:
            try:
                dest.touch(exist_ok=not skip_existing)
            except FileExistsError:
                return False
        elif skip_existing and dest.exists():
            return False
        return True

    def process_or_report(audiofile: Path, dest: Path):
        try:
            process(audiofile, dest)
        except Exception:  # keep going, like the reference (cli.py:185-191)
            print(f'Could not process "{audiofile}". Rerun with this file alone for details.', file=sys.stderr)

    if batch == 1:
        for audiofile, dest in tasks:
            if claim(dest):
                process_or_report(audiofile, dest)
        return

    # --batch N: File2Beats.many_async per batch; batch i + 1 is read and submitted before batch i's result is collected, so
    # the host's file reads and the write-out overlap the GPU's work.  Anything that raises in a batch sends that batch's
    # files through ``process`` one at a time: outputs and messages are then exactly those of the loop above.
    def submit(items):
        try:
            return file2file.many_async([a for a, _ in items])
        except Exception:
            return None

    def collect(items, handle):
        try:
            if handle is None:
                raise RuntimeError("the batch was not submitted")
            results = handle.result()
            if activations:
                beat, down, off = handle.logits
                beat, down = beat.cpu().numpy(), down.cpu().numpy()
        except Exception:
            for audiofile, dest in items:
                process_or_report(audiofile, dest)
            return
        for k, (audiofile, dest) in enumerate(items):
            try:
                if activations:
                    np.save(dest.with_suffix(".npy"), np.vstack([beat[off[k]: off[k + 1]], down[off[k]: off[k + 1]]]))
                save_beat_tsv(results[k][0], results[k][1], dest)
            except Exception:
                print(f'Could not process "{audiofile}". Rerun with this file alone for details.', file=sys.stderr)

    claimed = (((audiofile, dest), *batch_cost(audiofile)) for audiofile, dest in tasks if claim(dest))   # (claimed as its batch forms)
    pending = None
    for items in cut_batches(claimed, batch):
        handle = submit(items)
        if pending is not None:
            collect(*pending)
        pending = (items, handle)
    if pending is not None:
        collect(*pending)


def main():
    run(**vars(get_parser().parse_args()))


if __name__ == "__main__":
    sys.exit(main())
