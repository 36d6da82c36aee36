"""PCM WAV files as they lie on disk, for the device decoder (csrc/pcm.hip): ``probe`` reads the header and says where the
samples are and what they look like -- or None, which always means "take ``load_audio`` as before" -- and ``read_raw`` puts the
file's bytes, unconverted, into a caller-supplied (pinned) buffer.  Nothing here touches the GPU or converts a sample.
"""
from __future__ import annotations

import os
import struct
from typing import NamedTuple

from ._lib import (PCM_F32, PCM_F64, PCM_MAX_CHANNELS_FLOAT, PCM_MAX_CHANNELS_INT, PCM_S16, PCM_S24, PCM_S32, PCM_SAMPLE_BYTES,
                   PCM_U8)

WINDOW = 16   # the kernel reads whole aligned 16-byte windows around the payload (include/beat_this_amd.h)
_TAG_PCM, _TAG_FLOAT, _TAG_EXTENSIBLE = 1, 3, 0xFFFE
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")   # KSDATAFORMAT_SUBTYPE_*: the tag in the first two bytes, then this
_INT_FORMATS = {8: PCM_U8, 16: PCM_S16, 24: PCM_S24, 32: PCM_S32}
_FLOAT_FORMATS = {32: PCM_F32, 64: PCM_F64}


class PcmInfo(NamedTuple):
    """What ``probe`` found: ``format`` (BT_PCM_*), ``channels``, ``sample_rate``, the byte offset of the first sample in the
    file and the number of frames (samples per channel)."""
    format: int
    channels: int
    sample_rate: int
    data_offset: int
    n_frames: int

    @property
    def frame_bytes(self) -> int:
        return self.channels * PCM_SAMPLE_BYTES[self.format]

    @property
    def data_bytes(self) -> int:
        return self.n_frames * self.frame_bytes

    @property
    def raw_span(self):
        """(first file byte, byte count, offset of the payload in it): the aligned 16-byte windows that enclose the payload"""
        lo = self.data_offset // WINDOW * WINDOW
        hi = -(-(self.data_offset + self.data_bytes) // WINDOW) * WINDOW
        return lo, hi - lo, self.data_offset - lo


def _parse_fmt(body: bytes):
    """the ``fmt `` chunk -> (format code, channels, sample rate, block align), or None for anything but plain PCM / IEEE float"""
    if len(body) < 16:
        return None
    tag, channels, rate, _, align, bits = struct.unpack("<HHIIHH", body[:16])
    if tag == _TAG_EXTENSIBLE:
        if len(body) < 40 or struct.unpack("<H", body[16:18])[0] < 22:
            return None
        valid_bits = struct.unpack("<H", body[18:20])[0]
        tag = struct.unpack("<H", body[24:26])[0]
        if body[26:40] != _GUID_TAIL or valid_bits != bits:
            return None
    if tag == _TAG_PCM:
        fmt, limit = _INT_FORMATS.get(bits), PCM_MAX_CHANNELS_INT
    elif tag == _TAG_FLOAT:
        fmt, limit = _FLOAT_FORMATS.get(bits), PCM_MAX_CHANNELS_FLOAT
    else:
        return None
    if fmt is None or not 1 <= channels <= limit or rate <= 0 or align != channels * PCM_SAMPLE_BYTES[fmt]:
        return None
    return fmt, channels, rate, align


def _probe(path) -> PcmInfo | None:
    with open(path, "rb", buffering=0) as f:
        size = os.fstat(f.fileno()).st_size
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":   # (RIFX, RF64, BW64: not ours)
            return None
        fmt = None
        pos = 12
        while pos + 8 <= size:
            f.seek(pos)
            hdr = f.read(8)
            if len(hdr) < 8:
                return None
            cid, csize = hdr[:4], struct.unpack("<I", hdr[4:])[0]
            pos += 8
            if cid == b"data":
                if fmt is None or csize == 0 or pos + csize > size or csize % fmt[3]:
                    return None
                return PcmInfo(fmt[0], fmt[1], fmt[2], pos, csize // fmt[3])
            if cid == b"fmt ":
                if fmt is not None or csize > 4096:
                    return None
                body = f.read(csize)
                if len(body) < csize:
                    return None
                fmt = _parse_fmt(body)
                if fmt is None:
                    return None
            pos += csize + (csize & 1)   # (the pad byte after an odd-sized chunk)
    return None


def probe(path) -> PcmInfo | None:
    """The layout of a little-endian RIFF/WAVE file with plain PCM (u8, s16, s24 in 3 bytes, s32) or IEEE float (f32, f64)
    samples, or None for anything else -- a missing or unreadable file, another container (RIFX, RF64, BW64), another format
    tag or sub-format, valid bits that differ from the container's, a channel count outside the decoder's contract, a data
    chunk that is empty, longer than the file or not a whole number of frames.  Never raises.  None means: decode this file
    the way it always was (``preprocessing.load_audio``), with that path's results and messages."""
    try:
        return _probe(os.fspath(path))
    except Exception:
        return None


def read_raw(info: PcmInfo, path, out) -> int:
    """The bytes of ``info.raw_span`` -- the data chunk, widened to the enclosing aligned 16-byte windows where the file has
    those bytes -- into ``out`` (a writable contiguous uint8 buffer of at least ``info.raw_span[1]`` bytes: a pinned torch
    tensor, a numpy array), as they are.  -> the offset of the first sample in ``out``.  Raises OSError when the file no
    longer holds the data chunk."""
    lo, nbytes, pay = info.raw_span
    view = memoryview(out.numpy() if hasattr(out, "numpy") else out).cast("B")
    if len(view) < nbytes:
        raise ValueError(f"read_raw: the buffer has {len(view)} bytes, the file's samples need {nbytes}")
    need = pay + info.data_bytes
    with open(path, "rb", buffering=0) as f:
        f.seek(lo)
        got = 0
        while got < nbytes:   # (one readinto, but for the kernel's 2 GiB limit per read)
            n = f.readinto(view[got:nbytes])
            if not n:
                break
            got += n
    if got < need:
        raise OSError(f'"{path}" ends {need - got} bytes before its data chunk does')
    return pay
