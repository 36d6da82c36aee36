"""FLAC files as they lie on disk, for the device decoder (csrc/flac.hip): ``probe`` reads the head of the file -- the marker
behind an optional ID3v2 tag, the metadata block headers, STREAMINFO, the first two bytes of the first frame -- and says
what the stream is and where its frames begin, or None, which always means "take ``load_audio`` as before"; ``read_raw`` puts
the file's bytes, undecoded, into a caller-supplied (pinned) buffer.  Nothing here touches the GPU or decodes a sample: the
frames are found and decoded on the device (include/beat_this_amd.h, "FLAC decode").
"""
from __future__ import annotations

import os
from typing import NamedTuple

from . import _lib

MAX_BYTES = MAX_SAMPLES = (1 << 31) - 1     # the device entry points' limits


class FlacInfo(NamedTuple):
    """What ``probe`` found (bt_flac_info): the STREAMINFO fields, the blocking bit of the first frame, the byte offset of
    the first frame and the file's length."""
    sample_rate: int
    channels: int
    bps: int
    blocking: int
    min_block: int
    max_block: int
    total_samples: int
    first_frame: int
    n_bytes: int
    md5: bytes

    @property
    def n_frames(self) -> int:
        """samples per channel (``wav.PcmInfo``'s word for it)"""
        return self.total_samples

    @property
    def decoded_bytes(self) -> int:
        """the PCM bytes this stream stands for: what a batch cap counts"""
        return self.total_samples * self.channels * ((self.bps + 7) // 8)

    def c_info(self) -> "_lib.FlacInfo":
        c = _lib.FlacInfo(self.sample_rate, self.channels, self.bps, self.blocking, self.min_block, self.max_block,
                          self.total_samples, self.first_frame, self.n_bytes)
        c.md5[:] = self.md5
        return c


def _probe(path) -> FlacInfo | None:
    with open(path, "rb", buffering=0) as f:
        size = os.fstat(f.fileno()).st_size
        pos = 0
        head = f.read(10)
        if len(head) == 10 and head[:3] == b"ID3":
            if any(b & 0x80 for b in head[6:10]):
                return None
            pos = 10 + (head[6] << 21 | head[7] << 14 | head[8] << 7 | head[9]) + (10 if head[5] & 0x10 else 0)
        f.seek(pos)
        if f.read(4) != b"fLaC":          # (Ogg FLAC starts with OggS: not ours)
            return None
        pos += 4
        info = None
        last = False
        while not last:
            f.seek(pos)
            hdr = f.read(4)
            if len(hdr) < 4:
                return None
            last, kind, length = bool(hdr[0] & 0x80), hdr[0] & 0x7F, int.from_bytes(hdr[1:], "big")
            pos += 4
            if pos + length > size or kind == 127:
                return None
            if info is None:              # STREAMINFO comes first
                if kind != 0 or length != 34:
                    return None
                q = f.read(34)
                if len(q) < 34:
                    return None
                v = int.from_bytes(q[10:18], "big")
                info = dict(min_block=q[0] << 8 | q[1], max_block=q[2] << 8 | q[3], sample_rate=v >> 44, channels=((v >> 41) & 7) + 1,
                            bps=((v >> 36) & 31) + 1, total_samples=v & ((1 << 36) - 1), md5=bytes(q[18:34]))
            elif kind == 0:
                return None
            pos += length
        if not 0 < info["total_samples"] <= MAX_SAMPLES or not 4 <= info["bps"] <= 24 or info["sample_rate"] <= 0 or info["max_block"] < 1:
            return None
        if size > MAX_BYTES:
            return None
        f.seek(pos)
        sync = f.read(2)
        if len(sync) < 2 or sync[0] != 0xFF or sync[1] & 0xFE != 0xF8:
            return None
        return FlacInfo(blocking=sync[1] & 1, first_frame=pos, n_bytes=size, **info)


def probe(path) -> FlacInfo | None:
    """The layout of a native FLAC file inside the device decoder's subset -- 1 .. 8 channels, 4 .. 24 bits per sample, a
    known total_samples -- or None for anything else: a missing or unreadable file, Ogg FLAC, total_samples == 0, 25 .. 32
    bits per sample, a file or a stream of 2^31 bytes / samples or more, metadata that runs past the end of the file, no
    frame sync where the metadata ends.  Never raises.  None means: decode this file the way it always was
    (``preprocessing.load_audio``), with that path's results and messages.  (The same walk as bt_flac_probe_host, with seeks
    instead of the whole file in memory.)"""
    try:
        return _probe(os.fspath(path))
    except Exception:
        return None


def read_raw(info: FlacInfo, path, out) -> int:
    """The whole file -- ``info.n_bytes`` bytes -- into ``out`` (a writable contiguous uint8 buffer at least that long: a
    pinned torch tensor, a numpy array), as it is.  -> 0, the offset of the file's first byte in ``out`` (``first_frame``
    counts from there).  Raises OSError when the file no longer has that many bytes."""
    view = memoryview(out.numpy() if hasattr(out, "numpy") else out).cast("B")
    if len(view) < info.n_bytes:
        raise ValueError(f"read_raw: the buffer has {len(view)} bytes, the file needs {info.n_bytes}")
    with open(path, "rb", buffering=0) as f:
        got = 0
        while got < info.n_bytes:
            n = f.readinto(view[got:info.n_bytes])
            if not n:
                break
            got += n
    if got < info.n_bytes:
        raise OSError(f'"{path}" ends {info.n_bytes - got} bytes before its frames do')
    return 0
