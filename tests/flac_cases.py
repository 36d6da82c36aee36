"""A bit-level FLAC writer and the case table of the FLAC decode tests (test_flac_host.py, test_gpu_flac.py,
test_gpu_flac_files.py).  Written from the format facts of include/beat_this_amd.h ("FLAC decode") alone; it makes no attempt
to compress well: every choice a real encoder would search for -- subframe type, order, coefficients, precision, shift, wasted
bits, Rice method, partition order, parameters, escapes, channel assignment, block size and its coding, rate coding, blocking
strategy -- is given by the case, so that the table reaches every path of the decoder.  Not a test."""
import functools
import hashlib
import struct

import numpy as np

OK, BROKEN, LENGTH, CANDIDATES = range(4)     # BT_FLAC_*


# ---- bits and checksums ---------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        assert 0 <= v < (1 << n), (v, n)
        self.acc = (self.acc << n) | v
        self.n += n
        if self.n >= 512:
            self._flush()

    def _flush(self):
        rem = self.n & 7
        if self.n - rem:
            self.out += (self.acc >> rem).to_bytes((self.n - rem) // 8, "big")
            self.acc &= (1 << rem) - 1
            self.n = rem

    def signed(self, v, n):
        assert -(1 << (n - 1)) <= v < (1 << (n - 1)) if n else v == 0, (v, n)
        if n:
            self.put(v & ((1 << n) - 1), n)

    def unary(self, q):
        while q >= 256:          # (a long run: zeros in pieces)
            self.put(0, 256)
            q -= 256
        self.put(1, q + 1)

    def align(self):
        if self.n & 7:
            self.put(0, 8 - (self.n & 7))

    def bytes(self):
        assert self.n % 8 == 0
        self._flush()
        return bytes(self.out)


def _crc_table(poly, bits):
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    tab = []
    for b in range(256):
        c = b << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        tab.append(c)
    return tab


_T8, _T16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def crc8(data):
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


def coded_number(v):
    """UTF-8's scheme, extended to 7 bytes (36 bits)"""
    if v < 0x80:
        return bytes([v])
    for extra in range(1, 7):
        if v < 1 << (6 * extra + 6 - extra):
            lead = (0xFF << (7 - extra)) & 0xFF
            body = [0x80 | ((v >> (6 * k)) & 0x3F) for k in range(extra - 1, -1, -1)]
            return bytes([lead | (v >> (6 * extra))] + body)
    raise ValueError(v)


# ---- subframes ------------------------------------------------------------------------------------------------------------------
FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def _residuals(s, coefs, shift):
    a = np.asarray(s, dtype=np.int64)            # (25-bit samples x 15-bit coefficients x 32 taps: far inside int64)
    order = len(coefs)
    pred = np.zeros(len(a) - order, dtype=np.int64)
    for j, c in enumerate(coefs):
        pred += c * a[order - 1 - j: len(a) - 1 - j]
    res = a[order:] - (pred >> shift)            # (an arithmetic shift)
    assert len(res) == 0 or (-(1 << 31) <= res.min() and res.max() < (1 << 31))
    return res.tolist()


def _write_residual(bw, res, block, order, method, porder, params):
    """``params``: per partition a Rice parameter, ("esc", width) or None (chosen here); ``method`` None: 0 where 4-bit
    parameters do, else 1.  Nothing is validated: a case may ask for a reserved method or an impossible partition order."""
    parts, i = [], 0
    for p in range(1 << porder):
        cnt = max((block >> porder) - (order if p == 0 else 0), 0)
        parts.append(res[i: i + cnt])
        i += cnt
    parts[-1] = parts[-1] + res[i:]          # (an impossible order: the rest goes somewhere; the frame is invalid anyway)
    params = list(params) if params is not None else [None] * len(parts)
    for k, part in enumerate(parts):
        if params[k] is None:
            u = [(r << 1) if r >= 0 else ((-r - 1) << 1) | 1 for r in part]
            params[k] = max(int(sum(u) // max(len(u), 1)).bit_length() - 1, 0)
    if method is None:
        method = 1 if any(isinstance(k, int) and k > 14 for k in params) else 0
    bw.put(method, 2)
    bw.put(porder, 4)
    pbits = 5 if method == 1 else 4
    for k, part in zip(params, parts):
        if isinstance(k, tuple):
            bw.put((1 << pbits) - 1, pbits)
            bw.put(k[1], 5)
            for r in part:
                bw.signed(r, k[1])
        else:
            bw.put(k, pbits)
            for r in part:
                u = (r << 1) if r >= 0 else ((-r - 1) << 1) | 1
                bw.unary(u >> k)
                if k:
                    bw.put(u & ((1 << k) - 1), k)


def write_subframe(bw, samples, width, type="verbatim", order=0, coefs=None, precision=None, shift=0, wasted=0, method=None,
                   porder=0, params=None, raw_type=None, precision_code=None):
    """One subframe of ``samples`` (python ints that fit ``width`` bits; all multiples of 2^wasted)."""
    s = [int(v) for v in samples]
    if wasted:
        assert all(v % (1 << wasted) == 0 for v in s)
        s = [v >> wasted for v in s]
        width -= wasted
    code = {"constant": 0, "verbatim": 1}.get(type)
    if type == "fixed":
        code = 8 + order
    elif type == "lpc":
        order = len(coefs)
        code = 32 + order - 1
    bw.put(0, 1)
    bw.put(code if raw_type is None else raw_type, 6)
    bw.put(1 if wasted else 0, 1)
    if wasted:
        bw.unary(wasted - 1)
    if type == "constant":
        assert all(v == s[0] for v in s)
        bw.signed(s[0], width)
        return
    if type == "verbatim":
        for v in s:
            bw.signed(v, width)
        return
    for v in s[:order]:
        bw.signed(v, width)
    if type == "lpc":
        bw.put(precision - 1 if precision_code is None else precision_code, 4)
        bw.signed(shift, 5)
        for c in coefs:
            bw.signed(c, precision)
        res = _residuals(s, coefs, max(shift, 0))
    else:
        res = _residuals(s, FIXED[order], 0)
    _write_residual(bw, res, len(s), order, method, porder, params)


# ---- frames and streams -----------------------------------------------------------------------------------------------------------
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
SIZE_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}


def _block_code(n, force=None):
    if force is None:
        if n == 192:
            force = 1
        elif n in (576, 1152, 2304, 4608):
            force = 2 + (576, 1152, 2304, 4608).index(n)
        elif n in [256 << k for k in range(8)]:
            force = 8 + [256 << k for k in range(8)].index(n)
        else:
            force = 6 if n <= 256 else 7
    tail = bytes([n - 1]) if force == 6 else struct.pack(">H", n - 1) if force == 7 else b""
    return force, tail


def frame_body(pcm, bps, assign=None, subframes=None):
    """the subframes of one frame, padded to a byte: what lies between the header and the CRC-16 (it does not depend on the
    frame's number)"""
    pcm = np.asarray(pcm, dtype=np.int64).reshape(len(pcm), -1)
    ch = pcm.shape[1]
    if assign is None:
        assign = ch - 1
    if assign >= 8:
        left, right = pcm[:, 0], pcm[:, 1]
        side = left - right
        chans = {8: [(left, bps), (side, bps + 1)], 9: [(side, bps + 1), (right, bps)],
                 10: [((left + right) >> 1, bps), (side, bps + 1)]}[assign]
    else:
        chans = [(pcm[:, c], bps) for c in range(ch)]
    bw = BitWriter()
    for c, (vals, width) in enumerate(chans):
        write_subframe(bw, vals.tolist(), width, **(subframes[c] if subframes else {}))
    bw.align()
    return bw.bytes()


def write_frame(pcm, bps, rate, number, variable, assign=None, subframes=None, block_code=None, rate_code=0, size_code=None,
                flip_bit=None, bad_crc16=False, body=None, crc=None):
    """One frame of ``pcm`` (block, channels) integers.  ``assign``: None / 0 .. 7 = independent channels, 8 = left/side,
    9 = side/right, 10 = mid/side; ``subframes``: one dict of ``write_subframe`` keywords per channel (default: verbatim);
    ``rate_code``: 0, a table code, or 12 / 13 / 14 (the rate follows in kHz / Hz / tens of Hz); ``flip_bit``: a bit of the
    finished frame, counted from the end of the header, is inverted AFTER the CRC-16 was computed.  ``body``: a ``frame_body``
    made before (``pcm`` then only gives the shape); ``crc``: (header, body) -> the CRC-16, where a caller has a faster one."""
    pcm = np.asarray(pcm, dtype=np.int64).reshape(len(pcm), -1)
    block, ch = pcm.shape
    if assign is None:
        assign = ch - 1
    bcode, btail = _block_code(block, block_code)
    rtail = bytes([rate // 1000]) if rate_code == 12 else struct.pack(">H", rate) if rate_code == 13 else \
        struct.pack(">H", rate // 10) if rate_code == 14 else b""
    scode = SIZE_CODES.get(bps, 0) if size_code is None else size_code
    head = bytes([0xFF, 0xF8 | (1 if variable else 0), (bcode << 4) | rate_code, (assign << 4) | (scode << 1)])
    head += coded_number(number) + btail + rtail
    head += bytes([crc8(head)])
    if body is None:
        body = frame_body(pcm, bps, assign, subframes)
    value = (crc(head, body) if crc else crc16(head + body)) ^ (0x5A5A if bad_crc16 else 0)
    frame = bytearray(head + body + struct.pack(">H", value))
    if flip_bit is not None:
        at = 8 * len(head) + flip_bit
        frame[at // 8] ^= 0x80 >> (at % 8)
    return bytes(frame)


def pcm_md5(pcm, bps):
    nb = (bps + 7) // 8
    a = np.asarray(pcm, dtype="<i4").reshape(-1, 1).view(np.uint8)[:, :nb]
    return hashlib.md5(a.tobytes()).digest()


def streaminfo(min_block, max_block, rate, channels, bps, total, md5, min_frame=0, max_frame=0):
    v = (rate << 44) | ((channels - 1) << 41) | ((bps - 1) << 36) | total
    return struct.pack(">HH", min_block, max_block) + min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big") + \
        v.to_bytes(8, "big") + md5


def metadata(blocks):
    """[(type, body)] -> the metadata section, the last-block flag on the final one"""
    out = b""
    for k, (t, body) in enumerate(blocks):
        out += bytes([(0x80 if k == len(blocks) - 1 else 0) | t]) + len(body).to_bytes(3, "big") + body
    return out


def id3v2(n_body):
    size = bytes([(n_body >> 21) & 0x7F, (n_body >> 14) & 0x7F, (n_body >> 7) & 0x7F, n_body & 0x7F])
    return b"ID3\x04\x00\x00" + size + bytes((7 * k + 1) & 0xFF for k in range(n_body))


class Case:
    """name; data: the file's bytes; pcm: (total, channels) int64, the integers a decoder must restore; status: the code the
    decoder must report, ``where`` the byte it must name (None: not checked); kind: valid / false_frame / rejected"""

    def __init__(self, name, data, pcm, bps, rate, kind="valid", status=OK, where=None, first_frame=None, n_frames=None):
        self.name, self.data, self.pcm, self.bps, self.rate = name, data, np.asarray(pcm, dtype=np.int64), bps, rate
        self.kind, self.status, self.where, self.first_frame, self.n_frames = kind, status, where, first_frame, n_frames

    def __repr__(self):
        return f"Case({self.name})"

    @property
    def channels(self):
        return self.pcm.shape[1]

    def reference(self):
        """the numpy statement of the contract: s = v / 2^(bps-1) in fp64, numpy's channel mean, one rounding to fp32"""
        s = self.pcm.astype(np.float64) / float(1 << (self.bps - 1))
        return np.ascontiguousarray(s[:, 0] if s.shape[1] == 1 else s.mean(1), dtype=np.float32)


def build(name, pcm, bps, rate, frames, variable=False, extra_blocks=(), prefix=b"", trailing=b"", total=None, max_block=None,
          truncate=None, **case_kw):
    """``frames``: [dict(n=block size, + write_frame keywords)] that cover ``pcm`` in order -> a Case.  ``extra_blocks``:
    metadata behind STREAMINFO; ``prefix``: bytes in front of the marker (an ID3v2 tag); ``total``: the total_samples STREAMINFO
    claims; ``truncate``: cut the file this many bytes before its end."""
    pcm = np.asarray(pcm, dtype=np.int64).reshape(len(pcm), -1)
    audio, pos, starts = b"", 0, []
    for k, f in enumerate(frames):
        f = dict(f)
        n = f.pop("n")
        raw = f.pop("raw", None)
        starts.append(len(audio))
        if raw is not None:            # (bytes that are no frame of the chain)
            audio += raw
            continue
        number = f.pop("number", pos if variable else k)
        audio += write_frame(pcm[pos: pos + n], bps, rate, number, variable, **f)
        pos += n
    assert pos == len(pcm), (name, pos, len(pcm))
    sizes = [f["n"] for f in frames if "raw" not in f]
    info = streaminfo(min(sizes), max(sizes) if max_block is None else max_block, rate, pcm.shape[1], bps,
                      len(pcm) if total is None else total, pcm_md5(pcm, bps))
    head = prefix + b"fLaC" + metadata([(0, info)] + list(extra_blocks))
    data = head + audio + trailing
    if truncate:
        data = data[: len(data) - truncate]
    c = Case(name, data, pcm, bps, rate, first_frame=len(head), n_frames=len(sizes), **case_kw)
    c.frame_starts = [len(head) + s for s in starts]
    c.audio_end = len(head) + len(audio)
    return c


# ---- signals ----------------------------------------------------------------------------------------------------------------
def tone(n, channels, bps, seed, amp=0.6, noise=0.01):
    """a few partials plus noise, different per channel, scaled to ``amp`` of full scale"""
    rng = np.random.default_rng([seed, n, channels, bps])
    t = np.arange(n)[:, None]
    f = rng.uniform(0.002, 0.05, (3, 1, channels))
    x = sum(np.sin(2 * np.pi * f[k] * t + rng.uniform(0, 6, (1, channels))) / (k + 1) for k in range(3)) / 1.9
    x = amp * x + noise * rng.standard_normal((n, channels))
    full = (1 << (bps - 1)) - 1
    return np.clip(np.round(x * full), -full - 1, full).astype(np.int64)


def uniform(n, channels, bps, seed):
    """the whole range, extremes first"""
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    a = np.random.default_rng([seed, n, channels, bps, 1]).integers(lo, hi + 1, (n, channels), dtype=np.int64)
    edge = np.array([lo, hi, -1, 0, 1, lo + 1, hi, lo])[:n]
    a[: len(edge)] = edge[:, None]
    return a


def _lpc_coefs(order, precision, shift):
    """coefficients that fit ``precision`` bits and predict something: a decaying, alternating set scaled by 2^shift"""
    lim = (1 << (precision - 1)) - 1
    if precision == 1:
        return [-1 if j % 2 == 0 else 0 for j in range(order)]
    base = [(0.9 if order == 1 else 1.2) * (-0.6) ** j for j in range(order)]
    return [int(max(-lim - 1, min(lim, round(b * (1 << shift) if shift else (2 if j == 0 else -1 if j == 1 else 0)))))
            for j, b in enumerate(base)]


# ---- the table ------------------------------------------------------------------------------------------------------------------
def _valid_cases():
    cases = []
    add = cases.append
    V = dict(type="verbatim")

    # every subframe type, fixed orders 0 .. 4, in one 16-bit stereo track
    x = tone(5 * 192, 2, 16, 1)
    x[192 * 4:] = np.array([1234, -77])
    add(build("types", x, 16, 44100, [
        dict(n=192, subframes=[dict(type="fixed", order=0), dict(type="fixed", order=1)]),
        dict(n=192, subframes=[dict(type="fixed", order=2, porder=2), dict(type="fixed", order=3, porder=1)]),
        dict(n=192, subframes=[dict(type="fixed", order=4, porder=3), V]),
        dict(n=192, subframes=[dict(type="lpc", coefs=[14746], precision=15, shift=14), dict(type="lpc", coefs=[2, -1], precision=3, shift=0)]),
        dict(n=192, subframes=[dict(type="constant"), dict(type="constant")])]))

    # LPC orders x precisions x shifts, mono 16-bit, one frame each in one track
    frames = []
    for order in (1, 2, 8, 12, 32):
        for prec in (1, 12, 15):
            for shift in (0, 14):
                frames.append(dict(n=256, subframes=[dict(type="lpc", coefs=_lpc_coefs(order, prec, shift), precision=prec, shift=shift, porder=(order + prec) % 4)]))
    add(build("lpc_grid", tone(256 * len(frames), 1, 16, 2, amp=0.2), 16, 44100, frames))

    # full-scale 24-bit, order 32, precision 15: products of 2^23 x 2^14 x 32 need the 64-bit accumulator
    x = np.full((576, 2), (1 << 23) - 1, dtype=np.int64)
    x[::7, 0] = -(1 << 23)
    x[:, 1] = uniform(576, 1, 24, 3)[:, 0]
    wide = dict(type="lpc", coefs=[16383] * 32, precision=15, shift=14)
    add(build("wide_accumulator", x, 24, 96000, [dict(n=576, subframes=[wide, dict(type="lpc", coefs=[16383, -16384] * 16, precision=15, shift=14, porder=1)])]))

    # a 25-bit side channel: left at the top, right at the bottom of 24 bits
    x = uniform(192, 2, 24, 4)
    x[:8] = [[(1 << 23) - 1, -(1 << 23)], [-(1 << 23), (1 << 23) - 1]] * 4
    add(build("side_25_bits", x, 24, 48000, [dict(n=64, assign=8, subframes=[V, dict(type="fixed", order=1)]),
                                               dict(n=64, assign=9, subframes=[dict(type="fixed", order=0), V]),
                                               dict(n=64, assign=10, subframes=[V, V])], variable=True))

    # both Rice methods, partition orders 0 .. the largest the block allows (4096 = 2^12), parameters 0, 14 and 30
    frames, parts = [], []
    for k, p in enumerate(range(0, 13)):
        frames.append(dict(n=4096, subframes=[dict(type="fixed", order=1, porder=p, method=k % 2)]))
    parts.append(tone(4096 * 13, 1, 16, 5, amp=0.3))
    small = np.random.default_rng(6).integers(-1, 2, (256, 1))
    frames.append(dict(n=256, subframes=[dict(type="fixed", order=0, method=0, params=[0])]))
    parts.append(small)
    frames.append(dict(n=256, subframes=[dict(type="fixed", order=0, method=0, porder=1, params=[14, 14])]))
    parts.append(uniform(256, 1, 16, 7))
    frames.append(dict(n=256, subframes=[dict(type="fixed", order=0, method=1, porder=1, params=[30, 0])]))
    parts.append(np.concatenate([uniform(128, 1, 16, 8), small[:128]]))
    add(build("rice", np.concatenate(parts), 16, 44100, frames, variable=True))

    # escapes of width 0, 1, 16 and bps + 1; a unary run of 10 000
    x = np.zeros((192 * 5, 1), dtype=np.int64)
    x[:192] = 321                                                     # order 1: residuals all 0 -> width 0
    x[192:384, 0] = 321 + np.cumsum(np.random.default_rng(9).integers(-1, 1, 192))     # steps of -1 / 0 -> width 1
    x[384:576] = uniform(192, 1, 15, 10)                              # order 0: residuals fit 16 bits
    x[576:768, 0] = np.where(np.arange(192) % 2 == 0, 32767, -32768)  # order 1: steps of +-65535 -> 17 bits
    x[768:] = 5
    x[800] = 5005                                                     # order 0, parameter 0: u = 10010
    add(build("escapes", x, 16, 44100, [
        dict(n=192, subframes=[dict(type="fixed", order=1, params=[("esc", 0)])]),
        dict(n=192, subframes=[dict(type="fixed", order=1, porder=1, params=[("esc", 1), ("esc", 1)])]),
        dict(n=192, subframes=[dict(type="fixed", order=0, method=1, params=[("esc", 16)])]),
        dict(n=192, subframes=[dict(type="fixed", order=1, porder=2, params=[("esc", 17), 16, ("esc", 17), None], method=1)]),
        dict(n=192, subframes=[dict(type="fixed", order=0, method=0, params=[0])])]))

    # bits per sample (the odd ones come from STREAMINFO: size code 0) and wasted bits 1, 5, bps - 1
    for bps in (8, 12, 16, 20, 24, 4, 13):
        x = uniform(3 * 192, 2, bps, 11)
        w5 = min(5, bps - 2)
        x[192:384, 0] = x[192:384, 0] >> 1 << 1
        x[192:384, 1] = x[192:384, 1] >> w5 << w5
        x[384:, 0] = np.where(x[384:, 0] < 0, -(1 << (bps - 1)), 0)
        x[384:, 1] = tone(192, 1, bps, 12)[:, 0] >> 1 << 1
        add(build(f"bps_{bps}", x, bps, 32000, [
            dict(n=192, subframes=[dict(type="fixed", order=2), V]),
            dict(n=192, subframes=[dict(type="verbatim", wasted=1), dict(type="fixed", order=1, wasted=w5)]),
            dict(n=192, subframes=[dict(type="verbatim", wasted=bps - 1), dict(type="fixed", order=2, wasted=1)])],
            variable=bps in (12, 20)))

    # 1 .. 8 independent channels
    for ch in range(1, 9):
        sub = [dict(type="fixed", order=c % 5) if c % 3 else V for c in range(ch)]
        add(build(f"channels_{ch}", tone(2 * 576, ch, 16, 13 + ch, amp=0.9), 16, 22050, [dict(n=576, subframes=sub), dict(n=576)]))
    # the three stereo modes and independent stereo mixed in one track, wasted bits on a side channel
    x = tone(4 * 1152, 2, 16, 30, amp=0.95)
    x[1152:2304] = x[1152:2304] >> 2 << 2
    f2 = dict(type="fixed", order=2, porder=3)
    add(build("stereo_modes", x, 16, 44100, [dict(n=1152, assign=10, subframes=[f2, f2]),
                                               dict(n=1152, assign=8, subframes=[dict(type="fixed", order=1, wasted=2), dict(type="fixed", order=2, wasted=2)]),
                                               dict(n=1152, assign=9, subframes=[f2, V], rate_code=9), dict(n=1152, assign=1, subframes=[V, f2])]))

    # block sizes through every code family, a last frame of one sample (variable blocking: the sizes differ)
    sizes = [192, 576, 4608, 256, 4096, 1, 255, 4097, 192, 1]
    codes = [None, None, None, None, None, 6, 6, 7, 7, 6]
    x = tone(sum(sizes), 2, 16, 31)
    add(build("block_sizes", x, 16, 44100, [dict(n=n, block_code=c, subframes=[dict(type="fixed", order=min(2, n)), V]) for n, c in zip(sizes, codes)],
              variable=True))
    x = np.zeros((65535 + 7, 1), dtype=np.int64)
    x[:65535, 0] = tone(65535, 1, 8, 32)[:, 0]
    x[65535:] = -3
    add(build("block_65535", x, 8, 8000, [dict(n=65535, subframes=[V]), dict(n=7, subframes=[dict(type="constant")])]))

    # fixed blocking, 2 100 frames of 16 samples: the coded frame number grows from 1 to 2 to 3 bytes
    x = tone(2100 * 16, 1, 8, 33)
    add(build("many_frames", x, 8, 16000, [dict(n=16, subframes=[dict(type="fixed", order=1)]) for _ in range(2100)]))
    # variable blocking far into a stream: sample numbers of 4 and 5 coded bytes
    x = tone(3 * 256, 1, 16, 34)
    add(build("variable_numbers", x, 16, 44100, [dict(n=256, number=v) for v in (0x1FFF00, 0x200000, 0x200100)], variable=True))

    # rate codes 0, 9, 12, 13, 14
    for code, rate in ((0, 44100), (9, 44100), (12, 48000), (13, 22050), (13, 11025), (14, 22050), (0, 655350)):
        add(build(f"rate_code_{code}_{rate}", tone(2 * 192, 1, 16, 35), 16, rate, [dict(n=192, rate_code=code), dict(n=192, rate_code=code)]))

    # metadata: PADDING, SEEKTABLE, VORBIS_COMMENT, PICTURE; an ID3v2 prefix; trailing bytes
    blocks = [(3, bytes(18 * 3)), (4, struct.pack("<I", 5) + b"tests" + struct.pack("<I", 1) + struct.pack("<I", 7) + b"TITLE=x"),
              (6, struct.pack(">II", 3, 9) + b"image/png" + struct.pack(">I", 0) + bytes(16) + struct.pack(">I", 300) + bytes(range(256)) + bytes(44)),
              (1, bytes(77))]
    x = tone(2 * 576, 2, 16, 36)
    add(build("metadata", x, 16, 44100, [dict(n=576, assign=10), dict(n=576)], extra_blocks=blocks))
    add(build("id3_and_trailing", x, 16, 44100, [dict(n=576, assign=8), dict(n=576)], extra_blocks=blocks[:1], prefix=id3v2(301),
              trailing=b"TAG" + bytes(125)))
    # first_frame at all 16 residues modulo 16
    x = tone(1152 + 5, 2, 16, 37)
    for r in range(16):
        c = build(f"residue_{r}", x, 16, 44100, [dict(n=1152, assign=10, subframes=[dict(type="fixed", order=2)] * 2), dict(n=5)], extra_blocks=[(1, bytes(r + 2))])
        assert c.first_frame % 16 == (4 + 38 + 4 + r + 2) % 16
        add(c)
    assert sorted({c.first_frame % 16 for c in cases if c.name.startswith("residue_")}) == list(range(16))
    return cases


def _false_frame_cases():
    cases = []
    # a complete valid frame -- of this stream, with the number that would come next -- carried as verbatim payload
    inner_pcm = tone(40, 1, 8, 40)
    inner = write_frame(inner_pcm, 8, 8000, 1, False, subframes=[dict(type="fixed", order=1)])
    payload = np.frombuffer(inner, dtype=np.int8).astype(np.int64)
    x = np.concatenate([payload, tone(192 - len(payload), 1, 8, 41)[:, 0], tone(192, 1, 8, 42)[:, 0]])[:, None]
    cases.append(build("frame_as_payload", x, 8, 8000, [dict(n=192), dict(n=192, subframes=[dict(type="fixed", order=2)])], kind="false_frame"))
    # a header with a good CRC-8 in front of a bad CRC-16: as payload, between nothing and as trailing bytes
    fake = write_frame(tone(16, 1, 8, 43), 8, 8000, 1, False, bad_crc16=True)
    payload = np.frombuffer(fake, dtype=np.int8).astype(np.int64)
    x = np.concatenate([tone(50, 1, 8, 44)[:, 0], payload, tone(192 - 50 - len(payload), 1, 8, 45)[:, 0], tone(192, 1, 8, 46)[:, 0]])[:, None]
    cases.append(build("good_crc8_bad_crc16", x, 8, 8000, [dict(n=192), dict(n=192, subframes=[dict(type="fixed", order=1)])],
                       trailing=fake + fake[:9], kind="false_frame"))
    return cases


def _rejected_cases():
    cases = []
    x = tone(3 * 192, 2, 16, 50)
    f1 = dict(type="fixed", order=1)
    plain = [dict(n=192, subframes=[f1, f1]) for _ in range(3)]

    def rej(name, frames, status=BROKEN, broken_frame=None, where=None, **kw):
        c = build(name, x, 16, 44100, frames, kind="rejected", status=status, **kw)
        c.where = c.frame_starts[broken_frame] if broken_frame is not None else where(c) if where else None
        c.good_frames = broken_frame
        cases.append(c)

    rej("flipped_residual_bit", [plain[0], dict(plain[1], flip_bit=8 * 40 + 3), plain[2]], broken_frame=1)
    full = build("_", x, 16, 44100, plain)
    last = len(full.data) - full.frame_starts[2]
    rej("truncated_inside_a_frame", plain, broken_frame=2, truncate=last // 2)
    rej("truncated_between_frames", plain, where=lambda c: len(c.data), truncate=last)
    rej("total_one_too_many", plain, total=3 * 192 + 1, where=lambda c: c.audio_end)
    rej("total_one_too_few", plain, total=3 * 192 - 1, status=LENGTH, broken_frame=2)
    rej("reserved_subframe_type", [plain[0], dict(n=192, subframes=[f1, dict(f1, raw_type=0b000010)]), plain[2]], broken_frame=1)
    lpc = dict(type="lpc", coefs=[14746], precision=15, shift=14)
    rej("precision_code_15", [dict(n=192, subframes=[dict(lpc, precision_code=15), f1]), plain[1], plain[2]], broken_frame=0)
    rej("negative_shift", [plain[0], plain[1], dict(n=192, subframes=[f1, dict(lpc, shift=-1)])], broken_frame=2)
    rej("rice_method_2", [plain[0], dict(n=192, subframes=[dict(f1, method=2), f1]), plain[2]], broken_frame=1)
    rej("impossible_partition_order", [plain[0], dict(n=192, subframes=[f1, dict(f1, porder=7)]), plain[2]], broken_frame=1)
    rej("partition_shorter_than_order", [plain[0], dict(n=192, subframes=[dict(type="fixed", order=4, porder=6), f1]), plain[2]], broken_frame=1)
    return cases


@functools.lru_cache(maxsize=None)
def table():
    """{kind: [Case]}"""
    return {"valid": _valid_cases(), "false_frame": _false_frame_cases(), "rejected": _rejected_cases()}


def valid():
    return table()["valid"] + table()["false_frame"]


def rejected():
    return table()["rejected"]


def mutations(seed=0, per_case=4):
    """seeded byte flips of the valid cases' audio bytes: [(name, bytes)] -- whatever they decode to, the parser must stay
    inside the file"""
    rng = np.random.default_rng(seed)
    out = []
    for c in valid():
        if len(c.data) > 40000:
            continue
        for k in range(per_case):
            data = bytearray(c.data)
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(c.first_frame, len(data)))
                data[at] ^= int(rng.integers(1, 256))
            out.append((f"{c.name}_mut{k}", bytes(data)))
    return out
