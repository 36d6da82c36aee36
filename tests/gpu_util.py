"""Helpers for the -m gpu parity tests: thin ctypes wrappers over the single-operator C-ABI
entry points, and a JSONL report written under gpurun_out/ (merged back by gpurun)."""
import ctypes as C
import json
import math
import os

import numpy as np
import torch

from conftest import ROOT

REPORT = os.path.join(ROOT, "gpurun_out", "test_report.jsonl")


def report(name, **vals):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    clean = {k: (float(v) if isinstance(v, (np.floating, float)) else v) for k, v in vals.items()}
    with open(REPORT, "a") as f:
        f.write(json.dumps(dict(test=name, **clean)) + "\n")


def HALF():
    """torch dtype of the library's half-precision operands (float16, or bfloat16 in a -DBT_HALF_BF16 build)"""
    from beat_this_amd import _lib

    return _lib.half_torch_dtype()


def dev():
    return torch.device("cuda:0")


def tdtype(prec):
    return torch.float32 if prec == 0 else HALF()


def run_gemm(prec, A, W, N, epi, flags, bias=None, out=None, ldo=0, x=None, conv=None, qkv=None, sync=True):
    """A: device tensor (rows, lda) ; W: (Npad, K) in compute dtype."""
    from beat_this_amd import _lib

    a = _lib.GemmArgs()
    a.A, a.lda, a.W = A.data_ptr(), A.shape[-1], W.data_ptr()
    a.M = conv["M"] if conv else A.shape[0]
    a.N, a.K, a.epi, a.flags = N, W.shape[1], epi, flags
    a.bias = bias.data_ptr() if bias is not None else 0
    if out is not None:
        a.out, a.ldo = out.data_ptr(), ldo or out.shape[-1]
    if x is not None:
        a.x, a.ldx = x.data_ptr(), x.shape[-1]
    if conv:
        a.conv_C2, a.conv_T, a.conv_F = conv["C2"], conv["T"], conv["F"]
    if qkv:
        a.gates, a.inner, a.heads = qkv["gates"].data_ptr(), qkv["inner"], qkv["heads"]
        a.rope, a.pdiv, a.pmod = qkv["rope"].data_ptr(), qkv["pdiv"], qkv["pmod"]
        a.map_T, a.map_F = qkv.get("map_T", 0), qkv.get("map_F", 0)
    _lib.check(_lib.lib().bt_gemm(_lib.stream_ptr(dev()), prec, C.byref(a)))
    if sync:
        torch.cuda.synchronize()


def run_attn(prec, qkv, gates, out, n_seq, L, heads, o_div=1, o_outer=None, o_inner=0, o_tok=1):
    from beat_this_amd import _lib

    a = _lib.AttnArgs()
    a.qkv, a.ld, a.gates, a.out = qkv.data_ptr(), qkv.shape[-1], gates.data_ptr(), out.data_ptr()
    a.n_seq, a.L, a.heads, a.inner, a.o_div = n_seq, L, heads, heads * 32, o_div
    a.o_outer = L if o_outer is None else o_outer
    a.o_inner, a.o_tok = o_inner, o_tok
    _lib.check(_lib.lib().bt_attention(_lib.stream_ptr(dev()), prec, C.byref(a)))
    torch.cuda.synchronize()


# ---- inputs and references the inference kernel tests share --------------------------------------------------------------------
def _mk(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def _rel(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _attn_ref(q, k, v, gates):
    # q, k, v: (S, H, L, 32) float64, q already carries log2(e) / sqrt(d): softmax in base 2
    s = q @ k.transpose(-1, -2) * math.log(2.0)
    return torch.softmax(s, -1) @ v * gates[..., None]


def _pair_sd(dim, seed):
    """float64 weights of one attention + feed-forward pair of width ``dim``, under "a." and "f." """
    H = dim // 32
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, s=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * s
    return {
        "a.norm.gamma": 1 + 0.1 * rn(dim), "a.to_qkv.weight": rn(3 * dim, dim, s=1.6 / math.sqrt(dim)),
        "a.to_gates.weight": rn(H, dim, s=0.3), "a.to_gates.bias": rn(H, s=0.3),
        "a.to_out.0.weight": rn(dim, dim, s=1 / math.sqrt(dim)),
        "f.net.0.gamma": 1 + 0.1 * rn(dim), "f.net.1.weight": rn(4 * dim, dim, s=1 / math.sqrt(dim)),
        "f.net.1.bias": rn(4 * dim, s=0.2), "f.net.4.weight": rn(dim, 4 * dim, s=0.5 / math.sqrt(dim)),
        "f.net.4.bias": rn(dim, s=0.2),
    }


def pad_rows(w, mult=128):
    n = w.shape[0]
    npad = (n + mult - 1) // mult * mult
    out = torch.zeros((npad, w.shape[1]), dtype=w.dtype)
    out[:n] = w
    return out


# ---- fragment-major attention operands (csrc/attn2.hip) ---------------------------------------------
def frag_qk(x, nbp):
    """[SH, L, 32] -> half [SH, nbp, 4 (quarter), 32 (token), 8]"""
    SH, L, _ = x.shape
    pad = torch.zeros((SH, nbp * 32, 32), dtype=x.dtype)
    pad[:, :L] = x
    return pad.view(SH, nbp, 32, 4, 8).permute(0, 1, 3, 2, 4).contiguous().to(HALF())


def unfrag_qk(fr, L):
    SH, nbp = fr.shape[:2]
    return fr.view(SH, nbp, 4, 32, 8).permute(0, 1, 3, 2, 4).reshape(SH, nbp * 32, 32)[:, :L]


def frag_v(x, nbp):
    """[SH, L, 32] -> half [SH, nbp, 2 (s), 2 (g), 32 (d), 8]; token = 16 s + 8 (j >> 2) + 4 g + (j & 3)"""
    SH, L, _ = x.shape
    pad = torch.zeros((SH, nbp * 32, 32), dtype=x.dtype)
    pad[:, :L] = x
    t = pad.view(SH, nbp, 2, 2, 2, 4, 32)           # [s][jh][g][jl][d]
    return t.permute(0, 1, 2, 4, 6, 3, 5).contiguous().view(SH, nbp, 2, 2, 32, 8).to(HALF())


def unfrag_v(fr, L):
    SH, nbp = fr.shape[:2]
    t = fr.view(SH, nbp, 2, 2, 32, 2, 4)             # [s][g][d][jh][jl]
    return t.permute(0, 1, 2, 5, 3, 6, 4).reshape(SH, nbp * 32, 32)[:, :L]


def run_attn_frag(qf, kf, vf, gates, out, n_seq, L, heads, nbp, o_div=1, o_outer=None, o_inner=0, o_tok=1, variant=0):
    """variant (bt_attn_frag_args.x3 of the half path): 0 = the kernel the launch size selects, -1 = the one-query-block kernel,
    -2 = two query blocks per wave on the hand-scheduled loop (round 6)"""
    from beat_this_amd import _lib

    a = _lib.AttnFragArgs()
    a.x3 = variant
    a.q, a.k, a.v, a.gates, a.out = qf.data_ptr(), kf.data_ptr(), vf.data_ptr(), gates.data_ptr(), out.data_ptr()
    a.n_seq, a.L, a.heads, a.inner, a.nbp, a.o_div = n_seq, L, heads, heads * 32, nbp, o_div
    a.o_outer = L if o_outer is None else o_outer
    a.o_inner, a.o_tok = o_inner, o_tok
    _lib.check(_lib.lib().bt_attention_frag(_lib.stream_ptr(dev()), C.byref(a)))
    torch.cuda.synchronize()


# ---- BT_PREC_F32X3 operand formats (csrc/gemm3.hip, csrc/attn2.hip) --------------------------------------------------
def to_hl32(x):
    """fp32 [M, K] (K % 32 == 0) -> fp16 [M, 2 K]: per 32 columns the 32 hi halves, then the 32 lo halves (x = hi + lo)."""
    x = x.float()
    m, k = x.shape
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    return torch.stack([hi.view(m, k // 32, 32), lo.view(m, k // 32, 32)], 2).reshape(m, 2 * k).contiguous()


def from_hl32(h):
    """fp16 [M, 2 K] hl32 -> float64 [M, K] = hi + lo"""
    m, k2 = h.shape
    t = h.double().view(m, k2 // 64, 2, 32)
    return (t[:, :, 0] + t[:, :, 1]).reshape(m, k2 // 2)


HL8_ACT_SHIFT = 8.0   # the byte sections of an hl8 ACTIVATION carry 2^-3 of what a weight's carry (csrc/common.h: range to 3584)


def to_hl8(x, act=False):
    """fp32 [M, K] (K % 32 == 0) -> the "hl8" operand form of csrc/gemm3.hip (X3 = 2), returned as fp16 [M, 2 K] (128 B per 32
    columns like hl32): 32 hi halves | 32 hi bytes = e4m3(x) | 32 lo bytes = e4m3(2^11 (x - hi)) for a weight; an activation
    (act=True) carries e4m3(x / 8) and e4m3(2^8 (x - hi))."""
    x = x.float()
    m, k = x.shape
    hi = x.to(torch.float16)
    s = HL8_ACT_SHIFT if act else 1.0
    lo = (x - hi.float()) * (2048.0 / s)
    out = torch.empty((m, k // 32, 128), dtype=torch.uint8)
    out[:, :, :64] = hi.contiguous().view(m, k // 32, 32).view(torch.uint8)
    out[:, :, 64:96] = (x / s).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).view(m, k // 32, 32)
    out[:, :, 96:] = lo.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).view(m, k // 32, 32)
    return out.view(m, k // 32 * 128).view(torch.float16).contiguous()


def to_hl8a(x):
    return to_hl8(x, act=True)


def hl8_parts(h, act=False):
    """fp16 [M, 2 K] hl8 -> float64 (hi halves, the value the hi bytes stand for, the value the lo bytes stand for), each [M, K]"""
    m, k2 = h.shape
    s = HL8_ACT_SHIFT if act else 1.0
    b = h.contiguous().view(torch.uint8).view(m, k2 // 64, 128)
    hi = b[:, :, :64].contiguous().view(torch.float16).double().reshape(m, k2 // 2)
    h8 = b[:, :, 64:96].contiguous().view(torch.float8_e4m3fn).double().reshape(m, k2 // 2) * s
    l8 = b[:, :, 96:].contiguous().view(torch.float8_e4m3fn).double().reshape(m, k2 // 2) / 2048.0 * s
    return hi, h8, l8


def hl8_matmul(a, w):
    """what the hl8 GEMM computes (float64): hi . hi + e4m3(a) . lo8(w) + lo8(a) . e4m3(w); a an hl8 activation, w an hl8 weight"""
    ah, a8, al = hl8_parts(a, act=True)
    wh, w8, wl = hl8_parts(w)
    return ah @ wh.T + a8 @ wl.T + al @ w8.T


def frag_x3(x, nbp, kind):
    """[SH, L, 32] fp32-valued -> fp16 [SH, nbp, 2 (hi | lo), 1024]: the 4 KB blocks of the X3 attention operands"""
    f = frag_qk if kind == "qk" else frag_v
    x = x.float()
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    SH = x.shape[0]
    return torch.stack([f(hi.float(), nbp).view(SH, nbp, 1024), f(lo.float(), nbp).view(SH, nbp, 1024)], 2).contiguous()


def unfrag_x3(fr, L, kind):
    """inverse of frag_x3 -> float64 [SH, L, 32]"""
    u = unfrag_qk if kind == "qk" else unfrag_v
    return u(fr[:, :, 0].contiguous(), L).double() + u(fr[:, :, 1].contiguous(), L).double()


def run_attn_x3(q, k, v, gates, n_seq, L, heads, out_f32, variant=1, raw=False, status_out=None, **omap):
    """bt_attention_frag on x3 operands: q, k, v [SH, L, 32] fp32-valued, gates [SH, L]; out_f32: 0 = hl32 rows, 1 = fp32 rows,
    2 = hl8 rows; variant = bt_attn_frag_args.x3; omap: o_div / o_outer / o_inner / o_tok of the row map.  Returns the rows as
    float64 (raw: as the kernel stored them)."""
    from beat_this_amd import _lib as Lb

    nbp = Lb.lib().bt_attn_frag_blocks(L)
    SH = n_seq * heads
    gh = torch.zeros((SH, nbp * 32), dtype=torch.float32)
    gh[:, :L] = gates.float()
    rows = n_seq * L
    inner = heads * 32
    out = torch.zeros((rows, inner), dtype=torch.float32, device=dev()) if int(out_f32) == 1 else \
        torch.zeros((rows, 2 * inner), dtype=torch.float16, device=dev())
    qf, kf, vf = frag_x3(q, nbp, "qk"), frag_x3(k, nbp, "qk"), frag_x3(v, nbp, "v")
    nblk = (L + 31) // 32
    kf[:, nblk:] = float("nan")   # padding blocks beyond ceil(L / 32) must never be consumed
    vf[:, nblk:] = float("nan")
    a = Lb.AttnFragArgs()
    qd, kd, vd, gd = qf.to(dev()), kf.to(dev()), vf.to(dev()), gh.to(dev())
    st = torch.zeros(1, dtype=torch.int32, device=dev())
    a.q, a.k, a.v, a.gates, a.out = qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), gd.data_ptr(), out.data_ptr()
    a.n_seq, a.L, a.heads, a.inner, a.nbp, a.o_div = n_seq, L, heads, inner, nbp, omap.get("o_div", 1)
    a.o_outer, a.o_inner, a.o_tok = omap.get("o_outer", L), omap.get("o_inner", 0), omap.get("o_tok", 1)
    a.x3, a.out_f32, a.status = variant, int(out_f32), st.data_ptr()
    scratch = torch.full((SH, nbp), -1, dtype=torch.int32, device=dev())   # the launch's overflow map (stale bits must not matter)
    a.scratch = scratch.data_ptr()
    Lb.check(Lb.lib().bt_attention_frag(Lb.stream_ptr(dev()), C.byref(a)))
    torch.cuda.synchronize()
    if status_out is not None:   # (the caller looks at the range flag itself)
        status_out.append(int(st.item()))
    else:
        assert int(st.item()) == 0
    if raw:
        return out.cpu()
    if int(out_f32) == 2:   # hl8 rows: hi halves + what the lo bytes stand for
        hi, _, l8 = hl8_parts(out.cpu(), act=True)
        return hi + l8
    return out.double().cpu() if int(out_f32) == 1 else from_hl32(out.cpu())


# ---- guard bands and poisoned memory (tests/test_gpu_guard.py) -------------------------------------------------------
GUARD_BAND = 2 << 20   # bytes on each side of a guarded buffer: more than a whole 128-row tile of 2048 fp32 columns (1 MiB)
POISONS = (0xFF, 0x7B)  # 0xFF: NaN in fp32 / fp16 / bf16, -1 as int32;  0x7B: large finite (fp32 ~1.3e36, fp16 61280, bf16 ~1.3e36)


class Guarded:
    """One device uint8 allocation [band | payload (rounded up to 256 bytes) | band]; ``t`` is the payload as a typed tensor
    of ``shape`` (256-byte aligned: the band is a multiple of 256 and torch's allocations are 512-aligned)."""

    def __init__(self, shape, dtype, band=GUARD_BAND):
        shape = tuple(int(s) for s in shape)
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        self.band = band
        self.raw = torch.empty(band + (self.nbytes + 255) // 256 * 256 + band, dtype=torch.uint8, device=dev())
        self.pattern = None
        self.t = self.raw[band:band + self.nbytes].view(dtype).view(shape)
        assert self.t.data_ptr() % 256 == 0

    def fill(self, pattern_byte, data=None, payload_byte=None):
        """every byte (payload and bands) = pattern_byte; then ``data``, if given, goes into the payload, or else
        ``payload_byte``, if given, fills it (a buffer that may only be poisoned outside its payload)"""
        self.raw.fill_(pattern_byte)
        self.pattern = pattern_byte
        if data is not None:
            self.t.copy_(data.reshape(self.t.shape))
        elif payload_byte is not None:
            self.t.view(torch.uint8).view(-1).fill_(payload_byte)
        return self

    def ptr(self):
        return self.t.data_ptr()

    def bands_intact(self, what="buffer"):
        """None, or a message naming the first damaged byte of a band and its distance from the payload"""
        lo = self.raw[:self.band]
        hi = self.raw[self.band + self.nbytes:]
        for name, part, base in (("leading", lo, 0), ("trailing", hi, self.band + self.nbytes)):
            bad = torch.nonzero(part != self.pattern)
            if bad.numel():
                off = base + int(bad[0])
                dist = self.band - off if name == "leading" else off - (self.band + self.nbytes)
                return (f"{what}: {name} band damaged at byte {off} of the allocation, {dist} bytes "
                        f"{'before' if name == 'leading' else 'after'} the {self.nbytes}-byte payload "
                        f"({int(bad.shape[0])} bytes differ from 0x{self.pattern:02X})")
        return None


def assert_intact(*named):
    """named: (name, Guarded) pairs -> fails naming every damaged band"""
    bad = [m for m in (g.bands_intact(n) for n, g in named) if m]
    assert not bad, "; ".join(bad)


def workspace_regions(h, B, T, prec):
    """bt_workspace_regions: [(begin, end of the requested bytes)] of the forward's workspace regions"""
    from beat_this_amd import _lib

    n = _lib.lib().bt_workspace_regions(h, B, T, prec, None, 0)
    _lib.check(min(n, 0))
    buf = (C.c_int64 * (2 * n))()
    assert _lib.lib().bt_workspace_regions(h, B, T, prec, buf, n) == n
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(n)]


def gaps_intact(raw, pattern, regions, total, what="workspace"):
    """raw: the workspace's bytes (uint8).  None, or a message naming the first workspace region whose gap behind it (alignment
    slack + BT_OPT_WS_GUARD bytes, up to the next region / the end of the workspace) no longer holds the fill byte"""
    raw = raw.view(-1)
    ends = [b for b, _ in regions[1:]] + [total]
    for i, ((b, e), nxt) in enumerate(zip(regions, ends)):
        if nxt > e:
            bad = torch.nonzero(raw[e:nxt] != pattern)
            if bad.numel():
                return (f"{what}: gap behind region {i} [{b}, {e}) damaged {int(bad[0])} bytes past its end "
                        f"({int(bad.shape[0])} of {nxt - e} bytes differ from 0x{pattern:02X})")
    return None
