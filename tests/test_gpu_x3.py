"""Parity of the BT_PREC_F32X3 kernels (hi + lo fp16 operands, three MFMAs per product) on the MI355X against float64
restatements: the hl32 GEMM of csrc/gemm3.hip in its three epilogues and as the frontend convolution, the fragment-major
attention of csrc/attn2.hip on 4 KB [hi | lo] blocks, the frontend's time-direction QKV projection, the hl32 shadow of the
fused out-projection + FF kernel, and the range flag every operand-splitting kernel raises.  Tolerances are fp32-class
(1e-6 .. 1e-5 relative): this is the path that carries the 1e-3 logit / identical-beats gate."""
import ctypes as C
import math

import pytest
import torch

from gpu_util import HL8_ACT_SHIFT, _attn_ref, _mk, _rel, dev, frag_x3, from_hl32, hl8_matmul, hl8_parts, pad_rows, report, to_hl8, to_hl8a, to_hl32, unfrag_x3
from gpu_util import run_attn_x3 as _run_attn

pytestmark = pytest.mark.gpu


def _ssq_parts(x32):
    M, D = x32.shape
    return (x32.double() ** 2).view(M, D // 64, 64).sum(-1).T.contiguous().float()


def _call(nsplit=0, cfg=1, **kw):
    from beat_this_amd import _lib as L

    a = L.Gemm3Args()
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    # x3 & 15: 1 = the launcher's choice, 3 = 128 x 128 tiles, 4 = the 256 x 128 k16 configuration (gemm3.hip: G3CfgMX), 5 = the
    # 64 x 128 tiles (G3CfgHX, residual epilogue only);
    # bits 4.. force the number of XCD groups the weight matrix is split over (launch_cfg)
    a.x3 = cfg | (nsplit << 4)
    L.check(L.lib().bt_gemm3(L.stream_ptr(dev()), C.byref(a)))
    torch.cuda.synchronize()


def _status():
    return torch.zeros(1, dtype=torch.int32, device=dev())


@pytest.mark.parametrize("cfg", [1, 3, 4])
@pytest.mark.parametrize("M,K,N,nsplit", [(1500, 512, 2048, 0), (333, 128, 512, 0), (24000, 512, 2048, 0), (49500, 512, 2048, 0),
                                          (24000, 512, 2048, 2), (24000, 512, 2048, 4), (777, 512, 2048, 8), (1500, 128, 512, 2)])
def test_gemm3_x3_ff1(M, K, N, nsplit, cfg):
    if cfg != 1 and (nsplit or M == 49500):
        pytest.skip("forced tile configurations: one pass over the shapes without the XCD-split variants")
    """out = gelu_erf(rms(A) W^T + b) as hl32 planes; operands are fp32 values (exactly representable as hi + lo)."""
    x = _mk((M, K), 1, 2.0).float()
    W, b = _mk((N, K), 2, 1 / math.sqrt(K)).float(), _mk((N,), 3)
    out = torch.zeros((M, 2 * N), dtype=torch.float16, device=dev())
    st = _status()
    _call(nsplit, cfg, A=to_hl32(x).to(dev()), lda=K, M=M, K=K, W=to_hl32(pad_rows(W, 256)).to(dev()), N=N, epi=0, bias=b.float().to(dev()),
          ssq_in=_ssq_parts(x).to(dev()), ssq_parts=K // 64, out=out, ldo=N, status=st)
    rs = math.sqrt(K) / x.double().norm(dim=-1, keepdim=True).clamp_min(1e-12)
    ref = torch.nn.functional.gelu(from_hl32(to_hl32(x)) @ from_hl32(to_hl32(W)).T * rs + b)
    err = _rel(from_hl32(out.cpu()), ref)
    report("gemm3_x3_ff1", M=M, K=K, N=N, nsplit=nsplit, cfg=cfg, rel=err)
    assert err < 3e-6 and int(st.item()) == 0


# (M = 24000 runs on the 192 x 256 tiles, M = 32768 on the 256 x 256 ones, the others on 128 x 128)
@pytest.mark.parametrize("M,K,N,bias,nsplit", [(1500, 2048, 512, True, 0), (777, 512, 512, False, 0), (130, 128, 128, True, 0),
                                               (24000, 2048, 512, True, 0), (32768, 1024, 512, False, 0), (49500, 512, 512, True, 0),
                                               (24000, 2048, 512, True, 2), (32768, 1024, 512, False, 2), (777, 512, 512, False, 4)])
@pytest.mark.parametrize("cfg", [1, 3, 4, 5])   # (5 = the 64 x 128 tiles of a single-file forward's residual GEMMs, round 5)
def test_gemm3_x3_resid(M, K, N, bias, nsplit, cfg):
    if cfg != 1 and (nsplit or M == 32768):
        pytest.skip("forced tile configurations: one pass over the shapes without the XCD-split variants")
    A = _mk((M, K), 4).float()
    W = _mk((N, K), 5, 0.5 / math.sqrt(K)).float()
    b = _mk((N,), 6)
    x0 = _mk((M, N), 7).float()
    x = x0.to(dev()).clone()
    xb = torch.full((M, 2 * N), float("nan"), dtype=torch.float16, device=dev())
    ssq = torch.full((N // 64, M), -1.0, dtype=torch.float32, device=dev())
    st = _status()
    _call(nsplit, cfg, A=to_hl32(A).to(dev()), lda=K, M=M, K=K, W=to_hl32(pad_rows(W, 256)).to(dev()), N=N, epi=1,
          bias=b.float().to(dev()) if bias else 0, x=x, ldx=N, xb=xb, ssq_out=ssq, status=st)
    ref = x0.double() + from_hl32(to_hl32(A)) @ from_hl32(to_hl32(W)).T + (b if bias else 0)
    err = _rel(x, ref)
    xc = x.double().cpu()
    errb = float((from_hl32(xb.cpu()) - xc).abs().max() / xc.abs().max())   # the shadow IS the new x, to 2^-22
    errs = _rel(ssq, (ref ** 2).view(M, N // 64, 64).sum(-1).T)
    report("gemm3_x3_resid", M=M, K=K, N=N, nsplit=nsplit, cfg=cfg, rel=err, shadow=errb, ssq=errs)
    assert err < 2e-6 and errb < 1e-6 and errs < 1e-5 and int(st.item()) == 0


# ---- hl8 operands (round 5, BASELINE config 5): the cross terms of the hi + lo product on one block-scaled fp8 MFMA --------------
F8_IN, F8_OUT = 0x100, 0x200   # bt_gemm3_args.x3 flags (csrc/kernels.h: G3_X3_F8, G3_X3_OUT_F8)


@pytest.mark.parametrize("M,K,N", [(1500, 512, 2048), (333, 128, 512), (24000, 512, 2048), (3000, 512, 2048)])
def test_gemm3_f8_ff1(M, K, N):
    """FF1 on hl8 operands (hl32 output): against the float64 evaluation of the same arithmetic -- hi . hi + 2^-11 (hi bytes .
    lo bytes + lo bytes . hi bytes) -- to fp32 rounding, and against the exact product within the e4m3 cross terms' 2^-14."""
    x = _mk((M, K), 1, 2.0).float()
    W, b = _mk((N, K), 2, 1 / math.sqrt(K)).float(), _mk((N,), 3)
    a8, w8 = to_hl8a(x), to_hl8(pad_rows(W, 256))
    out = torch.zeros((M, 2 * N), dtype=torch.float16, device=dev())
    st = _status()
    _call(0, 1 | F8_IN, A=a8.to(dev()), lda=K, M=M, K=K, W=w8.to(dev()), N=N, epi=0, bias=b.float().to(dev()),
          ssq_in=_ssq_parts(x).to(dev()), ssq_parts=K // 64, out=out, ldo=N, status=st)
    rs = math.sqrt(K) / x.double().norm(dim=-1, keepdim=True).clamp_min(1e-12)
    emu = torch.nn.functional.gelu(hl8_matmul(a8, w8)[:, :N] * rs + b)
    exact = torch.nn.functional.gelu(x.double() @ W.double().T * rs + b)
    got = from_hl32(out.cpu())
    e_emu, e_exact = _rel(got, emu), _rel(got, exact)
    report("gemm3_f8_ff1", M=M, K=K, N=N, rel_vs_same_arithmetic=e_emu, rel_vs_exact=e_exact)
    assert e_emu < 3e-6 and e_exact < 2e-4 and int(st.item()) == 0


@pytest.mark.parametrize("M,K,N", [(1500, 2048, 512), (777, 512, 512), (24000, 2048, 512), (32768, 1024, 512), (3000, 2048, 512)])
def test_gemm3_f8_resid(M, K, N):
    A = _mk((M, K), 4).float()
    W = _mk((N, K), 5, 0.5 / math.sqrt(K)).float()
    b = _mk((N,), 6)
    x0 = _mk((M, N), 7).float()
    x = x0.to(dev()).clone()
    xb = torch.full((M, 2 * N), float("nan"), dtype=torch.float16, device=dev())
    ssq = torch.full((N // 64, M), -1.0, dtype=torch.float32, device=dev())
    a8, w8 = to_hl8a(A), to_hl8(pad_rows(W, 256))
    st = _status()
    _call(0, 1 | F8_IN, A=a8.to(dev()), lda=K, M=M, K=K, W=w8.to(dev()), N=N, epi=1, bias=b.float().to(dev()), x=x, ldx=N, xb=xb,
          ssq_out=ssq, status=st)
    emu = x0.double() + hl8_matmul(a8, w8)[:, :N] + b
    exact = x0.double() + A.double() @ W.double().T + b
    e_emu, e_exact = _rel(x, emu), _rel(x, exact)
    xc = x.double().cpu()
    errb = float((from_hl32(xb.cpu()) - xc).abs().max() / xc.abs().max())
    report("gemm3_f8_resid", M=M, K=K, N=N, rel_vs_same_arithmetic=e_emu, rel_vs_exact=e_exact, shadow=errb)
    assert e_emu < 2e-6 and e_exact < 2e-4 and errb < 1e-6 and int(st.item()) == 0


@pytest.mark.parametrize("big,flag", [(1000.0, 0), (3500.0, 0), (3700.0, 1), (60000.0, 1)])
def test_gemm3_hl8_range_flag(big, flag):
    """the byte sections of an hl8 activation end at 3584 (e4m3's 448 x the 2^3 an activation's bytes are shifted by): a producer
    that writes a larger value raises the range flag (the forward is then repeated in exact fp32), below it the product is right"""
    M, K, N = 256, 128, 128
    A, W = _mk((M, K), 1).float(), torch.eye(N, K)
    x0 = torch.zeros((M, N))
    x0[5, 7] = big
    x = x0.to(dev()).clone()
    xb = torch.zeros((M, 2 * N), dtype=torch.float16, device=dev())
    st = _status()
    _call(0, 1 | F8_OUT, A=to_hl32(A).to(dev()), lda=K, M=M, K=K, W=to_hl32(pad_rows(W, 256)).to(dev()), N=N, epi=1, x=x, ldx=N, xb=xb,
          ssq_out=torch.zeros((N // 64, M), device=dev()), status=st)
    torch.cuda.synchronize()
    assert int(st.item()) == flag
    if not flag:
        hi, h8, l8 = hl8_parts(xb.cpu(), act=True)
        want = x.double().cpu()
        assert float((hi + l8 - want).abs().max() / big) < 2e-5 and float(((h8 - want).abs() - 0.07 * want.abs() - 0.02).max()) <= 0


def _check_hl8_against_hl32(o8, o32, what):
    """an hl8 activation a kernel wrote against the hl32 form of the same launch: the hi halves are the same bits, the hi bytes
    are e4m3 of the value and the lo bytes e4m3 of 2^11 (value - hi) -- up to the rare tie that the 22-bit hl32 value rounds the
    other way"""
    hi, h8, l8 = hl8_parts(o8, act=True)
    m, k2 = o32.shape
    p32 = o32.view(m, k2 // 64, 2, 32)
    hi32, lo32 = p32[:, :, 0].reshape(m, k2 // 2).double(), p32[:, :, 1].reshape(m, k2 // 2).double()
    assert torch.equal(hi, hi32), what
    v = hi32 + lo32
    s = HL8_ACT_SHIFT
    want_h8 = (v / s).float().clamp(-448, 448).to(torch.float8_e4m3fn).double() * s
    want_l8 = (lo32 * 2048.0 / s).float().clamp(-448, 448).to(torch.float8_e4m3fn).double() / 2048.0 * s
    bad_h = float((h8 != want_h8).double().mean())
    bad_l = float((l8 != want_l8).double().mean())
    # a mismatch is one e4m3 step at most (3 mantissa bits: 12.5 % of the value; subnormal step 2^-9 for the hi bytes, 2^-20 for the lo bytes)
    assert float(((h8 - want_h8).abs() - 0.126 * want_h8.abs() - s * 2.0 ** -9).max()) <= 0, what
    assert float(((l8 - want_l8).abs() - 0.126 * want_l8.abs() - s * 2.0 ** -20).max()) <= 0, what
    assert bad_h < 1e-3 and bad_l < 0.05, (what, bad_h, bad_l)
    return bad_h, bad_l


def test_gemm3_hl8_producers_and_the_feed_forward_chain():
    """What the fp8-cross-term feed-forward of a main layer runs (BT_OPT_X3_FF_FP8): the out-projection leaves an hl8 shadow of the
    residual stream, FF1 reads it and leaves an hl8 hidden activation, FF2 reads that.  Producers against the hl32 form of the
    same launch, the chain against the exact float64 feed-forward."""
    M, D, HID = 3000, 512, 2048
    ao = _mk((M, D), 1).float()
    x0 = _mk((M, D), 2, 2.0).float()
    Wo = _mk((D, D), 3, 1 / math.sqrt(D)).float()
    W1, b1 = _mk((HID, D), 4, 1 / math.sqrt(D)).float(), _mk((HID,), 5)
    W2, b2 = _mk((D, HID), 6, 0.5 / math.sqrt(HID)).float(), _mk((D,), 7)
    res = {}
    for mode in ("hl32", "hl8"):
        f8_out = F8_OUT if mode == "hl8" else 0
        f8_in = F8_IN if mode == "hl8" else 0
        pack = to_hl8 if mode == "hl8" else to_hl32
        x = x0.to(dev()).clone()
        xb = torch.zeros((M, 2 * D), dtype=torch.float16, device=dev())
        ssq = torch.zeros((D // 64, M), dtype=torch.float32, device=dev())
        _call(0, 1 | f8_out, A=to_hl32(ao).to(dev()), lda=D, M=M, K=D, W=to_hl32(pad_rows(Wo, 256)).to(dev()), N=D, epi=1, x=x, ldx=D, xb=xb,
              ssq_out=ssq, status=_status())                       # out-projection: hl32 operands, shadow in `mode`
        hid = torch.zeros((M, 2 * HID), dtype=torch.float16, device=dev())
        _call(0, 1 | f8_in | f8_out, A=xb, lda=D, M=M, K=D, W=pack(pad_rows(W1, 256)).to(dev()), N=HID, epi=0, bias=b1.float().to(dev()),
              ssq_in=ssq, ssq_parts=D // 64, out=hid, ldo=HID, status=_status())
        x2 = x.clone()
        xb2 = torch.zeros((M, 2 * D), dtype=torch.float16, device=dev())
        _call(0, 1 | f8_in, A=hid, lda=HID, M=M, K=HID, W=pack(pad_rows(W2, 256)).to(dev()), N=D, epi=1, bias=b2.float().to(dev()), x=x2, ldx=D,
              xb=xb2, ssq_out=torch.zeros((D // 64, M), device=dev()), status=_status())
        res[mode] = (xb.cpu(), hid.cpu(), x2.double().cpu(), xb2.cpu(), x.double().cpu())
    bh, bl = _check_hl8_against_hl32(res["hl8"][0], res["hl32"][0], "residual shadow")
    assert torch.equal(res["hl8"][4], res["hl32"][4])               # (the out-projection itself is the same launch)
    x1 = x0.double() + ao.double() @ Wo.double().T
    xn = x1 / x1.norm(dim=-1, keepdim=True).clamp_min(1e-12) * math.sqrt(D)
    h = torch.nn.functional.gelu(xn @ W1.double().T + b1)
    ref = x1 + h @ W2.double().T + b2
    e32, e8 = _rel(res["hl32"][2], ref), _rel(res["hl8"][2], ref)
    # the hidden activation of the hl8 chain was computed from hl8 operands, so it is compared with the exact one, not bit for bit
    hi, h8, l8 = hl8_parts(res["hl8"][1], act=True)
    eh = float(((hi + l8) - h).abs().max() / h.abs().max())
    report("gemm3_hl8_chain", M=M, rel_hl32=e32, rel_hl8=e8, hidden_rel=eh, shadow_hi_byte_mismatch=bh, shadow_lo_byte_mismatch=bl)
    assert e32 < 3e-6 and e8 < 1e-4 and eh < 1e-4
    assert float((from_hl32(res["hl8"][3]) - res["hl8"][2]).abs().max() / res["hl8"][2].abs().max()) < 1e-6   # FF2 leaves an hl32 shadow


def test_gemm3_x3_tile_configurations_agree_bit_for_bit():
    """128 x 128 tiles on k-steps of 32 and 256 x 128 tiles on k-steps of 16 issue the same MFMAs on the same operand pieces
    in the same order per output element: identical bits (a piece's result must not depend on the batch it ran in)."""
    M, K, N = 3000, 512, 1024
    x = _mk((M, K), 1, 2.0).float()
    W, b = _mk((N, K), 2, 1 / math.sqrt(K)).float(), _mk((N,), 3)
    outs = []
    for cfg in (3, 4, 5):
        out = torch.zeros((M, 2 * N), dtype=torch.float16, device=dev())
        _call(0, cfg, A=to_hl32(x).to(dev()), lda=K, M=M, K=K, W=to_hl32(pad_rows(W, 256)).to(dev()), N=N, epi=0, bias=b.float().to(dev()),
              ssq_in=_ssq_parts(x).to(dev()), ssq_parts=K // 64, out=out, ldo=N, status=_status())
        xr = _mk((M, N), 7).float().to(dev())
        xb = torch.zeros((M, 2 * N), dtype=torch.float16, device=dev())
        _call(0, cfg, A=to_hl32(x).to(dev()), lda=K, M=M, K=K, W=to_hl32(pad_rows(W, 256)).to(dev()), N=N, epi=1, bias=b.float().to(dev()),
              x=xr, ldx=N, xb=xb, ssq_out=torch.zeros((N // 64, M), device=dev()), status=_status())
        outs.append((out, xr, xb))
    for other in outs[1:]:
        for a, c in zip(outs[0], other):
            assert torch.equal(a, c)


@pytest.mark.parametrize("f8", [False, True])   # (True: hl8 operands, BT_OPT_X3_GEMM_FP8 = 2)
@pytest.mark.parametrize("n_seq,L,heads", [(2, 1500, 4), (3, 77, 4), (1, 1, 4), (5, 130, 8), (16, 1500, 16)])
def test_gemm3_x3_qkv(n_seq, L, heads, f8):
    from beat_this_amd import _lib as Lb
    from beat_this_amd.pack import LOG2E
    from beat_this_amd.tables import rope_table

    D = heads * 32
    M = n_seq * L
    x = _mk((M, D), 10, 1.5).float()
    Wqkv = _mk((3 * D, D), 11, 1.6 / math.sqrt(D))
    Wqkv[:D] *= LOG2E / math.sqrt(32.0)
    Wg, bg = _mk((heads, D), 12, 0.3), _mk((heads,), 13, 0.3)
    W = pad_rows(torch.cat([Wqkv, Wg]).float(), 256)
    freqs = 10000.0 ** (-torch.arange(0, 32, 2).float() / 32)
    rope = torch.from_numpy(rope_table(freqs)).to(dev())
    nbp = Lb.lib().bt_attn_frag_blocks(L)
    SH = n_seq * heads
    qf = torch.full((SH, nbp, 2, 1024), float("nan"), dtype=torch.float16, device=dev())
    kf, vf = qf.clone(), qf.clone()
    gh = torch.zeros((SH, nbp * 32), dtype=torch.float32, device=dev())
    st = _status()
    pack = to_hl8 if f8 else to_hl32
    packa = to_hl8a if f8 else to_hl32
    _call(0, 1 | (F8_IN if f8 else 0), A=packa(x).to(dev()), lda=D, M=M, K=D, W=pack(W).to(dev()), N=3 * D + heads, epi=2,
          ssq_in=_ssq_parts(x).to(dev()), ssq_parts=D // 64, n_seq=n_seq, L=L, nbp=nbp, heads=heads, rope=rope, qf=qf, kf=kf, vf=vf,
          gates=gh, b_gates=bg.float().to(dev()), status=st)
    rs = math.sqrt(D) / x.double().norm(dim=-1, keepdim=True).clamp_min(1e-12)
    Wd, xd = from_hl32(to_hl32(W)), from_hl32(to_hl32(x))
    prod = hl8_matmul(packa(x), pack(W)) if f8 else xd @ Wd.T   # (hl8: against the float64 evaluation of the same arithmetic)
    qkv = (prod[:, :3 * D] * rs).view(n_seq, L, 3, heads, 32).permute(2, 0, 3, 1, 4)  # qkv s h t d
    ang = torch.arange(L, dtype=torch.float64)[:, None] * freqs.double()[None, :]
    cos, sin = ang.cos().repeat_interleave(2, -1), ang.sin().repeat_interleave(2, -1)

    def rot(t):
        te, to = t[..., 0::2], t[..., 1::2]
        return t * cos + torch.stack((-to, te), -1).flatten(-2) * sin
    q, k, v = rot(qkv[0]).reshape(SH, L, 32), rot(qkv[1]).reshape(SH, L, 32), qkv[2].reshape(SH, L, 32)
    gates = torch.sigmoid(prod[:, 3 * D:3 * D + heads] * rs + bg).view(n_seq, L, heads).permute(0, 2, 1).reshape(SH, L)
    nblk = (L + 31) // 32
    eq = _rel(unfrag_x3(qf.cpu()[:, :nblk], L, "qk"), q)
    ek = _rel(unfrag_x3(kf.cpu()[:, :nblk], L, "qk"), k)
    ev = _rel(unfrag_x3(vf.cpu()[:, :nblk], L, "v"), v)
    eg = _rel(gh.cpu()[:, :L], gates)
    report("gemm3_x3_qkv", n_seq=n_seq, L=L, heads=heads, f8=f8, q=eq, k=ek, v=ev, gates=eg)
    # (q, k: the rotary angles pos * freq are fp32 products like rotary-embedding-torch's -- 1e-4 rad at position 1500 -- so
    # against this float64 restatement the rotated values are 2e-5 off at L = 1500; v has no rotation)
    assert max(eq, ek) < (3e-6 if L < 200 else 4e-5) and ev < 3e-6 and eg < 3e-6 and int(st.item()) == 0
    if L % 32:  # tokens beyond L inside the last block: exact zeros for K and V, hi and lo
        tail_k = kf.cpu()[:, nblk - 1].view(SH, 2, 4, 32, 8)[:, :, :, L % 32:, :]
        assert torch.all(tail_k.float() == 0)
        assert torch.all(unfrag_x3(vf.cpu()[:, nblk - 1:nblk], 32, "v")[:, L % 32:] == 0)


@pytest.mark.parametrize("B,T,Fp,C2,N,planes_only", [(2, 50, 8, 128, 128, False), (1, 33, 4, 256, 256, True), (3, 7, 16, 128, 128, False),
                                                     (16, 1500, 4, 256, 256, True)])
def test_gemm3_x3_frontend_conv(B, T, Fp, C2, N, planes_only):
    """epi 1 as the (2,3) / stride (2,1) frontend convolution on the hl32 (b, t, f, c) activation: three time taps gathered
    by the LDS-DMA loader (zero rows outside 0 <= t < T), bias, exact erf GELU; fp32 output or hl32 planes only."""
    M = B * T * Fp
    xin = _mk((M, C2), 20, 1.2).float()
    W = _mk((N, 3 * C2), 21, 1 / math.sqrt(3 * C2)).float()
    b = _mk((N,), 22, 0.3)
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=dev())
    outb = torch.full((M, 2 * N), float("nan"), dtype=torch.float16, device=dev())
    _call(A=to_hl32(xin).to(dev()), lda=C2, M=M, K=3 * C2, W=to_hl32(pad_rows(W, 256)).to(dev()), N=N, epi=1, bias=b.float().to(dev()),
          x=0 if planes_only else out, ldx=N, xb=outb, no_resid=1, gelu=1, conv_C2=C2, conv_T=T, conv_F=Fp)
    x4 = xin.double().view(B, T, Fp, C2)
    pad = torch.zeros((B, 1, Fp, C2), dtype=torch.float64)
    taps = torch.cat([torch.cat([pad, x4[:, :-1]], 1), x4, torch.cat([x4[:, 1:], pad], 1)], -1).reshape(M, 3 * C2)
    ref = torch.nn.functional.gelu(taps @ W.double().T + b)
    errb = _rel(from_hl32(outb.cpu()), ref)
    err = errb if planes_only else _rel(out, ref)
    report("gemm3_x3_conv", B=B, T=T, Fp=Fp, C2=C2, N=N, rel=err, planes=errb)
    assert err < 3e-6 and errb < 3e-6


def test_gemm3_x3_range_flag():
    """A value beyond the fp16 range of a hi part raises the flag (and only then)."""
    M, K, N = 256, 128, 128
    A = _mk((M, K), 30).float()
    W = _mk((N, K), 31, 0.1).float()
    x0 = torch.zeros((M, N))
    for boost, expect in ((1.0, 0), (1e6, 1)):
        x = (x0 + (boost if expect else 0.0)).float().to(dev())
        xb = torch.zeros((M, 2 * N), dtype=torch.float16, device=dev())
        st = _status()
        _call(A=to_hl32(A).to(dev()), lda=K, M=M, K=K, W=to_hl32(pad_rows(W, 256)).to(dev()), N=N, epi=1, x=x, ldx=N, xb=xb, status=st)
        assert int(st.item()) == expect


# ---- attention ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [1, 2, 5])   # bt_attn_frag_args.x3: keys per LDS tile / 5 = the hand-scheduled two-query-block kernel, forced (4 = by launch size; attn2.hip)
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("n_seq,L,heads", [(3, 1500, 2), (2, 77, 1), (1, 128, 4), (5, 1012, 1), (2, 1, 1), (2, 33, 2),
                                           (1, 1499, 1), (2, 129, 1), (9, 96, 1), (2, 257, 1), (2, 250, 1), (1, 64, 1)])
def test_attention_frag_x3(n_seq, L, heads, out_f32, variant):
    SH = n_seq * heads
    q = _mk((SH, L, 32), 30, 0.6).float().double()
    k = _mk((SH, L, 32), 31).float().double()
    v = _mk((SH, L, 32), 32).float().double()
    k[0, 7 % L] *= 6.0  # one outlier key
    k = k.float().double()
    gates = torch.sigmoid(_mk((SH, L), 33)).float().double()
    out = _run_attn(q, k, v, gates, n_seq, L, heads, out_f32, variant)
    ref = _attn_ref(q, k, v, gates).view(n_seq, heads, L, 32).permute(0, 2, 1, 3).reshape(n_seq * L, heads * 32)
    err = _rel(out, ref)
    report("attn_frag_x3", n_seq=n_seq, L=L, heads=heads, out_f32=out_f32, variant=variant, rel=err)
    # hi + lo is a 22-bit representation: a score s = q . k carries an error of ~2^-22 |q| |k| / sqrt(32) and the
    # probability a relative error of ln 2 times that.  The outlier key (6 x) of sequence 0 makes |s| ~ 60: 1.1e-5 at
    # L = 1500 (the exact fp32 MFMA kernel: 2.7e-6 on the same inputs), 2e-6 .. 4e-6 on the ordinary sequences.
    assert err < (8e-6 if L <= 300 else 2e-5)


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("n_seq,L,heads", [(3, 1500, 2), (2, 257, 1), (1, 64, 1), (2, 77, 1), (1, 1499, 1), (2, 128, 2)])
def test_attention_frag_x3_variants_agree_bit_for_bit(n_seq, L, heads, out_f32):
    """The forward picks the x3 attention kernel by launch size (64-key tiles for small launches, the hand-scheduled
    two-query-block kernel for large ones): every kernel must produce the SAME bits -- same products in the same order, same
    row-sum tree, the reference maximum on the accumulator input everywhere -- or a piece's logits (and, through an exact
    x == maxpool(x) comparison, its beats) would depend on what else was in the batch."""
    SH = n_seq * heads
    q = _mk((SH, L, 32), 30, 0.6).float().double()
    k = _mk((SH, L, 32), 31).float().double()
    v = _mk((SH, L, 32), 32).float().double()
    gates = torch.sigmoid(_mk((SH, L), 33)).float().double()
    outs = [_run_attn(q, k, v, gates, n_seq, L, heads, out_f32, variant) for variant in (1, 2, 5)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


# ---- P16 (round 5, the forward's default; bt_attn_frag_args.x3 + 8): probabilities enter P.V as fp16 hi parts ---------------------
def _attn_ref_p16(q, k, v, gates):
    """float64 restatement of the P16 arithmetic: probabilities relative to the reference point of the fast pass (the maximum
    over the first two key blocks and the query's own key block, rounded up to a whole octave, plus three octaves of headroom)
    -- or, for the queries whose fast pass overflows fp16, of the re-run (row maximum at 2^14 .. 2^15) -- rounded to fp16, the
    SAME rounded values in numerator and denominator."""
    s = q @ k.transpose(-1, -2)                      # base-2 exponents: q carries log2(e) / sqrt(d)
    L = s.shape[-1]
    own = torch.arange(L)[:, None] // 32 == torch.arange(L)[None, :] // 32          # [query, key]: same 32-token block
    lead = (torch.arange(L) < 64)[None, :].expand(L, L)
    m = torch.ceil(s.masked_fill(~(own | lead), -1e30).max(-1).values) + 3.0
    over = (s.max(-1).values - m) >= 15.99
    m = torch.where(over, torch.ceil(s.max(-1).values) - 14.0, m)
    h = torch.exp2(s - m[..., None]).float().to(torch.float16).double()
    return h @ v / h.sum(-1, keepdim=True) * gates[..., None]


@pytest.mark.parametrize("variant", [9, 10, 13])
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("n_seq,L,heads", [(3, 1500, 2), (2, 77, 1), (1, 128, 4), (5, 1012, 1), (2, 1, 1), (2, 33, 2),
                                           (1, 1499, 1), (2, 129, 1), (9, 96, 1), (2, 257, 1), (2, 250, 1), (1, 64, 1)])
def test_attention_frag_x3_p16(n_seq, L, heads, out_f32, variant):
    SH = n_seq * heads
    q = _mk((SH, L, 32), 30, 0.6).float().double()
    k = _mk((SH, L, 32), 31).float().double()
    v = _mk((SH, L, 32), 32).float().double()
    k[0, 7 % L] *= 6.0  # one outlier key
    k = k.float().double()
    gates = torch.sigmoid(_mk((SH, L), 33)).float().double()
    out = _run_attn(q, k, v, gates, n_seq, L, heads, out_f32, variant)

    def rows(t):
        return t.view(n_seq, heads, L, 32).permute(0, 2, 1, 3).reshape(n_seq * L, heads * 32)
    err_sim = _rel(out, rows(_attn_ref_p16(q, k, v, gates)))
    err = _rel(out, rows(_attn_ref(q, k, v, gates)))
    report("attn_frag_x3_p16", n_seq=n_seq, L=L, heads=heads, out_f32=out_f32, variant=variant, rel=err, rel_vs_p16_restatement=err_sim)
    # against the restatement of its own arithmetic the kernel is as exact as the three-term one (what remains: the 22-bit
    # scores, and a probability here and there that rounds the other way because the reference point differs in its last
    # bit); against the exact softmax it carries the fp16 rounding of the probabilities, damped by the common denominator
    assert err_sim < 1.5e-4 and err < 3e-4   # (measured: 7e-6 .. 9e-5 against the restatement, 7e-5 .. 1.5e-4 against the exact softmax)


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("n_seq,L,heads", [(3, 1500, 2), (2, 257, 1), (1, 64, 1), (2, 77, 1), (1, 1499, 1), (2, 128, 2)])
def test_attention_frag_x3_p16_variants_agree_bit_for_bit(n_seq, L, heads, out_f32):
    """as test_attention_frag_x3_variants_agree_bit_for_bit, for the P16 arithmetic: 128-key tiles, 64-key tiles and the
    hand-scheduled statement ATTN_X3Q2P_ASM (row sums on 4x4x4 MFMAs in the same order everywhere)"""
    SH = n_seq * heads
    q = _mk((SH, L, 32), 30, 0.6).float().double()
    k = _mk((SH, L, 32), 31).float().double()
    v = _mk((SH, L, 32), 32).float().double()
    gates = torch.sigmoid(_mk((SH, L), 33)).float().double()
    outs = [_run_attn(q, k, v, gates, n_seq, L, heads, out_f32, variant) for variant in (9, 10, 13)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    three_term = _run_attn(q, k, v, gates, n_seq, L, heads, out_f32, 2)
    assert not torch.equal(outs[0], three_term) or L == 1   # (the option does select another arithmetic)


@pytest.mark.parametrize("variant", [1, 5, 9, 10, 13])
@pytest.mark.parametrize("n_seq,L,heads", [(3, 1500, 2), (2, 77, 1), (1, 128, 4), (2, 1, 1), (2, 33, 2), (4, 1500, 16)])
def test_attention_frag_x3_hl8_rows(n_seq, L, heads, variant):
    """bt_attn_frag_args.out_f32 = 2 (BT_OPT_X3_GEMM_FP8 = 2: the out-projection reads hl8 rows): the same launch as the hl32 one
    -- hi halves bit for bit, the byte sections e4m3 of the value and of 2^11 (value - hi)"""
    SH = n_seq * heads
    q = _mk((SH, L, 32), 30, 0.6).float().double()
    k = _mk((SH, L, 32), 31).float().double()
    v = _mk((SH, L, 32), 32).float().double()
    gates = torch.sigmoid(_mk((SH, L), 33)).float().double()
    o32 = _run_attn(q, k, v, gates, n_seq, L, heads, 0, variant, raw=True)
    o8 = _run_attn(q, k, v, gates, n_seq, L, heads, 2, variant, raw=True)
    bh, bl = _check_hl8_against_hl32(o8, o32, "attention rows")
    report("attn_frag_x3_hl8_rows", n_seq=n_seq, L=L, heads=heads, variant=variant, hi_byte_mismatch=bh, lo_byte_mismatch=bl)


@pytest.mark.parametrize("variant", [9, 10, 13])
@pytest.mark.parametrize("L", [300, 1500])
def test_attention_frag_x3_p16_overflow_fallback(L, variant):
    """the re-run on the row maxima (a key 16 + 4 octaves above the reference point of the fast pass) in the P16 arithmetic:
    an fp16 overflow of a probability is inf in the row sum taken from the rounded values"""
    SH = 3
    q = _mk((SH, L, 32), 50, 0.5)
    k = _mk((SH, L, 32), 51)
    v = _mk((SH, L, 32), 52)
    q[1, 5] = 0.0
    q[1, 5, 0] = 25.0
    k[1, L - 40] = 0.0
    k[1, L - 40, 0] = 24.0
    q, k, v = (t.float().double() for t in (q, k, v))
    gates = torch.ones((SH, L), dtype=torch.float64)
    out = _run_attn(q, k, v, gates, SH, L, 1, True, variant)
    ref = _attn_ref(q, k, v, gates).reshape(SH * L, 32)
    assert torch.isfinite(out).all()
    err = _rel(out, ref)
    report("attn_frag_x3_p16_overflow", L=L, variant=variant, rel=err)
    assert err < 3e-4


@pytest.mark.parametrize("out_f32", [0, 1])
@pytest.mark.parametrize("variant", [5, 13, 10])
def test_attention_frag_x3_hopeless_scores_raise_the_range_flag(variant, out_f32):
    """scores of ~1e6 whose hi . hi part alone is hundreds of units away from the full hi + lo score -- the fix-up
    launch's reference point (row maxima of the hi . hi scores + 2 octaves) then does not bound the probabilities, a row sum is
    inf (P16: the fp16 probability itself) or NaN, and gate / inf x inf = NaN rows used to be stored with the range flag down
    (fmaxf drops NaNs).  Now: either every row is finite, or the flag is up (the forward repeats such a batch in exact fp32)."""
    SH, L = 2, 300
    q = (_mk((SH, L, 32), 70) * 1000.0).float().double()
    k = (_mk((SH, L, 32), 71) * 1000.0).float().double()
    v = _mk((SH, L, 32), 72).float().double()
    gates = torch.ones((SH, L), dtype=torch.float64)
    flag = []
    out = _run_attn(q, k, v, gates, SH, L, 1, out_f32, variant, status_out=flag)
    finite = bool(torch.isfinite(out).all())
    report("attn_frag_x3_hopeless_scores", variant=variant, out_f32=out_f32, flag=flag[0], finite=finite)
    assert (flag[0] & 1) or finite, "non-finite attention rows with the range flag down"


@pytest.mark.parametrize("out_f32", [0, 1, 2])
@pytest.mark.parametrize("variant", [5, 13])
@pytest.mark.parametrize("L,heads,n_over", [(1500, 2, 1), (1500, 1, 40), (1500, 1, 200), (2300, 1, 70), (77, 2, 5), (33, 1, 33)])
def test_attention_frag_x3_fixup_launch(L, heads, n_over, variant, out_f32):
    """The queries whose fast pass overflows fp16 are left to the gathered fix-up launch (attn_fix_x3_kernel: 32 per round, keys
    split over the waves): one, more than a round, more than four rounds of them in a pair, sequences of more than 64 key blocks
    (the map is read 64 words at a time), short ones (waves without keys), in every output form -- against the exact softmax, and
    the other queries bit for bit what a launch without the overflowing key gives."""
    n_seq = 2
    SH = n_seq * heads
    q = _mk((SH, L, 32), 60, 0.5)
    k = _mk((SH, L, 32), 61)
    v = _mk((SH, L, 32), 62)
    q, k, v = (t.float().double() for t in (q, k, v))
    gates = torch.ones((SH, L), dtype=torch.float64)
    idx = [(37 * j + 5) % L for j in range(n_over)]
    q[SH - 1, idx] = 0.0
    q[SH - 1, idx, 1] = 25.0                 # these queries score key L - 9 at 600: far beyond the fast pass's headroom ...
    clean = _run_attn(q, k, v, gates, n_seq, L, heads, out_f32, variant)
    k[SH - 1, L - 9] = 0.0
    k[SH - 1, L - 9, 1] = 24.0               # ... once it is there (the other queries of the pair see it at |24 q_1| <= 25 or so)
    out = _run_attn(q, k, v, gates, n_seq, L, heads, out_f32, variant)
    assert torch.isfinite(out).all()
    assert torch.equal(out, _run_attn(q, k, v, gates, n_seq, L, heads, out_f32, variant))   # (no atomics, fixed summation order)
    if variant == 13:   # the kernel form in front does not matter: the 64-key-tile kernels leave the same queries to the same launch
        assert torch.equal(out, _run_attn(q, k, v, gates, n_seq, L, heads, out_f32, 10))
    ref = _attn_ref(q, k, v, gates).view(n_seq, heads, L, 32).permute(0, 2, 1, 3).reshape(n_seq * L, heads * 32)
    err = _rel(out, ref)
    report("attn_frag_x3_fixup", L=L, heads=heads, n_over=n_over, variant=variant, out_f32=out_f32, rel=err)
    assert err < (1e-5 if variant < 8 else 3e-4) + (1e-4 if out_f32 == 2 else 0)   # (hl8 rows: read back through their hi halves + lo bytes)
    if heads > 1:   # the other head of the last sequence never sees the changed key: the same bits with and without it
        cols = slice(0, 32 * (heads - 1))
        assert torch.equal(out[:, cols], clean[:, cols])
    assert torch.equal(out[:L], clean[:L])   # (the first sequence)


@pytest.mark.parametrize("base", [0, 8])
def test_attention_frag_x3_overflow_rerun_is_per_query(base):
    """A query whose fast pass overflows re-runs its WORKGROUP, but only that query takes the new reference point: the other
    queries of the workgroup reproduce their first result.  So the kernels with 128-query workgroups (64- / 128-key tiles) and
    the one with 256-query workgroups still agree bit for bit when an overflow occurs, and queries far from the overflowing
    one are bit-identical to a launch without it."""
    SH, L = 2, 1500
    q = _mk((SH, L, 32), 50, 0.5)
    k = _mk((SH, L, 32), 51)
    v = _mk((SH, L, 32), 52)
    q, k, v = (t.float().double() for t in (q, k, v))
    gates = torch.ones((SH, L), dtype=torch.float64)
    clean = _run_attn(q, k, v, gates, SH, L, 1, True, base + 2)
    q2, k2 = q.clone(), k.clone()
    q2[1, 5] = 0.0
    q2[1, 5, 0] = 25.0          # query 5 of sequence 1 scores key L - 40 at 600: far beyond the fast pass's headroom
    k2[1, L - 40] = 0.0
    k2[1, L - 40, 0] = 24.0
    outs = [_run_attn(q2, k2, v, gates, SH, L, 1, True, base + variant) for variant in (1, 2, 5)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    # sequence 0 is untouched; in sequence 1 every query sees the changed key, so only sequence 0 can be compared with `clean`
    assert torch.equal(outs[0][:L], clean[:L])
    ref = _attn_ref(q2, k2, v, gates).reshape(SH * L, 32)
    assert _rel(outs[0], ref) < (8e-6 if base == 0 else 3e-4)


def test_attention_frag_x3_time_direction_rowmap():
    B, T, F, heads = 2, 150, 4, 1
    SH = B * F
    q, k, v = (_mk((SH, T, 32), 40 + i).float().double() for i in range(3))
    gates = torch.sigmoid(_mk((SH, T), 44)).float().double()
    out = _run_attn(q, k, v, gates, SH, T, heads, True, 5, o_div=F, o_outer=T * F, o_inner=1, o_tok=F)
    ref = _attn_ref(q, k, v, gates).view(B, F, T, 32).permute(0, 2, 1, 3).reshape(B * T * F, 32)
    err = _rel(out, ref)
    report("attn_frag_x3_rowmap", rel=err)
    assert err < 6e-6


@pytest.mark.parametrize("variant", [1, 2, 5])
@pytest.mark.parametrize("L", [300, 1500])
def test_attention_frag_x3_overflow_fallback(L, variant):
    """Scores that exceed the first key block's maximum by more than the fp16 probabilities can hold force the SAFE
    (running-max) pass of the workgroup; the result must still be the exact softmax."""
    SH = 3
    q = _mk((SH, L, 32), 50, 0.5)
    k = _mk((SH, L, 32), 51)
    v = _mk((SH, L, 32), 52)
    q[1, 5] = 0.0
    q[1, 5, 0] = 25.0
    k[1, L - 40] = 0.0
    k[1, L - 40, 0] = 24.0
    q, k, v = (t.float().double() for t in (q, k, v))
    gates = torch.ones((SH, L), dtype=torch.float64)
    out = _run_attn(q, k, v, gates, SH, L, 1, True, variant)
    ref = _attn_ref(q, k, v, gates).reshape(SH * L, 32)
    assert torch.isfinite(out).all()
    err = _rel(out, ref)
    report("attn_frag_x3_overflow", L=L, rel=err)
    assert err < 8e-6


@pytest.mark.parametrize("variant", [1, 2, 4, 5, 12, 13])
def test_attention_frag_x3_at_scale_is_repeatable(variant):
    """The main-layer launch shape of a 16-chunk batch (256 sequence-heads x 1500 tokens) four times: bit-identical.
    (Round 3: the 64-key variant, capped to 128 registers, spilled two of them around the key loop; the reloads raced the
    LDS-DMA in flight and a 16-chunk forward differed from run to run -- the single-launch parity tests never saw it.)"""
    n_seq, L, heads = 16, 1500, 16
    SH = n_seq * heads
    q, k, v = (_mk((SH, L, 32), 60 + i, 0.7).float() for i in range(3))
    gates = torch.sigmoid(_mk((SH, L), 63)).float()
    from beat_this_amd import _lib as Lb

    nbp = Lb.lib().bt_attn_frag_blocks(L)
    qd, kd, vd = (frag_x3(t, nbp, kind).to(dev()) for t, kind in ((q, "qk"), (k, "qk"), (v, "v")))
    gh = torch.zeros((SH, nbp * 32), dtype=torch.float32)
    gh[:, :L] = gates
    gd = gh.to(dev())
    outs = []
    for _ in range(4):
        out = torch.zeros((n_seq * L, 2 * heads * 32), dtype=torch.float16, device=dev())
        a = Lb.AttnFragArgs()
        a.q, a.k, a.v, a.gates, a.out = qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), gd.data_ptr(), out.data_ptr()
        a.n_seq, a.L, a.heads, a.inner, a.nbp, a.o_div, a.o_outer, a.o_inner, a.o_tok = n_seq, L, heads, heads * 32, nbp, 1, L, 0, 1
        a.x3, a.out_f32, a.status = variant, 0, 0
        scratch = torch.zeros((SH, nbp), dtype=torch.int32, device=dev())
        a.scratch = scratch.data_ptr()
        Lb.check(Lb.lib().bt_attention_frag(Lb.stream_ptr(dev()), C.byref(a)))
        outs.append((out, scratch))
    torch.cuda.synchronize()
    outs = [o for o, _ in outs]
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    # spot check of two sequence-heads against fp64
    for sh in (0, SH - 1):
        ref = _attn_ref(q[sh].double(), k[sh].double(), v[sh].double(), gates[sh].double())
        s_, h_ = divmod(sh, heads)
        got = from_hl32(outs[0].cpu()[s_ * L:(s_ + 1) * L])[:, h_ * 32:(h_ + 1) * 32]
        e = _rel(got, ref)
        assert e < (1.5e-5 if variant < 8 else 3e-4), e


# ---- frontend: time-direction QKV projection and the shadow of the fused out-projection + FF kernel -------------------------
def _pair_sd(Cc, seed):
    H = Cc // 32
    g = torch.Generator().manual_seed(seed)

    def rn(*shape, s=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * s
    return {
        "a.norm.gamma": 1 + 0.1 * rn(Cc), "a.to_qkv.weight": rn(3 * Cc, Cc, s=1.6 / math.sqrt(Cc)),
        "a.to_gates.weight": rn(H, Cc, s=0.3), "a.to_gates.bias": rn(H, s=0.3),
        "a.to_out.0.weight": rn(Cc, Cc, s=1 / math.sqrt(Cc)),
        "f.net.0.gamma": 1 + 0.1 * rn(Cc), "f.net.1.weight": rn(4 * Cc, Cc, s=1 / math.sqrt(Cc)),
        "f.net.1.bias": rn(4 * Cc, s=0.2), "f.net.4.weight": rn(Cc, 4 * Cc, s=0.5 / math.sqrt(Cc)),
        "f.net.4.bias": rn(Cc, s=0.2),
    }


@pytest.mark.parametrize("Cc", [32, 64, 128])
@pytest.mark.parametrize("T", [70, 1500])
def test_qkv_front_x3(Cc, T):
    from beat_this_amd import _lib as L
    from beat_this_amd.pack import LOG2E, PackedPair
    from beat_this_amd.tables import rope_table

    H, F = Cc // 32, 1024 // Cc
    B = 2 if T < 1000 else 1
    if T >= 1000:
        F = 2
    sd = {k: v.float().double() for k, v in _pair_sd(Cc, 170 + Cc).items()}   # fp32-representable weights
    x0 = _mk((B, T, F, Cc), 180 + Cc, 1.5).float()
    freqs = 10000.0 ** (-torch.arange(0, 32, 2).float() / 32)
    rope = torch.from_numpy(rope_table(freqs)).to(dev())
    pp = PackedPair(sd, "a.", "f.", Cc, dev())
    assert pp.weights.w_qkv_frag_x3
    nbp = L.lib().bt_attn_frag_blocks(T)
    SH = B * F * H
    qf = torch.full((SH, nbp, 2, 1024), float("nan"), dtype=torch.float16, device=dev())
    kf, vf = qf.clone(), qf.clone()
    gh = torch.zeros((SH, nbp * 32), dtype=torch.float32, device=dev())
    xd = x0.to(dev())
    L.check(L.lib().bt_qkv_front(L.stream_ptr(dev()), L.PREC_F32X3, C.byref(pp.weights), rope.data_ptr(), xd.data_ptr(), B, T, F,
                                 qf.data_ptr(), kf.data_ptr(), vf.data_ptr(), gh.data_ptr(), nbp))
    torch.cuda.synchronize()
    x = x0.double()
    xn = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12) * math.sqrt(Cc)
    wq = (sd["a.to_qkv.weight"] * sd["a.norm.gamma"][None, :]).float().double()   # (gamma is folded at pack time, in fp32)
    qkv = (xn @ wq.T).reshape(B, T, F, 3, H, 32).permute(3, 0, 2, 4, 1, 5)  # qkv b f h t d
    ang = torch.arange(T, dtype=torch.float64)[:, None] * freqs.double()[None, :]
    cos, sin = ang.cos().repeat_interleave(2, -1), ang.sin().repeat_interleave(2, -1)

    def rot(t):
        te, to = t[..., 0::2], t[..., 1::2]
        return t * cos + torch.stack((-to, te), -1).flatten(-2) * sin
    q = rot(qkv[0]).reshape(SH, T, 32) * (LOG2E / math.sqrt(32.0))
    k = rot(qkv[1]).reshape(SH, T, 32)
    v = qkv[2].reshape(SH, T, 32)
    gates = torch.sigmoid(xn @ (sd["a.to_gates.weight"] * sd["a.norm.gamma"][None, :]).T + sd["a.to_gates.bias"])
    gates = gates.permute(0, 2, 3, 1).reshape(SH, T)
    nblk = (T + 31) // 32
    eq = _rel(unfrag_x3(qf.cpu()[:, :nblk], T, "qk"), q)
    ek = _rel(unfrag_x3(kf.cpu()[:, :nblk], T, "qk"), k)
    ev = _rel(unfrag_x3(vf.cpu()[:, :nblk], T, "v"), v)
    eg = _rel(gh.cpu()[:, :T], gates)
    report("qkv_front_x3", C=Cc, T=T, q=eq, k=ek, v=ev, gates=eg)
    assert max(eq, ek) < (6e-6 if T < 200 else 4e-5) and ev < 6e-6 and eg < 6e-6   # (q, k at T = 1500: fp32 rotary angles, see above)
    if T % 32:
        tail_k = kf.cpu()[:, nblk - 1].view(SH, 2, 4, 32, 8)[:, :, :, T % 32:, :]
        assert torch.all(tail_k.float() == 0)


@pytest.mark.parametrize("Cc", [64, 128])
def test_fused_out_ff_x3_shadow(Cc):
    """The hl32 shadow the (hi, lo) out-projection + FF kernel leaves for the following convolution equals its fp32 result."""
    from beat_this_amd import _lib as L
    from beat_this_amd.pack import PackedPair

    sd = _pair_sd(Cc, 250 + Cc)
    M = 1000 + Cc
    x0 = _mk((M, Cc), 260 + Cc, 1.5)
    ao = _mk((M, Cc), 270 + Cc).float()
    pp = PackedPair(sd, "a.", "f.", Cc, dev())
    x = x0.float().to(dev()).clone()
    xb = torch.full((M, 2 * Cc), float("nan"), dtype=torch.float16, device=dev())
    L.check(L.lib().bt_outff_fused(L.stream_ptr(dev()), L.PREC_F32X3, C.byref(pp.weights), ao.to(dev()).data_ptr(), x.data_ptr(), M,
                                   xb.data_ptr()))
    torch.cuda.synchronize()
    xc = x.double().cpu()
    err = float((from_hl32(xb.cpu()) - xc).abs().max() / xc.abs().max())
    report("outff_x3_shadow", C=Cc, rel=err)
    assert err < 1e-6
