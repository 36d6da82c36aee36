"""Work that the BT_PREC_F32X3 forward used to do for padding of its 1500-frame chunks, and the forms that leave it out -- each
against the form that still does it, BIT FOR BIT:

  * attention (csrc/attn2.hip): T = 1500 is 47 query blocks on 48 slots of the two-query-block kernel; the wave whose second
    block does not exist runs the one-block statement of the hand-scheduled loop (tools/gen/attn_x3_loop.py) -- against the
    one-query-block kernels (128-key and 64-key tiles), which never had a second block;
  * QKV projection (csrc/gemm3.hip): the gate columns (3 inner + heads) on their own narrow tile -- against the generic
    128-column tile (x3 & 15 = 3, the configuration tools/gemm3_fuzz.py forces);
  * stores nobody reads (csrc/engine.hip plan_route: x_dead, shadow_dead): the fp32 x of frontend blocks 1 and 2 whose conv reads
    the hl32 shadow, and the shadow / statistics behind the last layer's FF2 when the head follows -- the buffers they used to
    fill hold NaN patterns instead, and the logits are those of a forward on a clean workspace.

Nothing here has a tolerance: the forms issue the same MFMAs on the same operand pieces in the same order per output element."""
import pytest
import torch

from gpu_util import POISONS, dev, from_hl32, pad_rows, to_hl32
from test_gpu_guard import _chunk, _forward, _model, _same
from test_gpu_x3 import _call, _mk, _run_attn, _ssq_parts, _status

pytestmark = pytest.mark.gpu

# L: odd block counts (1500 -> 47, 200 -> 7: the last wave with a block holds ONE), even ones (1012 -> 32, 1472 -> 46: the waves
# behind the last block hold none), exact multiples of 32 (1472, 1504 -> 47, 1536 -> 48: no masked last block) and a single wave
# (33 -> 2 blocks, one of them masked).  (n_seq, heads): the main layers' 16 heads, the frontend's time direction (many
# sequences of 1 .. 4 heads).
ATTN_CASES = [(2, 1500, 16), (24, 1500, 2), (3, 1012, 4), (8, 200, 2), (2, 1472, 4), (3, 1504, 2), (2, 1536, 4), (5, 33, 1)]


def _attn_inputs(n_seq, L, heads, seed=70):
    SH = n_seq * heads
    q = _mk((SH, L, 32), seed, 0.6).float().double()
    k = _mk((SH, L, 32), seed + 1).float().double()
    v = _mk((SH, L, 32), seed + 2).float().double()
    gates = torch.sigmoid(_mk((SH, L), seed + 3)).float().double()
    return q, k, v, gates


@pytest.mark.parametrize("p16", [0, 8])        # (bt_attn_frag_args.x3 + 8: the P16 arithmetic, the forward's default)
@pytest.mark.parametrize("out_f32", [0, 1])    # hl32 rows of the main layers / fp32 rows of the frontend
@pytest.mark.parametrize("n_seq,L,heads", ATTN_CASES)
def test_two_block_kernel_without_the_padding_block_agrees_bit_for_bit(n_seq, L, heads, out_f32, p16):
    q, k, v, gates = _attn_inputs(n_seq, L, heads)
    two = _run_attn(q, k, v, gates, n_seq, L, heads, out_f32, 5 + p16, raw=True)
    for one_block in (1, 2):                   # 128-key tiles, 64-key tiles
        ref = _run_attn(q, k, v, gates, n_seq, L, heads, out_f32, one_block + p16, raw=True)
        assert torch.equal(two.view(torch.int16 if out_f32 == 0 else torch.int32), ref.view(torch.int16 if out_f32 == 0 else torch.int32))


@pytest.mark.parametrize("p16", [0, 8])
@pytest.mark.parametrize("out_f32", [0, 1])
@pytest.mark.parametrize("L", [1500, 200])
def test_overflowing_query_in_the_lone_block_of_a_half_empty_wave(L, out_f32, p16):
    """Block 46 of 47 (6 of 7) is the only block of its wave; one of its queries overflows the fast pass and goes through the
    overflow map to the fix-up launch like everywhere else."""
    n_seq, heads = 2, 2
    SH = n_seq * heads
    q, k, v, gates = _attn_inputs(n_seq, L, heads, seed=80)
    nblk = (L + 31) // 32
    assert nblk % 2 == 1
    over = (nblk - 1) * 32 + 5                 # a query of the last block
    q[SH - 1, over] = 0.0
    q[SH - 1, over, 1] = 25.0
    k[SH - 1, L - 40] = 0.0                    # ... scores this key at 600: far beyond the fast pass's headroom
    k[SH - 1, L - 40, 1] = 24.0
    two = _run_attn(q, k, v, gates, n_seq, L, heads, out_f32, 5 + p16, raw=True)
    assert torch.isfinite(two.float()).all()
    for one_block in (1, 2):
        ref = _run_attn(q, k, v, gates, n_seq, L, heads, out_f32, one_block + p16, raw=True)
        assert torch.equal(two.view(torch.int16 if out_f32 == 0 else torch.int32), ref.view(torch.int16 if out_f32 == 0 else torch.int32))
    # the overflowing query's row is the softmax's (nearly all weight on the one key), not a fast-pass inf / NaN
    rows = two.double() if out_f32 == 1 else from_hl32(two)
    row = rows[(n_seq - 1) * L + over, (heads - 1) * 32:]
    want = v[SH - 1, L - 40] * gates[SH - 1, over]
    assert float((row - want).abs().max()) < 1e-3 * float(want.abs().max())


def _qkv(n_seq, L, heads, cfg):
    from beat_this_amd import _lib as Lb
    from beat_this_amd.tables import rope_table

    D = heads * 32
    M = n_seq * L
    x = _mk((M, D), 10, 1.5).float()
    Wqkv = _mk((3 * D, D), 11, 1.6 / D ** 0.5)
    Wg, bg = _mk((heads, D), 12, 0.3), _mk((heads,), 13, 0.3)
    W = pad_rows(torch.cat([Wqkv, Wg]).float(), 256)
    freqs = 10000.0 ** (-torch.arange(0, 32, 2).float() / 32)
    rope = torch.from_numpy(rope_table(freqs)).to(dev())
    nbp = Lb.lib().bt_attn_frag_blocks(L)
    SH = n_seq * heads
    qf = torch.full((SH, nbp, 2, 1024), float("nan"), dtype=torch.float16, device=dev())
    kf, vf = qf.clone(), qf.clone()
    gh = torch.full((SH, nbp * 32), float("nan"), dtype=torch.float32, device=dev())
    st = _status()
    _call(0, cfg, A=to_hl32(x).to(dev()), lda=D, M=M, K=D, W=to_hl32(W).to(dev()), N=3 * D + heads, epi=2,
          ssq_in=_ssq_parts(x).to(dev()), ssq_parts=D // 64, n_seq=n_seq, L=L, nbp=nbp, heads=heads, rope=rope, qf=qf, kf=kf, vf=vf,
          gates=gh, b_gates=bg.float().to(dev()), status=st)
    assert int(st.item()) == 0
    return [t.cpu() for t in (qf, kf, vf, gh)]


# (2, 1500, 16): the main layers (N = 1552: 16 gate columns); heads = 8, 4: transformer_dim 256 and 128 of the ablation models
# (8 and 4 gate columns); 32: a full 32-column block; ragged and single-token sequences
@pytest.mark.parametrize("n_seq,L,heads", [(2, 1500, 16), (16, 1500, 16), (2, 1500, 8), (3, 77, 4), (1, 1, 4), (5, 130, 8), (2, 200, 32)])
def test_qkv_gate_columns_on_the_narrow_tile_agree_bit_for_bit(n_seq, L, heads):
    narrow = _qkv(n_seq, L, heads, 1)
    generic = _qkv(n_seq, L, heads, 3)
    for name, a, b in zip(("q", "k", "v", "gates"), narrow, generic):
        ia, ib = (a.view(torch.int16), b.view(torch.int16)) if a.dtype == torch.float16 else (a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(ia, ib), name
    # ... and what agrees is a gate, not a pattern both tiles left alone.  (The largest may BE 1: the gate logits here have a standard
    # deviation of 0.3 sqrt(D), 6.8 at D = 512, and an fp32 sigmoid is exactly 1 from 16.7 on -- 1 + e^-z rounds to 1.  The smallest,
    # 1 / (1 + e^37), is far inside the fp32 range.)
    g = narrow[3][:, :L]
    assert torch.isfinite(g).all() and float(g.min()) > 0.0 and float(g.max()) <= 1.0
    assert float(g.std()) > 0.1


@pytest.mark.parametrize("B,T", [(2, 1500), (3, 1012), (16, 1500)])
def test_forward_does_not_read_what_the_skipped_stores_used_to_write(B, T):
    """BT_PREC_F32X3, final0, stages 0..2: the whole workspace -- front_x of blocks 1 and 2, ws.xmb and ws.ssq[0] among it -- holds
    0xFF bytes (NaN in fp32 and fp16) or 0x7B bytes (large finite values) before the call; what the forward does not write stays
    that way, so a read of it would reach the logits or the range flag."""
    m, _, _ = _model("final0")
    eng = m.engine()
    x = torch.stack([_chunk(T, i) for i in range(B)])
    clean = _forward(eng, 3, 0, 2, x, 0x00)
    assert int(clean["range_flag"][0]) == 0
    assert torch.isfinite(clean["beat"]).all() and torch.isfinite(clean["downbeat"]).all()
    for pattern in POISONS:
        got = _forward(eng, 3, 0, 2, x, pattern)
        for k in ("beat", "downbeat"):
            assert _same(got[k], clean[k]), f"{k} differs under fill 0x{pattern:02X}"
        assert int(got["range_flag"][0]) == 0
    # a forward that stops in front of the head keeps the stores (its caller may look at the buffers): clean and poisoned agree too
    mid = _forward(eng, 3, 0, 1, x, 0x00)["out"]
    assert _same(_forward(eng, 3, 0, 1, x, 0xFF)["out"], mid) and torch.isfinite(mid).all()
