"""The inference attention kernels on the MI355X against tests/attn_exact_reference.py: inputs whose softmax is exact in every
arithmetic the kernels run in, through every entry the forward can take -- bt_attention (csrc/attn.hip) in fp32 and in the half
type, bt_attention_frag's half kernels, the three-term x3 kernels and the P16 ones with the by-launch-size choices, in half, fp32,
hl32 and hl8 rows, with one selection case per entry through the time-direction row map.

selection and graded: the same bits as the expectation rounded once to the output format, but for the sign of a zero.  Their row
sums are powers of two, on which the hardware reciprocal is exact (tests/test_gpu_train_exact.py relies on the same).
uniform: the row sum is L times a power of two, so the kernel's acc x (gate x 1 / l) is not exact:
  half-type rows (and the hi halves of hl8 rows)  bit for bit: c_d is representable and an fp32 error of 2 ulp rounds back to it;
  fp32 rows   within 4 ulp of fp32: one reciprocal (1 ulp) and one product (half an ulp, twice) account for 2, the factor of two on
              top is margin for the gate's product;
  hl32 rows   within 2^-20 relative: a 22-bit representation plus the same 2 ulp.
Both bounds are derived, not measured, and sit three decades under the 1 / (L + 1) >= 4e-4 of a miscounted key.

A failure prints describe(): the first differing (sequence, head, query, column), what that query selects, and whether it was
expected in the fast pass or in the SAFE re-run / the fix-up launch."""
import numpy as np
import pytest
import torch

import attn_exact_reference as R
from gpu_util import HALF, dev, frag_qk, frag_v, from_hl32, hl8_parts, report, run_attn, run_attn_frag, run_attn_x3

pytestmark = pytest.mark.gpu

FAMILIES = ("selection", "graded", "uniform")
ROWMAP = dict(o_div=2, o_inner=1, o_tok=2)   # sequences (b, f) of B = 1, F = 2 scattered to (b, t, f) rows; o_outer = L F


def _is_f16():
    from beat_this_amd import _lib as Lb

    return not Lb.lib().bt_half_is_bf16()


def _half():
    return "f16" if _is_f16() else "bf16"


def _cases(family):
    """[(case, row map or None)]: the family's cases, the row-map pass of R.ROWMAP behind the plain one"""
    out = []
    for c in (c for c in R.all_cases() if c.family == family):
        out.append((c, None))
        if family == "selection" and (c.S, c.L, c.H) == R.ROWMAP:
            out.append((c, dict(ROWMAP, o_outer=c.L * 2)))
    return out


def _unmap(case, rows, omap):
    """the rows a launch wrote [S L, w] -> [S, H, L, 32]"""
    rows = np.asarray(rows)
    if omap is not None:   # (b, t, f) rows of B = 1 -> (f, t)
        rows = rows.reshape(case.L, case.S, -1).transpose(1, 0, 2).reshape(case.S * case.L, -1)
    return case.unrows(rows)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _check(entry, family, fmt, half, rule, launch):
    """launch(case, omap) -> [S, H, L, 32] float64 as stored; asserts every case of the family and reports the counts"""
    msgs, differing, n, worst = [], 0, 0, 0.0
    for case, omap in _cases(family):
        got = launch(case, omap)
        want = R.round_out(case.want, fmt, half)
        tol = 0.0
        if family == "uniform" and fmt == "f32":
            tol = 4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        elif family == "uniform" and fmt == "hl32":
            tol = 2.0 ** -20 * np.abs(want)
        name = f"{entry}, {fmt} rows" + (", through the row map" if omap else "")
        msg = case.describe(name, got, want, rule, tol)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs((got + 0.0) - (want + 0.0))
            differing += int((~(err <= tol)).sum())
            if np.ndim(tol):   # the share of the derived bound that is used (uniform, fp32 and hl32 rows)
                worst = max(worst, float(np.nanmax(err / tol)))
        n += 1
        if msg:
            msgs.append(msg)
    report("attn_exact", entry=entry, family=family, fmt=fmt, cases=n, differing=differing, worst_share_of_bound=worst)
    assert not msgs, "\n".join(msgs)


# ---- bt_attention (csrc/attn.hip): row-major q | k | v, online softmax over tiles of 64 keys ------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("prec", [0, 1])   # BT_PREC_F32, BT_PREC_HALF
def test_attention_flash_exact(prec, family):
    dt = torch.float32 if prec == 0 else HALF()

    def launch(case, omap):
        qkv = _t(np.concatenate([case.rows(case.q), case.rows(case.k), case.rows(case.v)], axis=1)).to(dt).to(dev())
        gates = _t(case.rows(case.gates[..., None])).float().to(dev())           # [S L, H]
        out = torch.full((case.S * case.L, case.H * 32), float("nan"), dtype=dt, device=dev())
        run_attn(prec, qkv, gates, out, case.S, case.L, case.H, **(omap or {}))
        return _unmap(case, out.double().cpu().numpy(), omap)
    _check(f"bt_attention prec {prec}", family, "f32" if prec == 0 else "half", _half(), None, launch)


# ---- bt_attention_frag, half kernels (csrc/attn2.hip) ---------------------------------------------------------------------------------
def _frag_operands(case, to_q, to_v):
    from beat_this_amd import _lib as Lb

    nbp = Lb.lib().bt_attn_frag_blocks(case.L)
    nblk = (case.L + 31) // 32
    q, k, v = (_t(case.pairs(x)).float() for x in (case.q, case.k, case.v))
    qf, kf, vf = to_q(q, nbp), to_q(k, nbp), to_v(v, nbp)
    kf[:, nblk:] = float("nan")   # padding blocks beyond ceil(L / 32) must never be consumed; the padding slots of the last
    vf[:, nblk:] = float("nan")   # block are zeros, as the QKV producers write them
    gh = torch.zeros((case.S * case.H, nbp * 32), dtype=torch.float32)
    gh[:, :case.L] = _t(case.pairs(case.gates)).float()
    return nbp, qf, kf, vf, gh


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("variant", [-1, -2])
def test_attention_frag_half_exact(variant, family):
    if variant == -2 and not _is_f16():
        pytest.skip("the two-query-block kernel is an fp16 kernel")

    def launch(case, omap):
        nbp, qf, kf, vf, gh = _frag_operands(case, frag_qk, frag_v)
        out = torch.full((case.S * case.L, case.H * 32), float("nan"), dtype=HALF(), device=dev())
        run_attn_frag(qf.to(dev()), kf.to(dev()), vf.to(dev()), gh.to(dev()), out, case.S, case.L, case.H, nbp, variant=variant, **(omap or {}))
        return _unmap(case, out.double().cpu().numpy(), omap)
    _check(f"bt_attention_frag half variant {variant}", family, "half", _half(), "half", launch)


# ---- bt_attention_frag, x3 operands: three-term kernels 1, 2, 5 (4 by launch size), P16 kernels 9, 10, 13 (12 by launch size) -----------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("out_f32", [0, 1, 2])
@pytest.mark.parametrize("variant", [1, 2, 5, 4, 9, 10, 13, 12])
def test_attention_frag_x3_exact(variant, out_f32, family):
    if not _is_f16():
        pytest.skip("the x3 kernels are fp16 kernels")
    fmt = ("hl32", "f32", "hi")[out_f32]

    def launch(case, omap):
        q, k, v = (_t(case.pairs(x)) for x in (case.q, case.k, case.v))
        raw = run_attn_x3(q, k, v, _t(case.pairs(case.gates)), case.S, case.L, case.H, out_f32, variant, raw=True, **(omap or {}))
        rows = raw.double() if out_f32 == 1 else from_hl32(raw) if out_f32 == 0 else hl8_parts(raw, act=True)[0]
        return _unmap(case, rows.numpy(), omap)
    _check(f"bt_attention_frag x3 variant {variant}", family, fmt, "f16", "x3", launch)
