"""The training losses' host twin (bt_bce_loss_host, csrc/loss.hip) against the reference's own loss.py recorded on CPU torch
(tests/golden/loss_reference.npz, tools/make_loss_golden.py) and against the numpy restatement tests/loss_reference.py; the
Python modules' argument checks, losses_from_hparams, and the evaluator's framewise targets."""
import json
import os

import numpy as np
import pytest
import torch

import loss_reference as R
from conftest import GOLDEN

KINDS = {"MaskedBCELoss": 0, "ShiftTolerantBCELoss": 1, "SplittedShiftTolerantBCELoss": 2}
ORACLE = {0: "masked", 1: "shift_tolerant", 2: "splitted"}


def golden_cases():
    z = np.load(os.path.join(GOLDEN, "loss_reference.npz"))
    meta = json.loads(str(z["meta"]))
    out = []
    for i, c in enumerate(meta):
        m = z[f"c{i}_m"] if f"c{i}_m" in z.files else None
        out.append(dict(c, i=i, x=z[f"c{i}_x"], y=z[f"c{i}_y"], m=m, grad=z[f"c{i}_grad"], value=float(z[f"c{i}_value"])))
    return out


CASES = golden_cases()


def host(c):
    from beat_this_amd.loss import loss_host

    x, T = c["x"], c["x"].shape[-1]
    off = np.arange(x.size // T + 1, dtype=np.int64) * T
    m = None if c["m"] is None else c["m"].reshape(-1)
    r = loss_host(KINDS[c["cls"]], c["tol"], c["pw"], x.reshape(-1), c["y"].reshape(-1), m, off)
    r["mean_grad"] = (r["grad"] / r["row_count"].sum()).reshape(x.shape)
    return r


def check_against_golden(c, value, grad, gtol=1e-6):
    """value within 1e-5 relative (fp16 cases: fp16 tolerance, the reference computes them in half), gradient within 1e-6 of
    max |grad|, NaNs in the same places, and the same set of frames that receive gradient (fp16: the reference's half
    arithmetic flushes some tiny ones to zero, so only frames above 1e-3 of max |grad| must agree)"""
    half = c["dtype"] != "float32"
    want, g = c["value"], c["grad"].astype(np.float64)
    if np.isnan(want):
        assert np.isnan(value), (c["i"], value)
    else:
        assert value == pytest.approx(want, rel=2e-3 if half else 1e-5, abs=1e-7), (c["i"], c["note"], value, want)
    assert np.array_equal(np.isnan(grad), np.isnan(g)), c["i"]
    fin = np.isfinite(g) & np.isfinite(grad)
    scale = max(np.abs(g[fin]).max(), 1e-30) if fin.any() else 1.0
    err = np.abs(grad[fin] - g[fin]).max() / scale if fin.any() else 0.0
    assert err <= (2e-3 if half else gtol), (c["i"], c["note"], err)
    nz_ref = (g != 0) | np.isnan(g)
    nz = (grad != 0) | np.isnan(grad)
    if half:
        big = np.abs(np.nan_to_num(grad)) > 1e-3 * scale
        assert not (nz_ref & ~nz).any() and not (nz & ~nz_ref & big).any(), c["i"]
    else:
        assert np.array_equal(nz, nz_ref), (c["i"], c["note"], np.flatnonzero(nz != nz_ref)[:10])


@pytest.mark.parametrize("c", CASES, ids=[f"{c['i']}-{c['cls']}-tol{c['tol']}-{c['mask']}-{c['note'] or c['dtype']}" for c in CASES])
def test_host_matches_reference_golden(c):
    r = host(c)
    check_against_golden(c, r["loss"], r["mean_grad"])
    # terms: zero outside the output frames, and their sum is the row sum
    h = 0 if c["cls"] == "MaskedBCELoss" else 2 * c["tol"]
    T = c["x"].shape[-1]
    terms = r["terms"].reshape(-1, T)
    assert (terms[:, :h] == 0).all() and (terms[:, T - h:] == 0).all()
    assert (r["row_count"] == T - 2 * h).all()


def test_golden_covers_the_issue():
    seen = {(c["cls"], c["tol"], c["pw"], c["mask"], c["soft"]) for c in CASES}
    for cls in KINDS:
        for tol in ((0,) if cls == "MaskedBCELoss" else (0, 1, 3, 5)):
            for pw in (1.0, 2.7):
                for mk in (("bool", "float") if cls.startswith("Splitted") else ("none", "bool", "float")):
                    for soft in (False, True):
                        assert (cls, tol, pw, mk, soft) in seen
    notes = {c["note"] for c in CASES}
    assert {"T1500", "zeros", "plateau", "nan", "inf", "fp16", "NCT"} <= notes
    assert any(c["x"].shape[-1] == 1 + 4 * c["tol"] and c["tol"] == 5 for c in CASES)


def test_oracle_matches_reference_golden():
    """the numpy restatement itself against the reference (so the fuzz below compares with something pinned); fp64 against
    the reference's fp32, so the gradients agree to 1e-5 of max |grad| here"""
    for c in CASES:
        v, g = R.loss(ORACLE[KINDS[c["cls"]]], c["tol"], c["pw"], c["x"].astype(np.float64), c["y"].astype(np.float64), c["m"])
        check_against_golden(c, v, g, gtol=1e-5)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_host_matches_oracle_fuzz(kind):
    """~500 rows of random lengths in one ragged call per kind: each row's sum and gradient against the fp64 oracle"""
    from beat_this_amd.loss import loss_host

    tol = 3
    rows = R.fuzz_rows(seed=40 + kind, n_rows=170, tol=tol)
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([x.size for x, _, _ in rows])
    x = np.concatenate([r[0] for r in rows])
    y = np.concatenate([r[1] for r in rows])
    m = np.concatenate([r[2] for r in rows])
    res = loss_host(kind, tol, 2.7, x, y, m, off)
    for i, (xr, yr, mr) in enumerate(rows):
        s, n, g = R.row_terms(ORACLE[kind], tol, 2.7, xr, yr, mr)
        assert res["row_count"][i] == n
        assert res["row_sum"][i] == pytest.approx(s, rel=1e-5, abs=1e-5), i
        got = res["grad"][off[i]:off[i + 1]]
        np.testing.assert_allclose(got, g, rtol=0, atol=1e-5 * max(np.abs(g).max(), 1e-30))
        # the same frames receive gradient, except where fp32 rounds a term to exactly 0 that fp64 keeps (sigmoid(21) == 1)
        assert (g[got != 0] != 0).all() and (got[np.abs(g) > 1e-6 * np.abs(g).max()] != 0).all(), i
    assert res["loss"] == pytest.approx(res["row_sum"].sum() / res["row_count"].sum(), rel=1e-14)


def test_soft_targets_split_differs_binary_equal():
    from beat_this_amd.loss import loss_host

    rows = R.fuzz_rows(seed=7, n_rows=1, soft_frac=0.0, tol=3, max_len=400)
    x, y, m = rows[0]
    st = loss_host(1, 3, 2.7, x, y, m)
    sp = loss_host(2, 3, 2.7, x, y, m)
    assert sp["loss"] == pytest.approx(st["loss"], rel=1e-6)
    np.testing.assert_allclose(sp["grad"], st["grad"], rtol=0, atol=1e-6 * np.abs(st["grad"]).max())
    ys = (y * 0.8 + 0.1).astype(np.float32)
    st, sp = loss_host(1, 3, 2.7, x, ys, m), loss_host(2, 3, 2.7, x, ys, m)
    assert abs(sp["loss"] - st["loss"]) > 1e-3 * abs(st["loss"])
    for kind, r in ((1, st), (2, sp)):
        v, _ = R.loss(ORACLE[kind], 3, 2.7, x, ys, m)
        assert r["loss"] == pytest.approx(v, rel=1e-5)


def test_tolerance_zero_equals_masked():
    from beat_this_amd.loss import loss_host

    x, y, m = R.fuzz_rows(seed=8, n_rows=1, tol=0, max_len=300)[0]
    mk = loss_host(0, 0, 1.7, x, y, m)
    for kind in (1, 2):
        r = loss_host(kind, 0, 1.7, x, y, m)
        assert r["loss"] == pytest.approx(mk["loss"], rel=1e-6)
        np.testing.assert_allclose(r["grad"], mk["grad"], rtol=1e-6, atol=1e-7)


def test_host_rejects_bad_arguments():
    from beat_this_amd import _lib
    from beat_this_amd.loss import loss_host

    x = np.zeros(12, np.float32)
    with pytest.raises(ValueError, match="row 0 has 12 frames, the loss needs at least 13"):
        loss_host(1, 3, 1.0, x, x)
    loss_host(1, 3, 1.0, np.zeros(13, np.float32), np.zeros(13, np.float32))
    loss_host(0, 3, 1.0, x, x)   # (the masked loss has no minimum)
    with pytest.raises(ValueError, match="tolerance"):
        loss_host(1, 33, 1.0, x, x)
    with pytest.raises(ValueError, match="kind"):
        loss_host(5, 3, 1.0, x, x)
    L = _lib.lib()
    assert L.bt_bce_loss_host(1, 99, 1.0, x.ctypes.data, 0, x.ctypes.data, 0, None, 0, np.array([0, 12]).ctypes.data, 1,
                              None, None, None, None, None) == _lib.BT_ERR_ARG
    assert L.bt_bce_loss_host(7, 1, 1.0, x.ctypes.data, 0, x.ctypes.data, 0, None, 0, np.array([0, 12]).ctypes.data, 1,
                              None, None, None, None, None) == _lib.BT_ERR_ARG
    # the device entry refuses the same before launching anything (no stream or device memory is touched)
    assert L.bt_bce_loss(None, 1, 3, 1.0, None, 1, 0, 1, 0, None, 0, 1, 1, 12, 12, 1, 1 << 20, None, None, None, 0, None,
                         None) == _lib.BT_ERR_ARG
    assert L.bt_bce_loss(None, 1, 40, 1.0, None, 1, 0, 1, 0, None, 0, 1, 1, 200, 200, 1, 1 << 20, None, None, None, 0, None,
                         None) == _lib.BT_ERR_ARG
    assert L.bt_bce_loss(None, 1, 3, 1.0, None, 1, 0, 1, 0, None, 0, 1, 4, 13, 1500, 1, 8, None, None, None, 0, None,
                         None) == _lib.BT_ERR_WORKSPACE
    assert L.bt_bce_loss_workspace_bytes(4, 1500) == 4 * 6 * 8


def test_modules_reject_like_the_reference_and_refuse_cpu():
    from beat_this_amd.model.loss import MaskedBCELoss, ShiftTolerantBCELoss, SplittedShiftTolerantBCELoss

    x = torch.zeros(2, 20)
    for fn in (MaskedBCELoss(), ShiftTolerantBCELoss(), SplittedShiftTolerantBCELoss()):
        with pytest.raises(RuntimeError, match="ROCm GPUs only"):
            fn(x, x, torch.ones(2, 20))
    with pytest.raises(TypeError):
        SplittedShiftTolerantBCELoss()(x, x)   # the mask is required
    with pytest.raises(RuntimeError, match="require grad"):
        ShiftTolerantBCELoss()(x, x.clone().requires_grad_(True))
    st = ShiftTolerantBCELoss(pos_weight=2.5, tolerance=4)
    assert st.tolerance == 4 and float(st.pos_weight) == 2.5 and "pos_weight" not in st.state_dict()
    sp = SplittedShiftTolerantBCELoss(tolerance=2)
    assert sp.spread_preds == 2 and sp.spread_targets == 4
    assert MaskedBCELoss().pos_weight.dtype == torch.get_default_dtype()


def test_losses_from_hparams():
    from beat_this_amd.loss import losses_from_hparams
    from beat_this_amd.model.loss import MaskedBCELoss, ShiftTolerantBCELoss, SplittedShiftTolerantBCELoss

    pw = {"beat": 2.0, "downbeat": 7.5}
    b, d = losses_from_hparams({})
    assert type(b) is type(d) is ShiftTolerantBCELoss and float(b.pos_weight) == float(d.pos_weight) == 1
    b, d = losses_from_hparams({"loss_type": "shift_tolerant_weighted_bce", "pos_weights": pw})
    assert float(b.pos_weight) == 2.0 and float(d.pos_weight) == 7.5 and b.tolerance == 3
    b, d = losses_from_hparams({"loss_type": "weighted_bce", "pos_weights": pw})
    assert type(b) is MaskedBCELoss and float(d.pos_weight) == 7.5
    b, d = losses_from_hparams({"loss_type": "bce", "pos_weights": pw})
    assert type(b) is MaskedBCELoss and float(b.pos_weight) == float(d.pos_weight) == 1
    b, d = losses_from_hparams({"loss_type": "splitted_shift_tolerant_weighted_bce", "pos_weights": pw})
    assert type(b) is SplittedShiftTolerantBCELoss and float(d.pos_weight) == 7.5
    with pytest.raises(ValueError, match="loss_type must be one of 'shift_tolerant_weighted_bce', 'weighted_bce', 'bce'"):
        losses_from_hparams({"loss_type": "focal"})


def test_framewise_targets(tmp_path):
    from beat_this_amd.evaluate import _has_downbeats, framewise_targets

    two = tmp_path / "two.beats"
    two.write_text("0.0\t1\n0.49\t2\n1.01\t3\n1.5\t1\n2.03\t2\n-0.2\t4\n")   # 1.01 s -> frame 50 (rounded), 2.03 -> 101: cut
    beat, down, dm = framewise_targets(two, 100)
    assert beat.dtype == np.float32 and beat.shape == (100,) and dm == 1
    assert list(np.flatnonzero(beat)) == [0, 24, 50, 75] and list(np.flatnonzero(down)) == [0, 75]
    one = tmp_path / "one.beats"
    one.write_text("0.5\n1.0\n")
    beat, down, dm = framewise_targets(one, 60)
    assert list(np.flatnonzero(beat)) == [25, 50] and not down.any() and dm == 0
    _, _, dm = framewise_targets(two, 100, has_downbeats=False)
    assert dm == 0
    (tmp_path / "ds").mkdir()
    assert _has_downbeats(tmp_path, "ds") is None
    (tmp_path / "ds" / "info.json").write_text(json.dumps({"has_downbeats": False}))
    assert _has_downbeats(tmp_path, "ds") is False
    # np.round is half to even, as the reference's .round(): 0.01 s * 50 = 0.5 -> frame 0, 0.03 s -> 1.5 -> 2
    half = tmp_path / "half.beats"
    half.write_text("0.01\t1\n0.03\t2\n")
    beat, down, _ = framewise_targets(half, 10)
    assert list(np.flatnonzero(beat)) == [0, 2] and list(np.flatnonzero(down)) == [0]


def test_reference_import_path_of_the_losses():
    from beat_this_amd import loss as L
    from beat_this_amd.model.loss import MaskedBCELoss, ShiftTolerantBCELoss, SplittedShiftTolerantBCELoss

    assert MaskedBCELoss is L.MaskedBCELoss and ShiftTolerantBCELoss is L.ShiftTolerantBCELoss
    assert SplittedShiftTolerantBCELoss is L.SplittedShiftTolerantBCELoss
