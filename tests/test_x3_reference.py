"""The "32-high" training precision without a GPU: the split of an fp32 value into two bfloat16 halves, the
contract twin of tests/x3_reference.py held against the fp64 truth and against bfloat16 autocast on every case the GPU tests
(tests/test_gpu_train_formats.py) run -- e_x3 <= e_ref_bf16 / 64 -- and the setting on every surface that takes it.
"""
import copy
import pickle

import numpy as np
import pytest
import torch

import route_cases as RC
import x3_reference as X3
from beat_this_amd import _lib as L
from beat_this_amd import train
from beat_this_amd.model import BeatThis
from beat_this_amd.model.pl_module import PLBeatThis
from beat_this_amd.model.settings import DIFFERENTIABLE as DIFF, Route, TrainSettings, decide

SMALL = dict(transformer_dim=64, n_layers=2, ff_mult=2)
HIGH = "32-high"


# ---- 1. the split -------------------------------------------------------------------------------------------------------------------
def test_the_halves_keep_seventeen_bits_of_a_normal_value():
    bits = np.random.default_rng(25).integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    a = torch.from_numpy(bits.view(np.float32).copy())
    a = a[torch.isfinite(a) & (a.abs() >= 2.0 ** -126) & (a.abs() < 3.3e38)]   # (normal, and hi stays finite)
    assert a.numel() > 900000
    hi, lo = X3.split(a)
    left = (a.double() - hi.double() - lo.double()).abs()
    # lo is at most 2^-9 |a| and keeps 2^-9 of itself -- while it is a normal bfloat16.  Below |a| = 2^-117 it can fall among
    # bfloat16's subnormals (spacing 2^-133): there the halves keep a to 2^-134 absolutely, which is all the format has.
    big = a.abs() >= 2.0 ** -117
    assert int(big.sum()) > 850000 and int((~big).sum()) > 10000
    assert bool((left[big] <= 2.0 ** -17 * a[big].double().abs()).all()), float((left[big] / a[big].double().abs()).max())
    assert bool((left[~big] <= 2.0 ** -134).all()), float(left[~big].max())
    assert bool((hi.to(torch.bfloat16).float() == hi).all() and (lo.to(torch.bfloat16).float() == lo).all())
    # the subtraction is exact in fp32: in fp64 the same halves come out
    lo64 = (a.double() - hi.double()).to(torch.float32)
    assert torch.equal(lo64, a - hi)


def test_sixteen_bit_integers_split_exactly():
    a = torch.arange(-65536, 65537, dtype=torch.float32)
    hi, lo = X3.split(a)
    assert torch.equal(hi + lo, a) and bool((lo != 0).any())


def test_no_lo_half_where_hi_is_not_finite():
    inf, nan = float("inf"), float("nan")
    hi, lo = X3.split(torch.tensor([inf, -inf, nan, 3.4e38, -3.4e38, 3.0e38]))
    assert hi[:2].tolist() == [inf, -inf] and torch.isnan(hi[2]) and hi[3:5].tolist() == [inf, -inf] and torch.isfinite(hi[5])
    assert lo[:5].tolist() == [0.0] * 5 and lo[5] != 0
    assert torch.tensor(3.4e38) - torch.tensor(3.4e38).to(torch.bfloat16).float() == -inf   # (what the rule is there for)
    # an overflow stays an overflow and a NaN stays in its own row, against a B whose halves are all positive (an inf still meets
    # NaN where the other operand's lo half is zero or of the other sign: inf times that half)
    e = 2.0 ** -10
    a = torch.tensor([[inf, 1.0], [3.4e38, 1.0], [nan, 1.0], [2.0, 3.0]])
    b = torch.tensor([[1.0 + e, 0.5 + e], [2.0 + e, 4.0 + e]])
    assert bool((X3.split(b)[1] > 0).all())
    got = X3.mm(a, b)
    assert got[:2].tolist() == [[inf, inf], [inf, inf]] and bool(torch.isnan(got[2]).all())
    assert got[3].tolist() == [8.0 + 5 * e, 13.0 + 5 * e]


def test_the_product_drops_the_lo_lo_term_and_nothing_else():
    gen = torch.Generator().manual_seed(3)
    a = torch.randint(-4095, 4096, (33, 70), generator=gen).float()
    b = torch.randint(-4095, 4096, (70, 17), generator=gen).float()
    (ah, al), (bh, bl) = X3.split(a), X3.split(b)
    want = a.double() @ b.double() - al.double() @ bl.double()
    assert bool((al != 0).any() and (bl != 0).any()) and float(want.abs().max()) < 2.0 ** 40
    got = X3.mm(a.double(), b.double())
    assert torch.equal(got, want)
    with X3.high():
        assert X3.REF._MatMul is X3._MatMul and X3.REF._AttnCore is X3._AttnCore and X3.REF._Conv is X3._Conv
    assert X3.REF._MatMul is not X3._MatMul and X3.REF._AttnCore is not X3._AttnCore and X3.REF._Conv is not X3._Conv


# ---- 2. the twin sits where the issue's table says --------------------------------------------------------------------------------------
def check(name, case):
    """the twin within e_ref_bf16 / 64 of the fp64 truth (CAP_EXEMPT: printed alone), both figures finite and non-zero"""
    e_x3, e_bf = case["e"], case["e_ref_bf16"]
    print(f"x3 twin {name}: e_x3 = {e_x3:.3e}, e_ref_bf16 = {e_bf:.3e}, e_ref_bf16 / e_x3 = {e_bf / e_x3:.0f}")
    assert 0 < e_x3 < float("inf") and 0 < e_bf < float("inf")
    assert case["name"] == name
    if name not in X3.CAP_EXEMPT:
        assert e_x3 <= e_bf / X3.CAP, f"{name}: e_x3 = {e_x3:.3e} above e_ref_bf16 / 64 = {e_bf / X3.CAP:.3e}"
    return e_bf / e_x3


CASES = X3.gpu_cases()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_the_twin_is_64_times_inside_bfloat16(name):
    check(name, dict(CASES)[name]())


TABLE = {("attn", 64): (3.6e-5, 2.4e-2), ("attn", 192): (1.9e-5, 1.5e-2), ("ff", 64): (9.2e-6, 5.9e-3), ("ff", 192): (7.1e-6, 4.5e-3)}


def test_the_four_unit_cases_sit_where_the_table_of_section_25_says():
    """attention and feed-forward units of width 64 and 192 at B = 2, T = 40: (e_x3, e_ref_bf16) to the table's two digits, which
    is 630 to 790 times inside bfloat16 in two digits -- the cap of 64 with a further factor 9.8 to 12"""
    for (kind, D), (e_x3, e_bf) in TABLE.items():
        case = X3.unit_case(kind, D, 2, 40)
        ratio = check(f"{kind} D={D} B=2 T=40", case)
        assert abs(case["e"] / e_x3 - 1) < 0.03 and abs(case["e_ref_bf16"] / e_bf - 1) < 0.03, (kind, D, case["e"], case["e_ref_bf16"])
        assert 625 <= ratio < 795, (kind, D, ratio)


# ---- 3. settings and surfaces -------------------------------------------------------------------------------------------------------
def test_the_setters_take_the_value_and_no_loss_scale_follows():
    m = BeatThis(**SMALL)
    assert m.set_train_precision(HIGH) is m and m.set_frontend_precision(HIGH) is m
    assert (m.train_precision, m.frontend_precision, m.train_operand, m.frontend_operand) == (HIGH, HIGH, "fp16", "fp16")
    assert not m.train_settings.needs_loss_scale() and not m.train_settings.violations()
    assert not TrainSettings(train_precision=HIGH, frontend_precision="16-mixed", frontend_operand="bf16").needs_loss_scale()
    assert TrainSettings(train_precision=HIGH, frontend_precision="16-mixed").needs_loss_scale()   # (the other part on fp16)
    m.set_train_precision("32-true").set_frontend_precision("32-true")
    assert (m.train_precision, m.frontend_precision) == ("32-true", "32-true")
    assert L.OPERAND_BF16X3 == 3 and L.OPERANDS == {"fp16": 0, "bf16": 1}


@pytest.mark.parametrize("which", ["train", "frontend"])
def test_the_operand_beside_it_follows_the_rule_of_32_true(which):
    m = BeatThis(**SMALL)
    setter, operand = getattr(m, f"set_{which}_precision"), lambda: getattr(m, which + "_operand")
    setter(HIGH, operand=None)
    setter(HIGH, operand="fp16")
    assert operand() == "fp16"
    with pytest.raises(ValueError, match=rf"operand='bf16' needs set_{which}_precision\('16-mixed'\)"):
        setter(HIGH, operand="bf16")
    with pytest.raises(ValueError, match=f"{which} operand must be 'fp16' or 'bf16'"):
        setter(HIGH, operand="bf16x3")
    assert getattr(m, which + "_precision") == HIGH and operand() == "fp16"
    setter("16-mixed", "bf16")
    setter(HIGH)                 # the precision does not stay "16-mixed": the operand is fp16 again
    assert operand() == "fp16"
    setter("16-mixed")
    assert operand() == "fp16"


def test_the_violations_and_what_they_are_called(capsys):
    for bad in ("bf16-mixed", "16", "32-High", "high", "32", None):
        with pytest.raises(ValueError, match="train precision"):
            BeatThis(**SMALL).set_train_precision(bad)
        with pytest.raises(ValueError, match="frontend precision"):
            BeatThis(**SMALL).set_frontend_precision(bad)
    s = TrainSettings(train_precision=HIGH, train_operand="bf16", frontend_precision=HIGH)
    for level in ("model", "recipe"):
        found = {(v.what, v.needs) for v in s.violations(level)}
        assert ("train_operand", "train_mixed") in found and not any(w.startswith("frontend_operand") for w, _ in found), (level, found)
    assert ("frontend_precision", "train_frontend") in {(v.what, v.needs) for v in s.violations("recipe")}
    with pytest.raises(ValueError, match="16-mixed"):
        PLBeatThis(**SMALL, precision=HIGH, mixed_operand="bf16")
    base = ["--data-dir", "/nowhere/at/all", "--output", "o"]
    for flags, text in ((["--precision", HIGH, "--mixed-operand", "bf16"], "--mixed-operand needs --precision 16-mixed"),
                        (["--frontend-precision", HIGH], "--frontend-precision needs --train-frontend"),
                        (["--precision", "32-higher"], "invalid choice"), (["--precision", "bf16-mixed"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            train.main(base + flags)
        assert e.value.code == 2 and text in capsys.readouterr().err, flags


def test_the_route_is_a_mixed_call_on_the_split_operand():
    s = TrainSettings(frontend_trainable=True, train_precision=HIGH, train_operand="fp16", frontend_precision="16-mixed", frontend_operand="bf16")
    assert decide(s, "transformer", True, False, False, True) == Route(DIFF, mixed=True, operand="bf16x3")
    assert decide(s, "transformer", True, False, False, True).mixed_operand == "bf16x3"
    assert decide(s, "frontend", True, False, False, True) == Route(DIFF, mixed=True, operand="bf16")
    s = TrainSettings(frontend_trainable=True, frontend_precision=HIGH)
    assert decide(s, "frontend", True, False, False, True) == Route(DIFF, mixed=True, operand="bf16x3")
    assert decide(s, "transformer", True, False, False, True) == Route(DIFF)
    assert decide(s, "heads", True, False, False, True) == Route(DIFF)
    assert decide(s, "frontend", False) == Route("engine")
    m = BeatThis(**SMALL).set_frontend_trainable().set_frontend_precision(HIGH)
    x = torch.zeros(2, 8, 128)
    assert m._route("frontend", m.frontend, x) == Route(DIFF, mixed=True, operand="bf16x3")
    from beat_this_amd.model import backward as bw

    assert bw._operand("bf16x3") == 3 and bw._operand("bf16") == 1 and bw._operand(True) == 0 and bw._operand(False) == 0
    a = bw._front_args(2, 3, 32, 32, mixed="bf16x3")
    assert (a.mixed, a.operand) == (1, 3)


def test_the_setting_travels_with_the_model():
    m = BeatThis(**SMALL).set_train_precision(HIGH).set_frontend_trainable().set_frontend_precision(HIGH)
    for twin in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        assert (twin.train_precision, twin.frontend_precision) == (HIGH, HIGH) and twin.train_settings == m.train_settings
    assert "train_precision" not in m.state_dict() and not any("precision" in k for k in m.state_dict())


def test_the_module_and_the_parser():
    plain = PLBeatThis(**SMALL)
    pl = PLBeatThis(**SMALL, precision=HIGH, train_frontend=True, frontend_precision=HIGH)
    assert (pl.model.train_precision, pl.model.frontend_precision) == (HIGH, HIGH) and not pl.model.train_settings.needs_loss_scale()
    assert pl.hyper_parameters == plain.hyper_parameters
    p = train.get_parser()
    a = p.parse_args(["--data-dir", "d", "--output", "o", "--precision", HIGH, "--train-frontend", "--frontend-precision", HIGH])
    assert (a.precision, a.frontend_precision, a.mixed_operand, a.frontend_mixed_operand) == (HIGH, HIGH, None, None)
    assert p.parse_args(["--data-dir", "d", "--output", "o"]).precision == "32-true"


class NoData:
    def setup(self, stage):
        pass

    def train_dataloader(self):
        return []


def test_fit_takes_it_before_it_builds_anything():
    """on the CPU fit() ends where it builds the optimiser, after every setting was applied"""
    pl = PLBeatThis(**SMALL)
    with pytest.raises(RuntimeError, match="ROCm GPUs only"):
        train.fit(pl, NoData(), 0, log=lambda s: None, precision=HIGH, train_frontend=True, frontend_precision=HIGH)
    m = pl.model
    assert (m.train_precision, m.frontend_precision) == (HIGH, HIGH) and not m.train_settings.needs_loss_scale()
    with pytest.raises(ValueError, match="16-mixed"):
        train.fit(pl, NoData(), 0, log=lambda s: None, precision=HIGH, mixed_operand="bf16")
