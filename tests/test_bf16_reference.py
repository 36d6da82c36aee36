"""The bfloat16 operand format of the 16-mixed routes without a GPU: the settings on every surface that takes
them, the struct layouts, the parser, and the yardstick of tests/bf16_reference.py held against its own contract twin on every case
the GPU tests (tests/test_gpu_train_formats.py) run -- a finite, non-zero e_ref_bf16 and the twin within the gate.
"""
import pickle

import pytest
import torch

import bf16_reference as BF
import route_cases as RC
from beat_this_amd import _lib as L
from beat_this_amd import train
from beat_this_amd.model import BeatThis
from beat_this_amd.model.pl_module import PLBeatThis
from beat_this_amd.model.settings import DIFFERENTIABLE as DIFF, Route, TrainSettings, decide

SMALL = dict(transformer_dim=64, n_layers=2, ff_mult=2)


# ---- 1. the settings ----------------------------------------------------------------------------------------------------------------
def test_defaults():
    s = TrainSettings()
    assert (s.train_operand, s.frontend_operand) == ("fp16", "fp16") and not s.needs_loss_scale() and not s.violations()
    assert Route(DIFF).operand == "fp16" and Route(DIFF, mixed=True) == Route(DIFF, False, False, True, "fp16")
    assert Route(DIFF).mixed_operand is False and Route(DIFF, mixed=True, operand="bf16").mixed_operand == "bf16"
    m = BeatThis(**SMALL)
    assert (m.train_operand, m.frontend_operand) == ("fp16", "fp16")
    for name in ("train_operand", "frontend_operand"):
        with pytest.raises(AttributeError):
            setattr(m, name, "bf16")
    m.set_train_precision("16-mixed").set_frontend_precision("16-mixed")     # the calls of before: fp16 operands
    assert (m.train_operand, m.frontend_operand) == ("fp16", "fp16") and m.train_settings.needs_loss_scale()


@pytest.mark.parametrize("which", ["train", "frontend"])
def test_the_operand_is_kept_while_the_part_stays_mixed_and_reset_otherwise(which):
    m = BeatThis(**SMALL)
    setter, operand = getattr(m, f"set_{which}_precision"), lambda: getattr(m, which + "_operand")
    other = lambda: getattr(m, ("frontend" if which == "train" else "train") + "_operand")
    assert setter("16-mixed", operand="bf16") is m and operand() == "bf16" and other() == "fp16"
    assert getattr(m, which + "_precision") == "16-mixed"
    setter("16-mixed")                       # None keeps it while the value stays "16-mixed"
    assert operand() == "bf16"
    setter("16-mixed", "fp16")
    assert operand() == "fp16"
    setter("16-mixed", operand="bf16")
    setter("32-true")                        # ... and resets it otherwise
    assert operand() == "fp16"
    setter("16-mixed")                       # coming from "32-true" the value does not STAY "16-mixed": fp16
    assert operand() == "fp16"
    setter("16-mixed", "bf16")
    assert not m.train_settings.needs_loss_scale()
    m.set_train_precision("16-mixed") if which == "frontend" else m.set_frontend_precision("16-mixed")
    assert m.train_settings.needs_loss_scale()   # (the other part on fp16 operands)


def test_the_violations_and_what_they_are_called(capsys):
    for bad in ("bf16-mixed", "16", None):   # the string of Lightning stays refused: bfloat16 is an operand format of "16-mixed"
        with pytest.raises(ValueError, match="train precision"):
            BeatThis(**SMALL).set_train_precision(bad)
        with pytest.raises(ValueError, match="frontend precision"):
            BeatThis(**SMALL).set_frontend_precision(bad)
        with pytest.raises(ValueError, match="train precision"):
            BeatThis(**SMALL).set_train_precision(bad, operand="bf16")
    for which in ("train", "frontend"):
        m = BeatThis(**SMALL)
        setter = getattr(m, f"set_{which}_precision")
        for bad in ("bf15", "", "BF16", 1):
            with pytest.raises(ValueError, match=f"{which} operand must be 'fp16' or 'bf16'"):
                setter("16-mixed", operand=bad)
        with pytest.raises(ValueError, match=rf"operand='bf16' needs set_{which}_precision\('16-mixed'\)"):
            setter("32-true", operand="bf16")
        assert getattr(m, which + "_precision") == "32-true" and getattr(m, which + "_operand") == "fp16"   # a refusal changes nothing
        setter("32-true", operand="fp16")
    s = TrainSettings(train_operand="bf16", frontend_precision="16-mixed", frontend_operand="x")
    for level in ("model", "recipe"):
        found = {(v.what, v.needs) for v in s.violations(level)}
        assert {("train_operand", "train_mixed"), ("frontend_operand", None)} <= found, (level, found)
    with pytest.raises(ValueError, match="16-mixed"):
        PLBeatThis(**SMALL, mixed_operand="bf16")
    with pytest.raises(ValueError, match="16-mixed"):
        PLBeatThis(**SMALL, precision="16-mixed", frontend_mixed_operand="bf16")
    with pytest.raises(ValueError, match="16-mixed"):
        train.fit(PLBeatThis(**SMALL), None, 0, mixed_operand="bf16")
    base = ["--data-dir", "/nowhere/at/all", "--output", "o"]
    for flags, text in ((["--mixed-operand", "bf16"], "--mixed-operand needs --precision 16-mixed"),
                        (["--mixed-operand", "fp16"], "--mixed-operand needs --precision 16-mixed"),
                        (["--train-frontend", "--frontend-mixed-operand", "bf16"], "--frontend-mixed-operand needs --frontend-precision 16-mixed"),
                        (["--precision", "16-mixed", "--train-frontend", "--frontend-mixed-operand", "fp16"],
                         "--frontend-mixed-operand needs --frontend-precision 16-mixed"),
                        (["--frontend-precision", "16-mixed", "--frontend-mixed-operand", "bf16"], "--frontend-precision needs --train-frontend"),
                        (["--precision", "16-mixed", "--mixed-operand", "bf17"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            train.main(base + flags)
        assert e.value.code == 2 and text in capsys.readouterr().err, flags


def test_the_route_carries_the_operand_of_its_own_part():
    tf = dict(frontend_trainable=True)
    s = TrainSettings(**tf, train_precision="16-mixed", train_operand="bf16", frontend_precision="16-mixed")
    assert decide(s, "transformer", True, False, False, True) == Route(DIFF, mixed=True, operand="bf16")
    assert decide(s, "frontend", True, False, False, True) == Route(DIFF, mixed=True)
    s = TrainSettings(**tf, train_precision="16-mixed", frontend_precision="16-mixed", frontend_operand="bf16")
    assert decide(s, "transformer", True, False, False, True) == Route(DIFF, mixed=True)
    assert decide(s, "frontend", True, False, False, True) == Route(DIFF, mixed=True, operand="bf16")
    assert decide(s, "heads", True, False, False, True) == Route(DIFF)
    assert decide(s, "frontend", False).operand == "fp16"
    m = BeatThis(**SMALL).set_frontend_trainable().set_frontend_precision("16-mixed", "bf16")
    x = torch.zeros(2, 8, 128)
    assert m._route("frontend", m.frontend, x) == Route(DIFF, mixed=True, operand="bf16")
    assert m._route("transformer", m.transformer_blocks, x.clone().requires_grad_(True)) == Route(DIFF)


def test_the_settings_travel_with_the_model_and_old_pickles_load():
    m = BeatThis(**SMALL).set_train_precision("16-mixed", "bf16")
    twin = pickle.loads(pickle.dumps(m))
    assert twin.train_operand == "bf16" and twin.frontend_operand == "fp16" and twin.train_settings == m.train_settings
    # a model pickled when every setting was a loose attribute, and one whose settings object predates the two fields
    state = m.__getstate__()
    state.pop("train_settings")
    state["_train_precision"] = "16-mixed"
    old = BeatThis.__new__(BeatThis)
    old.__setstate__(state)
    assert (old.train_precision, old.train_operand, old.frontend_operand) == ("16-mixed", "fp16", "fp16")
    older = TrainSettings.__new__(TrainSettings)
    older.__dict__.update({k: v for k, v in vars(TrainSettings(train_precision="16-mixed")).items() if not k.endswith("_operand")})
    state = m.__getstate__()
    state["train_settings"] = older
    old = BeatThis.__new__(BeatThis)
    old.__setstate__(state)
    assert (old.train_precision, old.train_operand, old.frontend_operand) == ("16-mixed", "fp16", "fp16")
    assert old.set_train_precision("16-mixed", "bf16").train_operand == "bf16"


# ---- 2. the structs, the module, the parser ----------------------------------------------------------------------------------------
def test_the_operand_fields_lie_where_the_reserved_ones_lay():
    assert (L.OPERAND_F16, L.OPERAND_BF16) == (0, 1) and L.OPERANDS == {"fp16": 0, "bf16": 1}
    assert L.TrainArgs.operand.offset == 28 == L.TrainArgs.sum_head.offset + 4 and L.TrainArgs.rope.offset == 32
    assert L.FrontArgs.operand.offset == 24 == L.FrontArgs.mixed.offset + 4 and L.FrontArgs.w.offset == 32
    assert L.FrontBnArgs.operand.offset == 20 == L.FrontBnArgs.mixed.offset + 4 and L.FrontBnArgs.w.offset == 32
    for struct in (L.TrainArgs, L.FrontArgs, L.FrontBnArgs):
        assert struct.operand.size == 4 and struct().operand == 0 and not hasattr(struct, "reserved1") and not hasattr(struct, "reserved")
    # no struct changed its size, and the library agrees with the binding on it (its own self-check entries)
    import ctypes

    lib = L.lib()
    for struct, sizes, n, size in ((L.TrainArgs, lib.bt_train_struct_sizes, 7, 216), (L.FrontArgs, lib.bt_front_struct_sizes, 7, 216),
                                   (L.FrontBnArgs, lib.bt_front_bn_struct_sizes, 9, 248)):
        out = (ctypes.c_int32 * n)()
        sizes(out)
        assert ctypes.sizeof(struct) == out[0] == size, struct


def test_the_module_takes_the_operands_and_its_hyper_parameters_are_unchanged():
    plain = PLBeatThis(**SMALL)
    pl = PLBeatThis(**SMALL, precision="16-mixed", mixed_operand="bf16", train_frontend=True, frontend_precision="16-mixed",
                    frontend_mixed_operand="bf16")
    assert (pl.model.train_operand, pl.model.frontend_operand) == ("bf16", "bf16") and not pl.model.train_settings.needs_loss_scale()
    assert pl.hyper_parameters == plain.hyper_parameters
    assert not set(pl.hyper_parameters) & {"mixed_operand", "frontend_mixed_operand", "train_operand", "frontend_operand", "operand"}
    half = PLBeatThis(**SMALL, precision="16-mixed", mixed_operand="bf16", train_frontend=True, frontend_precision="16-mixed")
    assert (half.model.train_operand, half.model.frontend_operand) == ("bf16", "fp16") and half.model.train_settings.needs_loss_scale()
    assert PLBeatThis(**SMALL, precision="16-mixed").model.train_operand == "fp16"


class NoData:
    def setup(self, stage):
        pass

    def train_dataloader(self):
        return []


def test_fit_applies_the_operands_before_it_builds_anything():
    """on the CPU fit() ends where it builds the optimiser, after every setting was applied (tests/test_train_settings.py)"""
    pl = PLBeatThis(**SMALL)
    with pytest.raises(RuntimeError, match="ROCm GPUs only"):
        train.fit(pl, NoData(), 0, log=lambda s: None, precision="16-mixed", mixed_operand="bf16", train_frontend=True,
                  frontend_precision="16-mixed", frontend_mixed_operand="bf16")
    m = pl.model
    assert (m.train_precision, m.train_operand, m.frontend_precision, m.frontend_operand) == ("16-mixed", "bf16", "16-mixed", "bf16")
    with pytest.raises(RuntimeError, match="ROCm GPUs only"):   # an operand alone re-sets the part's present precision with it
        train.fit(pl, NoData(), 0, log=lambda s: None, mixed_operand="fp16")
    assert (m.train_precision, m.train_operand, m.frontend_operand) == ("16-mixed", "fp16", "bf16")


def test_the_parser():
    p = train.get_parser()
    base = ["--data-dir", "d", "--output", "o"]
    a = p.parse_args(base)
    assert a.mixed_operand is None and a.frontend_mixed_operand is None
    a = p.parse_args(base + ["--precision", "16-mixed", "--mixed-operand", "bf16", "--train-frontend", "--frontend-precision", "16-mixed",
                             "--frontend-mixed-operand", "fp16"])
    assert (a.precision, a.mixed_operand, a.frontend_precision, a.frontend_mixed_operand) == ("16-mixed", "bf16", "16-mixed", "fp16")
    try:   # past the parser: "no GPU" (returns 2) or the data folder that is not there
        train.main(["--data-dir", "/nowhere/at/all", "--output", "/nowhere/at/all/o", "--max-epochs", "0", "--precision", "16-mixed",
                    "--mixed-operand", "bf16"])
    except (OSError, ValueError, RuntimeError):
        pass


# ---- 3. the yardstick against its own contract ---------------------------------------------------------------------------------------
def check(name, case):
    """e_ref_bf16 is finite and non-zero and the contract twin sits within the gate, on every gradient key, y and the logits"""
    return BF.gate(name, case["twin"], case)


def test_the_rounding_is_to_nearest_even_and_keeps_the_range():
    t = torch.tensor([257.0, 259.0, 3.0e38, -1.0e-40, float("nan"), 65520.0])
    r = BF.rbf16(t)
    assert r[:2].tolist() == [256.0, 260.0] and torch.isfinite(r[2]) and r[3] != 0 and torch.isnan(r[4]) and r[5] == 65536.0
    assert torch.isinf(t.to(torch.float16)[5])   # (what fp16 does to the same value)
    with BF.bfloat16():
        assert BF.REF.r16 is BF.rbf16
    assert BF.REF.r16 is not BF.rbf16 and BF.G._run is not BF._run


@pytest.mark.parametrize("D", sorted(RC.UNIT_DIMS))
@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_units(kind, D):
    for B, T in RC.UNIT_SIZES:
        check(f"bf16 twin {kind} D={D} B={B} T={T}", BF.unit_case(kind, D, B, T))


@pytest.mark.parametrize("kind", ["attn", "ff"])
def test_units_with_dropout(kind):
    for i, (B, T) in enumerate(RC.DROP_SIZES):
        check(f"bf16 twin dropout {kind} T={T}", BF.unit_case(kind, 64, B, T, 40 + i))


def test_trunk():
    check("bf16 twin trunk", BF.trunk_case())


def test_frontend_units():
    for i, B, T in BF.CONV:
        check(f"bf16 twin conv{i} B={B} T={T}", BF.conv_case(i, B, T))
    for i, B, T in BF.CONV_BN:
        check(f"bf16 twin conv{i} batch statistics B={B} T={T}", BF.conv_case(i, B, T, batch=True))
    for i, leaf, B, T in BF.LEAVES:
        check(f"bf16 twin block {i} {leaf} B={B} T={T}", BF.leaf_case(i, leaf, B, T))
    for B, T in BF.LINEAR:
        check(f"bf16 twin projection B={B} T={T}", BF.linear_case(B, T))


def test_whole_model():
    check("bf16 twin whole model", BF.model_case())
