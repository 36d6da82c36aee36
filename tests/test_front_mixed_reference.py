"""The yardstick of 16-mixed in the differentiable frontend (tests/route_reference.py), on the CPU:
  1. with the rounding switched off the restatement reproduces the oracle's autograd (fp64, 1e-10 relative);
  2. for every case of tests/test_gpu_front_mixed.py the restatement alone, in fp32, is within 1.5 x e_ref16 of the fp64 truth and
     e_ref16 is finite.  The gate on the device is 2.0 (route_harness.MIXED_GATE); the device differs from the restatement only by the
     order of its fp32 sums.  This is a condition on the cases, not a measurement: a case that failed it would get another seed,
     recorded in section 19.
"""
import math

import pytest
import torch

import route_cases as RC
import route_grads as RG

D64 = torch.float64


def _close(a, b, keys, tol=1e-10):
    for k in keys:
        err = RG.rel(a[k], b[k])
        assert err <= tol, (k, err)


# ---- 1. without the rounding: the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 2])
def test_conv_restatement_without_rounding_is_the_oracle(i):
    sd = RC.model_state_dict()
    x, g = RC.conv_inputs(i, 2, 3)
    for batch in (False, True):
        a = RG.conv_grads(sd, i, x, g, D64, False, batch=batch)
        b = RG.conv_grads(sd, i, x, g, D64, None, batch=batch)
        _close(a, b, RG.grad_keys(b) + ["y"])
        assert len(RG.grad_keys(b)) == 4


def test_partial_and_projection_without_rounding_are_the_oracle():
    sd = RC.model_state_dict()
    x, g = RC.partial_inputs(1, 2, 3)
    a, b = (RG.partial_grads(sd, 1, x, g, D64, on) for on in (False, None))
    assert len(RG.grad_keys(b)) == 21
    _close(a, b, RG.grad_keys(b) + ["y"])
    x, g = RC.linear_inputs(2, 3)
    a, b = (RG.linear_grads(sd, x, g, D64, on) for on in (False, None))
    _close(a, b, RG.grad_keys(b) + ["y"])


@pytest.mark.parametrize("partial", [True, False])
def test_model_restatement_without_rounding_is_the_oracle(partial):
    sd = RC.model_state_dict("lively", partial)
    x, beat, down, mask = RC.model_inputs(2, 33, partial)
    loss_fn = RG.trunk_loss(beat, down, mask)
    a, b = (RG.model_grads(sd, x, loss_fn, D64, on) for on in (False, None))
    assert len(RG.grad_keys(b)) == (100 if partial else 40)
    _close(a, b, RG.grad_keys(b) + ["beat", "downbeat"])


# ---- 2. the contract alone against e_ref16, every GPU case ----------------------------------------------------------------------
def _check(name, case, got):
    e = case["e_ref16"]
    err, key = RG.worst(got, case["truth"])
    print(f"{name}: e_ref16 = {e:.3e} (scale {case['scale']:g}), the restatement is {err / e:.2f} x e_ref16 ({key})")
    assert math.isfinite(e) and e > 0, name
    assert err <= RC.GATE_CPU * e, (name, key, err / e)


@pytest.mark.parametrize("B,T", RC.CONV_SIZES)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_conv_cases(i, B, T):
    case = RC.conv_case(i, B, T)
    _check(f"conv{i} B={B} T={T}", case, RC.restate(case, "conv", i))


@pytest.mark.parametrize("B,T", RC.BN_SIZES)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_conv_batch_statistics_cases(i, B, T):
    case = RC.conv_case(i, B, T, batch=True)
    _check(f"conv{i} batch statistics B={B} T={T}", case, RC.restate(case, "conv", i, batch=True))


@pytest.mark.parametrize("B,T", RC.LINEAR_SIZES)
def test_projection_cases(B, T):
    case = RC.linear_case(B, T)
    _check(f"projection B={B} T={T}", case, RC.restate(case, "linear"))


@pytest.mark.parametrize("B,T", RC.PARTIAL_SIZES)
@pytest.mark.parametrize("i", [0, 1, 2])
def test_partial_cases(i, B, T):
    case = RC.partial_case(i, B, T)
    _check(f"partial{i} B={B} T={T}", case, RC.restate(case, "partial", i))


@pytest.mark.parametrize("B,T", RC.MODEL_SIZES)
@pytest.mark.parametrize("partial", [True, False])
@pytest.mark.parametrize("style", ["lively", "init0"])
def test_model_cases(style, partial, B, T):
    case = RC.model_case(style, partial, B, T)
    assert case["scale"] >= 1024.0, case["scale"]
    _check(f"whole model {style}{'' if partial else ' no partial'} B={B} T={T}", case, RC.restate(case, "model"))


# ---- 3. the opt-in keeps its books without a GPU ---------------------------------------------------------------------------------
def test_the_opt_in_on_a_cpu_model_and_the_command_line(capsys):
    from beat_this_amd import train
    from beat_this_amd.model import BeatThis
    from beat_this_amd.model.pl_module import PLBeatThis

    m = BeatThis(transformer_dim=64, ff_mult=2, n_layers=2)
    assert m.frontend_precision == "32-true" and m.train_precision == "32-true"
    assert m.set_frontend_precision("16-mixed") is m and m.frontend_precision == "16-mixed" and m.train_precision == "32-true"
    m.set_train_precision("16-mixed").set_frontend_precision("32-true")
    assert m.frontend_precision == "32-true" and m.train_precision == "16-mixed"
    for bad in ("bf16-mixed", "16", None, 16):
        with pytest.raises(ValueError, match="frontend precision"):
            m.set_frontend_precision(bad)
    with pytest.raises(AttributeError):
        m.frontend_precision = "16-mixed"
    pl = PLBeatThis(transformer_dim=64, ff_mult=2, n_layers=2, frontend_precision="16-mixed")
    assert pl.model.frontend_precision == "16-mixed" and "frontend_precision" not in pl.hyper_parameters
    assert PLBeatThis(transformer_dim=64, ff_mult=2, n_layers=2).model.frontend_precision == "32-true"
    with pytest.raises(SystemExit) as e:
        train.main(["--data-dir", "nowhere", "--output", "nothing.ckpt", "--frontend-precision", "16-mixed"])
    assert e.value.code == 2 and "--train-frontend" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.get_parser().parse_args(["--data-dir", "d", "--output", "o", "--train-frontend", "--frontend-precision", "bf16"])


def test_the_binding_names_the_field_and_the_queries():
    from beat_this_amd import _lib as L

    for struct in (L.FrontArgs, L.FrontBnArgs):
        names = [f[0] for f in struct._fields_]
        assert "mixed" in names and "reserved0" not in names
    assert L.FrontArgs.mixed.offset == 20 and L.FrontBnArgs.mixed.offset == 16      # the first reserved int32 of each
    assert {"bt_front_workspace_bytes_mixed", "bt_front_bn_workspace_bytes_mixed"} <= set(L.EXPORTS)
