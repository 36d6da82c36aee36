"""Frontend dropout without a GPU: the CPU restatement route_reference.py against the oracle and
against the host twin of the mask contract at the leaves' shapes, the opt-in's state on ``BeatThis``, the new switches of
``PLBeatThis`` and of the command line, and the seed of a new model's initial weights."""
import ctypes as C

import numpy as np
import pytest
import torch

import route_cases as RC
import route_grads as RG
import route_reference as REF
from route_harness import same_bits
from beat_this_amd import weights as W
from oracle import beat_this_oracle as O

HP = dict(transformer_dim=64, ff_mult=2, n_layers=2)
SEED = 0x5EED_0000_0000_0021
SMALL = dict(transformer_dim=64, n_layers=2, ff_mult=2)


def state_dict(partial=True):
    return W.random_state_dict(W.resolve_hparams(dict(HP, partial_transformers=partial)), seed=3, style="lively")


# ---- the helper -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("partial", [True, False])
def test_with_every_rate_zero_the_helper_is_the_oracle(partial):
    sd = state_dict(partial)
    x = RC.spect(2, 9, seed=1)
    pl, trunk, used = REF.model_plan(sd, 0.0, 0.0, SEED)
    assert used == 0 and trunk is None and all(v is None for v in pl.values())
    with torch.no_grad():
        assert same_bits(REF.frontend(x, sd, pl), O.frontend(x, sd))
        beat, down = REF.model(x, sd, pl, trunk)
        want = O.model_forward(sd, x)
    assert same_bits(beat, want[0]) and same_bits(down, want[1])


def test_the_plan_numbers_the_leaves_in_forward_order():
    pl = REF.plan(0.1, SEED, first=5)
    order = [(i, leaf) for i in range(3) for leaf in REF.LEAVES]
    assert list(pl) == order and [pl[k][2] for k in order] == list(range(5, 17))
    assert all(pl[k][:2] == (0.1, SEED) for k in order)
    sd = state_dict()
    _, trunk, used = REF.model_plan(sd, 0.1, 0.2, SEED, first=5)
    assert trunk == (0.2, SEED, 17) and used == 12 + 2 * HP["n_layers"]
    _, trunk, used = REF.model_plan(sd, 0.0, 0.2, SEED, first=5)                  # a rate of 0 takes no number
    assert trunk == (0.2, SEED, 5) and used == 2 * HP["n_layers"]
    _, trunk, used = REF.model_plan(state_dict(False), 0.1, 0.2, SEED, first=5)   # no partial transformers: no leaves
    assert trunk == (0.2, SEED, 5) and used == 2 * HP["n_layers"]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_the_host_twin_gives_the_masks_of_both_directions(i):
    """bt_dropout_mask_host at a leaf's (B', T', C) against the masks the helper multiplies by, at every (F, C) of the blocks;
    T = 3: a ragged last key group in the time direction, T' = F a multiple of 4 in the frequency direction"""
    from beat_this_amd import _lib

    _lib.build()
    B, T, p = 2, 3, 0.3
    F_, C_ = REF.BLOCK_SHAPES[i]
    assert REF.leaf_shape(i, "attnF", B, T) == (B * T, F_, C_) and REF.leaf_shape(i, "ffT", B, T) == (B * F_, T, C_)
    hidden = 2 * C_
    for j, leaf in enumerate(REF.LEAVES):
        Bp, Tp, _ = REF.leaf_shape(i, leaf, B, T)
        drop = (p, SEED, 100 + 4 * i + j)
        got = REF.leaf_masks(i, leaf, drop, B, T, hidden)
        sites = (REF.ATTN_P, REF.ATTN_OUT) if leaf.startswith("attn") else (REF.FF_HIDDEN, REF.FF_OUT)
        for m, site in zip(got, sites):
            d = _lib.TrainDropout(p=p, seed=SEED, stream=drop[2])
            out = np.full(m.size, 7, dtype=np.uint8)
            _lib.check(_lib.lib().bt_dropout_mask_host(C.byref(d), site, Bp, Tp, C_, hidden, out.ctypes.data))
            assert np.array_equal(out, m.reshape(-1)), (i, leaf, site)
            assert 0.5 < m.mean() < 0.9
        # the row order: the mask row of the time direction's (b, f, t) is (b F + f) T + t, of the frequency direction's (b T + t) F + f
        rows = got[1].reshape(Bp * Tp, C_)
        if leaf == "ffT":
            full = REF.mask(p, SEED, drop[2], REF.FF_OUT, B * F_, T, C_)
            b, f, t = 1, F_ - 1, T - 1
            assert np.array_equal(rows[(b * F_ + f) * T + t], full[(b * F_ + f) * T + t])
            assert np.array_equal(got[1][b * F_ + f, t], full[(b * F_ + f) * T + t])
        if leaf == "ffF":
            full = REF.mask(p, SEED, drop[2], REF.FF_OUT, B * T, F_, C_)
            b, t, f = 1, T - 1, F_ - 1
            assert np.array_equal(got[1][b * T + t, f], full[(b * T + t) * F_ + f])


def test_dropping_one_leaf_moves_the_output_and_the_truth_tells_leaves_apart():
    """the fp64 restatement with one leaf's stream changed is decades beyond 10 e_ref of the unchanged one: a device that took
    the wrong stream, or the rows of the other direction, cannot pass the gate"""
    sd = state_dict()
    i, B, T = 1, 2, 3
    F_, C_ = REF.BLOCK_SHAPES[i]
    gen = torch.Generator().manual_seed(7)
    x, g = torch.randn(B, T, F_, C_, generator=gen), torch.randn(B, T, F_, C_, generator=gen)
    drops = {leaf: (0.1, SEED, j) for j, leaf in enumerate(REF.LEAVES)}
    g32, g64 = (RG.partial_grads(sd, i, x, g, dt, drops=drops) for dt in (torch.float32, torch.float64))
    keys = RG.grad_keys(g64)
    assert len(keys) == 21
    e_ref = max(RG.rel(g32[k], g64[k]) for k in keys)
    assert 0 < e_ref < 1e-5
    for leaf in REF.LEAVES:
        other = RG.partial_grads(sd, i, x, g, torch.float64, drops=dict(drops, **{leaf: (0.1, SEED, 9)}))
        far = max(RG.rel(other[k], g64[k]) for k in keys)
        assert far > 1e3 * RG.GATE * e_ref, (leaf, far, e_ref)
    plain = RG.partial_grads(sd, i, x, g, torch.float64, drops={})
    want = RG.partial_grads(sd, i, x, g, torch.float64)
    for k in want:
        assert torch.equal(plain[k], want[k]), k


# ---- the opt-in's state ---------------------------------------------------------------------------------------------------------
def small_model(**kw):
    from beat_this_amd.model import BeatThis

    return BeatThis(**SMALL, **kw)


def test_the_opt_in_and_its_state():
    m = small_model()
    assert m.dropout_state() is None and not m.frontend_dropout
    m.enable_dropout(seed=5)
    assert m.dropout_state() == {"seed": 5, "calls": 0} and not m.frontend_dropout
    m.enable_dropout(seed=5, frontend=True)
    assert m.dropout_state() == {"seed": 5, "calls": 0, "frontend": True} and m.frontend_dropout
    m.set_dropout_state({"seed": 6, "calls": 40})                      # no key: the opt-in stays
    assert m.dropout_state() == {"seed": 6, "calls": 40, "frontend": True}
    m.set_dropout_state({"seed": 6, "calls": 40, "frontend": False})
    assert m.dropout_state() == {"seed": 6, "calls": 40}
    m.set_dropout_state({"seed": 6, "calls": 41, "frontend": True})
    assert m.frontend_dropout
    m.enable_dropout(seed=7)                                            # without the keyword: today's meaning
    assert m.dropout_state() == {"seed": 7, "calls": 0} and not m.frontend_dropout
    m.enable_dropout(seed=7, frontend=True).disable_dropout()
    assert m.dropout_state() is None and not m.frontend_dropout
    m.enable_dropout(seed=7)
    assert not m.frontend_dropout                                       # disable_dropout cleared both


@pytest.mark.parametrize("rate", [-0.1, 1.0, 1.5, float("nan")])
def test_the_frontend_rate_is_validated_like_the_trunk_rate(rate):
    m = small_model(dropout={"frontend": rate, "transformer": 0.2})
    m.enable_dropout(seed=1)                                            # not opted in: the rate is not looked at
    with pytest.raises(ValueError, match="frontend"):
        m.enable_dropout(seed=1, frontend=True)
    with pytest.raises(ValueError, match="frontend"):
        m.set_dropout_state({"seed": 1, "calls": 0, "frontend": True})
    with pytest.raises(ValueError, match="transformer"):
        small_model(dropout={"frontend": 0.1, "transformer": rate}).enable_dropout(seed=1, frontend=True)


# ---- PLBeatThis and the command line ------------------------------------------------------------------------------------------------
def test_pl_module_refuses_the_opt_in_without_its_prerequisites():
    from beat_this_amd.model.pl_module import PLBeatThis

    with pytest.raises(ValueError, match="apply_dropout"):
        PLBeatThis(**SMALL, apply_frontend_dropout=True, train_frontend=True)
    with pytest.raises(ValueError, match="train_frontend"):
        PLBeatThis(**SMALL, apply_frontend_dropout=True, apply_dropout=True)
    pl = PLBeatThis(**SMALL, apply_dropout=True, dropout_seed=4, train_frontend=True, apply_frontend_dropout=True, init_seed=2)
    assert pl.model.dropout_state() == {"seed": 4, "calls": 0, "frontend": True} and pl.model.frontend_trainable
    assert "apply_frontend_dropout" not in pl.hyper_parameters and "init_seed" not in pl.hyper_parameters
    plain = PLBeatThis(**SMALL, apply_dropout=True, dropout_seed=4, train_frontend=True)
    assert plain.model.dropout_state() == {"seed": 4, "calls": 0}
    assert set(plain.hyper_parameters) == set(pl.hyper_parameters)
    want = small_model().init_weights(2).state_dict()
    for k, v in pl.model.state_dict().items():
        assert torch.equal(v, want[k]), k


def test_the_parser_takes_the_new_flags_and_refuses_the_opt_in_alone(capsys):
    from beat_this_amd import train

    base = ["--data-dir", "d", "--output", "o"]
    args = train.get_parser().parse_args(base)
    assert args.frontend_dropout is None and args.apply_frontend_dropout is False and args.init_seed == 0
    args = train.get_parser().parse_args(base + ["--train-frontend", "--dropout", "--apply-frontend-dropout", "--frontend-dropout", "0.3",
                                                 "--init-seed", "7"])
    assert args.frontend_dropout == 0.3 and args.apply_frontend_dropout is True and args.init_seed == 7
    assert train.get_parser().parse_args(base + ["--no-apply-frontend-dropout"]).apply_frontend_dropout is False
    for have, missing in ((["--train-frontend"], "--dropout"), (["--dropout"], "--train-frontend"), ([], "--dropout")):
        with pytest.raises(SystemExit) as e:
            train.main(["--data-dir", "nowhere", "--output", "nothing.ckpt", "--apply-frontend-dropout"] + have)
        assert e.value.code == 2 and missing in capsys.readouterr().err


# ---- the initial weights ----------------------------------------------------------------------------------------------------------
def test_init_seed_zero_is_the_initial_state_as_ever_and_another_seed_moves_every_weight():
    hp = W.resolve_hparams(SMALL)
    want = W.random_state_dict(hp, seed=0, style="init0")
    default, zero, one = small_model().state_dict(), small_model().init_weights(0).state_dict(), small_model().init_weights(1).state_dict()
    assert list(default) == list(zero) == list(one) == list(want)
    moved = 0
    for k, v in want.items():
        assert torch.equal(default[k], v) and torch.equal(zero[k], v), k
        if not v.is_floating_point() or k.endswith("rotary_embed.freqs"):
            assert torch.equal(one[k], v), k
        elif v.dim() >= 2:                                              # the matrices and the convolutions
            assert one[k].shape == v.shape and not (one[k] == v).any(), k
            moved += 1
        else:                                                           # gains, biases, BatchNorm's weights and statistics
            assert torch.equal(one[k], v) and bool(((v == 0) | (v == 1)).all()), k
    assert moved == sum(1 for v in want.values() if v.is_floating_point() and v.dim() >= 2) > 40
    from beat_this_amd.model.pl_module import PLBeatThis

    assert torch.equal(PLBeatThis(**SMALL, init_seed=1).model.state_dict()["frontend.linear.weight"], one["frontend.linear.weight"])
    for k, v in PLBeatThis(**SMALL).model.state_dict().items():
        assert torch.equal(v, want[k]), k
    # the constructor's arguments stay the architecture, which a checkpoint's hyper-parameters carry one for one
    import inspect

    from beat_this_amd.model import BeatThis

    assert "init_seed" not in inspect.signature(BeatThis).parameters
    assert set(inspect.signature(BeatThis).parameters) <= set(PLBeatThis(**SMALL, init_seed=1).hyper_parameters)
