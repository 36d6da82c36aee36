"""CPU side of the trajectory tests (tests/test_gpu_finetune_trajectory.py): the yardstick of the whole fine-tuning loop -- the
fp32 run of tests/route_grads.py against its fp64 run, on ``p_final - p_initial`` of the worst tensor -- shown to tell a
correct loop from each of six one-line deviations by at least ten times the gate."""
import pytest
import torch

import route_grads as RG
from beat_this_amd import weights as W

HP = dict(transformer_dim=64, ff_mult=2, n_layers=2)
T, EPOCHS, PER_EPOCH, ACCUMULATE = 150, 2, 5, 2
# one clip level between the norms of the run: see test_the_yardstick_discriminates
SETTINGS = dict(n_layers=2, lr=2e-3, weight_decay=0.05, warmup=2, total_steps=EPOCHS * 3, accumulate=ACCUMULATE, max_grad_norm=4.0,
                pos_weights={"beat": 2.5, "downbeat": 6.0}, epochs=EPOCHS, batches_per_epoch=PER_EPOCH)


def synthetic_batches():
    """``h`` seeded normal (1, T, 64), targets as tests/test_gpu_backward.py::make_batch draws them; in every epoch batch 1 is
    padded after frame 97 and batch 3 comes from a dataset without downbeat annotation"""
    batches = []
    for i in range(EPOCHS * PER_EPOCH):
        gen = torch.Generator().manual_seed(700 + i)
        h = torch.randn(1, T, 64, generator=gen)
        beat = torch.rand(1, T, generator=gen) < 0.06
        down = beat & (torch.rand(1, T, generator=gen) < 0.3)
        mask = torch.ones(1, T, dtype=torch.bool)
        if i % PER_EPOCH == 1:
            mask[:, 97:] = False
        batches.append(dict(h=h, truth_beat=beat, truth_downbeat=down, padding_mask=mask,
                            downbeat_mask=torch.tensor([i % PER_EPOCH != 3])))
    return batches


@pytest.fixture(scope="module")
def runs():
    sd = W.random_state_dict(W.resolve_hparams(HP), seed=3, style="lively")
    batches = synthetic_batches()
    out = {"sd": sd, 64: RG.run(sd, batches, torch.float64, **SETTINGS), 32: RG.run(sd, batches, torch.float32, **SETTINGS)}
    for mutant in RG.MUTANTS:
        out[mutant] = RG.run(sd, batches, torch.float64, **SETTINGS, mutant=mutant)
    return out


def test_the_loop_is_the_one_described(runs):
    r = runs[64]
    assert [s["count"] for s in r["steps"]] == [2, 2, 1, 2, 2, 1]
    assert r["steps"][0]["lr"] == 0.0 and all(s["lr"] > 0 for s in r["steps"][1:])
    assert len(r["losses"]) == EPOCHS * PER_EPOCH and len(r["epochs"]) == EPOCHS
    for lb, ld, total in r["losses"]:
        assert total == lb + ld and lb > 0
    assert r["losses"][3][1] == 0.0 and r["losses"][8][1] == 0.0          # no downbeat loss without downbeat annotation
    # the first step has rate 0: nothing moves but the moments
    first = RG.run(runs["sd"], synthetic_batches()[:2], torch.float64, **dict(SETTINGS, epochs=1, batches_per_epoch=2))
    for k, d in RG.displacement(first["epochs"][0]["params"], runs["sd"]).items():
        assert float(d.abs().max()) == 0.0, k
    assert all(float(v.abs().max()) > 0 for v in first["epochs"][0]["exp_avg"].values())


def test_the_yardstick_discriminates(runs):
    """Every mutant's worst tensor is at least 100 e_ref from the truth on p_final - p_initial: ten times the gate of
    route_grads.py.  A condition on the inputs chosen above, not a tolerance."""
    sd = runs["sd"]
    norms = [s["norm"] for s in runs[64]["steps"]]
    clipped = [s["coef"] < 1.0 for s in runs[64]["steps"]]
    print("gradient norms of the fp64 run:", " ".join(f"{n:.4f}" for n in norms), "clipped:", clipped)
    assert any(clipped) and not all(clipped)
    d64, d32 = (RG.displacement(runs[k]["epochs"][-1]["params"], sd) for k in (64, 32))
    errs = sorted(RG.rel(d32[k], d64[k]) for k in d64)
    e_ref = RG.yardstick(d32, d64)
    print(f"e_ref = {e_ref:.3e} (median tensor {errs[len(errs) // 2]:.3e})")
    assert 1e-7 < e_ref < 1e-3, e_ref
    ratios = {}
    for mutant in RG.MUTANTS:
        dm = RG.displacement(runs[mutant]["epochs"][-1]["params"], sd)
        ratios[mutant] = max(RG.rel(dm[k], d64[k]) for k in d64) / e_ref
        print(f"{mutant}: worst tensor {ratios[mutant]:.0f} x e_ref")
    for mutant, ratio in ratios.items():
        assert ratio >= 10 * RG.GATE, (mutant, ratio)
