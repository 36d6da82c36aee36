"""The measure tests/test_gpu_logmel_spec.py holds csrc/logmel.hip to, checked on the CPU before any device sees it
(tests/logmel_reference.py): the gate comes from the reference's own fp32 arithmetic, a correct fp32 evaluation with the
kernel's dataflow stays well inside it, every single-entry mistake is far outside it on a NAMED signal, and the tables the
kernel reads are exactly the reference's."""
import math

import numpy as np
import pytest
import torch

import logmel_reference as LR
from oracle import beat_this_oracle as O

# the signal that sees each mutation of the twin: named, so that an edit of CASES cannot quietly drop the only one that does
SEES = {
    "tw1": "noise_0.1",
    "tw2": "tone_100_noise_1e-3",
    "tw3": "tone_300",
    "tap": "noise_0.1",
    "reflect": "tone_400",
    "frame": "tone_7",
}


@pytest.fixture(scope="module")
def T():
    from beat_this_amd import tables

    return tables.logmel_tables()


def test_case_table():
    assert len(LR.CASES) == 15 + len(LR.LENGTHS)
    for name in LR.CASES:
        x = LR.case(name)
        assert x.dtype == torch.float32 and x.dim() == 1 and bool(torch.isfinite(x).all()), name
        n = int(name.split("_")[1]) if name.startswith("length_") else LR.N_CASE
        assert x.shape[0] == n, name
    assert set(SEES) == set(LR.MUTATIONS) and set(SEES.values()) <= set(LR.CASES)
    assert min(LR.LENGTHS) == 513


def test_twin_stays_within_half_the_gate(T):
    """GATE = 3 R_REF, computed here, not typed in; the twin -- an fp32 evaluation with the kernel's factorisation and table
    twiddles -- must need no more than half of it, the other half being for what it does not model (FMA contraction, the
    butterflies' addition order, hardware sqrt and log)"""
    gate = LR.gate()
    rs = {name: LR.r(LR.twin(LR.case(name), T), LR.case(name)) for name in LR.CASES}
    worst = max(rs, key=rs.get)
    print(f"R_REF = {LR.r_ref_worst():.3g}, GATE = {gate:.3g}, twin worst r = {rs[worst]:.3g} ({worst})")
    assert math.isfinite(gate) and gate > 0
    assert rs[worst] <= gate / 2, rs


@pytest.mark.parametrize("mutate", LR.MUTATIONS)
def test_every_mutation_is_far_outside_the_gate(T, mutate):
    x = LR.case(SEES[mutate])
    got = LR.r(LR.twin(x, T, mutate), x)
    print(f"{mutate} on {SEES[mutate]}: r = {got:.3g}, GATE = {LR.gate():.3g}")
    assert got >= 10 * LR.gate()


def test_mutations_change_one_entry_each(T):
    """(so the figures above are those of the SMALLEST mistake of each kind) the mutated entry is one the kernel reads, and
    conjugating it changes it"""
    tw = T["twiddle"]
    for idx in (LR.MUT_TW1, LR.MUT_TW2, 576 + LR.MUT_TW3_BIN):
        assert tw[idx, 1] != 0.0
    m = LR.MUT_TAP_FILTER
    assert T["mel_w"][m, T["mel_len"][m] - 1] > 0.0
    n = 4410
    for mutate, rows in (("reflect", [0, 1]), ("frame", list(range(1 + n // 441)))):
        diff = np.nonzero((LR.frame_indices(n, mutate) != LR.frame_indices(n)).any(1))[0]
        assert list(diff) == rows, mutate


def test_reflect_index_is_the_reference_padding():
    for n in (513, 952, 1024, 4410):
        x = torch.arange(n, dtype=torch.float64)
        xp = torch.nn.functional.pad(x[None, None, :], (512, 512), mode="reflect")[0, 0]
        assert np.array_equal(xp.unfold(0, 1024, 441).numpy().astype(np.int64), LR.frame_indices(n)), n


def test_tables_are_the_reference_filterbank_and_window(T):
    start, length, w = T["mel_start"], T["mel_len"], T["mel_w"]
    assert w.shape == (128, 32) and w.dtype == np.float32 and start.shape == length.shape == (128,)
    assert int(length.max()) <= 32 and int(length.min()) >= 0 and int(start.min()) >= 0
    dense = np.zeros((513, 128), dtype=np.float32)
    for m in range(128):
        dense[start[m]: start[m] + length[m], m] = w[m, : length[m]]
        assert not w[m, length[m]:].any(), m                      # the kernel reads whole groups of four taps
    assert np.array_equal(dense, O.mel_filterbank(torch.float32).numpy())
    # the row of 520 magnitudes the kernel keeps per frame: it reads up to three bins past a filter's last one
    assert int((start + 4 * ((length + 3) // 4)).max()) <= 520
    assert np.array_equal(T["window"], torch.hann_window(1024, periodic=True, dtype=torch.float32).numpy())


def test_twiddles_are_correctly_rounded(T):
    tw = T["twiddle"]
    assert tw.shape == (1089, 2) and tw.dtype == np.float32
    b, p = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    c, m = np.meshgrid(np.arange(8), np.arange(64), indexing="ij")
    turns = np.concatenate([(b * p).ravel() / 64.0, (c * m).ravel() / 512.0, np.arange(513) / 1024.0])   # exact in float64
    want = np.stack([np.cos(2.0 * np.pi * turns), -np.sin(2.0 * np.pi * turns)], 1)
    # half an fp32 ulp of the entry, plus what the float64 cos / sin of a rounded angle can be off by
    tol = 0.5 * np.spacing(np.abs(tw)).astype(np.float64) + 2.0 ** -50
    assert (np.abs(tw.astype(np.float64) - want) <= tol).all()


def test_unit_is_positive_and_finite():
    xs = {name: LR.case(name) for name in LR.CASES}
    xs["zero"] = torch.zeros(LR.N_CASE)
    for name, x in xs.items():
        b = LR.unit(x)
        assert b.shape == (1 + x.shape[0] // 441, 128) and b.dtype == torch.float64, name
        assert bool(torch.isfinite(b).all()) and float(b.min()) > 0.0, name
    assert float(LR.unit(xs["zero"]).max()) == LR.U               # silence: the rounding of log(1 + 0) alone
    assert LR.r(torch.zeros(11, 128), xs["zero"]) == 0.0
