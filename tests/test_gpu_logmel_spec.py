"""csrc/logmel.hip on the device against its specification, on every input class (tests/logmel_reference.py holds the measure;
tests/test_logmel_reference.py shows on the CPU what it separates):

  * tolerance tests: r = max |out - float64 truth| / unit <= GATE = 3 R_REF, the reference's own fp32 error, for every signal of
    CASES, for a tone at every FFT bin on its own (one wrong tw3 entry or mel tap moves one of them by > 1000 GATE), for the
    track lengths at which the frame count or a frame's load path changes, and edge frames against the same 1024 samples
    read through the interior path;
  * exact tests (bits): silence gives 0.0; a sample changes exactly the frames whose index set holds it (the wave-private,
    barrier-free LDS exchange: four frames share a workgroup); a frame does not depend on the parity of its first sample
    (the 8-byte load at a 4-byte-aligned address), on the alignment of the track's base pointer, or on being one of a batch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import logmel_reference as LR
from gpu_util import dev, report

pytestmark = pytest.mark.gpu

NAN = float("nan")


@functools.lru_cache(maxsize=None)
def setup():
    """(LogMelSpect: owns the device tables, bt_logmel_tables pointing into them, the host tables)"""
    from beat_this_amd import tables
    from beat_this_amd.preprocessing import LogMelSpect

    lm = LogMelSpect(device=dev())
    return lm, lm._get_tables(), tables.logmel_tables()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def single(xd):
    """bt_logmel on a device fp32 vector (any 4-byte-aligned view) -> cpu (frames, 128); rows the kernel skips stay NaN"""
    from beat_this_amd import _lib

    assert xd.is_cuda and xd.dtype == torch.float32 and xd.dim() == 1 and xd.is_contiguous()
    n = xd.shape[0]
    out = torch.full((1 + n // 441, 128), NAN, dtype=torch.float32, device=dev())
    with torch.cuda.device(dev()):
        _lib.check(_lib.lib().bt_logmel(_lib.stream_ptr(dev()), C.byref(setup()[1]), xd.data_ptr(), n, out.data_ptr()))
    return out.cpu()


def one(x):
    return single(LR.as_f32(x).to(dev()))


def batch(xs):
    """bt_logmel_batch on tracks packed back to back in ONE allocation (a track starts wherever the one before ends) ->
    [cpu (frames, 128)] per track"""
    from beat_this_amd import _lib

    lens = [int(x.shape[0]) for x in xs]
    n_fr = [1 + n // 441 for n in lens]
    in_off = np.concatenate([[0], np.cumsum(lens)])
    out_off = np.concatenate([[0], np.cumsum(n_fr)])
    packed = torch.cat([LR.as_f32(x) for x in xs]).to(dev())
    spans = torch.tensor([[packed.data_ptr() + 4 * int(in_off[i]), lens[i], int(out_off[i]), n_fr[i]] for i in range(len(xs))],
                         dtype=torch.int64).to(dev())
    out = torch.full((int(out_off[-1]), 128), NAN, dtype=torch.float32, device=dev())
    with torch.cuda.device(dev()):
        _lib.check(_lib.lib().bt_logmel_batch(_lib.stream_ptr(dev()), C.byref(setup()[1]), spans.data_ptr(), len(xs), max(n_fr),
                                              out.data_ptr()))
    res = out.cpu()
    return [res[int(out_off[i]):int(out_off[i + 1])] for i in range(len(xs))]


# ---- tolerance tests: r <= GATE -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LR.CASES))
def test_every_case_within_the_gate(name):
    x = LR.case(name)
    out = one(x)
    got, ref, gate = LR.r(out, x), LR.r_ref(x), LR.gate()
    print(f"{name}: r = {got:.3g} (reference's own fp32: {ref:.3g}), GATE = {gate:.3g}")
    report("logmel_spec_case", case=name, r=got, r_ref=ref, gate=gate)
    assert out.shape == (1 + x.shape[0] // 441, 128)
    assert got <= gate


def test_the_golden_tone_and_noise_within_the_gate():
    """the 3 s 440 Hz tone test_gpu_model.py holds to |delta| < 2e-3 and its 30 s track (1e-4), under the normalised measure"""
    from beat_this_amd import weights as W

    tone = torch.from_numpy((0.5 * np.sin(2 * np.pi * 440.0 * np.arange(22050 * 3) / 22050.0)).astype(np.float32))
    a30 = torch.from_numpy(W.synthetic_audio(30.0, seed=12))
    rs = {name: LR.r(one(x), x) for name, x in (("tone_440hz", tone), ("noise_30s", a30))}
    print(f"r = {rs}, GATE = {LR.gate():.3g}")
    report("logmel_spec_golden_inputs", gate=LR.gate(), **rs)
    assert max(rs.values()) <= LR.gate(), rs


def test_module_forward_is_the_same_call():
    x = LR.case("noise_0.1").to(dev())
    assert same_bits(setup()[0](x).cpu(), single(x))


def test_every_fft_bin_on_its_own():
    """513 tracks of 1764 samples in one launch, track k a tone at bin k of 1024 with a random phase: frame 2 is an interior
    frame.  Bin k alone reads tw3[k], and the filters over bin k get their whole output from the one tap at k."""
    g = torch.Generator().manual_seed(513)
    phase = torch.rand(513, generator=g, dtype=torch.float64) * (2.0 * np.pi)
    xs = [LR.tone(1764, k, 0.5, float(phase[k])) for k in range(513)]
    outs = batch(xs)
    rs = np.array([LR.r(o, x) for o, x in zip(outs, xs)])
    refs = np.array([LR.r_ref(x) for x in xs])
    k = int(rs.argmax())
    print(f"worst r = {rs[k]:.3g} at bin {k} (median {np.median(rs):.3g}); reference's own fp32: worst {refs.max():.3g} at bin "
          f"{int(refs.argmax())}; GATE = {LR.gate():.3g}")
    report("logmel_spec_bins", r=float(rs[k]), bin=k, r_median=float(np.median(rs)), r_ref=float(refs.max()), gate=LR.gate())
    assert all(o.shape == (5, 128) for o in outs)
    assert rs[k] <= LR.gate(), {int(i): float(rs[i]) for i in np.nonzero(rs > LR.gate())[0]}


FRAMES_OF = {513: 2, 514: 2, 881: 2, 882: 3, 883: 3, 952: 3, 953: 3, 954: 3, 1023: 3, 1024: 3, 1025: 3, 1322: 3, 1323: 4, 1324: 4,
             1393: 4, 1394: 4, 1395: 4, 1764: 5, 1835: 5, 1836: 5}


def test_lengths_where_the_frame_count_or_the_load_path_changes():
    lm = setup()[0]
    assert tuple(FRAMES_OF) == LR.LENGTHS
    xs = [LR.case(f"length_{n}") for n in LR.LENGTHS]
    outs = batch(xs)
    rs = {}
    for n, x, o in zip(LR.LENGTHS, xs, outs):
        alone = lm(x.to(dev())).cpu()
        assert alone.shape == o.shape == (FRAMES_OF[n], 128) == tuple(LR.truth(x).shape), n
        assert same_bits(alone, o), n
        rs[n] = LR.r(o, x)
    worst = max(rs, key=rs.get)
    print(f"r per length: { {n: round(v, 2) for n, v in rs.items()} }; GATE = {LR.gate():.3g}")
    report("logmel_spec_lengths", r=rs[worst], n=worst, gate=LR.gate())
    assert rs[worst] <= LR.gate(), rs


def test_edge_path_against_interior_path():
    """Reflect-padded by 882 samples on the host, the track holds in its INTERIOR frame g + 2 the 1024 samples of frame g of
    the original: frames 0, 1, 9 and 10 of 4410 samples take the reflecting loads there and the contiguous ones here.  Each
    side may be GATE units from the truth, so they are within 2 GATE units of each other; they need not be bit-identical (the
    window product may be contracted differently in the two branches) -- whether they are is reported.  Frames 2 .. 8 take the
    interior path on both sides, at the same parity: those are the same bits."""
    x = LR.case("noise_0.1") + LR.tone(LR.N_CASE, 37.3, 0.3, 0.4)
    xp = torch.nn.functional.pad(x[None, None, :], (882, 882), mode="reflect")[0, 0].contiguous()
    a, b = one(x), one(xp)
    assert a.shape == (11, 128) and b.shape == (15, 128)
    idx, idxp = LR.frame_indices(4410), LR.frame_indices(6174)
    assert torch.equal(x[idx], xp[idxp[2:13]])                               # the premise: the same samples, frame by frame
    interior = [g for g in range(11) if g * 441 - 512 >= 0 and g * 441 + 512 <= 4410]
    edge = [g for g in range(11) if g not in interior]
    assert edge == [0, 1, 9, 10]
    assert same_bits(a[interior], b[2:13][interior])
    unit = LR.unit(x)
    d = ((a.double() - b[2:13].double()).abs() / unit)[edge]
    identical = same_bits(a[edge], b[2:13][edge])
    print(f"edge against interior path: worst difference {float(d.max()):.3g} units, bit-identical: {identical}; "
          f"2 GATE = {2 * LR.gate():.3g}")
    report("logmel_spec_edge_vs_interior", units=float(d.max()), identical=bool(identical), gate=LR.gate())
    assert float(d.max()) <= 2 * LR.gate()


# ---- exact tests ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0.0, -0.0])
def test_silence_is_exactly_zero(value):
    out = one(torch.full((LR.N_CASE,), value, dtype=torch.float32))
    assert out.shape == (11, 128) and torch.equal(out, torch.zeros(11, 128))


N_LOCAL = 6615      # 16 frames, four workgroups


@functools.lru_cache(maxsize=None)
def local_base():
    x = LR.gauss(N_LOCAL, 21, 0.1)
    return x, one(x)


@pytest.mark.parametrize("at", [3000, 100, N_LOCAL - 1], ids=["interior", "left_reflection", "last"])
@pytest.mark.parametrize("value", [0.37, NAN], ids=["finite", "nan"])
def test_a_sample_changes_exactly_the_frames_that_hold_it(at, value):
    """No barrier separates the four frames of a workgroup and their LDS rows lie side by side: a frame that does not read the
    sample keeps every bit, with a NaN next door as well."""
    x, base = local_base()
    y = x.clone()
    y[at] = value
    out = one(y)
    idx = LR.frame_indices(N_LOCAL)
    holds = (idx == at).any(1)
    weighted = (idx[:, 1:] == at).any(1)                  # (window[0] = 0: a sample held at position 0 only has no weight)
    assert holds.sum() >= 2 and (~holds).sum() >= 8
    wg = np.arange(16) // 4
    assert any(holds[wg == w].any() and not holds[wg == w].all() for w in range(4))    # a workgroup with both kinds of frame
    for f in range(16):
        if not holds[f]:
            assert same_bits(out[f], base[f]), f
        elif value != value:
            filled = torch.from_numpy(setup()[2]["mel_len"] > 0)
            assert bool(torch.isnan(out[f][filled]).all()), f
        elif weighted[f]:
            assert not same_bits(out[f], base[f]), f
            assert bool(torch.isfinite(out[f]).all()), f


def test_shift_by_one_hop():
    """Interior frame f of x[441:] holds the samples of interior frame f + 1 of x, and its first sample has the other parity:
    from a buffer of its own the 8-byte loads are aligned where those of x are not, and the other way round"""
    x, base = local_base()
    moved = single(x[441:].clone().to(dev()))
    view = single(x.to(dev())[441:])
    assert moved.shape == view.shape == (15, 128)
    interior = [f for f in range(15) if f * 441 - 512 >= 0 and f * 441 + 512 <= N_LOCAL - 441]
    assert interior == list(range(2, 13))
    assert same_bits(moved, view)
    assert same_bits(moved[interior], base[[f + 1 for f in interior]])


def test_base_pointer_alignment():
    x, base = local_base()
    buf = torch.zeros(N_LOCAL + 3, dtype=torch.float32, device=dev())
    assert buf.data_ptr() % 16 == 0
    for off in range(4):
        buf.fill_(NAN)
        buf[off:off + N_LOCAL] = x.to(dev())
        assert same_bits(single(buf[off:off + N_LOCAL]), base), off


@pytest.mark.parametrize("order", ["shortest_first", "longest_first"])
def test_batch_equals_single(order):
    """odd lengths back to back; 2 frames next to 31: whole workgroups of the short tracks leave early"""
    lens = [513, 13231, 1765, 4411, 999, 6617]
    if order == "longest_first":
        lens = [13231, 513, 999, 6617, 1765, 4411]
    xs = [LR.gauss(n, 300 + n, 0.1) + LR.tone(n, 61.7, 0.2) for n in lens]
    outs = batch(xs)
    for n, x, o in zip(lens, xs, outs):
        assert o.shape == (1 + n // 441, 128)
        assert same_bits(o, one(x)), n
