"""bt_resample (csrc/frontend.hip) and bt_resample_ratio (csrc/stretch.hip) on the device against their SPECIFICATION and
against the literal float64 sums of tests/resample_reference.py, at one input rate per kernel route of launch_resample
(tests/test_resample_spec.py asserts which route each rate takes):

  * sine tones in the pass band come out with complex gain 1 to 1e-6 (magnitude and phase: a delay of one filter tap at
    48 kHz turns a 10 kHz tone by 9e-3 rad), tones in the stop band come out below 1e-6 of their amplitude;
  * every output, both ends included, equals the float64 sum over the table the device reads;
  * tracks of 1, 2 and ``down`` samples and one shorter than the filter do the same inside guard bands, under both poisons.

The expected values are the specification's and the definition's, not another Kaiser design's (oracle/shims/soxr restates
tables.resample_filter and cannot see an error the two share)."""
import functools

import numpy as np
import pytest
import torch

import resample_reference as R
from gpu_util import POISONS, Guarded, _mk, assert_intact, dev, report

pytestmark = pytest.mark.gpu

TIME_TOL = 5e-6        # max |y - float64 sum| / max |float64 sum|: the gate tests/test_gpu_kernels.py holds this kernel to


@functools.lru_cache(maxsize=None)
def setup(sr):
    """(up, down, half, the table the device reads as float64, the same on the device)"""
    from beat_this_amd import tables
    from beat_this_amd.inference import _resample_filter

    up, down = R.up_down(sr)
    h, half = tables.resample_filter(up, down)
    h32 = h.astype(np.float32)
    hd, half_d = _resample_filter(up, down, dev())
    assert half_d == half and torch.equal(hd.cpu(), torch.from_numpy(h32))
    return up, down, half, h32.astype(np.float64), hd


def device_resample(x, sr, n_out):
    """bt_resample with an explicit output count -> numpy fp32 [n_out]"""
    from beat_this_amd import _lib

    up, down, half, _, hd = setup(sr)
    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev())
    y = torch.empty(n_out, dtype=torch.float32, device=dev())
    with torch.cuda.device(dev()):
        _lib.check(_lib.lib().bt_resample(_lib.stream_ptr(dev()), xd.data_ptr(), len(x), up, down, hd.data_ptr(), half, y.data_ptr(), n_out))
    return y.cpu().numpy()


def noise(n, seed):
    return _mk((n,), seed, 0.3).float().numpy()


@pytest.mark.parametrize("sr", R.RATES)
def test_tones_meet_the_specification(sr):
    up, down, half, _, _ = setup(sr)
    n_out = R.n_out_of(sr)
    g_err, s_max, cond = R.rational_tones(up, down, half, n_out, lambda x, ms: device_resample(x, sr, n_out)[ms])
    print(f"{sr} Hz ({up}/{down}): |G - 1| = {g_err:.3e}, stop = {R.db(s_max)} dB")
    report("resample_spec_tones", sr=sr, up=up, down=down, gain_err=g_err, stop_db=R.db(s_max))
    assert cond <= 1.5
    assert g_err <= R.SPEC
    assert s_max is None or s_max <= R.SPEC


@pytest.mark.parametrize("sr", R.RATES)
def test_every_output_equals_the_float64_sum(sr):
    from beat_this_amd.inference import resample_gpu

    up, down, half, h, _ = setup(sr)
    n_in = R.n_in_for(R.n_out_of(sr), up, down)
    n_out = -(-n_in * up // down)
    ms = np.arange(n_out)
    errs = {}
    for name, x in (("noise", noise(n_in, 500 + sr)),
                    ("tone", R.tone(n_in, R.PASS_END * 0.5 * min(1.0, up / down)).astype(np.float32))):
        y = resample_gpu(torch.from_numpy(x).to(dev()), sr, R.OUT_RATE).cpu().numpy()
        assert y.shape == (n_out,) and y.dtype == np.float32
        ref = R.polyphase(x, up, down, h, half, ms, np.float64)
        errs[name] = float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))
    print(f"{sr} Hz ({up}/{down}), {n_out} outputs: max error / max |ref| = {errs}")
    report("resample_spec_outputs", sr=sr, n_out=n_out, err_noise=errs["noise"], err_tone=errs["tone"])
    assert errs["noise"] <= TIME_TOL and errs["tone"] <= TIME_TOL


def degenerate_lengths(up, down, half):
    return sorted({1, 2, down} | ({half // up} if half // up >= 3 else set()))


@pytest.mark.parametrize("sr", R.RATES)
def test_degenerate_lengths_guarded_and_poisoned(sr):
    from beat_this_amd import _lib

    up, down, half, h, hd = setup(sr)
    worst = 0.0
    for n_in in degenerate_lengths(up, down, half):
        n_out = -(-n_in * up // down)
        x = noise(n_in, 900 + sr + n_in)
        ref = R.polyphase(x, up, down, h, half, np.arange(n_out), np.float64)
        outs = []
        for p in POISONS:
            gx = Guarded((n_in,), torch.float32).fill(p, torch.from_numpy(x).to(dev()))
            gh = Guarded((2 * half + 1,), torch.float32).fill(p, hd)
            gy = Guarded((n_out,), torch.float32).fill(p)
            with torch.cuda.device(dev()):
                _lib.check(_lib.lib().bt_resample(_lib.stream_ptr(dev()), gx.ptr(), n_in, up, down, gh.ptr(), half, gy.ptr(), n_out))
            torch.cuda.synchronize()
            where = f"{sr} Hz, {n_in} samples, fill 0x{p:02X}"
            assert_intact((f"input ({where})", gx), (f"filter ({where})", gh), (f"output ({where})", gy))
            assert torch.equal(gx.t.cpu(), torch.from_numpy(x)) and torch.equal(gh.t, hd)
            outs.append(gy.t.cpu().numpy())
            del gx, gh, gy
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), (sr, n_in)
        err = float(np.max(np.abs(outs[0] - ref)) / np.max(np.abs(ref)))
        worst = max(worst, err)
        assert err <= TIME_TOL, (sr, n_in, n_out, err)
    report("resample_spec_degenerate", sr=sr, lengths=degenerate_lengths(up, down, half), err=worst)


# ---- the arbitrary-ratio resampler ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ratio_table():
    from beat_this_amd import tables

    tab = tables.resample_ratio_table()
    return tab, torch.from_numpy(tab).to(dev()), tables.RATIO_TAPS_PER_CROSSING, tables.RATIO_CROSSINGS


def device_ratio(x, step, n_out):
    from beat_this_amd import _lib

    xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev())
    y = torch.empty(n_out, dtype=torch.float32, device=dev())
    with torch.cuda.device(dev()):
        _lib.check(_lib.lib().bt_resample_ratio(_lib.stream_ptr(dev()), xd.data_ptr(), len(x), step, ratio_table()[1].data_ptr(),
                                                y.data_ptr(), n_out))
    return y.cpu().numpy()


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("name", list(R.RATIO_STEPS))
def test_ratio_tones_meet_the_specification(name):
    step = R.RATIO_STEPS[name]
    n_out = int(R.RATIO_N_IN / step)
    g_err, s_max, cond = R.ratio_tones(step, lambda x, ms: device_ratio(x, step, n_out)[ms], ratio_table()[3])
    print(f"step {name}: |G - 1| = {g_err:.3e}, stop = {R.db(s_max)} dB")
    report("resample_ratio_spec_tones", step=name, gain_err=g_err, stop_db=R.db(s_max))
    assert cond <= 1.5
    assert g_err <= R.SPEC
    assert s_max is None or s_max <= R.SPEC


@pytest.mark.parametrize("name", list(R.RATIO_STEPS))
def test_ratio_every_output_equals_the_float64_sum(name):
    """gate: ten times e_ref, the fp32 restatement against the float64 one, relative L2 (the rule tests/test_gpu_stretch.py
    holds this kernel to)"""
    step = R.RATIO_STEPS[name]
    tab, _, P, Z = ratio_table()
    n_out = int(R.RATIO_N_IN / step)
    ms = np.arange(n_out)
    x = noise(R.RATIO_N_IN, 77)
    y64 = R.ratio(x, step, ms, tab, P, Z, np.float64)
    e_ref = rel_l2(R.ratio(x, step, ms, tab, P, Z, np.float32), y64)
    err = rel_l2(device_ratio(x, step, n_out), y64)
    print(f"step {name}, {n_out} outputs: e_ref = {e_ref:.3e}, device = {err:.3e}, ratio = {err / e_ref:.2f}")
    report("resample_ratio_spec_outputs", step=name, n_out=n_out, e_ref=e_ref, device=err)
    assert err <= 10 * e_ref
