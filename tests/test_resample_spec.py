"""The resamplers against their specification, on the CPU: the filter tables of beat_this_amd/tables.py measured by direct
summation, and the fp32 restatements of tests/resample_reference.py driven with sine tones.  Nothing here is compared with a
second Kaiser design (oracle/shims/soxr restates tables.resample_filter, so a shared design error passes every test that
uses it): the expected values are the specification's -- gain 1 and no delay up to 0.913 x the lower Nyquist frequency,
nothing from 1.0 x it on, both to 1e-6 (-120 dB).

The same file pins which kernel route of launch_resample (csrc/frontend.hip) each tested rate takes, so that a changed
constant cannot silently leave a route without its test rate (tests/test_gpu_resample_spec.py runs these rates on the device)."""
import functools

import numpy as np
import pytest

import resample_reference as R

from beat_this_amd import tables


@functools.lru_cache(maxsize=None)
def filters(sr):
    """(up, down, half, the float64 design, the table the device reads: its fp32 cast, as float64)"""
    up, down = R.up_down(sr)
    h, half = tables.resample_filter(up, down)
    return up, down, half, h, h.astype(np.float32).astype(np.float64)


def grids(sr, up, down):
    """(pass-band, stop-band) frequencies in cycles per sample of the rate the filter runs at (input rate x up); the lower
    Nyquist frequency is 0.5 / max(up, down) there.  About 17 points per ripple and 8 per stop-band lobe (lobe width =
    1 / taps, taps = 188 max(up, down)); the 4.1 M taps of 22051 Hz get a thinned grid with the same band edges."""
    nyq = 0.5 / max(up, down)
    n_pass, n_stop = (101, 201) if sr == 22051 else (1501, 4001)
    return np.linspace(0.0, R.PASS_END * nyq, n_pass), np.linspace(R.STOP_BEGIN * nyq, min(6.0 * nyq, 0.5), n_stop)


@pytest.mark.parametrize("table", ["float64", "float32"])
@pytest.mark.parametrize("sr", R.RATES)
def test_filter_meets_the_specification(sr, table):
    up, down, half, h64, h32 = filters(sr)
    h = h64 if table == "float64" else h32
    assert len(h) == 2 * half + 1 and len(h) % 2 == 1
    assert np.array_equal(h, h[::-1])                                   # linear phase, exactly
    dc = float(np.sum(h))
    if table == "float64":
        assert abs(dc - up) <= 1e-12 * up
    else:
        # Rounding a tap to fp32 moves it by at most 2^-24 of itself, so the sum of the rounded table can be off by
        # 2^-24 sum |h| and no more: that, not 1e-12, is what the number format allows (it is ~1e-9 of ``up`` in practice).
        assert abs(dc - up) <= 1e-12 * up + 2.0 ** -24 * float(np.sum(np.abs(h64)))
    f_pass, f_stop = grids(sr, up, down)
    ripple = float(np.max(np.abs(R.response(h, up, f_pass) - 1.0)))
    stop = float(np.max(R.response(h, up, f_stop)))
    print(f"{sr} Hz ({up}/{down}, half {half}, {table}): DC - up = {dc - up:.2e}, ripple = {ripple:.2e}, stop = {R.db(stop):.1f} dB")
    assert ripple <= R.SPEC
    assert stop <= R.SPEC


# ---- which kernel a rate runs (launch_resample, csrc/frontend.hip) ---------------------------------------------------------
RS_XMAX, RS_HMAX = 4096, 1024          # resample_kernel: staged input samples / staged taps (up == 1 only)
DEC_OUT, DEC_LDS = 256 * 8, 64 * 1024  # decimate_kernel: outputs per workgroup, its LDS bound


def routes(up, down, half, n_in, n_out):
    """the set of routes the workgroups of one launch take, and the largest staged input window"""
    n_taps = 2 * half + 1
    if up == 1 and down in (2, 3, 4):
        qp = ((n_taps + down - 1) // down + 7) & ~7
        if 4 * down * (DEC_OUT + qp) + 4 * down * qp <= DEC_LDS:
            return {f"decimate<{down}>"}, 0
    seen, nx_max = set(), 0
    for m0 in range(0, n_out, 256):
        c_first, c_last = m0 * down - half, (m0 + 255) * down + half
        k0 = 0 if c_first <= 0 else -(-c_first // up)
        k1 = min(c_last // up, n_in - 1)
        nx = k1 - k0 + 1
        nx_max = max(nx_max, nx)
        if nx > RS_XMAX:
            seen.add("x global")
        elif up == 1 and n_taps <= RS_HMAX:
            seen.add("x lds, h lds")
        else:
            seen.add("x lds, up == 1" if up == 1 else "x lds, up > 1")
    return seen, nx_max


EXPECTED_ROUTES = {
    44100: {"decimate<2>"}, 66150: {"decimate<3>"}, 88200: {"decimate<4>"},
    110250: {"x lds, h lds"},
    176400: {"x lds, up == 1"},
    352800: {"x global", "x lds, up == 1"},      # (the first and the last workgroups' windows are clipped by the track's ends)
    8000: {"x lds, up > 1"}, 11025: {"x lds, up > 1"}, 16000: {"x lds, up > 1"}, 32000: {"x lds, up > 1"},
    48000: {"x lds, up > 1"}, 96000: {"x lds, up > 1"}, 192000: {"x lds, up > 1"}, 22051: {"x lds, up > 1"},
}


def test_every_route_of_launch_resample_has_its_rate():
    assert set(EXPECTED_ROUTES) == set(R.RATES)
    for sr in R.RATES:
        up, down, half, _, _ = filters(sr)
        n_out = R.n_out_of(sr)
        got, nx = routes(up, down, half, R.n_in_for(n_out, up, down), n_out)
        assert got == EXPECTED_ROUTES[sr], (sr, up, down, half, got)
        if sr == 192000:
            assert 3800 <= nx <= RS_XMAX, nx          # the staged window nearly full
        if sr == 352800:
            assert nx > 7000, nx
        if sr == 22051:
            assert (n_out - 200) * down + half > 2 ** 31      # tap indices need 64 bits well inside the interior outputs
            assert (2 * half + 1) * 4 < 2 ** 31               # (the table itself stays small)
    # three whole decimator workgroups and a ragged 7: the last thread with outputs stores them one by one
    assert divmod(R.n_out_of(44100), DEC_OUT) == (3, 7)


# ---- tones through the fp32 restatements --------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", R.RATES)
def test_fp32_restatement_passes_and_stops_tones(sr):
    """what sequential fp32 accumulation over the device's table can reach: the reference's own distance from the specification"""
    up, down, half, _, h32 = filters(sr)
    g_err, s_max, cond = R.rational_tones(up, down, half, R.n_out_of(sr),
                                          lambda x, ms: R.polyphase(x, up, down, h32, half, ms, np.float32))
    print(f"{sr} Hz: |G - 1| = {g_err:.2e}, stop = {R.db(s_max)} dB, cond = {cond:.3f}")
    assert cond <= 1.5          # sin and cos at the output frequency are far from collinear on these outputs: the fit is sound
    assert g_err <= R.SPEC
    assert s_max is None or s_max <= R.SPEC
    assert (s_max is None) == (down / up <= R.STOP_TONES[0])


@pytest.mark.parametrize("name", list(R.RATIO_STEPS))
def test_ratio_table_passes_and_stops_tones(name):
    step = R.RATIO_STEPS[name]
    tab, P, Z = tables.resample_ratio_table(), tables.RATIO_TAPS_PER_CROSSING, tables.RATIO_CROSSINGS
    g_err, s_max, cond = R.ratio_tones(step, lambda x, ms: R.ratio(x, step, ms, tab, P, Z, np.float32), Z)
    print(f"step {name}: |G - 1| = {g_err:.2e}, stop = {R.db(s_max)} dB, cond = {cond:.3f}")
    assert cond <= 1.5
    assert g_err <= R.SPEC
    assert s_max is None or s_max <= R.SPEC
    assert (s_max is None) == (step <= R.STOP_TONES[0])


# ---- the tools themselves -----------------------------------------------------------------------------------------------------
def test_reference_tools_on_known_answers():
    """polyphase on an impulse returns the filter's phases; fit_gain recovers a planted gain and delay; response of a two-tap
    average is |cos(pi f)|"""
    rng = np.random.default_rng(3)
    up, down, half = 3, 2, 7
    h = rng.normal(size=2 * half + 1)
    x = np.zeros(9)
    x[4] = 1.0
    ms = np.arange(-(-9 * up // down))
    want = np.array([h[t] if 0 <= t <= 2 * half else 0.0 for t in ms * down + half - 4 * up])
    assert np.array_equal(R.polyphase(x, up, down, h, half, ms), want)
    brute = np.array([sum(xk * h[m * down + half - k * up] for k, xk in enumerate(x[:5] + 1.0)
                          if 0 <= m * down + half - k * up <= 2 * half) for m in ms])
    assert np.allclose(R.polyphase(x[:5] + 1.0, up, down, h, half, ms), brute, rtol=0, atol=1e-14)
    ms = np.arange(50, 3000)
    f = 0.1234
    y = 0.5 * 0.9 * np.sin(2 * np.pi * f * (ms - 0.25) + 0.7)          # gain 0.9, a quarter sample late
    G = R.fit_gain(y, ms, f)
    assert abs(abs(G) - 0.9) < 1e-12 and abs(np.angle(G) + 2 * np.pi * f * 0.25) < 1e-12
    fr = np.linspace(0, 0.5, 33)
    assert np.allclose(R.response([1.0, 1.0], 2, fr), np.abs(np.cos(np.pi * fr)), rtol=0, atol=1e-15)
    long = rng.normal(size=1000)
    direct = np.abs(np.exp(-2j * np.pi * fr[:, None] * np.arange(1000)[None, :]) @ long)
    assert np.allclose(R.response(long, 1, fr), direct, rtol=0, atol=1e-10)
