"""mir_eval.beat's goto, p_score, information_gain and evaluate (beat_this_amd/metrics.py, the host code of csrc/metrics.hip:
bt_beat_metrics_ext_host) against analytic values and against tests/metrics_ext_reference.py, the numpy oracle with mir_eval's
structure.  Gates: P-score, the Goto criteria and track length, the P-score window and hits and the status bit-identical; the
information gain, the Goto mean and std and the two entropies within 1e-12 relative + 1e-15 absolute (the project's gate for
Cemgil: numpy sums pairwise, log2 is the only transcendental); Goto identical except on tracks whose oracle mean, std or a beat
error lies within 1e-9 of its threshold (at most 0.5 % of the tracks)."""
import inspect
import warnings

import numpy as np
import pytest

import metrics_ext_reference as X
import metrics_ext_util as U
from beat_this_amd import metrics as M

REF = np.arange(61) * 0.5
IG_SHIFT = 0.977474597743615     # information gain of a constant shift by a quarter or an eighth of the beat
IG_HALF = 0.8133837745405175     # ... of every second beat


def three(ref, est):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return M.goto(ref, est), M.p_score(ref, est), M.information_gain(ref, est)


def test_analytic_values():
    assert three(REF, REF) == (1.0, 1.0, 1.0)
    g, p, ig = three(REF, REF + 0.25)
    assert (g, p) == (0.0, 0.0) and ig == pytest.approx(IG_SHIFT, rel=1e-12)
    g, p, ig = three(REF, REF + 0.0625)
    assert (g, p) == (0.0, 1.0) and ig == pytest.approx(IG_SHIFT, rel=1e-12)
    row = U.host_rows([(REF, REF + 0.0625)])[0]
    assert row[3] == 1 and row[5] == 0.25 and row[6] == 0      # Goto 0: the mean error 0.25 is above goto_mu
    g, p, ig = three(REF, REF[::2])
    assert p == 31 / 61 and ig == pytest.approx(IG_HALF, rel=1e-12)
    row = U.host_rows([(REF, REF[:31])])[0]
    assert row[0] == 0 and row[3] == 1 and row[4] == 32          # the slice holds both incorrect ends
    assert row[6] == pytest.approx(0.246, abs=5e-4) and row[6] > 0.2
    assert three(REF, np.zeros(0)) == (0.0, 0.0, 0.0)
    assert three(REF, REF[5:6]) == (0.0, 0.0, 0.0)
    for est in (np.zeros(0), REF[5:6]):
        row = U.host_rows([(REF, est)])[0]
        assert list(row[:3]) == [0.0, 0.0, 0.0] and row[11] == 0 and list(row[7:11]) == [0.0] * 4
    assert list(U.host_rows([(REF, np.zeros(0))])[0, 3:7]) == [0.0] * 4   # goto returned early: 0 diagnostics


@pytest.mark.parametrize("trim", [None, 5])
def test_host_matches_oracle_fuzz(trim):
    tracks = U.fuzz()
    assert len(tracks) == 2001 and tracks[-1][0].size == 20000
    mbt = -np.inf if trim is None else float(trim)
    want = U.fuzz_oracle(trim)
    # the counting form of the P-score equals the correlate form on every short track: only then may it score the long one
    for t, (r, e) in enumerate(tracks[:-1]):
        r, e = r[r >= mbt], e[e >= mbt]
        try:
            p, win, hits = X.p_score_count_parts(r, e)
        except ValueError:
            p = win = hits = np.nan
        assert U.same_bits(np.array([p, win, hits], np.float64), want[t, [1, 7, 8]]).all(), f"track {t}"
    if trim is None:   # the set is not trivial
        assert np.count_nonzero(want[:, 0] == 1) >= 150
        assert np.count_nonzero((want[:, 1] > 0) & (want[:, 1] < 1)) >= 1000
        assert np.count_nonzero((want[:, 2] > 0) & (want[:, 2] < 1)) >= 1500
        assert not any(U.goto_left_out(r, e) for r, e in tracks)
    worst = U.compare(U.host_rows(tracks, mbt), want, tracks, f"host vs oracle, trim {trim}", mbt)
    print(f"trim {trim}: Goto = 1 on {np.count_nonzero(want[:, 0] == 1)} tracks, largest differences {worst}")


def check(tracks, ext=U.EXT, mbt=-np.inf):
    got = U.host_rows(tracks, mbt, ext)
    U.compare(got, U.oracle_rows(tracks, mbt, ext), tracks, "edge case", mbt, ext)
    return got


def test_edge_one_index():
    """all reference beats in one 10 ms index: mir_eval's p_score raises; the other metrics are valid"""
    ref = np.array([10.001, 10.002, 10.003])
    est = np.array([9.5, 10.0, 10.5])
    row = check([(ref, est), (REF, REF), (np.array([7.0, 7.0]), est)])
    assert row[0, 11] == M.STATUS_PSCORE and np.isnan(row[0, [1, 7, 8]]).all() and not np.isnan(row[0, [0, 2, 3, 9, 10]]).any()
    assert row[1, 11] == 0 and row[2, 11] == M.STATUS_PSCORE
    with pytest.raises(ValueError):
        X.p_score(ref, est)
    with pytest.raises(ValueError, match="p_score undefined"):
        M.p_score(ref, est)
    assert M.goto(ref, est) == row[0, 0] and M.information_gain(ref, est) == row[0, 2]
    with pytest.raises(ValueError, match="p_score undefined"):
        M.evaluate(ref, est, min_beat_time=0.0)
    # a single reference index but fewer than two estimates: the early return comes first
    assert check([(ref, est[:1])])[0, 11] == 0


def test_edge_short_references():
    """2, 3 and 4 reference beats: empty and one-element Goto slices, no track at all"""
    tracks = []
    for n in (1, 2, 3, 4, 5):
        ref = 1.0 + np.arange(n) * 0.5
        tracks += [(ref, ref), (ref, ref + 0.01), (ref, ref[1:] + 0.3), (ref, np.sort(np.concatenate([ref, ref + 0.02])))]
    got = check(tracks)
    by = {(r.size, i % 4): got[i] for i, (r, _) in enumerate(tracks)}
    assert by[(2, 0)][3] == 1 and by[(2, 0)][4] == 0 and np.isnan(by[(2, 0)][5])       # beat_error[1:0]
    assert by[(3, 0)][4] == 0 and np.isnan(by[(3, 0)][5]) and by[(3, 0)][0] == 0       # beat_error[1:1]
    assert by[(4, 1)][4] == 1 and not np.isnan(by[(4, 1)][5]) and np.isnan(by[(4, 1)][6])   # one element: no std
    assert by[(3, 3)][3] == 0 and by[(3, 3)][4] == 0 and np.isnan(by[(3, 3)][5])       # three incorrect beats, gap too short


def test_edge_duplicates_and_wraparound():
    rng = np.random.default_rng(3)
    tracks = []
    for _ in range(40):
        ref = np.sort(rng.uniform(0, 20, rng.integers(2, 30)))
        est = np.sort(ref + rng.normal(0, 0.05, ref.size))
        ref = np.sort(np.concatenate([ref, ref[rng.integers(0, ref.size, 3)]]))     # zero intervals: errors of +-inf, NaN
        est = np.sort(np.concatenate([est, est[rng.integers(0, est.size, 3)]]))
        tracks.append((ref, np.clip(est, 0, None)))
    tracks.append((np.array([1.0, 1.0, 2.0, 2.0]), np.array([1.0, 1.0, 2.0, 2.0])))
    tracks.append((np.array([3.0, 3.0]), np.array([3.0, 3.0, 3.0])))                 # every error dropped: NaN entropies
    # estimates before the first reference beat: the interval wraps to the last beat, as reference_beats[-1] does
    tracks.append((np.array([5.0, 5.5, 6.0, 6.5]), np.array([4.9, 5.4, 6.1, 6.4])))
    tracks.append((np.array([5.0, 5.5, 6.0, 7.5]), np.array([1.0, 4.0, 4.99, 7.4])))
    got = check(tracks)
    assert np.isnan(got[41, 9]) and np.isnan(got[41, 10]) and np.isnan(got[41, 2]) and got[41, 11] == M.STATUS_PSCORE
    assert got[42, 11] == 0 and 0 < got[42, 2] < 1


def test_edge_dense_tracks():
    got = check(U.dense_tracks())
    assert got[0, 8] > 2000 and (got[:, 8] > 0).all() and (got[:, 11] == 0).all()


@pytest.mark.parametrize("bins", [1, 2, 40, 41])
def test_edge_bins(bins):
    tracks = U.fuzz()[:60] + [(REF, REF), (REF, REF + 0.25)]
    ext = U.EXT[:4] + (bins,)
    check(tracks, ext)
    r, e = tracks[0]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ig = M.information_gain(r, e, bins=bins)
    even = [x for x in w if "bins parameter is even" in str(x.message)]
    assert len(even) == (1 if bins % 2 == 0 else 0)
    want = X.information_gain(r, e, bins)
    assert (np.isnan(ig) and np.isnan(want)) or ig == pytest.approx(want, rel=1e-12, abs=1e-15)


def test_edge_bins_out_of_range():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (0 is even)
        for bins in (0, 1025, -3):
            with pytest.raises(Exception):
                M.information_gain(REF, REF, bins=bins)


def test_edge_window_rounds_half_to_even():
    """medians of the reference intervals that end in .5: np.round takes the even neighbour"""
    def at(indices):   # times whose impulse-train index is exactly ``indices`` (the estimates start at 0)
        return (np.asarray(indices) - 0.5) / 100

    est = np.array([0.0, 0.02, 0.5, 1.04])
    cases = [(at([1, 3, 6]), 1.0, 2), (at([1, 4, 8]), 1.0, 4), (at([1, 51, 106]), 0.2, 10), (at([1, 64, 126]), 0.2, 12),
             (at([1, 58, 116, 174, 232]), 0.2, 12)]
    for ref, thr, win in cases:
        ext = U.EXT[:3] + (thr, 41)
        row = check([(ref, est)], ext)[0]
        assert row[7] == win, (ref, thr, row)
        assert M.p_score(ref, est, p_score_threshold=thr) == row[1]


def test_evaluate_is_the_drop_ins():
    rng = np.random.default_rng(8)
    ref = np.sort(rng.uniform(0, 40, 70))
    est = np.sort(np.clip(ref + rng.normal(0, 0.03, ref.size), 0, None))[3:]
    res = M.evaluate(ref, est)
    assert list(res) == ["F-measure", "Cemgil", "Cemgil Best Metric Level", "Goto", "P-score", "Correct Metric Level Continuous",
                         "Correct Metric Level Total", "Any Metric Level Continuous", "Any Metric Level Total",
                         "Information gain"]
    r, e = M.trim_beats(ref), M.trim_beats(est)
    assert r.size < ref.size
    cont = M.continuity(r, e)
    assert list(res.values()) == [M.f_measure(r, e), *M.cemgil(r, e), M.goto(r, e), M.p_score(r, e), *cont,
                                  M.information_gain(r, e)]
    assert all(isinstance(v, float) for v in res.values())
    # keyword arguments reach the functions that take them; unknown names are ignored
    res2 = M.evaluate(ref, est, min_beat_time=0.0, bins=11, p_score_threshold=0.1, goto_mu=0.01, f_measure_threshold=0.01,
                      no_such_argument=3)
    assert res2["Information gain"] == M.information_gain(ref, est, bins=11)
    assert res2["P-score"] == M.p_score(ref, est, p_score_threshold=0.1)
    assert res2["Goto"] == M.goto(ref, est, goto_mu=0.01)
    assert res2["F-measure"] == M.f_measure(ref, est, f_measure_threshold=0.01)
    o = X.row_ext(ref, est, 5.0)
    assert res["Goto"] == o[0] and res["P-score"] == o[1] and res["Information gain"] == pytest.approx(o[2], rel=1e-12)


def test_drop_in_warnings():
    one = REF[10:11]
    for fn in (M.p_score, M.information_gain):
        with pytest.warns(UserWarning, match="Only one reference beat was provided"):
            assert fn(one, REF) == 0
        with pytest.warns(UserWarning, match="Only one estimated beat was provided"):
            assert fn(REF, one) == 0
    for fn in (M.goto, M.p_score, M.information_gain):
        with pytest.warns(UserWarning, match="Estimated beats are empty"):
            assert fn(REF, np.zeros(0)) == 0
        with pytest.warns(UserWarning, match="Reference beats are empty"):
            assert fn(np.zeros(0), REF) == 0
    with warnings.catch_warnings():   # goto has no one-beat warning, and two beats on both sides none at all
        warnings.simplefilter("error")
        M.goto(one, REF)
        M.goto(REF, one)
        three(REF, REF)
        M.information_gain(REF, REF, bins=41)
    with pytest.warns(UserWarning, match="bins parameter is even"):
        M.information_gain(REF, REF, bins=40)


@pytest.mark.parametrize("bad", ["unsorted", "2d", "late", "nan"])
def test_invalid_input_raises(bad):
    ref = REF.copy()
    if bad == "unsorted":
        ref[10], ref[11] = ref[11], ref[10]
    elif bad == "2d":
        ref = np.stack([REF, REF], 1)
    elif bad == "late":
        ref = REF + 29990.0
    else:
        ref[3] = np.nan
    # (evaluate trims first, and trim_beats' boolean index flattens a 2-d array and drops NaN, as in mir_eval)
    for fn in (M.goto, M.p_score, M.information_gain) + ((M.evaluate,) if bad in ("unsorted", "late") else ()):
        with pytest.raises(ValueError):
            fn(ref, REF)
        with pytest.raises(ValueError):
            fn(REF, ref)
    if bad == "nan":
        assert M.evaluate(REF, ref, min_beat_time=0.0)["P-score"] == M.p_score(REF, np.delete(REF, 3))
    if bad != "2d":
        rows = U.host_rows([(ref, REF), (REF, ref), (REF, REF)])
        assert rows[0, 11] != 0 and rows[1, 11] == int(rows[0, 11]) << 3 and rows[2, 11] == 0
        assert np.isnan(rows[:2, :11]).all() and not np.isnan(rows[2]).any()


def test_host_arguments():
    from beat_this_amd import _lib

    L = _lib.lib()
    ref, roff, est, eoff = U.csr([(REF, REF)])
    out = np.zeros(12)
    args = (ref.ctypes.data, roff.ctypes.data, est.ctypes.data, eoff.ctypes.data)
    for bins in (0, 1025):
        assert L.bt_beat_metrics_ext_host(*args, 1, 0.0, *U.EXT[:4], bins, out.ctypes.data) == _lib.BT_ERR_ARG
    assert L.bt_beat_metrics_ext_host(*args, 0, 0.0, *U.EXT, out.ctypes.data) == _lib.BT_ERR_ARG
    assert L.bt_beat_metrics_ext_host(*args, 1, 0.0, *U.EXT, None) == _lib.BT_ERR_ARG
    assert L.bt_beat_metrics_ext_host(*args, 1, 0.0, *U.EXT[:4], 1024, out.ctypes.data) == _lib.BT_OK
    assert L.bt_beat_metrics_ext_workspace_bytes(0, 0, 0) == 0 and L.bt_beat_metrics_ext_workspace_bytes(3, 10, 10) > 0
    bad = np.array([0, -1], np.int64)
    assert L.bt_beat_metrics_ext_host(ref.ctypes.data, bad.ctypes.data, est.ctypes.data, eoff.ctypes.data, 1, 0.0, *U.EXT,
                                      out.ctypes.data) == _lib.BT_OK
    assert out[11] == M.STATUS_OFFSETS and np.isnan(out[:11]).all()


def test_defaults_unchanged():
    assert M.COLUMNS == ("F", "P", "R", "Cemgil", "CemgilMax", "CMLc", "CMLt", "AMLc", "AMLt", "n_ref", "n_est", "status")
    sig = inspect.signature(M.beat_metrics_many)
    assert list(sig.parameters)[:5] == ["truths", "preds", "eval_trim_beats", "device", "raise_on_invalid"]
    assert sig.parameters["extended"].default is False
    assert {k: sig.parameters[k].default for k in M.EXT_DEFAULTS} == M.EXT_DEFAULTS
    plain = M.beat_metrics_many([], [])
    assert list(plain) == ["F-measure", "Precision", "Recall", "Cemgil", "CemgilMax", "CMLc", "CMLt", "AMLc", "AMLt", "n_ref",
                           "n_est", "status", "Cemgil_reported"]
    assert list(M.beat_metrics_many([], [], extended=True)) == list(plain) + list(M.EXT_KEYS)
    from beat_this_amd import evaluate as E

    assert inspect.signature(E.evaluate_bundle).parameters["extended"].default is False
    assert E.get_parser().parse_args(["--models", "m", "--bundle", "b", "--annotations", "a"]).all_metrics is False
