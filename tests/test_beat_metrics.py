"""Beat-tracking metrics (beat_this_amd/metrics.py, csrc/metrics.hip host code) against analytic values and against
tests/metrics_reference.py, a numpy restatement of mir_eval.beat (reference: Metrics, pl_module.py:320-339)."""
import warnings

import numpy as np
import pytest

import metrics_reference as R
from beat_this_amd import metrics as M
from beat_this_amd.evaluate import load_beat_annotations

N = 61
REF = np.arange(N) * 0.5   # 0 .. 30 s every 0.5 s: exact in binary
EXACT = [0, 1, 2, 5, 6, 7, 8, 9, 10, 11]   # every column but Cemgil / CemgilMax


def host_rows(tracks, min_beat_time=-np.inf, thresholds=(0.07, 0.04, 0.175, 0.175)):
    from beat_this_amd import _lib

    ref = np.concatenate([r for r, _ in tracks] + [np.zeros(1)])
    est = np.concatenate([e for _, e in tracks] + [np.zeros(1)])
    roff = np.zeros(len(tracks) + 1, np.int64)
    eoff = np.zeros(len(tracks) + 1, np.int64)
    roff[1:] = np.cumsum([r.size for r, _ in tracks])
    eoff[1:] = np.cumsum([e.size for _, e in tracks])
    out = np.full((len(tracks), 12), -1.0)
    _lib.check(_lib.lib().bt_beat_metrics_host(ref.ctypes.data, roff.ctypes.data, est.ctypes.data, eoff.ctypes.data,
                                               len(tracks), min_beat_time, *thresholds, out.ctypes.data))
    return out


def all_metrics(ref, est):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        F = M.f_measure(ref, est)
        cem = M.cemgil(ref, est)
        cont = M.continuity(ref, est)
    return F, cem, cont


def test_analytic_identity_and_shifts():
    F, cem, cont = all_metrics(REF, REF)
    assert F == 1 and cem == (1.0, 1.0) and cont == (1.0, 1.0, 1.0, 1.0)
    row = host_rows([(REF, REF)])[0]
    assert list(row[:9]) == [1.0] * 9 and row[9] == row[10] == N and row[11] == 0
    assert M.f_measure(REF, REF + 0.0625) == 1.0
    assert M.f_measure(REF, REF + 0.078125) == 0.0


def test_analytic_metrical_levels():
    off = (REF[1:] + REF[:-1]) / 2   # the n - 1 off-beat midpoints
    F, _, (cmlc, cmlt, amlc, amlt) = all_metrics(REF, off)
    assert F == 0 and cmlt == 0 and amlt == 1
    double = np.arange(2 * N - 1) * 0.25   # every 0.25 s: the double-tempo variation
    row = host_rows([(REF, double)])[0]
    assert row[6] == 0 and row[8] == 1
    assert row[1] == N / (2 * N - 1) and row[2] == 1
    assert M.continuity(REF, REF[::2])[3] == 1


def test_analytic_empty():
    with pytest.warns(UserWarning, match="Estimated beats are empty"):
        assert M.f_measure(REF, np.zeros(0)) == 0
    with pytest.warns(UserWarning, match="Reference beats are empty"):
        assert M.cemgil(np.zeros(0), REF) == (0.0, 0.0)
    with pytest.warns(UserWarning):
        assert M.continuity(np.zeros(0), REF) == (0.0, 0.0, 0.0, 0.0)
    for r, e in ((REF, np.zeros(0)), (np.zeros(0), REF), (np.zeros(0), np.zeros(0))):
        row = host_rows([(r, e)])[0]
        assert list(row[:9]) == [0.0] * 9 and row[11] == 0


def test_metrics_trim_edge():
    m = M.Metrics(5)
    truth = np.array([5.0, 5.5, 6.0, 6.5])
    kept = m(truth, np.array([5.0, 5.5, 6.0, 6.5]), "test")
    assert kept["F-measure"] == 1.0
    below = np.nextafter(5.0, 0)
    dropped = m(np.array([below, 5.5, 6.0, 6.5]), np.array([below, 5.5, 6.0, 6.5]), "test")
    assert dropped["F-measure"] == 1.0   # the beat below 5 s is gone from both sides
    # kept on one side only: the truth's 5.0 s beat has no partner once the prediction's is dropped
    one_sided = m(truth, np.array([below, 5.5, 6.0, 6.5]), "test")
    assert one_sided["F-measure"] == pytest.approx(2 * 1.0 * 0.75 / 1.75)
    assert M.trim_beats(np.array([below, 5.0, 7.0])).tolist() == [5.0, 7.0]


def test_metrics_keys_and_shapes():
    rng = np.random.default_rng(1)
    truth = np.sort(rng.uniform(0, 30, 60))
    preds = np.sort(truth + rng.normal(0, 0.03, 60))
    m = M.Metrics(5)
    val = m(truth, preds, "val")
    test = m(truth, preds, "test")
    assert list(val) == ["F-measure", "Cemgil"]
    assert list(test) == ["F-measure", "Cemgil", "CMLt", "AMLt"]
    assert isinstance(val["Cemgil"], tuple) and len(val["Cemgil"]) == 2
    assert val["F-measure"] == test["F-measure"] and val["Cemgil"] == test["Cemgil"]
    o = R.row(truth, preds, 5)
    assert test["F-measure"] == o[0] and test["CMLt"] == o[6] and test["AMLt"] == o[8]
    assert test["Cemgil"] == pytest.approx((o[3], o[4]), rel=1e-12)
    with pytest.raises(ValueError):
        m(truth, preds, "train")


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
    for fn in (M.f_measure, M.cemgil, M.continuity):
        with pytest.raises(ValueError):
            fn(ref, REF)
        with pytest.raises(ValueError):
            fn(REF, ref)
    if bad == "nan":   # trim_beats drops NaN (NaN >= t is false) before Metrics validates, as in the reference
        assert M.Metrics(0)(REF, ref, "test")["F-measure"] == M.f_measure(REF, np.delete(REF, 3))
    elif bad != "2d":
        with pytest.raises(ValueError):
            M.Metrics(0)(REF, ref, "test")
    if bad != "2d":
        # the host code's own status word says the same to a C caller
        st = host_rows([(ref, REF), (REF, ref)])[:, 11]
        assert st[0] != 0 and st[1] != 0 and np.isnan(host_rows([(ref, REF)])[0, :9]).all()


def test_host_status_bits():
    late = np.array([1.0, 30000.5])
    rows = host_rows([(late, REF), (REF, late), (REF[::-1].copy(), REF), (np.array([np.inf]), REF), (REF, REF)])
    assert rows[0, 11] == M.STATUS_LATE and rows[1, 11] == M.STATUS_LATE << 3
    assert rows[2, 11] == M.STATUS_UNSORTED
    assert rows[3, 11] == M.STATUS_NONFINITE | M.STATUS_LATE
    assert rows[4, 11] == 0
    # events before min_beat_time are trimmed before validation, as Metrics trims before mir_eval validates
    assert host_rows([(np.array([3.0, 1.0, 6.0, 7.0]), REF)], min_beat_time=5.0)[0, 11] == 0


@pytest.fixture(scope="module")
def fuzz():
    return R.fuzz_tracks(seed=11, n_tracks=2000, long_tracks=1)


def _compare(got, want, what):
    bad = np.nonzero((got[:, EXACT].view(np.int64) != want[:, EXACT].view(np.int64)).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} tracks differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    np.testing.assert_allclose(got[:, 3:5], want[:, 3:5], rtol=1e-12, atol=0, err_msg=what)


def test_host_matches_oracle_fuzz(fuzz):
    assert len(fuzz) >= 2001 and max(r.size for r, _ in fuzz) == 20000
    got = host_rows(fuzz)
    want = np.array([[*R.row(r, e), 0.0] for r, e in fuzz])
    _compare(got, want, "untrimmed")
    # with the reference's trim (eval_trim_beats = 5) on a subset
    sub = fuzz[:400]
    _compare(host_rows(sub, 5.0), np.array([[*R.row(r, e, 5.0), 0.0] for r, e in sub]), "trimmed at 5 s")


def test_oracle_matching_is_maximum_and_greedy_agrees():
    """the oracle's augmenting-path matching against brute force on tiny cases, and against the library's greedy count"""
    import itertools

    rng = np.random.default_rng(5)
    for _ in range(300):
        r = np.sort(rng.choice(np.arange(0, 1, 0.03125), rng.integers(0, 6), replace=True))
        e = np.sort(rng.choice(np.arange(0, 1, 0.03125), rng.integers(0, 6), replace=True))
        hits = set(zip(*R._fast_hit_windows(r, e, 0.07)))
        best = 0
        for k in range(min(len(r), len(e)), 0, -1):
            for es in itertools.combinations(range(len(e)), k):
                if any(all((ri, ei) in hits for ri, ei in zip(rs, es)) for rs in itertools.permutations(range(len(r)), k)):
                    best = k
                    break
            if best:
                break
        assert len(R.match_events(r, e, 0.07)) == best
        if len(r) and len(e):
            assert host_rows([(r, e)])[0, 1] * len(e) == best


def test_load_beat_annotations(tmp_path):
    two = tmp_path / "two.beats"
    two.write_text("0.5\t1\n1.0\t2\n1.5\t3\n2.0\t1\n2.5\t2\n")
    beats, downbeats = load_beat_annotations(two)
    assert beats.tolist() == [0.5, 1.0, 1.5, 2.0, 2.5] and downbeats.tolist() == [0.5, 2.0]
    one = tmp_path / "one.beats"
    one.write_text("0.25\n0.75\n1.25\n")
    beats, downbeats = load_beat_annotations(one)
    assert beats.tolist() == [0.25, 0.75, 1.25] and downbeats.size == 0 and downbeats.dtype == np.float64
    single = tmp_path / "single.beats"
    single.write_text("3.5\t1\n")
    beats, downbeats = load_beat_annotations(single)
    assert beats.tolist() == [3.5] and downbeats.tolist() == [3.5]
