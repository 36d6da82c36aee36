"""Shared by test_beat_metrics_ext.py and test_gpu_beat_metrics_ext.py: the host call on a list of tracks, the oracle's rows
(computed once per trim and cached), and the comparison of bt_beat_metrics_ext rows under the gates of the two tests."""
import functools

import numpy as np

import metrics_ext_reference as X
import metrics_reference as R

EXACT = [1, 3, 4, 7, 8]        # bit-identical (NaN where the other side has NaN); the status is compared apart
CLOSE = [2, 5, 6, 9, 10]       # within RTOL / ATOL: sums in another order, log2 the only transcendental (Cemgil's gate)
RTOL, ATOL = 1e-12, 1e-15
EXT = (0.35, 0.2, 0.2, 0.2, 41)   # goto_threshold, goto_mu, goto_sigma, p_score_threshold, bins
MAX_LEFT_OUT = 0.005           # of the tracks may be left out of the Goto comparison (goto_left_out)


def csr(tracks):
    ref = np.concatenate([r for r, _ in tracks] + [np.zeros(1)])
    est = np.concatenate([e for _, e in tracks] + [np.zeros(1)])
    roff = np.zeros(len(tracks) + 1, np.int64)
    eoff = np.zeros(len(tracks) + 1, np.int64)
    roff[1:] = np.cumsum([r.size for r, _ in tracks])
    eoff[1:] = np.cumsum([e.size for _, e in tracks])
    return ref, roff, est, eoff


def host_rows(tracks, min_beat_time=-np.inf, ext=EXT):
    from beat_this_amd import _lib

    ref, roff, est, eoff = csr(tracks)
    out = np.full((len(tracks), 12), -1.0)
    _lib.check(_lib.lib().bt_beat_metrics_ext_host(ref.ctypes.data, roff.ctypes.data, est.ctypes.data, eoff.ctypes.data,
                                                   len(tracks), float(min_beat_time), *ext, out.ctypes.data))
    return out


def oracle_rows(tracks, min_beat_time=-np.inf, ext=EXT):
    """rows of the numpy oracle with the status it implies: 256 where its p_score raises, else 0"""
    rows = np.array([X.row_ext(r, e, min_beat_time, *ext) for r, e in tracks]).reshape(len(tracks), 11)
    status = np.where(np.isnan(rows[:, 1]), float(X.PSCORE_UNDEFINED), 0.0)
    return np.concatenate([rows, status[:, None]], 1)


@functools.lru_cache(maxsize=None)
def fuzz():
    return R.fuzz_tracks(seed=0, n_tracks=2000, long_tracks=1)


@functools.lru_cache(maxsize=None)
def fuzz_oracle(trim):
    """the oracle's rows of the fuzz set, read-only; trim None or seconds"""
    rows = oracle_rows(fuzz(), -np.inf if trim is None else float(trim))
    rows.setflags(write=False)
    return rows


def dense_tracks():
    """tracks whose estimates or reference beats fill more than one 4096-event block of the P-score's distinct-index count:
    10 ms grids against sparse beats, on either side, and doubled events across the block boundaries"""
    grid = np.arange(6000) * 0.01 + 1.0
    sparse = np.arange(1.003, 60.0, 4.7)
    doubled = np.repeat(np.arange(2600) * 0.02 + 1.0, 2)
    return [(sparse, grid), (grid, sparse), (doubled, doubled + 0.004), (grid[::3], doubled), (doubled, grid[::7] + 0.001)]


def goto_left_out(ref, est, min_beat_time=-np.inf, ext=EXT):
    """whether a track may be left out of the Goto comparison: the oracle's GotoMean or GotoStd within 1e-9 of its threshold,
    or some |beat_error| within 1e-9 of goto_threshold"""
    r = R.trim_beats(np.asarray(ref, np.float64), min_beat_time)
    e = R.trim_beats(np.asarray(est, np.float64), min_beat_time)
    _, _, _, mean, std, be = X.goto_parts(r, e, *ext[:3])
    if be is None:
        return False
    return bool(abs(mean - ext[1]) <= 1e-9 or abs(std - ext[2]) <= 1e-9 or (np.abs(np.abs(be) - ext[0]) <= 1e-9).any())


def same_bits(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def compare(got, want, tracks, what, min_beat_time=-np.inf, ext=EXT):
    """got against want under the gates -> dict of the largest differences found (for a report)"""
    assert got.shape == want.shape == (len(tracks), 12)
    bad = np.nonzero(got[:, 11] != want[:, 11])[0]
    assert bad.size == 0, f"{what}: status differs on {bad.size} tracks, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    bad = np.nonzero(~same_bits(got[:, EXACT], want[:, EXACT]).all(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} tracks differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"
    worst = {}
    for c in CLOSE:
        a, b = got[:, c], want[:, c]
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: column {c}: NaN in other places"
        ok = ~np.isnan(a)
        err = np.abs(a[ok] - b[ok])
        over = np.nonzero(err > ATOL + RTOL * np.abs(b[ok]))[0]
        assert over.size == 0, f"{what}: column {c}: {over.size} tracks beyond the gate, first {np.nonzero(ok)[0][over[0]]}"
        worst[f"col{c}_max_abs"] = float(err.max()) if err.size else 0.0
    differ = np.nonzero(~same_bits(got[:, 0], want[:, 0]))[0]
    left_out = [int(t) for t in differ if goto_left_out(*tracks[t], min_beat_time, ext)]
    assert len(left_out) == differ.size, f"{what}: Goto differs on tracks {sorted(set(differ) - set(left_out))[:5]}"
    assert len(left_out) <= MAX_LEFT_OUT * len(tracks), f"{what}: {len(left_out)} tracks left out of the Goto comparison"
    worst["goto_left_out"] = len(left_out)
    return worst
