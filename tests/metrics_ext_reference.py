"""Plain numpy restatement of mir_eval.beat's goto, p_score and information_gain (mir_eval 0.7's beat.py, after validate),
with mir_eval's own structure: literal per-beat loops, impulse trains with np.correlate, np.histogram.  csrc/metrics.hip does
not follow that structure (ballots, selection instead of a median sort, counted pairs instead of a correlation), so this is an
independent statement to hold it to.  mir_eval is not installed here: it is not pinned against mir_eval itself.

Each function has a ``*_parts`` form that also returns the continuous quantities behind its decision (the diagnostic columns
of bt_beat_metrics_ext); ``row_ext`` returns the 11 leading columns of a row."""
import warnings

import numpy as np

from metrics_reference import trim_beats

PSCORE_UNDEFINED = 256   # BT_METRICS_PSCORE


def goto_parts(r, e, thr=0.35, mu=0.2, sigma=0.2):
    """-> (goto, criteria, len(track), mean(abs(track)), std(track, ddof=1), beat_error or None); an early return has 0
    diagnostics, no track has NaN mean and std"""
    if e.size == 0 or r.size == 0:
        return 0.0, 0, 0, 0.0, 0.0, None
    n = r.shape[0]
    beat_error = np.ones(n)
    paired = np.zeros(n)
    goto_criteria = 0
    for k in range(1, n - 1):
        prev_interval = 0.5 * (r[k] - r[k - 1])
        window_min = r[k] - prev_interval
        next_interval = 0.5 * (r[k + 1] - r[k])
        window_max = r[k] + next_interval
        beats_in_window = np.logical_and(e >= window_min, e < window_max)
        if beats_in_window.sum() == 0 or beats_in_window.sum() > 1:
            paired[k] = 0
            beat_error[k] = 1
        else:
            paired[k] = 1
            offset = (e[beats_in_window] - r[k])[0]
            if offset < 0:
                beat_error[k] = offset / prev_interval
            else:
                beat_error[k] = offset / next_interval
    incorrect_beats = np.flatnonzero(np.abs(beat_error) > thr)
    track = None
    if incorrect_beats.shape[0] < 3:
        track = beat_error[incorrect_beats[0] + 1:incorrect_beats[-1] - 1]
        goto_criteria = 1
    else:
        track_len = np.max(np.diff(incorrect_beats))
        track_start = np.flatnonzero(np.diff(incorrect_beats) == track_len)[0]
        if track_len - 1 > .25 * (r.shape[0] - 2):
            goto_criteria = 1
            start_beat = incorrect_beats[track_start]
            end_beat = incorrect_beats[track_start + 1]
            track = beat_error[start_beat:end_beat + 1]
    mean = std = np.nan
    if goto_criteria:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            mean = np.mean(np.abs(track))
            std = np.std(track, ddof=1)
        if mean < mu and std < sigma:
            goto_criteria = 3
    return 1.0 * (goto_criteria == 3), goto_criteria, 0 if track is None else track.size, mean, std, beat_error


def goto(r, e, thr=0.35, mu=0.2, sigma=0.2):
    return goto_parts(r, e, thr, mu, sigma)[0]


def _p_window(r, e, thr):
    """the two impulse trains and the window, as mir_eval builds them"""
    offset = min(e.min(), r.min())
    e = np.array(e - offset)
    r = np.array(r - offset)
    end_point = int(np.ceil(np.max([np.max(e), np.max(r)])))
    fs = 100
    reference_train = np.zeros(end_point * fs + 1)
    reference_train[np.ceil(r * fs).astype(int)] = 1.0
    estimated_train = np.zeros(end_point * fs + 1)
    estimated_train[np.ceil(e * fs).astype(int)] = 1.0
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        annotation_intervals = np.diff(np.flatnonzero(reference_train))
        win_size = int(np.round(thr * np.median(annotation_intervals)))   # ValueError: NaN to integer, if no interval
    return reference_train, estimated_train, win_size


def p_score_parts(r, e, thr=0.2):
    """the correlate form -> (p_score, win_size, hits); ValueError where mir_eval raises"""
    if e.size <= 1 or r.size <= 1:
        return 0.0, 0, 0
    reference_train, estimated_train, win_size = _p_window(r, e, thr)
    train_correlation = np.correlate(reference_train, estimated_train, "full")
    middle_lag = train_correlation.shape[0] // 2
    start = middle_lag - win_size
    end = middle_lag + win_size + 1
    train_correlation = train_correlation[start:end]
    n_beats = np.max([e.shape[0], r.shape[0]])
    hits = np.sum(train_correlation)
    return float(hits / n_beats), win_size, int(hits)


def p_score(r, e, thr=0.2):
    return p_score_parts(r, e, thr)[0]


def p_score_count_parts(r, e, thr=0.2):
    """the same numbers without the trains (for tracks too long to correlate)"""
    if e.size <= 1 or r.size <= 1:
        return 0.0, 0, 0
    off = min(e.min(), r.min())
    ri = np.unique(np.ceil((r - off) * 100).astype(np.int64))
    ei = np.unique(np.ceil((e - off) * 100).astype(np.int64))
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        win = int(np.round(thr * np.median(np.diff(ri))))
    hits = int(np.sum(np.searchsorted(ei, ri + win, "right") - np.searchsorted(ei, ri - win, "left")))
    return float(hits) / max(e.size, r.size), win, hits


def p_score_count(r, e, thr=0.2):
    return p_score_count_parts(r, e, thr)[0]


def _get_entropy(reference_beats, estimated_beats, bins):
    beat_error = np.zeros(estimated_beats.shape[0])
    with np.errstate(all="ignore"):
        for n in range(estimated_beats.shape[0]):
            beat_distances = estimated_beats[n] - reference_beats
            closest_beat = np.argmin(np.abs(beat_distances))
            absolute_error = beat_distances[closest_beat]
            if closest_beat == 0:
                interval = .5 * (reference_beats[1] - reference_beats[0])
            if closest_beat == (reference_beats.shape[0] - 1):
                interval = .5 * (reference_beats[-1] - reference_beats[-2])
            else:
                if absolute_error < 0:
                    start = reference_beats[closest_beat - 1]
                    end = reference_beats[closest_beat]
                    interval = .5 * (end - start)
                else:
                    start = reference_beats[closest_beat]
                    end = reference_beats[closest_beat + 1]
                    interval = .5 * (end - start)
            beat_error[n] = .5 * absolute_error / interval
        beat_error = np.mod(beat_error + .5, -1) + .5
        histogram_bin_edges = np.linspace(-.5, .5, bins + 1)
        raw_bin_values = np.histogram(beat_error, histogram_bin_edges)[0]
        raw_bin_values = raw_bin_values / (1.0 * np.sum(raw_bin_values))
        raw_bin_values[raw_bin_values == 0] = 1
        return -np.sum(raw_bin_values * np.log2(raw_bin_values))


def information_gain_parts(r, e, bins=41):
    """-> (information gain, forward entropy, backward entropy)"""
    if e.size <= 1 or r.size <= 1:
        return 0.0, 0.0, 0.0
    forward_entropy = _get_entropy(r, e, bins)
    backward_entropy = _get_entropy(e, r, bins)
    norm = np.log2(bins)
    with np.errstate(all="ignore"):
        if forward_entropy > backward_entropy:
            ig = (norm - forward_entropy) / norm
        else:
            ig = (norm - backward_entropy) / norm
    return float(ig), float(forward_entropy), float(backward_entropy)


def information_gain(r, e, bins=41):
    return information_gain_parts(r, e, bins)[0]


def row_ext(reference_beats, estimated_beats, min_beat_time=-np.inf, goto_threshold=0.35, goto_mu=0.2, goto_sigma=0.2,
            p_score_threshold=0.2, bins=41, correlate_limit=3000):
    """the 11 leading columns of a bt_beat_metrics_ext row (no validation status assumed): Goto, PScore, InfoGain,
    GotoCriteria, GotoTrackLen, GotoMean, GotoStd, PWindow, PHits, EntropyFwd, EntropyBwd.  Where mir_eval's p_score raises
    (no reference interval) columns 1, 7 and 8 are NaN.  Tracks of more than ``correlate_limit`` beats on a side take the
    counting form of the P-score."""
    r = trim_beats(np.asarray(reference_beats, np.float64), min_beat_time)
    e = trim_beats(np.asarray(estimated_beats, np.float64), min_beat_time)
    g, crit, tlen, mean, std, _ = goto_parts(r, e, goto_threshold, goto_mu, goto_sigma)
    try:
        parts = p_score_parts if max(r.size, e.size) <= correlate_limit else p_score_count_parts
        p, win, hits = parts(r, e, p_score_threshold)
    except ValueError:
        p = win = hits = np.nan
    ig, fwd, bwd = information_gain_parts(r, e, bins)
    return np.array([g, p, ig, crit, tlen, mean, std, win, hits, fwd, bwd], np.float64)
