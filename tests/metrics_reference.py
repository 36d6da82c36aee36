"""Plain numpy restatement of the mir_eval.beat functions behind the reference's Metrics (pl_module.py:320-339): trim_beats,
f_measure, cemgil, continuity, with mir_eval 0.7 / 0.8's default arguments.  mir_eval is not installed here; this follows its
published algorithm with its code structure (sequential loops, np.interp, np.argmin) so that csrc/metrics.hip, which does not
follow that structure, is checked against an independent statement.  It is not pinned against mir_eval itself.

The F-measure's matching is built from _fast_hit_windows' searchsorted windows plus a maximum bipartite matching by augmenting
paths -- not greedy -- so that it checks the library's claim that greedy ascending matching is maximum."""
import numpy as np

MAX_TIME = 30000.0


def trim_beats(beats, min_beat_time=5.0):
    return beats[beats >= min_beat_time]


def validate(reference_beats, estimated_beats):
    for beats in (reference_beats, estimated_beats):
        if (beats > MAX_TIME).any():
            raise ValueError("event after max_time")
        if beats.ndim != 1:
            raise ValueError("events must be 1-d")
        if (np.diff(beats) < 0).any():
            raise ValueError("events must be increasing")


def _fast_hit_windows(ref, est, window):
    ref_idx = np.argsort(ref, kind="stable")
    ref_sorted = ref[ref_idx]
    left_idx = np.searchsorted(ref_sorted, est - window, side="left")
    right_idx = np.searchsorted(ref_sorted, est + window, side="right")
    hit_ref, hit_est = [], []
    for j, (start, end) in enumerate(zip(left_idx, right_idx)):
        hit_ref.extend(ref_idx[start:end])
        hit_est.extend([j] * (end - start))
    return hit_ref, hit_est


def _bipartite_match(graph):
    """graph: est -> list of refs.  A maximum matching by augmenting paths (Kuhn's algorithm, iterative depth-first search
    from every estimate in turn) -> {est: ref}."""
    match_ref, match_est = {}, {}
    for root in graph:
        seen, parent = set(), {}
        stack = [(root, iter(graph[root]))]
        free = None
        while stack and free is None:
            u, refs = stack[-1]
            for r in refs:
                if r in seen:
                    continue
                seen.add(r)
                parent[r] = u
                if r not in match_ref:
                    free = r
                else:
                    stack.append((match_ref[r], iter(graph[match_ref[r]])))
                break
            else:
                stack.pop()
        r = free
        while r is not None:   # flip the augmenting path back to the root
            u = parent[r]
            nxt = match_est.get(u)
            match_ref[r], match_est[u] = u, r
            r = nxt
    return match_est


def match_events(ref, est, window):
    hits = _fast_hit_windows(ref, est, window)
    graph = {}
    for ref_i, est_i in zip(*hits):
        graph.setdefault(est_i, []).append(ref_i)
    return sorted(_bipartite_match(graph).items())


def f_measure_prf(reference_beats, estimated_beats, f_measure_threshold=0.07):
    """-> (F, precision, recall)"""
    validate(reference_beats, estimated_beats)
    if estimated_beats.size == 0 or reference_beats.size == 0:
        return 0.0, 0.0, 0.0
    matching = match_events(reference_beats, estimated_beats, f_measure_threshold)
    precision = float(len(matching)) / len(estimated_beats)
    recall = float(len(matching)) / len(reference_beats)
    if precision == 0 and recall == 0:
        return 0.0, precision, recall
    beta = 1.0
    return (1 + beta ** 2) * precision * recall / ((beta ** 2) * precision + recall), precision, recall


def f_measure(reference_beats, estimated_beats, f_measure_threshold=0.07):
    return f_measure_prf(reference_beats, estimated_beats, f_measure_threshold)[0]


def _get_reference_beat_variations(reference_beats):
    interpolated_indices = np.arange(0, reference_beats.shape[0] - 0.5, 0.5)
    original_indices = np.arange(0, reference_beats.shape[0])
    double_reference_beats = np.interp(interpolated_indices, original_indices, reference_beats)
    return (reference_beats, double_reference_beats[1::2], double_reference_beats, reference_beats[::2],
            reference_beats[1::2])


def cemgil(reference_beats, estimated_beats, cemgil_sigma=0.04):
    validate(reference_beats, estimated_beats)
    if estimated_beats.size == 0 or reference_beats.size == 0:
        return 0.0, 0.0
    accuracies = []
    for reference_beats in _get_reference_beat_variations(reference_beats):
        accuracy = 0
        for beat in reference_beats:
            beat_diff = np.min(np.abs(beat - estimated_beats))
            accuracy += np.exp(-(beat_diff ** 2) / (2.0 * cemgil_sigma ** 2))
        accuracy /= 0.5 * (estimated_beats.shape[0] + reference_beats.shape[0])
        accuracies.append(accuracy)
    return accuracies[0], np.max(accuracies)


def continuity(reference_beats, estimated_beats, continuity_phase_threshold=0.175, continuity_period_threshold=0.175):
    validate(reference_beats, estimated_beats)
    if estimated_beats.size <= 1 or reference_beats.size <= 1:
        return 0.0, 0.0, 0.0, 0.0
    continuous_accuracies, total_accuracies = [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for reference_beats in _get_reference_beat_variations(reference_beats):
            n_annotations = np.max([reference_beats.shape[0], estimated_beats.shape[0]])
            used_annotations = np.zeros(n_annotations)
            beat_successes = np.zeros(n_annotations)
            for m in range(estimated_beats.shape[0]):
                beat_success = 0
                beat_differences = np.abs(estimated_beats[m] - reference_beats)
                nearest = np.argmin(beat_differences)
                min_difference = beat_differences[nearest]
                if used_annotations[nearest] == 0:
                    if m == 0 or nearest == 0:
                        if nearest + 1 < reference_beats.shape[0]:
                            reference_interval = reference_beats[nearest + 1] - reference_beats[nearest]
                        else:
                            reference_interval = reference_beats[nearest] - reference_beats[nearest - 1]
                        if reference_interval == 0:
                            phase_condition = 0
                        else:
                            phase = np.abs(min_difference / reference_interval)
                            phase_condition = phase < continuity_phase_threshold
                        if m + 1 < estimated_beats.shape[0]:
                            estimated_interval = estimated_beats[m + 1] - estimated_beats[m]
                        else:
                            estimated_interval = estimated_beats[m] - estimated_beats[m - 1]
                        if reference_interval == 0:
                            period_condition = 0
                        else:
                            period = np.abs(1 - estimated_interval / reference_interval)
                            period_condition = period < continuity_period_threshold
                        if phase_condition and period_condition:
                            used_annotations[nearest] = 1
                            beat_success = 1
                    else:
                        reference_interval = reference_beats[nearest] - reference_beats[nearest - 1]
                        phase = np.abs(min_difference / reference_interval)
                        phase_condition = phase < continuity_phase_threshold
                        estimated_interval = estimated_beats[m] - estimated_beats[m - 1]
                        period = np.abs(1 - estimated_interval / reference_interval)
                        period_condition = period < continuity_period_threshold
                        if phase_condition and period_condition:
                            used_annotations[nearest] = 1
                            beat_success = 1
                beat_successes[m] = beat_success
            beat_successes = np.append(np.append(0, beat_successes), 0)
            beat_failures = np.nonzero(beat_successes == 0)[0]
            beat_successes = beat_successes[1:-1]
            longest_track = np.max(np.diff(beat_failures)) - 1
            continuous_accuracies.append(longest_track / (1.0 * beat_successes.shape[0]))
            total_accuracies.append(np.sum(beat_successes) / (1.0 * beat_successes.shape[0]))
    return continuous_accuracies[0], total_accuracies[0], np.max(continuous_accuracies), np.max(total_accuracies)


def row(reference_beats, estimated_beats, min_beat_time=-np.inf):
    """the 11 leading columns of a bt_beat_metrics row (status 0 assumed): F, P, R, Cemgil, CemgilMax, CMLc, CMLt, AMLc, AMLt,
    n_ref_trimmed, n_est_trimmed"""
    r = trim_beats(np.asarray(reference_beats, np.float64), min_beat_time)
    e = trim_beats(np.asarray(estimated_beats, np.float64), min_beat_time)
    F, P, R = f_measure_prf(r, e)
    return np.array([F, P, R, *cemgil(r, e), *continuity(r, e), len(r), len(e)], np.float64)


def fuzz_tracks(seed=0, n_tracks=2000, long_tracks=1):
    """A seeded list of (reference, estimates) pairs, sorted float64 arrays: random tempi with jitter, dropouts and
    insertions; duplicate times (zero intervals); one beat on either side; empty sides; estimates denser than the 70 ms
    window; hits exactly on the window edge; metrical-level errors (off-beat, double, half tempo); and ``long_tracks`` tracks of
    20 000 beats."""
    rng = np.random.default_rng(seed)
    out = []

    def tempo_track(dur, period, jitter, t0=0.0):
        t = np.arange(t0 + rng.uniform(0, period), dur, period)
        return t + rng.normal(0, jitter, t.size) if jitter else t

    for i in range(n_tracks):
        kind = i % 10
        dur = rng.uniform(6, 60)
        period = rng.uniform(0.3, 1.0)
        ref = tempo_track(dur, period, rng.uniform(0, 0.02))
        if kind == 0:      # jitter, dropouts, insertions
            est = ref + rng.normal(0, rng.uniform(0.005, 0.08), ref.size)
            est = est[rng.random(est.size) > rng.uniform(0, 0.3)]
            est = np.concatenate([est, rng.uniform(0, dur, rng.integers(0, 8))])
        elif kind == 1:    # metrical levels: off-beat, double, half tempo, with jitter
            mid = (ref[1:] + ref[:-1]) / 2
            est = [mid, np.sort(np.concatenate([ref, mid])), ref[::2], ref[1::2], ref * 1.0][rng.integers(0, 5)]
            est = est + rng.normal(0, 0.01, est.size)
        elif kind == 2:    # duplicate times on either side
            est = ref + rng.normal(0, 0.02, ref.size)
            if ref.size:
                ref = np.concatenate([ref, ref[rng.integers(0, ref.size, rng.integers(1, 5))]])
            if est.size:
                est = np.concatenate([est, est[rng.integers(0, est.size, rng.integers(1, 5))]])
        elif kind == 3:    # one or two beats on a side, or none
            k = int(rng.integers(0, 3))
            if rng.random() < 0.5:
                ref = ref[rng.integers(0, ref.size, k)] if ref.size else ref
                est = tempo_track(dur, period, 0.01)
            else:
                est = ref[rng.integers(0, ref.size, k)] + rng.normal(0, 0.03, k) if ref.size else ref
        elif kind == 4:    # estimates denser than the window
            est = np.arange(rng.uniform(0, 0.05), dur, rng.uniform(0.01, 0.069))
        elif kind == 5:    # hits exactly on the window edge (and one rounding step beyond it)
            ref = np.arange(int(dur / 0.5)) * 0.5 + rng.integers(0, 4) * 0.125
            step = rng.choice([0.07, -0.07, np.nextafter(0.07, 1), np.nextafter(-0.07, -1), 0.0625, 0.078125])
            est = ref + step
            est = est[rng.random(est.size) > 0.2]
        elif kind == 6:    # tempo mismatch and drift
            est = tempo_track(dur, period * rng.choice([0.5, 2 / 3, 1.0, 1.5, 2.0]) * rng.uniform(0.95, 1.05), 0.01)
        elif kind == 7:    # quantised times (many equal distances: argmin ties)
            ref = np.round(ref * 20) / 20
            est = np.round((ref + rng.normal(0, 0.03, ref.size)) * 20) / 20
        elif kind == 8:    # phase and period at the continuity thresholds
            est = ref + period * rng.choice([0.17, 0.175, 0.18]) * rng.choice([-1, 1])
            est = est * rng.choice([1.0, 1.17, 1.175, 0.825])
        else:              # tiny tracks
            ref = tempo_track(rng.uniform(0.5, 4), period, 0.02)
            est = tempo_track(rng.uniform(0.5, 4), period * rng.uniform(0.8, 1.2), 0.02)
        out.append((np.sort(np.clip(ref, 0, None)), np.sort(np.clip(est, 0, None))))
    for i in range(long_tracks):   # 20 000 beats: a 40 000-entry double-tempo variation
        ref = np.arange(20000) * 0.5 + rng.normal(0, 0.01, 20000) + 1.0
        est = ref + rng.normal(0, 0.03, 20000)
        est = est[rng.random(est.size) > 0.02]
        out.append((np.sort(ref), np.sort(est)))
    return [(np.asarray(r, np.float64), np.asarray(e, np.float64)) for r, e in out]
