"""Beat-tracking metrics of the paper (the reference's Metrics, pl_module.py:320-339): mir_eval.beat's trim_beats,
f_measure, cemgil and continuity, restated in csrc/metrics.hip.  mir_eval is never imported.

Drop-in forms (``trim_beats``, ``f_measure``, ``cemgil``, ``continuity``, ``Metrics``) take mir_eval's arguments, return what
it returns, raise ``ValueError`` where its ``validate`` raises (and, in addition, on non-finite times) and warn on empty input
as it does; they run the library's host code (bt_beat_metrics_host).  ``beat_metrics_many`` scores many tracks in one device
call (bt_beat_metrics)."""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib

COLUMNS = ("F", "P", "R", "Cemgil", "CemgilMax", "CMLc", "CMLt", "AMLc", "AMLt", "n_ref", "n_est", "status")
MAX_TIME = 30000.0
DEFAULTS = dict(f_measure_threshold=0.07, cemgil_sigma=0.04, continuity_phase_threshold=0.175,
                continuity_period_threshold=0.175)
# BT_METRICS_* status bits (include/beat_this_amd.h); those of the estimates are shifted left by 3
STATUS_NONFINITE, STATUS_UNSORTED, STATUS_LATE, STATUS_NEAREST, STATUS_OFFSETS = 1, 2, 4, 64, 128


def _thresholds(kw):
    unknown = set(kw) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown threshold(s) {sorted(unknown)}; known: {sorted(DEFAULTS)}")
    t = {**DEFAULTS, **kw}
    return (t["f_measure_threshold"], t["cemgil_sigma"], t["continuity_phase_threshold"], t["continuity_period_threshold"])


def _events(x, what):
    a = np.asarray(x, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{what} times should be a 1-d array, but shape={a.shape}")
    return np.ascontiguousarray(a)


def validate(reference_beats, estimated_beats):
    """mir_eval.beat.validate: warn on empty input; raise ValueError for events after 30000 s, not 1-d or decreasing (and,
    unlike mir_eval, for non-finite times, which the library's status word also flags)."""
    if np.size(reference_beats) == 0:
        warnings.warn("Reference beats are empty.")
    if np.size(estimated_beats) == 0:
        warnings.warn("Estimated beats are empty.")
    for what, beats in (("reference", reference_beats), ("estimated", estimated_beats)):
        beats = np.asarray(beats, dtype=np.float64)
        if (beats > MAX_TIME).any():
            raise ValueError(f"An event at time {beats.max()} was found which is greater than the maximum allowable time of "
                             f"max_time = {MAX_TIME} (did you supply event times in seconds?)")
        if beats.ndim != 1:
            raise ValueError(f"Event times should be 1-d numpy ndarray, but shape={beats.shape}")
        if not np.isfinite(beats).all():
            raise ValueError(f"{what} event times must be finite")
        if (np.diff(beats) < 0).any():
            raise ValueError("Events should be in increasing order.")


def _host_row(ref, est, thresholds, min_beat_time=-np.inf) -> np.ndarray:
    ref, est = _events(ref, "reference"), _events(est, "estimated")
    out = np.zeros(len(COLUMNS), np.float64)
    roff = np.array([0, ref.size], np.int64)
    eoff = np.array([0, est.size], np.int64)
    _lib.check(_lib.lib().bt_beat_metrics_host(ref.ctypes.data, roff.ctypes.data, est.ctypes.data, eoff.ctypes.data, 1,
                                               float(min_beat_time), *thresholds, out.ctypes.data))
    if out[11]:
        raise ValueError(_status_text(int(out[11])))
    return out


def _status_text(status: int) -> str:
    parts = []
    for shift, side in ((0, "reference"), (3, "estimated")):
        for bit, text in ((STATUS_NONFINITE, "not finite"), (STATUS_UNSORTED, "not in increasing order"),
                          (STATUS_LATE, f"after max_time = {MAX_TIME}")):
            if status & (bit << shift):
                parts.append(f"{side} events {text}")
    if status & STATUS_NEAREST:
        parts.append("nearest annotation not monotone in the estimates (events closer than the rounding of their distances)")
    if status & STATUS_OFFSETS:
        parts.append("bad track offsets")
    return "; ".join(parts) or f"status {status}"


def trim_beats(beats, min_beat_time=5.0):
    """mir_eval.beat.trim_beats: the beats at or after ``min_beat_time``"""
    beats = np.asarray(beats)
    return beats[beats >= min_beat_time]


def f_measure(reference_beats, estimated_beats, f_measure_threshold=0.07):
    """mir_eval.beat.f_measure"""
    validate(reference_beats, estimated_beats)
    return float(_host_row(reference_beats, estimated_beats, _thresholds(dict(f_measure_threshold=f_measure_threshold)))[0])


def cemgil(reference_beats, estimated_beats, cemgil_sigma=0.04):
    """mir_eval.beat.cemgil -> (cemgil, cemgil_max over the five reference variations)"""
    validate(reference_beats, estimated_beats)
    row = _host_row(reference_beats, estimated_beats, _thresholds(dict(cemgil_sigma=cemgil_sigma)))
    return float(row[3]), float(row[4])


def continuity(reference_beats, estimated_beats, continuity_phase_threshold=0.175, continuity_period_threshold=0.175):
    """mir_eval.beat.continuity -> (CMLc, CMLt, AMLc, AMLt)"""
    validate(reference_beats, estimated_beats)
    if np.size(reference_beats) == 1:
        warnings.warn("Only one reference beat was provided, so beat intervals cannot be computed.")
    if np.size(estimated_beats) == 1:
        warnings.warn("Only one estimated beat was provided, so beat intervals cannot be computed.")
    row = _host_row(reference_beats, estimated_beats,
                    _thresholds(dict(continuity_phase_threshold=continuity_phase_threshold,
                                     continuity_period_threshold=continuity_period_threshold)))
    return tuple(float(v) for v in row[5:9])


class Metrics:
    """The reference's Metrics (pl_module.py:320-339): trim both arrays to ``eval_trim_beats`` seconds, then
    ``{"F-measure", "Cemgil"}`` for step "val" and ``{"F-measure", "Cemgil", "CMLt", "AMLt"}`` for step "test"; "Cemgil" is
    the (cemgil, cemgil_max) tuple mir_eval returns.  One host call computes every value."""

    def __init__(self, eval_trim_beats: int) -> None:
        self.min_beat_time = eval_trim_beats

    def __call__(self, truth, preds, step):
        if step not in ("val", "test"):
            raise ValueError("step must be either val or test")
        truth = trim_beats(truth, min_beat_time=self.min_beat_time)
        preds = trim_beats(preds, min_beat_time=self.min_beat_time)
        validate(truth, preds)
        row = _host_row(truth, preds, _thresholds({}))
        out = {"F-measure": float(row[0]), "Cemgil": (float(row[3]), float(row[4]))}
        if step == "test":
            out["CMLt"] = float(row[6])
            out["AMLt"] = float(row[8])
        return out


def _csr(tracks, what):
    arrs = [_events(t, f"{what} {i}") for i, t in enumerate(tracks)]
    off = np.zeros(len(arrs) + 1, np.int64)
    np.cumsum([a.size for a in arrs], out=off[1:])
    flat = np.concatenate(arrs) if arrs and off[-1] else np.zeros(1, np.float64)   # (never an empty allocation)
    return flat, off


def beat_metrics_many(truths, preds, eval_trim_beats=5, device="cuda", raise_on_invalid=True, **thresholds) -> dict:
    """Metrics of many tracks in ONE bt_beat_metrics call: one upload (truths, predictions and offsets in one pinned buffer),
    one launch pair, one device-to-host copy.  ``truths`` / ``preds``: sequences of 1-d beat-time arrays of equal length;
    ``eval_trim_beats``: trim_beats' min_beat_time (None keeps every beat); ``thresholds``: mir_eval's keyword names
    (f_measure_threshold, cemgil_sigma, continuity_phase_threshold, continuity_period_threshold).

    -> dict of (n_tracks,) float64 arrays: "F-measure", "Precision", "Recall", "Cemgil", "CemgilMax", "CMLc", "CMLt", "AMLc",
    "AMLt", "n_ref", "n_est", "status", and "Cemgil_reported" = (Cemgil + CemgilMax) / 2.  The last is what
    compute_paper_metrics.py prints as "Cemgil": Metrics returns mir_eval's (cemgil, cemgil_max) tuple per piece, and the
    np.mean over pieces (pl_module.py:156-160) averages both values of every tuple.
    A track whose status is non-zero (where mir_eval's validate raises) raises ValueError, or, with
    ``raise_on_invalid=False``, keeps NaN metrics and its status bits."""
    if len(truths) != len(preds):
        raise ValueError(f"{len(truths)} truth arrays but {len(preds)} prediction arrays")
    n = len(truths)
    th = _thresholds(thresholds)
    keys = ("F-measure", "Precision", "Recall", "Cemgil", "CemgilMax", "CMLc", "CMLt", "AMLc", "AMLt", "n_ref", "n_est",
            "status")
    if n == 0:
        out = {k: np.zeros(0) for k in keys}
        out["Cemgil_reported"] = np.zeros(0)
        return out
    ref, roff = _csr(truths, "truth")
    est, eoff = _csr(preds, "prediction")
    dev = torch.device(device)
    _lib.require_gpu(torch.empty(0, device=dev), "beat_metrics_many's device")
    # one host block -> one upload: [ref | est | ref offsets | est offsets] as float64 / int64 words
    host = np.concatenate([ref, est, roff.view(np.float64), eoff.view(np.float64)])
    d_in = _lib.upload(host, dev)
    d_ref = d_in.data_ptr()
    d_est = d_ref + 8 * ref.size
    d_roff = d_est + 8 * est.size
    d_eoff = d_roff + 8 * roff.size
    L = _lib.lib()
    ws_bytes = L.bt_beat_metrics_workspace_bytes(n, int(roff[-1]), int(eoff[-1]))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    d_out = torch.empty((n, len(keys)), dtype=torch.float64, device=dev)
    mbt = -np.inf if eval_trim_beats is None else float(eval_trim_beats)
    with torch.cuda.device(dev):
        _lib.check(L.bt_beat_metrics(_lib.stream_ptr(dev), d_ref, d_roff, d_est, d_eoff, n, mbt, *th, ws.data_ptr(), ws_bytes,
                                     d_out.data_ptr()))
    rows = d_out.cpu().numpy()
    out = {k: rows[:, i].copy() for i, k in enumerate(keys)}
    out["Cemgil_reported"] = (out["Cemgil"] + out["CemgilMax"]) / 2
    bad = np.nonzero(out["status"])[0]
    if raise_on_invalid and bad.size:
        raise ValueError(f"track {int(bad[0])}: {_status_text(int(out['status'][bad[0]]))}"
                         + (f" (and {bad.size - 1} more tracks)" if bad.size > 1 else ""))
    return out
