"""bench.py's bookkeeping on CPU: the algorithmic FLOP table must reproduce SURVEY.md 8d / Appendix B, the track arithmetic
must match split_piece, and the command line must expose the driver contract."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flop_table_matches_survey():
    b = _bench()
    fl = b.flops_per_chunk(512)
    total = sum(v for k, v in fl.items() if k != "layer_tail")
    assert abs(total - 134.71e9) < 0.01e9          # 67.355 GMAC = 134.71 GFLOP per final0 chunk
    assert fl["layer_tail"] == fl["out_gemm"] + fl["ff1_gemm"] + fl["ff2_gemm"]
    small = b.flops_per_chunk(128)
    assert abs(sum(v for k, v in small.items() if k != "layer_tail") - 59.57e9) < 0.01e9
    # per layer: qkv 1.1796 + gates 0.0123 + QK^T+PV 2.3040 + out 0.3932 + ff 3.1457 GMAC
    assert abs(fl["attn_flash"] - 2 * (6 * 2.3040e9 + 3 * 4.608e9)) < 1e7


def test_track_arithmetic_matches_split_piece():
    from beat_this_amd.inference import chunk_starts
    from beat_this_amd.parallel import track_frames

    assert track_frames(int(300.0 * 44100), 44100) == 15001
    assert len(chunk_starts(15001, 1500, 6)) == 11  # a 5-minute track is 11 chunks
    assert track_frames(int(300.0 * 22050), 22050) == 15001


def test_command_line_contract():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True).stdout
    for flag in ("--gpus", "--steps", "--warmup", "--prec", "--workload", "--tracks", "--dump-outputs", "--full"):
        assert flag in out


def test_dump_outputs_writes_what_the_caller_receives(tmp_path):
    import numpy as np
    import torch

    b = _bench()
    tracks = [(np.array([0.5, 1.0, 1.5]), np.array([0.5])), (np.array([0.25]), np.array([], dtype=np.float64))]
    b.dump_outputs(str(tmp_path / "tr"), tracks, "tracks")
    assert sorted(os.listdir(tmp_path / "tr")) == ["track000_beats.npy", "track000_downbeats.npy", "track001_beats.npy",
                                                   "track001_downbeats.npy"]
    got = np.load(tmp_path / "tr" / "track000_beats.npy")
    assert got.dtype == np.float64 and np.array_equal(got, tracks[0][0])
    r = {"beat": torch.randn(4, 1500, dtype=torch.float16), "downbeat": torch.randn(4, 1500)}
    b.dump_outputs(str(tmp_path / "fw"), r, "forward")
    beat = np.load(tmp_path / "fw" / "beat.npy")
    assert beat.dtype == np.float32 and beat.shape == (4, 1500) and np.array_equal(beat, r["beat"].float().numpy())
    # larger than the cap: a fixed, seeded sample of the rows, the same on every call
    b.DUMP_MAX_BYTES = 4 * 1500 * 4 * 2 // 2
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), r, "forward")
    rows = np.load(tmp_path / "s1" / "sampled_rows.npy")
    assert len(rows) == 2 and np.array_equal(rows, np.load(tmp_path / "s2" / "sampled_rows.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "downbeat.npy"), r["downbeat"].numpy()[rows.astype(int)])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_run_measures_the_headline_only(tmp_path):
    """without --full the line carries the headline and its timed region, every side leg is null, and --dump-outputs still
    writes the last timed step's outputs"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--tracks", "2",
                        "--min-seconds", "0", "--watchdog", "240", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["full"] is False and d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 3
    assert d["timed_region"]["steps_timed"] == 3
    for k in ("parity", "roofline", "breakdown", "cpu_baseline", "half_path", "fp32_exact_path", "latency", "stress_weights",
              "frontend", "forward_only", "host_inclusive", "configs", "strong_scaling_cfg4"):
        assert d[k] is None, k
    assert not [k for k in d if k.startswith("value_p16")]
    for leg in ("roofline leg", "cpu baseline", "strong-scaling leg"):
        assert leg not in r.stderr
    assert sorted(os.listdir(tmp_path / "out")) == [f"track{i:03d}_{k}.npy" for i in range(2) for k in ("beats", "downbeats")]
