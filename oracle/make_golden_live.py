"""Generate tests/golden/reference_live.npz by running the UNMODIFIED reference on CPU: the outputs that
tests/test_oracle.py's two "live reference" tests used to compute from the reference package at test time, so that they
run on any checkout of this repository (the reference is not needed to run the suite, only to regenerate this fixture).

TEST INFRASTRUCTURE ONLY.  Run where a checkout of the reference is available:

    BEAT_THIS_REFERENCE=<path of the reference checkout> PYTHONDONTWRITEBYTECODE=1 python oracle/make_golden_live.py

Same import arrangement as oracle/make_golden.py (the reference's package, the three third-party stand-ins of oracle/shims
first on sys.path); a file of its own so that the existing fixtures are not regenerated.  Inputs are regenerated from seeds
(beat_this_amd.weights, numpy PCG64): the fixture holds only the reference's OUTPUTS and its state-dict key order.
"""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("BEAT_THIS_REFERENCE")
if not REF:
    raise SystemExit("set BEAT_THIS_REFERENCE to the path of a checkout of the reference")
sys.path[:0] = [os.path.join(ROOT, "oracle", "shims"), REF, ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from beat_this.model.beat_tracker import BeatThis  # noqa: E402
from beat_this.preprocessing import LogMelSpect  # noqa: E402

from beat_this_amd import weights as W  # noqa: E402
from oracle.cases import LIVE_CASES  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MODEL_KEYS = ("spect_dim", "transformer_dim", "ff_mult", "n_layers", "head_dim", "stem_dim")


def reference_model(hp_name, seed, style):
    hp = W.resolve_hparams(hp_name)
    m = BeatThis(**{k: hp[k] for k in MODEL_KEYS}).eval()
    m.load_state_dict(W.random_state_dict(hp, seed=seed, style=style))
    return m


def main():
    torch.manual_seed(0)
    arrs = {}
    with torch.inference_mode():
        # 1. BeatThis.forward on one short chunk, and the module's own state-dict key order (beat_tracker.py:188-192)
        c = LIVE_CASES["forward"]
        m = reference_model(c["hparams"], c["weight_seed"], c["style"])
        arrs["state_dict_keys"] = np.array(list(m.state_dict().keys()))
        r = m(torch.from_numpy(W.synthetic_spect(c["frames"], seed=c["input_seed"]))[None])
        arrs["forward_beat"], arrs["forward_downbeat"] = r["beat"].numpy(), r["downbeat"].numpy()
        # 2. LogMelSpect on a short 22.05 kHz waveform (preprocessing.py)
        c = LIVE_CASES["logmel"]
        arrs["logmel"] = LogMelSpect()(torch.from_numpy(W.synthetic_audio(c["seconds"], seed=c["audio_seed"]))).numpy()
        # 3. BeatThis.forward on one full chunk: what tools/port_speed.py times the CPU oracle against
        c = LIVE_CASES["port_chunk"]
        m = reference_model(c["hparams"], c["weight_seed"], c["style"])
        r = m(torch.from_numpy(W.synthetic_spect(c["frames"], seed=c["input_seed"]))[None])
        arrs["port_chunk_beat"], arrs["port_chunk_downbeat"] = r["beat"].numpy(), r["downbeat"].numpy()
    for k, v in arrs.items():
        print(k, v.shape, v.dtype)
    np.savez_compressed(os.path.join(OUT, "reference_live.npz"), **arrs)


if __name__ == "__main__":
    main()
