"""Training data on the GPU, mirroring the reference's ``beat_this.dataset`` package: ``BeatTrackingDataset`` and
``BeatDataModule`` (dataset.py), the augmentation helpers (augment.py), the batch planner (plan.py) and the memory-mapped
``.npz`` reader under the reference's name (mmnpz.py).  DESIGN.md section 12."""
from .dataset import BatchLoader, BeatDataModule, BeatTrackingDataset  # noqa: F401
from .mmnpz import MemmappedNpzFile  # noqa: F401
