"""The reference's ``beat_this.dataset.mmnpz.MemmappedNpzFile`` is this package's ``SpectBundle`` (bundle.py): a read-only
mapping over the stored ``.npy`` members of an uncompressed ``.npz`` archive, mapped without a copy."""
from ..bundle import SpectBundle

MemmappedNpzFile = SpectBundle

__all__ = ["MemmappedNpzFile"]
