"""``beat_this.model.loss`` of the reference: the training losses, computed by csrc/loss.hip (see beat_this_amd.loss)."""
from ..loss import MaskedBCELoss, ShiftTolerantBCELoss, SplittedShiftTolerantBCELoss

__all__ = ["MaskedBCELoss", "ShiftTolerantBCELoss", "SplittedShiftTolerantBCELoss"]
