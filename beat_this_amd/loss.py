"""The reference's training losses (beat_this/model/loss.py) on the GPU, with their gradients: ``MaskedBCELoss``,
``ShiftTolerantBCELoss`` and ``SplittedShiftTolerantBCELoss`` take what the reference's modules take, reject what they
reject and return the dtype they return; the value and the gradient with respect to ``preds`` come from csrc/loss.hip (fp32
terms, fp64 sums, no host synchronisation, no atomics).  ``losses_from_hparams`` picks the pair a
checkpoint was trained with (pl_module.py:63-91); ``piece_losses`` scores many pieces in one device call; ``loss_host`` runs
the library's host twin on numpy arrays.  Only ``preds`` is differentiable; there is no CPU path for tensors."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MASKED, SHIFT_TOLERANT, SPLITTED = 0, 1, 2               # BT_LOSS_* kinds
F32, F16, BF16, U8 = 0, 1, 2, 3                           # BT_LOSS_* element types
MAX_TOLERANCE = 32                                        # BT_LOSS_MAX_TOLERANCE
_DT = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
_NP_DT = {np.dtype(np.float32): F32, np.dtype(np.float16): F16, np.dtype(np.uint8): U8, np.dtype(np.bool_): U8}


def _autocast_on(device) -> bool:
    try:
        return torch.is_autocast_enabled(device.type)
    except TypeError:   # (older torch: no device argument)
        return torch.is_autocast_enabled()


def _check_settings(kind, tolerance):
    if kind not in (MASKED, SHIFT_TOLERANT, SPLITTED):
        raise ValueError(f"unknown loss kind {kind}")
    if not isinstance(tolerance, (int, np.integer)) or not 0 <= tolerance <= MAX_TOLERANCE:
        raise ValueError(f"tolerance must be an integer in [0, {MAX_TOLERANCE}], got {tolerance!r}")


def _layout(kind, tolerance, preds, targets, mask):
    """-> (logits, targets, mask or None) as contiguous tensors of kernel element types, n_rows, T.  Raises where the reference
    raises: 1-D / 4-D input with a tolerance (max_pool1d), rows shorter than 1 + 4 tolerance, targets of another shape."""
    if targets.requires_grad or (mask is not None and mask.requires_grad):
        raise RuntimeError("beat_this_amd's losses are differentiable with respect to preds only: targets and mask must not "
                           "require grad")
    _lib.require_gpu(preds, "preds")
    _lib.require_gpu(targets, "targets")
    if mask is not None:
        _lib.require_gpu(mask, "mask")
    pooled = kind != MASKED and tolerance > 0
    if pooled and preds.dim() not in (2, 3):
        raise RuntimeError(f"max_pool1d() Expected 2D or 3D input tensor, but got {tuple(preds.shape)}")
    if targets.shape != preds.shape:
        raise ValueError(f"Target size ({tuple(targets.shape)}) must be the same as input size ({tuple(preds.shape)})")
    T = preds.shape[-1] if preds.dim() else 1
    if pooled and T < 1 + 4 * tolerance:
        raise RuntimeError(f"the loss pools targets over 1 + 4 * tolerance = {1 + 4 * tolerance} frames, but the input has "
                           f"{T} frames")
    x = preds if preds.dtype in _DT else preds.float()
    y = targets if targets.dtype in (torch.float32, torch.float16) else targets.float()
    m = None
    if mask is not None:
        m = mask.expand(preds.shape) if mask.shape != preds.shape else mask
        if m.dtype == torch.bool:
            m = m.contiguous().view(torch.uint8)
        elif m.dtype not in (torch.float32, torch.uint8):
            m = m.float()
        m = m.contiguous()
    n_rows = max(1, preds.numel() // T) if T else 1
    return x.contiguous(), y.contiguous(), m, n_rows, T


def _pos_weight_args(pos_weight, device):
    """-> (host value, device pointer or 0, tensor to keep alive): a pos_weight already on the GPU is read by the kernel from
    device memory (no synchronisation), one on the host is passed by value"""
    if isinstance(pos_weight, torch.Tensor):
        if pos_weight.numel() != 1:
            raise ValueError("pos_weight must be a scalar")
        if pos_weight.is_cuda:
            pw = pos_weight.to(device=device, dtype=torch.float32).reshape(())
            return 1.0, pw.data_ptr(), pw
        return float(pos_weight), 0, None
    return float(pos_weight), 0, None


class _BCELoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, targets, mask, kind, tolerance, pos_weight, out_dtype):
        x, y, m, n_rows, T = _layout(kind, tolerance, preds, targets, mask)
        dev = preds.device
        L = _lib.lib()
        pw_args = _pos_weight_args(pos_weight, dev)
        ws_bytes = L.bt_bce_loss_workspace_bytes(n_rows, T)
        if ws_bytes == 0:
            raise ValueError(f"loss input of {n_rows} rows of {T} frames is out of range")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        offsets = torch.arange(0, (n_rows + 1) * T, T, dtype=torch.int64, device=dev) if T else \
            torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
        loss = torch.empty((), dtype=out_dtype, device=dev)
        need_grad = ctx.needs_input_grad[0]
        grad = torch.empty(preds.shape, dtype=torch.float32, device=dev) if need_grad else None
        _lib.check(L.bt_bce_loss(_lib.stream_ptr(dev), kind, tolerance, pw_args[0], pw_args[1], x.data_ptr(), _DT[x.dtype],
                                 y.data_ptr(), _DT[y.dtype], _lib.ptr(m), U8 if m is not None and m.dtype == torch.uint8 else F32,
                                 offsets.data_ptr(), n_rows, T, T, ws.data_ptr(), ws_bytes, None, None, loss.data_ptr(),
                                 _DT[out_dtype], _lib.ptr(grad), None))
        if need_grad:
            ctx.save_for_backward(grad)
            h = 0 if kind == MASKED else 2 * tolerance
            ctx.count = n_rows * (T - 2 * h)
            ctx.preds_dtype = preds.dtype
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        kdt = ctx.preds_dtype if ctx.preds_dtype in _DT else torch.float32
        go = grad_output.contiguous() if grad_output.dtype in _DT else grad_output.float().contiguous()
        out = torch.empty(grad.shape, dtype=kdt, device=grad.device)
        _lib.check(_lib.lib().bt_bce_loss_backward(_lib.stream_ptr(grad.device), grad.data_ptr(), grad.numel(), go.data_ptr(),
                                                   _DT[go.dtype], ctx.count, out.data_ptr(), _DT[kdt]))
        if kdt != ctx.preds_dtype:
            out = out.to(ctx.preds_dtype)
        return out, None, None, None, None, None, None


def bce_loss(preds, targets, mask=None, kind=SHIFT_TOLERANT, tolerance=3, pos_weight=1.0):
    """The functional form of the three modules: a 0-d tensor of preds' dtype (fp32 under autocast), differentiable in preds"""
    _check_settings(kind, tolerance)
    if not isinstance(preds, torch.Tensor) or not isinstance(targets, torch.Tensor):
        raise TypeError("preds and targets must be tensors")
    out_dtype = torch.float32 if _autocast_on(preds.device) else preds.dtype
    if out_dtype not in _DT:
        return _BCELoss.apply(preds, targets, mask, kind, tolerance, pos_weight, torch.float32).to(out_dtype)
    return _BCELoss.apply(preds, targets, mask, kind, tolerance, pos_weight, out_dtype)


class MaskedBCELoss(torch.nn.Module):
    """Plain binary cross-entropy on logits with an optional mask (zeros ignore an entry), the mean over all elements
    (loss.py:9-35).  pos_weight: weight of positive examples."""

    def __init__(self, pos_weight: float = 1):
        super().__init__()
        self.register_buffer("pos_weight", torch.tensor(pos_weight, dtype=torch.get_default_dtype()), persistent=False)

    def forward(self, preds: torch.Tensor, targets: torch.Tensor, mask: torch.Tensor | None = None):
        return bce_loss(preds, targets, mask, MASKED, 0, self.pos_weight)


class ShiftTolerantBCELoss(torch.nn.Module):
    """BCE that tolerates shifts of up to ``tolerance`` frames between predictions and targets (loss.py:38-99): the
    predictions are max-pooled over 1 + 2 tolerance frames, the frames near a positive target are ignored, the edges
    (2 tolerance frames each side) are cropped.  Input (B, T) or (N, C, T)."""

    def __init__(self, pos_weight: float = 1, tolerance: int = 3):
        super().__init__()
        self.register_buffer("pos_weight", torch.tensor(pos_weight, dtype=torch.get_default_dtype()), persistent=False)
        self.tolerance = tolerance

    def forward(self, preds: torch.Tensor, targets: torch.Tensor, mask: torch.Tensor | None = None):
        return bce_loss(preds, targets, mask, SHIFT_TOLERANT, self.tolerance, self.pos_weight)


class SplittedShiftTolerantBCELoss(torch.nn.Module):
    """The split form of ShiftTolerantBCELoss (loss.py:102-171): a positive part on the targets and a negative part on the
    targets max-pooled over 1 + 4 tolerance frames.  Equal to ShiftTolerantBCELoss for binary targets; for soft targets it
    follows the paper's equation.  The mask is required."""

    def __init__(self, pos_weight: float = 1, tolerance: int = 3):
        super().__init__()
        self.tolerance = 3   # (as the reference: the attribute is not what the loss uses)
        self.spread_preds = tolerance
        self.spread_targets = 2 * tolerance
        self.register_buffer("pos_weight", torch.tensor(pos_weight, dtype=torch.get_default_dtype()), persistent=False)

    def forward(self, preds: torch.Tensor, targets: torch.Tensor, mask: torch.Tensor):
        return bce_loss(preds, targets, mask, SPLITTED, self.spread_preds, self.pos_weight)


LOSS_TYPES = ("shift_tolerant_weighted_bce", "weighted_bce", "bce", "splitted_shift_tolerant_weighted_bce")


def losses_from_hparams(hyper_parameters: dict):
    """(beat_loss, downbeat_loss) as PLBeatThis builds them from its hyper-parameters (pl_module.py:63-91), with its defaults
    for absent keys (loss_type "shift_tolerant_weighted_bce", pos_weights {"beat": 1, "downbeat": 1})."""
    hp = hyper_parameters or {}
    loss_type = hp.get("loss_type", "shift_tolerant_weighted_bce")
    pos_weights = hp.get("pos_weights", {"beat": 1, "downbeat": 1})
    if loss_type == "shift_tolerant_weighted_bce":
        return ShiftTolerantBCELoss(pos_weight=pos_weights["beat"]), ShiftTolerantBCELoss(pos_weight=pos_weights["downbeat"])
    if loss_type == "weighted_bce":
        return MaskedBCELoss(pos_weight=pos_weights["beat"]), MaskedBCELoss(pos_weight=pos_weights["downbeat"])
    if loss_type == "bce":
        return MaskedBCELoss(), MaskedBCELoss()
    if loss_type == "splitted_shift_tolerant_weighted_bce":
        return (SplittedShiftTolerantBCELoss(pos_weight=pos_weights["beat"]),
                SplittedShiftTolerantBCELoss(pos_weight=pos_weights["downbeat"]))
    raise ValueError("loss_type must be one of 'shift_tolerant_weighted_bce', 'weighted_bce', 'bce'")


def _kind_of(module):
    if isinstance(module, SplittedShiftTolerantBCELoss):
        return SPLITTED, module.spread_preds
    if isinstance(module, ShiftTolerantBCELoss):
        return SHIFT_TOLERANT, module.tolerance
    if isinstance(module, MaskedBCELoss):
        return MASKED, 0
    raise TypeError(f"not one of this module's losses: {type(module).__name__}")


def piece_losses(loss, logits, targets, masks=None, names=None):
    """Per-piece losses of many pieces in one device call: ``loss`` one of the three modules; ``logits`` a list of 1-D device
    tensors (one piece each, any length), ``targets`` a list of as many 1-D arrays or tensors, ``masks`` None or a list of
    the same (None entries: all ones).  Each piece is scored alone, as the reference scores a test batch of one full piece.
    -> float64 numpy array: row sum / output frames per piece.  A piece shorter than 1 + 4 tolerance raises ValueError naming
    it (``names[i]`` or its index)."""
    kind, tol = _kind_of(loss)
    _check_settings(kind, tol)
    if len(targets) != len(logits) or (masks is not None and len(masks) != len(logits)):
        raise ValueError("logits, targets and masks must have one entry per piece")
    n = len(logits)
    if n == 0:
        return np.zeros(0, np.float64)
    dev = logits[0].device
    _lib.require_gpu(logits[0], "logits")
    lens = np.array([int(x.numel()) for x in logits], np.int64)
    need = 1 + 4 * tol if kind != MASKED else 0
    for i, (x, T) in enumerate(zip(logits, lens)):
        if x.dim() != 1:
            raise ValueError(f"piece {names[i] if names else i}: expected 1-D logits, got {tuple(x.shape)}")
        if T < need:
            raise ValueError(f"piece {names[i] if names else i} has {T} frames, the loss needs at least {need} "
                             f"(1 + 4 * tolerance)")
        if np.size(targets[i]) != T or (masks is not None and masks[i] is not None and np.size(masks[i]) != T):
            raise ValueError(f"piece {names[i] if names else i}: targets / mask do not have the logits' {T} frames")
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(lens)
    x = torch.cat([t.to(torch.float32) for t in logits])

    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    y = np.concatenate([host(t).astype(np.float32, copy=False).reshape(-1) for t in targets])
    m = None
    if masks is not None:
        m = np.concatenate([np.ones(T, np.float32) if mk is None else host(mk).astype(np.float32, copy=False).reshape(-1)
                            for mk, T in zip(masks, lens)])
    L = _lib.lib()
    ws_bytes = L.bt_bce_loss_workspace_bytes(n, int(lens.max()))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    d_y, d_off = _lib.upload(y, dev), _lib.upload(off, dev)
    d_m = None if m is None else _lib.upload(m, dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    cnt = torch.empty(n, dtype=torch.int64, device=dev)
    pw = float(loss.pos_weight)
    _lib.check(L.bt_bce_loss(_lib.stream_ptr(dev), kind, tol, pw, None, x.data_ptr(), F32, d_y.data_ptr(), F32, _lib.ptr(d_m),
                             F32, d_off.data_ptr(), n, int(lens.min()), int(lens.max()), ws.data_ptr(), ws_bytes,
                             out.data_ptr(), cnt.data_ptr(), None, F32, None, None))
    sums, counts = out.cpu().numpy(), cnt.cpu().numpy()
    return sums / counts


def loss_host(kind, tolerance, pos_weight, logits, targets, mask=None, offsets=None):
    """The library's host twin (bt_bce_loss_host) on numpy arrays: logits float32 / float16 (or uint16: bfloat16 bits),
    targets float32 / float16, mask None / float32 / bool / uint8, all of one length, split into rows by
    ``offsets`` (default: one row).  -> dict: row_sum, row_count, loss (the mean), grad (d row sum / d logit, float32), terms."""
    _check_settings(kind, tolerance)
    x = np.ascontiguousarray(logits)
    ldt = BF16 if x.dtype == np.uint16 else _NP_DT.get(x.dtype)
    y = np.ascontiguousarray(targets)
    m = None if mask is None else np.ascontiguousarray(mask)
    if ldt not in (F32, F16, BF16) or _NP_DT.get(y.dtype) not in (F32, F16) or (m is not None and _NP_DT.get(m.dtype) not in (F32, U8)):
        raise TypeError("loss_host: logits float32 / float16 / uint16 (bfloat16 bits), targets float32 / float16, mask float32 / "
                        "bool / uint8")
    n = x.size
    if y.size != n or (m is not None and m.size != n):
        raise ValueError("logits, targets and mask must have the same number of elements")
    off = np.array([0, n], np.int64) if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    rows = off.size - 1
    row_sum = np.zeros(rows, np.float64)
    row_count = np.zeros(rows, np.int64)
    total = C.c_double()
    grad = np.zeros(n, np.float32)
    terms = np.zeros(n, np.float32)
    _lib.check(_lib.lib().bt_bce_loss_host(kind, tolerance, float(pos_weight), x.ctypes.data, ldt, y.ctypes.data,
                                           _NP_DT[y.dtype], None if m is None else m.ctypes.data,
                                           F32 if m is None else _NP_DT[m.dtype], off.ctypes.data, rows, row_sum.ctypes.data,
                                           row_count.ctypes.data, C.byref(total), grad.ctypes.data, terms.ctypes.data))
    return dict(row_sum=row_sum, row_count=row_count, loss=total.value, grad=grad, terms=terms)
