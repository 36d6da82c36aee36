"""The optimiser side of fine-tuning: ``AdamW`` (torch.optim.AdamW's default semantics on csrc/optim.hip: one launch for all
tensors, the global gradient norm and its clip coefficient in two more, nothing read back), ``CosineWarmupScheduler`` (the
reference's schedule, pl_module.py:342-369) and ``param_groups_for`` (its grouping, pl_module.py:283-296).  DESIGN.md section 14.
``adamw_step_host`` / ``adamw_ema_step_host`` / ``grad_norm_host`` / ``plan`` expose the library's host twins and its planner on
numpy arrays.  ``AdamW(ema_decay=...)`` keeps an exponential moving average of the weights in the pass of the step (DESIGN.md
section 22).
``LossScaler`` is the dynamic loss scale of 16-mixed training with ``torch.amp.GradScaler``'s rule,
``scale_update`` that rule as a pure function.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import _lib

CHUNK, NORM_SLICE, MAX_GROUPS = _lib.OPTIM_CHUNK, _lib.OPTIM_NORM_SLICE, _lib.OPTIM_MAX_GROUPS


# ---- the C ABI on host data -----------------------------------------------------------------------------------------------
def plan(pointers, numels, groups, n_groups):
    """bt_optim_plan -> (tensor table, chunk table, total elements of a flat buffer): ctypes arrays of ``_lib.OptimTensor`` /
    ``_lib.OptimChunk``.  Tensor i starts at a multiple of 4 elements; one chunk table entry per BT_OPTIM_CHUNK elements."""
    L = _lib.lib()
    n = len(numels)
    ptrs = (C.c_void_p * max(n, 1))(*[int(p) if p else None for p in pointers])
    nel = (C.c_int64 * max(n, 1))(*[int(x) for x in numels])
    grp = (C.c_int32 * max(n, 1))(*[int(g) for g in groups])
    tensors = (_lib.OptimTensor * max(n, 1))()
    total, n_chunks = C.c_int64(), C.c_int64()
    _lib.check(L.bt_optim_plan(n, ptrs, nel, grp, n_groups, tensors, C.byref(total), None, 0, C.byref(n_chunks)))
    chunks = (_lib.OptimChunk * max(n_chunks.value, 1))()
    _lib.check(L.bt_optim_plan(n, ptrs, nel, grp, n_groups, tensors, C.byref(total), chunks, n_chunks.value, C.byref(n_chunks)))
    return tensors, chunks, int(total.value), int(n_chunks.value)


def hyper(groups, step, grad_scale=1.0, zero_grads=True) -> _lib.OptimHyper:
    """The by-value scalars of step number ``step`` (1 for the first): per group 1 - lr wd, 1 - beta1, beta2, 1 - beta2,
    lr / (1 - beta1^t), sqrt(1 - beta2^t) and eps, computed in fp64 and rounded to fp32 once.  ``groups``: dicts with lr, betas,
    eps, weight_decay (an optimiser's ``param_groups``)."""
    if not 1 <= len(groups) <= MAX_GROUPS:
        raise ValueError(f"between 1 and {MAX_GROUPS} parameter groups are supported, got {len(groups)}")
    h = _lib.OptimHyper()
    h.n_groups, h.zero_grads, h.grad_scale = len(groups), int(bool(zero_grads)), float(grad_scale)
    for i, g in enumerate(groups):
        lr, (b1, b2), eps, wd = float(g["lr"]), g["betas"], float(g["eps"]), float(g["weight_decay"])
        b1, b2 = float(b1), float(b2)
        hg = h.g[i]
        hg.decay = 1.0 - lr * wd
        hg.one_minus_beta1 = 1.0 - b1
        hg.beta2 = b2
        hg.one_minus_beta2 = 1.0 - b2
        hg.step_size = lr / (1.0 - b1 ** step)
        hg.bias2_sqrt = math.sqrt(1.0 - b2 ** step)
        hg.eps = eps
    return h


def grad_norm_host(flat_grad: np.ndarray, max_norm: float, grad_scale: float = 1.0):
    """bt_grad_norm_host on a flat fp32 array whose length is a multiple of 4 -> (norm, coef) as fp32"""
    g = np.ascontiguousarray(flat_grad, dtype=np.float32)
    rec = np.zeros(2, np.float32)
    _lib.check(_lib.lib().bt_grad_norm_host(g.ctypes.data, g.size, float(grad_scale), float(max_norm), rec.ctypes.data))
    return rec[0], rec[1]


def adamw_step_host(tensors, n_tensors, chunks, n_chunks, grad, m, v, h: _lib.OptimHyper, coef=None) -> None:
    """bt_adamw_step_host: the tensor table's ``param`` pointers and grad / m / v (flat fp32 numpy arrays) are updated in place"""
    c = None if coef is None else np.asarray([coef], np.float32)
    _lib.check(_lib.lib().bt_adamw_step_host(tensors, n_tensors, chunks, n_chunks, grad.ctypes.data, m.ctypes.data, v.ctypes.data,
                                             grad.size, C.byref(h), None if c is None else c.ctypes.data))


def adamw_ema_step_host(tensors, n_tensors, chunks, n_chunks, grad, m, v, ema, h: _lib.OptimHyper, ema_weight, ema_copy,
                        coef=None) -> None:
    """bt_adamw_ema_step_host: ``adamw_step_host`` plus the flat fp32 array of the averages, ``ema_weight`` = 1 - decay (rounded
    to fp32 once on the way in) and ``ema_copy`` (this step copies the new parameters instead of averaging)"""
    c = None if coef is None else np.asarray([coef], np.float32)
    _lib.check(_lib.lib().bt_adamw_ema_step_host(tensors, n_tensors, chunks, n_chunks, grad.ctypes.data, m.ctypes.data, v.ctypes.data,
                                                 ema.ctypes.data, grad.size, C.byref(h), None if c is None else c.ctypes.data,
                                                 float(ema_weight), int(bool(ema_copy))))


# ---- the loss scale of 16-mixed training ------------------------------------------------------------------------------------------
def scale_update(scale: float, growth_tracker: int, found_inf: bool, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000):
    """``torch.amp.GradScaler.update``'s rule on plain numbers -> (scale, growth_tracker).  A step with a non-finite gradient
    multiplies the scale by ``backoff_factor`` and clears the tracker; the ``growth_interval``-th finite step in a row
    multiplies it by ``growth_factor`` (unless that leaves fp32's range) and clears the tracker.  The scale is an fp32 number,
    as torch's is."""
    scale = np.float32(scale)
    if found_inf:
        return float(scale * np.float32(backoff_factor)), 0
    streak = int(growth_tracker) + 1
    if streak == int(growth_interval):
        with np.errstate(over="ignore"):
            grown = scale * np.float32(growth_factor)
        return float(grown if np.isfinite(grown) else scale), 0
    return float(scale), streak


class LossScaler:
    """The dynamic loss scale of 16-mixed training, ``torch.amp.GradScaler``'s semantics and defaults: multiply the loss by
    ``scale`` before ``backward()`` and hand the scaler to ``AdamW.step(loss_scaler=...)``, which divides the gradients by it
    inside its kernel, skips the step when a gradient is not finite, and calls ``update``.  With the default factors the
    scale stays a power of two, so scaling and unscaling are exact."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000):
        if not (init_scale > 0 and growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and int(growth_interval) >= 1):
            raise ValueError("LossScaler needs init_scale > 0, growth_factor > 1, 0 < backoff_factor < 1 and growth_interval >= 1")
        self.scale = float(np.float32(init_scale))
        self.growth_factor, self.backoff_factor = float(growth_factor), float(backoff_factor)
        self.growth_interval, self.growth_tracker = int(growth_interval), 0
        self.skipped_steps = 0

    def get_scale(self) -> float:
        return self.scale

    def update(self, found_inf: bool) -> None:
        self.skipped_steps += int(bool(found_inf))
        self.scale, self.growth_tracker = scale_update(self.scale, self.growth_tracker, bool(found_inf), self.growth_factor,
                                                       self.backoff_factor, self.growth_interval)

    def state_dict(self) -> dict:
        """``torch.amp.GradScaler.state_dict``'s keys"""
        return {"scale": self.scale, "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": self.growth_tracker}

    def load_state_dict(self, state: dict) -> None:
        self.scale = float(np.float32(state["scale"]))
        self.growth_factor, self.backoff_factor = float(state["growth_factor"]), float(state["backoff_factor"])
        self.growth_interval, self.growth_tracker = int(state["growth_interval"]), int(state["_growth_tracker"])


# ---- the optimiser ------------------------------------------------------------------------------------------------------------
class AdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` at its defaults (decoupled decay, no amsgrad, no maximize) for fp32 parameters on a ROCm GPU, on
    the library's fused kernels.  ``param_groups`` is torch's: schedulers work unchanged, ``lr`` and ``weight_decay`` are read
    from it at every step.  Up to 8 groups.

    The optimiser owns three flat fp32 device buffers (gradients, exp_avg, exp_avg_sq).  Every ``p.grad`` is set to its view of
    the gradient buffer, so autograd accumulates in place; ``step()`` is one launch over all tensors, which also clears the
    gradients it has consumed (``zero_grad()`` between steps is allowed and not needed).  ``max_grad_norm``: the gradients are
    clipped to that global L2 norm as ``torch.nn.utils.clip_grad_norm_`` does, by two more launches that leave the coefficient
    on the device.  ``accumulate``: the gradients are the sum over that many backward passes and are scaled by its inverse
    inside the kernel (``step(accumulated=k)`` overrides it for one step, e.g. the remainder of an epoch).  Nothing in
    ``step()`` waits for the GPU; ``last_grad_norm()`` is the only call that does -- unless a ``LossScaler`` is given.

    ``step(loss_scaler=s)`` (16-mixed training): the gradients were computed from ``s.scale`` times the loss.  The step always
    measures the gradient norm, with the kernel's gradient scale set to 1 / (count * scale), and THE HOST READS that 4-byte
    norm: the one wait per optimiser step, the wait ``torch.amp.GradScaler.step`` has too.  A norm that is not finite means
    some gradient was not: the step is skipped entirely -- parameters, moments and the step count stay as they are, the
    gradients are cleared -- and ``last_step_skipped`` is True; either way ``s.update`` then backs the scale off or counts
    towards its growth.

    Unlike torch, which skips a parameter whose ``grad`` is None, every parameter handed to this optimiser is updated on every
    step: a ``None`` gradient counts as zero (decay and the decaying momentum still move the parameter, as torch does for a
    zero gradient).  A gradient that is no longer the optimiser's view -- ``model.zero_grad(set_to_none=True)`` followed by a
    backward pass, or an assigned tensor -- is copied into the flat buffer at the next step and the view is attached again.

    ``ema_decay`` (a float in [0, 1); None: off, and nothing below exists): the optimiser also owns a fourth flat buffer, the
    exponential moving average of the parameters with ``torch.optim.swa_utils.AveragedModel``'s semantics under
    ``get_ema_multi_avg_fn(ema_decay)``: the first step taken copies the new parameters (``n_averaged`` 0 -> 1), every later one
    does e = e + (p - e) * (1 - decay) in the pass that has just made p.  A step that the ``LossScaler`` skips leaves the
    average and ``n_averaged`` as they are.  ``ema_parameters()`` are views of the averages; ``with opt.averaged_weights():``
    exchanges parameters and averages in one launch on entry and again on exit, so that the model computes with the averaged
    weights in between (``step()`` raises there).  The average travels in ``state_dict()`` under ``"ema"``; the decay is always the
    constructor's.  BatchNorm buffers are not parameters and are not averaged.

    ``process_group`` (a ``torch.distributed`` group; None: none of this exists): data-parallel training.  Every rank holds the
    same parameters and calls ``step()`` at the same points; after the gradients are attached and before anything reads them,
    the ranks' flat gradient buffers are added in rank order (``parallel.GradientExchange``, csrc/reduce.hip), so the norm,
    the clip coefficient, the loss scaler's decision and the update are computed from the same bits on every rank.
    ``accumulate`` and ``accumulated`` count the backward passes of ALL ranks.  ``staged``: the collectives go through host
    copies (gloo).  ``state_dict()`` and ``load_state_dict()`` are unchanged.  DESIGN.md section 26.

    Capturing ``step()`` into a HIP graph is out of scope: the learning rate, the bias corrections and the other scalars travel
    to the kernel by value, so a replay would repeat one step's scalars.  ``state_dict()`` and ``load_state_dict()`` are this
    class's own (the state lives in the flat buffers, not in ``self.state``): torch's state-dict pre- and post-hooks are not run."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, accumulate=1,
                 ema_decay=None, process_group=None, staged=False):
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError(f"invalid AdamW settings: lr {lr}, betas {betas}, eps {eps}, weight_decay {weight_decay}")
        if int(accumulate) < 1:
            raise ValueError(f"accumulate must be a positive number of backward passes, got {accumulate}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"max_grad_norm must be positive (or None), got {max_grad_norm}")
        if ema_decay is not None and not (isinstance(ema_decay, numbers.Real) and not isinstance(ema_decay, bool)
                                          and 0.0 <= ema_decay < 1.0):   # (numpy's scalars are numbers.Real too)
            raise ValueError(f"ema_decay must be a float in [0, 1) (or None), got {ema_decay!r}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.accumulate = int(accumulate)
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"at most {MAX_GROUPS} parameter groups are supported, got {len(self.param_groups)}")
        self._params, self._groups = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                _lib.require_gpu(p, "a parameter handed to beat_this_amd.optim.AdamW")
                if p.dtype != torch.float32:
                    raise TypeError(f"beat_this_amd.optim.AdamW updates float32 parameters only, got {p.dtype}")
                if not p.is_contiguous():
                    raise TypeError("beat_this_amd.optim.AdamW needs contiguous parameters (a view with an offset is fine)")
                self._params.append(p)
                self._groups.append(gi)
        if not self._params:
            raise ValueError("optimizer got an empty parameter list")
        self.device = self._params[0].device
        if any(p.device != self.device for p in self._params):
            raise ValueError("all parameters of one beat_this_amd.optim.AdamW must live on the same GPU")
        self._t = 0
        self._tables = None
        self._build_tables()
        dev = self.device
        self._reducer = None
        if process_group is None:
            self._grad = torch.zeros(self._total, dtype=torch.float32, device=dev)
        else:   # (the gradient buffer is the head of the exchange's store: the collectives need no staging copy)
            from .parallel import GradientExchange

            self._reducer = GradientExchange(process_group, self._total, dev, staged=staged)
            self._grad = self._reducer.flat
        self._m = torch.zeros_like(self._grad)
        self._v = torch.zeros_like(self._grad)
        self._ema = None if self.ema_decay is None else torch.zeros_like(self._grad)
        self._n_averaged, self._exchanged = 0, False
        self._norm_ws = torch.empty(_lib.lib().bt_grad_norm_workspace_bytes(self._total), dtype=torch.uint8, device=dev)
        self._record = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)   # {norm, coef}
        self._views = [self._grad[o:o + p.numel()].view(p.shape) for o, p in zip(self._offsets, self._params)]
        self._attach()

    def add_param_group(self, param_group) -> None:
        """Groups are fixed once the flat buffers and the device tables exist (the base class calls this during construction)"""
        if getattr(self, "_tables", None) is not None:
            raise RuntimeError("beat_this_amd.optim.AdamW lays its parameters out once: build a new optimiser for more parameters "
                               "(load_state_dict carries the moments over)")
        super().add_param_group(param_group)

    # -- layout -------------------------------------------------------------------------------------------------------------
    def _build_tables(self) -> None:
        ptrs = [p.data_ptr() for p in self._params]
        tensors, chunks, total, n_chunks = plan(ptrs, [p.numel() for p in self._params], self._groups, len(self.param_groups))
        if self._tables is not None and total != self._total:
            raise RuntimeError("a parameter changed its size after the optimiser was built")
        n = len(self._params)
        self._total, self._n_chunks, self._ptrs = total, n_chunks, ptrs
        self._offsets = [int(tensors[i].offset) for i in range(n)]
        host = (np.frombuffer(tensors, dtype=np.uint8, count=n * C.sizeof(_lib.OptimTensor)).copy(),
                np.frombuffer(chunks, dtype=np.uint8, count=max(n_chunks, 1) * C.sizeof(_lib.OptimChunk)).copy())
        self._tables = tuple(_lib.upload(a, self.device) for a in host)

    def _attach(self) -> None:
        """Every ``p.grad`` is the optimiser's view again; a foreign gradient is copied in first, None counts as zero.  A
        parameter whose storage moved (``p.data = ...``) gets the tables rebuilt."""
        moved = False
        for p, view, ptr in zip(self._params, self._views, self._ptrs):
            g = p.grad
            if g is view:   # (the usual case: autograd accumulated in place)
                pass
            elif g is None:
                view.zero_()
                p.grad = view
            elif g.data_ptr() != view.data_ptr() or g.shape != view.shape or g.stride() != view.stride() or g.dtype != view.dtype:
                view.copy_(g)
                p.grad = view
            moved = moved or p.data_ptr() != ptr
        if moved:
            self._build_tables()

    # -- torch.optim.Optimizer's interface ------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none: bool = True) -> None:
        """Clears the flat gradient buffer and attaches the views again (``set_to_none`` is accepted and ignored: the gradients
        stay views of the flat buffer)."""
        self._grad.zero_()
        for p, view in zip(self._params, self._views):
            p.grad = view

    @torch.no_grad()
    def step(self, closure=None, *, accumulated=None, loss_scaler=None):
        if self._exchanged:
            raise RuntimeError("step() inside averaged_weights(): the parameters hold the averages there")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._attach()
        if self._reducer is not None:   # (the sum over the ranks, in rank order: everything below sees the same bits on every rank)
            self._reducer.reduce_(self._grad)
        count = self.accumulate if accumulated is None else int(accumulated)
        if count < 1:
            raise ValueError(f"accumulated must be a positive number of backward passes, got {accumulated}")
        grad_scale = 1.0 / count if loss_scaler is None else 1.0 / (count * loss_scaler.scale)
        h = hyper(self.param_groups, self._t + 1, grad_scale=grad_scale, zero_grads=True)
        L = _lib.lib()
        self.last_step_skipped = False
        with torch.cuda.device(self.device):
            stream = _lib.stream_ptr(self.device)
            coef = None
            if self.max_grad_norm is not None or loss_scaler is not None:
                max_norm = math.inf if self.max_grad_norm is None else self.max_grad_norm   # (inf: the coefficient is 1)
                _lib.check(L.bt_grad_norm(stream, self._grad.data_ptr(), self._total, h.grad_scale, max_norm,
                                          self._norm_ws.data_ptr(), self._norm_ws.numel(), self._record.data_ptr()))
                if self.max_grad_norm is not None:
                    coef = self._record.data_ptr() + 4
            if loss_scaler is not None:
                finite = math.isfinite(float(self._record[0]))   # (the step's one wait for the GPU)
                loss_scaler.update(not finite)
                if not finite:
                    self._grad.zero_()
                    self.last_step_skipped = True
                    return loss
            self._t += 1
            if self._ema is None:
                _lib.check(L.bt_adamw_step(stream, self._tables[0].data_ptr(), len(self._params), self._tables[1].data_ptr(),
                                           self._n_chunks, self._grad.data_ptr(), self._m.data_ptr(), self._v.data_ptr(), self._total,
                                           C.byref(h), coef))
            else:   # (1 - decay in fp64; ctypes rounds it to fp32 once)
                _lib.check(L.bt_adamw_ema_step(stream, self._tables[0].data_ptr(), len(self._params), self._tables[1].data_ptr(),
                                               self._n_chunks, self._grad.data_ptr(), self._m.data_ptr(), self._v.data_ptr(),
                                               self._ema.data_ptr(), self._total, C.byref(h), coef, 1.0 - self.ema_decay,
                                               int(self._n_averaged == 0)))
                self._n_averaged += 1
        # the kernel wrote the parameters behind autograd's back: bump their versions, so that BeatThis packs its inference
        # engine again and a graph that saved a parameter refuses a stale backward
        torch.autograd.graph.increment_version(self._params)
        return loss

    def flat_state(self) -> dict:
        """The optimiser's own buffers, not copies: ``grad``, ``exp_avg`` and ``exp_avg_sq`` (flat fp32 device tensors of
        ``total`` elements), ``offsets`` (where each parameter starts, in the order of ``param_groups``; multiples of 4, zero
        padding in between) and ``step`` (the number of steps taken).  With ``ema_decay`` also ``ema`` (the flat buffer of the
        averages) and ``n_averaged``."""
        st = dict(grad=self._grad, exp_avg=self._m, exp_avg_sq=self._v, offsets=list(self._offsets), total=self._total,
                  step=self._t)
        if self._ema is not None:
            st.update(ema=self._ema, n_averaged=self._n_averaged)
        return st

    # -- weight averaging -----------------------------------------------------------------------------------------------------
    def _need_ema(self, what: str) -> None:
        if self._ema is None:
            raise RuntimeError(f"{what} needs weight averaging: build the optimiser with ema_decay")

    def ema_parameters(self) -> list:
        """Views of the averages, shaped like the parameters, in the order of ``param_groups`` (inside ``averaged_weights()``
        they hold the live weights)."""
        self._need_ema("ema_parameters()")
        return [self._ema[o:o + p.numel()].view(p.shape) for o, p in zip(self._offsets, self._params)]

    def _exchange(self) -> None:
        if any(p.data_ptr() != ptr for p, ptr in zip(self._params, self._ptrs)):   # (a parameter's storage moved)
            self._build_tables()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bt_ema_exchange(_lib.stream_ptr(self.device), self._tables[0].data_ptr(), len(self._params),
                                                  self._tables[1].data_ptr(), self._n_chunks, self._ema.data_ptr(), self._total))
        torch.autograd.graph.increment_version(self._params)   # (BeatThis packs its inference engine again)

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside the context the parameters hold the averages (and the optimiser's buffer the live weights): one exchange
        launch on entry, one on exit, which restores every bit.  Not re-entrant; needs at least one averaged step."""
        self._need_ema("averaged_weights()")
        if self._n_averaged == 0:
            raise RuntimeError("averaged_weights() before the first averaged step: there is no average yet")
        if self._exchanged:
            raise RuntimeError("averaged_weights() is not re-entrant")
        self._exchange()
        self._exchanged = True
        try:
            yield self
        finally:
            self._exchange()
            self._exchanged = False

    def last_grad_norm(self) -> float:
        """The global gradient norm (after the 1 / accumulate scaling, before clipping) that the last ``step()`` with
        ``max_grad_norm`` measured.  Reads the device record: this call waits for the GPU."""
        if self.max_grad_norm is None:
            raise RuntimeError("last_grad_norm() needs max_grad_norm: no norm is computed without it")
        return float(self._record[0])

    def state_dict(self) -> dict:
        """``torch.optim.AdamW``'s layout: per parameter index ``step`` (a float32 scalar tensor), ``exp_avg``, ``exp_avg_sq``
        (copies, shaped like the parameter), and ``param_groups`` with parameter indices.  With ``ema_decay`` also ``ema``:
        ``decay``, ``n_averaged`` and ``params`` (per parameter index a copy of its average).  Raises inside
        ``averaged_weights()``, where weights and averages are exchanged: a state saved there would hold them swapped."""
        if self._exchanged:
            raise RuntimeError("state_dict() inside averaged_weights(): the parameters hold the averages there")
        state, groups, k = {}, [], 0
        index = {id(p): i for i, p in enumerate(self._params)}
        for group in self.param_groups:
            packed = {key: val for key, val in group.items() if key != "params"}
            packed["params"] = [index[id(p)] for p in group["params"]]
            groups.append(packed)
        for i, (p, o) in enumerate(zip(self._params, self._offsets)):
            n = p.numel()
            state[i] = {"step": torch.tensor(float(self._t), dtype=torch.float32),
                        "exp_avg": self._m[o:o + n].view(p.shape).clone(),
                        "exp_avg_sq": self._v[o:o + n].view(p.shape).clone()}
        out = {"state": state, "param_groups": groups}
        if self._ema is not None:
            out["ema"] = {"decay": self.ema_decay, "n_averaged": self._n_averaged,
                          "params": {i: e.clone() for i, e in enumerate(self.ema_parameters())}}
        return out

    @torch.no_grad()
    def load_state_dict(self, state_dict: dict) -> None:
        """Takes a state dict of this class or of ``torch.optim.AdamW`` over the same parameters in the same order: the moments
        are copied into the flat buffers (bit for bit), the groups' settings replace the current ones.  Weight averaging: an
        ``"ema"`` entry is restored bit for bit when this optimiser averages (``ema_decay`` stays the constructor's) and ignored
        when it does not; a state without one starts the average over, the next step copies.  The averages are checked
        before anything is written: a state whose averages do not fit leaves the optimiser as it was."""
        if self._exchanged:
            raise RuntimeError("load_state_dict() inside averaged_weights(): the parameters hold the averages there")
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(g["params"]) != len(mine["params"])
                                                        for g, mine in zip(groups, self.param_groups)):
            raise ValueError("loaded state dict has different parameter groups")
        if any(g.get("amsgrad") or g.get("maximize") for g in groups):
            raise ValueError("beat_this_amd.optim.AdamW has no amsgrad / maximize")
        order = [i for g in groups for i in g["params"]]
        averages = None
        if self._ema is not None and state_dict.get("ema") is not None:
            saved = state_dict["ema"]["params"]
            averages = [saved.get(i, saved.get(str(i))) for i in range(len(self._params))]
            for i, (p, src) in enumerate(zip(self._params, averages)):
                if src is None or tuple(src.shape) != tuple(p.shape):
                    raise ValueError(f"loaded average of parameter {i} is missing or has the wrong shape")
        state = state_dict.get("state", {})
        steps = set()
        self._m.zero_()
        self._v.zero_()
        for p, o, key in zip(self._params, self._offsets, order):
            s = state.get(key, state.get(str(key)))
            if s is None:
                steps.add(0)
                continue
            n = p.numel()
            if tuple(s["exp_avg"].shape) != tuple(p.shape) or tuple(s["exp_avg_sq"].shape) != tuple(p.shape):
                raise ValueError(f"loaded state of parameter {key} has shape {tuple(s['exp_avg'].shape)}, expected {tuple(p.shape)}")
            self._m[o:o + n].view(p.shape).copy_(s["exp_avg"])
            self._v[o:o + n].view(p.shape).copy_(s["exp_avg_sq"])
            steps.add(int(s["step"]))
        if len(steps) > 1:
            raise ValueError(f"beat_this_amd.optim.AdamW keeps one step count for all parameters, the state has {sorted(steps)}")
        self._t = steps.pop() if steps else 0
        if self._ema is not None:
            self._ema.zero_()
            self._n_averaged = 0
            if averages is not None:
                for e, src in zip(self.ema_parameters(), averages):
                    e.copy_(src)
                self._n_averaged = int(state_dict["ema"]["n_averaged"])
        for g, mine in zip(groups, self.param_groups):
            for key, val in g.items():
                if key != "params":
                    mine[key] = tuple(val) if key == "betas" else val


# ---- schedule and grouping ----------------------------------------------------------------------------------------------------
class CosineWarmupScheduler(torch.optim.lr_scheduler.LRScheduler):
    """The reference's learning-rate schedule (pl_module.py:342-369), stepped once per optimiser step.  The cosine runs over
    ``decay_steps = int((1 - raise_last) * max_iters)`` steps; the factor on every group's base rate at step ``s`` is

        s <  decay_steps:  0.5 (1 + cos(pi s / decay_steps)), times s / warmup while s <= warmup   (warm-up into a cosine decay)
        s >= decay_steps:  raise_to * min((s - decay_steps) / warmup, 1)                          (the optional final re-raise)

    so the rate is 0 at step 0, and beyond ``max_iters`` stays at ``raise_to`` times the base rate.  Works with any torch
    optimiser; the three numbers are part of its ``state_dict()``."""

    def __init__(self, optimizer, warmup, max_iters, raise_last=0, raise_to=0.5):
        if not 0 <= raise_last < 1:
            raise ValueError(f"raise_last is a fraction of the run in [0, 1), got {raise_last}")
        self.warmup_steps, self.plateau = warmup, raise_to
        self.decay_steps = int(max_iters * (1 - raise_last))
        super().__init__(optimizer)   # (takes the first step: the attributes above have to exist)

    def get_lr_factor(self, step):
        into_raise = step - self.decay_steps
        if into_raise >= 0:
            return float(self.plateau * min(into_raise / self.warmup_steps, 1))
        ramp = step / self.warmup_steps if step <= self.warmup_steps else 1.0
        return float(0.5 * (1 + np.cos(np.pi * (step / self.decay_steps))) * ramp)

    def get_lr(self):
        factor = self.get_lr_factor(self.last_epoch)
        return [base * factor for base in self.base_lrs]


def param_groups_for(module: torch.nn.Module, weight_decay: float) -> list:
    """The reference's two groups (pl_module.py:283-296): trainable parameters with two or more dimensions are decayed, biases
    and norm gains (one dimension or none) are not."""
    trainable = [p for p in module.parameters() if p.requires_grad]
    return [{"params": [p for p in trainable if p.ndim >= 2], "weight_decay": weight_decay},
            {"params": [p for p in trainable if p.ndim <= 1], "weight_decay": 0}]
