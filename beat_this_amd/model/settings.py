"""What the differentiable route of ``BeatThis`` is configured by, as one object (``TrainSettings``, ``model.train_settings``), the
one place that knows the prerequisites between its opt-ins (``TrainSettings.violations``) and the one decision which route a call
takes (``decide``).  ``BeatThis``, ``PLBeatThis``, ``fit()`` and the command line all check what they are asked for here, each
refusing with its own exception type and under its own names for the switches.  Plain Python: nothing here touches a tensor."""
from __future__ import annotations

import dataclasses
from typing import NamedTuple, Optional


PRECISIONS = ("16-mixed", "32-high", "32-true")   # what ``train_precision`` and ``frontend_precision`` take
X3_OPERAND = "bf16x3"                             # the operand format of a "32-high" part's calls (BT_OPERAND_BF16X3)


class Violation(NamedTuple):
    """The switch ``what`` needs the switch ``needs`` because of ``why``, or (``needs`` None) a value is out of range and ``why``
    says it all.  The switches: "batch_statistics", "frontend_precision", "frontend_dropout", "dropout", "train_frontend",
    "train_operand", "frontend_operand" and, as what those need, "train_mixed", "frontend_mixed" (the part on "16-mixed")."""
    what: str
    needs: Optional[str]
    why: str

    def message(self, names: dict) -> str:   # (in the words of a surface that calls the switches ``names``)
        return self.why if self.needs is None else f"{names[self.what]} needs {names[self.needs]}: {self.why}"


@dataclasses.dataclass
class TrainSettings:
    """The opt-ins of the differentiable route (DESIGN.md sections 15-21 have the arithmetic).  None changes what ``no_grad``,
    inference or ``eval()`` validation run, none is inferred from ``requires_grad``, ``train()`` or ``torch.autocast``, and none
    is a hyper-parameter: they pickle and deep-copy with the model, and a checkpoint carries ``dropout_state()`` alone.

    ``train_precision`` (``set_train_precision``, section 16): "32-true", or "16-mixed" -- the trunk's attention and feed-forward
    round both operands of every matrix product to fp16 and accumulate in fp32; everything else stays fp32.  Use it with a
    loss scale (``optim.LossScaler``; ``fit(precision="16-mixed")`` does).

    ``frontend_trainable`` (``set_frontend_trainable``, section 17): whole-model fine-tuning.  In grad mode ``model(x)`` and
    ``model.frontend(x)`` run the frontend on the differentiable route too, and gradients reach ``x`` when it requires grad.
    Without it the frontend is frozen, and a frontend parameter that requires grad makes a grad-mode forward raise
    ``NotImplementedError`` rather than silently leaving its ``.grad`` empty.  The callable nodes below ``frontend`` (``stem``,
    ``blocks[i]``, ``.partial``, ``.linear`` ...) stay inference-only and the route does not pass through them: forward hooks
    registered BELOW ``frontend`` do not fire on a grad-mode call with the flag set (hooks on ``frontend`` itself and on the
    trunk's nodes do; under ``no_grad`` all fire as ever).

    ``frontend_precision`` (``set_frontend_precision``, section 19): the same two values, independent of ``train_precision``, for
    the matrix products of the differentiable frontend's conv units, twelve partial-transformer leaves and projection, not its stem.

    ``train_operand`` / ``frontend_operand`` (the ``operand`` argument of the two setters above, section 24): the 16-bit format both
    operands of a 16-mixed part's products are rounded to, "fp16" (the default: the reference's ``16-mixed``) or "bf16" (what
    Lightning calls ``bf16-mixed``: fp32's exponent range, so nothing overflows by rounding and no loss scale is needed).  Read
    only where the part's precision is "16-mixed"; "bf16" beside "32-true" or "32-high" is refused.

    "32-high" (section 25), a third value of both precisions: the same products as "16-mixed", each fp32 operand multiplied as the
    sum of two bfloat16 numbers on three bfloat16 MFMAs (what ``torch.set_float32_matmul_precision("high")`` names) -- about
    2^-17 of an operand kept, fp32's exponent range, no loss scale.  The operand field is not read beside it.

    ``batch_statistics`` (``set_batch_statistics``, section 18): training from scratch; needs ``frontend_trainable``.  Without
    it the frontend's BatchNorms use ``running_mean`` / ``running_var``, in ``train()`` as in ``eval()``, and never update them.
    With it, in ``train()`` mode and grad mode, the five BatchNorms (``stem.bn1d``, ``stem.bn2d``, ``blocks[i].norm``) are
    torch's training-mode ones: they normalise with the statistics of the call's own batch, the backward differentiates through
    them, and every forward call WRITES the model's buffers -- it moves ``running_mean`` / ``running_var`` and adds 1 to
    ``num_batches_tracked``, each micro-batch of an accumulated step on its own -- so a sequence's input gradient is no longer
    the same alone and inside a batch.  Batch x time = 1 raises torch's ``ValueError`` before any launch.  In ``eval()``, under
    ``no_grad`` and on the inference paths the running statistics are used as ever (the engine packs the moved buffers again).

    ``dropout_rng`` (``enable_dropout(seed)`` / ``set_dropout_state``, section 15): None -- off -- or {"seed", "calls"}.  Then, in
    ``train()`` mode and with ``dropout["transformer"]`` above 0, the main layers drop where the reference's do, with this
    package's own masks (Philox under ``seed``, not torch's generator): every attention / feed-forward call that drops takes the
    next stream number from the counter ``calls``, which ``set_dropout_state()`` rewinds to repeat a run bit for bit.  A graph
    capture with dropout active raises ``RuntimeError`` (a replay would repeat its masks).

    ``frontend_dropout`` (``enable_dropout(seed, frontend=True)``, section 21): a second opt-in on top, read only where the
    differentiable frontend runs (the frozen frontend runs the inference path, which never drops).  Then, in ``train()`` mode and
    with ``dropout["frontend"]`` above 0, the twelve leaves drop too -- never the stem, the conv units or the projection -- and
    take their stream numbers from the same counter in forward order (block 0 ``attnF``, ``ffF``, ``attnT``, ``ffT``, then blocks
    1 and 2, then the trunk's units): a whole-model forward advances ``calls`` by 12 + 2 ``n_layers``.

    ``stats_moved``: a batch-statistics forward wrote the running buffers since the engine packed its copies (through raw
    pointers: no ``_version`` tells); the next inference call packs again."""
    train_precision: str = "32-true"
    frontend_precision: str = "32-true"
    frontend_trainable: bool = False
    batch_statistics: bool = False
    dropout_rng: Optional[dict] = None
    frontend_dropout: bool = False
    stats_moved: bool = False
    train_operand: str = "fp16"
    frontend_operand: str = "fp16"

    def needs_loss_scale(self) -> bool:
        """Some part is 16-mixed with fp16 operands: its gradients can overflow, so the recipe scales the loss (section 24)"""
        return any(precision == "16-mixed" and operand == "fp16" for precision, operand in
                   ((self.train_precision, self.train_operand), (self.frontend_precision, self.frontend_operand)))

    @classmethod
    def from_loose_attributes(cls, state: dict) -> "TrainSettings":
        """Taken out of the ``__dict__`` of a model pickled when every field was an attribute of its own ("_" + the field's
        name); a field that did not exist yet gets its default."""
        return cls(**{f.name: state.pop("_" + f.name, f.default) for f in dataclasses.fields(cls)})

    def violations(self, level: str = "model", rates: dict = {}) -> list:
        """The prerequisites this combination violates, each written here and nowhere else.  ``level`` "model": what ``BeatThis``
        refuses -- batch statistics on a frozen frontend and values out of range (``rates``: the dropout rates to look at, by
        part; the frontend's only with its opt-in), not frontend dropout on a frozen frontend; "recipe": what training needs."""
        found = []
        if self.batch_statistics and not self.frontend_trainable:
            found.append(Violation("batch_statistics", "train_frontend", "batch statistics belong to the differentiable frontend"))
        if level == "recipe":
            found += self._operand_violations()
            if self.frontend_precision != "32-true" and not self.frontend_trainable:   # (the command line alone insists on it)
                found.append(Violation("frontend_precision", "train_frontend", "it belongs to the differentiable frontend"))
            if self.frontend_dropout and self.dropout_rng is None:
                found.append(Violation("frontend_dropout", "dropout", "the frontend's dropout is a second opt-in on top of it"))
            if self.frontend_dropout and not self.frontend_trainable:
                found.append(Violation("frontend_dropout", "train_frontend", "only the differentiable frontend drops"))
            return found
        for which, value in (("train", self.train_precision), ("frontend", self.frontend_precision)):
            if value not in PRECISIONS:
                found.append(Violation(which + "_precision", None,
                                       f"{which} precision must be '16-mixed', '32-high' or '32-true', got {value!r}"))
        found += self._operand_violations()
        for part, p in rates.items():
            if (part != "frontend" or self.frontend_dropout) and not 0.0 <= float(p) < 1.0:   # (NaN fails both comparisons)
                found.append(Violation("dropout", None, f"dropout[{part!r}] = {float(p)}: the rate must satisfy 0 <= p < 1"))
        rng = self.dropout_rng or {"seed": 0, "calls": 0}
        if not (0 <= rng["seed"] < 1 << 64 and 0 <= rng["calls"] < 1 << 64):
            found.append(Violation("dropout", None, f"dropout seed and calls must fit 64 unsigned bits, got {rng['seed']} and {rng['calls']}"))
        return found

    def _operand_violations(self) -> list:
        """An operand format nobody knows, or "bf16" on a part that is not 16-mixed (the same at both levels)"""
        found = []
        for which in ("train", "frontend"):
            operand, precision = getattr(self, which + "_operand"), getattr(self, which + "_precision")
            if operand not in ("fp16", "bf16"):
                found.append(Violation(which + "_operand", None, f"{which} operand must be 'fp16' or 'bf16', got {operand!r}"))
            elif operand == "bf16" and precision != "16-mixed":
                found.append(Violation(which + "_operand", which + "_mixed",
                                       "bf16 is the operand format of 16-mixed products; a 32-true part rounds nothing"))
        return found

    def changed(self, level: str, error: type, names: dict, rates: dict = {}, only: str = None, **fields) -> "TrainSettings":
        """A copy with ``fields`` replaced, or ``error`` with the first prerequisite that copy violates at ``level`` (``only``:
        among those about that switch), in the caller's words for the switches (``names``)"""
        new = dataclasses.replace(self, **fields)
        for v in new.violations(level, rates):
            if only is None or v.what == only:
                raise error(v.message(names))
        return new


# ---- which route a call takes ----------------------------------------------------------------------------------------------------
DIFFERENTIABLE, ENGINE, MODULES, REFUSE = "differentiable", "engine", "modules", "refuse"


class Route(NamedTuple):
    """``how``: DIFFERENTIABLE (backward.py), ENGINE (the inference path), MODULES (that path through the sub-modules, so that a
    hook below fires) or REFUSE (a frozen frontend was asked for gradients).  The rest is False unless ``how`` is DIFFERENTIABLE:
    the frontend's BatchNorms use this call's batch; this part's calls draw dropout masks; its unit calls are 16-mixed;
    ``operand``: "fp16" unless they are 16-mixed on "bf16" operands; a "32-high" part's calls are mixed calls whose operand is
    "bf16x3"."""
    how: str
    batch_statistics: bool = False
    drop: bool = False
    mixed: bool = False
    operand: str = "fp16"

    @property
    def mixed_operand(self):
        """What backward.py takes as ``mixed``: False, or the operand format of the 16-mixed calls"""
        return self.operand if self.mixed else False


_PLAIN = {how: Route(how) for how in (ENGINE, MODULES, REFUSE)}   # (built once: the inference path builds nothing per call)


def decide(s: TrainSettings, part: str, grad: bool, training: bool = False, x_grad: bool = False, param_grad: bool = False,
           hooked: bool = False, rate: float = 0.0) -> Route:
    """The route of one call of ``part`` -- "frontend", "transformer" (the trunk or one of its units) or "heads" -- from plain
    values: the settings, ``torch.is_grad_enabled()``, ``model.training``, whether the tensor handed in requires grad, whether
    a parameter below the node does, whether a sub-module below it is hooked, and the part's rate ``model.dropout[part]``.
    The frontend is differentiable iff its opt-in is set and grad mode is on, whatever requires grad; without the opt-in a
    parameter that requires grad is refused in grad mode.  The trunk and the heads are differentiable iff grad mode is on and
    the input or one of their parameters requires grad.  Everything else is the inference path, through the modules when
    something below is hooked (never the heads: nothing below them is callable)."""
    frontend = part == "frontend"
    if grad and (s.frontend_trainable if frontend else x_grad or param_grad):
        if part == "heads":
            return Route(DIFFERENTIABLE)
        drop = s.dropout_rng is not None and training and rate > 0.0 and (s.frontend_dropout or not frontend)
        precision = s.frontend_precision if frontend else s.train_precision
        mixed = precision in ("16-mixed", "32-high")
        operand = X3_OPERAND if precision == "32-high" else (s.frontend_operand if frontend else s.train_operand) if mixed else "fp16"
        return Route(DIFFERENTIABLE, frontend and s.batch_statistics and training, drop, mixed, operand)
    if grad and frontend and param_grad:
        return _PLAIN[REFUSE]
    return _PLAIN[MODULES if hooked and part != "heads" else ENGINE]
