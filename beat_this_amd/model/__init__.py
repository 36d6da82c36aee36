"""``BeatThis`` -- drop-in for beat_this.model.beat_tracker.BeatThis (beat_tracker.py:18-203).

Same constructor signature, same ``state_dict`` keys (so reference checkpoints load with
``load_state_dict``), same ``forward(x: (B,T,128)) -> {"beat": (B,T), "downbeat": (B,T)}``;
the arithmetic runs in the hand-written HIP kernels of libbeat_this_amd.so.  (A package like the reference's
``beat_this.model``: ``beat_this_amd.model.beat_tracker.BeatThis`` and ``beat_this_amd.model.postprocessor.Postprocessor`` resolve
to the same classes, so ``pl_module.py``-style imports keep working.)  Precision
follows the caller exactly like the reference: under ``torch.autocast`` (what
``Spect2Frames(float16=True)`` enters, inference.py:246) the half-precision (fp16 MFMA operand) path runs, otherwise
an fp32-class path: exact fp32 MFMAs, or -- ``fp32_split_gemms``, what the inference classes select for
``float16=False`` -- three fp16 MFMAs per product on hi + lo operand halves.  There is no CPU implementation here.

Fine-tuning: the main transformer layers, the final RMSNorm and the task heads are differentiable (``backward.py``), and with
``set_frontend_trainable()`` the frontend is too; see the ``BeatThis`` class docstring.
"""
from __future__ import annotations

import weakref

import torch
from torch import nn

from .. import _lib
from . import backward as _bw
from ..pack import Engine, PackedModel
from ..weights import random_state_dict, resolve_hparams, state_dict_shapes
from .settings import DIFFERENTIABLE, ENGINE, MODULES, REFUSE, TrainSettings, decide

_BUFFER_LEAVES = ("running_mean", "running_var", "num_batches_tracked")
_PARTS = ("frontend", "transformer", "heads")   # of settings.decide, by stage; "frontend" / "transformer" are the keys of ``dropout``
_SETTERS = {"batch_statistics": "set_batch_statistics()", "train_frontend": "set_frontend_trainable() first",   # (names in a refusal)
            "train_operand": "operand='bf16'", "train_mixed": "set_train_precision('16-mixed')",
            "frontend_operand": "operand='bf16'", "frontend_mixed": "set_frontend_precision('16-mixed')"}
_TREE_EPOCH = [0]   # bumped whenever a module is assigned to / removed from a node of a BeatThis tree (_hooked_below's cache)


class _TracksChildren:
    """nn.Module mix-in: assigning, adding or deleting a sub-module bumps _TREE_EPOCH."""

    def __setattr__(self, name, value):
        if isinstance(value, (nn.Module, nn.Parameter)):   # (a replaced Parameter: the cached parameter lists are stale too)
            _TREE_EPOCH[0] += 1
        super().__setattr__(name, value)

    def __delattr__(self, name):
        _TREE_EPOCH[0] += 1
        super().__delattr__(name)

    def add_module(self, name, module):
        _TREE_EPOCH[0] += 1
        super().add_module(name, module)


class _Node(_TracksChildren, nn.Module):
    """Container that carries the reference's dotted parameter names.  The nodes that are callable sub-modules in the
    reference -- ``frontend.stem``, ``.blocks``, ``.blocks[i]``, ``.blocks[i].partial``, ``.concat``, ``.linear``,
    ``transformer_blocks.layers[l][0]`` (Attention), ``[l][1]`` (FeedForward), ``.norm`` (beat_tracker.py:54-80,108-168,
    roformer.py:138-181) -- are bound to a unit of the owning model's engine (BeatThis._bind_units, bt_forward_unit) and can
    be called with the reference's tensor layouts: (b, c, f, t) inside the frontend, (b, n, dim) in the transformer; so are
    the four leaves of a partial transformer (``partial.attnF / .ffF / .attnT / .ffT``: (sequences, tokens, C), the branch
    without its residual, beat_tracker.py:251-301).  They run on the generic kernels (exact fp32, or half operands under
    autocast), one launch group per call; the fused fast path is ``BeatThis.forward`` / the three stages.  Nodes below them
    (``...norm``, ``.to_qkv``, ``.net`` ...) hold parameters only.
    Digit-named children index like the reference's ModuleList / Sequential (``layers[3][0]``, ``blocks[1]``)."""

    _unit = None   # (kind, index) once bound

    def __getstate__(self):  # (copy.deepcopy / pickle: the owner re-binds itself, BeatThis.__setstate__)
        state = self.__dict__.copy()
        state.pop("_root", None)
        return state

    def _indexed(self):
        keys = [k for k in self._modules if k.isdigit()]
        return sorted(keys, key=int)

    def __len__(self):
        return len(self._indexed())

    def __bool__(self):   # (a module is truthy whatever its number of indexed children)
        return True

    def __getitem__(self, i: int):
        keys = self._indexed()
        if not keys:
            raise TypeError(f"{type(self).__name__} node is not indexable")
        return self._modules[keys[i]]

    def __iter__(self):
        return iter(self._modules[k] for k in self._indexed())

    def forward(self, x: torch.Tensor):
        if self._unit is None:
            raise NotImplementedError(
                "this node only carries parameters under the reference's names; the callable sub-modules are frontend.stem / "
                ".blocks / .blocks[i] / .blocks[i].partial (and its attnF / ffF / attnT / ffT) / .concat / .linear, "
                "transformer_blocks.layers[l][0] / [l][1] / .norm and the three stages")
        return self._root()._run_unit(x, *self._unit)


class _Stage(_Node):
    """``BeatThis.frontend`` / ``.transformer_blocks`` / ``.task_heads`` (beat_tracker.py:54-106): parameter containers
    with the reference's names that can also be CALLED like the reference's sub-modules -- the stage runs in the owning
    model's engine (bt_forward_stages), so forward hooks and partial forwards written against the reference keep working:
    frontend (B,T,128) -> (B,T,D); transformer_blocks (B,T,D) -> (B,T,D) incl. its final RMSNorm; task_heads (B,T,D) ->
    {"beat", "downbeat"}."""

    def __init__(self, root: "BeatThis", stage: int):
        super().__init__()
        object.__setattr__(self, "_root", weakref.ref(root))   # (not a registered sub-module: no cycle)
        self._stage = stage

    def forward(self, x: torch.Tensor):
        root = self._root()
        route = root._route(_PARTS[self._stage], self, x, hooks=self._stage < 2)
        if route.how == ENGINE:
            out = root._run(x, self._stage, self._stage)
            return {"beat": out[0], "downbeat": out[1]} if self._stage == 2 else out
        if self._stage == 1:
            # the reference's container loop over the units (roformer.py:176-181), each of which takes its own route: the
            # differentiable one (backward.py), or somebody hooked a sub-module of this stage and the hook has to fire
            for attn, ff in self.layers:
                x = attn(x) + x
                x = ff(x) + x
            return self.norm(x)
        if route.how == MODULES:   # a hook below the frontend: through its sub-modules (beat_tracker.py:77-80)
            return self.linear(self.concat(self.blocks(self.stem(x))))
        return root._head_train(x) if self._stage == 2 else root._frontend_train(x, route)


def _hooked_below(node: nn.Module) -> bool:
    """A forward (pre-)hook is registered on a sub-module of ``node`` (not on ``node`` itself).  Asked on every forward and every
    single-file call: walking ``node.modules()`` costs 0.1 ms for final0's ~200 nodes, so the hook dictionaries of the tree
    (created once per module, mutated in place by ``register_forward_*hook``) are collected once and only looked at afterwards;
    the collection is redone when any node of a BeatThis tree had a sub-module assigned, added or removed (_TREE_EPOCH)."""
    epoch = _TREE_EPOCH[0]
    cache = node.__dict__.get("_bt_hook_dicts")
    if cache is None or cache[0] != epoch:
        cache = (epoch, [(m._forward_hooks, m._forward_pre_hooks) for m in node.modules() if m is not node])
        node.__dict__["_bt_hook_dicts"] = cache
    for fwd, pre in cache[1]:
        if fwd or pre:
            return True
    return False


def _params_of(node: nn.Module) -> tuple:
    """The parameters below ``node``, collected once per tree epoch (asked on every call in grad mode)."""
    epoch = _TREE_EPOCH[0]
    cache = node.__dict__.get("_bt_params")
    if cache is None or cache[0] != epoch:
        cache = (epoch, tuple(node.parameters()))
        node.__dict__["_bt_params"] = cache
    return cache[1]


def _any_requires_grad(node: nn.Module) -> bool:
    for p in _params_of(node):
        if p.requires_grad:
            return True
    return False


def _attach(root: nn.Module, key: str, value: torch.Tensor) -> None:
    *path, leaf = key.split(".")
    node = root
    for part in path:
        if part not in node._modules:
            node.add_module(part, _Node())
        node = node._modules[part]
    if leaf in _BUFFER_LEAVES:
        node.register_buffer(leaf, value)
    else:
        node.register_parameter(leaf, nn.Parameter(value, requires_grad=False))


class BeatThis(_TracksChildren, nn.Module):
    """The reference's ``BeatThis`` on the HIP kernels.  Inference is the default: parameters are created with
    ``requires_grad=False``, the model is in ``eval()``, and nothing below changes what such a model runs.

    Fine-tuning.  ``model.transformer_blocks.requires_grad_(True)`` and / or ``model.task_heads.requires_grad_(True)`` opt in.
    When grad mode is on and one of those parameters requires grad -- or the tensor handed to ``transformer_blocks``,
    ``task_heads``, ``layers[l][0]``, ``layers[l][1]`` or ``.norm`` does -- the differentiable route runs: ``forward`` computes
    the frontend on the usual fast path under ``no_grad`` (at the model's own precision), then the six main layers, the final
    RMSNorm and the heads go through ``torch.autograd.Function``s over the library's training kernels, composed like the
    reference's containers.  Its arithmetic is fp32, whatever ``fp32_split_gemms`` says and also under ``torch.autocast``;
    ``rotary_embed.freqs`` never receives a gradient, as in the reference; parameters on the CPU raise the same ``RuntimeError``
    as ever.  Which route a call takes is decided in one place (``_route``, over ``settings.decide``).

    Everything else about that route is an opt-in, held in ``self.train_settings``; ``settings.TrainSettings`` says what each means:
      * ``set_train_precision("16-mixed")`` -> ``train_precision``: the reference's training precision in the trunk; with
        ``operand="bf16"`` -> ``train_operand``: its products on bfloat16 operands, which need no loss scale (likewise
        ``set_frontend_precision`` -> ``frontend_operand``);
      * ``set_frontend_trainable()`` -> ``frontend_trainable``: whole-model fine-tuning; ``False`` restores the frozen state and
        drops the engine's packed copies, so the frozen frontend runs on the weights as trained;
      * ``set_frontend_precision("16-mixed")`` -> ``frontend_precision``: fp16 matrix products in that frontend;
      * ``set_batch_statistics()`` -> ``batch_statistics``: training from scratch; such a forward writes the running buffers;
      * ``enable_dropout(seed)`` -> ``dropout_rng``: in the main layers in ``train()`` mode; with ``frontend=True`` ->
        ``frontend_dropout``: in the frontend's leaves too.

    The route reads the parameters' storage at call time, so an optimizer step is seen at once.  The inference paths run on
    packed copies: the ``_version`` of every parameter is recorded when they are packed, and a parameter that requires grad
    and was changed in place since makes the next inference call pack again (checked only for parameters that require grad);
    so does a batch-statistics forward, which leaves a note that the running buffers moved.
    """

    def __init__(self, spect_dim: int = 128, transformer_dim: int = 512, ff_mult: int = 4, n_layers: int = 6,
                 head_dim: int = 32, stem_dim: int = 32, dropout: dict = {"frontend": 0.1, "transformer": 0.2},
                 sum_head: bool = True, partial_transformers: bool = True):
        super().__init__()
        self.hparams = resolve_hparams(dict(
            spect_dim=spect_dim, transformer_dim=transformer_dim, ff_mult=ff_mult, n_layers=n_layers,
            head_dim=head_dim, stem_dim=stem_dim, sum_head=sum_head, partial_transformers=partial_transformers))
        # reference init statistics (beat_tracker.py:170-186); inference-only, so plain tensors (``init_weights`` draws others)
        init = random_state_dict(self.hparams, seed=0, style="init0")
        for i, name in enumerate(("frontend", "transformer_blocks", "task_heads")):
            self.add_module(name, _Stage(self, i))
        for key in state_dict_shapes(self.hparams):
            _attach(self, key, init[key])
        self._bind_units()
        self.dropout = dict(dropout)
        self.train_settings = TrainSettings()   # every opt-in of the differentiable route
        self._engine = None
        self._packed_versions = ()   # (is frontend, parameter, its _version when the engine was packed)
        # outside autocast: True = every product of the forward on three half MFMAs over hi + lo operand halves
        # (BT_PREC_F32X3: fp32-class results -- 1e-5 at the logits, identical beats -- at 16/3 of the fp32 matrix rate; operands
        # beyond the fp16 range of a hi half are detected and the batch is repeated on the exact path, Engine.forward_stages);
        # False = exact fp32 MFMAs.  True is the default of the module itself since round 5: load_model()
        # -- what hubconf.py exports as ``beat_this`` and what pl_module.py hands to split_predict_aggregate -- returns a
        # model on the same precision the inference classes run (a bfloat16 build has no hi + lo path: exact there).
        self.fp32_split_gemms = True
        self.eval()

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_engine"] = None   # (a handle of the HIP library: rebuilt on first use)
        state["_packed_versions"] = ()
        return state

    def __setstate__(self, state):
        if "train_settings" not in state:   # (pickled when every setting was an attribute of its own; the only place that knows)
            state = dict(state)
            state["train_settings"] = TrainSettings.from_loose_attributes(state)
        super().__setstate__(state)
        for name in ("frontend", "transformer_blocks", "task_heads"):
            object.__setattr__(self._modules[name], "_root", weakref.ref(self))
        self._bind_units()

    def _bind_units(self) -> None:
        """Make the reference's callable sub-modules callable here (see _Node)."""
        def bind(node, kind, index=0):
            object.__setattr__(node, "_root", weakref.ref(self))
            node._unit = (kind, index)
        fr = self.frontend
        if "concat" not in fr._modules:   # (parameter-free in the reference: Rearrange("b c f t -> b t (c f)"))
            fr.add_module("concat", _Node())
        bind(fr.stem, "stem")
        bind(fr.blocks, "blocks")
        for i, blk in enumerate(fr.blocks):
            bind(blk, "block", i)
            if "partial" in blk._modules:
                bind(blk.partial, "partial", i)
                # its four leaves are ordinary Attention / FeedForward modules in the reference (beat_tracker.py:251-301)
                for j, (attn, ff) in enumerate((("attnF", "ffF"), ("attnT", "ffT"))):
                    bind(blk.partial._modules[attn], "fattn", 2 * i + j)
                    bind(blk.partial._modules[ff], "fff", 2 * i + j)
        bind(fr.concat, "concat")
        bind(fr.linear, "linear")
        for l, layer in enumerate(self.transformer_blocks.layers):
            bind(layer[0], "attn", l)
            bind(layer[1], "ff", l)
        bind(self.transformer_blocks.norm, "norm")

    def init_weights(self, init_seed: int = 0) -> "BeatThis":
        """The reference's initial state (beat_tracker.py:170-186) drawn under ``init_seed``, written in place: the matrices and
        the convolutions follow the seed; BatchNorm, gains and biases are ones and zeros and ``num_batches_tracked`` 0 whatever
        it is.  Seed 0 is the state a new ``BeatThis`` holds.  (A method, not a constructor argument: the constructor's
        arguments are the architecture, which a checkpoint's hyper-parameters carry one for one; this is none.)"""
        init = random_state_dict(self.hparams, seed=int(init_seed), style="init0")
        with torch.no_grad():
            for key, t in self.state_dict().items():
                t.copy_(init[key])
        self._engine = None
        return self

    # -- state dict plumbing (beat_tracker.py:194-203: strip torch.compile's "_orig_mod.") ----
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        state_dict = {k.replace("_orig_mod.", ""): v for k, v in state_dict.items()}
        self._engine = None
        _TREE_EPOCH[0] += 1   # (assign=True replaces the Parameter objects)
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def _apply(self, fn, *args, **kwargs):
        self._engine = None
        _TREE_EPOCH[0] += 1
        return super()._apply(fn, *args, **kwargs)

    @property
    def device(self) -> torch.device:
        return self.task_heads.beat_downbeat_lin.weight.device

    def _stale(self, frontend_only: bool) -> bool:
        """A parameter that requires grad was changed in place since the engine packed its copy (an optimizer step), or a
        batch-statistics forward moved the running buffers (the kernels write them through raw pointers: no ``_version``
        tells, the route leaves a note instead)."""
        if self.train_settings.stats_moved:
            return True
        for front, p, version in self._packed_versions:
            if p.requires_grad and p._version != version and (front or not frontend_only):
                return True
        return False

    def engine(self, frontend_only: bool = False) -> Engine:
        """The inference engine on packed copies of the parameters; packed again when a trainable parameter changed in place
        (``frontend_only``: the caller runs the frontend alone, whose parameters are frozen)."""
        if self._engine is not None and self._stale(frontend_only):
            self._engine = None
        if self._engine is None:
            dev = self.device
            if dev.type != "cuda":
                raise RuntimeError(
                    f"beat_this_amd.BeatThis has no CPU implementation (parameters are on '{dev}'); "
                    "move the model to a ROCm GPU: model.to('cuda')")
            _lib.lib()  # fail loudly if the HIP library is missing
            self._engine = Engine(PackedModel(self.state_dict(), self.hparams, dev))
            self._packed_versions = tuple((name.startswith("frontend."), p, p._version) for name, p in self.named_parameters())
            self.train_settings.stats_moved = False
        return self._engine

    # -- the opt-ins of the differentiable route: delegates to self.train_settings (settings.TrainSettings has the meanings) --------
    def _set(self, error=ValueError, rates={}, **fields) -> "BeatThis":
        self.train_settings = self.train_settings.changed("model", error, _SETTERS, rates, **fields)
        return self

    def set_frontend_trainable(self, flag: bool = True) -> "BeatThis":
        """The opt-in to the differentiable frontend: ``requires_grad`` of the frontend's weights (not of the rotary tables; the
        BatchNorm buffers stay what they are) becomes ``flag``.  ``False`` restores the frozen state and clears ``batch_statistics``."""
        flag = bool(flag)
        for name, p in self.frontend.named_parameters():
            p.requires_grad_(flag and not name.endswith("rotary_embed.freqs"))
        self._engine = None   # (the re-pack check looks at parameters that require grad only: frozen again, trained weights would stay unpacked)
        return self._set(frontend_trainable=flag, batch_statistics=flag and self.batch_statistics)

    def set_batch_statistics(self, flag: bool = True) -> "BeatThis":
        """The opt-in to training-mode BatchNorm in the differentiable frontend; ``RuntimeError`` on a frozen frontend"""
        return self._set(RuntimeError, batch_statistics=bool(flag))

    def _operand_for(self, which: str, precision: str, operand) -> str:
        """The operand format a precision setter leaves: the one asked for; with None the present one while the part stays
        "16-mixed", else the default "fp16" again"""
        s = self.train_settings
        if operand is not None:
            return operand
        stays = precision == "16-mixed" and getattr(s, which + "_precision") == "16-mixed"
        return getattr(s, which + "_operand") if stays else "fp16"

    def set_train_precision(self, precision: str, operand: str = None) -> "BeatThis":
        """"16-mixed", "32-high" or "32-true" (the default) for the trunk's units on the differentiable route.  "32-high": every
        product of "16-mixed" with each fp32 operand as the sum of two bfloat16 numbers, on three bfloat16 MFMAs (DESIGN.md section
        25).  ``operand``: "fp16" or "bf16", the format the 16-mixed products round their operands to (``train_operand``); None
        keeps it while the precision stays "16-mixed" and otherwise resets it to "fp16"; "bf16" with "32-true" or "32-high" is a
        ``ValueError``"""
        return self._set(train_precision=precision, train_operand=self._operand_for("train", precision, operand))

    def set_frontend_precision(self, precision: str, operand: str = None) -> "BeatThis":
        """"16-mixed", "32-high" or "32-true" (the default) for the differentiable frontend, independent of ``set_train_precision``;
        ``operand`` as there (``frontend_operand``)"""
        return self._set(frontend_precision=precision, frontend_operand=self._operand_for("frontend", precision, operand))

    def enable_dropout(self, seed: int = 0, frontend: bool = False) -> "BeatThis":
        """Opt in to dropout at ``dropout["transformer"]`` under ``seed``, the call counter at 0; ``frontend=True``: a second opt-in,
        the leaves of the differentiable frontend drop at ``dropout["frontend"]``"""
        return self._set(rates={part: self.dropout.get(part, 0.0) for part in ("transformer", "frontend")},
                         dropout_rng={"seed": int(seed), "calls": 0}, frontend_dropout=bool(frontend))

    def disable_dropout(self) -> "BeatThis":
        return self._set(dropout_rng=None, frontend_dropout=False)

    def dropout_state(self):
        """{"seed", "calls"} -- the seed and how many attention / feed-forward calls have drawn masks so far -- or None when
        dropout is not enabled; with the frontend's opt-in also ``"frontend": True``"""
        s = self.train_settings
        return None if s.dropout_rng is None else dict(s.dropout_rng, **({"frontend": True} if s.frontend_dropout else {}))

    def set_dropout_state(self, state: dict) -> None:
        """Enable dropout at ``state`` (what ``dropout_state()`` returned): the next call that drops takes stream ``calls``.
        ``state["frontend"]``, when present, sets the frontend's opt-in; absent, the opt-in stays what it is."""
        self._set(rates={"frontend": self.dropout.get("frontend", 0.0)} if state.get("frontend") else {},
                  dropout_rng={"seed": int(state["seed"]), "calls": int(state["calls"])},
                  frontend_dropout=bool(state.get("frontend", self.train_settings.frontend_dropout)))

    train_precision = property(lambda self: self.train_settings.train_precision)
    frontend_precision = property(lambda self: self.train_settings.frontend_precision)
    train_operand = property(lambda self: self.train_settings.train_operand)
    frontend_operand = property(lambda self: self.train_settings.frontend_operand)
    frontend_trainable = property(lambda self: self.train_settings.frontend_trainable)
    batch_statistics = property(lambda self: self.train_settings.batch_statistics)
    frontend_dropout = property(lambda self: self.train_settings.dropout_rng is not None and self.train_settings.frontend_dropout,
                                doc="The frontend's leaves are opted in to dropout (``enable_dropout(frontend=True)``)")

    # -- which route a call takes (settings.decide), and the differentiable route (backward.py) ------------------------------------
    def _route(self, part: str, node: nn.Module = None, x: torch.Tensor = None, hooks: bool = False):
        """``settings.decide`` for a call of ``part`` issued now, on ``node`` (None: no parameter is asked) with input ``x``;
        ``hooks``: a hook below ``node`` sends the inference path through the modules.  Raises where a frozen frontend was asked
        for gradients.  The parameters, the hooks and the rate are looked at only where the answer can depend on them."""
        s = self.train_settings
        if not torch.is_grad_enabled():
            args = (False,)
        else:
            x_grad = x is not None and x.requires_grad
            look = node is not None and not (s.frontend_trainable if part == "frontend" else x_grad)
            rate = float(self.dropout.get(part, 0.0)) if s.dropout_rng is not None else 0.0
            args = (True, self.training, x_grad, look and _any_requires_grad(node), False, rate)
        route = decide(s, part, *args)
        if hooks and route.how == ENGINE and _hooked_below(node):
            route = decide(s, part, *args[:4], hooked=True)
        if route.how == REFUSE:
            raise NotImplementedError(
                "the frontend is frozen in this version: only transformer_blocks and task_heads are differentiable; "
                "call model.frontend.requires_grad_(False) (or run under torch.no_grad())")
        return route

    def _batch_route(self) -> bool:   # (a frontend call issued now would use batch statistics)
        return self._route("frontend").batch_statistics

    def _next_dropout(self, part: str, active: bool):
        """(p, seed, stream) for one attention / feed-forward call of the differentiable route whose ``part``'s dropout is
        ``active`` (``Route.drop``), else None: a call that does not drop takes no number."""
        if not active:
            return None
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("dropout is active during a graph capture: seed and stream number travel by value, so every replay "
                               "would repeat the masks of the captured step; capture in eval() or after disable_dropout()")
        rng = self.train_settings.dropout_rng
        stream = rng["calls"]
        rng["calls"] = stream + 1
        return float(self.dropout[part]), rng["seed"], stream

    def _rope(self, T: int):
        """The engine's rotary table for ``T`` frames (the table does not depend on anything that is trained)."""
        eng = self._engine if self._engine is not None else self.engine()
        eng.ensure_positions(T)
        return eng.packed._rope_t, int(eng.packed.desc.rope_len)

    def _nothing_to_do(self, x: torch.Tensor, what: str, last=None) -> bool:
        """What every stage and unit call starts with: a (batch, time, ``last``) input on a GPU (``last`` None: any width, and the
        model's own device is the engine's to refuse); True for an empty batch or zero frames"""
        _lib.require_gpu(x, what)
        if last is not None and self.device.type != "cuda":
            self.engine()   # (raises: no CPU implementation)
        if x.dim() != 3 or last not in (None, x.shape[2]):
            raise ValueError(f"expected a (batch, time, {last or 'features'}) input, got {tuple(x.shape)}")
        return x.shape[0] == 0 or x.shape[1] == 0

    def _frontend_train(self, x: torch.Tensor, route) -> torch.Tensor:
        if self._nothing_to_do(x, "stage input", self.hparams["spect_dim"]):
            return _bw.empty_with_graph((x.shape[0], x.shape[1], self.hparams["transformer_dim"]), x, _params_of(self.frontend))
        # the leaves' dropout: asked once per leaf call, in forward order (None where nothing drops)
        drops = (lambda: self._next_dropout("frontend", True)) if route.drop else None
        h = _bw.frontend_train(self, x.to(torch.float32), route.batch_statistics, route.mixed_operand, drops)
        if route.batch_statistics:   # noted AFTER the call: an engine that ``_rope`` packed half way through it is stale as well
            self.train_settings.stats_moved = True
        return h

    def _unit_train(self, x: torch.Tensor, kind: str, node: nn.Module, route) -> torch.Tensor:
        if self._nothing_to_do(x, "sub-module input", self.hparams["transformer_dim"]):
            return _bw.empty_with_graph(x.shape, x, _params_of(node))
        x = x.to(torch.float32)
        if kind == "attn":
            return _bw.attention(node, x, *self._rope(x.shape[1]), self._next_dropout("transformer", route.drop), route.mixed_operand)
        if kind == "ff":
            return _bw.feedforward(node, x, self._next_dropout("transformer", route.drop), route.mixed_operand)
        return _bw.final_norm(node, x)

    def _head_train(self, x: torch.Tensor) -> dict:
        if self._nothing_to_do(x, "stage input", self.hparams["transformer_dim"]):
            params = _params_of(self.task_heads)
            return {"beat": _bw.empty_with_graph(x.shape[:2], x, params), "downbeat": _bw.empty_with_graph(x.shape[:2], x, params)}
        beat, down = _bw.head(self.task_heads, x.to(torch.float32), self.hparams["sum_head"])
        return {"beat": beat, "downbeat": down}

    def forward(self, x: torch.Tensor) -> dict:
        if x.dim() != 3:
            raise ValueError(f"expected (batch, time, {self.hparams['spect_dim']}) input, got {tuple(x.shape)}")
        _lib.require_gpu(x, "model input")
        if torch.is_grad_enabled():
            if self._route("frontend", self.frontend).how == DIFFERENTIABLE:
                # whole-model fine-tuning: the frontend, the trunk and the heads on the differentiable route
                return self.task_heads(self.transformer_blocks(self.frontend(x)))
            if (self._route("transformer", self.transformer_blocks).how == DIFFERENTIABLE
                    or self._route("heads", self.task_heads).how == DIFFERENTIABLE):
                # fine-tuning: the frozen frontend on the fast path, the trunk and the heads on the differentiable route
                with torch.no_grad():
                    h = self.frontend(x)
                return self.task_heads(self.transformer_blocks(h))
        if x.shape[0] == 0 or x.shape[1] == 0:
            empty = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
            return {"beat": empty, "downbeat": empty.clone()}
        if _hooked_below(self):
            # somebody hooked a sub-module: run the stages through the modules so the hooks fire (beat_tracker.py:188-192)
            return self.task_heads(self.transformer_blocks(self.frontend(x)))
        beat, down = self._run(x, 0, 2)
        return {"beat": beat, "downbeat": down}

    def _precision(self) -> int:
        """BT_PREC_* of a forward issued now: half under autocast, else hi + lo (fp32_split_gemms) or exact fp32."""
        half = torch.is_autocast_enabled("cuda") if hasattr(torch, "is_autocast_enabled") else False
        if half:
            return _lib.PREC_HALF
        return _lib.PREC_F32X3 if self.fp32_split_gemms and not _lib.lib().bt_half_is_bf16() else _lib.PREC_F32

    def _run(self, x: torch.Tensor, first: int, last: int, out=None, prec=None, checks=None):
        """Stages first..last in the engine at ``prec`` (BT_PREC_*; None: follows autocast like the whole forward).  ``out``
        (the logits' tensors) and ``checks`` (where the range flag goes; None: looked at now): see Engine.forward_stages."""
        if self._nothing_to_do(x, "stage input"):
            D = self.hparams["transformer_dim"]
            empty = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
            return (empty, empty.clone()) if last == 2 else torch.empty((x.shape[0], x.shape[1], D), dtype=torch.float32, device=x.device)
        prec = self._precision() if prec is None else prec
        return self.engine(frontend_only=last == 0).forward_stages(x, prec, first, last, logits_out=out, checks=checks)

    def _run_unit(self, x: torch.Tensor, kind: str, index: int):
        """A sub-module call (see _Node): reference layouts in and out, fp32 results; precision follows autocast (the hi + lo
        mode of ``fp32_split_gemms`` is the exact fp32 path here)."""
        _lib.require_gpu(x, "sub-module input")
        if kind in ("attn", "ff", "norm"):
            tb = self.transformer_blocks
            node = tb.norm if kind == "norm" else tb.layers[index][0 if kind == "attn" else 1]
            route = self._route("transformer", node, x)
            if route.how == DIFFERENTIABLE:
                return self._unit_train(x, kind, node, route)
        elif self._route("frontend").how == DIFFERENTIABLE:
            raise NotImplementedError(
                "the sub-modules below frontend are inference-only: with set_frontend_trainable() the differentiable route is "
                "model(x) / model.frontend(x); call this node under torch.no_grad()")
        half = torch.is_autocast_enabled("cuda") if hasattr(torch, "is_autocast_enabled") else False
        prec = _lib.PREC_HALF if half else _lib.PREC_F32
        eng = self.engine()
        D = self.hparams["transformer_dim"]

        def to_btfc(t, i):   # (b, c, f, t) of frontend block i's input -> this library's (b, t, f, c)
            c, f = 32 << i, 32 >> i
            if t.dim() != 4 or t.shape[1] != c or t.shape[2] != f:
                raise ValueError(f"expected a (batch, {c}, {f}, time) input, got {tuple(t.shape)}")
            return t.permute(0, 3, 2, 1).contiguous()

        def partial(t, i):   # (b, t, f, c) -> (b, t, f, c)
            if not self.hparams["partial_transformers"]:
                return t
            return eng.forward_unit(t, prec, _lib.UNIT_PARTIAL, i, t.shape)

        def conv(t, i):      # (b, t, f, c) -> (b, t, f / 2, 2 c)
            b, n, f, c = t.shape
            return eng.forward_unit(t, prec, _lib.UNIT_CONV, i, (b, n, f // 2, 2 * c))

        if kind == "stem":
            if x.dim() != 3 or x.shape[2] != 128:
                raise ValueError(f"expected a (batch, time, 128) input, got {tuple(x.shape)}")
            return eng.forward_unit(x, prec, _lib.UNIT_STEM, 0, (x.shape[0], x.shape[1], 32, 32)).permute(0, 3, 2, 1)
        if kind == "partial":
            return partial(to_btfc(x, index), index).permute(0, 3, 2, 1)
        if kind == "block":
            blk = self.frontend.blocks[index]
            if _hooked_below(blk) and "partial" in blk._modules:   # (through the module: a hook on .partial fires)
                return conv(to_btfc(blk.partial(x), index), index).permute(0, 3, 2, 1)
            return conv(partial(to_btfc(x, index), index), index).permute(0, 3, 2, 1)
        if kind == "blocks":
            if _hooked_below(self.frontend.blocks):
                for blk in self.frontend.blocks:
                    x = blk(x)
                return x
            t = to_btfc(x, 0)
            for i in range(3):
                t = conv(partial(t, i), i)
            return t.permute(0, 3, 2, 1)
        if kind == "concat":
            if x.dim() != 4:
                raise ValueError(f"expected a (batch, channels, freq, time) input, got {tuple(x.shape)}")
            b, c, f, n = x.shape
            return x.permute(0, 3, 1, 2).reshape(b, n, c * f)
        if kind == "linear":
            if x.dim() != 3 or x.shape[2] != 1024:
                raise ValueError(f"expected a (batch, time, 1024) input, got {tuple(x.shape)}")
            b, n, _ = x.shape
            t = x.reshape(b, n, 256, 4).transpose(2, 3).contiguous()   # (c f) -> (f c): the packed weight's column order
            return eng.forward_unit(t, prec, _lib.UNIT_LINEAR, 0, (b, n, D))
        if kind in ("fattn", "fff"):
            # leaves of a PartialFTTransformer: Attention / FeedForward of width C on "(b t) f c" or "(b f) t c" rows; the branch
            # WITHOUT the residual like the main layers' (see below)
            c = 32 << (index >> 1)
            if x.dim() != 3 or x.shape[2] != c:
                raise ValueError(f"expected a (sequences, tokens, {c}) input, got {tuple(x.shape)}")
            xf = x.to(torch.float32).contiguous()
            y = eng.forward_unit(xf, prec, _lib.UNIT_FRONT_ATTN if kind == "fattn" else _lib.UNIT_FRONT_FF, index, xf.shape)
            return y - xf
        if x.dim() != 3 or x.shape[2] != D:
            raise ValueError(f"expected a (batch, time, {D}) input, got {tuple(x.shape)}")
        if kind == "norm":
            return eng.forward_unit(x, prec, _lib.UNIT_NORM, 0, x.shape)
        # Attention / FeedForward return their branch WITHOUT the residual (roformer.py:176-181 adds it); the engine computes
        # the residual form x + f(x) in fp32, so f(x) is that minus x (exact to the rounding of the fp32 sum)
        xf = x.to(torch.float32).contiguous()
        y = eng.forward_unit(xf, prec, _lib.UNIT_ATTN if kind == "attn" else _lib.UNIT_FF, index, xf.shape)
        return y - xf
