"""The plumbing every engine-backed model family shares: arena layout, arena model, train-step frame.

A model here holds no compute.  Its parameters live in ONE flat fp32 arena (``param``), its BatchNorm running statistics in a second
one (``stat``), every ``num_batches_tracked`` in an int64 one (``nbt``), and the gradients in a fourth (``grad``) that has the
parameter arena's offsets and exists once something asks for it.  Every ``state_dict`` entry is a strided view of an arena, under the
reference's key, shape and order, so reference checkpoints load and torch optimisers see ordinary parameters; the engine
(``engine.Engine``, one per input size and device) binds the arenas by pointer and runs the whole graph.  Moving the model moves the
arenas and rebuilds the views.  There is no CPU path: a model on the CPU raises when it is run.

* ``ArenaLayout`` hands out arena offsets and records the ``state_dict`` slots and the per-convolution ``spec`` dicts the graph
  builders read.  (YOLOv8's ``graph.ParamLayout`` fuses sibling convolutions and is built differently; it offers the same attributes.)
* ``ArenaModel`` owns the arenas, the views, the engine cache, the forward and the ONE engine backward with its gradient-arena
  bookkeeping.  A family overrides the graph builder, the engine cache key, the post-bind hook, the input check,
  ``_init_like_reference`` and ``ctor_args``.
* ``EngineTrainStep`` owns what the fused train steps share: the constructor with the world-size detection, the backward with or
  without the overlapped gradient exchange, and the finite check / Adam / loss-scale tail.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List

import torch
import torch.nn as nn

from . import _lib as L
from .ema import clone_model
from .engine import Engine, check_finite
from .graph import TensorSlot


class ArenaLayout:
    """Arena offsets for every tensor of a reference ``state_dict`` (same keys, shapes, order); offsets and sizes are multiples of 4."""

    def __init__(self):
        self.slots: "OrderedDict[str, TensorSlot]" = OrderedDict()
        self.nbt_keys: List[str] = []
        self.convs: Dict[str, dict] = {}                # conv key -> offsets for the engine op
        self._p = self._s = 0

    def _take(self, arena, n):
        if arena == "param":
            off, self._p = self._p, (self._p + n + 3) & ~3
        else:
            off, self._s = self._s, (self._s + n + 3) & ~3
        return off

    def conv(self, key, cout, cin, k, bias=False, w_off=None, b_off=None, **spec_extra):
        """conv (+ optional bias) whose weights the engine reads as [cout][kh][kw][cin], cout padded to 8; ``w_off`` / ``b_off`` place it
        inside a block taken by the caller; ``spec_extra`` (stride, pad, dil) goes into the spec as given."""
        ce = (cout + 7) & ~7
        spec = dict(cout=cout, cout_eng=ce, cin=cin, k=k, **spec_extra, w_off=self._take("param", ce * k * k * cin) if w_off is None else w_off)
        self.slots[key + ".weight"] = TensorSlot("param", spec["w_off"], (cout, cin, k, k), (k * k * cin, 1, k * cin, cin))
        if bias:
            spec["bias_off"] = self._take("param", ce) if b_off is None else b_off
            self.slots[key + ".bias"] = TensorSlot("param", spec["bias_off"], (cout,), (1,))
        self.convs[key] = spec
        return spec

    def bn(self, key, c, spec):
        spec.update(gamma_off=self._take("param", c), beta_off=self._take("param", c), rmean_off=self._take("stat", c),
                    rvar_off=self._take("stat", c))
        self.slots[key + ".weight"] = TensorSlot("param", spec["gamma_off"], (c,), (1,))
        self.slots[key + ".bias"] = TensorSlot("param", spec["beta_off"], (c,), (1,))
        self.slots[key + ".running_mean"] = TensorSlot("stat", spec["rmean_off"], (c,), (1,), False)
        self.slots[key + ".running_var"] = TensorSlot("stat", spec["rvar_off"], (c,), (1,), False)
        self.slots[key + ".num_batches_tracked"] = TensorSlot("nbt", len(self.nbt_keys), (), (), False)
        self.nbt_keys.append(key + ".num_batches_tracked")

    def conv_bn(self, ckey, bkey, cout, cin, k, **spec_extra):
        self.bn(bkey, cout, self.conv(ckey, cout, cin, k, **spec_extra))

    def _finish(self):
        self.n_params = (self._p + 3) & ~3
        self.n_stats = (self._s + 3) & ~3

    def views(self, arena, which="param"):
        """{state_dict key: strided view of `arena`} for the slots of one arena ("param" or "stat")."""
        return {k: torch.as_strided(arena, sl.shape, sl.strides, sl.offset) for k, sl in self.slots.items() if sl.arena == which}


class _Holder(nn.Module):
    """A module that only owns tensors; compute happens in the engine."""

    def forward(self, *a, **k):  # pragma: no cover
        raise L.CvxError(f"{type(self).__name__} has no standalone forward: the engine executes the whole graph (call the model that owns it)")


class ArenaModel(nn.Module):
    """An ``nn.Module`` whose parameters and buffers are views of the flat arenas of ``layout`` (module docstring)."""

    bn_eps_momentum = (1e-5, 0.1)        # nn.BatchNorm2d's defaults
    _bind_grads_in_eval = False          # an eval-mode engine gets the gradient arena only if one exists already

    def __init__(self, layout, num_classes: int, loss_scale: float):
        super().__init__()
        self.layout = layout
        self.num_classes = num_classes
        self.loss_scale = float(loss_scale)
        n_bn = sum(1 for key in layout.slots if key.endswith(".running_mean"))
        self._flat = {"param": torch.zeros(layout.n_params), "stat": torch.zeros(layout.n_stats), "nbt": torch.zeros(n_bn, dtype=torch.long),
                      "grad": None}
        self._anchor = torch.zeros(1, requires_grad=True)
        self._grads_attached = False
        self._engines: Dict = {}
        self._build_tree()
        self._attach_views()
        self._init_like_reference()

    __deepcopy__ = clone_model       # copy.deepcopy(model): arenas copied, views rebuilt (ema.py)

    # ---- what a family provides ------------------------------------------------------------------------------
    def _build_graph(self, h: int, w: int):
        raise NotImplementedError

    def _init_like_reference(self):
        raise NotImplementedError

    def ctor_args(self) -> dict:
        """The keyword arguments that construct a model like this one (``ema.clone_model``)."""
        return dict(num_classes=self.num_classes, loss_scale=self.loss_scale)

    def _engine_key(self, h, w, dev):
        return (h, w, dev)

    def _after_bind(self, eng):
        pass

    def _check_input(self, x, training):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("expected images of shape (B, 3, H, W)")

    # ---- arenas <-> module tree ------------------------------------------------------------------------------
    def _build_tree(self):
        """Parameter holders under the reference's module names (state_dict keys / order)."""
        for key in self.layout.slots:
            mod = self
            for name in key.split(".")[:-1]:
                if name not in mod._modules:
                    mod.add_module(name, _Holder())
                mod = mod._modules[name]

    def _attach_views(self):
        for key, sl in self.layout.slots.items():
            mod = self
            parts = key.split(".")
            for name in parts[:-1]:
                mod = mod._modules[name]
            if sl.arena == "nbt":
                mod._buffers[parts[-1]] = self._flat["nbt"][sl.offset]
                continue
            view = torch.as_strided(self._flat[sl.arena], sl.shape, sl.strides, sl.offset)
            if sl.trainable:
                old = mod._parameters.get(parts[-1])
                mod._parameters[parts[-1]] = nn.Parameter(view, requires_grad=True if old is None else old.requires_grad)
            else:
                mod._buffers[parts[-1]] = view
        self._grads_attached = False

    def _apply(self, fn, recurse=True):
        """Move / cast the ARENAS, then rebuild every parameter and buffer as a view of them; the gradient arena is dropped."""
        moved = {k: fn(self._flat[k]) for k in ("param", "stat", "nbt")}
        if moved["param"].dtype != torch.float32 or moved["stat"].dtype != torch.float32:
            raise L.CvxError("the engine keeps fp32 master parameters; half()/bfloat16() are not supported (compute is fp16 inside)")
        for k, t in moved.items():
            self._flat[k] = (t.long() if k == "nbt" else t).contiguous()
        self._flat["grad"] = None
        self._anchor = fn(self._anchor.detach()).requires_grad_(True)
        self._attach_views()
        self._engines.clear()
        return self

    @property
    def flat_params(self) -> torch.Tensor:
        return self._flat["param"]

    @property
    def flat_stats(self) -> torch.Tensor:
        return self._flat["stat"]

    @property
    def flat_grads(self) -> torch.Tensor:
        if self._flat["grad"] is None or self._flat["grad"].device != self._flat["param"].device:
            self._flat["grad"] = torch.zeros_like(self._flat["param"])
            self._grads_attached = False
        return self._flat["grad"]

    def attach_grads(self):
        """Make ``p.grad`` of every parameter a view of the flat gradient arena (torch optimisers / GradScaler)."""
        g = self.flat_grads
        modules = dict(self.named_modules())
        for key, slot in self.layout.slots.items():
            if not slot.trainable:
                continue
            mod_name, attr = key.rsplit(".", 1)
            modules[mod_name]._parameters[attr].grad = torch.as_strided(g, slot.shape, slot.strides, slot.offset)
        self._grads_attached = True

    # ---- engine ------------------------------------------------------------------------------------------------
    def engine_for(self, h: int, w: int) -> Engine:
        dev = self._flat["param"].device
        key = self._engine_key(h, w, dev)
        eng = self._engines.get(key)
        if eng is None:
            if dev.type != "cuda":
                raise L.CvxError(f"{type(self).__name__} runs on an MI355X only: move the model with .to('cuda') first (there is no CPU fallback)")
            eng = Engine(self._build_graph(h, w), dev)
            eng.set_bn(*self.bn_eps_momentum)
            self._engines[key] = eng
        eng.bind(self._flat["param"], self.flat_grads if self.training or self._bind_grads_in_eval else self._flat["grad"], self._flat["stat"])
        self._after_bind(eng)
        return eng

    def _run_forward(self, x: torch.Tensor, training: bool, pred=None) -> torch.Tensor:
        """(B,3,H,W) -> the engine's fp32 head rows (B, rows, row pitch), written to ``pred`` if one is given."""
        self._check_input(x, training)
        eng = self.engine_for(int(x.shape[2]), int(x.shape[3]))
        self._last_engine = eng
        rows = eng.forward(x, training, pred)
        if training:
            self._flat["nbt"] += 1
        return rows

    def _engine_backward(self, dpred: torch.Tensor, loss_scale: float, run_backward=None):
        """Backward of the last forward's engine from ``loss_scale * dLoss/drows`` (fp16): parameter gradients accumulate in the gradient
        arena and every ``p.grad`` is a view of it afterwards.  ``run_backward(eng, dpred, loss_scale)`` replaces the plain
        ``eng.backward`` (the data-parallel steps run it bucket by bucket)."""
        first = next(p for p in self.parameters() if p.requires_grad)
        if first.grad is None:               # optimizer.zero_grad(set_to_none=True) happened (or first step)
            self.flat_grads.zero_()
            self._grads_attached = False
        if run_backward is not None:
            run_backward(self._last_engine, dpred, loss_scale)
        else:
            self._last_engine.backward(dpred, loss_scale)
        if not self._grads_attached or first.grad is None:
            self.attach_grads()


class EngineTrainStep:
    """What the fused train steps share; a family's ``__call__`` is its buffers, its forward and its loss ``op`` between
    ``_begin()`` and ``_backward()`` / ``_update()``."""

    def __init__(self, model, criterion, optimizer, scaler=None, process_group=None, n_buckets: int = 4):
        self.model, self.criterion, self.optimizer, self.scaler = model, criterion, optimizer, scaler
        self.pg, self.n_buckets = process_group, n_buckets
        self.world, self.distributed = 1, False
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(process_group)
            self.distributed = True     # a 1-rank group still exercises the RCCL exchange path
        self._side = None

    def _begin(self) -> float:
        """-> the loss scale of this step (the scaler's, or the model's static one)"""
        if not self.model.training:
            raise L.CvxError(f"{type(self).__name__}: call model.train() first")
        self.optimizer.sync_lr()
        return self.scaler.begin_step() if self.scaler is not None else self.model.loss_scale

    def _backward(self, eng, dpred, scale):
        m = self.model
        if self.distributed and m.flat_params.device.type == "cuda":   # gradient exchange overlapped with the backward pass, bucket by bucket
            if self._side is None:
                from .train import OverlappedExchange
                self._side = OverlappedExchange(self.pg, self.n_buckets)
            self._side.backward(eng, m.flat_grads, dpred, scale)
        else:
            eng.backward(dpred, scale)

    def _update(self):
        """GradScaler.step (skip the update when a gradient is not finite), the optimiser step with the mean's 1/world folded in, zeroed
        gradients.  An optimiser that clips measures the global norm first, and that launch raises ``found_inf`` on a norm that is not
        finite: no ``check_finite`` of its own then."""
        if self.scaler is not None:
            if getattr(self.optimizer, "clip_grad_norm", None) is None:
                check_finite(self.model.flat_grads, self.scaler.found_inf)
            self.optimizer.found_inf = self.scaler.found_inf
        self.optimizer.step(zero_grad=True, grad_scale=1.0 / self.world)
        if self.scaler is not None:
            self.scaler.end_step()
