"""Weight averaging: the reference's ``ModelEMA`` (core/trainer/lr_scheduler.py:46-84) on the flat arenas.

* ``clone_model`` -- a second model of the same class and constructor arguments whose three arenas are copies and whose
  parameters and buffers are views of those copies.  ``copy.deepcopy`` of an ``nn.Module`` copies tensor by tensor, which
  leaves the copy's parameters detached from the copy's own arenas -- the arenas the engine binds -- so every model class
  routes ``__deepcopy__`` here, and the reference's ``deepcopy(model).eval()`` idiom gives a working model.
* ``ModelEMA`` -- the reference's surface (``.ema``, ``.updates``, ``.decay(x)``, ``.update(model)``, ``.update_attr``).
  ``update`` is two ``cvx_ema_update`` launches, one per floating-point arena, instead of two torch kernels per
  ``state_dict`` entry; ``num_batches_tracked`` is not floating-point and keeps the value it was cloned with, as in the
  reference.  ``FlatAdam.attach_ema`` (train.py) folds the parameter half into the Adam pass.

The recurrence, as the reference's ``v *= d; v += (1 - d) * msd[k]`` computes it in fp32::

    e_new = rn( rn(e * float(d)) + rn(float(1 - d) * p) ),   d = decay * (1 - exp(-updates / tau)) in double precision

One deliberate difference: tensors that live outside the arenas (YOLOv8's fixed DFL weight ``arange(16)``) are constants;
the clone keeps them exactly, where the reference's in-place arithmetic may move such a value by one rounding.
"""
from __future__ import annotations

import math

import torch

from . import _lib as L
from .engine import ema_update

_ARENAS = ("param", "stat", "nbt")


def clone_model(model, memo=None):
    """A model of the same class, constructor arguments, device and mode whose ``param`` / ``stat`` / ``nbt`` arenas are copies of
    ``model``'s; its parameters and buffers are views of those copies.  It has no engines and no gradient arena until it is run.
    (The signature doubles as ``__deepcopy__``.)"""
    from .arena import ArenaModel
    if not isinstance(model, ArenaModel):
        raise L.CvxError(f"clone_model: {type(model).__name__} is not one of the engine-backed models (an arena.ArenaModel)")
    with torch.random.fork_rng(devices=[]):          # the constructor draws an initialisation: not from the caller's stream
        clone = type(model)(**model.ctor_args())
    clone.to(model.flat_params.device)
    with torch.no_grad():
        for k in _ARENAS:
            src, dst = model._flat[k], clone._flat[k]
            if src.shape != dst.shape:
                raise L.CvxError(f"clone_model: the {k} arena of the clone has {dst.numel()} values, the model's {src.numel()}")
            dst.copy_(src)
    own = dict(clone.named_parameters())
    for name, p in model.named_parameters():
        own[name].requires_grad_(p.requires_grad)
    if hasattr(model, "seed"):
        clone.seed = model.seed
    clone.train(model.training)
    if memo is not None:
        memo[id(model)] = clone
    return clone


def _arenas_match(a, b):
    return all(a._flat[k].shape == b._flat[k].shape for k in _ARENAS)


class ModelEMA:
    """Exponential moving average of every floating-point ``state_dict`` entry, with the ramped decay
    ``d = decay * (1 - exp(-updates / tau))`` (core/trainer/lr_scheduler.py:55-80)."""

    def __init__(self, model, decay=0.9999, tau=2000, updates=0):
        self.ema = clone_model(model).eval()
        self.updates = updates
        self.decay = lambda x: decay * (1 - math.exp(-x / tau))
        for p in self.ema.parameters():
            p.requires_grad_(False)

    def factors(self):
        """(d, 1 - d) of the current ``updates``, in double precision; the kernels take them cast to fp32."""
        d = self.decay(self.updates)
        return d, 1 - d

    def check(self, model):
        if not _arenas_match(self.ema, model):
            raise L.CvxError(f"ModelEMA: {type(model).__name__}'s arenas do not have the shapes of the averaged {type(self.ema).__name__}'s")
        if not model.flat_params.is_cuda or not self.ema.flat_params.is_cuda:
            raise L.CvxError("ModelEMA.update runs on an MI355X only: move the model with .to('cuda') before the average is made "
                             "(there is no CPU fallback)")
        if model.flat_params.device != self.ema.flat_params.device:
            raise L.CvxError(f"ModelEMA: the model is on {model.flat_params.device}, its average on {self.ema.flat_params.device}")

    def update(self, model):
        self.check(model)
        self.updates += 1
        d, omd = self.factors()
        ema_update(self.ema.flat_params, model.flat_params, d, omd)
        ema_update(self.ema.flat_stats, model.flat_stats, d, omd)

    def update_attr(self, model, include=(), exclude=("process_group", "reducer")):
        """The reference's copy_attr (lr_scheduler.py:46-52, 82-84); ``training`` is never copied: the average stays in eval mode."""
        for k, v in model.__dict__.items():
            if (len(include) and k not in include) or k.startswith("_") or k in exclude or k == "training":
                continue
            setattr(self.ema, k, v)

    def state_dict(self):
        return {"model": {k: v.detach().cpu().clone() for k, v in self.ema.state_dict().items()}, "updates": int(self.updates)}

    def load_state_dict(self, sd):
        self.ema.load_state_dict(sd["model"])
        self.updates = int(sd["updates"])

    def restart_from(self, model):
        """The average starts over from ``model``'s present weights (a checkpoint without an average was resumed)."""
        if not _arenas_match(self.ema, model):
            raise L.CvxError("ModelEMA.restart_from: different arenas")
        with torch.no_grad():
            for k in _ARENAS:
                self.ema._flat[k].copy_(model._flat[k])
