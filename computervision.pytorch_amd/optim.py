"""Optimisers with parameter groups on the flat arenas: ``FlatSGD`` and ``FlatAdamW`` over ``cvx_optim_step`` / ``cvx_grad_norm``.

``FlatAdam`` (train.py) stays what the reference's one recipe runs.  These two add what the standard recipes of the five model families
need and the flat-arena step would otherwise give up to ``torch.optim``: weight decay on the weights only, a frozen backbone, clipping
by the global gradient norm -- still one update launch over the arenas, the ``found_inf`` skip on the device, the weight average in the
same pass, and nothing on the host between steps.

* A parameter's group is one byte per 16-byte chunk of the arena (``build_group_map``): arena offsets and sizes are multiples of 4, so a
  chunk belongs to at most one parameter.  255 marks chunks no trainable parameter owns (the zero rows that pad a convolution to the
  engine's channel count, alignment gaps): the kernels leave them alone.  The surplus lanes of a parameter's last chunk (21 or 255
  channels) are alignment padding that moves with its group; nothing reads them.
* ``param_groups`` are real torch groups, one per device group, so ``MultiStepLR`` and ``LinearWarmup`` work unchanged; ``sync_lr`` pushes
  the table of per-group values to the device when one of them changed.
* ``state_dict()`` is the layout of the installed ``torch.optim.SGD`` / ``torch.optim.AdamW`` built with the same grouping.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import engine as E

NO_DECAY_NORM_BIAS = "no_decay_norm_bias"
GROUP_NAMES = {None: ("all",), NO_DECAY_NORM_BIAS: ("weights", "norm", "bias")}


def classify(name: str, ndim: int, groups) -> int:
    """The live group of a parameter: everything in group 0 without grouping; with "no_decay_norm_bias" weights of more than one
    dimension in 0 (decayed), one-dimensional weights (BatchNorm gamma, SSD's L2Normalize scale) in 1, ``.bias`` (convolution biases,
    BatchNorm beta) in 2."""
    if groups is None:
        return 0
    if groups != NO_DECAY_NORM_BIAS:
        raise ValueError(f"groups: None or {NO_DECAY_NORM_BIAS!r}, got {groups!r}")
    if ndim > 1:
        return 0
    return 2 if name.endswith(".bias") else 1


def build_group_map(layout, group_of: Dict[str, int], n_groups: int) -> np.ndarray:
    """uint8 per 16-byte chunk of the parameter arena: ``group_of[key]`` over the logical extent of every trainable slot, 255 elsewhere.
    Raises unless every trainable slot is covered exactly once, on 4-aligned offsets, by an id below ``n_groups``, with no chunk
    claimed twice -- a layout that ever breaks the multiple-of-4 rule is refused here instead of being stepped wrongly."""
    if not 1 <= n_groups <= E.OPTIM_MAX_GROUPS:
        raise L.CvxError(f"1 <= n_groups <= {E.OPTIM_MAX_GROUPS}, got {n_groups}")
    n = int(layout.n_params)
    if n % 4:
        raise L.CvxError(f"the parameter arena holds {n} values, not a multiple of 4")
    gmap = np.full(n // 4, E.OPTIM_UNMAPPED, np.uint8)
    seen = set()
    for key, sl in layout.slots.items():
        if sl.arena != "param" or not sl.trainable:
            continue
        if key not in group_of:
            raise L.CvxError(f"group map: the trainable slot {key} belongs to no group")
        gid = int(group_of[key])
        if not 0 <= gid < n_groups:
            raise L.CvxError(f"group map: {key} has group id {gid}, not below n_groups = {n_groups}")
        numel = int(np.prod(sl.shape)) if len(sl.shape) else 1
        extent = 1 + sum((s - 1) * st for s, st in zip(sl.shape, sl.strides))
        if extent != numel:
            raise L.CvxError(f"group map: the slot {key} is not dense in the arena ({numel} values over {extent})")
        if sl.offset % 4:
            raise L.CvxError(f"group map: the slot {key} starts at offset {sl.offset}, not a multiple of 4: a chunk would have two owners")
        c0, c1 = sl.offset // 4, (sl.offset + numel + 3) // 4
        if c1 > gmap.size:
            raise L.CvxError(f"group map: the slot {key} ends behind the arena")
        if (gmap[c0:c1] != E.OPTIM_UNMAPPED).any():
            raise L.CvxError(f"group map: a chunk of {key} is claimed twice")
        gmap[c0:c1] = gid
        seen.add(key)
    extra = set(group_of) - seen
    if extra:
        raise L.CvxError(f"group map: {sorted(extra)[:4]} are not trainable slots of the parameter arena")
    return gmap


class GroupPlan:
    """Which parameter goes where: ``keys[g]`` the ``named_parameters()`` names of torch group g in model order (the live groups, then the
    frozen group if any parameter stands still), ``names[g]`` its label, ``frozen`` the index of the frozen group or None, ``gmap`` the
    chunk map."""

    def __init__(self, model, groups=None, freeze: Sequence[str] = ()):
        named = list(model.named_parameters())
        if isinstance(freeze, str):
            freeze = (freeze,)
        for prefix in freeze:
            hit = [p for k, p in named if k.startswith(prefix)]
            if not hit:
                raise ValueError(f"freeze: no parameter's state_dict key starts with {prefix!r}")
            for p in hit:
                p.requires_grad_(False)
        live_names = GROUP_NAMES.get(groups)
        if live_names is None:
            raise ValueError(f"groups: None or {NO_DECAY_NORM_BIAS!r}, got {groups!r}")
        self.names: List[str] = list(live_names)
        self.keys: List[List[str]] = [[] for _ in live_names]
        still = [k for k, p in named if not p.requires_grad]
        self.frozen: Optional[int] = None
        if still:
            self.frozen = len(self.names)
            self.names.append("frozen")
            self.keys.append(still)
        for k, p in named:
            if p.requires_grad:
                self.keys[classify(k, p.dim(), groups)].append(k)
        slots = model.layout.slots
        group_of = {k: g for g, keys in enumerate(self.keys) for k in keys if k in slots}     # (YOLOv8's DFL projection owns no slot)
        self.gmap = build_group_map(model.layout, group_of, len(self.names))


def _torch_group_defaults(cls) -> dict:
    """the ``param_groups`` entry the installed ``cls`` writes for default arguments (its keys differ between torch versions)"""
    g = dict(cls([torch.zeros(1, requires_grad=True)], lr=1.0).state_dict()["param_groups"][0])
    g.pop("params")
    return g


class FlatStep(torch.optim.Optimizer):
    """The surface and the step skeleton of every optimiser over a model's flat arenas (``FlatAdam`` in train.py, ``FlatSGD`` and
    ``FlatAdamW`` here): ``step(closure=None, zero_grad=False, grad_scale=1.0)``, ``found_inf``, ``attach_ema``, ``ema_fused``,
    ``zero_grad``, ``device_step()``.  A subclass supplies ``_ensure_state`` (device buffers and ``_state``, whose [1] is the step count),
    ``sync_lr`` and ``_launch``."""

    def __init__(self, model, params, defaults):
        self.model = model
        super().__init__(params, defaults)
        self._step = 0
        self._state = None          # device step state: the step advances on the device
        self.found_inf: Optional[torch.Tensor] = None
        self._ema = None            # attach_ema: a ModelEMA whose average moves with every step()
        self.ema_fused = True       # False: the average as launches of its own after the step (tools/ema_cost.py, tools/optim_cost.py time both)

    def attach_ema(self, ema):
        """Every ``step()`` from now on also moves ``ema`` (a ``ModelEMA`` of this optimiser's model; None detaches it): the parameters inside
        the step kernel, the BatchNorm statistics with one ``cvx_ema_update`` launch, ``ema.updates`` + 1 -- what ``ema.update(model)`` after
        ``optimizer.step()`` does in the reference's loop shape, a step skipped by ``found_inf`` included."""
        if ema is not None:
            ema.check(self.model)
        self._ema = ema

    def _ensure_state(self):
        raise NotImplementedError

    def sync_lr(self):
        """Push what a scheduler changed in ``param_groups`` to the device (call outside graph capture)."""
        raise NotImplementedError

    def _launch(self, zero_grad, grad_scale, ema_arena, d, omd):
        """the step's launches; ``ema_arena``: the average of the parameters to move in the same pass, or None"""
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None, zero_grad: bool = False, grad_scale: float = 1.0):
        self._ensure_state()
        if not torch.cuda.is_current_stream_capturing():
            self.sync_lr()               # a scheduler (or GradScaler.step -> optimizer.step) may have changed param_groups["lr"]
        m = self.model
        self._step += 1                  # host mirror only; the authoritative count lives in the device state
        ema = self._ema
        fused = ema is not None and self.ema_fused
        d = omd = 0.0
        if fused:
            ema.check(m)
            ema.updates += 1
            d, omd = ema.factors()
        self._launch(zero_grad, grad_scale, ema.ema.flat_params if fused else None, d, omd)
        if fused:
            E.ema_update(ema.ema.flat_stats, m.flat_stats, d, omd)
        elif ema is not None:
            ema.update(m)

    def zero_grad(self, set_to_none: bool = True):
        self.model.flat_grads.zero_()

    def device_step(self) -> int:
        """Steps actually applied: read from the device state (skipped steps and graph replays are counted there)."""
        return self._step if self._state is None else int(self._state[1].item())


class FlatOptimizer(FlatStep):
    """What ``FlatSGD`` and ``FlatAdamW`` share: the grouping, the device tables, the launches of a step, the checkpoint layout.

    ``groups``: None (one group, uniform decay -- torch's meaning of a plain parameter list) or ``"no_decay_norm_bias"`` (``classify``);
    ``bias_lr_scale`` multiplies the bias group's learning rate.  ``freeze``: state_dict key prefixes; the matching parameters get
    ``requires_grad_(False)`` and, with every parameter that stands still already (YOLOv8's DFL projection), form a frozen group the step
    leaves bit for bit.  A prefix that matches nothing raises.  As in torch, the BatchNorm running statistics of frozen layers keep moving
    while the model is in train mode.  ``clip_grad_norm``: None or the max norm; the step then launches ``cvx_grad_norm`` first, which also
    raises ``found_inf`` on a non-finite norm; ``last_grad_norm`` is the device scalar, never read by the host here."""

    kind: int = -1
    torch_cls = None
    state_keys: Sequence[str] = ()

    def __init__(self, model, hyper: dict, weight_decay: float, groups, bias_lr_scale: float, freeze, clip_grad_norm):
        if clip_grad_norm is not None and not float(clip_grad_norm) > 0:
            raise ValueError(f"clip_grad_norm: None or a positive max norm, got {clip_grad_norm}")
        self.plan = GroupPlan(model, groups, freeze)
        self.clip_grad_norm = None if clip_grad_norm is None else float(clip_grad_norm)
        named = dict(model.named_parameters())
        lr = hyper["lr"]
        entries = []
        for g, (name, keys) in enumerate(zip(self.plan.names, self.plan.keys)):
            glr = lr * bias_lr_scale if name == "bias" else lr
            wd = weight_decay if name in ("all", "weights") else 0.0
            entries.append(dict(hyper, params=[named[k] for k in keys], lr=glr, initial_lr=glr, weight_decay=wd, name=name, frozen=g == self.plan.frozen))
        super().__init__(model, entries, dict(hyper, weight_decay=weight_decay))
        self._buf1 = self._buf2 = None
        # _state: device [group 0's lr, step, group 0's lr/(1-b1^t), 1/sqrt(1-b2^t)]
        self._gs = None             # device (n_groups, 8) group table
        self._rows_on_device = None
        self._map = self._clip = self._ws = None

    # ---- per-kind pieces ----------------------------------------------------------------------------------------------------------------
    def _row(self, g) -> List[float]:
        """[lr, decay_coupled, decay_factor, frozen, momentum, nesterov] of one param_group"""
        raise NotImplementedError

    def _betas_eps(self):
        return (0.0, 0.0), 0.0

    # ---- device state ---------------------------------------------------------------------------------------------------------------------
    def _rows(self):
        return [[float(v) for v in self._row(g)] for g in self.param_groups]

    def _ensure_state(self):
        p = self.model.flat_params
        if self._buf1 is not None and self._buf1.device == p.device:
            return
        if p.numel() != self.plan.gmap.size * 4:
            raise L.CvxError("the model's parameter arena changed size after the optimiser was built")
        self._buf1 = torch.zeros_like(p)
        self._buf2 = torch.zeros_like(p) if self.kind == E.OPTIM_ADAM else None
        rows = self._rows()
        self._gs = torch.tensor([r + [0.0, 0.0] for r in rows], dtype=torch.float32).to(p.device)
        self._rows_on_device = rows
        self._state = torch.tensor([rows[0][0], float(self._step), 0.0, 0.0], device=p.device)
        self._map = torch.from_numpy(self.plan.gmap).to(p.device)
        self._clip = torch.zeros(4, device=p.device)
        self._ws = torch.zeros(1024, device=p.device)          # cvx_grad_norm_workspace(n) <= 1024

    def sync_lr(self):
        """Push the per-group values a scheduler changed to the device table (call outside graph capture)."""
        self._ensure_state()
        rows = self._rows()
        if rows != self._rows_on_device:
            self._gs[:, :6].copy_(torch.tensor(rows, dtype=torch.float32), non_blocking=False)
            self._rows_on_device = rows

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """The norm the last clipping step measured, on the device (None without clipping or before the first step)."""
        return None if self.clip_grad_norm is None or self._clip is None else self._clip[0]

    def _launch(self, zero_grad, grad_scale, ema_arena, d, omd):
        m = self.model
        clip = None
        if self.clip_grad_norm is not None:
            E.grad_norm(m.flat_grads, self._map, self._gs, self.clip_grad_norm, self._clip, self._ws, grad_scale, self.found_inf)
            clip = self._clip
        betas, eps = self._betas_eps()
        E.optim_step(self.kind, m.flat_params, m.flat_grads, self._buf1, self._buf2, self._map, self._gs, self._state, betas, eps, self.found_inf,
                     zero_grad, grad_scale, clip, ema_arena, d, omd)

    # ---- checkpoint interchange: the installed torch optimiser's state_dict layout ------------------------------------------------------------
    def _buffers(self):
        return [b for b in (self._buf1, self._buf2) if b is not None]

    def _views(self, key):
        """the slices of the flat state arenas that belong to the parameter `key`, in its logical shape (None: it owns no slot)"""
        sl = self.model.layout.slots.get(key)
        if sl is None or sl.arena != "param":
            return None
        return [torch.as_strided(b, sl.shape, sl.strides, sl.offset) for b in self._buffers()]

    def _has_state(self, g) -> bool:
        return not g["frozen"]

    def state_dict(self):
        """``torch_cls``'s layout: one ``param_groups`` entry per group with ``params`` indices in ``model.parameters()`` order, per-parameter
        state in the reference's logical shapes (copies of the flat arenas' slices).  The stock optimiser built with the same grouping loads
        it, and ``load_state_dict`` loads the stock optimiser's."""
        self._ensure_state()
        step = float(self.device_step())
        index = {k: i for i, (k, _) in enumerate(self.model.named_parameters())}
        defaults = _torch_group_defaults(self.torch_cls)
        state, out_groups = {}, []
        for g, keys in zip(self.param_groups, self.plan.keys):
            group = dict(defaults)
            group.update({k: (tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in g.items() if k != "params"})
            group["params"] = [index[k] for k in keys]
            out_groups.append(group)
            if not self._has_state(g) or (self.kind == E.OPTIM_ADAM and step == 0):
                continue
            for k in keys:
                views = self._views(k)
                if views is None:
                    continue
                st = {name: v.detach().clone().contiguous() for name, v in zip(self.state_keys, views)}
                if self.kind == E.OPTIM_ADAM:
                    st = dict(step=torch.tensor(step), **st)
                state[index[k]] = st
        return {"state": state, "param_groups": out_groups}

    def load_state_dict(self, sd):
        """Accepts ``state_dict()`` above and the stock ``torch_cls``'s, built with the same grouping: as in torch, the saved ids are matched
        to the parameters by position, group by group."""
        saved = sd["param_groups"]
        if len(saved) != len(self.param_groups) or any(len(s["params"]) != len(k) for s, k in zip(saved, self.plan.keys)):
            raise L.CvxError(f"optimizer checkpoint: {[len(s['params']) for s in saved]} parameters per group, this optimiser has "
                             f"{[len(k) for k in self.plan.keys]}")
        for g, s in zip(self.param_groups, saved):
            g.update({k: v for k, v in s.items() if k != "params"})
        key_of = {i: k for s, keys in zip(saved, self.plan.keys) for i, k in zip(s["params"], keys)}
        self._ensure_state()
        for b in self._buffers():
            b.zero_()
        step = 0
        shapes = {k: tuple(p.shape) for k, p in self.model.named_parameters()}
        for i, st in sd.get("state", {}).items():
            key = key_of.get(int(i))
            if key is None:
                raise L.CvxError(f"optimizer checkpoint has state for parameter {i}, which no group lists")
            views = self._views(key)
            if views is None:
                continue
            for name, view in zip(self.state_keys, views):
                t = st.get(name)
                if t is None:                                   # torch.optim.SGD before its first step with momentum
                    continue
                if tuple(t.shape) != shapes[key]:
                    raise L.CvxError(f"optimizer checkpoint: {name} of {key} has shape {tuple(t.shape)}, the model's is {shapes[key]}")
                view.copy_(t)
            if "step" in st:
                step = max(step, int(float(st["step"])))
        self._step = max(step, int(sd.get("flat_step", 0)))
        rows = self._rows()
        self._gs.copy_(torch.tensor([r + [0.0, 0.0] for r in rows], dtype=torch.float32))
        self._rows_on_device = rows
        self._state.copy_(torch.tensor([rows[0][0], float(self._step), 0.0, 0.0]))


class FlatSGD(FlatOptimizer):
    """``torch.optim.SGD`` (dampening 0) over the flat arenas: momentum, Nesterov, weight decay added to the gradient.  Arguments as
    ``FlatOptimizer``'s."""

    kind = E.OPTIM_SGD
    torch_cls = torch.optim.SGD
    state_keys = ("momentum_buffer",)

    def __init__(self, model, lr=1e-3, momentum=0.0, nesterov=False, weight_decay=0.0, groups=None, bias_lr_scale=1.0, freeze=(),
                 clip_grad_norm=None):
        if nesterov and not momentum > 0:
            raise ValueError("Nesterov momentum requires a momentum")
        super().__init__(model, dict(lr=lr, momentum=momentum, dampening=0, nesterov=bool(nesterov)), weight_decay, groups, bias_lr_scale, freeze,
                         clip_grad_norm)

    def _row(self, g):
        return [g["lr"], g["weight_decay"], 1.0, 1.0 if g["frozen"] else 0.0, g["momentum"], 1.0 if g["nesterov"] else 0.0]

    def _has_state(self, g):
        return not g["frozen"] and g["momentum"] != 0      # torch keeps no buffer without momentum

    def state_dict(self):
        sd = super().state_dict()
        sd["flat_step"] = self.device_step()                # torch.optim.SGD counts no steps; its load_state_dict ignores the extra entry
        return sd


class FlatAdamW(FlatOptimizer):
    """``torch.optim.AdamW`` over the flat arenas: ``cvx_adam_step_dev``'s Adam after ``param.mul_(1 - lr * weight_decay)``; with
    ``weight_decay=0`` it is Adam with groups, freezing and clipping.  Coupled L2 is not offered.  Arguments as ``FlatOptimizer``'s."""

    kind = E.OPTIM_ADAM
    torch_cls = torch.optim.AdamW
    state_keys = ("exp_avg", "exp_avg_sq")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, groups=None, bias_lr_scale=1.0, freeze=(),
                 clip_grad_norm=None):
        super().__init__(model, dict(lr=lr, betas=tuple(betas), eps=eps), weight_decay, groups, bias_lr_scale, freeze, clip_grad_norm)

    def _row(self, g):
        return [g["lr"], 0.0, decay_factor(g["lr"], g["weight_decay"]), 1.0 if g["frozen"] else 0.0, 0.0, 0.0]

    def _betas_eps(self):
        g = self.param_groups[0]                             # one moment recurrence for the whole arena: betas and eps are not per group
        return tuple(g["betas"]), g["eps"]


def decay_factor(lr: float, weight_decay: float) -> float:
    """the fp32 value of the double ``1 - lr * weight_decay``: what ``param.mul_(1 - lr * wd)`` multiplies an fp32 tensor by"""
    return float(np.float32(1.0 - float(lr) * float(weight_decay)))
