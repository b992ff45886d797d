"""``EngineTrainer`` -- what the five trainers share on top of the ``BaseTrainer`` template: the ``dataloader=`` / ``val_dataloader=``
constructor, the algorithm and model, the injected or synthetic loader, FlatAdam, the iteration schedule with linear warm-up, the fused
train step under a dynamic loss scale, and the validation-loss loop.  A trainer names its classes (``algorithm_cls``, ``step_cls``), its
metrics, its ``synthetic_loader()``, its ``train_loop`` and the loss of one validation batch (``validation_loss``); what a model does
differently it overrides."""
from typing import Dict

import torch

from computervision.pytorch_amd.optim import FlatAdamW, FlatSGD
from computervision.pytorch_amd.train import DynamicLossScale, FlatAdam
from core.trainer.base import BaseTrainer, LinearWarmup


# cfg.optimizer options beyond the reference's `name`, with their defaults; `freeze` is read from cfg.train
OPTIMIZER_OPTIONS = dict(momentum=0.937, nesterov=True, weight_decay=0.0, groups=None, bias_lr_scale=1.0, clip_grad_norm=None)


def get_optimizer(optimizer_name, model, initial_lr, cfg=None):
    """Without ``cfg`` this is the reference's function (core/trainer/lr_scheduler.py:37-43): Adam only, ``FlatAdam``, any other name raises --
    the call ``EngineTrainer.set_optimizer`` makes, so the five trainers accept what they accepted before.  With ``cfg`` it also builds
    ``FlatSGD`` ("sgd") and ``FlatAdamW`` ("adamw") from ``OPTIMIZER_OPTIONS`` in ``cfg.optimizer`` and ``cfg.train.freeze``; "adam" with none
    of them set is still ``FlatAdam``, with any of them ``FlatAdamW`` with its weight decay (0 by default)."""
    name = optimizer_name.lower()
    if name not in (("adam", "adamw", "sgd") if cfg is not None else ("adam",)):
        raise ValueError(f"{optimizer_name} is not supported")
    group, train = getattr(cfg, "optimizer", None), getattr(cfg, "train", None)
    opts = {k: getattr(group, k, d) for k, d in OPTIMIZER_OPTIONS.items()}
    freeze = tuple(getattr(train, "freeze", ()) or ())
    asked = freeze or any(hasattr(group, k) for k in OPTIMIZER_OPTIONS)
    if name == "adam" and not asked:
        return FlatAdam(model, lr=initial_lr)
    shared = dict(weight_decay=opts["weight_decay"], groups=opts["groups"], bias_lr_scale=opts["bias_lr_scale"], freeze=freeze,
                  clip_grad_norm=opts["clip_grad_norm"])
    if name == "sgd":
        return FlatSGD(model, lr=initial_lr, momentum=opts["momentum"], nesterov=opts["nesterov"], **shared)
    return FlatAdamW(model, lr=initial_lr, **shared)


class EngineTrainer(BaseTrainer):
    algorithm_cls = None                    # the core.algorithms class, built from (cfg, device)
    step_cls = None                         # the fused train step: step_cls(model, criterion, optimizer, scaler=...)
    metric_names, show_option = ["loss"], [True]
    use_iter_milestones = True              # cfg.train.milestones are epochs (BaseTrainer converts them); False: iterations already

    def __init__(self, cfg, device, dataloader=None, val_dataloader=None):
        self._injected_loader, self._injected_val_loader = dataloader, val_dataloader
        super().__init__(cfg, device, self.use_iter_milestones)
        cls = type(self)
        self.metric_names, self.show_option = list(cls.metric_names), list(cls.show_option)     # BaseTrainer's constructor empties the first

    def set_model_algorithm(self):
        self.model_algorithm = self.algorithm_cls(self.cfg, self.device)

    def initialize_model(self):
        self.model, self.model_name = self.model_algorithm.build_model()
        self.model.to(device=self.device)

    def synthetic_loader(self):
        """The seeded stand-in for the model's dataset + collate, used when no ``dataloader=`` is given"""
        raise NotImplementedError

    def load_data(self):
        loader = self._injected_loader or self.synthetic_loader()
        self.train_dataloader = loader
        self.val_dataloader = self._injected_val_loader if self._injected_val_loader is not None else loader

    def set_optimizer(self):
        self.optimizer = get_optimizer(self.optimizer_name, self.model, self.initial_lr)

    def set_lr_scheduler(self):
        """EnhancedMultiStepLR over ITERATION milestones + LinearWarmup (reference yolo8_train.py:76-88, lr_scheduler.py:87-91: an empty
        milestone list means 'never')."""
        milestones = list(self.milestones) or [int(1e8), int(1e8) + 1]
        self.lr_scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optimizer, milestones=milestones, gamma=self.gamma,
                                                                 last_epoch=self.last_iter if self.last_iter > 0 else -1)
        if self.warmup_iters > 0:
            self.warmup_scheduler = LinearWarmup(self.optimizer, warmup_period=self.warmup_iters,
                                                 last_step=self.last_iter if self.last_iter > 0 else -1)

    def set_criterion(self):
        self.criterion = self.model_algorithm.build_loss()
        scaler = DynamicLossScale(self.device, init_scale=self.model.loss_scale) if self.mixed_precision else None   # GradScaler()
        self._step = self.step_cls(self.model, self.criterion, self.optimizer, scaler=scaler)

    def validation_loss(self, model, images, targets):
        """The criterion's scalar for one batch of ``val_dataloader`` under ``model`` (in eval mode, no gradient)"""
        raise NotImplementedError

    def evaluate_loop(self) -> Dict:
        model = self.eval_model                        # the weight average when cfg.train.ema is on
        model.eval()
        total, n = 0.0, 0
        with torch.no_grad():
            for images, targets in self.val_dataloader:
                total += float(self.validation_loss(model, images, targets))
                n += 1
        return {"val_loss": total / max(n, 1)}
