"""``Yolo8Trainer`` -- registered as ``trainer_yolo8_det`` like the reference's
(core/trainer/yolo8_train.py:19-129).  ``train_loop`` keeps the reference's step semantics
(zero_grad -> forward -> loss -> backward -> Adam over all parameters, :93-111) and runs it as the
engine's fused step; with ``torch.distributed`` initialised the step also averages gradients (RCCL).
``dataloader=`` takes a ``DeviceAugLoader(fmt="yolo8")`` or any iterable of yolo8_collate's format; ``evaluate_loop`` runs on
``val_dataloader=`` when one is given (``DeviceAugmenter(train=False)``), else on the training loader.
"""
from typing import List

import torch

from computervision.pytorch_amd.train import DynamicLossScale, FusedTrainStep
from core.algorithms.yolo_v8 import YOLOv8
from core.trainer.engine_trainer import EngineTrainer
from registry import trainer_registry


class SyntheticDetectionLoader:
    """Seeded stand-in for DetectionDataset + yolo8_collate (core/data/collate.py:17-29): yields
    ``(images (B,3,H,W) in [0,1), {"batch_idx","cls","bboxes"})``."""

    def __init__(self, batch_size, hw, num_classes, length=64, boxes_per_img=3, seed=1):
        self.b, self.hw, self.nc, self.length, self.k, self.seed = batch_size, hw, num_classes, length, boxes_per_img, seed

    def __len__(self):
        return self.length

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        for _ in range(self.length):
            n = self.b * self.k
            images = torch.rand(self.b, 3, *self.hw, generator=g)
            cls = torch.randint(0, self.nc, (n, 1), generator=g).float()
            boxes = torch.cat((torch.rand(n, 2, generator=g) * 0.5 + 0.25, torch.rand(n, 2, generator=g) * 0.3 + 0.1), 1)
            yield images, {"batch_idx": torch.arange(self.b).repeat_interleave(self.k).float(), "cls": cls, "bboxes": boxes}


@trainer_registry("yolo8_det")
class Yolo8Trainer(EngineTrainer):
    algorithm_cls = YOLOv8

    def synthetic_loader(self):
        return SyntheticDetectionLoader(self.batch_size, self.input_image_size[1:], self.cfg.dataset.num_classes)

    def set_criterion(self):
        self.criterion = self.model_algorithm.build_loss(model=self.model)
        eng_cfg = self.cfg.engine
        scaler = None
        if self.mixed_precision and getattr(eng_cfg, "dynamic_loss_scale", False) and not getattr(eng_cfg, "graph_capture", False):
            scaler = DynamicLossScale(self.device, init_scale=getattr(eng_cfg, "init_loss_scale", 65536.0))
        self._step = FusedTrainStep(self.model, self.criterion, self.optimizer, n_buckets=getattr(eng_cfg, "allreduce_buckets", 4),
                                    scaler=scaler)

    def train_loop(self, batch_data, scaler) -> List:
        images = batch_data[0].to(self.device, non_blocking=True)
        items = self._step(images, batch_data[1])
        return [items.sum() * images.shape[0]]          # the reference's scalar: sum(box,cls,dfl) * batch

    def validation_loss(self, model, images, targets):
        return self.criterion(model(images.to(self.device)), targets)[0]
