"""``Yolo7Trainer`` -- registered as ``trainer_yolo7`` like the reference's (core/trainer/yolo7_train.py).  ``train_loop`` keeps the
reference's step semantics (zero_grad -> forward -> Yolo7Loss(preds, targets, images) -> backward -> Adam under AMP, :79-97) and runs it
as the engine's fused step (``Yolo7TrainStep``: engine forward, ``cvx_yolo7_loss`` -- candidate generation, SimOTA assignment and the loss
terms on the device --, engine backward, fused Adam with GradScaler's skip-on-overflow); with ``torch.distributed`` initialised the step
also sums the gradients over the ranks (RCCL).  The input side is ``DeviceAugLoader(fmt="yolo7")`` (resize, mosaic, HSV and box
arithmetic on the device) or any iterable yielding ``(images, targets (N, 6) [image, class, cx, cy, w, h])`` (yolo7_collate's format) as
``dataloader=``; seeded synthetic batches stand in without one.  ``evaluate_loop`` runs on ``val_dataloader=`` when one is given
(``DeviceAugmenter(train=False)``), else on the training loader."""
from typing import List

import torch

from computervision.pytorch_amd.yolov7 import Yolo7TrainStep
from core.algorithms.yolo_v7 import YOLOv7
from core.trainer.engine_trainer import EngineTrainer
from registry import trainer_registry


class SyntheticYolo7Loader:
    """Seeded stand-in for DetectionDataset + yolo7_collate (core/data/collate.py:5-14): images (B,3,H,W) in [0,1) and targets (N, 6)
    [image index, class, cx, cy, w, h] normalised, grouped by image."""

    def __init__(self, batch_size, hw, num_classes, boxes_per_img=4, length=16, seed=1):
        self.b, self.hw, self.nc, self.k, self.length, self.seed = batch_size, hw, num_classes, boxes_per_img, length, seed

    def __len__(self):
        return self.length

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        for _ in range(self.length):
            images = torch.rand(self.b, 3, *self.hw, generator=g)
            n = self.b * self.k
            t = torch.zeros(n, 6)
            t[:, 0] = torch.arange(self.b).repeat_interleave(self.k).float()
            t[:, 1] = torch.randint(0, self.nc, (n,), generator=g).float()
            t[:, 2:4] = torch.rand(n, 2, generator=g) * 0.7 + 0.15
            t[:, 4:6] = torch.rand(n, 2, generator=g) * 0.4 + 0.05
            yield images, t


@trainer_registry("yolo7")
class Yolo7Trainer(EngineTrainer):
    algorithm_cls, step_cls = YOLOv7, Yolo7TrainStep
    metric_names, show_option = ["loss", "box_loss", "obj_loss", "cls_loss"], [True, True, True, True]

    def synthetic_loader(self):
        return SyntheticYolo7Loader(self.batch_size, self.input_image_size[1:], self.cfg.dataset.num_classes)

    def train_loop(self, batch_data, scaler) -> List:
        images = batch_data[0].to(self.device, non_blocking=True)
        targets = batch_data[1].to(self.device, non_blocking=True)
        items = self._step(images, targets)
        return [items[0], items[1], items[2], items[3]]

    def validation_loss(self, model, images, targets):
        images = images.to(self.device)
        return self.criterion(model(images), targets.to(self.device), images)[0]
