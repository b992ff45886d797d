"""``SsdTrainer`` -- registered as ``trainer_ssd`` like the reference's (core/trainer/ssd_train.py).  ``train_loop`` keeps the reference's
step semantics (zero_grad -> forward -> MultiBoxLossV2 -> backward -> Adam under AMP, :96-115) and runs it as the engine's fused step
(``SsdTrainStep``: engine forward, ``cvx_multibox_loss``, engine backward, fused Adam with GradScaler's skip-on-overflow); with
``torch.distributed`` initialised the step also sums the gradients over the ranks (RCCL).  The input side is the device pipeline: ``dataloader=`` / ``val_dataloader=`` take a ``DeviceAugLoader(fmt="ssd")`` over
``DeviceAugmenter(target=Ssd(cfg, device))`` -- ``DetectionDataset`` + ``ssd_collate`` of the reference (core/data/collate.py:32-49,
core/algorithms/ssd.py:327-480) as the augmentation launches followed by ``cvx_ssd_encode_targets``, without a host synchronisation -- or
any iterable yielding ``(images, y_true (B, 8732, 4 + (nc + 1) + 1))``; without one, seeded synthetic batches of that format stand in.
``evaluate_loop`` runs on ``val_dataloader`` when one is given (``DeviceAugmenter(train=False)``), else on the training loader."""
from typing import List

import torch

from computervision.pytorch_amd.ssd import SsdTrainStep
from core.algorithms.ssd import Ssd
from core.trainer.engine_trainer import EngineTrainer
from registry import trainer_registry


class SyntheticSsdLoader:
    """Seeded stand-in for DetectionDataset + ssd_collate: images (B,3,300,300) in [0,1) and encoded targets (B, 8732, 4 + (nc+1) + 1):
    a few positive priors per image with box regression targets and a one-hot class, background one-hot elsewhere."""

    def __init__(self, batch_size, hw, num_classes, anchors=8732, n_pos=24, length=16, seed=1):
        self.b, self.hw, self.nc, self.a, self.n_pos, self.length, self.seed = batch_size, hw, num_classes, anchors, n_pos, length, seed

    def __len__(self):
        return self.length

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        for _ in range(self.length):
            images = torch.rand(self.b, 3, *self.hw, generator=g)
            y = torch.zeros(self.b, self.a, 4 + self.nc + 1 + 1)
            y[:, :, 4] = 1.0
            for b in range(self.b):
                idx = torch.randperm(self.a, generator=g)[:self.n_pos]
                y[b, idx, :4] = torch.randn(self.n_pos, 4, generator=g)
                y[b, idx, 4] = 0.0
                y[b, idx, 5 + torch.randint(0, self.nc, (self.n_pos,), generator=g)] = 1.0
                y[b, idx, -1] = 1.0
            yield images, y


@trainer_registry("ssd")
class SsdTrainer(EngineTrainer):
    algorithm_cls, step_cls = Ssd, SsdTrainStep
    metric_names, show_option = ["loss", "loc_loss", "conf_loss"], [True, True, True]

    def synthetic_loader(self):
        return SyntheticSsdLoader(self.batch_size, self.input_image_size[1:], self.cfg.dataset.num_classes)

    def train_loop(self, batch_data, scaler) -> List:
        images = batch_data[0].to(self.device, non_blocking=True)
        targets = batch_data[1].to(self.device, non_blocking=True)
        items = self._step(images, targets)
        return [items[0], items[1], items[2]]

    def validation_loss(self, model, images, targets):
        return self.criterion(y_pred=model(images.to(self.device)), y_true=targets.to(self.device))[0]
