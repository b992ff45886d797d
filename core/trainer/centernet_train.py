"""``CenterNetTrainer`` -- registered as ``trainer_centernet`` like the reference's (core/trainer/centernet_train.py:21-135).
``train_loop`` keeps the reference's step semantics (zero_grad -> forward -> CombinedLoss -> backward -> Adam under AMP, :104-121) and
runs it as the engine's fused step (``CenterNetTrainStep``: engine forward, ``cvx_centernet_loss``, engine backward, fused Adam with
GradScaler's skip-on-overflow); with ``torch.distributed`` initialised the step also sums the gradients over the ranks (RCCL).
The input side is the device pipeline: ``dataloader=`` / ``val_dataloader=`` take a ``DeviceAugLoader(fmt="centernet")`` over
``DeviceAugmenter(target=CenterNetA(cfg, device))`` -- ``DetectionDataset`` + ``centernet_collate`` of the reference
(core/data/collate.py:52-68, core/algorithms/centernet.py:66-120) as the augmentation launches followed by ``cvx_centernet_draw_targets``,
without a host synchronisation -- or any iterable yielding ``(images, [heatmap, reg, wh, reg_mask, indices])``; without one, seeded
synthetic batches of that format stand in.  ``evaluate_loop`` runs on ``val_dataloader`` when one is given
(``DeviceAugmenter(train=False)``), else on the training loader."""
from typing import List

import torch

from computervision.pytorch_amd.dla import CenterNetTrainStep
from core.algorithms.centernet import CenterNetA
from core.trainer.engine_trainer import EngineTrainer
from registry import trainer_registry


class SyntheticCenterNetLoader:
    """Seeded stand-in for DetectionDataset + centernet_collate: images (B,3,H,W) in [0,1) and the five target tensors in the format of
    CenterNet.generate_targets -- Gaussian bumps with an exact 1 at each centre, sub-pixel offsets, sizes, mask, flat indices."""

    def __init__(self, batch_size, hw, num_classes, max_boxes=30, ratio=4, length=16, seed=1):
        self.b, self.hw, self.nc, self.k, self.ratio, self.length, self.seed = batch_size, hw, num_classes, max_boxes, ratio, length, seed

    def __len__(self):
        return self.length

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        H, W = self.hw
        h, w = H // self.ratio, W // self.ratio
        ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
        for _ in range(self.length):
            images = torch.rand(self.b, 3, H, W, generator=g)
            heat = torch.zeros(self.b, h, w, self.nc)
            reg, wh = torch.zeros(self.b, self.k, 2), torch.zeros(self.b, self.k, 2)
            mask, idx = torch.zeros(self.b, self.k), torch.zeros(self.b, self.k, dtype=torch.long)
            for b in range(self.b):
                for k in range(3):
                    cx, cy = float(torch.rand(1, generator=g)) * (w - 1), float(torch.rand(1, generator=g)) * (h - 1)
                    bw, bh = 2 + float(torch.rand(1, generator=g)) * w / 3, 2 + float(torch.rand(1, generator=g)) * h / 3
                    c, ix, iy = int(torch.randint(0, self.nc, (1,), generator=g)), int(cx), int(cy)
                    sigma = max(1.0, min(bw, bh) / 6)
                    heat[b, :, :, c] = torch.maximum(heat[b, :, :, c], torch.exp(-((xs - ix) ** 2 + (ys - iy) ** 2) / (2 * sigma * sigma)))
                    reg[b, k], wh[b, k] = torch.tensor([cx - ix, cy - iy]), torch.tensor([bw, bh])
                    mask[b, k], idx[b, k] = 1.0, iy * w + ix
            yield images, [heat, reg, wh, mask, idx]


@trainer_registry("centernet")
class CenterNetTrainer(EngineTrainer):
    algorithm_cls, step_cls = CenterNetA, CenterNetTrainStep

    def synthetic_loader(self):
        return SyntheticCenterNetLoader(self.batch_size, self.input_image_size[1:], self.cfg.dataset.num_classes,
                                        getattr(self.cfg.train, "max_num_boxes", 30), self.cfg.arch.downsampling_ratio)

    def train_loop(self, batch_data, scaler) -> List:
        images = batch_data[0].to(self.device, non_blocking=True)
        targets = [t.to(self.device, non_blocking=True) for t in batch_data[1]]
        return [self._step(images, targets)[0]]

    def validation_loss(self, model, images, targets):
        return self.criterion(model(images.to(self.device)), [t.to(self.device) for t in targets])
