"""``DeeplabV3PlusTrainer`` -- registered as ``trainer_deeplabv3plus`` like the reference's
(core/trainer/segmentation_trainer.py:21-159).  ``train_loop`` keeps the reference's step semantics (zero_grad -> forward ->
criterion -> backward -> Adam under AMP, :114-131) and runs it as the engine's fused step (``SegTrainStep``: engine forward,
``cvx_seg_criterion_loss``, engine backward, fused Adam with GradScaler's skip-on-overflow); with ``torch.distributed`` initialised the step
also sums the gradients over the ranks (RCCL).  ``evaluate_loop`` reports the reference's numbers (loss, Overall / Mean / FreqW
accuracy, Mean IoU, :133-159) from a confusion matrix accumulated on the device.  The VOC / Cityscapes / SBD readers are outside
the hot path: a dataloader is injected, or seeded synthetic batches stand in.  The input side is the device
pipeline: ``dataloader=`` / ``val_dataloader=`` take a ``DeviceSegLoader`` (computervision.pytorch_amd/seg_pipeline.py, the reference's
segmentation transforms as one launch per batch).  With ``val_dataloader=`` given, ``evaluate_loop`` is the fused pass: engine forward to
the low-resolution logits rows, then ``cvx_seg_criterion_eval`` (upsampling + arg max + confusion matrix + criterion in one launch, no
full-resolution logits, no gradient), one host synchronisation after the last batch; without it the unfused loop runs on the training
loader as before.
"""
import ctypes
from typing import Dict, List

import torch

from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd.deeplab import SegTrainStep
from configs import DeeplabV3PlusConfig
from core.algorithms.segmentation_2d import DeeplabV3PlusA
from core.trainer.engine_trainer import EngineTrainer
from registry import trainer_registry


class SyntheticSegmentationLoader:
    """Seeded stand-in for get_voc_dataloader (core/data/segmentation_dataset.py): yields ``(images (B,3,H,W) in [0,1),
    targets (B,H,W) int64 in [0, num_classes) with blocky regions and a few ignored pixels)``."""

    def __init__(self, batch_size, hw, num_classes, length=32, seed=1, ignore_index=-100):
        self.b, self.hw, self.nc, self.length, self.seed, self.ignore = batch_size, hw, num_classes, length, seed, ignore_index

    def __len__(self):
        return self.length

    def __iter__(self):
        g = torch.Generator().manual_seed(self.seed)
        h, w = self.hw
        for _ in range(self.length):
            images = torch.rand(self.b, 3, h, w, generator=g)
            coarse = torch.randint(0, self.nc, (self.b, 1, (h + 31) // 32, (w + 31) // 32), generator=g).float()
            targets = torch.nn.functional.interpolate(coarse, size=(h, w), mode="nearest")[:, 0].long()
            targets[torch.rand(self.b, h, w, generator=g) < 0.02] = self.ignore
            yield images, targets


class SegmentationMetrics:
    """core/metrics/seg_metrics.py:4-44 with the confusion matrix kept on the device: ``add_batch`` takes predictions (one bincount per
    batch, into the float64 ``confusion_matrix``), ``add_rows`` the engine's low-resolution logits rows (``cvx_seg_criterion_eval``: one launch, into
    the exact int64 ``counts``).  ``fold()`` adds ``counts`` into ``confusion_matrix`` and clears them; ``get_results`` folds first."""

    def __init__(self, num_classes, device="cpu"):
        self.num_classes = num_classes
        self.confusion_matrix = torch.zeros(num_classes, num_classes, dtype=torch.float64, device=device)
        self.counts = None                  # (nc, nc) int64 on the rows' device, created by the first add_rows

    def reset(self):
        self.confusion_matrix.zero_()
        if self.counts is not None:
            self.counts.zero_()

    def fold(self):
        """``confusion_matrix`` += what ``add_rows`` has counted since the last fold (float64 is exact below 2^53); returns the matrix."""
        if self.counts is not None:
            self.confusion_matrix += self.counts.to(self.confusion_matrix.device).double()
            self.counts.zero_()
        return self.confusion_matrix

    def add_labels_counts(self, device):
        """The exact int64 ``counts`` on ``device``, created on first use (and again when the device changes): what a kernel that counts
        labels itself -- ``cvx_seg_stitch`` behind ``DeeplabV3PlusA.segment_tiled`` -- adds to."""
        device = torch.device(device)
        if self.counts is None or self.counts.device != device:
            self.counts = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=device)
        return self.counts

    def add_rows(self, rows, targets, hw, criterion, loss_slot):
        """One validation batch from the logits rows ``(B, lh*lw, ld)`` fp32 of ``model.forward_rows`` and the targets ``(B, H, W)`` int64:
        ``confusion[target][argmax of the upsampled logits] += 1`` and ``criterion``'s (a ``SegLoss``) value of the batch into
        ``loss_slot``, a one-element float32 view on the rows' device, in one ``cvx_seg_criterion_eval`` call.  A criterion with options
        (class weights, label smoothing) gives the weighted, smoothed value over all valid pixels and the same matrix; its OHEM setting
        is not applied in evaluation.  With a region term (``SegLoss(region=)`` or ``SegLoss(lovasz=)``) the value-only chain of that term follows (no gradient plane,
        no adjoint), so that the slot holds ``base_weight * base + weight * region`` of the batch; the matrix is the
        eval launch's.  Asynchronous: nothing is read back."""
        if not (torch.is_tensor(rows) and rows.is_cuda):
            raise L.CvxError("SegmentationMetrics.add_rows runs on an MI355X only (there is no CPU path); add_batch takes host predictions")
        lib = L.load()
        dev = rows.device
        B, A, ld = rows.shape
        lh, lw = int(hw[0]), int(hw[1])
        if targets.dim() != 3 or targets.shape[0] != B or A != lh * lw or rows.dtype != torch.float32 or not rows.is_contiguous():
            raise ValueError("rows must be contiguous fp32 (B, lh*lw, ld) and targets (B, H, W)")
        if loss_slot.dtype != torch.float32 or loss_slot.numel() != 1 or loss_slot.device != dev:
            raise ValueError("loss_slot: one float32 element on the rows' device")
        targets = targets.to(device=dev, dtype=torch.long).contiguous()
        if self.counts is None or self.counts.device != dev:
            self.counts = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=dev)
        dims = L.SegDims(ld, B, self.num_classes, lh, lw, int(targets.shape[1]), int(targets.shape[2]))
        crit = criterion._criterion_struct(dev, self.num_classes, B)
        ws = criterion._ensure_buffers(lib, dev, dims, crit, for_eval=True)
        with torch.cuda.device(dev):
            L.check(lib.cvx_seg_criterion_eval(L.ptr(rows), ctypes.byref(dims), L.ptr(targets), ctypes.byref(crit), L.ptr(self.counts),
                                               L.ptr(loss_slot), L.ptr(criterion.region_stats), L.ptr(ws), L.stream_ptr(dev)),
                    "cvx_seg_criterion_eval")

    def add_batch(self, predictions, gts):
        predictions, gts = torch.as_tensor(predictions).reshape(-1), torch.as_tensor(gts).reshape(-1)
        mask = (gts >= 0) & (gts < self.num_classes)
        idx = (self.num_classes * gts[mask].long() + predictions[mask].long()).to(self.confusion_matrix.device)
        self.confusion_matrix += torch.bincount(idx, minlength=self.num_classes ** 2).reshape(self.num_classes, self.num_classes).double()

    def get_results(self):
        hist = self.fold().cpu()
        diag = torch.diag(hist)
        acc = float(diag.sum() / hist.sum())
        acc_cls = diag / hist.sum(1)
        iu = diag / (hist.sum(1) + hist.sum(0) - diag)
        freq = hist.sum(1) / hist.sum()
        return {"Overall Acc": acc, "Mean Acc": float(torch.nanmean(acc_cls)), "FreqW Acc": float((freq[freq > 0] * iu[freq > 0]).sum()),
                "Mean IoU": float(torch.nanmean(iu)), "Class IoU": dict(zip(range(self.num_classes), iu.tolist()))}


@trainer_registry("deeplabv3plus")
class DeeplabV3PlusTrainer(EngineTrainer):
    algorithm_cls, step_cls = DeeplabV3PlusA, SegTrainStep
    use_iter_milestones = False

    def __init__(self, cfg: DeeplabV3PlusConfig, device, dataloader=None, val_dataloader=None):
        if val_dataloader is not None:
            # the trainer's device, and the device the loader declares if it declares one (DeviceSegLoader does); a loader without a
            # ``device`` attribute is taken at its word, and host batches it yields are moved by evaluate_loop
            on = [torch.device(device)] + ([torch.device(val_dataloader.device)] if hasattr(val_dataloader, "device") else [])
            if any(d.type != "cuda" for d in on):
                raise L.CvxError("val_dataloader= selects the fused evaluation (cvx_seg_criterion_eval), which runs on an MI355X only: the trainer's "
                                 f"device and the loader's (here {', '.join(str(d) for d in on)}) must be GPUs, "
                                 "e.g. DeviceSegLoader(..., device='cuda')")
        super().__init__(cfg, device, dataloader, val_dataloader)
        self.metrics = SegmentationMetrics(num_classes=cfg.dataset.num_classes, device=device)

    def synthetic_loader(self):
        return SyntheticSegmentationLoader(self.batch_size, self.cfg.arch.crop_size, self.cfg.dataset.num_classes)

    def set_criterion(self):
        # dropout masks (aspp.project.3, deeplabv3plus.py:67) are a counter-based hash of (seed, training pass, op, element) on the engine:
        # derive the seed from torch's global seed, the rank (the reference's ranks draw independent masks) and the iteration a resumed run
        # starts at (a resumed job must not replay the mask sequence from pass 0)
        import torch.distributed as dist
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.model.seed = (int(torch.initial_seed()) * 0x9E3779B97F4A7C15 + rank * 0xBF58476D1CE4E5B9 + int(self.last_iter) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        super().set_criterion()

    def train_loop(self, batch_data, scaler) -> List:
        images = batch_data[0].to(self.device, non_blocking=True)
        targets = batch_data[1].to(self.device, non_blocking=True)
        return [self._step(images, targets)]

    def evaluate_loop(self) -> Dict:
        if self._injected_val_loader is not None:
            return fused_evaluation(self.eval_model, self.criterion, self.metrics, self.val_dataloader, self.device)
        model = self.eval_model                        # the weight average when cfg.train.ema is on
        model.eval()
        self.metrics.reset()
        total, n = 0.0, 0
        with torch.no_grad():
            for images, targets in self.val_dataloader:
                images, targets = images.to(self.device), targets.to(self.device)
                preds = model(images)
                total += float(self.criterion(preds, targets))
                self.metrics.add_batch(torch.argmax(preds, dim=1), targets)
                n += 1
        r = self.metrics.get_results()
        return {"Loss": total / max(n, 1), "Overall Acc": r["Overall Acc"], "Mean Acc": r["Mean Acc"], "FreqW Acc": r["FreqW Acc"],
                "Mean IoU": r["Mean IoU"]}


def fused_evaluation(model, criterion, metrics: SegmentationMetrics, dataloader, device) -> Dict:
    """The reference's validation pass (:133-159) without the full-resolution logits: per batch ``model.forward_rows`` and
    ``metrics.add_rows`` into a per-batch loss buffer; the host synchronises ONCE, when the buffer and the matrix are read after the
    last batch.  Returns the reference's five numbers."""
    model.eval()
    metrics.reset()
    losses = torch.zeros(max(len(dataloader), 1), dtype=torch.float32, device=device)
    n = 0
    with torch.no_grad():
        for images, targets in dataloader:
            if n >= losses.numel():              # a loader that yields more batches than its len()
                losses = torch.cat([losses, torch.zeros_like(losses)])
            rows = model.forward_rows(images.to(device, non_blocking=True))
            metrics.add_rows(rows, targets, model._last_engine.graph.level_hw[0], criterion, losses[n:n + 1])
            n += 1
    total = float(losses[:n].double().sum()) if n else 0.0
    r = metrics.get_results()
    return {"Loss": total / max(n, 1), "Overall Acc": r["Overall Acc"], "Mean Acc": r["Mean Acc"], "FreqW Acc": r["FreqW Acc"],
            "Mean IoU": r["Mean IoU"]}


def _tta_pass(model, metrics: SegmentationMetrics, dataloader, device, tta, boundary=None) -> Dict:
    """The loop of ``fused_evaluation_tta``; with ``boundary`` (a ``seg_boundary.BoundaryMetrics``) the fusion also writes its label maps and
    one ``cvx_seg_boundary`` call per batch counts them against the targets."""
    model.eval()
    metrics.reset()
    counts = metrics.add_labels_counts(device)
    with torch.no_grad():
        for images, targets in dataloader:
            images = images.to(device, non_blocking=True)
            views = tta.run(model, images)
            labels = tta.fuse(views, metrics.num_classes, model.layout.nc_pad, images.shape[2:], targets=targets, counts=counts,
                              labels=boundary is not None)
            if boundary is not None:
                boundary.add_labels(labels, targets.to(device, non_blocking=True))
    r = metrics.get_results()
    return {"Overall Acc": r["Overall Acc"], "Mean Acc": r["Mean Acc"], "FreqW Acc": r["FreqW Acc"], "Mean IoU": r["Mean IoU"]}


def fused_evaluation_tta(model, metrics: SegmentationMetrics, dataloader, device, tta) -> Dict:
    """The validation pass under multi-scale / flip test-time augmentation (``tta``: a ``computervision.pytorch_amd.seg_tta.SegTTA``, DESIGN.md
    section 7n): per batch ``tta.run`` (one input launch and one ``forward_rows`` per scale) and one ``cvx_seg_fuse`` launch that counts
    into ``metrics.add_labels_counts(device)``; the host synchronises ONCE, when the matrix is read after the last batch.  Returns the
    four accuracies; the criterion's value is not defined on this path, so there is no "Loss"."""
    return _tta_pass(model, metrics, dataloader, device, tta)


def fused_evaluation_boundary(model, metrics: SegmentationMetrics, dataloader, device, tta, boundary) -> Dict:
    """``fused_evaluation_tta`` with the boundary metrics: ``boundary`` is a ``seg_boundary.BoundaryMetrics`` (reset
    here); every batch's fused label maps go through one ``cvx_seg_boundary`` call against the targets (values outside ``[0,
    num_classes)`` are void).  Nothing waits on the host inside the loop; the confusion matrix and the boundary tables are read after the
    last batch.  Returns the four accuracies and the dicts of ``boundary.get_results()``."""
    boundary.reset()
    r = _tta_pass(model, metrics, dataloader, device, tta, boundary)
    r.update(boundary.get_results())
    return r
