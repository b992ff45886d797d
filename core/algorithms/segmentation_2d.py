"""DeepLabv3+ algorithm wrapper -- the duck-typed interface of the reference's ``DeeplabV3PlusA``
(core/algorithms/segmentation_2d.py:43-201): ``__init__(cfg, device)``, ``build_model() -> (nn.Module, name)``,
``build_loss()`` (FocalLoss / CrossEntropyLoss, :59-64, as the engine's fused ``SegLoss``), ``postprocess_seg2d`` (argmax ->
colour map), ``predict``, ``evaluate_on_voc`` (:115-166, the fused validation pass over an injected device loader).  The network runs
on the MI355X engine (``computervision.pytorch_amd.deeplab``).
"""
import os
import time

import numpy as np
import torch

from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd.deeplab import DeepLabV3PlusR101, SegLoss
from configs import DeeplabV3PlusConfig
from core.algorithms.base import FramePredictor
from registry import model_registry


def voc_colormap(n: int = 21):
    """The PASCAL VOC palette (core/data/segmentation_dataset.py:14-36 lists its first 21 entries): class index bits spread over
    the high bits of R, G, B, three bits per round."""
    cmap = []
    for i in range(n):
        r = g = b = 0
        c = i
        for j in range(8):
            r |= ((c >> 0) & 1) << (7 - j)
            g |= ((c >> 1) & 1) << (7 - j)
            b |= ((c >> 2) & 1) << (7 - j)
            c >>= 3
        cmap.append((r, g, b))
    return cmap


def postprocess_seg2d(dataset_type, pred, device):
    """(B, C, H, W) logits -> (B, H, W, 3) colours (reference :20-30)."""
    if dataset_type.lower() not in ("voc", "sbd"):
        raise NotImplementedError(f"不支持{dataset_type}数据集")
    colormap = torch.tensor(voc_colormap(), device=device)
    return colormap[torch.argmax(pred, dim=1).long(), :]


@model_registry("deeplabv3plus")
class DeeplabV3PlusA(FramePredictor):
    def __init__(self, cfg: DeeplabV3PlusConfig, device) -> None:
        self.cfg, self.device = cfg, device
        self.loss_type = cfg.loss.loss_type
        self.num_classes = cfg.dataset.num_classes
        self.input_image_size = cfg.arch.input_size
        self.batch_size = cfg.train.batch_size
        self.dataset_name = cfg.dataset.dataset_name

    def build_model(self):
        if self.cfg.arch.output_stride != 16 or self.cfg.arch.backbone_name != "resnet101":
            raise L.CvxError("the MI355X engine builds DeepLabv3+ with a ResNet-101 backbone at output stride 16 (the reference's configuration)")
        if self.cfg.arch.backbone_pretrained:
            raise L.CvxError("backbone_pretrained needs a torchvision download; load a checkpoint with load_state_dict instead")
        return DeepLabV3PlusR101(self.num_classes), "deeplabv3plus"

    def build_loss(self):
        """Reference :59-64: "ce" -> nn.CrossEntropyLoss(reduction="mean"), "focal" -> FocalLoss() (alpha 0.25, gamma 2,
        ignore_index -100, mean over all pixels; core/loss/focal_loss.py:6-22).  Beyond the reference, ``cfg.loss.class_weights``,
        ``cfg.loss.label_smoothing`` and ``cfg.loss.ohem`` (absent by default: the config file stays the reference's) select the
        options of the fused cross-entropy, and ``cfg.loss.region = dict(kind="dice" | "tversky", ...)`` adds a region loss to either
        loss type and ``cfg.loss.lovasz = dict(...)`` the Lovasz-Softmax loss, see ``SegLoss``."""
        if self.loss_type not in ("ce", "focal"):
            raise L.CvxError(f"loss_type {self.loss_type!r}: the reference knows 'ce' and 'focal'")
        loss_cfg = self.cfg.loss
        return SegLoss(self.loss_type, class_weights=getattr(loss_cfg, "class_weights", None),
                       label_smoothing=getattr(loss_cfg, "label_smoothing", 0.0), ohem=getattr(loss_cfg, "ohem", None),
                       region=getattr(loss_cfg, "region", None), lovasz=getattr(loss_cfg, "lovasz", None))

    def predict_tensor(self, model, images: torch.Tensor, scales=None, flip=False, fuse="prob"):
        """(B,3,H,W) normalised images on the device -> (B,H,W,3) class colours (the tensor part of ``predict``).  ``scales`` / ``flip``
        select test-time augmentation (``predict_labels``): the colours of the fused labels."""
        if scales is None and not flip:
            model.eval()
            with torch.no_grad():
                return postprocess_seg2d(self.dataset_name, model(images), images.device)
        if self.dataset_name.lower() not in ("voc", "sbd"):
            raise NotImplementedError(f"不支持{self.dataset_name}数据集")
        labels = self.predict_labels(model, images, scales=(1.0,) if scales is None else scales, flip=flip, fuse=fuse)
        return torch.tensor(voc_colormap(), device=labels.device)[labels.long(), :]

    def predict_labels(self, model, images: torch.Tensor, scales=(1.0,), flip=False, fuse="prob", probs=False):
        """Multi-scale and flip test-time augmentation: the network runs on ``images`` ((B,3,H,W) on the device) at
        every zoom of ``scales`` (``seg_tta.view_size``) and, with ``flip``, on their mirror image; one ``cvx_seg_fuse`` launch brings the
        logits of all views to (H, W), fuses them (``fuse``: ``"prob"``, the mean of the views' softmax, or ``"logits"``, the sum of their
        logits) and takes the arg max.  Returns the (B, H, W) uint8 labels on the device and, with ``probs`` (``"prob"`` only), the
        (B, num_classes, H, W) mean probabilities as well.  Nothing waits on the host."""
        from computervision.pytorch_amd.seg_tta import SegTTA
        tta = SegTTA(scales, flip, fuse)
        self._need_gpu("predict_labels")
        model.eval()
        views = tta.run(model, images)
        return tta.fuse(views, self.num_classes, model.layout.nc_pad, images.shape[2:], probs=probs)

    def predict(self, model, image_path, print_on, save_result):
        """Reference :80-113: read, resize to the network size (no letterbox), forward, colour, resize back, blend 50 % with the
        original image, RGB -> BGR.  Image I/O needs OpenCV, imported lazily as in the other algorithm classes."""
        import cv2
        original = cv2.cvtColor(cv2.imread(image_path), cv2.COLOR_BGR2RGB)
        h, w = original.shape[:2]
        size = self.cfg.arch.input_size[1:]
        img = cv2.resize(original, (size[1], size[0])).astype(np.float32) / 255.0
        x = torch.from_numpy(img).permute(2, 0, 1).unsqueeze(0).to(self.device)
        colours = self.predict_tensor(model, x)[0].to(torch.uint8).cpu().numpy()
        colours = cv2.resize(colours, (w, h), interpolation=cv2.INTER_NEAREST)
        result = cv2.addWeighted(original, 0.5, colours, 0.5, 0.0)[..., ::-1]
        if save_result:
            os.makedirs(self.cfg.decode.test_results, exist_ok=True)
            cv2.imwrite(os.path.join(self.cfg.decode.test_results, os.path.basename(image_path).split(".")[0] + "@cvx.jpg"), result)
            return None
        return result

    def predict_batch(self, model, frames, draw=True, sync=False, bgr=False):
        """``predict`` for a batch, on the device: ``frames`` is a list of uint8 HWC RGB device tensors of any sizes.  One launch stretches
        them to ``cfg.arch.input_size`` (``cvx_aug_images_plain`` jobs: bicubic, / 255, no mean / std -- what ``predict`` feeds; it resizes
        with OpenCV's default bilinear filter), one ``forward_rows``, and with ``draw`` one ``cvx_seg_overlay``
        launch colours, resizes (nearest) and blends 50/50 into the frames, in place (``bgr``: written as B, G, R, the channel order
        ``predict`` returns).  Returns the logits rows (B, h * w, nc_pad) on the device; nothing waits on the host unless ``sync``."""
        from computervision.pytorch_amd import render
        self._need_gpu("predict_batch")
        frames = list(frames)
        net_hw = tuple(int(v) for v in self.cfg.arch.input_size[1:])
        batch = render.FrameBatch(frames, net_hw, letterbox=False)
        model.eval()
        with torch.no_grad():
            rows = model.forward_rows(batch.network_input())
        if draw:
            render.seg_overlay(frames, rows, self.num_classes, model._last_engine.graph.level_hw[0], net_hw, bgr=bgr, batch=batch)
        if sync:
            torch.cuda.synchronize(rows.device)
        return rows

    def segment_tiled(self, model, frames, overlap=0.2, weight="linear", batch_size=16, draw=True, bgr=False, targets=None, metrics=None,
                      sync=False, boundary=None):
        """Sliding-window segmentation for frames much larger than the network input, where ``predict_batch``'s stretch loses the thin
        structures and the aspect ratio: every frame is cut into tiles of ``cfg.arch.input_size`` that overlap by
        ``overlap`` (``render.tile_grid``; zoom 1, no whole-picture slot), one ``cvx_tiles_u8_to_nchw`` launch builds all slots (/ 255, no
        mean / std: ``predict_batch``'s feed), ``forward_rows`` runs them in chunks of at most ``batch_size`` (``render.slot_chunks``: equal chunks, so the
        engine keeps one plan) into one (slots, h * w, nc_pad) block on the device, and one ``cvx_seg_stitch`` launch blends the up-sampled logits of the tiles that cover each pixel (``weight``:
        ``"linear"``, the distance to the tile's borders, or ``"mean"``), takes the arg max and, with ``draw``, blends the class colours
        50/50 into the frames in place (``bgr`` as in ``predict_batch``).  ``targets`` (one (h, w) uint8 device map per frame; values
        >= num_classes are ignored) with ``metrics`` (a ``SegmentationMetrics``) adds the exact confusion counts to ``metrics.counts``;
        ``fold()`` / ``get_results()`` then work as after ``add_rows``.  ``boundary`` (a ``seg_boundary.BoundaryMetrics``, DESIGN.md section
        7z) needs ``targets`` too -- ``metrics`` may then be None -- and adds, after the stitch, the boundary counts of the returned label
        maps against ``targets`` to its tables (one ``cvx_seg_boundary`` call).  Returns the list of (h, w) uint8 label maps on the device;
        nothing waits on the host unless ``sync``."""
        from computervision.pytorch_amd import render
        self._need_gpu("segment_tiled")
        if int(batch_size) <= 0:
            raise ValueError("batch_size is positive")
        if boundary is None:
            if (targets is None) != (metrics is None):
                raise ValueError("targets and metrics come together")
        else:
            from computervision.pytorch_amd.seg_boundary import BoundaryMetrics
            if not isinstance(boundary, BoundaryMetrics):
                raise ValueError(f"boundary: a seg_boundary.BoundaryMetrics, got {type(boundary).__name__}")
            if targets is None:
                raise ValueError("boundary needs targets")
        frames = list(frames)
        net_hw = tuple(int(v) for v in self.cfg.arch.input_size[1:])
        batch = render.TileBatch(frames, net_hw, overlap, full_frame=False)
        x = batch.network_input()
        model.eval()
        block = None
        with torch.no_grad():
            for c0, c1 in render.slot_chunks(batch.slots, batch_size):
                chunk = x[c0:c1]
                if chunk.data_ptr() % 8:                          # the engine reads 8-byte aligned images: an odd slot size at an odd c0
                    chunk = chunk.clone()
                rows = model.forward_rows(chunk)
                if block is None:
                    block = torch.empty(batch.slots, rows.shape[1], rows.shape[2], dtype=torch.float32, device=rows.device)
                block[c0:c0 + rows.shape[0]].copy_(rows)
        counts = metrics.add_labels_counts(block.device) if metrics is not None else None
        labels = render.stitch_segmentation(frames, block, self.num_classes, model._last_engine.graph.level_hw[0], net_hw, batch, weight=weight,
                                            labels=True, draw=draw, bgr=bgr, targets=targets if metrics is not None else None,
                                            counts=counts)
        if boundary is not None:
            boundary.add_labels(labels, list(targets))
        if sync:
            torch.cuda.synchronize(block.device)
        return labels

    def predict_regions(self, model, frames, regions=None, conf=False, draw=False, tracker=None, sync=False, **tiled):
        """Things from the label maps: ``segment_tiled(model, frames, draw=draw, **tiled)`` -- frames of any size, a
        frame no larger than the network input is one tile -- and then ``seg_regions.label_regions`` on its label maps under ``regions``
        (a ``seg_regions.SegRegions``, default ``SegRegions()``): the connected regions of every class as rows ``[x1, y1, x2, y2, score,
        cls]`` with counts, the detectors' format.  With ``draw`` the boxes are painted over the class overlay (``cvx_draw_detections``);
        ``tracker``: a ``track.Tracker`` -- the frames are consecutive frames of its stream 0, the batch gains ``ids`` and ``draw`` paints
        them with ``cvx_draw_tracks``.  Returns the ``seg_regions.RegionBatch`` (with ``labels``, the label maps) on the device; ``sync``
        waits for the device, ``RegionBatch.read()`` is the one host read.  ``conf=True`` is refused: ``segment_tiled`` keeps no
        probabilities (every region scores 1); ``predict_labels(..., probs=True)`` has them, see ``seg_regions.label_regions``."""
        from computervision.pytorch_amd import render, seg_regions
        self._need_gpu("predict_regions")
        if conf:
            raise L.CvxError("predict_regions(conf=True): segment_tiled stitches labels and keeps no probabilities, so there is no confidence "
                             "to average; use predict_labels(..., probs=True) and pass conf= to seg_regions.label_regions")
        if tracker is not None:
            from computervision.pytorch_amd.track import Tracker
            if not isinstance(tracker, Tracker):
                raise ValueError(f"tracker: a track.Tracker, got {type(tracker).__name__}")
        frames = list(frames)
        labels = self.segment_tiled(model, frames, draw=draw, sync=False, **tiled)
        found = seg_regions.label_regions(labels, regions)
        found.labels = labels
        if tracker is not None:
            found.ids = tracker.update(found.rows, found.counts)
        if draw:
            if tracker is not None:
                render.draw_tracks(frames, found.rows, found.ids, found.counts)
            else:
                render.draw_detections(frames, found.rows, found.counts)
        if sync:
            torch.cuda.synchronize(found.rows.device)
        return found

    def segment_frames(self, model, frames, batch_size, regions=None, track=None, **tiled):
        """``detect_frames`` for ``segment_tiled``: a generator over any iterable of uint8 HWC RGB device frames that yields the list of
        drawn frames of each batch of ``batch_size`` (the last one may be short).  Each batch is one ``segment_tiled(..., draw=True,
        sync=False, **tiled)``, so nothing inside the loop waits on the host.  ``batch_size`` counts frames; the slots per forward stay at
        ``segment_tiled``'s default.  (``detect_frames(..., tiled=...)`` stays the detectors'.)
        ``regions``: a ``seg_regions.SegRegions`` -- each batch is then one ``predict_regions(..., regions=regions, draw=True)``: the boxes
        of the connected regions are painted over the overlay.  ``track``: a ``track.Tracker``, or a dict of its parameters from which one
        is created for the generator's lifetime -- the regions keep an identity from frame to frame and are painted with their track ids
        (``regions`` defaults to ``SegRegions()`` then).  With both None nothing changes."""
        self._need_gpu("segment_frames")
        if int(batch_size) <= 0:
            raise ValueError("batch_size is positive")
        if {"draw", "sync"} & set(tiled):
            raise ValueError("segment_frames draws and does not wait: it takes neither draw nor sync")
        if regions is None and track is None:
            def segment(batch):
                self.segment_tiled(model, batch, draw=True, sync=False, **tiled)
        else:
            tracker = None
            if track is not None:
                from computervision.pytorch_amd.track import Tracker
                tracker = track if isinstance(track, Tracker) else Tracker(self.device, **dict(track))

            def segment(batch):
                self.predict_regions(model, batch, regions=regions, draw=True, tracker=tracker, sync=False, **tiled)

        def batches():
            batch = []
            for frame in frames:
                batch.append(frame)
                if len(batch) == int(batch_size):
                    segment(batch)
                    yield batch
                    batch = []
            if batch:
                segment(batch)
                yield batch

        return batches()

    def evaluate_on_voc(self, model, results_out_root, subset="val", dataloader=None, scales=None, flip=False, fuse="prob", boundary=None):
        """Reference :115-166: the validation metrics of ``model`` over VOC-``subset``, printed and written to
        ``results_out_root/DeepLabV3Plus/DeepLabV3Plus_<dataset>_<time>.txt`` as four lines (Overall Acc, Mean Acc, FreqW Acc, Mean IoU).
        Reading VOC from disk is outside the hot path: ``dataloader`` is a ``DeviceSegLoader`` over the pictures with
        ``DeviceSegAugmenter(crop_hw=cfg.arch.crop_size, base_size=max(cfg.arch.input_size[1:]), colormap=voc_colormap(), train=False)``.
        Each batch is one engine forward and one ``cvx_seg_criterion_eval`` launch; the host waits once, at the end.  ``scales`` / ``flip`` /
        ``fuse`` select test-time augmentation (``predict_labels``): each batch is then one forward per scale and
        one ``cvx_seg_fuse`` launch, still with one host wait at the end.  ``boundary`` (a ``seg_boundary.SegBoundary``)
        adds the boundary metrics: after the four lines the report gains three per width, ``Trimap mIoU@d``, ``Boundary IoU@d`` and
        ``BF@d``.  They need label maps and the plain pass (``cvx_seg_criterion_eval``) writes none, so ``boundary=`` without ``scales`` /
        ``flip`` runs the label-writing path with one view, ``SegTTA((1.0,), False, fuse)``: its four accuracies are the fusion's, not the
        criterion's.  Each batch gains one ``cvx_seg_boundary`` call; the host still waits once, at the end.  Returns the path written."""
        from core.trainer.segmentation_trainer import SegmentationMetrics, fused_evaluation, fused_evaluation_boundary, fused_evaluation_tta
        if subset != "val":
            raise ValueError(f"不支持VOC-{subset}")
        if dataloader is None:
            raise L.CvxError("evaluate_on_voc reads no dataset from disk: pass dataloader=DeviceSegLoader(source, batch_size, "
                             "DeviceSegAugmenter(crop_hw, base_size, colormap=voc_colormap(), train=False)) over the VOC-val pictures")
        tta = None
        if boundary is not None:
            from computervision.pytorch_amd.seg_boundary import BoundaryMetrics, SegBoundary, report_lines
            if not isinstance(boundary, SegBoundary):
                raise ValueError(f"boundary: a seg_boundary.SegBoundary, got {type(boundary).__name__}")
        if scales is not None or flip or boundary is not None:
            from computervision.pytorch_amd.seg_tta import SegTTA
            tta = SegTTA((1.0,) if scales is None else scales, flip, fuse)
            self._need_gpu("evaluate_on_voc with boundary metrics" if scales is None and not flip else "evaluate_on_voc with test-time augmentation")
        model_name = "DeepLabV3Plus"
        results_out_root = os.path.join(results_out_root, model_name)
        os.makedirs(results_out_root, exist_ok=True)
        results_filepath = os.path.join(results_out_root, f"{model_name}_{self.dataset_name}_{time.strftime('%Y-%m-%d-%H-%M-%S')}.txt")
        metrics = SegmentationMetrics(num_classes=self.num_classes, device=self.device)
        if tta is None:
            r = fused_evaluation(model, self.build_loss(), metrics, dataloader, self.device)
        elif boundary is None:
            r = fused_evaluation_tta(model, metrics, dataloader, self.device, tta)
        else:
            r = fused_evaluation_boundary(model, metrics, dataloader, self.device, tta, BoundaryMetrics(self.num_classes, boundary, self.device))
        formatted = (f"Overall Acc: {r['Overall Acc']}\n"
                     f"Mean Acc: {r['Mean Acc']}\n"
                     f"FreqW Acc: {r['FreqW Acc']}\n"
                     f"Mean IoU: {r['Mean IoU']}")
        if boundary is not None:
            formatted = "\n".join([formatted] + report_lines(r, boundary.keys))
        print(f"结果：\n{formatted}")
        with open(results_filepath, mode="w", encoding="utf-8") as f:
            f.write(formatted)
        return results_filepath
