"""Weighted Boxes Fusion and detector ensembles on the device (``csrc/box_fusion.hip``).

Weighted Boxes Fusion (Solovyev et al., 2021) combines what several sources report for a frame without discarding any of it: every box
joins the cluster whose *current fused box* it overlaps best, the fused box is the score-weighted mean of the cluster's members, and the
cluster's confidence falls when only a few of the sources agree.  The sources are the views of a test-time augmentation
(``DetTTA(fusion=WBF())``) or the members of a ``DetEnsemble``: any of the four detector families, several sets of weights per
architecture, each with its own input size in ``predict_batch``.  One ``cvx_det_fuse_wbf`` launch fuses every frame of the batch; nothing
waits on the host.  The reference has no counterpart; ``tests/box_fusion_restatement.py`` is the specification.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .det_tta import FUSE_CAP, pad_blocks

MAX_SOURCES = 32                                # cvx_det_fuse_wbf's frame-local ids come from a table of 32 counts
CONF_MODES = {"avg": 0, "max": 1}


def _checked_weights(weights, n: Optional[int] = None):
    """None, or the weights as a tuple of positive finite floats (``n`` of them when given)"""
    if weights is None:
        return None
    if torch.is_tensor(weights):
        if weights.is_cuda:
            raise ValueError("weights: host values (a sequence, an array or a CPU tensor) -- checking device values would read them back")
        weights = weights.tolist()
    weights = tuple(float(w) for w in np.asarray(weights, np.float64).reshape(-1))
    if not 1 <= len(weights) <= MAX_SOURCES or (n is not None and len(weights) != n):
        raise ValueError(f"weights: one per source, {'1 to ' + str(MAX_SOURCES) if n is None else n}, got {len(weights)}")
    if any(not math.isfinite(w) or w <= 0.0 or np.float32(w) <= 0 or not np.isfinite(np.float32(w)) for w in weights):
        raise ValueError(f"weights: positive and finite (in fp32), got {weights}")
    return weights


class WBF:
    """The parameters of one Weighted Boxes Fusion.  ``iou``: a box joins the cluster whose fused box it overlaps by more than this;
    ``skip_score``: rows below it are left out; ``conf``: a cluster's confidence is the mean (``"avg"``) or the largest (``"max"``) weighted
    score of its members, and with ``rescale`` it is scaled by ``min(members, sum of weights) / sum of weights``; ``weights``: one per
    source, None for ones; ``max_det``: rows per frame after the fusion.  ``class_agnostic``: boxes of different classes fuse, and a
    cluster has the class of its first (best) member -- then one wave of the kernel walks the whole frame, which at the capacity of 8192
    candidates takes tens of milliseconds (DESIGN.md section 7v has the timings); per class the 16 waves share the classes."""

    def __init__(self, iou: float = 0.55, skip_score: float = 0.0, conf: str = "avg", rescale: bool = True, weights: Optional[Sequence[float]] = None,
                 class_agnostic: bool = False, max_det: int = 300):
        if not 0.0 <= float(iou) <= 1.0:
            raise ValueError("iou lies in [0, 1]")
        if not (math.isfinite(float(skip_score)) and float(skip_score) >= 0.0):
            raise ValueError("skip_score is finite and not negative")
        if conf not in CONF_MODES:
            raise ValueError(f"conf: one of {sorted(CONF_MODES)}, got {conf!r}")
        if not 1 <= int(max_det) <= FUSE_CAP:
            raise ValueError(f"max_det lies in [1, {FUSE_CAP}]")
        self.iou, self.skip_score, self.conf, self.rescale = float(iou), float(skip_score), conf, bool(rescale)
        self.weights, self.class_agnostic, self.max_det = _checked_weights(weights), bool(class_agnostic), int(max_det)

    def fuse(self, rows, counts, view_map, frame_hw, weights=None, max_det: Optional[int] = None, overflow=None):
        """``fuse_wbf`` with this object's parameters; ``weights`` stand in where the object has none"""
        return fuse_wbf(rows, counts, view_map, frame_hw, self.weights if self.weights is not None else weights, self.iou, self.skip_score, self.conf,
                        self.rescale, self.class_agnostic, self.max_det if max_det is None else max_det, overflow)


_weights_on = {}          # (device, weights) -> (the pinned host tensor the copy reads, the device tensor)


def _device_weights(weights, n, device):
    """(n) fp32 on ``device``, without a wait: ones are filled there, others come by an asynchronous copy from pinned memory, once"""
    key = (device, weights if weights is not None else n)
    hit = _weights_on.get(key)
    if hit is None:
        if weights is None:
            hit = (None, torch.ones(n, dtype=torch.float32, device=device))
        else:
            host = torch.tensor(weights, dtype=torch.float32).pin_memory()
            hit = (host, host.to(device, non_blocking=True))
        _weights_on[key] = hit
    return hit[1]


def fuse_wbf(rows: torch.Tensor, counts: torch.Tensor, view_map: torch.Tensor, frame_hw: torch.Tensor, weights=None, iou: float = 0.55,
             skip_score: float = 0.0, conf: str = "avg", rescale: bool = True, class_agnostic: bool = False, max_det: int = 300,
             overflow: Optional[torch.Tensor] = None):
    """``cvx_det_fuse_wbf``: the inputs of ``det_tta.fuse_views`` -- rows (S * B, K, 6) fp32 and counts (S * B) int32 as ``det_to_image``
    leaves them, slot ``k * B + b`` what source k reports for frame b; ``view_map`` (S * B, 4) fp32 [ax, cx, ay, cy]; ``frame_hw`` (B, 2)
    int32 -- and ``weights``: S positive finite host values, None for ones.  Per frame the rows go through their map (as in
    ``fuse_views``); those below ``skip_score`` or without area are left out; the rest are ordered by (class, score * weight descending,
    ordinal) and clustered class by class (one segment per frame with ``class_agnostic``): a box joins the cluster whose fused box it
    overlaps best, by more than ``iou``, or opens one; the fused box is the mean of the members weighted by score * weight.  ``conf``,
    ``rescale``: see ``WBF``.  Returns what ``fuse_views`` returns: (rows (B, max_det, 6) by score descending, counts (B) int32, source
    (B, max_det) int32 -- slot * K + row of each cluster's first member, -1 past the count --, members (B, max_det) int32, the overflow word
    (1) int32, added to when given).  A frame with more than ``FUSE_CAP`` rows has count -1 and adds 1 to the overflow word.  No host
    read."""
    if not (torch.is_tensor(rows) and rows.is_cuda):
        raise L.CvxError("box_fusion.fuse_wbf runs on an MI355X only: there is no CPU path")
    if rows.dim() != 3 or rows.shape[2] != 6 or rows.dtype != torch.float32 or rows.shape[0] <= 0 or rows.shape[1] <= 0:
        raise ValueError(f"rows: (S * B, K, 6) float32, got {tuple(rows.shape)} {rows.dtype}")
    SB, K = int(rows.shape[0]), int(rows.shape[1])
    if SB * K >= 2 ** 31:
        raise ValueError("rows: slots * K must stay below 2^31 (the ordinal is 32 bits)")
    if not torch.is_tensor(frame_hw) or frame_hw.dtype != torch.int32 or frame_hw.dim() != 2 or frame_hw.shape[1] != 2 or frame_hw.shape[0] <= 0 \
            or frame_hw.device != rows.device:
        raise ValueError("frame_hw: (B, 2) int32 on the rows' device")
    B = int(frame_hw.shape[0])
    if SB % B or not 1 <= SB // B <= MAX_SOURCES:
        raise ValueError(f"rows: {SB} slots are not 1 to {MAX_SOURCES} sources of {B} frames")
    S = SB // B
    if not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.numel() != SB or counts.device != rows.device:
        raise ValueError("counts: (S * B) int32 on the rows' device")
    if not torch.is_tensor(view_map) or view_map.dtype != torch.float32 or tuple(view_map.shape) != (SB, 4) or view_map.device != rows.device:
        raise ValueError("view_map: (S * B, 4) float32 [ax, cx, ay, cy] on the rows' device")
    weights = _checked_weights(weights, S)
    if conf not in CONF_MODES:
        raise ValueError(f"conf: one of {sorted(CONF_MODES)}, got {conf!r}")
    if not 0.0 <= float(iou) <= 1.0:
        raise ValueError("iou lies in [0, 1]")
    if not (math.isfinite(float(skip_score)) and float(skip_score) >= 0.0):
        raise ValueError("skip_score is finite and not negative")
    if not 1 <= int(max_det) <= FUSE_CAP:
        raise ValueError(f"max_det lies in [1, {FUSE_CAP}]")
    rows, counts, view_map, frame_hw = rows.contiguous(), counts.contiguous(), view_map.contiguous(), frame_hw.contiguous()
    out_rows = torch.empty(B, int(max_det), 6, dtype=torch.float32, device=rows.device)
    out_counts = torch.empty(B, dtype=torch.int32, device=rows.device)
    out_source = torch.empty(B, int(max_det), dtype=torch.int32, device=rows.device)
    out_members = torch.empty(B, int(max_det), dtype=torch.int32, device=rows.device)
    if overflow is None:
        overflow = torch.zeros(1, dtype=torch.int32, device=rows.device)
    lib = L.load()
    ws = L.workspace("det_fuse_wbf", rows.device, int(lib.cvx_det_wbf_workspace_bytes(B)))
    with torch.cuda.device(rows.device):
        w = _device_weights(weights, S, rows.device)
        L.check(lib.cvx_det_fuse_wbf(L.ptr(rows), L.ptr(counts), K, L.ptr(view_map), L.ptr(frame_hw), B, S, L.ptr(w), float(iou), float(skip_score),
                                     int(bool(class_agnostic)), CONF_MODES[conf], int(bool(rescale)), int(max_det), L.ptr(out_rows),
                                     L.ptr(out_counts), L.ptr(out_source), L.ptr(out_members), L.ptr(overflow), L.ptr(ws), ws.numel(),
                                     L.stream_ptr(rows.device)), "cvx_det_fuse_wbf")
    return out_rows, out_counts, out_source, out_members, overflow


class DetEnsemble:
    """Several detectors on the same frames, one answer.  ``members``: 1 to 32 of ``(algo, model)`` or ``(algo, model, weight)``, every
    ``algo`` one of the four detector classes (``core.algorithms.base.Detector``), all on one device with one ``num_classes``;
    ``fusion``: the ``WBF`` that fuses what the members report (its own ``weights`` must be None: a member's weight is the third element
    of its tuple, default 1); ``tta``: a ``det_tta.DetTTA`` every member runs behind -- each member fuses its own views as the ``DetTTA``
    says, then the ensemble fuses the members."""

    def __init__(self, members, fusion: Optional[WBF] = None, tta=None):
        from core.algorithms.base import Detector
        from .det_tta import DetTTA
        fusion = WBF() if fusion is None else fusion
        if not isinstance(fusion, WBF):
            raise ValueError(f"fusion: a box_fusion.WBF, got {type(fusion).__name__}")
        if fusion.weights is not None:
            raise ValueError("fusion.weights: an ensemble takes a member's weight from its tuple, (algo, model, weight)")
        if tta is not None and not isinstance(tta, DetTTA):
            raise ValueError(f"tta: a det_tta.DetTTA or None, got {type(tta).__name__}")
        members = [tuple(m) for m in members]
        if not 1 <= len(members) <= MAX_SOURCES:
            raise ValueError(f"members: 1 to {MAX_SOURCES}, got {len(members)}")
        if any(len(m) not in (2, 3) for m in members):
            raise ValueError("members: (algo, model) or (algo, model, weight)")
        self.algos, self.models = [m[0] for m in members], [m[1] for m in members]
        for a in self.algos:
            if not isinstance(a, Detector):
                raise ValueError(f"members: {type(a).__name__} is not one of the detectors")
        if len({torch.device(a.device) for a in self.algos}) != 1:
            raise ValueError(f"members: one device, got {[str(a.device) for a in self.algos]}")
        if len({int(a.num_classes) for a in self.algos}) != 1:
            raise ValueError(f"members: one num_classes, got {[a.num_classes for a in self.algos]}")
        self.weights = _checked_weights([m[2] if len(m) == 3 else 1.0 for m in members])
        self.fusion, self.tta = fusion, tta
        self.device, self.num_classes = self.algos[0].device, int(self.algos[0].num_classes)
        self.eval_max_det = max(int(a.eval_max_det) for a in self.algos)

    def _fuse(self, parts, image_hw, max_det):
        """[(rows, counts, flagged)] of the members, final boxes -> the fused (rows, counts); a frame a member's tail flagged comes back
        with count -1 and no rows"""
        device = parts[0][0].device
        B = int(parts[0][0].shape[0])
        slot_rows, slot_counts = pad_blocks([(r, c) for r, c, _ in parts], device)
        vmap = torch.zeros(len(parts) * B, 4, dtype=torch.float32, device=device)
        vmap[:, 0] = 1.0
        vmap[:, 2] = 1.0
        rows, counts, _, _, _ = self.fusion.fuse(slot_rows, slot_counts, vmap, image_hw.to(device, torch.int32), self.weights, max_det)
        bad = parts[0][2]
        for _, _, flagged in parts[1:]:
            bad = bad | flagged
        counts = torch.where(bad, torch.full_like(counts, -1), counts)
        rows = torch.where(bad.view(B, 1, 1), torch.zeros_like(rows), rows)
        return rows, counts

    @staticmethod
    def _member_rows(rows_of, images, meta, conf):
        from . import render
        rows, counts, box_map = rows_of(images, meta, conf)
        flagged = (counts < 0) | (counts > rows.shape[1])
        rows, counts, _ = render.det_to_image(rows, counts, box_map)
        return rows, counts, flagged

    def rows_of(self, max_det: Optional[int] = None, evaluation: bool = False):
        """A callable with the signature of what ``Detector._evaluation_rows`` returns, ``(images, meta, conf_threshold=0.001) -> (rows (B,
        max_det, 6), counts (B), None)`` with final boxes: every member's own tail (behind ``tta`` when the ensemble has one) on the same
        ``images``, ``render.det_to_image`` per member, the row blocks padded to one width, one ``cvx_det_fuse_wbf`` launch under identity
        maps.  A frame flagged by any member's tail comes back with count -1.  ``max_det`` defaults to the fusion's; ``evaluation`` lets a
        member's ``tta`` keep ``min(eval_max_det, 8192)`` rows, as ``Detector.evaluate_on_voc`` does.  No host read of its own."""
        max_det = self.fusion.max_det if max_det is None else int(max_det)
        tails = [a._augmented(m, self.tta, min(a.eval_max_det, FUSE_CAP) if evaluation else None) for a, m in zip(self.algos, self.models)]

        def ensemble_rows_of(images, meta, conf_threshold=0.001):
            parts = [self._member_rows(t, images, meta, conf_threshold) for t in tails]
            return (*self._fuse(parts, meta["image_hw"], max_det), None)

        return ensemble_rows_of

    def predict_batch(self, frames, conf_threshold=None, draw=False, sync=True, tracker=None):
        """``Detector.predict_batch`` for the ensemble: ``frames`` is a list of uint8 HWC RGB device tensors of any sizes.  Every member
        builds its own network batch (``render.FrameBatch`` at its own input size and letterboxing), runs its own tail at
        ``conf_threshold`` (default: its own configured one) and ``cvx_det_to_image``; one ``cvx_det_fuse_wbf`` launch fuses the members, and ``cvx_det_to_image`` turns a flagged frame into the overflow word.
        ``draw``, ``sync`` and ``tracker`` as in ``Detector.predict_batch``, on the fused rows ``(B, fusion.max_det, 6)``."""
        from . import render
        first = self.algos[0]
        first._need_gpu("DetEnsemble.predict_batch")
        frames = list(frames)
        parts, batch = [], None
        for algo, model in zip(self.algos, self.models):
            input_hw, letterbox = algo._predict_input()
            fb = render.FrameBatch(frames, input_hw, letterbox)
            batch = fb if batch is None else batch
            model.eval()
            conf = algo.conf_threshold if conf_threshold is None else conf_threshold
            parts.append(self._member_rows(algo._augmented(model, self.tta), fb.network_input(), {"image_hw": fb.image_hw}, conf))
        rows, counts, overflow = render.det_to_image(*self._fuse(parts, batch.image_hw, self.fusion.max_det))
        if tracker is not None:
            return first._tracked(tracker, frames, batch, rows, counts, overflow, draw, sync)
        if draw:
            render.draw_detections(frames, rows, counts, batch=batch)
        if sync:
            return render.read_detections(rows, counts, overflow)
        return rows, counts

    def _evaluation_tails(self, what):
        """the loader's images have one network size: every member must expect it"""
        inputs = {a._predict_input() for a in self.algos}
        if len(inputs) != 1:
            raise ValueError(f"{what}: the dataloader's images have one network size and letterboxing, the members expect {sorted(inputs)}; "
                             "predict_batch builds each member's own input")
        for m in self.models:
            m.eval()
        return self.rows_of(min(self.eval_max_det, FUSE_CAP), evaluation=True)

    def evaluate_on_voc(self, map_out_root, subset="val", dataloader=None, capacity=None, coco_metric=False, diagnostics=None):
        """``Detector.evaluate_on_voc`` on the ensemble's fused rows (at most ``min(eval_max_det, 8192)`` per image); the dataloader and the
        result are those of the detectors' method, ``diagnostics`` included.  All members must share ``_predict_input()``."""
        if subset not in ("val", "test"):
            raise ValueError(f"sub_set must be one of 'test' and 'val', but got {subset}")
        if dataloader is None:
            raise L.CvxError("evaluate_on_voc reads no dataset from disk: pass dataloader= yielding (images, dict(image_hw, gt, gt_counts)) on the "
                             "device over the VOC-" + subset + " pictures in sorted-id order")
        from . import det_eval
        from configs.dataset_cfg import VOC_CFG
        return det_eval.evaluate_detector(self._evaluation_tails("evaluate_on_voc"), dataloader, self.num_classes, self.device, map_out_root,
                                          det_eval.class_names(VOC_CFG, self.num_classes), self.eval_max_det, capacity, coco_metric, diagnostics)

    def evaluate_on_coco(self, map_out_root, subset="val", dataloader=None, capacity=None):
        """``Detector.evaluate_on_coco`` on the ensemble's fused rows; see ``evaluate_on_voc``"""
        from . import coco_eval
        coco_eval.check_coco_arguments(subset, dataloader)
        return coco_eval.evaluate_detector_coco(self._evaluation_tails("evaluate_on_coco"), dataloader, self.num_classes, map_out_root,
                                                self.eval_max_det, capacity)
