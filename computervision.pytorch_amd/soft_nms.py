"""Soft-NMS on the device (``csrc/soft_nms.hip``).

Soft-NMS (Bodla et al., ICCV 2017) decays the score of a box that overlaps a better one instead of deleting it: ``linear`` multiplies the
score by ``1 - IoU`` above the threshold, ``gaussian`` by ``exp(-IoU^2 / sigma)`` for any overlap.  A box in a crowd keeps a place in the
ranking, which is what COCO-style AP at a confidence threshold of 0.001 counts.  The pick order depends on the scores as they change, so
this is a kernel of its own, ``cvx_soft_nms``, beside ``cvx_nms_variant``: same input, same outputs.  ``engine.nms(..., soft=SoftNMS(...))``
dispatches to it, and the YOLOv8, YOLOv7 and SSD tails pass ``cfg.decode.soft_nms`` there.  ``include/cvx_engine.h`` states the rules;
``tests/soft_nms_restatement.py`` restates them in numpy float32, and the kernel equals it bit for bit.
"""
from __future__ import annotations

import numbers
from typing import Optional

import torch

from . import _lib as L

METHODS = {"hard": 0, "linear": 1, "gaussian": 2}
FLAG_BOXES_XYXY = 0x100          # CVX_NMS_BOXES_XYXY
FLAG_CLASS_AGNOSTIC = 0x200      # CVX_SOFT_NMS_CLASS_AGNOSTIC
CAPACITY = 16384                 # candidates per block, and the most rows per block


class SoftNMS:
    """The parameters of one Soft-NMS.  ``method``: ``"gaussian"`` (any overlap o decays the score by ``exp(-o^2 / sigma)``), ``"linear"``
    (an overlap above ``iou`` decays it by ``1 - o``) or ``"hard"`` (an overlap above ``iou`` removes the box: plain per-class NMS through
    the same kernel).  ``sigma`` lies in [0.05, 10]; ``iou`` in [0, 1], None for the detector's configured NMS threshold; a segment stops
    when its best remaining score is not above ``min_score``, in [0, 1) (not in ``"hard"``).  ``class_agnostic``: boxes of different classes
    decay each other -- then one wave of the kernel walks the whole image (DESIGN.md section 7w has the timings)."""

    def __init__(self, method: str = "gaussian", sigma: float = 0.5, iou: Optional[float] = None, min_score: float = 0.001,
                 class_agnostic: bool = False):
        if method not in METHODS:
            raise ValueError(f"method: one of {sorted(METHODS)}, got {method!r}")
        if not (isinstance(sigma, numbers.Real) and 0.05 <= float(sigma) <= 10.0):
            raise ValueError(f"sigma lies in [0.05, 10], got {sigma!r}")
        if iou is not None and not (isinstance(iou, numbers.Real) and 0.0 <= float(iou) <= 1.0):
            raise ValueError(f"iou lies in [0, 1] (None: the detector's NMS threshold), got {iou!r}")
        if not (isinstance(min_score, numbers.Real) and 0.0 <= float(min_score) < 1.0):
            raise ValueError(f"min_score lies in [0, 1), got {min_score!r}")
        self.method, self.sigma, self.iou = method, float(sigma), None if iou is None else float(iou)
        self.min_score, self.class_agnostic = float(min_score), bool(class_agnostic)

    def __repr__(self):
        return (f"SoftNMS(method={self.method!r}, sigma={self.sigma}, iou={self.iou}, min_score={self.min_score}, "
                f"class_agnostic={self.class_agnostic})")

    @staticmethod
    def of(value) -> Optional["SoftNMS"]:
        """``cfg.decode.soft_nms`` -> None, or the ``SoftNMS`` it describes (a dict of the keywords above, or a ``SoftNMS``)"""
        if value is None or isinstance(value, SoftNMS):
            return value
        if isinstance(value, dict):
            return SoftNMS(**value)
        raise ValueError(f"soft_nms: None, a dict of SoftNMS keywords or a SoftNMS, got {type(value).__name__}")


def configured(cfg) -> Optional[SoftNMS]:
    """The ``SoftNMS`` of ``cfg.decode.soft_nms``; None where the field is absent or None"""
    return SoftNMS.of(getattr(getattr(cfg, "decode", None), "soft_nms", None))


def soft_nms(y: torch.Tensor, conf_thres: float, soft: SoftNMS, iou_thres: float, max_det: int = 300, boxes_xyxy: bool = False):
    """The bare ``cvx_soft_nms`` launch: y (B, 4+nc, A) fp32 -> (rows (B, max_det, 6) [x1, y1, x2, y2, final score, cls], anchor_index
    (B, max_det) int32, counts (B,) int32), all on the device, exactly like ``engine.nms``.  ``iou_thres`` stands in where ``soft.iou`` is
    None.  A block with more than 16384 candidates has count -1.  No host read."""
    if not (torch.is_tensor(y) and y.is_cuda):
        raise L.CvxError("soft_nms.soft_nms runs on an MI355X only: there is no CPU path")
    if not isinstance(soft, SoftNMS):
        raise ValueError(f"soft: a soft_nms.SoftNMS, got {type(soft).__name__}")
    iou = float(iou_thres if soft.iou is None else soft.iou)
    if not (0 <= conf_thres <= 1 and 0 <= iou <= 1):
        raise AssertionError("thresholds must lie in [0, 1]")
    if y.dim() != 3 or y.shape[1] < 5 or y.shape[0] <= 0 or y.shape[2] <= 0:
        raise ValueError(f"y: (B, 4 + nc, A), got {tuple(y.shape)}")
    if not 1 <= int(max_det) <= CAPACITY:
        raise ValueError(f"max_det lies in [1, {CAPACITY}]")
    lib = L.load()
    y = y.contiguous().float()
    B, ch, A = y.shape
    ws = L.workspace("soft_nms", y.device, int(lib.cvx_soft_nms_workspace_bytes(B, A)))
    rows = torch.empty(B, int(max_det), 6, dtype=torch.float32, device=y.device)
    index = torch.empty(B, int(max_det), dtype=torch.int32, device=y.device)
    counts = torch.empty(B, dtype=torch.int32, device=y.device)
    flags = (FLAG_BOXES_XYXY if boxes_xyxy else 0) | (FLAG_CLASS_AGNOSTIC if soft.class_agnostic else 0)
    with torch.cuda.device(y.device):
        L.check(lib.cvx_soft_nms(L.ptr(y), B, A, ch - 4, float(conf_thres), iou, int(max_det), METHODS[soft.method], soft.sigma, soft.min_score,
                                 flags, L.ptr(rows), L.ptr(index), L.ptr(counts), L.ptr(ws), ws.numel(), L.stream_ptr(y.device)), "cvx_soft_nms")
    return rows, index, counts
