"""Multi-scale and flip test-time augmentation for DeepLabv3+ on the device (``csrc/seg_tta.hip``).

The network runs on the batch at several zooms and on its mirror image; the per-pixel class scores of all views are brought to the
picture's size, fused, and the arg max of the fusion is the label.  Per scale: one ``cvx_seg_tta_inputs`` launch (resize, then mirror) and
one ``model.forward_rows`` on the ``B * (1 + flip)`` batch -- the model keeps one engine per input size over one set of weight arenas.
Then one ``cvx_seg_fuse`` launch for all views: labels, confusion counts and, in ``"prob"`` mode, the mean probabilities.  Nothing waits
on the host and no full-resolution logits exist in memory.  The reference has no counterpart; ``tests/seg_tta_restatement.py`` is the
specification.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

MIN_VIEW = 33                                   # the engine's smallest input (deeplab.build_deeplab_graph)
MAX_VIEWS = 16                                  # the view table is a kernel argument: 16 entries of 24 bytes
MODES = {"logits": 0, "prob": 1}


class SegView(NamedTuple):
    """One view of the fusion: ``rows`` (B, lh * lw, ld) fp32 on the device as ``forward_rows`` leaves them, the logit level's size, and
    whether the view saw the mirrored picture."""
    rows: torch.Tensor
    level_hw: Tuple[int, int]
    flip: bool


def view_size(n: int, s: float) -> int:
    """The extent of a view of an ``n``-pixel axis at zoom ``s``: ``floor(n * s + 0.5)``, refused below the engine's minimum input"""
    v = int(math.floor(n * s + 0.5))
    if v < MIN_VIEW:
        raise ValueError(f"a view of {n} pixels at scale {s} is {v} pixels: the network takes no input below {MIN_VIEW}")
    return v


def tta_inputs(images: torch.Tensor, out_hw, flip: bool = False) -> torch.Tensor:
    """``cvx_seg_tta_inputs``: (B, c, h, w) fp32 on the device -> (B * (1 + flip), c, oh, ow): the bilinear resize (``align_corners=False``,
    no antialiasing) and, behind it, the same pictures mirrored along x.  One launch, no host read."""
    if not (torch.is_tensor(images) and images.is_cuda):
        raise L.CvxError("seg_tta.tta_inputs runs on an MI355X only (there is no CPU path)")
    if images.dim() != 4 or images.dtype != torch.float32:
        raise ValueError("images: (B, c, h, w) float32")
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if oh <= 0 or ow <= 0:
        raise ValueError("out_hw is positive")
    images = images.contiguous()
    B, c, h, w = (int(v) for v in images.shape)
    out = torch.empty(B * (2 if flip else 1), c, oh, ow, dtype=torch.float32, device=images.device)
    with torch.cuda.device(images.device):
        L.check(L.load().cvx_seg_tta_inputs(L.ptr(images), B, c, h, w, oh, ow, int(bool(flip)), L.ptr(out), L.stream_ptr(images.device)),
                "cvx_seg_tta_inputs")
    return out


def fuse(views: Sequence[SegView], nc: int, ld: int, out_hw, targets: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
         probs: bool = False, mode: str = "prob", labels: bool = True):
    """``cvx_seg_fuse``: per pixel of the ``out_hw`` picture the logits of every view, up-sampled from its level by the taps of
    ``cvx_resize_bilinear_rows_to_nchw`` (read at the mirrored column for a flipped view) and fused in the order of ``views`` --
    ``"logits"``: their sum; ``"prob"``: the sum of their softmax.  Returns the (B, H, W) uint8 labels on the device (None with
    ``labels=False``) and, with ``probs`` (``"prob"`` only), ``(labels, (B, nc, H, W) mean probabilities)``.  ``targets`` ((B, H, W) int64)
    with ``counts`` ((nc, nc) int64 on the device): ``counts[target][label] += 1`` for targets in [0, nc).  One launch, no host read."""
    views = list(views)
    nc, ld = int(nc), int(ld)
    H, W = int(out_hw[0]), int(out_hw[1])
    if mode not in MODES:
        raise ValueError(f"mode: one of {sorted(MODES)}, got {mode!r}")
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError(f"1 to {MAX_VIEWS} views, got {len(views)}")
    if not 1 <= nc <= 256 or ld < nc:
        raise ValueError(f"nc {nc}, ld {ld}: labels are bytes, 1 <= nc <= 256, and nc <= ld")
    if H <= 0 or W <= 0:
        raise ValueError("out_hw is positive")
    if probs and mode != "prob":
        raise ValueError("probabilities are an output of mode 'prob' only")
    if (targets is None) != (counts is None):
        raise ValueError("targets and counts come together")
    if not (labels or probs or counts is not None):
        raise ValueError("no output asked for")
    for v in views:
        if not torch.is_tensor(v.rows):
            raise ValueError("a view's rows are a tensor")
    if not all(v.rows.is_cuda for v in views):
        raise L.CvxError("seg_tta.fuse runs on an MI355X only (there is no CPU path)")
    dev, B = views[0].rows.device, int(views[0].rows.shape[0])
    table = np.zeros(len(views), dtype=L.SEG_VIEW_DTYPE)
    keep = []
    for k, v in enumerate(views):
        lh, lw = int(v.level_hw[0]), int(v.level_hw[1])
        if lh <= 0 or lw <= 0 or v.rows.dim() != 3 or tuple(v.rows.shape) != (B, lh * lw, ld) or v.rows.dtype != torch.float32 or v.rows.device != dev:
            raise ValueError(f"view {k}: rows ({B}, {lh * lw}, {ld}) float32 on {dev}, got {tuple(v.rows.shape)} {v.rows.dtype} on {v.rows.device}")
        rows = v.rows.contiguous()
        keep.append(rows)
        table[k] = (rows.data_ptr(), lh, lw, int(bool(v.flip)), 0)
    if targets is not None:
        if not torch.is_tensor(targets) or tuple(targets.shape) != (B, H, W):
            raise ValueError(f"targets: ({B}, {H}, {W})")
        if not torch.is_tensor(counts) or counts.dtype != torch.int64 or tuple(counts.shape) != (nc, nc) or counts.device != dev or not counts.is_contiguous():
            raise ValueError(f"counts: ({nc}, {nc}) int64, contiguous, on {dev}")
        targets = targets.to(device=dev, dtype=torch.long, non_blocking=True).contiguous()
    out = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if labels else None
    p = torch.empty(B, nc, H, W, dtype=torch.float32, device=dev) if probs else None
    with torch.cuda.device(dev):
        L.check(L.load().cvx_seg_fuse(table.ctypes.data_as(L.C.c_void_p), len(views), ld, B, nc, H, W, MODES[mode], L.ptr(out), L.ptr(targets),
                                      L.ptr(counts), L.ptr(p), L.stream_ptr(dev)), "cvx_seg_fuse")
    return (out, p) if probs else out


class SegTTA:
    """The views of one test-time augmentation: ``scales`` (zooms of the picture, ``view_size``) times plain / mirrored.  The view order is
    scale-major, the plain half before the flipped half.  ``mode``: ``"prob"`` averages the views' softmax, ``"logits"`` their logits."""

    def __init__(self, scales: Sequence[float] = (1.0,), flip: bool = False, mode: str = "prob"):
        scales = tuple(float(s) for s in scales)
        if not scales or any(not math.isfinite(s) or s <= 0.0 for s in scales):
            raise ValueError(f"scales: positive finite zooms, got {scales}")
        flip = bool(flip)
        if len(scales) * (2 if flip else 1) > MAX_VIEWS:
            raise ValueError(f"{len(scales)} scales{' with flip' if flip else ''} are more than {MAX_VIEWS} views")
        if mode not in MODES:
            raise ValueError(f"mode: one of {sorted(MODES)}, got {mode!r}")
        self.scales, self.flip, self.mode = scales, flip, mode

    @property
    def n_views(self) -> int:
        return len(self.scales) * (2 if self.flip else 1)

    def view_sizes(self, h: int, w: int) -> List[Tuple[int, int]]:
        """the network input of each scale for an (h, w) picture"""
        return [(view_size(h, s), view_size(w, s)) for s in self.scales]

    def run(self, model, images: torch.Tensor) -> List[SegView]:
        """Per scale one ``cvx_seg_tta_inputs`` launch and one ``model.forward_rows`` on the ``B * (1 + flip)`` batch.  ``forward_rows``
        writes every call's rows into a tensor of their own, so the views stay valid while the next scale runs.  Returns the view list
        without a host wait."""
        if not (torch.is_tensor(images) and images.is_cuda):
            raise L.CvxError("SegTTA.run runs on an MI355X only (there is no CPU path)")
        if images.dim() != 4:
            raise ValueError("images: (B, 3, H, W)")
        B, H, W = int(images.shape[0]), int(images.shape[2]), int(images.shape[3])
        sizes = self.view_sizes(H, W)
        images = images.float()
        views = []
        with torch.no_grad():
            for hw in sizes:
                rows = model.forward_rows(tta_inputs(images, hw, self.flip))
                level = tuple(int(v) for v in model._last_engine.graph.level_hw[0])
                views.append(SegView(rows[:B], level, False))
                if self.flip:
                    views.append(SegView(rows[B:], level, True))
        return views

    def fuse(self, views, nc, ld, out_hw, targets=None, counts=None, probs=False, labels=True):
        return fuse(views, nc, ld, out_hw, targets=targets, counts=counts, probs=probs, mode=self.mode, labels=labels)
