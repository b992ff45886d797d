"""Scale and flip test-time augmentation for the four detectors on the device (``csrc/det_tta.hip``).

The network runs on the batch at a few zooms and on its mirror image, and the boxes of all views of a frame are fused.  Every view has the
network's own input size -- the picture, resized by ``z <= 1``, sits in the middle of the letterbox's grey --, so the engine and its planned
batch size do not change.  One ``cvx_det_tta_inputs`` launch builds all ``V * B`` slots (view-major: slot ``k * B + b``), the class's own
tail runs on the ``B`` slots of each view, and one ``cvx_det_fuse_views`` launch maps every row back to the picture and fuses the views:
greedy suppression alone (``"nms"``) or with the kept boxes voted by their members (``"vote"``, the ``merge`` of YOLOv5's NMS).  Nothing
waits on the host.  The reference has no counterpart; ``tests/det_tta_restatement.py`` is the specification.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L

MAX_VIEWS = 8                                   # the view table is a kernel argument: 8 entries of 24 bytes
MIN_CONTENT = 32                                # pixels of picture a view keeps per axis, at least
FUSE_CAP = 8192                                 # candidates per frame cvx_det_fuse_views sorts
FUSE_MODES = {"nms": 0, "vote": 1}
SCORE_MODES = {"max": 0, "views": 1}
PAD = 128 / 255


def view_size(n: int, z: float) -> int:
    """The extent of an ``n``-pixel axis in a view at zoom ``z``: ``floor(n * z + 0.5)``, the rounding of ``seg_tta.view_size``; refused
    below ``MIN_CONTENT``"""
    v = int(math.floor(n * z + 0.5))
    if v < MIN_CONTENT:
        raise ValueError(f"a view of {n} pixels at zoom {z} keeps {v} pixels of the picture: fewer than {MIN_CONTENT}")
    return v


def view_table(views, input_hw) -> np.ndarray:
    """``cvx_det_view`` rows for ``views`` = [(h_k, w_k, flip_k)] inside an ``input_hw`` network input: the content in the middle"""
    H, W = int(input_hw[0]), int(input_hw[1])
    views = list(views)
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError(f"1 to {MAX_VIEWS} views, got {len(views)}")
    table = np.zeros(len(views), dtype=L.DET_VIEW_DTYPE)
    for k, (h, w, flip) in enumerate(views):
        h, w = int(h), int(w)
        if not (1 <= h <= H and 1 <= w <= W):
            raise ValueError(f"view {k}: a content size of {(h, w)} does not fit the network input {(H, W)}")
        table[k] = (h, w, (H - h) // 2, (W - w) // 2, int(bool(flip)), 0)
    return table


def tta_inputs(images: torch.Tensor, table: np.ndarray, pad: float = PAD, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``cvx_det_tta_inputs``: (B, 3, H, W) fp32 on the device and a ``view_table`` of V views -> (V * B, 3, H, W), slot ``k * B + b`` --
    picture b resized to view k's content size (bilinear, ``align_corners=False``, no antialiasing) inside its rectangle, ``pad`` around
    it, mirrored along x for a flipped view.  ``out``: a contiguous fp32 tensor of at least V * B slots to write into; its further slots
    stay as they are.  One launch, no host read."""
    if not (torch.is_tensor(images) and images.is_cuda):
        raise L.CvxError("det_tta.tta_inputs runs on an MI355X only (there is no CPU path)")
    if images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32:
        raise ValueError("images: (B, 3, H, W) float32")
    if not isinstance(table, np.ndarray) or table.dtype != L.DET_VIEW_DTYPE or table.ndim != 1 or not 1 <= len(table) <= MAX_VIEWS:
        raise ValueError(f"table: 1 to {MAX_VIEWS} cvx_det_view rows (view_table)")
    if not math.isfinite(float(pad)):
        raise ValueError("pad is finite")
    images = images.contiguous()
    B, _, H, W = (int(v) for v in images.shape)
    V = len(table)
    if out is None:
        out = torch.empty(V * B, 3, H, W, dtype=torch.float32, device=images.device)
    elif (out.dtype != torch.float32 or out.dim() != 4 or tuple(out.shape[1:]) != (3, H, W) or out.shape[0] < V * B or out.device != images.device
          or not out.is_contiguous()):
        raise ValueError(f"out: (>= {V * B}, 3, {H}, {W}) float32, contiguous, on {images.device}")
    table = np.ascontiguousarray(table)
    with torch.cuda.device(images.device):
        L.check(L.load().cvx_det_tta_inputs(L.ptr(images), B, H, W, table.ctypes.data_as(L.C.c_void_p), V, float(pad), L.ptr(out),
                                            L.stream_ptr(images.device)), "cvx_det_tta_inputs")
    return out


def box_map_terms(image_hw: torch.Tensor, input_hw, letterbox: bool):
    """The affine map a tail reports its boxes through, ``x_rep = (x_net - px) * gx``: float64 (px, py, gx, gy), each (B), on ``image_hw``'s
    device.  The arithmetic of ``det_eval.letterbox_box_map`` / ``correct_boxes_device``; plain stretching without ``letterbox``."""
    in_h, in_w = float(input_hw[0]), float(input_hw[1])
    hw = image_hw.to(torch.float64)
    img_h, img_w = hw[:, 0], hw[:, 1]
    if letterbox:
        gain = torch.maximum(img_h / in_h, img_w / in_w)
        return torch.floor((in_w - img_w / gain) / 2), torch.floor((in_h - img_h / gain) / 2), gain, gain
    zero = torch.zeros_like(img_h)
    return zero, zero, img_w / in_w, img_h / in_h


def pad_blocks(parts, device):
    """[(rows (B, K_k, 6), counts (B))] of S sources -> (rows (S * B, K, 6), counts (S * B)), slot ``k * B + b``: the tails' row blocks may
    differ in size -- one block, the rest zero"""
    B = int(parts[0][0].shape[0])
    K = max(int(r.shape[1]) for r, _ in parts)
    slot_rows = torch.zeros(len(parts) * B, K, 6, dtype=torch.float32, device=device)
    for k, (r, _) in enumerate(parts):
        slot_rows[k * B:(k + 1) * B, :r.shape[1]] = r
    return slot_rows, torch.cat([c for _, c in parts])


def fuse_views(rows: torch.Tensor, counts: torch.Tensor, view_map: torch.Tensor, frame_hw: torch.Tensor, threshold: float = 0.5,
               class_agnostic: bool = False, fuse: str = "vote", score: str = "max", max_det: int = 300, overflow: Optional[torch.Tensor] = None):
    """``cvx_det_fuse_views``: rows (V * B, K, 6) fp32 and counts (V * B) int32 as ``det_to_image`` leaves them, slot ``k * B + b``;
    ``view_map`` (V * B, 4) fp32 [ax, cx, ay, cy] and ``frame_hw`` (B, 2) int32 on the same device.  Per frame the rows of its V slots go
    through their map (``x * ax + cx``, corners re-ordered, clamped to the frame), are ordered by (score, ordinal) and suppressed greedily
    by IoU above ``threshold`` (inside a class unless ``class_agnostic``).  ``fuse="vote"``: a kept box becomes the mean of its members --
    itself and every candidate it overlaps by more than ``threshold`` -- weighted by IoU * score.  ``score="views"``: a kept score is scaled
    by the share of the views that have a member.  Returns (rows (B, max_det, 6), counts (B) int32, source (B, max_det) int32 -- slot * K +
    row of each kept row, -1 past the count --, members (B, max_det) int32, the overflow word (1) int32, added to when given).  A frame
    with more than ``FUSE_CAP`` candidates has count -1 and adds 1 to the overflow word.  No host read."""
    if not (torch.is_tensor(rows) and rows.is_cuda):
        raise L.CvxError("det_tta.fuse_views runs on an MI355X only: there is no CPU path")
    if rows.dim() != 3 or rows.shape[2] != 6 or rows.dtype != torch.float32 or rows.shape[0] <= 0 or rows.shape[1] <= 0:
        raise ValueError(f"rows: (V * B, K, 6) float32, got {tuple(rows.shape)} {rows.dtype}")
    S, K = int(rows.shape[0]), int(rows.shape[1])
    if S * K >= 2 ** 31:
        raise ValueError("rows: slots * K must stay below 2^31 (the ordinal is 32 bits)")
    if not torch.is_tensor(frame_hw) or frame_hw.dtype != torch.int32 or frame_hw.dim() != 2 or frame_hw.shape[1] != 2 or frame_hw.shape[0] <= 0 \
            or frame_hw.device != rows.device:
        raise ValueError("frame_hw: (B, 2) int32 on the rows' device")
    B = int(frame_hw.shape[0])
    if S % B or not 1 <= S // B <= MAX_VIEWS:
        raise ValueError(f"rows: {S} slots are not 1 to {MAX_VIEWS} views of {B} frames")
    if not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.numel() != S or counts.device != rows.device:
        raise ValueError("counts: (V * B) int32 on the rows' device")
    if not torch.is_tensor(view_map) or view_map.dtype != torch.float32 or tuple(view_map.shape) != (S, 4) or view_map.device != rows.device:
        raise ValueError("view_map: (V * B, 4) float32 [ax, cx, ay, cy] on the rows' device")
    if fuse not in FUSE_MODES:
        raise ValueError(f"fuse: one of {sorted(FUSE_MODES)}, got {fuse!r}")
    if score not in SCORE_MODES:
        raise ValueError(f"score: one of {sorted(SCORE_MODES)}, got {score!r}")
    if not 0.0 <= float(threshold) <= 1.0:
        raise ValueError("threshold lies in [0, 1]")
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
    ws = L.workspace("det_fuse_views", rows.device, int(lib.cvx_det_merge_workspace_bytes(B)))
    with torch.cuda.device(rows.device):
        L.check(lib.cvx_det_fuse_views(L.ptr(rows), L.ptr(counts), K, L.ptr(view_map), L.ptr(frame_hw), B, S // B, float(threshold),
                                       int(bool(class_agnostic)), FUSE_MODES[fuse], SCORE_MODES[score], int(max_det), L.ptr(out_rows),
                                       L.ptr(out_counts), L.ptr(out_source), L.ptr(out_members), L.ptr(overflow), L.ptr(ws), ws.numel(),
                                       L.stream_ptr(rows.device)), "cvx_det_fuse_views")
    return out_rows, out_counts, out_source, out_members, overflow


class DetTTA:
    """The views of one test-time augmentation: view k is the picture at zoom ``scales[k]``, mirrored when ``flips[k]``.  The defaults
    are YOLOv5's three (``augment=True``).  ``fuse``: ``"vote"`` or ``"nms"``; ``iou``: the fusion's IoU threshold, None for the
    detector's configured NMS threshold; ``score``: ``"max"`` or ``"views"``; ``max_det``: rows per frame after the fusion; ``pad``: the
    value around a view's content.  ``fusion``: a ``box_fusion.WBF`` -- the views are then fused by Weighted Boxes Fusion
    (``cvx_det_fuse_wbf``) with the views as its sources, ``fusion.weights`` one per view or None for ones; ``fuse``, ``iou``, ``score`` and
    ``class_agnostic`` are unused (the ``WBF`` has its own), ``max_det`` still bounds the rows.  With None every path is what it was."""

    def __init__(self, scales: Sequence[float] = (1.0, 0.83, 0.67), flips: Sequence[bool] = (False, True, False), fuse: str = "vote",
                 iou: Optional[float] = None, score: str = "max", class_agnostic: bool = False, max_det: int = 300, pad: float = PAD, fusion=None):
        scales, flips = tuple(float(z) for z in scales), tuple(bool(f) for f in flips)
        if not scales or len(scales) != len(flips):
            raise ValueError(f"scales and flips: one entry per view, got {len(scales)} and {len(flips)}")
        if len(scales) > MAX_VIEWS:
            raise ValueError(f"{len(scales)} views are more than {MAX_VIEWS}")
        if any(not math.isfinite(z) or z <= 0.0 for z in scales):
            raise ValueError(f"scales: positive finite zooms, got {scales}")
        if any(z > 1.0 for z in scales):
            raise ValueError(f"scales {scales}: a view is the picture at a zoom of at most 1 inside the network input; for objects too small "
                             "at zoom 1 use predict_tiled")
        if fuse not in FUSE_MODES:
            raise ValueError(f"fuse: one of {sorted(FUSE_MODES)}, got {fuse!r}")
        if score not in SCORE_MODES:
            raise ValueError(f"score: one of {sorted(SCORE_MODES)}, got {score!r}")
        if iou is not None and not 0.0 <= float(iou) <= 1.0:
            raise ValueError("iou lies in [0, 1]")
        if not 1 <= int(max_det) <= FUSE_CAP:
            raise ValueError(f"max_det lies in [1, {FUSE_CAP}]")
        if not math.isfinite(float(pad)):
            raise ValueError("pad is finite")
        self.scales, self.flips, self.fuse_mode, self.score = scales, flips, fuse, score
        self.iou = None if iou is None else float(iou)
        self.class_agnostic, self.max_det, self.pad = bool(class_agnostic), int(max_det), float(pad)
        if fusion is not None:
            from .box_fusion import WBF
            if not isinstance(fusion, WBF):
                raise ValueError(f"fusion: a box_fusion.WBF or None, got {type(fusion).__name__}")
            if fusion.weights is not None and len(fusion.weights) != len(scales):
                raise ValueError(f"fusion.weights: one per view, {len(scales)}, got {len(fusion.weights)}")
        self.fusion = fusion

    @property
    def n_views(self) -> int:
        return len(self.scales)

    def views(self, input_hw):
        """[(h_k, w_k, flip_k)] for an ``input_hw`` network input"""
        H, W = int(input_hw[0]), int(input_hw[1])
        return [(view_size(H, z), view_size(W, z), f) for z, f in zip(self.scales, self.flips)]

    def inputs(self, x: torch.Tensor) -> torch.Tensor:
        """(B, 3, H, W) -> (V * B, 3, H, W), view-major: one ``cvx_det_tta_inputs`` launch"""
        if not (torch.is_tensor(x) and x.is_cuda):
            raise L.CvxError("DetTTA.inputs runs on an MI355X only (there is no CPU path)")
        if x.dim() != 4:
            raise ValueError("images: (B, 3, H, W)")
        return tta_inputs(x, view_table(self.views(x.shape[2:]), x.shape[2:]), self.pad)

    def view_map(self, image_hw: torch.Tensor, input_hw, letterbox: bool = True, terms=None) -> torch.Tensor:
        """(V * B, 4) fp32 [ax, cx, ay, cy], slot ``k * B + b``: what the tail reports for view k of picture b -> its true place in the
        picture, ``x_true = ax * x_rep + cx``.  The tail reports through ``x_rep = (x_net - px) * gx``; ``terms`` are its float64
        (px, py, gx, gy) (``Detector._box_map_terms``), by default ``box_map_terms(image_hw, input_hw, letterbox)``.  With s = w_k / W:
        a = 1 / s, c = gx * (px * (1 / s - 1) - left_k / s), and for a flipped view a = -1 / s, c = gx * ((W - px - left_k) / s - px);
        likewise y, which is never flipped.  float64 torch operations on ``image_hw``'s device, rounded once; no host read."""
        H, W = int(input_hw[0]), int(input_hw[1])
        px, py, gx, gy = box_map_terms(image_hw, (H, W), letterbox) if terms is None else terms
        out = []
        for h, w, top, left, flip, _ in view_table(self.views((H, W)), (H, W)).tolist():
            rx, ry = W / w, H / h                                  # 1 / s, float64
            if flip:
                ax, cx = torch.full_like(gx, -rx), gx * ((W - px - left) * rx - px)
            else:
                ax, cx = torch.full_like(gx, rx), gx * (px * (rx - 1.0) - left * rx)
            ay, cy = torch.full_like(gy, ry), gy * (py * (ry - 1.0) - top * ry)
            out.append(torch.stack((ax, cx, ay, cy), 1))
        return torch.cat(out).to(torch.float32).contiguous()

    def fuse(self, rows, counts, view_map, frame_hw, iou: Optional[float] = None, max_det: Optional[int] = None, overflow=None):
        """``fuse_views`` with this object's parameters; ``iou`` stands in where the object has none.  With a ``fusion``: its ``fuse_wbf``"""
        if self.fusion is not None:
            return self.fusion.fuse(rows, counts, view_map, frame_hw, None, self.max_det if max_det is None else max_det, overflow)
        thr = self.iou if self.iou is not None else iou
        if thr is None:
            raise ValueError("iou: this DetTTA has no threshold of its own; pass iou=")
        return fuse_views(rows, counts, view_map, frame_hw, thr, self.class_agnostic, self.fuse_mode, self.score,
                          self.max_det if max_det is None else max_det, overflow)

    def wrap(self, detector, rows_of, max_det: Optional[int] = None):
        """``rows_of`` of ``Detector._evaluation_rows`` -> a callable with the same signature that runs it on every view and returns
        ``(rows (B, max_det, 6), counts (B), None)`` with final boxes: one ``cvx_det_tta_inputs`` launch, ``rows_of`` on the B slots of
        each view (``meta`` unchanged), ``render.det_to_image`` per view, the row blocks padded to one width, one ``cvx_det_fuse_views``
        launch (``cvx_det_fuse_wbf`` with a ``fusion``).  A frame one of whose views overflowed its tail comes back with count -1, as the
        tail's own overflow does.  No host read of its own."""
        from . import render
        nms = getattr(detector, "iou_threshold", None)
        nms = getattr(detector, "nms_threshold", None) if nms is None else nms
        max_det = self.max_det if max_det is None else int(max_det)
        V = self.n_views

        def tta_rows_of(images, meta, conf_threshold=0.001):
            x = images.to(detector.device, torch.float32)
            B, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
            image_hw = meta["image_hw"].to(x.device)
            views = self.inputs(x)
            vmap = self.view_map(image_hw, (H, W), terms=detector._box_map_terms(image_hw, (H, W)))
            parts, bad = [], None
            for k in range(V):
                rows, counts, box_map = rows_of(views[k * B:(k + 1) * B], meta, conf_threshold)
                flagged = (counts < 0) | (counts > rows.shape[1])
                bad = flagged if bad is None else bad | flagged
                rows, counts, _ = render.det_to_image(rows, counts, box_map)
                parts.append((rows, counts))
            slot_rows, slot_counts = pad_blocks(parts, x.device)
            rows, counts, _, _, _ = self.fuse(slot_rows, slot_counts, vmap, image_hw.to(torch.int32), iou=nms, max_det=max_det)
            counts = torch.where(bad, torch.full_like(counts, -1), counts)
            rows = torch.where(bad.view(B, 1, 1), torch.zeros_like(rows), rows)
            return rows, counts, None

        return tta_rows_of
