"""Boundary metrics for segmentation on the device (``csrc/seg_boundary.hip``): trimap mIoU, Boundary IoU and BF.

A global confusion matrix cannot see what ``segment_tiled``, test-time augmentation and the region losses are for: border pixels are a
few per cent of a picture.  This module counts, in bands of given widths around the label changes, the three measures the field uses:
the trimap mIoU of the DeepLab papers, Boundary IoU (Cheng et al., CVPR 2021) and the boundary F-score BF (Csurka et al. 2013, DAVIS).
One ``cvx_seg_boundary`` call takes the predicted and the target label maps of a batch -- three launches, int64 counts added to device
tables -- and nothing waits on the host; ``BoundaryMetrics.get_results`` is the one host read and folds the counts in double.  The
reference has no counterpart; ``tests/seg_boundary_restatement.py`` is the specification.
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch

from . import _lib as L
from .seg_regions import SEG_MAP_DTYPE, _maps_of

MAX_WIDTH = 64                                       # CVX_SEG_BOUNDARY_MAX_WIDTH
MAX_WIDTHS = 8                                       # CVX_SEG_BOUNDARY_MAX_WIDTHS
VOID = 255
DEFAULT_WIDTHS = (1, 2, 4, 8)


class SegBoundary:
    """The bands of one measurement: either ``widths``, up to 8 distinct band widths in pixels (1 .. 64, Chebyshev), or ``ratio``, up to 8
    distinct fractions of the frame diagonal in (0, 1] -- the width of a frame is then ``clamp(floor(ratio * hypot(h, w) + 0.5), 1, 64)``,
    worked out per frame on the host (0.02 at 513 x 513 gives 15).  Exactly one of the two; ``keys`` are the widths or the ratios, the
    keys of the result dicts."""

    def __init__(self, widths=DEFAULT_WIDTHS, ratio=None):
        if ratio is not None:
            if widths is not None and widths is not DEFAULT_WIDTHS:
                raise ValueError("give exactly one of widths and ratio")
            try:
                values = [r for r in ratio]
            except TypeError:
                raise ValueError(f"ratio: a tuple of fractions of the frame diagonal, got {ratio!r}") from None
            for r in values:
                if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not math.isfinite(r) or not 0 < r <= 1:
                    raise ValueError(f"ratio: fractions in (0, 1], got {r!r}")
            self.ratio, self.widths = tuple(float(r) for r in values), None
            self.keys = self.ratio
        else:
            if widths is None:
                raise ValueError("give exactly one of widths and ratio")
            try:
                values = [d for d in widths]
            except TypeError:
                raise ValueError(f"widths: a tuple of band widths in pixels, got {widths!r}") from None
            for d in values:
                if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 1 <= int(d) <= MAX_WIDTH:
                    raise ValueError(f"widths: integers in [1, {MAX_WIDTH}], got {d!r}")
            self.widths, self.ratio = tuple(int(d) for d in values), None
            self.keys = self.widths
        if not 1 <= len(self.keys) <= MAX_WIDTHS:
            raise ValueError(f"between 1 and {MAX_WIDTHS} bands, got {len(self.keys)}")
        if len(set(self.keys)) != len(self.keys):
            raise ValueError(f"the bands are distinct (they key the results), got {self.keys!r}")
        self.K = len(self.keys)

    def frame_widths(self, h: int, w: int) -> List[int]:
        """the K band widths of an (h, w) frame"""
        if self.widths is not None:
            return list(self.widths)
        return [min(max(int(math.floor(r * math.hypot(h, w) + 0.5)), 1), MAX_WIDTH) for r in self.ratio]

    def __repr__(self):
        return f"SegBoundary(widths={self.widths})" if self.ratio is None else f"SegBoundary(ratio={self.ratio})"


def new_tables(num_classes: int, K: int, device):
    """``(flat, trimap (K, nc, nc), biou (K, nc, 3), bf (K, nc, 4))``: zeroed int64 tables, views of the one buffer ``flat`` so that a
    single copy reads all three"""
    nc = int(num_classes)
    sizes = [K * nc * nc, K * nc * 3, K * nc * 4]
    flat = torch.zeros(sum(sizes), dtype=torch.int64, device=device)
    a, b, c = torch.split(flat, sizes)
    return flat, a.view(K, nc, nc), b.view(K, nc, 3), c.view(K, nc, 4)


class BoundaryCounts:
    """What ``boundary_counts`` returns, all on the device: ``trimap`` (K, nc, nc) ``[k][target][prediction]``, ``biou`` (K, nc, 3) ``(I,
    Gb, Pb)``, ``bf`` (K, nc, 4) ``(mp, cp, mg, cg)``, int64; ``planes``: None, or per frame a (6, h, w) uint8 view -- D_G^edge,
    D_G^noedge, D_P^edge, D_P^noedge, N_{P->G} + 1, N_{G->P} + 1 (the last two 0 off the contour); ``widths`` the (frames, K) host list."""

    def __init__(self, trimap, biou, bf, planes, widths):
        self.trimap, self.biou, self.bf, self.planes, self.widths = trimap, biou, bf, planes, widths


def _frames_of(maps, what):
    """a list whose entries are (h, w) uint8 device maps or None (no frame here), or one (B, H, W) tensor -> (list, device)"""
    if torch.is_tensor(maps):
        if maps.dim() != 3:
            raise ValueError(f"{what}: a list of (h, w) maps or one (B, H, W) tensor, got {tuple(maps.shape)}")
        maps = list(maps.unbind(0))
    maps = list(maps)
    present = [t for t in maps if t is not None]
    if not present:
        raise ValueError(f"{what}: at least one map")
    for t in present:
        if torch.is_tensor(t) and not t.is_cuda:
            raise L.CvxError("seg_boundary.boundary_counts runs on an MI355X only: there is no CPU path")
    _maps_of(present, torch.uint8, what, None)
    return maps, present[0].device


def boundary_counts(pred, target, num_classes: int, spec: Optional[SegBoundary] = None, out=None, planes: bool = False) -> BoundaryCounts:
    """``cvx_seg_boundary``: the boundary counts of the predicted label maps ``pred`` against the target label maps ``target`` -- each a
    list of (h, w) uint8 device maps of any sizes (row views with a pitch are read in place; None: no frame here, the frame is skipped) or
    one (B, H, W) tensor -- under ``spec`` (a ``SegBoundary``, default ``SegBoundary()``).  Target values >= ``num_classes`` are void, and
    so is a prediction >= ``num_classes`` or under a void target.  ``out``: ``(trimap, biou, bf)`` int64 device tables to add onto (as
    ``new_tables`` lays them out), default fresh zeroed ones.  ``planes``: also return the six distance planes per frame.  All frames run
    together in three launches; no host read."""
    spec = SegBoundary() if spec is None else spec
    if not isinstance(spec, SegBoundary):
        raise ValueError(f"spec: a seg_boundary.SegBoundary, got {type(spec).__name__}")
    nc = int(num_classes)
    if isinstance(num_classes, bool) or nc != num_classes or not 1 <= nc <= 255:
        raise ValueError(f"num_classes lies in [1, 255] (255 is the void byte), got {num_classes!r}")
    preds, dev = _frames_of(pred, "pred")
    targets, tdev = _frames_of(target, "target")
    if tdev != dev:
        raise ValueError(f"pred and target live on one device, got {dev} and {tdev}")
    F, K = len(preds), spec.K
    if len(targets) != F:
        raise ValueError(f"one target per prediction, got {len(targets)} for {F}")
    if F > 65535:
        raise ValueError("at most 65535 frames per call")
    sizes = []
    for p, g in zip(preds, targets):
        if p is None or g is None:
            sizes.append((0, 0))
            continue
        if tuple(p.shape) != tuple(g.shape):
            raise ValueError(f"a prediction and its target have one size, got {tuple(p.shape)} and {tuple(g.shape)}")
        sizes.append((int(p.shape[0]), int(p.shape[1])))
    max_h, max_w = max(1, max(h for h, _ in sizes)), max(1, max(w for _, w in sizes))
    if max_h * max_w >= 2 ** 31:
        raise ValueError(f"the largest frame ({max_h} x {max_w}) has 2^31 pixels or more")
    widths = [spec.frame_widths(h, w) if h > 0 and w > 0 else [1] * K for h, w in sizes]
    if any(not 1 <= d <= MAX_WIDTH for row in widths for d in row):
        raise L.CvxError(f"seg_boundary.boundary_counts: a width outside 1 .. {MAX_WIDTH}")
    if out is None:
        _, trimap, biou, bf = new_tables(nc, K, dev)
    else:
        trimap, biou, bf = out
        for t, shape in ((trimap, (K, nc, nc)), (biou, (K, nc, 3)), (bf, (K, nc, 4))):
            if not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                raise ValueError(f"out: contiguous int64 tables (K, nc, nc), (K, nc, 3), (K, nc, 4) on {dev}")
    plane_store = torch.zeros(F, 6, max_h, max_w, dtype=torch.uint8, device=dev) if planes else None

    def table(tensors):
        return [(0, 0, 0) if t is None else (t.data_ptr(), t.stride(0), 0) for t in tensors]

    # the per-call tables: one pinned blob, one asynchronous copy -- frame_hw, widths, then the two 16-byte map tables
    hw_bytes = 8 * F + (-8 * F) % 16
    wd_bytes = 4 * F * K + (-4 * F * K) % 16
    head = hw_bytes + wd_bytes
    host = torch.zeros(head + 32 * F, dtype=torch.uint8, pin_memory=True)
    view = host.numpy()
    view[:8 * F].view("<i4")[:] = np.array(sizes, dtype="<i4").reshape(-1)
    view[hw_bytes:hw_bytes + 4 * F * K].view("<i4")[:] = np.array(widths, dtype="<i4").reshape(-1)
    skip = [p is None or g is None for p, g in zip(preds, targets)]
    for i, part in enumerate((preds, targets)):
        rows = table([None if s else t for s, t in zip(skip, part)])
        view[head + 16 * F * i:head + 16 * F * (i + 1)].view(SEG_MAP_DTYPE)[:] = np.array(rows, dtype=SEG_MAP_DTYPE)
    blob = torch.empty(host.numel(), dtype=torch.uint8, device=dev)
    blob.copy_(host, non_blocking=True)
    lib = L.load()
    need = int(lib.cvx_seg_boundary_workspace_bytes(F, max_h, max_w))
    if need <= 0:
        raise ValueError(f"the largest frame ({max_h} x {max_w}) has 2^31 pixels or more")
    ws = L.workspace("seg_boundary", dev, need)
    base = blob.data_ptr()

    def launch():
        with torch.cuda.device(dev):
            L.check(lib.cvx_seg_boundary(L.C.c_void_p(base + head), L.C.c_void_p(base + head + 16 * F), L.C.c_void_p(base), F, max_h, max_w, nc,
                                         L.C.c_void_p(base + hw_bytes), K, L.ptr(trimap), L.ptr(biou), L.ptr(bf), L.ptr(plane_store), L.ptr(ws),
                                         ws.numel(), L.stream_ptr(dev)), "cvx_seg_boundary")

    launch()
    views = [plane_store[f, :, :h, :w] for f, (h, w) in enumerate(sizes)] if planes else None
    got = BoundaryCounts(trimap, biou, bf, views, widths)
    got._host, got._blob, got._inputs = host, blob, (preds, targets)             # alive until the copy and the launches have run
    got._launch = launch                                                          # the entry alone, again (tools/seg_boundary_cost.py times it)
    return got


def fold_counts(trimap, biou, bf, keys):
    """The metrics from the three tables (tensors or arrays, any device), in double: ``"Trimap mIoU"``, ``"Boundary IoU"`` and ``"BF"`` as
    dicts keyed by ``keys``, and ``"Class Trimap IoU"``, ``"Class Boundary IoU"``, ``"Class BF"`` as dicts of per-class lists (NaN where a
    class does not enter the mean).  Per width the trimap matrix folds as ``SegmentationMetrics`` folds its own; Boundary IoU is the mean of
    ``I / (Gb + Pb - I)`` over the classes with ``Gb + Pb > 0``; BF the mean of ``2PR / (P + R)``, ``P = mp / cp``, ``R = mg / cg``, 0 when
    ``mp`` or ``mg`` is 0, over the classes with ``cp + cg > 0``.  A width without a single class gives NaN."""
    trimap, biou, bf = ((t.cpu() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))).double() for t in (trimap, biou, bf))
    nan = torch.tensor(float("nan"), dtype=torch.float64)
    out = {name: {} for name in ("Trimap mIoU", "Boundary IoU", "BF", "Class Trimap IoU", "Class Boundary IoU", "Class BF")}
    for k, key in enumerate(keys):
        hist = trimap[k]
        diag = torch.diag(hist)
        iu = diag / (hist.sum(1) + hist.sum(0) - diag)
        i, gb, pb = biou[k].unbind(1)
        b = torch.where(gb + pb > 0, i / (gb + pb - i), nan)
        mp, cp, mg, cg = bf[k].unbind(1)
        prec, rec = mp / cp, mg / cg
        f = torch.where((mp == 0) | (mg == 0), torch.zeros_like(mp), 2 * prec * rec / (prec + rec))
        f = torch.where(cp + cg > 0, f, nan)
        for name, per_class in (("Trimap mIoU", iu), ("Boundary IoU", b), ("BF", f)):
            out[name][key] = float(torch.nanmean(per_class))
            out["Class " + name.replace("mIoU", "IoU")][key] = per_class.tolist()
    return out


class BoundaryMetrics:
    """The boundary counts of a data set, kept on ``device``: ``trimap``, ``biou`` and ``bf`` are the int64 device tables that
    ``add_labels`` adds to (one ``cvx_seg_boundary`` call per batch, no host wait), ``reset()`` clears them, ``get_results()`` does the one
    host read and folds (``fold_counts``).  Everything is summed over the data set, not averaged per image."""

    def __init__(self, num_classes: int, spec: Optional[SegBoundary] = None, device="cuda"):
        spec = SegBoundary() if spec is None else spec
        if not isinstance(spec, SegBoundary):
            raise ValueError(f"spec: a seg_boundary.SegBoundary, got {type(spec).__name__}")
        if isinstance(num_classes, bool) or int(num_classes) != num_classes or not 1 <= int(num_classes) <= 255:
            raise ValueError(f"num_classes lies in [1, 255] (255 is the void byte), got {num_classes!r}")
        self.num_classes, self.spec, self.device = int(num_classes), spec, torch.device(device)
        if self.device.type != "cuda":
            raise L.CvxError("seg_boundary.BoundaryMetrics runs on an MI355X only: there is no CPU path")
        self._flat = self.trimap = self.biou = self.bf = None                   # created by the first add_labels: a device name touches no GPU

    def _tables(self):
        if self._flat is None:
            self._flat, self.trimap, self.biou, self.bf = new_tables(self.num_classes, self.spec.K, self.device)
        return self.trimap, self.biou, self.bf

    def reset(self):
        if self._flat is not None:
            self._flat.zero_()

    def _as_bytes(self, maps):
        """uint8 maps as they are; maps of another integer type (int64 targets) with every value outside [0, nc) turned into 255 first"""
        def one(t):
            if not torch.is_tensor(t) or t.dtype == torch.uint8:
                return t
            if not t.is_cuda:
                raise L.CvxError("seg_boundary.BoundaryMetrics.add_labels runs on an MI355X only: there is no CPU path")
            return torch.where((t >= 0) & (t < self.num_classes), t, VOID).to(torch.uint8)

        return one(maps) if torch.is_tensor(maps) else [one(t) for t in maps]

    def add_labels(self, pred, target, planes: bool = False) -> BoundaryCounts:
        """one batch: ``pred`` and ``target`` as ``boundary_counts`` takes them; maps of another integer type than uint8 (int64 targets) are
        accepted too, values outside ``[0, num_classes)`` become 255 first.  Asynchronous: nothing is read back."""
        for maps in (pred, target):
            if any(torch.is_tensor(t) and not t.is_cuda for t in ([maps] if torch.is_tensor(maps) else maps)):
                raise L.CvxError("seg_boundary.BoundaryMetrics.add_labels runs on an MI355X only: there is no CPU path")
        pred, target = self._as_bytes(pred), self._as_bytes(target)
        return boundary_counts(pred, target, self.num_classes, self.spec, out=self._tables(), planes=planes)

    def get_results(self):
        """the one host read; ``fold_counts`` of the tables (NaN everywhere before the first ``add_labels``)"""
        K, nc = self.spec.K, self.num_classes
        if self._flat is None:
            flat = torch.zeros(K * nc * (nc + 7), dtype=torch.int64)
        else:
            flat = self._flat.cpu()
        a, b, c = torch.split(flat, [K * nc * nc, K * nc * 3, K * nc * 4])
        return fold_counts(a.view(K, nc, nc), b.view(K, nc, 3), c.view(K, nc, 4), self.spec.keys)


def report_lines(results, keys) -> List[str]:
    """three lines per width for ``evaluate_on_voc``'s report: ``Trimap mIoU@d``, ``Boundary IoU@d``, ``BF@d``"""
    lines = []
    for key in keys:
        lines += [f"Trimap mIoU@{key}: {results['Trimap mIoU'][key]}", f"Boundary IoU@{key}: {results['Boundary IoU'][key]}",
                  f"BF@{key}: {results['BF'][key]}"]
    return lines
