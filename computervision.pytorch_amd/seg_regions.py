"""Connected-component regions of label maps on the device (``csrc/seg_regions.hip``): boxes from label maps.

DeepLabv3+ answers per pixel; this module turns its uint8 label maps (``segment_tiled``, ``predict_labels``) into *things*: the connected
regions of each class with their boxes, areas and scores, in the detectors' row format ``[x1, y1, x2, y2, score, cls]`` plus counts, so
``render.draw_detections``, ``render.draw_tracks``, ``track.Tracker``, ``render.read_detections``, ``DetectionEvaluator`` and
``CocoEvaluator`` work on segmentation results unchanged.  One ``cvx_seg_regions`` call labels every frame of a batch -- a lock-free
union-find over the pixels, a fixed number of launches -- and nothing waits on the host.  The reference has no counterpart;
``tests/seg_regions_restatement.py`` is the specification.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from . import _lib as L

REGION_CAP = 8192                                    # candidates per frame cvx_seg_regions sorts (render.MERGE_CAP)
SEG_MAP_DTYPE = np.dtype([("data", "<u8"), ("pitch", "<i4"), ("reserved", "<i4")])   # cvx_seg_map (render.SEG_MAP_DTYPE)


class SegRegions:
    """The parameters of one labelling.  ``connectivity``: 4 or 8 neighbours connect; ``min_area``: regions of fewer pixels are dropped
    (and, with ``fill``, painted over); ``classes``: ``"foreground"`` (every label but 0 and 255, the background and VOC's void), ``"all"``,
    or an iterable of labels 0 .. 255 -- pixels of other labels belong to no region; ``max_det``: rows per frame, the largest regions
    first; ``fill``: None, or the label 0 .. 255 that replaces the pixels of the regions below ``min_area`` in the clean maps."""

    def __init__(self, connectivity: int = 8, min_area: int = 64, classes="foreground", max_det: int = 300, fill: Optional[int] = None):
        if connectivity not in (4, 8) or isinstance(connectivity, bool):
            raise ValueError(f"connectivity: 4 or 8, got {connectivity!r}")
        if isinstance(min_area, bool) or int(min_area) != min_area or not 1 <= int(min_area) < 2 ** 31:
            raise ValueError(f"min_area: an integer >= 1, got {min_area!r}")
        if isinstance(max_det, bool) or int(max_det) != max_det or not 1 <= int(max_det) <= REGION_CAP:
            raise ValueError(f"max_det lies in [1, {REGION_CAP}], got {max_det!r}")
        if fill is not None and (isinstance(fill, bool) or int(fill) != fill or not 0 <= int(fill) <= 255):
            raise ValueError(f"fill: None or a label 0 .. 255, got {fill!r}")
        mask = np.zeros(256, bool)
        if isinstance(classes, str):
            if classes == "foreground":
                mask[1:255] = True
            elif classes == "all":
                mask[:] = True
            else:
                raise ValueError(f"classes: 'foreground', 'all' or an iterable of labels, got {classes!r}")
        else:
            try:
                chosen = [c for c in classes]
            except TypeError:
                raise ValueError(f"classes: 'foreground', 'all' or an iterable of labels, got {classes!r}") from None
            for c in chosen:
                if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) <= 255:
                    raise ValueError(f"classes: labels are integers 0 .. 255, got {c!r}")
                mask[int(c)] = True
            if not chosen:
                raise ValueError("classes: at least one label")
        self.connectivity, self.min_area, self.max_det = int(connectivity), int(min_area), int(max_det)
        self.fill = None if fill is None else int(fill)
        self.classes = classes if isinstance(classes, str) else tuple(int(c) for c in np.nonzero(mask)[0])
        self.mask = mask
        self.mask_words = np.packbits(mask, bitorder="little").view("<u4").copy()      # 8 uint32: bit (c & 31) of word c >> 5

    def __repr__(self):
        return (f"SegRegions(connectivity={self.connectivity}, min_area={self.min_area}, classes={self.classes!r}, max_det={self.max_det}, "
                f"fill={self.fill})")


class RegionBatch:
    """What ``label_regions`` returns, all on the device: ``rows`` (B, max_det, 6) fp32 ``[x1, y1, x2, y2, score, cls]`` (x2, y2 exclusive:
    ``max + 1``), zero past the count; ``counts`` (B) int32, -1 for a frame with more than 8192 candidates; ``total`` (B) int32, the regions
    with ``area >= min_area`` before the ``max_det`` cut; ``areas`` and ``seeds`` (B, max_det) int32 (pixels; ``y * w + x`` of the region's
    first pixel in raster order), -1 past the count; ``region_maps`` / ``clean_maps``: lists with one (h, w) int32 / uint8 map or None per
    frame, or None; ``overflow`` (1) int32, the number of flagged frames; with a tracker, ``ids`` (B, max_det) int32."""

    def __init__(self, rows, counts, total, areas, seeds, region_maps, clean_maps, overflow, ids=None):
        self.rows, self.counts, self.total, self.areas, self.seeds = rows, counts, total, areas, seeds
        self.region_maps, self.clean_maps, self.overflow, self.ids = region_maps, clean_maps, overflow, ids

    def read(self):
        """The single host read, through ``render.read_detections``: per frame ``(boxes (k, 4), scores (k), classes (k))`` -- and ``ids``
        (k) with a tracker; raises ``CvxError`` when a frame was flagged."""
        from . import render
        return render.read_detections(self.rows, self.counts, self.overflow, self.ids)


def _per_frame(flag, n, what) -> List[bool]:
    if isinstance(flag, (bool, np.bool_)):
        return [bool(flag)] * n
    flags = [bool(v) for v in flag]
    if len(flags) != n:
        raise ValueError(f"{what}: a bool or one per frame, got {len(flags)} for {n} frames")
    return flags


def _maps_of(maps, dtype, what, device):
    """a list of (h, w) device maps with unit pixel stride, or one (B, H, W) tensor -> the list of 2-d views"""
    if torch.is_tensor(maps):
        if maps.dim() != 3:
            raise ValueError(f"{what}: a list of (h, w) maps or one (B, H, W) tensor, got {tuple(maps.shape)}")
        maps = list(maps.unbind(0))
    maps = list(maps)
    if not maps:
        raise ValueError(f"{what}: at least one map")
    for t in maps:
        if not torch.is_tensor(t):
            raise ValueError(f"{what}: tensors, got {type(t).__name__}")
        if not t.is_cuda:
            raise L.CvxError("seg_regions.label_regions runs on an MI355X only: there is no CPU path")
    device = maps[0].device if device is None else device
    itemsize = torch.empty(0, dtype=dtype).element_size()
    for t in maps:
        if t.dtype != dtype or t.dim() != 2 or t.device != device:
            raise ValueError(f"{what}: (h, w) {dtype} maps on {device}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        if t.shape[0] > 0 and t.shape[1] > 0 and (t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
            raise ValueError(f"{what}: rows with unit pixel stride (a row-padded view is fine), got strides {t.stride()}")
        if t.data_ptr() % itemsize or (t.stride(0) * itemsize) >= 2 ** 31:
            raise ValueError(f"{what}: misaligned or over-long rows")
    return maps


def label_regions(labels, regions: Optional[SegRegions] = None, conf=None, region_maps=False, clean_maps=None) -> RegionBatch:
    """``cvx_seg_regions``: the connected regions of ``labels`` -- a list of (h, w) uint8 device maps of any sizes (row views with a pitch
    are read in place) or one (B, H, W) tensor -- under ``regions`` (a ``SegRegions``, default ``SegRegions()``).  ``conf``: the same
    shapes in fp32, a confidence per pixel; a region's score is then the mean of its pixels' confidences, quantised to 1 / 65535 and summed
    in integers (bit-identical from call to call), else 1.  After ``predict_labels(..., probs=True)`` the confidence of the winning class is
    ``conf=probs.gather(1, labels.long().unsqueeze(1))[:, 0]``.  ``region_maps``: a bool, or one per frame -- an (h, w) int32 map of row
    indices (-1: no row).  ``clean_maps``: a bool or one per frame, default every frame when ``regions.fill`` is set -- the labels with the
    regions below ``min_area`` replaced by ``fill``.  Returns a ``RegionBatch``; a frame with more than 8192 regions of ``min_area`` or more
    has count -1 and adds 1 to its overflow word.  All frames run together in a fixed number of launches; no host read."""
    regions = SegRegions() if regions is None else regions
    if not isinstance(regions, SegRegions):
        raise ValueError(f"regions: a seg_regions.SegRegions, got {type(regions).__name__}")
    maps = _maps_of(labels, torch.uint8, "labels", None)
    dev = maps[0].device
    F = len(maps)
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in maps]
    if any(h * w >= 2 ** 31 for h, w in sizes):
        raise ValueError("labels: a frame has fewer than 2^31 pixels")
    if F > 65535:
        raise ValueError("labels: at most 65535 frames per call")
    planes = None
    if conf is not None:
        planes = _maps_of(conf, torch.float32, "conf", dev)
        if [tuple(t.shape) for t in planes] != [tuple(t.shape) for t in maps]:
            raise ValueError("conf: one fp32 plane of the label map's size per frame")
    want_region = _per_frame(region_maps, F, "region_maps")
    want_clean = _per_frame(regions.fill is not None if clean_maps is None else clean_maps, F, "clean_maps")
    if any(want_clean) and regions.fill is None:
        raise ValueError("clean_maps need regions.fill")
    max_h, max_w = max(1, max(h for h, _ in sizes)), max(1, max(w for _, w in sizes))
    K = regions.max_det
    rows = torch.empty(F, K, 6, dtype=torch.float32, device=dev)
    counts = torch.empty(F, dtype=torch.int32, device=dev)
    total = torch.empty(F, dtype=torch.int32, device=dev)
    areas = torch.empty(F, K, dtype=torch.int32, device=dev)
    seeds = torch.empty(F, K, dtype=torch.int32, device=dev)
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    rmaps = [torch.empty(h, w, dtype=torch.int32, device=dev) if on else None for on, (h, w) in zip(want_region, sizes)] if any(want_region) else None
    cmaps = [torch.empty(h, w, dtype=torch.uint8, device=dev) if on else None for on, (h, w) in zip(want_clean, sizes)] if any(want_clean) else None

    def table(tensors):
        return [(0, 0, 0) if t is None else (t.data_ptr(), t.stride(0), 0) for t in tensors]   # torch strides are in elements

    # the per-call tables: one pinned blob, one asynchronous copy -- frame_hw first, then 16-byte entries
    parts = [table(p) for p in (maps, planes, rmaps, cmaps) if p is not None]
    head = 8 * F + (-8 * F) % 16
    host = torch.zeros(head + 16 * F * len(parts), dtype=torch.uint8, pin_memory=True)
    view = host.numpy()
    view[:8 * F].view("<i4")[:] = np.array(sizes, dtype="<i4").reshape(-1)
    for i, part in enumerate(parts):
        view[head + 16 * F * i:head + 16 * F * (i + 1)].view(SEG_MAP_DTYPE)[:] = np.array(part, dtype=SEG_MAP_DTYPE)
    blob = torch.empty(host.numel(), dtype=torch.uint8, device=dev)
    blob.copy_(host, non_blocking=True)
    at = iter(range(1, len(parts)))
    address = [blob.data_ptr() + head] + [blob.data_ptr() + head + 16 * F * next(at) if p is not None else None for p in (planes, rmaps, cmaps)]
    lib = L.load()
    need = int(lib.cvx_seg_regions_workspace_bytes(F, max_h, max_w))
    if need <= 0:
        raise ValueError(f"labels: the largest frame ({max_h} x {max_w}) has 2^31 pixels or more")
    ws = L.workspace("seg_regions", dev, need)
    words = (L.C.c_uint32 * 8)(*[int(v) for v in regions.mask_words])

    def launch():
        with torch.cuda.device(dev):
            L.check(lib.cvx_seg_regions(L.C.c_void_p(address[0]), L.C.c_void_p(blob.data_ptr()), F, max_h, max_w, L.C.cast(words, L.C.c_void_p),
                                        regions.connectivity, regions.min_area, K, 0 if regions.fill is None else regions.fill,
                                        L.C.c_void_p(address[1]), L.C.c_void_p(address[2]), L.C.c_void_p(address[3]), L.ptr(rows), L.ptr(counts),
                                        L.ptr(total), L.ptr(areas), L.ptr(seeds), L.ptr(overflow), L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
                    "cvx_seg_regions")

    launch()
    batch = RegionBatch(rows, counts, total, areas, seeds, rmaps, cmaps, overflow)
    batch._host, batch._blob, batch._inputs = host, blob, (maps, planes)          # alive until the copy and the launches have run
    batch._launch = launch                                                        # the entry alone, again (tools/seg_regions_cost.py times it)
    return batch
