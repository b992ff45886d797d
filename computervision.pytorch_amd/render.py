"""Batched prediction on the device, input and output side: a list of uint8 HWC frames of any sizes becomes the network batch in one launch
(``cvx_letterbox_batch_u8_to_nchw``, or ``cvx_aug_images_plain`` jobs for the bicubic stretch), the NMS rows become image coordinates
without a read-back (``cvx_det_to_image``), and the result is painted into the frames in place (``cvx_draw_detections``,
``cvx_seg_overlay``; csrc/render.hip).  ``FrameBatch`` puts every job table of a batch into ONE pinned blob and one asynchronous copy, so
none of this waits on the host.  There is no CPU path: frames that are not in GPU memory raise ``CvxError``.

Tiled prediction for frames much larger than the network input (csrc/tiles.hip): ``tile_grid`` is the host geometry,
``TileBatch`` the ``FrameBatch`` idea for tiles (``cvx_tiles_u8_to_nchw`` crops every tile of every frame into the batch in one launch), and
``merge_tiles`` suppresses the duplicates across tile borders (``cvx_det_merge_tiles``, one workgroup per frame).  For segmentation the tiles'
logits are stitched instead (csrc/seg_tiles.hip): ``stitch_segmentation`` blends the up-sampled logits of every tile
that covers a pixel and writes the label, the overlay and the confusion counts in one ``cvx_seg_stitch`` launch.

``draw_tracks`` paints rows that carry track ids (``track.py``; ``cvx_draw_tracks``, one kernel body with
``cvx_draw_detections``).

``palette``, ``format_label`` and ``FONT`` are the host statement of the drawing rules, shared with the tests'
restatement (tests/render_restatement.py)."""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .augment import JOB_DTYPE as AUG_JOB_DTYPE

LETTERBOX_JOB_DTYPE = np.dtype([("src", "<u8"), ("h", "<i4"), ("w", "<i4"), ("out", "<i4"), ("reserved", "<i4")])
FRAME_JOB_DTYPE = np.dtype([("data", "<u8"), ("h", "<i4"), ("w", "<i4"), ("stride", "<i4"), ("reserved", "<i4")])
assert LETTERBOX_JOB_DTYPE.itemsize == 24 and FRAME_JOB_DTYPE.itemsize == 24      # struct cvx_letterbox_job / cvx_frame_job, include/cvx_engine.h

GLYPHS = "0123456789:.%"
# the project's 5 x 7 font: one byte per glyph row, bit 4 is the left column (csrc/render.hip holds the same table)
FONT = {
    "0": (0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E), "1": (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E), "2": (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F),
    "3": (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E), "4": (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02), "5": (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),
    "6": (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E), "7": (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08), "8": (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E),
    "9": (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C), ":": (0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x0C, 0x00), ".": (0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C),
    "%": (0x18, 0x19, 0x02, 0x04, 0x08, 0x13, 0x03),
}
MAX_CLASS, MAX_TENTHS = 9999, 9999      # what a label spells; larger values are clamped


def palette(n: int = 256) -> np.ndarray:
    """(n, 3) uint8 RGB: the bit-spread PASCAL VOC palette of ``segmentation_2d.voc_colormap``.  Entry 0 is black, so class ``c`` of a
    detector is drawn with entry ``c + 1``."""
    from core.algorithms.segmentation_2d import voc_colormap
    return np.asarray(voc_colormap(int(n)), dtype=np.uint8).reshape(int(n), 3)


def format_label(cls, score) -> str:
    """``"{cls}:{p}%"``: the class index and ``'{:.1f}'.format`` of the float32 product ``score * 100`` -- round-half-even on the exact
    value, i.e. ``tenths = rint(double(score * 100.0f) * 10.0)`` (the product by 10 is exact in fp64), which is what the kernel computes."""
    cls = min(max(int(cls), 0), MAX_CLASS)
    t = np.rint(np.float64(np.float32(score) * np.float32(100.0)) * 10.0)
    tenths = int(min(max(t, 0.0), float(MAX_TENTHS))) if t == t else 0
    return f"{cls}:{tenths // 10}.{tenths % 10}%"


def _align(n, a=16):
    return (n + a - 1) // a * a


def _check_frames(frames) -> torch.device:
    if len(frames) == 0 or not all(torch.is_tensor(t) and t.is_cuda for t in frames):
        raise L.CvxError("batched prediction takes uint8 HWC frames in GPU memory (there is no CPU path)")
    dev = frames[0].device
    for t in frames:
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] <= 0 or t.shape[1] <= 0 or t.device != dev:
            raise L.CvxError(f"frame {tuple(t.shape)} {t.dtype} on {t.device}: expected (h, w, 3) uint8 on {dev}")
        if t.stride(2) != 1 or t.stride(1) != 3 or t.stride(0) < 3 * t.shape[1]:
            raise L.CvxError(f"frame strides {t.stride()}: pixels are 3 adjacent bytes and rows do not overlap")
    return dev


class FrameBatch:
    """The job tables of one batch of frames in device memory, from one pinned blob and one asynchronous copy: ``frame_jobs`` (the frames
    themselves, with their row strides, for the two painters), ``input_jobs`` (the pictures for the input side: ``cvx_letterbox_job`` rows,
    or ``cvx_aug_job`` rows + ``job_start`` that stretch each picture to ``input_hw``), ``image_hw`` (B, 2) int32 and, for ``letterbox`` not
    None, ``box_map`` (B, 4) float32 (``det_eval.letterbox_box_map``, worked out on the host from the sizes)."""

    def __init__(self, frames: Sequence[torch.Tensor], input_hw=None, letterbox: Optional[bool] = None):
        self.device = _check_frames(frames)
        self.frames = list(frames)
        B = self.n = len(frames)
        self.max_h, self.max_w = max(int(t.shape[0]) for t in frames), max(int(t.shape[1]) for t in frames)
        self.letterbox = letterbox
        # the input side reads tightly packed pictures; a frame with padded rows is copied on the device (no host wait)
        self.sources = [t if t.is_contiguous() else t.contiguous() for t in frames] if input_hw is not None else []
        sizes = [(int(t.shape[0]), int(t.shape[1])) for t in frames]
        o_frame = 0
        o_hw = _align(o_frame + 24 * B)
        o_map = _align(o_hw + 8 * B)
        o_in = _align(o_map + 16 * B)
        o_js = _align(o_in + (24 if letterbox else 64) * B)
        total = _align(o_js + 4 * (B + 1))
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        hv[:] = 0
        hv[o_frame:o_frame + 24 * B].view(FRAME_JOB_DTYPE)[:] = np.array([(t.data_ptr(), h, w, t.stride(0), 0) for t, (h, w) in zip(frames, sizes)],
                                                                           dtype=FRAME_JOB_DTYPE)
        hv[o_hw:o_hw + 8 * B].view(np.int32).reshape(B, 2)[:] = sizes
        if input_hw is not None:
            H, W = int(input_hw[0]), int(input_hw[1])
            self.input_hw = (H, W)
            from . import det_eval
            bm = det_eval.letterbox_box_map(torch.tensor(sizes, dtype=torch.int64), (H, W), bool(letterbox))
            hv[o_map:o_map + 16 * B].view(np.float32).reshape(B, 4)[:] = bm.numpy()
            if letterbox:
                from .engine import letterbox_geometry
                for h, w in sizes:
                    letterbox_geometry(h, w, H, W)            # raises CvxError where a picture collapses to nothing, as the per-image entry does
                hv[o_in:o_in + 24 * B].view(LETTERBOX_JOB_DTYPE)[:] = np.array(
                    [(s.data_ptr(), h, w, i, 0) for i, (s, (h, w)) in enumerate(zip(self.sources, sizes))], dtype=LETTERBOX_JOB_DTYPE)
            else:                                             # DeviceAugmenter's validation job with the picture stretched over the whole canvas
                hv[o_in:o_in + 64 * B].view(AUG_JOB_DTYPE)[:] = np.array(
                    [(s.data_ptr(), h, w, H, W, 0, 0, 0, i, 0, 0, W, H, -1, 0) for i, (s, (h, w)) in enumerate(zip(self.sources, sizes))],
                    dtype=AUG_JOB_DTYPE)
                hv[o_js:o_js + 4 * (B + 1)].view(np.int32)[:] = np.arange(B + 1)
        self.blob = torch.empty(total, dtype=torch.uint8, device=self.device)
        self.blob.copy_(host, non_blocking=True)
        self._host = host                                     # alive until the copy has run
        base = self.blob.data_ptr()
        self.frame_jobs, self.input_jobs, self.job_start = L.C.c_void_p(base + o_frame), L.C.c_void_p(base + o_in), L.C.c_void_p(base + o_js)
        self.image_hw = self.blob[o_hw:o_hw + 8 * B].view(torch.int32).view(B, 2)
        self.box_map = self.blob[o_map:o_map + 16 * B].view(torch.float32).view(B, 4) if input_hw is not None else None

    def network_input(self, swap_rb: bool = False) -> torch.Tensor:
        """The (B, 3, H, W) fp32 batch in [0, 1], one launch: the reference's letter_box + to_tensor per picture when ``letterbox``, else the
        bicubic stretch to the network size (the host ``cv2.resize(..., INTER_CUBIC)`` of ``read_image_and_convert_to_tensor``)."""
        H, W = self.input_hw
        out = torch.empty(self.n, 3, H, W, dtype=torch.float32, device=self.device)
        lib = L.load()
        with torch.cuda.device(self.device):
            stream = L.stream_ptr(self.device)
            if self.letterbox:
                L.check(lib.cvx_letterbox_batch_u8_to_nchw(self.input_jobs, self.n, 1, int(bool(swap_rb)), L.ptr(out), H, W, stream),
                        "cvx_letterbox_batch_u8_to_nchw")
            else:
                if swap_rb:
                    raise L.CvxError("the bicubic stretch keeps the channel order: pass RGB frames")
                L.check(lib.cvx_aug_images_plain(self.input_jobs, self.job_start, self.n, L.ptr(out), H, W, stream), "cvx_aug_images_plain")
        return out


def letterbox_batch(frames: Sequence[torch.Tensor], input_hw, letterbox: bool = True, swap_rb: bool = False) -> torch.Tensor:
    """``cvx_letterbox_batch_u8_to_nchw``: frames of any sizes -> (B, 3, H, W) fp32, slot i bit-identical to ``engine.letterbox_u8`` of frame
    i.  ``letterbox=False`` is that entry's plain nearest resize."""
    H, W = int(input_hw[0]), int(input_hw[1])
    fb = _letterbox_table(frames)
    if letterbox:
        from .engine import letterbox_geometry
        for t in frames:
            letterbox_geometry(int(t.shape[0]), int(t.shape[1]), H, W)      # raises CvxError where a picture collapses, as the per-image entry does
    out = torch.empty(fb.n, 3, H, W, dtype=torch.float32, device=fb.device)
    with torch.cuda.device(fb.device):
        L.check(L.load().cvx_letterbox_batch_u8_to_nchw(fb.input_jobs, fb.n, 1 if letterbox else 0, int(bool(swap_rb)), L.ptr(out), H, W,
                                                        L.stream_ptr(fb.device)), "cvx_letterbox_batch_u8_to_nchw")
    return out


def _letterbox_table(frames):
    """A bare FrameBatch that holds only the ``cvx_letterbox_job`` rows of ``frames`` (slot i for frame i)"""
    fb = FrameBatch.__new__(FrameBatch)
    fb.device = _check_frames(frames)
    fb.n = len(frames)
    fb.sources = [t.contiguous() for t in frames]
    table = np.array([(s.data_ptr(), int(s.shape[0]), int(s.shape[1]), i, 0) for i, s in enumerate(fb.sources)], dtype=LETTERBOX_JOB_DTYPE)
    host = torch.empty(24 * fb.n, dtype=torch.uint8, pin_memory=True)
    host.numpy()[:] = table.view(np.uint8)
    fb.blob = torch.empty(24 * fb.n, dtype=torch.uint8, device=fb.device)
    fb.blob.copy_(host, non_blocking=True)
    fb._host = host
    fb.input_jobs = L.C.c_void_p(fb.blob.data_ptr())
    return fb


def det_to_image(rows: torch.Tensor, counts: torch.Tensor, box_map: Optional[torch.Tensor] = None, overflow: Optional[torch.Tensor] = None):
    """``cvx_det_to_image``: rows (B, K, 6) fp32 and counts (B) int32 as the NMS leaves them, ``box_map`` (B, 4) fp32 or None (boxes already
    final) -> (rows in image coordinates with the rows past each count zero, counts with -1 / too large replaced by 0, the overflow word
    (1) int32 -- ``overflow`` is added to when given).  No host read."""
    if not (torch.is_tensor(rows) and rows.is_cuda):
        raise L.CvxError("det_to_image runs on an MI355X only: there is no CPU path")
    if rows.dim() != 3 or rows.shape[2] != 6 or rows.dtype != torch.float32 or rows.shape[1] <= 0:
        raise ValueError(f"rows: (B, K, 6) float32, got {tuple(rows.shape)} {rows.dtype}")
    B, K = int(rows.shape[0]), int(rows.shape[1])
    if counts.dtype != torch.int32 or counts.numel() != B or counts.device != rows.device:
        raise ValueError("counts: (B) int32 on the rows' device")
    if box_map is not None and (box_map.dtype != torch.float32 or tuple(box_map.shape) != (B, 4) or box_map.device != rows.device):
        raise ValueError("box_map: (B, 4) float32 [px, py, gx, gy] on the rows' device")
    rows, counts = rows.contiguous(), counts.contiguous()
    box_map = None if box_map is None else box_map.contiguous()
    out_rows, out_counts = torch.empty_like(rows), torch.empty_like(counts)
    if overflow is None:
        overflow = torch.zeros(1, dtype=torch.int32, device=rows.device)
    with torch.cuda.device(rows.device):
        L.check(L.load().cvx_det_to_image(L.ptr(rows), L.ptr(counts), B, K, 0 if box_map is None else 1, L.ptr(box_map), L.ptr(out_rows),
                                          L.ptr(out_counts), L.ptr(overflow), L.stream_ptr(rows.device)), "cvx_det_to_image")
    return out_rows, out_counts, overflow


# ---- tiled prediction for large frames (csrc/tiles.hip) --------------------------------------------------------------
TILE_JOB_DTYPE = np.dtype([("src", "<u8"), ("h", "<i4"), ("w", "<i4"), ("stride", "<i4"), ("y0", "<i4"), ("x0", "<i4"), ("th", "<i4"), ("tw", "<i4"),
                           ("out", "<i4")])
assert TILE_JOB_DTYPE.itemsize == 40                 # struct cvx_tile_job, include/cvx_engine.h
SEG_TILE_FRAME_DTYPE = np.dtype([("first_slot", "<i4"), ("ny", "<i4"), ("nx", "<i4"), ("y_off", "<i4"), ("x_off", "<i4"), ("reserved", "<i4")])
SEG_MAP_DTYPE = np.dtype([("data", "<u8"), ("pitch", "<i4"), ("reserved", "<i4")])
assert SEG_TILE_FRAME_DTYPE.itemsize == 24 and SEG_MAP_DTYPE.itemsize == 16      # struct cvx_seg_tile_frame / cvx_seg_map, include/cvx_engine.h
MERGE_CAP = 8192                                     # candidates per frame cvx_det_merge_tiles sorts
MERGE_METRICS = {"iou": 0, "ios": 1}


def _axis_tiles(n, T, stride):
    if n <= T:
        return [(0, n)]
    starts, s = [], 0
    while s + T < n:
        starts.append(s)
        s += stride
    if not starts or starts[-1] != n - T:
        starts.append(n - T)                         # the last tile is shifted back inside the frame, never padded
    return [(s, T) for s in starts]


def tile_grid(h, w, tile_hw, overlap):
    """The tiles of an (h, w) frame at tile size ``tile_hw = (TH, TW)``, row-major, as ``(y0, x0, th, tw)``.  Per axis the stride is
    ``T - int(T * overlap)``; an axis no longer than the tile has one tile of its own extent at 0, a longer one has tiles at 0, stride,
    2 * stride, ... while ``start + T < n`` and a last one at ``n - T``.  Every tile lies inside the frame and their union covers it."""
    h, w, TH, TW = int(h), int(w), int(tile_hw[0]), int(tile_hw[1])
    if h <= 0 or w <= 0 or TH <= 0 or TW <= 0:
        raise ValueError("tile_grid: sizes are positive")
    if not 0 <= overlap < 1:
        raise ValueError(f"tile_grid: overlap {overlap} outside [0, 1)")
    sy, sx = TH - int(TH * overlap), TW - int(TW * overlap)
    if sy < 1 or sx < 1:
        raise ValueError(f"tile_grid: overlap {overlap} leaves no stride at tile size {(TH, TW)}")
    return [(y0, x0, th, tw) for y0, th in _axis_tiles(h, TH, sy) for x0, tw in _axis_tiles(w, TW, sx)]


class TileBatch:
    """``FrameBatch`` for tiles: every table of one batch of large frames in device memory, from one pinned blob and one asynchronous copy.
    Frame f contributes the slots of ``tile_grid(h, w, input_hw, tile_overlap)`` and, with ``full_frame``, one more slot after them that
    holds the whole picture at network size (letterboxed, or stretched when ``letterbox`` is false -- the input ``predict_batch`` builds).
    ``tile_jobs`` (``cvx_tile_job`` rows, slot order), ``slot_map`` (slots, 4) int32 [frame, x0, y0, 0], ``frame_hw`` (n, 2) int32,
    ``image_hw`` (slots, 2) int32 -- ``input_hw`` for a tile slot, so the class's own box map is the identity there, and the frame's size
    for a full-frame slot -- and ``frame_jobs`` for the painters.  ``tiles[f]`` is the frame's grid, ``slot_frame`` the frame of each slot.
    ``seg_frames`` (``cvx_seg_tile_frame`` rows) and ``seg_axes`` (``n_axes`` int32: the per-axis tile starts and extents) are the grid as
    ``cvx_seg_stitch`` reads it; they lie at the blob's end."""

    def __init__(self, frames: Sequence[torch.Tensor], input_hw, tile_overlap: float = 0.2, full_frame: bool = True, letterbox: bool = True):
        self.device = _check_frames(frames)
        self.frames = list(frames)
        F = self.n = len(frames)
        H, W = int(input_hw[0]), int(input_hw[1])
        self.input_hw, self.letterbox, self.full_frame = (H, W), bool(letterbox), bool(full_frame)
        sizes = [(int(t.shape[0]), int(t.shape[1])) for t in frames]
        self.max_h, self.max_w = max(h for h, _ in sizes), max(w for _, w in sizes)
        self.tiles = [tile_grid(h, w, (H, W), tile_overlap) for h, w in sizes]
        tile_jobs, slot_map, image_hw, self.slot_frame, full_slots = [], [], [], [], []
        for f, (t, (h, w)) in enumerate(zip(frames, sizes)):
            for y0, x0, th, tw in self.tiles[f]:
                tile_jobs.append((t.data_ptr(), h, w, t.stride(0), y0, x0, th, tw, len(slot_map)))
                slot_map.append((f, x0, y0, 0))
                image_hw.append((H, W))
            if full_frame:
                full_slots.append(len(slot_map))
                slot_map.append((f, 0, 0, 0))
                image_hw.append((h, w))
            self.slot_frame += [f] * (len(slot_map) - len(self.slot_frame))
        T, S = self.n_tiles, self.slots = len(tile_jobs), len(slot_map)
        # the whole-picture path reads tightly packed pictures; a frame with padded rows is copied on the device (no host wait)
        self.sources = [t if t.is_contiguous() else t.contiguous() for t in frames] if full_frame else []
        o_frame = 0
        o_fhw = _align(o_frame + 24 * F)
        o_tile = _align(o_fhw + 8 * F)
        o_map = _align(o_tile + 40 * T)
        o_hw = _align(o_map + 16 * S)
        o_in = _align(o_hw + 8 * S)
        o_js = _align(o_in + (24 if letterbox else 64) * F)
        o_full = _align(o_js + 4 * (F + 1))
        # the stitch's view of the grid (cvx_seg_tile_frame): a frame's tiles are the product of its y tiles and its x tiles
        seg_frames, axes, first = [], [], 0
        for f, grid in enumerate(self.tiles):
            ys, xs = sorted({(y0, th) for y0, _, th, _ in grid}), sorted({(x0, tw) for _, x0, _, tw in grid})
            assert [(y0, x0, th, tw) for y0, th in ys for x0, tw in xs] == grid
            seg_frames.append((first, len(ys), len(xs), len(axes), len(axes) + 2 * len(ys), 0))
            axes += [v for pair in ys + xs for v in pair]
            first += len(grid) + (1 if full_frame else 0)
        A = self.n_axes = len(axes)
        o_seg = _align(o_full + 8 * F)
        o_axes = _align(o_seg + 24 * F)
        total = _align(o_axes + 4 * A)
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        hv[:] = 0
        hv[o_frame:o_frame + 24 * F].view(FRAME_JOB_DTYPE)[:] = np.array([(t.data_ptr(), h, w, t.stride(0), 0) for t, (h, w) in zip(frames, sizes)],
                                                                           dtype=FRAME_JOB_DTYPE)
        hv[o_fhw:o_fhw + 8 * F].view(np.int32).reshape(F, 2)[:] = sizes
        hv[o_tile:o_tile + 40 * T].view(TILE_JOB_DTYPE)[:] = np.array(tile_jobs, dtype=TILE_JOB_DTYPE)
        hv[o_map:o_map + 16 * S].view(np.int32).reshape(S, 4)[:] = slot_map
        hv[o_hw:o_hw + 8 * S].view(np.int32).reshape(S, 2)[:] = image_hw
        if full_frame:
            if letterbox:
                from .engine import letterbox_geometry
                for h, w in sizes:
                    letterbox_geometry(h, w, H, W)            # raises CvxError where a picture collapses to nothing, as the per-image entry does
                hv[o_in:o_in + 24 * F].view(LETTERBOX_JOB_DTYPE)[:] = np.array(
                    [(s.data_ptr(), h, w, slot, 0) for slot, s, (h, w) in zip(full_slots, self.sources, sizes)], dtype=LETTERBOX_JOB_DTYPE)
            else:                                             # FrameBatch's stretch jobs: they fill a batch of their own, moved to the slots after
                hv[o_in:o_in + 64 * F].view(AUG_JOB_DTYPE)[:] = np.array(
                    [(s.data_ptr(), h, w, H, W, 0, 0, 0, i, 0, 0, W, H, -1, 0) for i, (s, (h, w)) in enumerate(zip(self.sources, sizes))],
                    dtype=AUG_JOB_DTYPE)
                hv[o_js:o_js + 4 * (F + 1)].view(np.int32)[:] = np.arange(F + 1)
            hv[o_full:o_full + 8 * F].view(np.int64)[:] = full_slots
        hv[o_seg:o_seg + 24 * F].view(SEG_TILE_FRAME_DTYPE)[:] = np.array(seg_frames, dtype=SEG_TILE_FRAME_DTYPE)
        hv[o_axes:o_axes + 4 * A].view(np.int32)[:] = axes
        self.blob = torch.empty(total, dtype=torch.uint8, device=self.device)
        self.blob.copy_(host, non_blocking=True)
        self._host = host                                     # alive until the copy has run
        base = self.blob.data_ptr()
        P = L.C.c_void_p
        self.frame_jobs, self.tile_jobs, self.input_jobs, self.job_start = P(base + o_frame), P(base + o_tile), P(base + o_in), P(base + o_js)
        self.frame_hw = self.blob[o_fhw:o_fhw + 8 * F].view(torch.int32).view(F, 2)
        self.slot_map = self.blob[o_map:o_map + 16 * S].view(torch.int32).view(S, 4)
        self.image_hw = self.blob[o_hw:o_hw + 8 * S].view(torch.int32).view(S, 2)
        self.full_slots = self.blob[o_full:o_full + 8 * F].view(torch.int64) if full_frame else None
        self.seg_frames, self.seg_axes = P(base + o_seg), P(base + o_axes)

    def network_input(self, swap_rb: bool = False) -> torch.Tensor:
        """The (slots, 3, H, W) fp32 batch in [0, 1]: one ``cvx_tiles_u8_to_nchw`` launch for every tile of every frame and, with
        ``full_frame``, the whole-picture launch of ``FrameBatch.network_input`` for the frames' own slots."""
        H, W = self.input_hw
        out = torch.empty(self.slots, 3, H, W, dtype=torch.float32, device=self.device)
        lib = L.load()
        with torch.cuda.device(self.device):
            stream = L.stream_ptr(self.device)
            L.check(lib.cvx_tiles_u8_to_nchw(self.tile_jobs, self.n_tiles, int(bool(swap_rb)), L.ptr(out), H, W, stream), "cvx_tiles_u8_to_nchw")
            if self.full_frame and self.letterbox:
                L.check(lib.cvx_letterbox_batch_u8_to_nchw(self.input_jobs, self.n, 1, int(bool(swap_rb)), L.ptr(out), H, W, stream),
                        "cvx_letterbox_batch_u8_to_nchw")
            elif self.full_frame:
                if swap_rb:
                    raise L.CvxError("the bicubic stretch keeps the channel order: pass RGB frames")
                whole = torch.empty(self.n, 3, H, W, dtype=torch.float32, device=self.device)
                L.check(lib.cvx_aug_images_plain(self.input_jobs, self.job_start, self.n, L.ptr(whole), H, W, stream), "cvx_aug_images_plain")
                out.index_copy_(0, self.full_slots, whole)
        return out


def merge_tiles(rows: torch.Tensor, counts: torch.Tensor, slot_map: torch.Tensor, frame_hw: torch.Tensor, metric: str = "ios",
                threshold: float = 0.5, class_agnostic: bool = False, max_det: int = 300, overflow: Optional[torch.Tensor] = None):
    """``cvx_det_merge_tiles``: rows (slots, K, 6) fp32 and counts (slots) int32 as ``det_to_image`` leaves them, boxes in each slot's own
    pixels; ``slot_map`` (slots, 4) int32 [frame, x0, y0, 0] and ``frame_hw`` (frames, 2) int32 on the same device.  Per frame the rows of
    its slots are moved to frame coordinates, clamped to the frame, ordered by (score, ordinal) and suppressed greedily: a candidate goes
    when an earlier kept one (of its class, unless ``class_agnostic``) overlaps it by more than ``threshold`` in ``metric`` -- ``"iou"`` or
    ``"ios"``, intersection over the smaller box, which removes the part-boxes tile borders cut.  Returns (rows (frames, max_det, 6), counts
    (frames) int32, source (frames, max_det) int32 -- slot * K + row of each kept row, -1 past the count --, the overflow word (1) int32,
    added to when given).  A frame with more than ``MERGE_CAP`` candidates has count -1 and adds 1 to the overflow word.  No host read."""
    if not (torch.is_tensor(rows) and rows.is_cuda):
        raise L.CvxError("merge_tiles runs on an MI355X only: there is no CPU path")
    if rows.dim() != 3 or rows.shape[2] != 6 or rows.dtype != torch.float32 or rows.shape[0] <= 0 or rows.shape[1] <= 0:
        raise ValueError(f"rows: (slots, K, 6) float32, got {tuple(rows.shape)} {rows.dtype}")
    S, K = int(rows.shape[0]), int(rows.shape[1])
    if S * K >= 2 ** 31:
        raise ValueError("rows: slots * K must stay below 2^31 (the ordinal is 32 bits)")
    if counts.dtype != torch.int32 or counts.numel() != S or counts.device != rows.device:
        raise ValueError("counts: (slots) int32 on the rows' device")
    if slot_map.dtype != torch.int32 or tuple(slot_map.shape) != (S, 4) or slot_map.device != rows.device:
        raise ValueError("slot_map: (slots, 4) int32 [frame, x0, y0, 0] on the rows' device")
    if frame_hw.dtype != torch.int32 or frame_hw.dim() != 2 or frame_hw.shape[1] != 2 or frame_hw.shape[0] <= 0 or frame_hw.device != rows.device:
        raise ValueError("frame_hw: (frames, 2) int32 on the rows' device")
    if metric not in MERGE_METRICS:
        raise ValueError(f"metric: one of {sorted(MERGE_METRICS)}, got {metric!r}")
    if not 0.0 <= float(threshold) <= 1.0:
        raise ValueError("threshold lies in [0, 1]")
    if not 1 <= int(max_det) <= MERGE_CAP:
        raise ValueError(f"max_det lies in [1, {MERGE_CAP}]")
    F = int(frame_hw.shape[0])
    rows, counts, slot_map, frame_hw = rows.contiguous(), counts.contiguous(), slot_map.contiguous(), frame_hw.contiguous()
    out_rows = torch.empty(F, int(max_det), 6, dtype=torch.float32, device=rows.device)
    out_counts = torch.empty(F, dtype=torch.int32, device=rows.device)
    out_source = torch.empty(F, int(max_det), dtype=torch.int32, device=rows.device)
    if overflow is None:
        overflow = torch.zeros(1, dtype=torch.int32, device=rows.device)
    lib = L.load()
    ws = L.workspace("det_merge_tiles", rows.device, int(lib.cvx_det_merge_workspace_bytes(F)))
    with torch.cuda.device(rows.device):
        L.check(lib.cvx_det_merge_tiles(L.ptr(rows), L.ptr(counts), S, K, L.ptr(slot_map), L.ptr(frame_hw), F, MERGE_METRICS[metric], float(threshold),
                                        int(bool(class_agnostic)), int(max_det), L.ptr(out_rows), L.ptr(out_counts), L.ptr(out_source),
                                        L.ptr(overflow), L.ptr(ws), ws.numel(), L.stream_ptr(rows.device)), "cvx_det_merge_tiles")
    return out_rows, out_counts, out_source, overflow


_lut_cache = {}


def _device_lut(n, device, lut=None):
    if lut is not None:
        t = torch.as_tensor(lut)
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != 3 or not t.is_cuda:
            raise ValueError("lut: (n, 3) uint8 on the device")
        return t.contiguous()
    key = (int(n), torch.device(device))
    if key not in _lut_cache:
        host = torch.from_numpy(palette(n)).pin_memory()
        _lut_cache[key] = (host.to(device, non_blocking=True), host)
    return _lut_cache[key][0]


def draw_detections(frames, rows: torch.Tensor, counts: torch.Tensor, lut=None, thickness: int = 2, font_scale: int = 2, batch: FrameBatch = None):
    """``cvx_draw_detections``: paints rows[b, :counts[b]] (image coordinates) into frames[b], in place.  ``lut``: (n, 3) uint8 device
    colours in the frames' channel order, default ``palette(256)``.  ``batch``: the frames' ``FrameBatch`` when the caller has one."""
    fb = batch if batch is not None else FrameBatch(frames)
    if rows.dim() != 3 or rows.shape[0] != fb.n or rows.shape[2] != 6 or rows.dtype != torch.float32 or rows.device != fb.device:
        raise ValueError(f"rows: ({fb.n}, K, 6) float32 on {fb.device}")
    if counts.dtype != torch.int32 or counts.numel() != fb.n or counts.device != fb.device:
        raise ValueError("counts: (B) int32 on the frames' device")
    rows, counts = rows.contiguous(), counts.contiguous()
    lut = _device_lut(256, fb.device, lut)
    with torch.cuda.device(fb.device):
        L.check(L.load().cvx_draw_detections(fb.frame_jobs, fb.n, fb.max_h, fb.max_w, L.ptr(rows), L.ptr(counts), int(rows.shape[1]), L.ptr(lut),
                                             int(lut.shape[0]), int(thickness), int(font_scale), L.stream_ptr(fb.device)), "cvx_draw_detections")
    return fb.frames


def draw_tracks(frames, rows: torch.Tensor, ids: torch.Tensor, counts: torch.Tensor, lut=None, thickness: int = 2, font_scale: int = 2,
                batch: FrameBatch = None):
    """``cvx_draw_tracks``: ``draw_detections`` for rows with track ids (``track.Tracker.update``).  ``ids``: (B, K)
    int32 on the device; a row whose id is negative is not painted, the label is ``"{id % 1000000}:{cls}"`` and the colour entry
    ``(id + 1) % len(lut)``, so an object keeps its colour while it keeps its id."""
    fb = batch if batch is not None else FrameBatch(frames)
    if rows.dim() != 3 or rows.shape[0] != fb.n or rows.shape[2] != 6 or rows.dtype != torch.float32 or rows.device != fb.device:
        raise ValueError(f"rows: ({fb.n}, K, 6) float32 on {fb.device}")
    if counts.dtype != torch.int32 or counts.numel() != fb.n or counts.device != fb.device:
        raise ValueError("counts: (B) int32 on the frames' device")
    if ids.dtype != torch.int32 or tuple(ids.shape) != tuple(rows.shape[:2]) or ids.device != fb.device:
        raise ValueError("ids: (B, K) int32 on the frames' device")
    rows, counts, ids = rows.contiguous(), counts.contiguous(), ids.contiguous()
    lut = _device_lut(256, fb.device, lut)
    with torch.cuda.device(fb.device):
        L.check(L.load().cvx_draw_tracks(fb.frame_jobs, fb.n, fb.max_h, fb.max_w, L.ptr(rows), L.ptr(counts), int(rows.shape[1]), L.ptr(ids),
                                         L.ptr(lut), int(lut.shape[0]), int(thickness), int(font_scale), L.stream_ptr(fb.device)), "cvx_draw_tracks")
    return fb.frames


def seg_overlay(frames, logits_rows: torch.Tensor, nc: int, level_hw, net_hw, lut=None, bgr: bool = False, batch: FrameBatch = None):
    """``cvx_seg_overlay``: logits_rows (B, lh * lw, ld) fp32 as ``forward_rows`` leaves them for a ``net_hw`` input -> class colours
    blended 50/50 into the RGB frames, in place; ``bgr`` writes B, G, R.  ``lut``: (nc, 3) uint8 RGB on the device, default the VOC palette."""
    fb = batch if batch is not None else FrameBatch(frames)
    lh, lw = int(level_hw[0]), int(level_hw[1])
    if (logits_rows.dim() != 3 or logits_rows.shape[0] != fb.n or logits_rows.shape[1] != lh * lw or logits_rows.shape[2] < nc
            or logits_rows.dtype != torch.float32 or logits_rows.device != fb.device):
        raise ValueError(f"logits_rows: ({fb.n}, {lh * lw}, >= {nc}) float32 on {fb.device}, got {tuple(logits_rows.shape)} {logits_rows.dtype}")
    logits_rows = logits_rows.contiguous()
    lut = _device_lut(nc, fb.device, lut)
    if lut.shape[0] < nc:
        raise ValueError(f"lut: at least {nc} colours")
    with torch.cuda.device(fb.device):
        L.check(L.load().cvx_seg_overlay(fb.frame_jobs, fb.n, fb.max_h, fb.max_w, L.ptr(logits_rows), int(logits_rows.shape[2]), int(nc), lh, lw,
                                         int(net_hw[0]), int(net_hw[1]), L.ptr(lut), int(bool(bgr)), L.stream_ptr(fb.device)), "cvx_seg_overlay")
    return fb.frames


def slot_chunks(slots: int, batch_size: int):
    """``[(c0, c1), ...]``: ``slots`` cut into the fewest chunks of at most ``batch_size``, of one size ``ceil(slots / n)`` with at most one shorter chunk at
    the end.  The engine re-plans its per-batch buffers, and waits for its streams, whenever a forward's batch size
    differs from the previous one; 30 slots at ``batch_size`` 16 are 15 + 15, not 16 + 14."""
    slots, batch_size = int(slots), int(batch_size)
    if slots <= 0 or batch_size <= 0:
        raise ValueError("slots and batch_size are positive")
    n = -(-slots // batch_size)
    size = -(-slots // n)
    return [(c0, min(c0 + size, slots)) for c0 in range(0, slots, size)]


STITCH_WEIGHTS = {"mean": 0, "linear": 1}
STITCH_COUNT_MAX_NC = 128                            # cvx_seg_stitch counts through an nc x nc int32 histogram in LDS


def stitch_segmentation(frames, logits_rows: torch.Tensor, nc: int, level_hw, net_hw, tile_batch: TileBatch, weight: str = "linear",
                        labels: bool = True, draw: bool = False, bgr: bool = False, targets=None, counts: Optional[torch.Tensor] = None, lut=None):
    """``cvx_seg_stitch``: logits_rows (slots, lh * lw, ld) fp32 as ``forward_rows`` leaves them for the slots of
    ``tile_batch`` (a ``TileBatch`` of ``frames`` at ``net_hw`` with ``full_frame=False``) -> per frame pixel the logits of every covering
    tile, up-sampled by the taps of ``cvx_resize_bilinear_rows_to_nchw`` and blended (``weight``: ``"mean"``, every tile counts 1, or
    ``"linear"``, the product of the distances to the tile's borders), and their arg max.  ``labels``: returns the list of (h, w) uint8
    label maps on the device (else None); ``draw``: the class colours blended 50/50 into the frames in place, as ``seg_overlay`` (``bgr``,
    ``lut``); ``targets`` (a list of (h, w) uint8 device maps, rows may be padded) with ``counts`` ((nc, nc) int64 on the device):
    ``counts[target][label] += 1`` where ``target < nc``.  One launch for all frames, no host read."""
    lh, lw = int(level_hw[0]), int(level_hw[1])
    NH, NW = int(net_hw[0]), int(net_hw[1])
    nc = int(nc)
    if weight not in STITCH_WEIGHTS:
        raise ValueError(f"weight: one of {sorted(STITCH_WEIGHTS)}, got {weight!r}")
    if not 1 <= nc <= 256:
        raise ValueError(f"nc {nc}: labels are bytes, 1 <= nc <= 256")
    if lh <= 0 or lw <= 0 or NH <= 0 or NW <= 0:
        raise ValueError("level_hw and net_hw are positive")
    if not torch.is_tensor(logits_rows) or logits_rows.dim() != 3 or logits_rows.shape[1] != lh * lw or logits_rows.shape[2] < nc \
            or logits_rows.dtype != torch.float32:
        raise ValueError(f"logits_rows: (slots, {lh * lw}, >= {nc}) float32, got "
                         f"{tuple(logits_rows.shape) if torch.is_tensor(logits_rows) else type(logits_rows).__name__} {getattr(logits_rows, 'dtype', '')}")
    if (targets is None) != (counts is None):
        raise ValueError("targets and counts come together")
    if targets is not None and nc > STITCH_COUNT_MAX_NC:
        raise ValueError(f"the confusion counts are kept for nc <= {STITCH_COUNT_MAX_NC}")
    frames = list(frames)
    dev = _check_frames(frames)
    if not isinstance(tile_batch, TileBatch) or tile_batch.full_frame or tile_batch.input_hw != (NH, NW):
        raise ValueError(f"tile_batch: the TileBatch of the frames at {(NH, NW)} with full_frame=False")
    if len(frames) != tile_batch.n or any(a is not b for a, b in zip(frames, tile_batch.frames)):
        raise ValueError("tile_batch was built for other frames")
    if logits_rows.device != dev or logits_rows.shape[0] != tile_batch.slots:
        raise ValueError(f"logits_rows: {tile_batch.slots} slots on {dev}, got {tuple(logits_rows.shape)} on {logits_rows.device}")
    logits_rows = logits_rows.contiguous()
    F = tile_batch.n
    sizes = [(int(t.shape[0]), int(t.shape[1])) for t in frames]
    if targets is not None:
        targets = list(targets)
        if len(targets) != F:
            raise ValueError(f"targets: one (h, w) uint8 map per frame, got {len(targets)} for {F} frames")
        for t, (h, w) in zip(targets, sizes):
            if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != (h, w) or t.device != dev or t.stride(1) != 1 or t.stride(0) < w:
                raise ValueError(f"targets: a ({h}, {w}) uint8 map on {dev} with unit pixel stride per frame")
        if counts.dtype != torch.int64 or tuple(counts.shape) != (nc, nc) or counts.device != dev or not counts.is_contiguous():
            raise ValueError(f"counts: ({nc}, {nc}) int64, contiguous, on {dev}")
    if draw:
        lut = _device_lut(nc, dev, lut)
        if lut.shape[0] < nc or lut.device != dev:
            raise ValueError(f"lut: at least {nc} colours on {dev}")
    out = [torch.empty(h, w, dtype=torch.uint8, device=dev) for h, w in sizes] if labels else None
    label_maps = target_maps = None
    if labels or targets is not None:                         # the per-call pointer tables: one pinned blob, one asynchronous copy
        maps = ([(t.data_ptr(), t.stride(0), 0) for t in out] if labels else []) + \
               ([(t.data_ptr(), t.stride(0), 0) for t in targets] if targets is not None else [])
        host = torch.empty(16 * len(maps), dtype=torch.uint8, pin_memory=True)
        host.numpy().view(SEG_MAP_DTYPE)[:] = np.array(maps, dtype=SEG_MAP_DTYPE)
        blob = torch.empty(16 * len(maps), dtype=torch.uint8, device=dev)
        blob.copy_(host, non_blocking=True)
        tile_batch._stitch_host = host                        # alive until the copy has run
        label_maps = blob.data_ptr() if labels else None
        target_maps = (blob.data_ptr() + (16 * F if labels else 0)) if targets is not None else None
    with torch.cuda.device(dev):
        L.check(L.load().cvx_seg_stitch(L.ptr(logits_rows), tile_batch.slots, int(logits_rows.shape[2]), nc, lh, lw, NH, NW, tile_batch.seg_frames,
                                        tile_batch.seg_axes, tile_batch.n_axes, tile_batch.frame_jobs, F, tile_batch.max_h, tile_batch.max_w,
                                        L.C.c_void_p(label_maps), L.C.c_void_p(target_maps), L.ptr(counts), L.ptr(lut) if draw else L.C.c_void_p(0),
                                        STITCH_WEIGHTS[weight], int(bool(draw)), int(bool(bgr)), L.stream_ptr(dev)), "cvx_seg_stitch")
    return out


def read_detections(rows: torch.Tensor, counts: torch.Tensor, overflow: torch.Tensor, ids: Optional[torch.Tensor] = None) -> List[tuple]:
    """ONE host read of (rows, counts, overflow) -> per image ``(boxes (k, 4) float32, scores (k) float32, classes (k) int64)``, the format of
    ``decode_box``.  Raises ``CvxError`` when an image was dropped (NMS count -1 or a count past its block).  With ``ids`` (B, K) int32, a
    tracker's, the tuples gain ``ids (k) int32`` as a fourth element, -1 where a row has no track."""
    B, K = int(rows.shape[0]), int(rows.shape[1])
    parts = (rows.reshape(-1), counts.view(torch.float32).reshape(-1), overflow.view(torch.float32).reshape(-1))
    if ids is not None:
        parts += (ids.contiguous().view(torch.float32).reshape(-1),)
    flat = torch.cat(parts).cpu().numpy()
    r = flat[:B * K * 6].reshape(B, K, 6)
    tail = flat[B * K * 6:].view(np.int32)
    if int(tail[B]):
        raise L.CvxError(f"predict_batch: {int(tail[B])} image(s) dropped: an NMS count of -1 (more candidates than cvx_nms sorts), a count "
                         f"past its block or, tiled, a frame with more than {MERGE_CAP} candidates; raise the confidence threshold")
    found = [(r[b, :n, :4].copy(), r[b, :n, 4].copy(), r[b, :n, 5].astype(np.int64)) for b, n in enumerate(int(v) for v in tail[:B])]
    if ids is None:
        return found
    track = tail[B + 1:].reshape(B, K)
    return [t + (track[b, :len(t[1])].copy(),) for b, t in enumerate(found)]
