"""Device-side input pipeline of the DeepLabv3+ trainer: the reference's segmentation transforms (core/data/segmentation_dataset.py:82-293)
as ONE HIP launch per batch (``csrc/seg_pipeline.hip``: ``cvx_seg_pipeline``).

    training    ToTensor -> RGB2idx -> Resize(base) -> RandomCrop(crop) -> RandomHorizontalFlip -> Normalize      (get_voc_dataloader :262-276)
    validation  ToTensor -> RGB2idx -> Resize((H, W)) -> Normalize                                               (:280-291)

A batch of uint8 HWC pictures and their label pictures (uint8 ``(h, w, 3)`` colour coded, or uint8 ``(h, w)`` class indices) already in
device memory becomes the fp32 ``(B, 3, H, W)`` normalised batch and the int64 ``(B, H, W)`` targets ``SegTrainStep`` / ``cvx_seg_loss``
take.  The random draws are made on the host by ``draw_seg_params`` in the reference's order -- per item the crop origin ``i``, ``j`` from a
``torch.Generator`` (``RandomCrop.get_params``), then the flip from a ``random.Random`` (``RandomHorizontalFlip``) --; the job table and the
colour table go up in ONE pinned copy per batch, and nothing is read back.  There is no CPU fallback: pictures that are not on a GPU raise
``CvxError``.

What the reference does, kept, and where this differs:

1. **labels are resized bilinearly as floats and rounded half to even** -- ``Resize`` hands the integer class map to torchvision's
   ``F.resize``, which casts it to fp32, interpolates bilinearly, ``torch.round``s and casts back, so pixels on a class boundary get
   in-between labels (a pixel between classes 3 and 15 may become class 9).  That quirk is the default, ``label_resize="bilinear"``;
   ``label_resize="nearest"`` (``F.interpolate(mode="nearest")`` indexing) is offered beside it;
2. a mask colour that is not in the colour table becomes class 0, which is what the reference's 2^24-entry ``colormap2label`` holds there;
   the table here has K rows and is searched;
3. the resize is ``torch.nn.functional.interpolate(mode="bilinear", align_corners=False)`` without antialiasing, what torchvision 0.14.1's
   tensor resize calls; torchvision itself is not pinned by a fixture.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # segmentation_dataset.py:273
LABEL_RESIZE = {"bilinear": 0, "nearest": 1}

SEG_JOB_DTYPE = np.dtype([("image", "<u8"), ("mask", "<u8"), ("ih", "<i4"), ("iw", "<i4"), ("rh", "<i4"), ("rw", "<i4"), ("i", "<i4"), ("j", "<i4"),
                          ("flip", "<i4"), ("mask_channels", "<i4"), ("reserved", "<i4", (4,))])
assert SEG_JOB_DTYPE.itemsize == 64                  # struct cvx_seg_job, include/cvx_engine.h


def resized_size(ih: int, iw: int, base: int):
    """``Resize(size=base)`` with an int: the smaller edge becomes ``base``, the other ``int(base * long / short)`` (torchvision's
    ``_compute_resized_output_size``)."""
    ih, iw, base = int(ih), int(iw), int(base)
    if iw <= ih:
        return int(base * ih / iw), base
    return base, int(base * iw / ih)


def draw_seg_params(gen: Optional[torch.Generator], pyrng, size, base, crop_hw, train=True) -> Dict:
    """The host side of one output image of a ``(ih, iw)`` picture.  Training: ``Resize(base)`` fixes ``(rh, rw)``; ``RandomCrop.get_params``
    draws nothing when the resized picture already has the crop size, else ``i = torch.randint(0, rh - H + 1, (1,))`` and then
    ``j = torch.randint(0, rw - W + 1, (1,))`` from ``gen``; then ``flip = pyrng.random() < 0.5``.  A resized picture smaller than the crop
    raises ``CvxError``.  Validation (``train=False``): ``Resize((H, W))`` regardless of the aspect ratio, no crop, no flip, and neither
    generator is touched."""
    ih, iw = int(size[0]), int(size[1])
    H, W = int(crop_hw[0]), int(crop_hw[1])
    if ih <= 0 or iw <= 0:
        raise L.CvxError(f"segmentation pipeline: empty picture {ih} x {iw}")
    if not train:
        return dict(ih=ih, iw=iw, rh=H, rw=W, i=0, j=0, flip=0)
    rh, rw = resized_size(ih, iw, base)
    if rh < H or rw < W:
        raise L.CvxError(f"segmentation pipeline: a {ih} x {iw} picture resized to {rh} x {rw} is smaller than the {H} x {W} crop")
    if (rh, rw) == (H, W):
        i = j = 0
    else:
        i = int(torch.randint(0, rh - H + 1, (1,), generator=gen).item())
        j = int(torch.randint(0, rw - W + 1, (1,), generator=gen).item())
    return dict(ih=ih, iw=iw, rh=rh, rw=rw, i=i, j=j, flip=int(pyrng.random() < 0.5))


def _align(n, a=16):
    return (n + a - 1) // a * a


class DeviceSegAugmenter:
    """``aug(images, masks)`` -> ``(images (B, 3, H, W) fp32, targets (B, H, W) int64)`` on the pictures' device.

    ``images``: one uint8 HWC device tensor per output image; ``masks``: its label picture, uint8 ``(h, w, 3)`` in the colours of
    ``colormap`` (a sequence of K ``(r, g, b)``, e.g. ``voc_colormap()`` of core/algorithms/segmentation_2d.py) or, with ``colormap=None``,
    uint8 ``(h, w)`` class indices.  ``base_size`` is the reference's ``max(cfg.arch.input_size[1:])``.  ``train=False`` is the
    validation transform.  ``label_resize``: "bilinear" (the reference's float resize + round, module docstring) or "nearest"."""

    def __init__(self, crop_hw, base_size, colormap=None, train=True, seed=None, label_resize="bilinear", mean=MEAN, std=STD):
        import random
        self.crop_hw = (int(crop_hw[0]), int(crop_hw[1]))
        self.base_size = int(base_size)
        self.train = bool(train)
        if label_resize not in LABEL_RESIZE:
            raise ValueError(f'label_resize must be "bilinear" or "nearest", not {label_resize!r}')
        self.label_resize = label_resize
        self.colormap = None if colormap is None else np.asarray(colormap, np.uint8).reshape(-1, 3)
        if self.colormap is not None and not 0 < len(self.colormap) <= 256:
            raise ValueError("the colour table holds 1 ... 256 colours")
        self.gen = torch.Generator()
        if seed is not None:
            self.gen.manual_seed(int(seed))
        self.pyrng = random.Random(seed)
        self._mean = (C.c_float * 3)(*[float(v) for v in mean])
        self._std = (C.c_float * 3)(*[float(v) for v in std])

    def __call__(self, images: Sequence[torch.Tensor], masks: Sequence[torch.Tensor]):
        params = [draw_seg_params(self.gen, self.pyrng, tuple(t.shape[:2]), self.base_size, self.crop_hw, train=self.train) for t in images]
        return self.apply(params, images, masks)

    def apply(self, params: List[Dict], images: Sequence[torch.Tensor], masks: Sequence[torch.Tensor]):
        """Runs the launch for drawn parameters (``draw_seg_params`` results, or hand-made ones of the same form)."""
        H, W = self.crop_hw
        B = len(params)
        if B == 0 or len(images) != B or len(masks) != B:
            raise ValueError("parameters, pictures and masks must pair up, at least one of each")
        if not all(torch.is_tensor(t) and t.is_cuda for t in list(images) + list(masks)):
            raise L.CvxError("DeviceSegAugmenter takes uint8 pictures and masks in GPU memory (there is no CPU path)")
        dev = images[0].device
        channels = 1 if self.colormap is None else 3
        want_mask = "(h, w) class indices" if channels == 1 else "(h, w, 3) colours"
        jobs, keep_alive = [], []
        for p, t, m in zip(params, images, masks):
            ih, iw = int(p["ih"]), int(p["iw"])
            if t.dtype != torch.uint8 or t.dim() != 3 or tuple(t.shape) != (ih, iw, 3) or t.device != dev:
                raise L.CvxError(f"picture {tuple(t.shape)} {t.dtype} on {t.device} does not fit its job ({ih}, {iw}, 3) uint8 on {dev}")
            if m.dtype != torch.uint8 or tuple(m.shape) != ((ih, iw) if channels == 1 else (ih, iw, 3)) or m.device != dev:
                raise L.CvxError(f"mask {tuple(m.shape)} {m.dtype} on {m.device}: expected uint8 {want_mask} of a {ih} x {iw} picture on {dev}")
            rh, rw, i, j = int(p["rh"]), int(p["rw"]), int(p["i"]), int(p["j"])
            if ih <= 0 or iw <= 0 or not (0 <= i <= rh - H and 0 <= j <= rw - W):
                raise L.CvxError(f"crop origin ({i}, {j}) of a {H} x {W} crop outside the {rh} x {rw} resized picture")
            t, m = t.contiguous(), m.contiguous()
            keep_alive += [t, m]
            jobs.append((t.data_ptr(), m.data_ptr(), ih, iw, rh, rw, i, j, int(bool(p["flip"])), channels, (0, 0, 0, 0)))
        K = 0 if self.colormap is None else len(self.colormap)
        # one pinned blob: jobs | colour table (3 K bytes, sent along every time: cheaper than a second copy and a "changed" flag).  As in
        # augment.py the blob is a fresh tensor per call: torch's caching host allocator hands back a pinned block it has seen the
        # previous copy finish on, which a buffer kept here and rewritten while that copy is in flight would not guarantee
        o_col = _align(B * 64)
        total = _align(o_col + 3 * K) if K else o_col
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        hv[:B * 64].view(SEG_JOB_DTYPE)[:] = np.array(jobs, dtype=SEG_JOB_DTYPE)
        if K:
            hv[o_col:o_col + 3 * K] = self.colormap.reshape(-1)
        blob = torch.empty(total, dtype=torch.uint8, device=dev)
        blob.copy_(host, non_blocking=True)
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        targets = torch.empty(B, H, W, dtype=torch.int64, device=dev)
        self._launch(blob, o_col, B, K, out, targets)
        return out, targets

    def _launch(self, blob, o_col, B, K, out, targets):
        """the launch on the current stream of the blob's device"""
        H, W = self.crop_hw
        base, P, lib = blob.data_ptr(), C.c_void_p, L.load()
        with torch.cuda.device(blob.device):
            L.check(lib.cvx_seg_pipeline(P(base), B, P(base + o_col if K else 0), K, LABEL_RESIZE[self.label_resize], self._mean, self._std,
                                         L.ptr(out), L.ptr(targets), H, W, L.stream_ptr(blob.device)), "cvx_seg_pipeline")


class DeviceSegLoader:
    """Iterable of ``(images, targets)`` batches over any indexable ``source`` of ``(uint8 HWC image tensor, uint8 mask tensor)``: what
    ``VOCSegmentation`` + the transforms + ``DataLoader`` are in the reference, to be passed as ``dataloader=`` / ``val_dataloader=`` to
    ``DeeplabV3PlusTrainer`` or as ``dataloader=`` to ``DeeplabV3PlusA.evaluate_on_voc``.  Pictures that are still on the host are moved to
    ``device`` first.

    Training (``augmenter.train``): ``length`` batches; items are taken in order, wrapping around.  Validation
    (``DeviceSegAugmenter(train=False)``): the source is walked once, in order; ``drop_last=False`` (the reference's segmentation
    ``DataLoader`` setting) yields a short last batch, ``drop_last=True`` leaves it out; ``length`` is not needed."""

    def __init__(self, source, batch_size, augmenter: DeviceSegAugmenter, length: Optional[int] = None, device="cuda", drop_last=False):
        self.source, self.batch_size, self.augmenter = source, int(batch_size), augmenter
        self.device, self.drop_last = torch.device(device), bool(drop_last)
        if augmenter.train:
            if length is None:
                raise ValueError("a training loader needs its length in batches")
            self.length = int(length)
        else:
            n = len(source)
            self.length = n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __len__(self):
        return self.length

    def _item(self, i):
        image, mask = self.source[int(i)]
        return image.to(self.device, non_blocking=True), mask.to(self.device, non_blocking=True)

    def __iter__(self):
        n, aug = len(self.source), self.augmenter
        for k in range(self.length):
            first = k * self.batch_size
            ids = [i % n for i in range(first, first + self.batch_size)] if aug.train else range(first, min(first + self.batch_size, n))
            picked = [self._item(i) for i in ids]
            yield aug([p[0] for p in picked], [p[1] for p in picked])
