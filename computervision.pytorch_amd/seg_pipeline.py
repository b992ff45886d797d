"""Device-side input pipeline of the DeepLabv3+ trainer: the reference's segmentation transforms (core/data/segmentation_dataset.py:82-293)
as ONE HIP launch per batch (``csrc/seg_pipeline.hip``: ``cvx_seg_pipeline``).

    training    ToTensor -> RGB2idx -> Resize(base) -> RandomCrop(crop) -> RandomHorizontalFlip -> Normalize      (get_voc_dataloader :262-276)
    validation  ToTensor -> RGB2idx -> Resize((H, W)) -> Normalize                                               (:280-291)

A batch of uint8 HWC pictures and their label pictures (uint8 ``(h, w, 3)`` colour coded, or uint8 ``(h, w)`` class indices) already in
device memory becomes the fp32 ``(B, 3, H, W)`` normalised batch and the int64 ``(B, H, W)`` targets ``SegTrainStep`` / ``cvx_seg_criterion_loss``
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

Beyond the reference, ``DeviceSegAugmenter(recipe=...)`` adds what published DeepLabv3+ recipes train with -- random zoom with padding,
rotation, photometric distortion, Gaussian blur -- and ``unlisted="ignore"`` sends unlisted colours to ``ignore_index``; both go through
``cvx_seg_pipeline_aug``, still one launch per batch (``draw_seg_aug_params``).  Without them nothing changes.
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


# ---- the training recipe (cvx_seg_pipeline_aug) -----------------------------------------------------------------------
SEG_AUG_JOB_DTYPE = np.dtype([("image", "<u8"), ("mask", "<u8"), ("ih", "<i4"), ("iw", "<i4"), ("rh", "<i4"), ("rw", "<i4"), ("i", "<i4"), ("j", "<i4"),
                              ("flip", "<i4"), ("mask_channels", "<i4"), ("cos", "<f4"), ("sin", "<f4"), ("flags", "<i4"), ("beta", "<f4"),
                              ("alpha", "<f4"), ("sat", "<f4"), ("hue", "<f4"), ("blur_k", "<i4"), ("taps", "<f4", (9,)), ("reserved", "<i4", (3,))])
assert SEG_AUG_JOB_DTYPE.itemsize == 128             # struct cvx_seg_aug_job, include/cvx_engine.h
AUG_BRIGHTNESS, AUG_CONTRAST, AUG_CONTRAST_LAST, AUG_SATURATION, AUG_HUE, AUG_BLUR = 1, 2, 4, 8, 16, 32      # CVX_SEG_AUG_*
UNLISTED = {"class0": 0, "ignore": 1}
RECIPE_KEYS = ("scale", "rotate", "photometric", "blur", "fill")
DEFAULT_FILL = (124, 116, 104)
MAX_EXTENT = 1 << 20                                 # sizes and origins stay far below 2^22, where x + 0.5 is exact in fp32


def gaussian_taps(kernel: int, sigma: float) -> np.ndarray:
    """torchvision's ``_get_gaussian_kernel1d``: ``exp(-x^2 / 2 sigma^2)`` at ``x = -(k-1)/2 ... (k-1)/2``, normalised in float64, rounded to
    fp32"""
    half = (int(kernel) - 1) * 0.5
    x = np.linspace(-half, half, int(kernel), dtype=np.float64)
    pdf = np.exp(-0.5 * (x / float(sigma)) ** 2)
    return (pdf / pdf.sum()).astype(np.float32)


def check_recipe(recipe: Dict) -> Dict:
    """The recipe with its missing keys filled in as ``None`` (that part off) and its values checked."""
    unknown = set(recipe) - set(RECIPE_KEYS)
    if unknown:
        raise ValueError(f"recipe: unknown keys {sorted(unknown)}; it takes {RECIPE_KEYS}")
    r = {k: recipe.get(k) for k in RECIPE_KEYS}
    if r["scale"] is not None:
        lo, hi = (float(v) for v in r["scale"])
        if not 0 < lo <= hi:
            raise ValueError(f"recipe scale {r['scale']}: 0 < low <= high")
        r["scale"] = (lo, hi)
    if r["rotate"] is not None:
        r["rotate"] = dict(degrees=float(r["rotate"]["degrees"]), p=float(r["rotate"].get("p", 0.5)))
    if r["photometric"] is not None:
        ph = dict(r["photometric"])
        extra = set(ph) - {"brightness", "contrast", "saturation", "hue", "p"}
        if extra:
            raise ValueError(f"recipe photometric: unknown keys {sorted(extra)}")
        out = dict(brightness=ph.get("brightness"), contrast=ph.get("contrast"), saturation=ph.get("saturation"), hue=ph.get("hue"),
                   p=float(ph.get("p", 0.5)))
        for key in ("contrast", "saturation"):
            if out[key] is not None:
                lo, hi = (float(v) for v in out[key])
                if not 0 <= lo <= hi:
                    raise ValueError(f"recipe photometric {key} {out[key]}: 0 <= low <= high")
                out[key] = (lo, hi)
        if out["brightness"] is not None and not 0 <= float(out["brightness"]) <= 255:
            raise ValueError("recipe photometric brightness: 0 ... 255")
        if out["hue"] is not None and not 0 <= float(out["hue"]) <= 360:
            raise ValueError("recipe photometric hue: 0 ... 360 degrees")
        r["photometric"] = out
    if r["blur"] is not None:
        k = int(r["blur"]["kernel"])
        if k not in (3, 5, 7, 9):
            raise ValueError(f"recipe blur kernel {k}: an odd number of taps, 3 ... 9")
        lo, hi = (float(v) for v in r["blur"].get("sigma", (0.1, 2.0)))
        if not 0 < lo <= hi:
            raise ValueError("recipe blur sigma: 0 < low <= high")
        r["blur"] = dict(kernel=k, sigma=(lo, hi), p=float(r["blur"].get("p", 0.5)))
    fill = DEFAULT_FILL if r["fill"] is None else tuple(float(v) for v in r["fill"])
    if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
        raise ValueError("recipe fill: three values in 0 ... 255")
    r["fill"] = fill
    return r


def draw_seg_aug_params(pyrng, size, base, crop_hw, recipe: Dict) -> Dict:
    """The host side of one output image under a recipe (``check_recipe``'s form).  Every draw comes from ``pyrng`` (a ``random.Random``), in
    this order, which is part of the interface; a part that is off draws nothing, and a value is drawn only after its coin came up:

    1. zoom ``s = uniform(*scale)``; ``(rh, rw) = max(1, int(v * s + 0.5))`` of ``resized_size(ih, iw, base)``;
    2. rotation: ``random() < p``, then ``uniform(-degrees, degrees)``; ``cos`` / ``sin`` are taken in float64 and rounded to fp32;
    3. crop origin ``i = randint(min(0, rh - H), max(0, rh - H))``, then ``j`` likewise: a negative origin places a picture smaller than
       the crop at a random spot inside it;
    4. flip: ``random() < 0.5``;
    5. photometric, in mmseg's ``PhotoMetricDistortion`` order of decisions, each coin ``random() < p``: brightness coin, then
       ``uniform(-brightness, brightness) / 255``; the contrast-first / contrast-last coin (``random() < 0.5`` means last; drawn when
       contrast is on); contrast coin, then ``uniform(*contrast)``; saturation coin, then ``uniform(*saturation)``; hue coin, then
       ``uniform(-hue, hue)`` degrees;
    6. blur: ``random() < p``, then ``sigma = uniform(*sigma)`` and the ``kernel`` taps of ``gaussian_taps``."""
    ih, iw = int(size[0]), int(size[1])
    H, W = int(crop_hw[0]), int(crop_hw[1])
    if ih <= 0 or iw <= 0:
        raise L.CvxError(f"segmentation pipeline: empty picture {ih} x {iw}")
    rh, rw = resized_size(ih, iw, base)
    if recipe["scale"] is not None:
        s = pyrng.uniform(*recipe["scale"])
        rh, rw = max(1, int(rh * s + 0.5)), max(1, int(rw * s + 0.5))
    job = dict(ih=ih, iw=iw, rh=rh, rw=rw, cos=1.0, sin=0.0, flags=0, beta=0.0, alpha=1.0, sat=1.0, hue=0.0, blur_k=0, taps=(0.0,) * 9)
    rot = recipe["rotate"]
    if rot is not None and pyrng.random() < rot["p"]:
        angle = np.deg2rad(np.float64(pyrng.uniform(-rot["degrees"], rot["degrees"])))
        job["cos"], job["sin"] = float(np.float32(np.cos(angle))), float(np.float32(np.sin(angle)))
    job["i"] = pyrng.randint(min(0, rh - H), max(0, rh - H))
    job["j"] = pyrng.randint(min(0, rw - W), max(0, rw - W))
    job["flip"] = int(pyrng.random() < 0.5)
    ph = recipe["photometric"]
    if ph is not None:
        p = ph["p"]
        if ph["brightness"] is not None and pyrng.random() < p:
            job["flags"] |= AUG_BRIGHTNESS
            job["beta"] = float(np.float32(pyrng.uniform(-float(ph["brightness"]), float(ph["brightness"])) / 255.0))
        if ph["contrast"] is not None:
            if pyrng.random() < 0.5:
                job["flags"] |= AUG_CONTRAST_LAST
            if pyrng.random() < p:
                job["flags"] |= AUG_CONTRAST
                job["alpha"] = float(np.float32(pyrng.uniform(*ph["contrast"])))
        if ph["saturation"] is not None and pyrng.random() < p:
            job["flags"] |= AUG_SATURATION
            job["sat"] = float(np.float32(pyrng.uniform(*ph["saturation"])))
        if ph["hue"] is not None and pyrng.random() < p:
            job["flags"] |= AUG_HUE
            job["hue"] = float(np.float32(pyrng.uniform(-float(ph["hue"]), float(ph["hue"]))))
    blur = recipe["blur"]
    if blur is not None and pyrng.random() < blur["p"]:
        taps = gaussian_taps(blur["kernel"], pyrng.uniform(*blur["sigma"]))
        job["flags"] |= AUG_BLUR
        job["blur_k"] = blur["kernel"]
        job["taps"] = tuple(float(v) for v in taps) + (0.0,) * (9 - len(taps))
    return job


def neutral_aug_job(p: Dict) -> Dict:
    """A ``draw_seg_params`` result in the form ``cvx_seg_pipeline_aug`` takes: no rotation, no flags, no blur"""
    return dict(p, cos=1.0, sin=0.0, flags=0, beta=0.0, alpha=1.0, sat=1.0, hue=0.0, blur_k=0, taps=(0.0,) * 9)


def _align(n, a=16):
    return (n + a - 1) // a * a


class DeviceSegAugmenter:
    """``aug(images, masks)`` -> ``(images (B, 3, H, W) fp32, targets (B, H, W) int64)`` on the pictures' device.

    ``images``: one uint8 HWC device tensor per output image; ``masks``: its label picture, uint8 ``(h, w, 3)`` in the colours of
    ``colormap`` (a sequence of K ``(r, g, b)``, e.g. ``voc_colormap()`` of core/algorithms/segmentation_2d.py) or, with ``colormap=None``,
    uint8 ``(h, w)`` class indices.  ``base_size`` is the reference's ``max(cfg.arch.input_size[1:])``.  ``train=False`` is the
    validation transform.  ``label_resize``: "bilinear" (the reference's float resize + round, module docstring) or "nearest".

    ``recipe`` (training only) adds what the reference's transforms lack -- any key may be missing or ``None``, which turns that part off::

        recipe=dict(scale=(0.5, 2.0), rotate=dict(degrees=10, p=0.5),
                    photometric=dict(brightness=32, contrast=(0.5, 1.5), saturation=(0.5, 1.5), hue=18, p=0.5),
                    blur=dict(kernel=5, sigma=(0.1, 2.0), p=0.5), fill=(124, 116, 104))

    With a recipe the draws are ``draw_seg_aug_params``'s, all from the ``random.Random``; a picture smaller than the crop is padded: the
    image with ``fill``, the targets with ``ignore_index`` (-100, ``SegLoss``'s default).  ``unlisted="ignore"`` sends a mask colour that
    is not in ``colormap`` (VOC's void outline) to ``ignore_index`` instead of class 0; it needs ``label_resize="nearest"``.  A recipe or
    ``unlisted="ignore"`` goes through ``cvx_seg_pipeline_aug``; without either the class is what it was: ``cvx_seg_pipeline`` and
    ``draw_seg_params``'s draws."""

    def __init__(self, crop_hw, base_size, colormap=None, train=True, seed=None, label_resize="bilinear", mean=MEAN, std=STD, recipe=None,
                 ignore_index=-100, unlisted="class0"):
        import random
        self.crop_hw = (int(crop_hw[0]), int(crop_hw[1]))
        self.base_size = int(base_size)
        self.train = bool(train)
        if label_resize not in LABEL_RESIZE:
            raise ValueError(f'label_resize must be "bilinear" or "nearest", not {label_resize!r}')
        self.label_resize = label_resize
        if unlisted not in UNLISTED:
            raise ValueError(f'unlisted must be "class0" or "ignore", not {unlisted!r}')
        if unlisted == "ignore" and label_resize == "bilinear":
            raise ValueError('unlisted="ignore" needs label_resize="nearest": an ignore value cannot be mixed as a float')
        if recipe is not None and not self.train:
            raise ValueError("a recipe belongs to training: train=False takes none")
        self.unlisted = unlisted
        self.ignore_index = int(ignore_index)
        if not -2 ** 31 <= self.ignore_index < 2 ** 31:
            raise ValueError("ignore_index must fit an int32")
        self.recipe = None if recipe is None else check_recipe(recipe)
        self._fill = (C.c_float * 3)(*(self.recipe["fill"] if self.recipe else DEFAULT_FILL))
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
        if self.recipe is not None:
            params = [draw_seg_aug_params(self.pyrng, tuple(t.shape[:2]), self.base_size, self.crop_hw, self.recipe) for t in images]
        else:
            params = [draw_seg_params(self.gen, self.pyrng, tuple(t.shape[:2]), self.base_size, self.crop_hw, train=self.train) for t in images]
        return self.apply(params, images, masks)

    @staticmethod
    def _aug_fields(p):
        """the recipe half of one hand-made job, checked: (cos, sin, flags, beta, alpha, sat, hue, blur_k, taps[9])"""
        cos, sin, flags = float(p.get("cos", 1.0)), float(p.get("sin", 0.0)), int(p.get("flags", 0))
        beta, alpha, sat, hue = (float(p.get(k, d)) for k, d in (("beta", 0.0), ("alpha", 1.0), ("sat", 1.0), ("hue", 0.0)))
        blur_k = int(p.get("blur_k", 0))
        taps = tuple(float(v) for v in p.get("taps", ()))
        if not all(np.isfinite(v) for v in (cos, sin, beta, alpha, sat, hue) + taps) or flags & ~63 or abs(hue) > 360.0:
            raise L.CvxError("segmentation recipe job: finite values, flags below 64 and a hue shift within 360 degrees")
        if bool(flags & AUG_BLUR) != (blur_k > 0) or blur_k not in (0, 3, 5, 7, 9) or len(taps) > 9 or len(taps) < blur_k:
            raise L.CvxError(f"segmentation recipe job: blur_k {blur_k} with {len(taps)} taps and flags {flags}: 3, 5, 7 or 9 taps with the blur "
                             "flag, or 0 without it")
        return cos, sin, flags, beta, alpha, sat, hue, blur_k, taps + (0.0,) * (9 - len(taps))

    def apply(self, params: List[Dict], images: Sequence[torch.Tensor], masks: Sequence[torch.Tensor]):
        """Runs the launch for drawn parameters (``draw_seg_params`` results, or hand-made ones of the same form).  With a recipe the jobs
        have ``draw_seg_aug_params``'s form: beside ``ih, iw, rh, rw, i, j, flip`` the fields ``cos``, ``sin``, ``flags`` (``AUG_*`` bits),
        ``beta``, ``alpha``, ``sat``, ``hue``, ``blur_k`` and ``taps``, each optional (neutral when missing), and the origin may lie
        anywhere."""
        H, W = self.crop_hw
        B = len(params)
        if B == 0 or len(images) != B or len(masks) != B:
            raise ValueError("parameters, pictures and masks must pair up, at least one of each")
        if not all(torch.is_tensor(t) and t.is_cuda for t in list(images) + list(masks)):
            raise L.CvxError("DeviceSegAugmenter takes uint8 pictures and masks in GPU memory (there is no CPU path)")
        dev = images[0].device
        channels = 1 if self.colormap is None else 3
        want_mask = "(h, w) class indices" if channels == 1 else "(h, w, 3) colours"
        aug = self.recipe is not None or self.unlisted != "class0"           # cvx_seg_pipeline_aug; else cvx_seg_pipeline as ever
        jobs, keep_alive = [], []
        for p, t, m in zip(params, images, masks):
            ih, iw = int(p["ih"]), int(p["iw"])
            if t.dtype != torch.uint8 or t.dim() != 3 or tuple(t.shape) != (ih, iw, 3) or t.device != dev:
                raise L.CvxError(f"picture {tuple(t.shape)} {t.dtype} on {t.device} does not fit its job ({ih}, {iw}, 3) uint8 on {dev}")
            if m.dtype != torch.uint8 or tuple(m.shape) != ((ih, iw) if channels == 1 else (ih, iw, 3)) or m.device != dev:
                raise L.CvxError(f"mask {tuple(m.shape)} {m.dtype} on {m.device}: expected uint8 {want_mask} of a {ih} x {iw} picture on {dev}")
            rh, rw, i, j = int(p["rh"]), int(p["rw"]), int(p["i"]), int(p["j"])
            if self.recipe is None:
                if ih <= 0 or iw <= 0 or not (0 <= i <= rh - H and 0 <= j <= rw - W):
                    raise L.CvxError(f"crop origin ({i}, {j}) of a {H} x {W} crop outside the {rh} x {rw} resized picture")
            elif ih <= 0 or iw <= 0 or not (0 < rh <= MAX_EXTENT and 0 < rw <= MAX_EXTENT and abs(i) <= MAX_EXTENT and abs(j) <= MAX_EXTENT):
                raise L.CvxError(f"segmentation recipe job: resized size {rh} x {rw} and origin ({i}, {j}) must stay within {MAX_EXTENT}")
            t, m = t.contiguous(), m.contiguous()
            keep_alive += [t, m]
            head = (t.data_ptr(), m.data_ptr(), ih, iw, rh, rw, i, j, int(bool(p["flip"])), channels)
            if aug:                            # without a recipe (unlisted="ignore" alone) the jobs are draw_seg_params's: neutral
                jobs.append(head + self._aug_fields(p if self.recipe is not None else {}) + ((0, 0, 0),))
            else:
                jobs.append(head + ((0, 0, 0, 0),))
        K = 0 if self.colormap is None else len(self.colormap)
        # one pinned blob: jobs | colour table (3 K bytes, sent along every time: cheaper than a second copy and a "changed" flag).  As in
        # augment.py the blob is a fresh tensor per call: torch's caching host allocator hands back a pinned block it has seen the
        # previous copy finish on, which a buffer kept here and rewritten while that copy is in flight would not guarantee
        dtype = SEG_AUG_JOB_DTYPE if aug else SEG_JOB_DTYPE
        o_col = _align(B * dtype.itemsize)
        total = _align(o_col + 3 * K) if K else o_col
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        hv[:B * dtype.itemsize].view(dtype)[:] = np.array(jobs, dtype=dtype)
        if K:
            hv[o_col:o_col + 3 * K] = self.colormap.reshape(-1)
        blob = torch.empty(total, dtype=torch.uint8, device=dev)
        blob.copy_(host, non_blocking=True)
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        targets = torch.empty(B, H, W, dtype=torch.int64, device=dev)
        (self._launch_aug if aug else self._launch)(blob, o_col, B, K, out, targets)
        return out, targets

    def _launch(self, blob, o_col, B, K, out, targets):
        """the launch on the current stream of the blob's device"""
        H, W = self.crop_hw
        base, P, lib = blob.data_ptr(), C.c_void_p, L.load()
        with torch.cuda.device(blob.device):
            L.check(lib.cvx_seg_pipeline(P(base), B, P(base + o_col if K else 0), K, LABEL_RESIZE[self.label_resize], self._mean, self._std,
                                         L.ptr(out), L.ptr(targets), H, W, L.stream_ptr(blob.device)), "cvx_seg_pipeline")

    def _launch_aug(self, blob, o_col, B, K, out, targets):
        """the same for a table of ``cvx_seg_aug_job``"""
        H, W = self.crop_hw
        base, P, lib = blob.data_ptr(), C.c_void_p, L.load()
        with torch.cuda.device(blob.device):
            L.check(lib.cvx_seg_pipeline_aug(P(base), B, P(base + o_col if K else 0), K, LABEL_RESIZE[self.label_resize], UNLISTED[self.unlisted],
                                             self.ignore_index, self._fill, self._mean, self._std, L.ptr(out), L.ptr(targets), H, W,
                                             L.stream_ptr(blob.device)), "cvx_seg_pipeline_aug")


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
