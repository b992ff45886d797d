"""Device-side input pipeline of the four detection trainers: resize + jitter, paste, flip, mosaic, HSV colour transform and the box
arithmetic of the reference's ``DetectionDataset`` (core/data/detection_dataset.py:100-345, 405-449) plus its collate functions
(core/data/collate.py:5-68), as two HIP launches per batch (``csrc/augment.hip``: ``cvx_aug_images``, ``cvx_aug_boxes``) for the YOLO
formats, and the padded box launch (``cvx_aug_boxes_padded``) followed by the target kernels (``cvx_ssd_encode_targets``,
``cvx_centernet_draw_targets``) for ``fmt="ssd"`` / ``fmt="centernet"``.  ``DeviceAugmenter(train=False)`` is the validation path,
``DetectionDataset(train=False)`` (get_random_data(random=False), :137-166): aspect-preserving bicubic resize centred on the canvas of
128, no flip, no colour transform (``cvx_aug_images_plain``), no random numbers.

A batch of uint8 HWC pictures already in device memory and their boxes become the fp32 ``(B, 3, H, W)`` batch and the targets the fused
train steps consume.  The randomisation is drawn on the host by ``draw_params`` in exactly the reference's order (so a seeded
``np.random.RandomState`` reproduces the reference's geometry and LUTs, pinned by tests/golden/aug_ref.npz); the job table, the LUTs and the
boxes go up in ONE pinned copy per batch.  There is no CPU fallback: pictures that are not on a GPU raise ``CvxError``.

Deliberate deviations from the reference:

1. the reference shuffles each picture's boxes (``np.random.shuffle``, :209,272); here boxes keep their source order (job order, then box
   order), so the compaction is deterministic;
2. ``mosaic_body`` reads ``iw, ih, _ = image.shape`` (:224), rows first, so its aspect ratio and box scaling are wrong for non-square
   sources; here width is the column count everywhere;
3. ``fmt="centernet"`` keeps the FIRST ``max_num_boxes`` boxes of an image in source order; the reference truncates to the same number
   after its shuffle (a consequence of deviation 1);
4. validation images are in [0, 1] like training images.  The reference's validation picture is ``np.float32`` in 0...255 (:150), and
   ``TF.to_tensor`` (:101) divides only uint8 input, so its validation batches are in 0...255; a network trained on [0, 1] inputs is meant
   to be validated on [0, 1] inputs.

The pixel primitives (bicubic resize, RGB<->HSV) follow OpenCV's uint8 algorithms as restated in tests/aug_restatement.py; their parity with
OpenCV's bytes is not pinned.

Beyond the reference: ``DeviceAugmenter(affine=..., mixup=...)`` runs a second stage of two launches behind the
first -- ``cvx_aug_warp_mix`` warps every canvas by its own random affine / perspective matrix and mixes a partner canvas of the same batch
in, ``cvx_aug_boxes_warp`` sends the labels through the same matrices and writes any of the four target formats -- with rules modelled on
YOLOv5's ``random_perspective``, ``box_candidates`` and ``mixup`` (``draw_warp``, restated in tests/aug_warp_restatement.py), and
``DeviceAugLoader(close_after=...)`` switches mosaic and MixUp off for the last epochs.  Both options default to off; then nothing new is
drawn or launched.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import engine as _engine

YOLO_FORMATS, TARGET_FORMATS = ("yolo8", "yolo7"), ("ssd", "centernet", "padded")

JOB_DTYPE = np.dtype([("src", "<u8"), ("ih", "<i4"), ("iw", "<i4"), ("nh", "<i4"), ("nw", "<i4"), ("dx", "<i4"), ("dy", "<i4"), ("flip", "<i4"),
                      ("out", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("quad", "<i4"), ("reserved", "<i4")])
assert JOB_DTYPE.itemsize == 64                      # struct cvx_aug_job, include/cvx_engine.h


def _rand(rng, a=0.0, b=1.0):
    """core/utils/useful_tools.py:16-18 get_random_number"""
    return rng.rand() * (b - a) + a


def make_lut(r) -> np.ndarray:
    """detection_dataset.py:200-203: (3, 256) uint8 hue / saturation / value tables of the gains r"""
    x = np.arange(0, 256, dtype=r.dtype)
    return np.stack([((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8)])


def _jitter_size(rng, ih, iw, h, w, jitter):
    new_ar = iw / ih * _rand(rng, 1 - jitter, 1 + jitter) / _rand(rng, 1 - jitter, 1 + jitter)
    scale = _rand(rng, 0.4, 1.0)
    if new_ar < 1:
        nh = int(scale * h)
        nw = int(nh * new_ar)
    else:
        nw = int(scale * w)
        nh = int(nw / new_ar)
    return nh, nw


def identity_lut() -> np.ndarray:
    return np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def draw_params(rng: np.random.RandomState, sizes: Sequence, input_shape, mosaic: bool, nboxes: Sequence[int] = None, jitter=0.3, hue=0.1,
                sat=0.7, val=0.4, train=True) -> Dict:
    """The host side of one output image.  ``sizes``: ``[(ih, iw)]`` for a plain image (get_random_data, :169-203), four of them in quadrant
    order for a mosaic (mosaic_for_voc :301-339 around mosaic_body :224-263).  Random numbers are consumed in the reference's order: plain --
    two jitter draws, scale, dx, dy, flip, uniform(-1, 1, 3); mosaic -- the two cut offsets, then per picture flip, two jitter draws, scale,
    and uniform(-1, 1, 3) last.  ``nboxes`` (mosaic): boxes per picture -- the reference mirrors a picture only when it has boxes (:228).
    ``train=False`` is get_random_data(random=False) (:137-142): ``scale = min(w / iw, h / ih)``, the picture centred, no flip, no mosaic,
    and ``rng`` is not touched; ``lut`` is the identity and ``r`` None (the validation image path applies no table).
    Returns ``{"jobs": [...], "lut": (3, 256) uint8, "r": gains, "cut": (cutx, cuty) | None}``."""
    h, w = int(input_shape[0]), int(input_shape[1])
    jobs = []
    cut = None
    if not train:
        if mosaic:
            raise ValueError("validation has no mosaic")
        (ih, iw), = sizes
        scale = min(w / iw, h / ih)
        nw, nh = int(iw * scale), int(ih * scale)
        if nh <= 0 or nw <= 0:
            raise L.CvxError(f"augmentation: a {ih} x {iw} picture collapses to {nh} x {nw}")
        jobs.append(dict(ih=int(ih), iw=int(iw), nh=nh, nw=nw, dx=(w - nw) // 2, dy=(h - nh) // 2, flip=0, quad=-1, rect=(0, 0, w, h)))
        return {"jobs": jobs, "lut": identity_lut(), "r": None, "cut": None}
    if not mosaic:
        (ih, iw), = sizes
        nh, nw = _jitter_size(rng, ih, iw, h, w, jitter)
        dx = int(_rand(rng, 0, w - nw))
        dy = int(_rand(rng, 0, h - nh))
        flip = bool(_rand(rng) < 0.5)
        jobs.append(dict(ih=int(ih), iw=int(iw), nh=nh, nw=nw, dx=dx, dy=dy, flip=int(flip), quad=-1, rect=(0, 0, w, h)))
    else:
        assert len(sizes) == 4
        nboxes = [1] * 4 if nboxes is None else nboxes
        min_offset_x = _rand(rng, 0.3, 0.7)
        min_offset_y = _rand(rng, 0.3, 0.7)
        cutx, cuty = int(w * min_offset_x), int(h * min_offset_y)
        cut = (cutx, cuty)
        rects = [(0, 0, cutx, cuty), (0, cuty, cutx, h), (cutx, cuty, w, h), (cutx, 0, w, cuty)]
        for index, (ih, iw) in enumerate(sizes):
            flip = bool(_rand(rng) < 0.5) and nboxes[index] > 0
            nh, nw = _jitter_size(rng, ih, iw, h, w, jitter)
            dx = cutx - nw if index in (0, 1) else cutx
            dy = cuty - nh if index in (0, 3) else cuty
            jobs.append(dict(ih=int(ih), iw=int(iw), nh=nh, nw=nw, dx=dx, dy=dy, flip=int(flip), quad=index, rect=rects[index]))
    r = rng.uniform(-1, 1, 3) * [hue, sat, val] + 1
    for jb in jobs:
        if jb["nh"] <= 0 or jb["nw"] <= 0:
            raise L.CvxError(f"augmentation: a {jb['ih']} x {jb['iw']} picture collapses to {jb['nh']} x {jb['nw']}")
    return {"jobs": jobs, "lut": make_lut(r), "r": r, "cut": cut}


def _align(n, a=16):
    return (n + a - 1) // a * a


# ---- stage 2: affine / perspective warp and MixUp ----
VIEW_DTYPE = np.dtype([("m", "<f4", (9,)), ("inv", "<f4", (9,)), ("s", "<f4"), ("partner", "<i4"), ("r", "<f4"), ("r1", "<f4"), ("reserved", "<i4", (2,))])
assert VIEW_DTYPE.itemsize == 96                     # struct cvx_aug_view, include/cvx_engine.h

AFFINE_DEFAULTS = dict(degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, min_wh=2.0, min_area_ratio=0.1, max_aspect=100.0)


def check_affine(affine, input_shape) -> Optional[Dict]:
    """``affine`` completed with the defaults, or None; refuses unknown keys, ranges the draws cannot take and a perspective that could bring
    the homogeneous w near 0 inside the picture (``perspective * max(H, W) >= 0.5``)."""
    if affine is None:
        return None
    unknown = set(affine) - set(AFFINE_DEFAULTS)
    if unknown:
        raise ValueError(f"affine: unknown option(s) {sorted(unknown)}; known: {sorted(AFFINE_DEFAULTS)}")
    a = {k: float(affine.get(k, v)) for k, v in AFFINE_DEFAULTS.items()}
    if not all(np.isfinite(v) for v in a.values()):
        raise ValueError(f"affine: {a}")
    if a["degrees"] < 0 or a["translate"] < 0 or a["perspective"] < 0 or not 0 <= a["scale"] < 1 or not 0 <= a["shear"] < 90:
        raise ValueError(f"affine: degrees, translate, perspective >= 0, 0 <= scale < 1 and 0 <= shear < 90 are needed, got {a}")
    if a["min_wh"] < 0 or a["min_area_ratio"] < 0 or a["max_aspect"] <= 1:
        raise ValueError(f"affine: min_wh >= 0, min_area_ratio >= 0 and max_aspect > 1 are needed, got {a}")
    if abs(a["perspective"]) * max(int(input_shape[0]), int(input_shape[1])) >= 0.5:
        raise ValueError(f"affine: perspective {a['perspective']} times the longer side of {tuple(input_shape)} reaches 0.5: the homogeneous w "
                         "would come near 0 inside the picture")
    return a


def warp_matrix(eight, input_shape) -> np.ndarray:
    """``M = T . Sh . R . P . C`` in float64 from the eight drawn numbers ``(p_x, p_y, angle in degrees, zoom s, shear_x in degrees, shear_y in
    degrees, t_x, t_y)``, YOLOv5's random_perspective: C moves the canvas centre to the origin, P carries the perspective terms, R is
    cv2.getRotationMatrix2D(angle, (0, 0), s), Sh the shears' tangents, T the translation by ``(t_x W, t_y H)``."""
    h, w = int(input_shape[0]), int(input_shape[1])
    px, py, angle, zoom, shx, shy, tx, ty = (float(v) for v in eight)
    C, P, R, Sh, T = (np.eye(3) for _ in range(5))
    C[0, 2], C[1, 2] = -w / 2, -h / 2
    P[2, 0], P[2, 1] = px, py
    ca, sa = zoom * np.cos(np.deg2rad(angle)), zoom * np.sin(np.deg2rad(angle))
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = ca, sa, -sa, ca
    Sh[0, 1], Sh[1, 0] = np.tan(np.deg2rad(shx)), np.tan(np.deg2rad(shy))
    T[0, 2], T[1, 2] = tx * w, ty * h
    return T @ Sh @ R @ P @ C


def draw_warp(rng: np.random.RandomState, B: int, input_shape, affine=None, mixup=0.0) -> Optional[Dict]:
    """The host side of stage 2 for a batch of ``B`` outputs, drawn AFTER the batch's ``draw_params`` draws, in a fixed order:

    1. with ``affine``: per canvas the eight numbers in YOLOv5's order, always all eight -- ``uniform(-perspective, perspective)`` twice,
       ``uniform(-degrees, degrees)``, ``uniform(1 - scale, 1 + scale)``, ``uniform(-shear, shear)`` twice, ``uniform(0.5 - translate,
       0.5 + translate)`` twice;
    2. with ``mixup > 0`` and ``B > 1``: per output ``rand() < mixup``, then the partner ``j = randint(B - 1)``, ``p = j + (j >= i)``, then
       ``beta(32, 32)``, always all three.

    With both off nothing is drawn and None is returned.  Otherwise ``{"M", "Minv": (B, 3, 3) float64, "s": (B,) float64, "partner": (B,)
    int (-1: none), "r", "r1": (B,) float32}`` -- what ``DeviceAugmenter.apply(warp=...)`` takes."""
    a = check_affine(affine, input_shape)
    mixup = float(mixup)
    if not 0.0 <= mixup <= 1.0:
        raise ValueError(f"mixup is a probability, got {mixup}")
    mix = mixup > 0 and B > 1
    if a is None and not mix:
        return None
    M, s = np.tile(np.eye(3), (B, 1, 1)), np.ones(B)
    if a is not None:
        for i in range(B):
            e = [rng.uniform(-a["perspective"], a["perspective"]), rng.uniform(-a["perspective"], a["perspective"]),
                 rng.uniform(-a["degrees"], a["degrees"]), rng.uniform(1 - a["scale"], 1 + a["scale"]),
                 rng.uniform(-a["shear"], a["shear"]), rng.uniform(-a["shear"], a["shear"]),
                 rng.uniform(0.5 - a["translate"], 0.5 + a["translate"]), rng.uniform(0.5 - a["translate"], 0.5 + a["translate"])]
            M[i], s[i] = warp_matrix(e, input_shape), e[3]
    partner, r = np.full(B, -1, np.int64), np.ones(B, np.float32)
    if mix:
        for i in range(B):
            take = rng.rand() < mixup
            j = int(rng.randint(B - 1))
            ratio = np.float32(rng.beta(32.0, 32.0))
            if take:
                partner[i], r[i] = j + (j >= i), ratio
    return {"M": M, "Minv": np.linalg.inv(M), "s": s, "partner": partner, "r": r, "r1": np.float32(1) - r}


def view_table(warp: Dict, B: int) -> np.ndarray:
    """``warp`` (a ``draw_warp`` result, or a hand-made one: ``M`` is needed, ``Minv`` defaults to the float64 inverse, ``s`` to 1, ``partner``
    to none, ``r`` to 1, ``r1`` to ``fp32(1) - r``) as ``B`` ``cvx_aug_view`` records, everything rounded to fp32 here."""
    M = np.asarray(warp["M"], np.float64).reshape(-1, 3, 3)
    Minv = np.asarray(warp["Minv"], np.float64).reshape(-1, 3, 3) if warp.get("Minv") is not None else np.linalg.inv(M)
    s = np.asarray(warp.get("s", np.ones(B)), np.float64).reshape(-1)
    partner = np.asarray(warp.get("partner", np.full(B, -1)), np.int64).reshape(-1)
    r = np.asarray(warp.get("r", np.ones(B)), np.float32).reshape(-1)
    r1 = np.asarray(warp["r1"], np.float32).reshape(-1) if warp.get("r1") is not None else np.float32(1) - r
    if not (len(M) == len(Minv) == len(s) == len(partner) == len(r) == len(r1) == B):
        raise ValueError(f"warp: every entry needs one value per output image ({B})")
    if not (np.isfinite(M).all() and np.isfinite(Minv).all() and np.isfinite(s).all() and (s > 0).all() and np.isfinite(r).all() and np.isfinite(r1).all()):
        raise ValueError("warp: matrices, zooms and mixing weights must be finite, zooms positive")
    if ((partner < -1) | (partner >= B) | (partner == np.arange(B))).any():
        raise ValueError(f"warp: a partner is another output of the batch (0 .. {B - 1}) or -1, got {partner.tolist()}")
    v = np.zeros(B, VIEW_DTYPE)
    v["m"], v["inv"], v["s"], v["partner"], v["r"], v["r1"] = M.reshape(B, 9), Minv.reshape(B, 9), s, partner, r, r1
    return v


class SsdTargetSpec(NamedTuple):
    """What ``fmt="ssd"`` needs of the algorithm object: ``priors`` (A, 4) fp32 corner boxes (numpy or tensor), the class count without
    background, the matching threshold and the two variances."""
    priors: object
    num_classes: int
    overlap_threshold: float
    variances: Tuple[float, float]


class CenterNetTargetSpec(NamedTuple):
    """What ``fmt="centernet"`` needs: the heat map's (h, w), the class count and K = cfg.train.max_num_boxes."""
    feature_hw: Tuple[int, int]
    num_classes: int
    max_boxes: int


def target_spec(fmt: str, algorithm):
    """The spec of ``fmt`` from an ``Ssd`` / ``CenterNetA`` object (duck-typed: this module does not import ``core``)."""
    if fmt == "ssd":
        return SsdTargetSpec(algorithm.anchors, int(algorithm.num_classes), float(algorithm.overlap_threshold),
                             tuple(float(v) for v in algorithm.variance[::2]))
    if fmt == "centernet":
        cfg = algorithm.cfg
        ratio = int(cfg.arch.downsampling_ratio)
        return CenterNetTargetSpec((int(cfg.arch.input_size[1]) // ratio, int(cfg.arch.input_size[2]) // ratio), int(algorithm.num_classes),
                                   int(getattr(cfg.train, "max_num_boxes", 30)))
    raise ValueError(fmt)


class DeviceAugmenter:
    """``aug(images, boxes)`` -> ``(images (B, 3, H, W) fp32, targets)`` on the pictures' device.

    ``images``: one entry per output image -- a uint8 HWC device tensor, or (mosaic) a sequence of four of them in quadrant order (top-left,
    bottom-left, bottom-right, top-right); ``boxes`` the same nesting of ``(n, 5)`` arrays ``(x1, y1, x2, y2, cls)`` in source pixels.
    ``targets`` is yolo8_collate's dict ``{"batch_idx", "cls", "bboxes"}`` or, with ``fmt="yolo7"``, yolo7_collate's ``(N, 6)`` tensor
    ``[image, cls, cx, cy, w, h]``; both are views of the box kernel's output.  With ``exact=True`` (what the loss kernels need) the
    number of surviving boxes is read back -- the only host synchronisation; ``exact=False`` returns all rows (unused ones carry image
    index -1) and leaves the count in ``last_count`` on the device.

    ``fmt="ssd"`` returns ssd_collate's ``y_true (B, A, 4 + (nc + 1) + 1)`` and ``fmt="centernet"`` centernet_collate's ``[heatmap, reg, wh,
    reg_mask, indices]``; both need ``target=``, the ``Ssd`` / ``CenterNetA`` object or a ``SsdTargetSpec`` / ``CenterNetTargetSpec``.  The
    box kernel writes ``(B, capacity, 5)`` labels and per-image counts that the target kernel reads in place, so these two formats have NO
    host synchronisation (``exact`` is ignored): the capacity is known on the host beforehand -- for SSD the largest number of source boxes
    of one image in the batch, so nothing can overflow; for CenterNet K = max_num_boxes, longer lists are cut to their first K boxes.  The
    per-image counts stay on the device in ``last_count`` and the overflow word (non-zero when an image was cut) in ``last_overflow``.

    ``train=False`` is the validation path (module docstring): no mosaic, no flip, no colour transform, no random numbers, all four formats.

    ``affine`` (None, or a dict of any of ``AFFINE_DEFAULTS``' keys: degrees, translate, scale, shear, perspective and the box tests min_wh,
    min_area_ratio, max_aspect) and ``mixup`` (the probability that an output takes a partner from its own batch) are training options and
    off by default; with either on, ``draw_warp`` draws after the batch's ``draw_params`` draws and ``apply`` runs stage 2.  The warp last
    applied (None without stage 2) stays in ``last_warp``.  ``__call__(..., mixup=0.0)`` overrides the probability for one batch."""

    def __init__(self, input_shape, mosaic=False, mosaic_prob=0.5, seed=None, jitter=0.3, hue=0.1, sat=0.7, val=0.4, train=True, target=None,
                 affine=None, mixup=0.0):
        self.input_shape = (int(input_shape[0]), int(input_shape[1]))
        self.train = bool(train)
        self.affine, self.mixup = check_affine(affine, self.input_shape), float(mixup)
        if not 0.0 <= self.mixup <= 1.0:
            raise ValueError(f"mixup is a probability, got {mixup}")
        if not self.train and (self.affine is not None or self.mixup > 0):
            raise ValueError("affine and mixup are training options: validation pictures are not warped or mixed")
        self.last_warp = None
        self.mosaic, self.mosaic_prob = bool(mosaic) and self.train, float(mosaic_prob)
        self.rng = np.random.RandomState(seed)
        self.gains = dict(jitter=jitter, hue=hue, sat=sat, val=val)
        self.target = target
        self.last_count = None
        self.last_overflow = None
        self._priors = None

    def want_mosaic(self) -> bool:
        """The per-item draw of DetectionDataset.__getitem__ (:62): a loader asks before it fetches the three further pictures.  Validation
        draws nothing."""
        return self.mosaic and _rand(self.rng) < self.mosaic_prob

    def _spec(self, fmt):
        if self.target is None:
            raise ValueError(f'fmt="{fmt}" needs DeviceAugmenter(target=...): the algorithm object or a target spec')
        spec = self.target if isinstance(self.target, (SsdTargetSpec, CenterNetTargetSpec)) else target_spec(fmt, self.target)
        if not isinstance(spec, SsdTargetSpec if fmt == "ssd" else CenterNetTargetSpec):
            raise ValueError(f'fmt="{fmt}" with a {type(spec).__name__}')
        return spec

    def __call__(self, images, boxes, fmt="yolo8", exact=True, mixup=None):
        groups = [list(e) if isinstance(e, (list, tuple)) else [e] for e in images]
        bgroups = [list(b) if isinstance(b, (list, tuple)) else [b] for b in boxes]
        params = []
        for g, bg in zip(groups, bgroups):
            if len(g) not in (1, 4) or len(bg) != len(g):
                raise ValueError("an output image takes one picture, or four for a mosaic, and as many box arrays")
            params.append(draw_params(self.rng, [tuple(t.shape[:2]) for t in g], self.input_shape, len(g) == 4,
                                      nboxes=[len(np.asarray(b).reshape(-1, 5)) for b in bg], train=self.train, **self.gains))
        warp = draw_warp(self.rng, len(params), self.input_shape, self.affine, self.mixup if mixup is None else mixup)
        return self.apply(params, groups, bgroups, fmt=fmt, exact=exact, warp=warp)

    def apply(self, params: List[Dict], sources: List[List[torch.Tensor]], boxes: List[List], fmt="yolo8", exact=True, max_boxes=None, warp=None):
        """Runs the launches for drawn parameters (``draw_params`` results, or hand-made ones of the same form).  ``fmt="padded"`` stops
        after the padded box kernel and returns ``(images, (labels (B, capacity, 5), counts (B)))`` with capacity ``max_boxes``, or
        without it the largest number of source boxes of one image.  ``warp``: a ``draw_warp`` result or hand-made matrices and partners
        (``view_table``); with it stage 1 writes into scratch and the two stage-2 launches write the batch and the targets, without it
        (None) exactly the stage-1 launches run."""
        if fmt not in YOLO_FORMATS + TARGET_FORMATS:
            raise ValueError(fmt)
        spec = self._spec(fmt) if fmt in ("ssd", "centernet") else None
        H, W = self.input_shape
        B = len(params)
        if warp is not None and not self.train:
            raise ValueError("the warp and MixUp are training options")
        views = None if warp is None else view_table(warp, B)
        flat_src = [t for g in sources for t in g]
        if B == 0 or not all(torch.is_tensor(t) and t.is_cuda for t in flat_src):
            raise L.CvxError("DeviceAugmenter takes uint8 pictures in GPU memory (there is no CPU path)")
        dev = flat_src[0].device
        jobs, job_start, box_start, box_rows, keep_alive = [], [0], [0], [], []
        for i, (p, g, bg) in enumerate(zip(params, sources, boxes)):
            if len(p["jobs"]) != len(g) or len(bg) != len(g) or len(g) not in (1, 4):
                raise ValueError("jobs, pictures and box arrays of an output image must pair up (1 or 4 each)")
            for jb, t, b in zip(p["jobs"], g, bg):
                if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or tuple(t.shape[:2]) != (jb["ih"], jb["iw"]) or t.device != dev:
                    raise L.CvxError(f"picture {tuple(t.shape)} {t.dtype} on {t.device} does not fit its job ({jb['ih']}, {jb['iw']}, 3) uint8 on {dev}")
                if jb["nh"] <= 0 or jb["nw"] <= 0 or jb["ih"] <= 0 or jb["iw"] <= 0:
                    raise L.CvxError("augmentation job with an empty picture")
                t = t.contiguous()
                keep_alive.append(t)
                x0, y0, x1, y1 = jb["rect"]
                if not (0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H):
                    raise L.CvxError(f"job rect {jb['rect']} outside the {H} x {W} output")
                jobs.append((t.data_ptr(), jb["ih"], jb["iw"], jb["nh"], jb["nw"], jb["dx"], jb["dy"], int(bool(jb["flip"])), i, x0, y0, x1, y1,
                             jb["quad"], 0))
                b = np.asarray(b, np.float32).reshape(-1, 5)
                box_rows.append(b)
                box_start.append(box_start[-1] + len(b))
            job_start.append(len(jobs))
        J, N = len(jobs), box_start[-1]
        # one pinned blob: jobs | job_start | job_box_start | luts | boxes | views (stage 2 only)
        o_jobs = 0
        o_js = _align(o_jobs + J * 64)
        o_bs = _align(o_js + 4 * (B + 1))
        o_lut = _align(o_bs + 4 * (J + 1))
        o_box = _align(o_lut + 768 * B)
        o_view = _align(o_box + 20 * N)
        total = o_view if views is None else _align(o_view + 96 * B)
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        hv[o_jobs:o_jobs + J * 64].view(JOB_DTYPE)[:] = np.array(jobs, dtype=JOB_DTYPE)
        hv[o_js:o_js + 4 * (B + 1)].view(np.int32)[:] = job_start
        hv[o_bs:o_bs + 4 * (J + 1)].view(np.int32)[:] = box_start
        hv[o_lut:o_lut + 768 * B].reshape(B, 3, 256)[:] = np.stack([np.asarray(p["lut"], np.uint8).reshape(3, 256) for p in params])
        if N:
            hv[o_box:o_box + 20 * N].view(np.float32).reshape(N, 5)[:] = np.concatenate(box_rows, 0)
        if views is not None:
            hv[o_view:o_view + 96 * B].view(VIEW_DTYPE)[:] = views
        blob = torch.empty(total, dtype=torch.uint8, device=dev)
        blob.copy_(host, non_blocking=True)
        self.last_warp = warp
        if views is not None:
            n_src = [box_start[job_start[i + 1]] - box_start[job_start[i]] for i in range(B)]
            return self._apply_warp(fmt, spec, blob, (o_jobs, o_js, o_bs, o_lut, o_box), o_view, views["partner"].tolist(), n_src, N, exact, max_boxes)
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        if fmt in TARGET_FORMATS:
            most = max(box_start[job_start[i + 1]] - box_start[job_start[i]] for i in range(B))
            return out, self._targets(fmt, spec, blob, (o_jobs, o_js, o_bs, o_lut, o_box), B, N, out, most, max_boxes)
        rows = torch.empty(max(N, 1), 6, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        self._launch(blob, (o_jobs, o_js, o_bs, o_lut, o_box), B, J, N, out, rows, count)
        self.last_count = count
        n = int(count.item()) if exact else N
        t = rows[:n]
        if fmt == "yolo7":
            return out, t
        return out, {"batch_idx": t[:, 0], "cls": t[:, 1:2], "bboxes": t[:, 2:6]}

    def _targets(self, fmt, spec, blob, offsets, B, N, out, most_boxes, max_boxes):
        """``fmt="ssd"`` / ``"centernet"`` / ``"padded"``: image launch, padded box launch, target kernel -- nothing is read back"""
        dev = blob.device
        cap = self._capacity(fmt, spec, most_boxes, max_boxes, dev)
        labels = torch.empty(B, cap, 5, dtype=torch.float32, device=dev)
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        overflow = torch.empty(1, dtype=torch.int32, device=dev)
        self._launch_padded(blob, offsets, B, N, out, labels, counts, overflow)
        self.last_count, self.last_overflow = counts, overflow
        return self._finish(fmt, spec, labels, counts)

    def _capacity(self, fmt, spec, most_boxes, max_boxes, dev):
        """rows per image of the padded labels, known on the host; caches SSD's priors on ``dev`` and checks CenterNet's feature size"""
        if fmt == "padded":
            cap = max(most_boxes, 1) if max_boxes is None else int(max_boxes)
        elif fmt == "ssd":
            cap = max(most_boxes, 1)                       # every source box has a row: the padded kernel cannot overflow
            if self._priors is None or self._priors.device != dev:
                self._priors = torch.as_tensor(spec.priors, dtype=torch.float32).to(dev).contiguous()
        else:
            cap = int(spec.max_boxes)
            fh, fw = (int(v) for v in spec.feature_hw)
            ratio = self.input_shape[0] // fh if fh > 0 else 0
            if ratio <= 0 or (self.input_shape[0] // ratio, self.input_shape[1] // ratio) != (fh, fw):
                raise ValueError(f"CenterNet feature size {tuple(spec.feature_hw)} does not belong to a {self.input_shape} input")
        return cap

    def _finish(self, fmt, spec, labels, counts):
        if fmt == "padded":
            return labels, counts
        if fmt == "ssd":
            return _engine.ssd_encode_targets(labels, counts, self._priors, spec.num_classes, spec.overlap_threshold, spec.variances)
        return _engine.centernet_draw_targets(labels, counts, spec.feature_hw, spec.num_classes)

    def _images(self, lib, blob, offsets, B, out, stream):
        H, W = self.input_shape
        base, P = blob.data_ptr(), L.C.c_void_p
        if self.train:
            L.check(lib.cvx_aug_images(P(base + offsets[0]), P(base + offsets[1]), P(base + offsets[3]), B, L.ptr(out), H, W, stream), "cvx_aug_images")
        else:
            L.check(lib.cvx_aug_images_plain(P(base + offsets[0]), P(base + offsets[1]), B, L.ptr(out), H, W, stream), "cvx_aug_images_plain")

    def _launch(self, blob, offsets, B, J, N, out, rows, count):
        """the two launches on the current stream of the blob's device (tools/aug_cost.py times exactly this)"""
        H, W = self.input_shape
        o_jobs, o_js, o_bs, o_lut, o_box = offsets
        base, P, lib = blob.data_ptr(), L.C.c_void_p, L.load()
        with torch.cuda.device(blob.device):
            stream = L.stream_ptr(blob.device)
            self._images(lib, blob, offsets, B, out, stream)
            L.check(lib.cvx_aug_boxes(P(base + o_jobs), P(base + o_bs), J, P(base + o_box), N, H, W, L.ptr(rows), L.ptr(count), stream),
                    "cvx_aug_boxes")

    def _launch_padded(self, blob, offsets, B, N, out, labels, counts, overflow):
        """image launch + ``cvx_aug_boxes_padded`` (labels (B, capacity, 5), counts (B), overflow (1)) on the current stream"""
        H, W = self.input_shape
        o_jobs, o_js, o_bs, o_lut, o_box = offsets
        base, P, lib = blob.data_ptr(), L.C.c_void_p, L.load()
        with torch.cuda.device(blob.device):
            stream = L.stream_ptr(blob.device)
            self._images(lib, blob, offsets, B, out, stream)
            L.check(lib.cvx_aug_boxes_padded(P(base + o_jobs), P(base + o_js), P(base + o_bs), B, P(base + o_box), N, H, W, int(labels.shape[1]),
                                             L.ptr(labels), L.ptr(counts), L.ptr(overflow), stream), "cvx_aug_boxes_padded")

    def _apply_warp(self, fmt, spec, blob, offsets, o_view, partner, n_src, N, exact, max_boxes):
        """Stage 1 into scratch (image launch + ``cvx_aug_boxes_padded`` with a row for every source box, so it cannot overflow), then
        ``cvx_aug_warp_mix`` and ``cvx_aug_boxes_warp``.  Output i can carry the boxes of its canvas and of its partner's, so the
        capacities count both: the compact rows their sum over the batch, SSD the largest pair."""
        dev, B, (H, W) = blob.device, len(n_src), self.input_shape
        pair = [n + (n_src[p] if p >= 0 else 0) for n, p in zip(n_src, partner)]
        canvases = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        labels1 = torch.empty(B, max(max(n_src), 1), 5, dtype=torch.float32, device=dev)
        counts1 = torch.empty(B, dtype=torch.int32, device=dev)
        overflow1 = torch.empty(1, dtype=torch.int32, device=dev)
        self._launch_padded(blob, offsets, B, N, canvases, labels1, counts1, overflow1)
        if fmt in YOLO_FORMATS:
            rows = torch.empty(max(sum(pair), 1), 6, dtype=torch.float32, device=dev)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            self._launch_warp(blob, o_view, canvases, out, labels1, counts1, True, rows, count, None)
            self.last_count = count
            t = rows[:int(count.item()) if exact else sum(pair)]
            if fmt == "yolo7":
                return out, t
            return out, {"batch_idx": t[:, 0], "cls": t[:, 1:2], "bboxes": t[:, 2:6]}
        cap = self._capacity(fmt, spec, max(pair), max_boxes, dev)
        labels = torch.empty(B, cap, 5, dtype=torch.float32, device=dev)
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        overflow = torch.empty(1, dtype=torch.int32, device=dev)
        self._launch_warp(blob, o_view, canvases, out, labels1, counts1, False, labels, counts, overflow)
        self.last_count, self.last_overflow = counts, overflow
        return out, self._finish(fmt, spec, labels, counts)

    def _launch_warp(self, blob, o_view, canvases, out, labels1, counts1, compact, rows, counts, overflow):
        """the two stage-2 launches on the current stream of the blob's device (tools/aug_warp_cost.py times this behind ``_launch_padded``)"""
        H, W = self.input_shape
        c = self.affine or AFFINE_DEFAULTS
        views, lib = L.C.c_void_p(blob.data_ptr() + o_view), L.load()
        with torch.cuda.device(blob.device):
            stream = L.stream_ptr(blob.device)
            L.check(lib.cvx_aug_warp_mix(L.ptr(canvases), views, int(canvases.shape[0]), L.ptr(out), H, W, stream), "cvx_aug_warp_mix")
            L.check(lib.cvx_aug_boxes_warp(L.ptr(labels1), L.ptr(counts1), int(labels1.shape[1]), views, int(canvases.shape[0]), H, W, c["min_wh"],
                                           c["min_area_ratio"], c["max_aspect"], int(compact), L.ptr(rows), int(rows.shape[-2]), L.ptr(counts),
                                           L.ptr(overflow), stream), "cvx_aug_boxes_warp")


class DeviceAugLoader:
    """Iterable of augmented batches over any indexable ``source`` of ``(uint8 HWC image tensor, (n, 5) boxes)``: what ``DetectionDataset`` +
    ``DataLoader`` + the collate function are in the reference, to be passed as ``dataloader=`` / ``val_dataloader=`` to ``Yolo8Trainer``
    (``fmt="yolo8"``), ``Yolo7Trainer`` (``"yolo7"``), ``SsdTrainer`` (``"ssd"``) or ``CenterNetTrainer`` (``"centernet"``; the last two
    with ``DeviceAugmenter(target=...)``).  Pictures that are still on the host are moved to ``device`` first.

    Training (``augmenter.train``): ``length`` batches; items are taken in order, wrapping around; a mosaic item takes three further random
    items and shuffles the four, like mosaic_for_voc (:292-298).  Validation (``DeviceAugmenter(train=False)``): the source is walked once,
    in order; ``drop_last=True`` (the reference's DataLoader setting) leaves out a short last batch, ``drop_last=False`` yields it;
    ``length`` is not needed.

    ``close_after=E`` ("close mosaic", YOLOv8): every ``__iter__`` call is an epoch, counted in ``epoch`` (settable, for a resumed run); from
    epoch ``E`` on no mosaic is asked for and the augmenter is called with ``mixup=0``, while its ``affine`` stays on."""

    def __init__(self, source, batch_size, augmenter: DeviceAugmenter, length: Optional[int] = None, fmt="yolo8", device="cuda", drop_last=True,
                 close_after: Optional[int] = None):
        self.source, self.batch_size, self.augmenter, self.fmt = source, int(batch_size), augmenter, fmt
        self.device, self.drop_last = torch.device(device), bool(drop_last)
        if close_after is not None and (int(close_after) < 0 or not augmenter.train):
            raise ValueError("close_after is a number of training epochs")
        self.close_after = None if close_after is None else int(close_after)
        self.epoch = 0                                   # __iter__ calls so far; settable, for a resumed run
        if fmt not in YOLO_FORMATS + ("ssd", "centernet"):
            raise ValueError(fmt)
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
        image, box = self.source[int(i)]
        return image.to(self.device, non_blocking=True), box

    def __iter__(self):
        """One epoch.  The loader counts these calls in ``epoch``; from epoch ``close_after`` on ("close mosaic", YOLOv8) it asks for no
        mosaic -- ``want_mosaic`` is not called, so its draw is not made -- and passes ``mixup=0``; ``affine`` stays on."""
        closed = self.close_after is not None and self.epoch >= self.close_after
        self.epoch += 1
        return self._batches(closed)

    def _batches(self, closed):
        n, aug = len(self.source), self.augmenter
        if not aug.train:
            for k in range(self.length):
                picked = [self._item(i) for i in range(k * self.batch_size, min((k + 1) * self.batch_size, n))]
                yield aug([p[0] for p in picked], [p[1] for p in picked], fmt=self.fmt)
            return
        item = 0
        for _ in range(self.length):
            images, boxes = [], []
            for _ in range(self.batch_size):
                if not closed and aug.want_mosaic():
                    ids = list(aug.rng.choice(n, 3, replace=n < 3)) + [item % n]
                    aug.rng.shuffle(ids)
                    picked = [self._item(i) for i in ids]
                    images.append([p[0] for p in picked])
                    boxes.append([p[1] for p in picked])
                else:
                    image, box = self._item(item % n)
                    images.append(image)
                    boxes.append(box)
                item += 1
            yield aug(images, boxes, fmt=self.fmt, mixup=0.0 if closed else None)
