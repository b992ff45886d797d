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

    ``train=False`` is the validation path (module docstring): no mosaic, no flip, no colour transform, no random numbers, all four formats."""

    def __init__(self, input_shape, mosaic=False, mosaic_prob=0.5, seed=None, jitter=0.3, hue=0.1, sat=0.7, val=0.4, train=True, target=None):
        self.input_shape = (int(input_shape[0]), int(input_shape[1]))
        self.train = bool(train)
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

    def __call__(self, images, boxes, fmt="yolo8", exact=True):
        groups = [list(e) if isinstance(e, (list, tuple)) else [e] for e in images]
        bgroups = [list(b) if isinstance(b, (list, tuple)) else [b] for b in boxes]
        params = []
        for g, bg in zip(groups, bgroups):
            if len(g) not in (1, 4) or len(bg) != len(g):
                raise ValueError("an output image takes one picture, or four for a mosaic, and as many box arrays")
            params.append(draw_params(self.rng, [tuple(t.shape[:2]) for t in g], self.input_shape, len(g) == 4,
                                      nboxes=[len(np.asarray(b).reshape(-1, 5)) for b in bg], train=self.train, **self.gains))
        return self.apply(params, groups, bgroups, fmt=fmt, exact=exact)

    def apply(self, params: List[Dict], sources: List[List[torch.Tensor]], boxes: List[List], fmt="yolo8", exact=True, max_boxes=None):
        """Runs the launches for drawn parameters (``draw_params`` results, or hand-made ones of the same form).  ``fmt="padded"`` stops
        after the padded box kernel and returns ``(images, (labels (B, capacity, 5), counts (B)))`` with capacity ``max_boxes``, or
        without it the largest number of source boxes of one image."""
        if fmt not in YOLO_FORMATS + TARGET_FORMATS:
            raise ValueError(fmt)
        spec = self._spec(fmt) if fmt in ("ssd", "centernet") else None
        H, W = self.input_shape
        B = len(params)
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
        # one pinned blob: jobs | job_start | job_box_start | luts | boxes
        o_jobs = 0
        o_js = _align(o_jobs + J * 64)
        o_bs = _align(o_js + 4 * (B + 1))
        o_lut = _align(o_bs + 4 * (J + 1))
        o_box = _align(o_lut + 768 * B)
        total = _align(o_box + 20 * N)
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        hv[o_jobs:o_jobs + J * 64].view(JOB_DTYPE)[:] = np.array(jobs, dtype=JOB_DTYPE)
        hv[o_js:o_js + 4 * (B + 1)].view(np.int32)[:] = job_start
        hv[o_bs:o_bs + 4 * (J + 1)].view(np.int32)[:] = box_start
        hv[o_lut:o_lut + 768 * B].reshape(B, 3, 256)[:] = np.stack([np.asarray(p["lut"], np.uint8).reshape(3, 256) for p in params])
        if N:
            hv[o_box:o_box + 20 * N].view(np.float32).reshape(N, 5)[:] = np.concatenate(box_rows, 0)
        blob = torch.empty(total, dtype=torch.uint8, device=dev)
        blob.copy_(host, non_blocking=True)
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
        labels = torch.empty(B, cap, 5, dtype=torch.float32, device=dev)
        counts = torch.empty(B, dtype=torch.int32, device=dev)
        overflow = torch.empty(1, dtype=torch.int32, device=dev)
        self._launch_padded(blob, offsets, B, N, out, labels, counts, overflow)
        self.last_count, self.last_overflow = counts, overflow
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


class DeviceAugLoader:
    """Iterable of augmented batches over any indexable ``source`` of ``(uint8 HWC image tensor, (n, 5) boxes)``: what ``DetectionDataset`` +
    ``DataLoader`` + the collate function are in the reference, to be passed as ``dataloader=`` / ``val_dataloader=`` to ``Yolo8Trainer``
    (``fmt="yolo8"``), ``Yolo7Trainer`` (``"yolo7"``), ``SsdTrainer`` (``"ssd"``) or ``CenterNetTrainer`` (``"centernet"``; the last two
    with ``DeviceAugmenter(target=...)``).  Pictures that are still on the host are moved to ``device`` first.

    Training (``augmenter.train``): ``length`` batches; items are taken in order, wrapping around; a mosaic item takes three further random
    items and shuffles the four, like mosaic_for_voc (:292-298).  Validation (``DeviceAugmenter(train=False)``): the source is walked once,
    in order; ``drop_last=True`` (the reference's DataLoader setting) leaves out a short last batch, ``drop_last=False`` yields it;
    ``length`` is not needed."""

    def __init__(self, source, batch_size, augmenter: DeviceAugmenter, length: Optional[int] = None, fmt="yolo8", device="cuda", drop_last=True):
        self.source, self.batch_size, self.augmenter, self.fmt = source, int(batch_size), augmenter, fmt
        self.device, self.drop_last = torch.device(device), bool(drop_last)
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
                if aug.want_mosaic():
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
            yield aug(images, boxes, fmt=self.fmt)
