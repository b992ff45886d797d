"""Seeded cases and reference glue for the sweeps of the detection eval tail -- ``cvx_nms_variant``, ``cvx_centernet_decode``,
``cvx_yolo7_decode`` -- shared by tests/test_eval_tail_cpu.py (which shows from the references alone that every case has the property it
was built for, and that deliberately wrong restatements change the expected outputs) and tests/test_eval_tail_gpu.py (which runs the
kernels on them).  No GPU dependency.

The references are the project's oracles (oracle/nms_ref.py, oracle/centernet_ref.py, oracle/yolov7_ref.py).  Two front ends are added
where an oracle's entry point does not fit: ``nms_xyxy`` (corner boxes, as the SSD tail feeds ``CVX_NMS_BOXES_XYXY``) and
``centernet_reference`` (CenterNetA.decode_boxes per image, stopped before the letterbox inverse).  ``nms_restated`` and ``peak_map`` /
``topk_restated`` are restatements with switches for the mutants; without a switch they are asserted equal to the oracles.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

from oracle import centernet_ref as C
from oracle import nms_ref, synth
from oracle import yolov7_ref as Y

NMS_CAP = 16384          # candidates per image cvx_nms_variant sorts (csrc/nms.hip); more -> counts = -1
CAND_CAP = 2048          # candidates of one slice cvx_centernet_decode sorts (csrc/centernet_decode.hip); more -> counts = -1
VARIANTS = nms_ref.VARIANTS


# ----------------------------------------------------------------------------------------------------------------------------------------
# NMS
# ----------------------------------------------------------------------------------------------------------------------------------------
@dataclass(eq=False)
class NmsCase:
    name: str
    pred: np.ndarray                 # (B, 4 + nc, A) fp32
    n: tuple                         # candidates per image under the reference's rule (asserted by the generator)
    conf: float = 0.25
    iou: float = 0.7
    max_det: int = 2048
    xyxy: bool = False
    overflow: tuple = ()             # images with more than NMS_CAP candidates: counts = -1, nothing else compared
    borderline: bool = False         # built from pairs at IoU = thr +- 1e-6: exempt from the margin check
    tags: tuple = field(default_factory=tuple)

    def __hash__(self):
        return hash(self.name)


def candidate_counts(pred: np.ndarray, conf: float) -> tuple:
    """ultralytics_ops.py:190 -- best class score > conf, fp32."""
    return tuple(int(v) for v in (pred[:, 4:].max(1) > np.float32(conf)).sum(1))


def clustered(seed: int, a: int, nc: int, n, decimals: int = 2, pick=None) -> np.ndarray:
    """synth.nms_pred's construction (40 clusters of jittered centres, sizes U(20, 200), background scores below 0.2) with exactly n[i]
    candidates planted per image: scores U(0.3, 0.95) rounded to ``decimals`` in one of the first six classes."""
    ns = [n] if isinstance(n, int) else list(n)
    rng = np.random.default_rng(seed)
    pred = np.zeros((len(ns), 4 + nc, a), np.float32)
    centers = rng.uniform(40, 600, size=(len(ns), 40, 2))
    for i, k in enumerate(ns):
        which = rng.integers(0, 40, a)
        pred[i, 0:2] = (centers[i, which] + rng.normal(0, 6, (a, 2))).T
        pred[i, 2:4] = rng.uniform(20, 200, (2, a))
        pred[i, 4:] = rng.uniform(0, 0.2, (nc, a))
        idx = rng.choice(a, k, replace=False) if pick is None else pick(rng, a, k)
        pred[i, 4 + rng.integers(0, min(6, nc), k), idx] = np.round(rng.uniform(0.3, 0.95, k), decimals)
    return pred


def _case(name, pred, n, **kw) -> NmsCase:
    n = (n,) * pred.shape[0] if isinstance(n, int) else tuple(n)
    got = candidate_counts(pred, kw.get("conf", 0.25))
    assert got == n, (name, got, n)
    return NmsCase(name, pred, n, **kw)


# (candidates, anchors, classes): every n at a 64-bit mask-word edge or a power-of-two edge of the bitonic sort; no A a multiple of 64
WORD_EDGES = ((1, 65, 1), (2, 65, 3), (63, 65, 80), (64, 65, 3), (65, 65, 1), (65, 130, 80), (127, 130, 3), (128, 130, 80), (129, 130, 1),
              (1023, 1500, 3), (1024, 1500, 80), (1024, 3000, 3), (1025, 3000, 1))


def _plant_singleton(pred: np.ndarray) -> np.ndarray:
    """One more candidate, class 0, far from every pair of synth.nms_pred_borderline (their boxes start at x >= 20), in the highest
    anchor the generator left unused; it does not move boxes.max()."""
    pred = pred.copy()
    free = np.nonzero(pred[0, 4:].max(0) < 0.1)[0]
    pred[0, 0:4, free[-1]] = (5.0, 5.0, 4.0, 4.0)
    pred[0, 4, free[-1]] = 0.5
    return pred


def _xyxy_pred(seed: int, a: int = 130, nc: int = 3, hot: int = 96) -> np.ndarray:
    """Corner boxes as SSD's decode leaves them: cx -/+ w/2 clipped to [0, 1] in fp32.  Twelve clusters, some centred outside the image,
    plus eight candidates wholly outside it -- clipped to zero area, four of them the very same box -- where IoU is 0 / 0."""
    rng = np.random.default_rng(seed)
    pred = np.zeros((1, 4 + nc, a), np.float32)
    centers = rng.uniform(-0.1, 1.1, (12, 2))
    c = (centers[rng.integers(0, 12, a)] + rng.normal(0, 0.02, (a, 2))).astype(np.float32)
    wh = rng.uniform(0.05, 0.4, (a, 2)).astype(np.float32)
    idx = rng.choice(a, hot, replace=False)
    out = idx[:8]
    c[out[:4]] = (-0.5, 0.5)                  # x1 = x2 = 0, the same rows of y: identical zero-area boxes
    wh[out[:4]] = (0.2, 0.3)
    c[out[4:]] = np.stack((rng.uniform(0.1, 0.9, 4), np.full(4, 1.6)), 1)   # y1 = y2 = 1
    half = wh * np.float32(0.5)
    pred[0, 0:4] = np.clip(np.concatenate((c - half, c + half), 1), 0, 1).T
    pred[0, 4:] = rng.uniform(0, 0.2, (nc, a))
    cls = rng.integers(0, nc, hot)
    cls[:8] = 1
    pred[0, 4 + cls, idx] = np.round(rng.uniform(0.3, 0.95, hot), 2)
    return pred


@functools.lru_cache(maxsize=None)
def nms_cases() -> tuple:
    cases = []
    for k, (n, a, nc) in enumerate(WORD_EDGES):
        cases.append(_case(f"edge_n{n}_a{a}_nc{nc}", clustered(100 + k, a, nc, n), n, tags=("edge",)))
    mixed = (0, 1, 64, 700, 65)
    cases.append(_case("mixed_batch", clustered(120, 1500, 3, mixed), mixed, tags=("mixed",)))
    for a, pairs in ((2048, 500), (10240, 2500)):
        p = synth.nms_pred_borderline(3, a=a, pairs=pairs)
        cases.append(_case(f"switch_n{2 * pairs}", p, 2 * pairs, max_det=4096, borderline=True, tags=("switch",)))
        cases.append(_case(f"switch_n{2 * pairs + 1}", _plant_singleton(p), 2 * pairs + 1, max_det=4096, borderline=True, tags=("switch",)))
    cases.append(_case("mass_ties", clustered(130, 1500, 3, 900, decimals=1), 900, tags=("ties",)))
    base = clustered(140, 1500, 3, 700)
    s = len(nms_ref.non_max_suppression(base, 0.25, 0.7, NMS_CAP, variant="vanilla")[0][1])
    for md in (1, 7, s - 1, s, s + 1):
        cases.append(_case(f"max_det_{md}_of_{s}", base, 700, max_det=md, tags=("max_det",)))
    small = clustered(150, 130, 3, 100)
    i0, i1 = np.nonzero(small[0, 4:].max(0) > 0.25)[0][:2]         # one exact duplicate, same class, lower score: IoU == 1 exactly
    small[0, :, i1] = small[0, :, i0]
    small[0, 4 + small[0, 4:, i0].argmax(), i1] = 0.29
    cases.append(_case("iou_thres_0", small, 100, iou=0.0, tags=("ends",)))
    cases.append(_case("iou_thres_1", small, 100, iou=1.0, tags=("ends",)))
    z = clustered(151, 130, 3, 60)
    z[0, 4:, ::3] = 0.0                                            # exact zeros: not candidates even at conf 0
    cases.append(_case("conf_thres_0", z, int((z[0, 4:].max(0) > 0).sum()), conf=0.0, tags=("ends",)))
    cases.append(_case("xyxy_clipped", _xyxy_pred(160), 96, xyxy=True, tags=("xyxy",)))

    def high(rng, a, k):                                           # nine in ten above anchor 16384
        lo = k // 10
        return np.concatenate((rng.choice(NMS_CAP, lo, replace=False), NMS_CAP + rng.choice(a - NMS_CAP, k - lo, replace=False)))

    cases.append(_case("large_a_25200", clustered(170, 25200, 3, 500, pick=high), 500, tags=("large",)))
    over = clustered(171, 16500, 1, (0, 300))
    over[0, 4] = np.random.default_rng(172).uniform(0.3, 0.9, 16500)   # every anchor of image 0 a candidate: 16500 > NMS_CAP
    cases.append(_case("large_a_overflow", over, (16500, 300), overflow=(0,), tags=("large",)))
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def nms_case(name: str) -> NmsCase:
    return next(c for c in nms_cases() if c.name == name)


def _candidates(x: np.ndarray, conf: float, xyxy: bool, tie_desc: bool = False):
    """Candidate rule and order of ultralytics_ops.py:190-240 as oracle/nms_ref.non_max_suppression states them: (score desc, anchor asc)."""
    scores = x[4:]
    best = scores.max(0)
    cand = np.nonzero(best > np.float32(conf))[0]
    box = x[:4, cand].T.astype(np.float32) if xyxy else nms_ref.xywh2xyxy(x[:4, cand].T)
    sc, cls = best[cand], scores[:, cand].argmax(0)
    order = np.lexsort((-cand if tie_desc else cand, -sc.astype(np.float64)))
    return box[order], sc[order], cls[order], cand[order]


def _rows(box, sc, cls, cand, keep):
    rows = np.concatenate((box[keep], sc[keep, None], cls[keep, None].astype(np.float32)), 1).astype(np.float32).reshape(-1, 6)
    return rows, cand[keep].astype(np.int64)


def nms_xyxy(pred: np.ndarray, conf: float, iou: float, max_det: int, variant: str):
    """oracle/nms_ref.non_max_suppression for rows 0..3 that already hold corners: same candidate rule, same order, same batched_nms."""
    out = []
    for x in np.asarray(pred, np.float32):
        box, sc, cls, cand = _candidates(x, conf, True)
        out.append(_rows(box, sc, cls, cand, nms_ref.batched_nms(box, cls, iou, variant)[:max_det]))
    return out


@functools.lru_cache(maxsize=None)
def nms_reference(case: NmsCase, variant: str) -> tuple:
    """Per image (rows (k, 6), anchor indices (k,)) from the oracle; None for an image of ``case.overflow``."""
    fn = nms_xyxy if case.xyxy else (lambda p, c, i, m, variant: nms_ref.non_max_suppression(p, c, i, m, variant=variant))
    return tuple(None if b in case.overflow else fn(case.pred[b:b + 1], case.conf, case.iou, case.max_det, variant)[0]
                 for b in range(case.pred.shape[0]))


def _greedy_restated(boxes, same, thr, ge=False, word_exempt=False):
    """oracle/nms_ref._greedy with two switches: ``>=`` in the suppression test; position 0 of every 64-box word never suppressed."""
    n = boxes.shape[0]
    x1, y1, x2, y2 = (boxes[:, i].astype(np.float32) for i in range(4))
    area = (x2 - x1) * (y2 - y1)
    thr = np.float32(thr)
    dead = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        j = np.arange(i + 1, n)
        j = j[~dead[j]] if same is None else j[(~dead[j]) & (same[j] == same[i])]
        if word_exempt:
            j = j[j % 64 != 0]
        if j.size == 0:
            continue
        w = np.maximum(np.float32(0), np.minimum(x2[i], x2[j]) - np.maximum(x1[i], x1[j]))
        h = np.maximum(np.float32(0), np.minimum(y2[i], y2[j]) - np.maximum(y1[i], y1[j]))
        inter = w * h
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / (area[i] + area[j] - inter)
        dead[j[(ovr >= thr) if ge else (ovr > thr)]] = True
    return np.asarray(keep, dtype=np.int64)


def nms_restated(case: NmsCase, variant: str, tie_desc=False, ge=False, word_exempt=False, switch_shift=0, max_det_shift=0) -> tuple:
    """The whole NMS tail restated in one place.  Without a switch it equals ``nms_reference`` (asserted in test_eval_tail_cpu.py); each
    switch is one way a kernel could be subtly wrong."""
    out = []
    for b, x in enumerate(case.pred):
        if b in case.overflow:
            out.append(None)
            continue
        box, sc, cls, cand = _candidates(x, case.conf, case.xyxy, tie_desc)
        mode = variant
        if variant.startswith("tv0141"):
            limit = (5000 if variant.endswith("cuda") else 1000) + switch_shift      # boxes.numel() > 20000 / 4000
            mode = "vanilla" if box.shape[0] > limit else "offset"
        if box.shape[0] == 0:
            keep = np.zeros((0,), np.int64)
        elif mode == "vanilla":
            keep = _greedy_restated(box, cls, case.iou, ge, word_exempt)
        else:
            off = cls.astype(np.float32) * (box.max() + np.float32(1))
            keep = _greedy_restated(box + off[:, None], None, case.iou, ge, word_exempt)
        out.append(_rows(box, sc, cls, cand, keep[:max(case.max_det + max_det_shift, 0)]))
    return tuple(out)


def same_nms(a, b) -> bool:
    return all((p is None and q is None) or (p is not None and q is not None and np.array_equal(p[1], q[1]) and np.array_equal(p[0], q[0]))
               for p, q in zip(a, b))


def nms_iou_margin(case: NmsCase) -> float:
    """Smallest |IoU - iou_thres| (fp64 on the fp32 corners) over the same-class candidate pairs of the compared images.  A pair that sits
    exactly on a threshold of 0 (disjoint boxes) or 1 (identical boxes) is not counted: both sides get exactly that value."""
    worst = np.inf
    for b, x in enumerate(case.pred):
        if b in case.overflow:
            continue
        box, _, cls, _ = _candidates(x, case.conf, case.xyxy)
        box = box.astype(np.float64)
        area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
        for c in np.unique(cls):
            bx, ar = box[cls == c], area[cls == c]
            w = np.maximum(0, np.minimum(bx[:, None, 2], bx[None, :, 2]) - np.maximum(bx[:, None, 0], bx[None, :, 0]))
            h = np.maximum(0, np.minimum(bx[:, None, 3], bx[None, :, 3]) - np.maximum(bx[:, None, 1], bx[None, :, 1]))
            inter = w * h
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = inter / (ar[:, None] + ar[None, :] - inter)
            d = np.abs(iou - case.iou)[np.triu_indices(len(bx), 1)]
            d = d[np.isfinite(d)]
            if case.iou in (0.0, 1.0):
                d = d[d != 0]
            if d.size:
                worst = min(worst, float(d.min()))
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------------
# CenterNet decode
# ----------------------------------------------------------------------------------------------------------------------------------------
@dataclass(eq=False)
class CnCase:
    name: str
    H: int
    W: int
    nc: int
    K: int
    s: int                           # logits are integers in [-6 s, 3 s] divided by s
    seed: int
    B: int = 3
    conf: float = 0.3
    nms_thr: float = 0.5
    use_nms: bool = True
    slack: bool = False              # rows [logits | NaN | offsets | NaN | sizes | NaN]: pred_ld = nc + 7, reg_col = nc + 1, wh_col = nc + 4
    saturated: bool = False
    overflow: tuple = ()
    boundary_tie: bool = False       # more peaks tie at the K-th score than the list has room for

    def __hash__(self):
        return hash(self.name)

    @property
    def cols(self):
        return (self.nc + 7, self.nc + 1, self.nc + 4) if self.slack else (self.nc + 4, self.nc, self.nc + 2)


CN_SHAPES = (  # H, W, nc, K, s, seed, boundary tie
    (12, 12, 7, 100, 4, 200, True),    # per = 63: every slice starts misaligned
    (9, 13, 3, 256, 4, 201, False),    # S = 8, K at its maximum, fewer than K peaks
    (5, 5, 4, 100, 4, 202, False),     # N = K: per = 7, slices 15 is empty, 14 holds two scores
    (32, 32, 80, 100, 8, 204, True),    # the aligned path; a thousand peaks tie at the top score
    (17, 19, 20, 37, 16, 203, True),
    (1, 40, 3, 50, 4, 205, False),
    (23, 1, 5, 64, 4, 206, False),
    (8, 8, 1, 10, 4, 210, True),
    (16, 16, 5, 1, 4, 201, True),
)


@functools.lru_cache(maxsize=None)
def centernet_cases() -> tuple:
    cases = [CnCase(f"cn_{h}x{w}x{nc}_k{k}", h, w, nc, k, s, seed, boundary_tie=t) for h, w, nc, k, s, seed, t in CN_SHAPES]
    cases += [
        CnCase("cn_saturated", 12, 12, 7, 100, 4, 220, saturated=True),
        CnCase("cn_saturated_aligned", 32, 32, 80, 100, 16, 221, saturated=True),
        CnCase("cn_row_stride", 12, 12, 7, 100, 8, 222, slack=True),
        CnCase("cn_row_stride_k256", 9, 13, 3, 256, 4, 223, slack=True),
        CnCase("cn_no_nms", 17, 19, 20, 37, 8, 224, use_nms=False),
        CnCase("cn_conf_0.6", 12, 12, 7, 100, 16, 225, conf=0.6),
        CnCase("cn_conf_0.6_aligned", 32, 32, 80, 100, 8, 226, conf=0.6),
        CnCase("cn_overflow", 64, 64, 20, 100, 8, 227, B=2, overflow=(0,)),
    ]
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def centernet_pred(case: CnCase) -> torch.Tensor:
    """Compact head tensor (B, H*W, nc + 4) = [logits | centre offsets | sizes], the layout the reference's decode_boxes reads."""
    g = torch.Generator().manual_seed(case.seed)
    hw = case.H * case.W
    logits = torch.randint(-6 * case.s, 3 * case.s + 1, (case.B, hw, case.nc), generator=g).float() / case.s
    if case.saturated:                                   # sigmoid == 1.0 exactly on both sides: ties through the sigmoid
        flat = logits.view(case.B, -1)
        for b in range(case.B):
            at = torch.randperm(flat.shape[1], generator=g)[:36]
            flat[b, at] = torch.tensor([20.0, 25.0, 30.0])[torch.randint(0, 3, (36,), generator=g)]
    for b in case.overflow:
        logits[b] = 0.5
    off = torch.rand(case.B, hw, 2, generator=g)
    size = (torch.rand(case.B, hw, 2, generator=g) * 0.45 + 0.05) * torch.tensor([float(case.W), float(case.H)])
    return torch.cat((logits, off, size), 2)


def centernet_device_input(case: CnCase) -> torch.Tensor:
    """The tensor the kernel gets: the compact one, or with NaN slack columns between and behind the three groups."""
    p = centernet_pred(case)
    if not case.slack:
        return p
    nan = torch.full((case.B, p.shape[1], 1), float("nan"))
    nc = case.nc
    return torch.cat((p[..., :nc], nan, p[..., nc:nc + 2], nan, p[..., nc + 2:], nan), 2)


def slices_for(K: int) -> int:
    S = 16
    while S > 1 and S * K > CAND_CAP:
        S >>= 1
    return S


def peak_map(pred: torch.Tensor, H: int, W: int, nc: int, window: str = "xc") -> torch.Tensor:
    """(B, H*W*nc) scores with every non-peak zeroed.  'xc' is the reference's window (centernet.py:279-280: the NHWC tensor pooled as if
    it were NCHW, so 3 x 3 over (x, class)); 'yx' is the window a reader would expect -- the mutant."""
    heat = torch.sigmoid(pred[..., :nc]).reshape(-1, H, W, nc)
    if window == "xc":
        hmax = F.max_pool2d(heat, 3, 1, 1)
    else:
        hmax = F.max_pool2d(heat.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)
    return (heat * (heat == hmax).float()).reshape(heat.shape[0], -1)


def topk_restated(flat: torch.Tensor, K: int, tie_desc: bool = False, per_slice: bool = False) -> torch.Tensor:
    """Top-K flat indices of one image's peak map, (score desc, index asc).  Switches: ties by descending index; the per-slice lists
    of the kernel's first stage concatenated in slice order without the merging sort."""
    N = flat.numel()
    if tie_desc:
        return (N - 1 - torch.sort(flat.flip(0), descending=True, stable=True).indices)[:K]
    if not per_slice:
        return torch.sort(flat, descending=True, stable=True).indices[:K]
    S = slices_for(K)
    per = (N + S - 1) // S
    parts = [i0 + torch.sort(flat[i0:i0 + per], descending=True, stable=True).indices[:K] for i0 in range(0, N, per)]
    return torch.cat(parts)[:K]


@functools.lru_cache(maxsize=None)
def centernet_reference(case: CnCase) -> tuple:
    """CenterNetA.decode_boxes (centernet.py:271-311) image by image up to -- not including -- the letterbox inverse, from the oracle's
    suppress_and_topk / diou_nms: per image dict(index, classes, scores (K,), boxes (K, 4) normalised xyxy, mask = score >= conf,
    keep = positions in the list of the DIoU-NMS survivors)."""
    pred, H, W, nc, K = centernet_pred(case), case.H, case.W, case.nc, case.K
    out = []
    for b in range(case.B):
        if b in case.overflow:
            out.append(None)
            continue
        p = pred[b:b + 1].reshape(1, H, W, nc + 4)
        scores, inds = C.suppress_and_topk(p, nc, K)
        cls = inds % nc
        pixel = torch.div(inds, nc, rounding_mode="floor")
        ys, xs = torch.div(pixel, W, rounding_mode="floor"), pixel % W
        feat = p.reshape(1, H * W, nc + 4)
        pix = (ys * W + xs).long().unsqueeze(2).expand(-1, -1, 2)
        reg, wh = feat[..., nc:nc + 2].gather(1, pix), feat[..., nc + 2:].gather(1, pix)
        bb = torch.cat(((xs.float() + reg[..., 0]).unsqueeze(-1), (ys.float() + reg[..., 1]).unsqueeze(-1), wh), -1)
        bb[..., ::2] /= W
        bb[..., 1::2] /= H
        bb = torch.clamp(bb, min=0, max=1)
        bb = torch.cat((bb[..., 0:1] - bb[..., 2:3] / 2, bb[..., 1:2] - bb[..., 3:4] / 2, bb[..., 0:1] + bb[..., 2:3] / 2,
                        bb[..., 1:2] + bb[..., 3:4] / 2), -1)
        mask = scores[0] >= case.conf
        pos = torch.nonzero(mask).flatten()
        if case.use_nms and pos.numel():
            pos = pos[C.diou_nms(bb[0][mask], scores[0][mask], case.nms_thr)]
        out.append(dict(index=inds[0], classes=cls[0], scores=scores[0], boxes=bb[0], mask=mask, keep=pos))
    return tuple(out)


def centernet_tie_stats(case: CnCase, b: int) -> dict:
    """From the reference's peak map of image b: peaks tied at the K-th score, how many of them the list holds, the slices (of the kernel's
    first stage) they lie in, repeated scores inside the list, and the most candidates (score >= the slice's own K-th, zeros never) any
    slice hands to its sort."""
    flat = peak_map(centernet_pred(case)[b:b + 1], case.H, case.W, case.nc)[0]
    N, K = flat.numel(), case.K
    order = torch.sort(flat, descending=True, stable=True).indices[:K]
    top = flat[order]
    kth = float(top[-1])
    tied = torch.nonzero(flat == kth).flatten()
    S = slices_for(K)
    per = (N + S - 1) // S
    most = 0
    for i0 in range(0, N, per):
        sl = flat[i0:i0 + per]
        nz = torch.sort(sl[sl > 0], descending=True).values
        if nz.numel():
            most = max(most, int((sl >= nz[min(K, nz.numel()) - 1]).sum()))
    return dict(kth=kth, n_tie=int(tied.numel()), n_inside=int((top == kth).sum()), slices=sorted(set((tied // per).tolist())),
                repeats=int((top[1:] == top[:-1]).logical_and(top[1:] > 0).sum()), nonzero=int((top > 0).sum()), most_per_slice=most,
                per=per, S=S)


def centernet_diou_margin(case: CnCase) -> float:
    """Smallest |DIoU - nms_thr| (fp64 on the fp32 boxes) over the pairs of boxes that pass the score mask."""
    worst = np.inf
    for r in centernet_reference(case):
        if r is None:
            continue
        bx = r["boxes"][r["mask"]].double()
        if bx.shape[0] > 1:
            d = (C.box_diou(bx[:, None, :], bx[None, :, :]) - case.nms_thr).abs()
            worst = min(worst, float(d[torch.triu(torch.ones_like(d), 1) > 0].min()))
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------------
# YOLOv7 anchor decode
# ----------------------------------------------------------------------------------------------------------------------------------------
Y7_LEVELS = ((2, 2), (3, 4), (5, 7))          # coarsest first, as the engine orders its head rows
Y7_INPUT_HW = (160, 224)
Y7_NC = (1, 20, 59, 60, 80)                   # 6, 25, 64, 65, 85 attributes: below, at and above one wave per anchor
Y7_B = 3
Y7_ANCHORS = [[tuple(float(v) for v in np.asarray(Y.ANCHORS, np.float32).reshape(-1, 2)[i]) for i in mask] for mask in Y.ANCHORS_MASK]


@functools.lru_cache(maxsize=None)
def yolo7_case(nc: int, slack: int):
    """-> (the three NCHW head outputs oracle/yolov7_ref.decode takes, the engine's rows (B, sum h*w, 3 (5 + nc) + slack) with NaN in the
    slack columns, the oracle's decode)."""
    g = torch.Generator().manual_seed(300 + nc)
    preds = tuple(torch.randn(Y7_B, 3 * (5 + nc), h, w, generator=g) * 3 for h, w in Y7_LEVELS)
    rows = torch.cat([p.permute(0, 2, 3, 1).reshape(Y7_B, h * w, -1) for p, (h, w) in zip(preds, Y7_LEVELS)], 1)
    if slack:
        rows = torch.cat((rows, torch.full((Y7_B, rows.shape[1], slack), float("nan"))), 2)
    return preds, rows.contiguous(), Y.decode(preds, nc, Y7_INPUT_HW)
