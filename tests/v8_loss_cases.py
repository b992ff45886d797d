"""Seeded cases and reference glue for the sweep of the YOLOv8 loss chain (csrc/loss_v8.hip: task-aligned assigner, CIoU, DFL, BCE), shared
by tests/test_v8_loss_sweep_cpu.py (which shows from the oracle alone that every case has the property it was built for, that the discrete
decisions of the assigner keep clear of float32 round-off, and that deliberately wrong restatements change the expected outputs) and
tests/test_v8_loss_sweep_gpu.py (which runs ``V8LossOp`` on them).  No GPU dependency.

The reference is the project's oracle (oracle/yolov8_ref.py) in float64.  ``v8_forward`` restates the assigner and the loss per TARGET ROW,
as the kernel organises them, with switches for the mutants; without a switch it is asserted equal to the oracle.

Predictions.  ``randn`` predictions give noise boxes: a handful of foreground anchors and a score sum of about 1.  ``v8_inputs`` builds the
DFL logits of every anchor from the two-bin construction (log(1 - f), log(f) on the two bins around a distance) aimed at a jittered ground
truth that covers the anchor, over a seeded floor of about -7 on the other bins, and raises the class logit of a covering ground truth on
about 60 % of the covered anchors.  Metrics then spread over (0, 1), far more than ten anchors compete for most ground truths and the
score sum is well above 1 (``low_score`` is built to stay below).

The filler rule.  Where a ground truth has fewer than ten anchors with a positive metric, the reference's ``torch.topk`` fills the ten
with zero-metric anchors, and which ones is unspecified.  A filler inside the box becomes a zero-weight foreground anchor; if another
ground truth claims it too, the overlap arg-max over ALL ground truths decides, which can hand the anchor to a third one.  The kernel never
selects a zero metric.  ``fillers="none"`` is that rule and the expected output of every case; ``fillers="topk"`` asks ``torch.topk`` and
reproduces the oracle.  The CPU test names the cases in which the two differ and asserts the difference itself.

Margins.  The assigner takes four kinds of discrete decision: inside-the-box (``dmin > 1e-9``), positive against zero metric (the clamp
of the CIoU at 0, and float32 underflow of iou^6), the tenth against the eleventh metric of a ground truth, and the two largest overlaps
of an anchor several ground truths claim.  ``v8_margins`` runs the restatement in float32 and float64 and reports how far each decision is
from flipping and the largest float32-vs-float64 difference of the same quantity.  A case is admissible when both precisions assign
identically and every margin is at least MARGIN_FACTOR times that difference.  Exact ties in both precisions are decided by rule, not by
rounding, so they are excluded from the margins and counted: an anchor centre exactly on an edge (``dmin == 0``: outside) and the equal
overlaps of duplicate rows (the lower row wins).
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import yolov8_ref as O

REG = O.REG_MAX
MARGIN_FACTOR = 100.0
GAINS = (7.5, 0.5, 1.5)
MIN_POSITIVE_METRIC = 1e-34      # four orders above the smallest normal float32; no factor of sqrt(score) * iou^6 is smaller than the product
ITEM_RTOL = 2e-5                 # the GPU bounds (tests/test_v8_loss_sweep_gpu.py)
GRAD_BOUND = 5e-4
FP16_FLOOR = 2.5e-4


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@dataclass(frozen=True)
class V8Case:
    name: str
    seed: int
    B: int
    hw: tuple                        # input height, width
    strides: tuple = (8, 16, 32)
    nc: int = 80
    ld: int = 0                      # row pitch of the padded prediction buffer; 0: rows of exactly 64 + nc values
    scale: float = 256.0             # loss scale of the GPU run: the first 256 * (1 + k / 32) at which v8_fp16_floor(...) stays below 2.4e-4
    jitter: float = 0.35

    @property
    def levels(self):
        return tuple((self.hw[0] // s, self.hw[1] // s) for s in self.strides)

    @property
    def A(self):
        return sum(h * w for h, w in self.levels)

    @property
    def no(self):
        return 4 * REG + self.nc

    def anchors(self, dtype=torch.float64):
        pts, st = O.make_anchors(list(self.levels), [float(s) for s in self.strides])
        return pts.to(dtype), st.to(dtype)

    def level_slices(self):
        out, off = [], 0
        for h, w in self.levels:
            out.append(slice(off, off + h * w))
            off += h * w
        return out


# the seeds are the first (from 0) at which the case has its property (tests/test_v8_loss_sweep_cpu.py) and v8_margins(...) is admissible
V8_CASES = (
    V8Case("crowd", 1, 3, (128, 128), scale=264.0),
    V8Case("duplicates", 3, 2, (64, 64)),
    V8Case("edge_on", 0, 1, (128, 128)),
    V8Case("tiny", 0, 2, (128, 128), scale=264.0),
    V8Case("fillers", 1, 1, (128, 128)),
    V8Case("huge", 0, 1, (256, 256)),
    V8Case("nonsquare", 0, 2, (96, 160), nc=20, ld=88, scale=272.0),
    V8Case("saturated", 0, 2, (64, 64), scale=264.0),
    V8Case("low_score", 1, 1, (64, 64), jitter=0.7, scale=328.0),
    V8Case("levels1", 0, 2, (64, 64), strides=(8,)),
    V8Case("levels2", 0, 2, (64, 64), strides=(8, 16), scale=264.0),
    V8Case("levels4", 1, 2, (128, 128), strides=(8, 16, 32, 64), scale=360.0),
    V8Case("nc1", 0, 2, (64, 64), nc=1, ld=68, scale=272.0),
    V8Case("nc3", 0, 2, (64, 64), nc=3, scale=272.0),
    V8Case("empty", 0, 2, (64, 64)),
)
V8_NAMES = tuple(c.name for c in V8_CASES)


def v8_case(name) -> V8Case:
    return next(c for c in V8_CASES if c.name == name)


# ----------------------------------------------------------------------------------------------------------------------------------------
# targets: rows [image, class, cx, cy, w, h], normalised, in the order the case wants them handed over
# ----------------------------------------------------------------------------------------------------------------------------------------
def _boxes(g, n, b, nc, lo=0.16, hi=0.40, c_lo=0.08, c_hi=0.92):
    t = torch.zeros(n, 6)
    t[:, 0] = b
    t[:, 1] = torch.randint(0, nc, (n,), generator=g).float()
    t[:, 2:4] = torch.rand(n, 2, generator=g) * (c_hi - c_lo) + c_lo
    t[:, 4:6] = torch.rand(n, 2, generator=g) * (hi - lo) + lo
    return t


def _px(c, rows):
    """rows [image, class, x1, y1, x2, y2] in pixels -> normalised cxcywh rows; exact where the pixels are dyadic"""
    H, W = c.hw
    t = torch.tensor(rows, dtype=torch.float64)
    out = torch.zeros(len(rows), 6, dtype=torch.float64)
    out[:, :2] = t[:, :2]
    out[:, 2], out[:, 3] = (t[:, 2] + t[:, 4]) / 2 / W, (t[:, 3] + t[:, 5]) / 2 / H
    out[:, 4], out[:, 5] = (t[:, 4] - t[:, 2]) / W, (t[:, 5] - t[:, 3]) / H
    assert torch.equal(out.float().double(), out)
    return out.float()


def _t_crowd(c, g):
    t = torch.cat((_boxes(g, 40, 0, c.nc), _boxes(g, 25, 2, c.nc)))
    return t[torch.randperm(65, generator=g)]                           # interleaved by image, image 1 empty


def _t_duplicates(c, g):
    a, b = _boxes(g, 3, 0, c.nc, 0.3, 0.6, 0.3, 0.7), _boxes(g, 3, 1, c.nc, 0.3, 0.6, 0.3, 0.7)
    dup_same = a[0].clone()                                            # image 0: row 0 again, same class, one row in between
    dup_other = b[1].clone()                                           # image 1: row 1 again, another class, directly behind it
    dup_other[1] = (b[1, 1] + 1) % c.nc
    return torch.cat((a[:2], dup_same[None], a[2:], b[:2], dup_other[None], b[2:]))


def _t_edge_on(c, g):
    # 128 x 128: anchor centres at 4 + 8 k (stride 8), 8 + 16 k (stride 16), 16 + 32 k (stride 32); every number is dyadic
    return _px(c, [
        [0, 3, 12, 8, 48, 60],                       # x1 through stride-8 centres, y1 stride 16, x2 stride 32, y2 stride 8
        [0, 7, 16, 16, 80, 112],                     # all four edges through stride-32 centres (and x1 = y1 = 16 ... )
        [0, 1, 40, 24, 100, 72],                     # stride-16 centres on x1, y1 and y2; stride 8 on x2
        [0, 9, -20, -20, 20, 20],                    # corner sum exactly 0: not a ground truth, though it holds anchor centres
        [0, 2, -10, 30, 30, 70.5],                   # crossing the left border
        [0, 4, 100.5, 50, 140, 90.25],               # the right
        [0, 5, 40.25, -12, 90, 20.5],                # the top
        [0, 6, 50, 100.75, 90.5, 150],               # the bottom
    ])


def _t_tiny(c, g):
    rows = []
    for b in range(c.B):
        rows += [
            [b, 1 + b, 9, 9, 11.5, 11.5],                          # between the centres: no anchor
            [b, 3, 33, 33, 39, 39],                                # one stride-8 centre (36, 36)
            [b, 4, 66, 2, 78, 14],                                 # 4 stride-8 centres and 1 stride-16 centre
            [b, 5, 90, 40, 106, 62],                               # 2 x 3 stride-8 centres, 1 stride-16 centre
            [b, 6, 2.5, 60, 22, 78],                               # 3 x 2 (y = 60 is the edge itself), 1 stride-16 centre
        ]
    t = _px(c, rows)
    return torch.cat((t, _boxes(g, 2, 0, c.nc, 0.25, 0.45), _boxes(g, 2, 1, c.nc, 0.25, 0.45)))


def _t_fillers(c, g):
    # two strips along the bottom edge on the left -- where this build's torch.topk happens to look for its fillers when A = 336 (anchors
    # 212 .. 231: the stride-8 rows y = 108 and y = 116) -- under two large boxes that most of the strips' anchors aim at (AIM_WEIGHT)
    return _px(c, [
        [0, 1, 0, 108.5, 64.25, 128],                                # 8 x 2 stride-8 centres, 4 stride-16 centres
        [0, 2, 0.5, 100.25, 40, 122.5],                              # 5 x 2 stride-8 centres, 2 x 1 stride-16 centres, (16, 112)
        [0, 3, -4, 10, 100, 130],
        [0, 4, -3.5, 5, 104.5, 131.5],
        [0, 5, 60.5, 10.25, 120, 70],
    ])


AIM_WEIGHT = {"fillers": (0.2, 0.2, 1.0, 1.0, 1.0)}                   # per row: how readily an anchor inside aims its box at it
# per level: the share of covered anchors with a raised class logit.  A stride-8 anchor reaches 15 cells to each side, an overlap of at
# most 0.88 with the whole image, so it enters the ten only where few of the coarser anchors (which can match the box) score well.
RAISE_SHARE = {"huge": (0.6, 0.08, 0.08)}


def _t_huge(c, g):
    return torch.cat((_px(c, [[0, 11, 0, 0, 256, 256]]), _boxes(g, 2, 0, c.nc, 0.2, 0.5)))


def _t_random(n, lo=0.2, hi=0.6):
    def f(c, g):
        t = torch.cat([_boxes(g, n, b, c.nc, lo, hi) for b in range(c.B)])
        return t[torch.randperm(t.shape[0], generator=g)]
    return f


MICRO_ANCHOR = 64 + 16            # low_score: the stride-32 anchor with its centre at (16, 16) px = (0.5, 0.5) cells
MICRO_W = 2.0 ** -14             # cells: the width of the micro box (2^-9 px); its height is twice that


def _t_low_score(c, g):
    # a handful of anchors inside: their normalised scores add up to < 1.  And a box of 6e-5 x 1.2e-4 cells around one stride-32 centre:
    # eps = 1e-7 is 1 / 600 of its width, so whether the CIoU adds it to the widths as well as the heights shows in that anchor's
    # gradient -- the only foreground anchor of its level, hence a gradient group of its own.  All its numbers are dyadic (exact in float32).
    t = _boxes(g, 1, 0, c.nc, 0.2, 0.3, 0.3, 0.7)
    w, h = MICRO_W * 32, 2 * MICRO_W * 32
    return torch.cat((t, _px(c, [[0, 7, 16 - w / 2, 16 - h / 2, 16 + w / 2, 16 + h / 2]])))


def _micro(c, g, pred):
    """the micro box's anchor predicts a box 5 times as wide and 1.5 times as high around it (pure two-bin rows: a floor of e^-7 on the
    other bins would move the expectation by a thousand box widths), with its class raised.  The distances are 5 and 3 times 2^-15
    cells, so that 0.5 -+ distance is a float32: the kernel's corners do not carry a rounding of 3e-8 on a width of 3e-4.  The overlap is
    small (0.1) but the gradient is that of an ordinary anchor: every derivative of the CIoU grows as the boxes shrink."""
    d = torch.tensor([5.0, 3.0, 5.0, 3.0], dtype=torch.float64) * 2.0 ** -15
    pred[0, MICRO_ANCHOR, :4 * REG] = _two_bin(d, torch.full((4, REG), -80.0, dtype=torch.float64)).reshape(-1)
    pred[0, MICRO_ANCHOR, 4 * REG + 7] = 2.0
    return pred


def _t_nc(c, g):
    t = _t_random(4)(c, g)
    t[0, 1] = -1.0                                                     # a label below the range: clamped to class 0
    return t


def _t_empty(c, g):
    return torch.zeros(0, 6)


V8_BUILDERS = {"crowd": _t_crowd, "duplicates": _t_duplicates, "edge_on": _t_edge_on, "tiny": _t_tiny, "fillers": _t_fillers, "huge": _t_huge,
               "nonsquare": _t_random(6, 0.15, 0.5), "saturated": _t_random(4), "low_score": _t_low_score, "levels1": _t_random(4),
               "levels2": _t_random(4), "levels4": _t_random(5, 0.2, 0.8), "nc1": _t_nc, "nc3": _t_nc, "empty": _t_empty}


# ----------------------------------------------------------------------------------------------------------------------------------------
# predictions
# ----------------------------------------------------------------------------------------------------------------------------------------
def _two_bin(d, floor):
    """(…) distances in [0, 15) -> (…, 16) logits: `floor` everywhere, log(1 - f) and log(f) on the two bins around d"""
    lo = d.floor()
    f = d - lo
    out = floor.clone()
    out.scatter_(-1, lo.long().unsqueeze(-1), torch.log1p(-f).unsqueeze(-1).clamp_min(-80.0))
    out.scatter_(-1, (lo.long() + 1).unsqueeze(-1), torch.log(f.clamp_min(1e-30)).unsqueeze(-1).clamp_min(-80.0))
    return out


def _predictions(c: V8Case, g, t):
    B, A, nc = c.B, c.A, c.nc
    anc, st = c.anchors()
    px = anc * st                                                       # (A, 2) pixels
    H, W = c.hw
    box = torch.zeros(B, A, 4, REG, dtype=torch.float64)
    cls = torch.randn(B, A, nc, generator=g).double() - 4.5
    dist = torch.rand(B, A, 4, generator=g).double() * 6.0               # images without ground truths: anything
    tight = torch.rand(B, A, generator=g) < 0.3
    jit = 1.0 + (torch.rand(B, A, 4, generator=g).double() * 2 - 1) * torch.where(tight, 0.05, c.jitter).unsqueeze(-1)
    pick_a, pick_c = torch.rand(B, max(t.shape[0], 1), A, generator=g), torch.rand(B, max(t.shape[0], 1), A, generator=g)
    share = torch.cat([torch.full((h * w,), p) for (h, w), p in zip(c.levels, RAISE_SHARE.get(c.name, (0.6,) * len(c.levels)))])
    raise_it, same = torch.rand(B, A, generator=g) < share, torch.rand(B, A, generator=g) < 0.75
    level = torch.rand(B, A, generator=g).double() * 5.5 - 2.5
    floor = torch.randn(B, A, 4, REG, generator=g).double() * 0.5 - 7.0
    if c.name in AIM_WEIGHT:
        pick_a = pick_a * torch.tensor(AIM_WEIGHT[c.name]).view(1, -1, 1)
    for b in range(B):
        r = torch.nonzero(t[:, 0] == b).flatten()
        if len(r):
            tt = t[r].double()
            x1, y1 = (tt[:, 2] - tt[:, 4] / 2) * W, (tt[:, 3] - tt[:, 5] / 2) * H
            x2, y2 = (tt[:, 2] + tt[:, 4] / 2) * W, (tt[:, 3] + tt[:, 5] / 2) * H
            ltrb = torch.stack((px[None, :, 0] - x1[:, None], px[None, :, 1] - y1[:, None], x2[:, None] - px[None, :, 0],
                                y2[:, None] - px[None, :, 1]), -1)    # (n, A, 4) pixels
            cover = ltrb.amin(-1) >= 0
            aim = torch.where(cover, pick_a[b, :len(r)], pick_a[b, :len(r)] - 2.0).argmax(0)          # a covering one where there is any
            other = torch.where(cover, pick_c[b, :len(r)], pick_c[b, :len(r)] - 2.0).argmax(0)
            dist[b] = ltrb[aim, torch.arange(A)] / st * jit[b]
            who = torch.where(same[b], aim, other)
            lab = tt[who, 1].long().clamp(0, nc - 1)
            hit = cover.any(0) & raise_it[b]
            cls[b, hit, lab[hit]] = level[b, hit]
        box[b] = _two_bin(dist[b].clamp(0.02, REG - 1.02), floor[b])
    return torch.cat((box.reshape(B, A, 4 * REG), cls), 2)


def _saturate(c, g, pred):
    """class logits of +-30 and +-12, DFL rows with one dominant bin (-80 elsewhere) and flat rows"""
    B, A, nc = c.B, c.A, c.nc
    vals = torch.tensor([30.0, -30.0, 12.0, -12.0], dtype=torch.float64)
    cls = pred[..., 4 * REG:]
    raised = cls > -2.6
    pick = vals[torch.randint(0, 4, cls.shape, generator=g)]
    cls[:] = torch.where((raised & (torch.rand(cls.shape, generator=g) < 0.5)) | (torch.rand(cls.shape, generator=g) < 0.05), pick, cls)
    box = pred[..., :4 * REG].reshape(B, A, 4, REG)
    e = box.softmax(3).matmul(torch.arange(REG, dtype=torch.float64))
    u = torch.rand(B, A, 4, generator=g)
    dominant = torch.full_like(box, -80.0).scatter_(3, e.round().long().unsqueeze(-1), 0.0)
    box = torch.where((u < 0.25).unsqueeze(-1), dominant, box)
    box = torch.where((u > 0.9).unsqueeze(-1), torch.zeros_like(box), box)
    return torch.cat((box.reshape(B, A, 4 * REG), cls), 2)


@functools.lru_cache(maxsize=None)
def _inputs(c: V8Case):
    g = torch.Generator().manual_seed(1000 * c.seed + 29)
    t = V8_BUILDERS[c.name](c, g).float()
    pred = _predictions(c, g, t)
    if c.name == "saturated":
        pred = _saturate(c, g, pred)
    if c.name == "low_score":
        pred = _micro(c, g, pred)
    batch = {"batch_idx": t[:, 0].clone(), "cls": t[:, 1:2].clone(), "bboxes": t[:, 2:6].clone()}
    return pred.float().contiguous(), batch


def v8_inputs(c):
    """(pred (B, A, 64 + nc) float32, the collate dict batch_idx (N,), cls (N, 1), bboxes (N, 4) normalised cxcywh)"""
    return _inputs(c if isinstance(c, V8Case) else v8_case(c))


def v8_rows(batch):
    """the (N, 6) target rows grouped by image, the order inside an image kept: what the wrapper (train.flatten_targets) hands the kernel"""
    t = torch.cat((batch["batch_idx"].reshape(-1, 1).float(), batch["cls"].reshape(-1, 1).float(), batch["bboxes"].reshape(-1, 4).float()), 1)
    return t[torch.sort(t[:, 0], stable=True).indices].contiguous()


def v8_feats(c: V8Case, pred):
    """(B, A, no) rows -> the head's maps [(B, no, h, w)] as the oracle takes them"""
    return [pred[:, sl].permute(0, 2, 1).reshape(pred.shape[0], pred.shape[2], h, w) for sl, (h, w) in zip(c.level_slices(), c.levels)]


# ----------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------------------------
def ciou(box1, box2, eps=1e-7, eps_w=False, alpha_grad=False):
    """O.ciou with the mutants' switches: eps on the widths too, the gradient passed through alpha"""
    ax1, ay1, ax2, ay2 = box1.unbind(-1)
    bx1, by1, bx2, by2 = box2.unbind(-1)
    w1, h1 = ax2 - ax1 + (eps if eps_w else 0), ay2 - ay1 + eps
    w2, h2 = bx2 - bx1 + (eps if eps_w else 0), by2 - by1 + eps
    inter = (torch.minimum(ax2, bx2) - torch.maximum(ax1, bx1)).clamp(0) * (torch.minimum(ay2, by2) - torch.maximum(ay1, by1)).clamp(0)
    union = w1 * h1 + w2 * h2 - inter + eps
    iou = inter / union
    cw = torch.maximum(ax2, bx2) - torch.minimum(ax1, bx1)
    chh = torch.maximum(ay2, by2) - torch.minimum(ay1, by1)
    c2 = cw ** 2 + chh ** 2 + eps
    rho2 = ((bx1 + bx2 - ax1 - ax2) ** 2 + (by1 + by2 - ay1 - ay2) ** 2) / 4
    v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)).pow(2)
    alpha = v / (v - iou + (1 + eps))
    return iou - (rho2 / c2 + v * (alpha if alpha_grad else alpha.detach()))


@torch.no_grad()
def v8_assign(scores, boxes_px, anc_px, rows, c: V8Case, topk=10, fillers="none", resolve="overlap", claimants_only=False, box_ge=False,
              pos_before=False, last_wins=False, valid_area=False, eps_w=False):
    """The task-aligned assigner per target row.  scores (B, A, nc) sigmoid, boxes_px (B, A, 4), anc_px (A, 2), rows (N, 6) grouped by image.
    Returns dict: gt_index (B, A) row or -1, norm (B, A), and per (row, anchor) dmin / ciou / inbox / metric / ov / mask (the selection before
    the conflicts are resolved), valid (N,), gtbox (N, 4).
    Switches: `topk`; fillers none | topk (torch.topk, the oracle) | inbox (zero metrics selectable: the lowest in-box indices fill the
    ten); conflicts resolved by metric; arg-max over the claimants only; box test `>= 0`; pos_align over the selection before the
    resolution; the last row wins ties; validity by area; eps on the widths of the CIoU."""
    dtype = scores.dtype
    B, A, nc = scores.shape
    N = rows.shape[0]
    H, W = c.hw
    gt_index = torch.full((B, A), -1, dtype=torch.long)
    norm = torch.zeros(B, A, dtype=dtype)
    if N == 0:
        return dict(gt_index=gt_index, norm=norm, N=0)
    rows = rows.to(dtype)
    img, label = rows[:, 0].long(), rows[:, 1].long()
    cxcywh = rows[:, 2:6] * torch.tensor([W, H, W, H], dtype=dtype)
    xy, wh = cxcywh[:, :2], cxcywh[:, 2:]
    gtbox = torch.cat((xy - wh / 2, xy + wh / 2), -1)
    if valid_area:
        valid = ((gtbox[:, 2] - gtbox[:, 0]) * (gtbox[:, 3] - gtbox[:, 1])) > 0
    else:
        valid = gtbox.sum(1) > 0
    dmin = torch.cat((anc_px[None] - gtbox[:, None, :2], gtbox[:, None, 2:] - anc_px[None]), -1).amin(-1)      # (N, A)
    inbox = ((dmin >= 0) if box_ge else (dmin > 1e-9)) & valid[:, None]
    cr = ciou(gtbox[:, None, :], boxes_px[img], eps_w=eps_w)                                                     # (N, A), unclamped
    zero = torch.zeros_like(cr)
    ov = torch.where(inbox, cr.clamp(0), zero)
    sc = torch.where(inbox, scores[img[:, None], torch.arange(A)[None], label.clamp(0, nc - 1)[:, None]], zero)
    metric = sc.pow(0.5) * ov.pow(6.0)
    mask = torch.zeros(N, A, dtype=torch.bool)
    for n in range(N):
        m = metric[n]
        if fillers == "none":
            sel = torch.argsort(-m, stable=True)[:topk]                 # ties to the lower index
            sel = sel[m[sel] > 0]
        elif fillers == "topk":
            sel = torch.topk(m, topk)[1] if bool(valid[n]) else torch.zeros(0, dtype=torch.long)
            sel = sel[inbox[n][sel]]
        else:
            sel = torch.argsort(-torch.where(inbox[n], m, torch.full_like(m, -1.0)), stable=True)[:topk]
            sel = sel[inbox[n][sel]]
        mask[n, sel] = True
    claims = torch.zeros(B, A, dtype=torch.long)
    for b in range(B):
        r = torch.nonzero(img == b).flatten()
        if not len(r):
            continue
        mk = mask[r]
        cnt = mk.sum(0)
        claims[b] = cnt
        key = metric[r] if resolve == "metric" else ov[r]
        if claimants_only:
            key = torch.where(mk, key, torch.full_like(key, -1.0))
        arg = (len(r) - 1 - key.flip(0).argmax(0)) if last_wins else key.argmax(0)
        first = mk.long().argmax(0)
        gt_index[b] = torch.where(cnt == 0, torch.full_like(arg, -1), torch.where(cnt == 1, r[first], r[arg]))
    final = gt_index[img] == torch.arange(N)[:, None]                   # (N, A)
    pos_align = torch.where(mask if pos_before else final, metric, zero).amax(1)
    pos_ov = torch.where(final, ov, zero).amax(1)
    g = gt_index.clamp(0)
    a = torch.arange(A)[None].expand(B, A)
    norm = torch.where(gt_index >= 0, metric[g, a] * pos_ov[g] / (pos_align[g] + 1e-9), norm)
    return dict(gt_index=gt_index, norm=norm, N=N, dmin=dmin, ciou=cr, inbox=inbox, metric=metric, ov=ov, mask=mask, valid=valid, gtbox=gtbox,
                claims=claims, img=img, label=label, pos_align=pos_align, pos_ov=pos_ov)


def v8_forward(pred, rows, c: V8Case, dtype=torch.float64, dfl_clamp=REG - 1 - 0.01, alpha_grad=False, eps_w=False, clamp_sum=True, **assign_sw):
    """The loss of oracle/yolov8_ref.v8_loss on (B, A, 64 + nc) rows and (N, 6) grouped target rows, in `dtype`, with the mutants' switches
    (those of v8_assign, and: the DFL clamp, the gradient through alpha, eps on the widths, no clamp of the score sum).
    Returns (loss = sum(items) * B, items (3,), the assignment dict)."""
    B, A, no = pred.shape
    nc = c.nc
    anchors, stride = c.anchors(dtype)
    p = pred.to(dtype)
    pred_dist, pred_scores = p[..., :4 * REG].contiguous(), p[..., 4 * REG:].contiguous()
    ltrb = pred_dist.view(B, A, 4, REG).softmax(3).matmul(torch.arange(REG, dtype=dtype))
    pred_boxes = torch.cat((anchors - ltrb[..., :2], anchors + ltrb[..., 2:]), -1)
    a = v8_assign(pred_scores.detach().sigmoid(), pred_boxes.detach() * stride, anchors * stride, rows, c, eps_w=eps_w, **assign_sw)
    fg = a["gt_index"] >= 0
    t_scores = torch.zeros(B, A, nc, dtype=dtype)
    t_boxes = torch.zeros(B, A, 4, dtype=dtype)
    if a["N"]:
        g = a["gt_index"].clamp(0)
        t_scores = F.one_hot(a["label"][g].clamp(0), nc).to(dtype) * fg.unsqueeze(-1) * a["norm"].unsqueeze(-1)
        t_boxes = a["gtbox"][g] / stride
    score_sum = max(t_scores.sum(), 1) if clamp_sum else t_scores.sum()
    loss_cls = F.binary_cross_entropy_with_logits(pred_scores, t_scores, reduction="none").sum() / score_sum
    loss_box = torch.zeros((), dtype=dtype)
    loss_dfl = torch.zeros((), dtype=dtype)
    if fg.sum():
        w = t_scores.sum(-1)[fg].unsqueeze(-1)
        iou = ciou(pred_boxes[fg], t_boxes[fg], eps_w=eps_w, alpha_grad=alpha_grad).unsqueeze(-1)
        loss_box = ((1.0 - iou) * w).sum() / score_sum
        t_ltrb = torch.cat((anchors - t_boxes[..., :2], t_boxes[..., 2:] - anchors), -1).clamp(0, dfl_clamp)
        logits = pred_dist[fg].view(-1, REG)
        t = t_ltrb[fg]
        lo = t.long()
        w_lo = (lo + 1) - t
        ce_lo = F.cross_entropy(logits, lo.view(-1), reduction="none").view(lo.shape)
        ce_hi = F.cross_entropy(logits, (lo + 1).clamp(max=REG - 1).view(-1), reduction="none").view(lo.shape)     # (weight 0 where lo = 15)
        dfl = (ce_lo * w_lo + ce_hi * (1 - w_lo)).mean(-1, keepdim=True)
        loss_dfl = (dfl * w).sum() / score_sum
    items = torch.stack((loss_box * GAINS[0], loss_cls * GAINS[1], loss_dfl * GAINS[2]))
    a["score_sum"] = float(t_scores.sum())
    a["t_ltrb_raw"] = None if not a["N"] else torch.cat((anchors - t_boxes[..., :2], t_boxes[..., 2:] - anchors), -1)
    return items.sum() * B, items.detach(), a


def v8_run(name, dtype=torch.float64, **sw):
    """restatement on a case: dict(items, grad (B, A, no), a: the assignment dict)"""
    c = v8_case(name)
    pred, batch = v8_inputs(c)
    p = pred.to(dtype).clone().requires_grad_(True)
    loss, items, a = v8_forward(p, v8_rows(batch), c, dtype, **sw)
    loss.backward()
    return dict(items=items, grad=p.grad, a=a)


def v8_oracle(name, dtype=torch.float64):
    """oracle/yolov8_ref.v8_loss on a case: dict(items, grad (B, A, no), gt_index (B, A) row of the grouped list or -1, norm (B, A), aux)"""
    c = v8_case(name)
    pred, batch = v8_inputs(c)
    p = pred.to(dtype).clone().requires_grad_(True)
    aux = {}
    loss, items = O.v8_loss(v8_feats(c, p), batch, c.nc, tuple(float(s) for s in c.strides), GAINS, aux, dtype=dtype)
    loss.backward()
    rows = v8_rows(batch)
    start = torch.tensor([int((rows[:, 0] < b).sum()) for b in range(c.B)])
    fg = aux["fg_mask"]
    gt_index = torch.where(fg, aux["target_gt_idx"] + start[:, None], torch.full_like(aux["target_gt_idx"], -1))
    return dict(items=items, grad=p.grad, gt_index=gt_index, norm=aux["target_scores"].sum(-1), aux=aux)


@functools.lru_cache(maxsize=None)
def v8_reference(name):
    """The expected output of a case, computed once: the float64 restatement with the kernel's filler rule."""
    return v8_run(name, torch.float64)


# ----------------------------------------------------------------------------------------------------------------------------------------
# margins
# ----------------------------------------------------------------------------------------------------------------------------------------
def _assign_only(name, dtype):
    c = v8_case(name)
    pred, batch = v8_inputs(c)
    with torch.no_grad():
        return v8_forward(pred.to(dtype), v8_rows(batch), c, dtype)[2]


@functools.lru_cache(maxsize=None)
def v8_margins(name):
    """The admissibility condition of the module docstring on one case.  dict(same, admissible, kinds: {box, positive, topk, overlap} ->
    (margin in float64, largest float32-vs-float64 difference of the quantity), edge_ties, overlap_ties, min_metric: the smallest positive
    metric, a: the float64 assignment)."""
    a64, a32 = _assign_only(name, torch.float64), _assign_only(name, torch.float32)
    if a64["N"] == 0:
        return dict(same=True, admissible=True, kinds={}, edge_ties=0, overlap_ties=0, min_metric=float("inf"), a=a64)
    same = torch.equal(a64["gt_index"], a32["gt_index"]) and torch.equal(a64["mask"], a32["mask"]) and torch.equal(a64["inbox"], a32["inbox"])
    inf = float("inf")
    kinds = {}
    # inside the box
    v = a64["valid"][:, None].expand_as(a64["dmin"])
    d64, d32 = a64["dmin"][v], a32["dmin"][v].double()
    tie = (d64 == 0) & (d32 == 0)
    edge_ties = int(tie.sum())
    kinds["box"] = (float((d64[~tie] - 1e-9).abs().min()) if bool((~tie).any()) else inf, float((d64 - d32).abs().max()) if len(d64) else 0.0)
    # positive against zero metric
    ib = a64["inbox"]
    c64, c32 = a64["ciou"][ib], a32["ciou"][ib].double()
    kinds["positive"] = (float(c64.abs().min()) if len(c64) else inf, float((c64 - c32).abs().max()) if len(c64) else 0.0)
    pos = a64["metric"][a64["metric"] > 0]
    min_metric = float(pos.min()) if len(pos) else inf
    same = same and torch.equal(a64["metric"] > 0, a32["metric"] > 0)
    # the tenth against the eleventh
    g64, g32 = [], []
    for n in range(a64["N"]):
        for a, out in ((a64, g64), (a32, g32)):
            m = torch.sort(a["metric"][n], descending=True)[0]
            out.append(float((m[9] - m[10]) / m[9]) if len(m) > 10 and float(m[10]) > 0 else None)      # relative: metrics span 30 orders
    if [x is None for x in g64] != [x is None for x in g32]:
        same = False
    gaps = [(x, y) for x, y in zip(g64, g32) if x is not None and y is not None]
    kinds["topk"] = (min([x for x, _ in gaps], default=inf), max([abs(x - y) for x, y in gaps], default=0.0))
    # the two largest overlaps of a multiply claimed anchor
    margin, diff, overlap_ties = inf, 0.0, 0
    for b, k in torch.nonzero(a64["claims"] > 1).tolist():
        r = torch.nonzero(a64["img"] == b).flatten()
        t64, t32 = torch.sort(a64["ov"][r, k], descending=True)[0][:2], torch.sort(a32["ov"][r, k], descending=True)[0][:2]
        gap64, gap32 = float(t64[0] - t64[1]), float(t32[0] - t32[1])
        if gap64 == 0.0 and gap32 == 0.0:
            overlap_ties += 1
            continue
        margin, diff = min(margin, gap64), max(diff, abs(gap64 - gap32))
    kinds["overlap"] = (margin, diff)
    admissible = same and min_metric >= MIN_POSITIVE_METRIC and all(m >= MARGIN_FACTOR * d for m, d in kinds.values())
    return dict(same=same, admissible=admissible, kinds=kinds, edge_ties=edge_ties, overlap_ties=overlap_ties, min_metric=min_metric, a=a64)


# ----------------------------------------------------------------------------------------------------------------------------------------
# gradient groups
# ----------------------------------------------------------------------------------------------------------------------------------------
def v8_groups(c: V8Case, gt_index):
    """{(level, columns, kind): (anchor mask (B, A), column slice)}: per level, DFL columns 0:64 / class columns 64:64+nc, foreground /
    background anchors"""
    out = {}
    fg = gt_index >= 0
    for lv, sl in enumerate(c.level_slices()):
        inlv = torch.zeros_like(fg)
        inlv[:, sl] = True
        for cols, cs in (("dfl", slice(0, 4 * REG)), ("cls", slice(4 * REG, c.no))):
            for kind, m in (("fg", fg), ("bg", ~fg)):
                if bool((inlv & m).any()):
                    out[(lv, cols, kind)] = (inlv & m, cs)
    return out


def group_errors(c: V8Case, gt_index, have, want):
    """{group: relative L2 error of `have` against `want`, or None where `want` is identically zero (then `have` must be too)}"""
    out = {}
    for key, (m, cs) in v8_groups(c, gt_index).items():
        w, h = want[m][:, cs], have[m][:, cs]
        out[key] = None if float(w.abs().max()) == 0.0 else rel(h, w)
    return out


def v8_fp16_floor(name, scale=None):
    """per group the relative L2 error of the float64 gradient, scaled by the case's loss scale and rounded to fp16: the part no kernel
    can avoid"""
    c = v8_case(name)
    ref = v8_reference(name)
    s = c.scale if scale is None else scale
    scaled = ref["grad"] * s
    assert float(scaled.abs().max()) < 65504.0
    return group_errors(c, ref["a"]["gt_index"], scaled.half().double() / s, ref["grad"])


# ----------------------------------------------------------------------------------------------------------------------------------------
# what each case was built for
# ----------------------------------------------------------------------------------------------------------------------------------------
def filler_difference(name, dtype=torch.float64):
    """anchors on which fillers="topk" (the oracle) and fillers="none" (the kernel) assign differently: dict(zero_weight: anchors that are
    foreground with weight 0 for the oracle and background for the kernel, reassigned: anchors both make foreground but hand to different
    rows -- with (image, anchor, oracle's row, kernel's row, rows that selected it by a positive metric))"""
    c = v8_case(name)
    pred, batch = v8_inputs(c)
    with torch.no_grad():
        none = v8_forward(pred.to(dtype), v8_rows(batch), c, dtype)[2]
        topk = v8_forward(pred.to(dtype), v8_rows(batch), c, dtype, fillers="topk")[2]
    zero, moved, other = [], [], []
    for b, a in torch.nonzero(none["gt_index"] != topk["gt_index"]).tolist():
        gn, gt = int(none["gt_index"][b, a]), int(topk["gt_index"][b, a])
        if gn < 0 and gt >= 0 and float(topk["norm"][b, a]) == 0.0:
            zero.append((b, a, gt))
        elif gn >= 0 and gt >= 0:
            moved.append((b, a, gt, gn, torch.nonzero(none["mask"][:, a] & (none["img"] == b)).flatten().tolist()))
        else:
            other.append((b, a, gt, gn))
    return dict(zero_weight=zero, reassigned=moved, other=other)


@functools.lru_cache(maxsize=None)
def v8_facts(name):
    """what the float64 expected output of a case contains, for the property assertions"""
    c = v8_case(name)
    pred, batch = v8_inputs(c)
    m = v8_margins(name)
    a = v8_reference(name)["a"]
    f = dict(N=a["N"], A=c.A, edge_ties=m["edge_ties"], overlap_ties=m["overlap_ties"], score_sum=a.get("score_sum", 0.0),
             fg=int((a["gt_index"] >= 0).sum()), per_image=[int((batch["batch_idx"] == b).sum()) for b in range(c.B)])
    bi = batch["batch_idx"]
    f["grouped"] = bool((bi[1:] >= bi[:-1]).all())
    if not a["N"]:
        return f
    final = a["gt_index"][a["img"]] == torch.arange(a["N"])[:, None]
    f.update(labels=a["label"].tolist(), multi=int((a["claims"] > 1).sum()), inbox=a["inbox"].sum(1).tolist(), positive=(a["metric"] > 0).sum(1).tolist(),
             selected=a["mask"].sum(1).tolist(), kept=final.sum(1).tolist(), valid=a["valid"].tolist(), pos_align=a["pos_align"].tolist(),
             third_party=int(((a["claims"] > 1) & ~a["mask"][a["gt_index"].clamp(0), torch.arange(c.A)[None].expand(c.B, c.A)]
                              & (a["gt_index"] >= 0)).sum()))
    # centres exactly on an edge, per level; centres strictly inside a box that is no ground truth
    on_edge = (a["dmin"] == 0) & a["valid"][:, None]
    f["edge_ties_per_level"] = [int(on_edge[:, sl].sum()) for sl in c.level_slices()]
    f["inside_invalid"] = int(((a["dmin"] > 1e-9) & ~a["valid"][:, None]).sum())
    # DFL targets at the clamp, per level, over the foreground anchors' four sides
    fg = a["gt_index"] >= 0
    raw = a["t_ltrb_raw"]
    f["clamped_sides"] = [int((raw[:, sl][fg[:, sl]] > REG - 1 - 0.01).sum()) for sl in c.level_slices()]
    f["fg_per_level"] = [int(fg[:, sl].sum()) for sl in c.level_slices()]
    f["kept_per_level"] = [[int(final[n, sl].sum()) for sl in c.level_slices()] for n in range(a["N"])]
    return f


def _saturated_ok(f):
    pred, _ = v8_inputs("saturated")
    cls, box = pred[..., 4 * REG:], pred[..., :4 * REG].reshape(pred.shape[0], pred.shape[1], 4, REG)
    fg = v8_reference("saturated")["a"]["gt_index"] >= 0
    dominant = (box == -80.0).sum(-1) == REG - 1
    flat = (box == 0.0).all(-1)
    return (all(int((cls[fg] == v).sum()) > 0 and int((cls[~fg] == v).sum()) > 0 for v in (30.0, -30.0, 12.0, -12.0))
            and int(dominant[fg].sum()) > 10 and int(flat[fg].sum()) > 2 and f["multi"] > 0)


def _fillers_ok(f):
    d = filler_difference("fillers")
    few = [n for n in range(f["N"]) if f["positive"][n] < 10 and f["inbox"][n] > f["positive"][n]]
    third = [r for r in d["reassigned"] if r[3] in r[4] and r[2] not in r[4]]      # the kernel keeps a claimant, the oracle moves to a non-claimant
    return len(few) >= 2 and len(d["zero_weight"]) > 0 and len(third) > 0 and not d["other"]


V8_PROPERTY = {
    "crowd": lambda f: f["per_image"] == [40, 0, 25] and not f["grouped"] and f["multi"] >= 24 and f["score_sum"] > 10,
    "duplicates": lambda f: f["overlap_ties"] >= 10 and [f["selected"][n] > 0 and f["kept"][n] == 0 and f["pos_align"][n] == 0.0 for n in (2, 6)] == [True, True]
    and f["kept"][0] > 0 and f["kept"][5] > 0,
    "edge_on": lambda f: min(f["edge_ties_per_level"]) > 0 and f["valid"].count(False) == 1 and f["inside_invalid"] > 0,
    "tiny": lambda f: 0 in f["inbox"] and 1 in f["inbox"] and any(2 <= k <= 9 for k in f["inbox"]) and any(0 < p < 10 for p in f["positive"])
    and 0 in f["kept"],
    "fillers": _fillers_ok,
    "huge": lambda f: f["A"] > 1024 and f["clamped_sides"][0] > 0 and f["clamped_sides"][1] > 0 and f["inbox"][0] == f["A"] and all(k > 0 for k in f["kept_per_level"][0][:2]),
    "nonsquare": lambda f: f["fg"] > 50 and f["score_sum"] > 10,
    "saturated": _saturated_ok,
    "low_score": lambda f: 0.0 < f["score_sum"] < 1.0 and f["kept"][0] >= 2 and f["kept_per_level"][1] == [0, 0, 1] and f["fg_per_level"][2] == 1,
    "levels1": lambda f: f["fg"] > 20 and f["multi"] > 0,
    "levels2": lambda f: min(f["fg_per_level"]) > 0,
    "levels4": lambda f: min(f["fg_per_level"]) > 0,
    "nc1": lambda f: f["labels"].count(-1) == 1 and f["kept"][f["labels"].index(-1)] > 0 and f["multi"] > 0,
    "nc3": lambda f: f["labels"].count(-1) == 1 and f["kept"][f["labels"].index(-1)] > 0 and f["multi"] > 0,
    "empty": lambda f: f["N"] == 0,
}
