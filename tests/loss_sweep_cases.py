"""Seeded cases and reference glue for the sweeps of the training-side loss and target kernels -- ``cvx_yolo7_loss``,
``cvx_centernet_loss``, ``cvx_centernet_draw_targets``, ``cvx_ssd_encode_targets`` -- shared by tests/test_loss_sweep_cpu.py (which shows
from the oracles alone that every case has the property it was built for, that the discrete decisions of the SimOTA assignment keep
clear of float32 round-off, and that deliberately wrong restatements change the expected outputs) and tests/test_loss_sweep_gpu.py (which
runs the kernels on them).  No GPU dependency.

The references are the project's oracles (oracle/yolov7_ref.py, oracle/centernet_ref.py, oracle/ssd_ref.py), run in float64 where the
kernel computes in float32.  ``y7_candidates`` / ``y7_assign`` / ``cn_loss`` / ``draw`` / ``ssd_encode`` are restatements with switches
for the mutants; without a switch they are asserted equal to the oracles.

The SimOTA margins.  The assignment takes three kinds of discrete decision per ground truth: dynamic k = int(sum of the top-20 IoUs)
(clamped to >= 1), the k cheapest candidates, and the cheapest ground truth of a candidate several ground truths claim.  ``y7_assign``
reports how far each is from flipping: the distance of the IoU sum from the nearest integer at which k changes (2, 3, ...: below 2 the
clamp makes int() immaterial, so a sum of exactly 0 -- a saturated head -- is 2 away, not 0), the gap between the k-th and the (k+1)-th
cheapest cost, and for each contested candidate the gap between its two lowest costs.  ``y7_margins`` runs it in float32 and float64 and
records the largest difference of those same quantities; a case is admissible when both runs assign identically and every margin is
at least 100 times that difference (the kernel's expf / logf / summation order differ from torch's by a few ulp more).

One kind of tie no margin can cover: two candidates of one image that name the SAME cell (two ground truths whose half-cell offsets reach
it) read the same head row, so their cost columns are bit-identical in every precision, on the CPU and in the kernel.  When such a pair
straddles a ground truth's k, the value gap is exactly 0 and which of the two is taken is a rule, not a rounding: the kernel takes the
lower list index; ``torch.topk`` (the reference and the oracle) leaves it unspecified.  These pairs are what makes a cell receive two
matched entries of DIFFERENT ground truths (without one, both duplicates always go to the same ground truth: they have the same
claimants), so the clusters case needs them, and a crowded image has dozens.  They are excluded from the value margin and counted
(``straddles``); the expected output is the oracle with ``ties="lower"`` (oracle/yolov7_ref.simota_assign), which differs from the default
only in taking the lower index of such a pair.  The CPU test asserts oracle(ties="lower") == restatement in both precisions, and
oracle(default) == restatement on the cases that have no such pair.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from oracle import centernet_ref as C
from oracle import ssd_ref as S
from oracle import yolov7_ref as Y

Y7_GMAX, Y7_CMAX = 64, 2880      # ground truths / candidates per image the assignment kernel holds (csrc/loss_yolov7.hip)
Y7_SCALE = 256.0                 # loss scale of every YOLOv7 case
MARGIN_FACTOR = 100.0


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ----------------------------------------------------------------------------------------------------------------------------------------
# YOLOv7 loss
# ----------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Y7Case:
    name: str
    seed: int
    B: int
    nc: int = 20
    ld: int = 80
    levels: tuple = ((4, 4), (8, 8), (16, 16))
    input_hw: tuple = (128, 128)
    smoothing: float = 0.0
    gain: float = 1.5                # head outputs = N(0, 1) * gain

    @property
    def img_size(self):
        return float(self.input_hw[0])                # imgs[b].shape[1], as the reference passes it


def _boxes(g, n, b, nc, lo=0.16, hi=0.40, c_lo=0.08, c_hi=0.92):
    t = torch.zeros(n, 6)
    t[:, 0] = b
    t[:, 1] = torch.randint(0, nc, (n,), generator=g).float()
    t[:, 2:4] = torch.rand(n, 2, generator=g) * (c_hi - c_lo) + c_lo
    t[:, 4:6] = torch.rand(n, 2, generator=g) * (hi - lo) + lo
    return t


def _targets_crowd(c, g):
    t = torch.cat((_boxes(g, 40, 0, c.nc), _boxes(g, 30, 2, c.nc)))
    return t[torch.randperm(70, generator=g)]                          # interleaved by image, image 1 empty


def _targets_cap64(c, g):
    t = torch.cat((_boxes(g, 3, 0, c.nc), _boxes(g, Y7_GMAX, 1, c.nc, 0.1, 0.45)))
    return t[torch.randperm(t.shape[0], generator=g)]


def _targets_clusters(c, g):
    rows = []
    for b, sizes in ((0, (4, 3, 4)), (1, (3, 4))):
        for n in sizes:
            base = _boxes(g, 1, b, c.nc, 0.18, 0.30, 0.2, 0.8)[0]
            cls = torch.randperm(c.nc, generator=g)[:n]
            for k in range(n):                                          # one centre, sizes 6 % apart, different classes
                r = base.clone()
                r[1] = float(cls[k])
                r[4:6] = base[4:6] * (1.0 + 0.06 * k)
                rows.append(r)
    return torch.stack(rows)


def _targets_borders(c, g):
    s = 16.0                                                           # every number below is a multiple of 1/64 of a level-2 cell: exact in float32
    cells = [(0.5, 8.25, 3.0, 4.0), (15.625, 8.25, 3.0, 4.0), (7.25, 0.375, 4.0, 3.0), (8.75, 15.75, 4.0, 3.0),   # within one cell of each border
             (0.25, 0.25, 2.5, 2.5), (15.75, 15.75, 2.5, 2.5),                                                 # two corners
             (5.0, 9.0, 3.5, 3.5),                       # exactly on a cell boundary of level 2 in x and y
             (6.5, 3.5, 3.0, 5.0),                       # fraction exactly 0.5 at level 2: neither the left nor the right neighbour
             (1.0, 4.25, 3.0, 3.0), (15.0, 11.75, 3.0, 3.0), (4.25, 1.0, 3.0, 3.0), (11.75, 15.0, 3.0, 3.0),   # gx == 1 / W - gx == 1: `> 1` is strict
             (8.25, 8.25, 6.0, 3.0),                     # width exactly 4 x the 1.5-cell anchor of level 2: excluded by the strict `<`
             (10.25, 5.75, 3.0, 8.0)]                    # height exactly 4 x its 2-cell height
    t = torch.zeros(len(cells), 6)
    t[:, 0] = torch.tensor([0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1, 0, 1], dtype=torch.float32)
    t[:, 1] = torch.randint(0, c.nc, (len(cells),), generator=g).float()
    t[:, 2:6] = torch.tensor(cells) / s
    return t


def _targets_small(c, g):
    return torch.cat([_boxes(g, 5, b, c.nc, 0.12, 0.45) for b in range(c.B)])


def _targets_nonsquare(c, g):
    t = torch.cat([_boxes(g, 6, b, c.nc, 0.10, 0.35) for b in range(c.B)])
    return t[torch.randperm(t.shape[0], generator=g)]


def _targets_saturated(c, g):
    # three ordinary boxes and three of 4 to 6 pixels per image: those pass the ratio test of the smallest level-2 anchor alone, and a saturated
    # centre (offset -0.5 or 1.5 cells, size ~0 or 4 x the anchor) can miss them altogether
    return torch.cat([torch.cat((_boxes(g, 3, b, c.nc, 0.12, 0.40), _boxes(g, 3, b, c.nc, 0.03, 0.05))) for b in range(c.B)])


Y7_BUILDERS = {"crowd": _targets_crowd, "capacity64": _targets_cap64, "clusters": _targets_clusters, "borders": _targets_borders,
               "nonsquare": _targets_nonsquare, "nc1": _targets_small, "nc80": _targets_small, "smoothing": _targets_small,
               "saturated": _targets_saturated}

# the seeds are the first (from 0) at which the case has its property and y7_margins(...) is admissible
Y7_CASES = (
    Y7Case("crowd", 0, 3),
    Y7Case("capacity64", 0, 2),
    Y7Case("clusters", 2, 2),
    Y7Case("borders", 0, 2),
    Y7Case("nonsquare", 0, 2, levels=((5, 7), (10, 14), (20, 28)), input_hw=(160, 224)),
    Y7Case("nc1", 0, 2, nc=1, ld=18),
    Y7Case("nc80", 0, 2, nc=80, ld=256),
    Y7Case("smoothing", 0, 2, smoothing=0.1),
    Y7Case("saturated", 78, 2, gain=6.0),
)


def y7_case(name) -> Y7Case:
    return next(c for c in Y7_CASES if c.name == name)


def y7_inputs(c: Y7Case):
    """(outs: three (B, 3 * (5 + nc), h, w) float32 maps, coarsest first; targets (N, 6) float32)"""
    g = torch.Generator().manual_seed(1000 * c.seed + 17)
    outs = [torch.randn(c.B, 3 * (5 + c.nc), h, w, generator=g) * c.gain for h, w in c.levels]
    return outs, Y7_BUILDERS[c.name](c, g)


def y7_preds(outs, dtype):
    return [o.to(dtype).reshape(o.shape[0], 3, -1, o.shape[2], o.shape[3]).permute(0, 1, 3, 4, 2) for o in outs]


def y7_rows(outs, ld):
    """the engine's head rows (B, A, ld): level after level, (gj, gi) order, anchor a in columns a * (5 + nc) ..., zero padding"""
    B = outs[0].shape[0]
    rows = torch.zeros(B, sum(o.shape[2] * o.shape[3] for o in outs), ld, dtype=outs[0].dtype)
    a_off = 0
    for o in outs:
        hw = o.shape[2] * o.shape[3]
        rows[:, a_off:a_off + hw, :o.shape[1]] = o.permute(0, 2, 3, 1).reshape(B, hw, -1)
        a_off += hw
    return rows


def y7_candidates(targets, level_hw, ratio_le=False, half_le=False, border_ge=False, anchor_major=False):
    """Y.loss_candidates restated with the mutants' switches: ratio `<= 4`, half cell `<= 0.5`, border `>= 1`, anchor-major list order."""
    out = []
    N = targets.shape[0]
    one, half, thr = torch.tensor(1.0), torch.tensor(0.5), torch.tensor(4.0)
    for lv, (h, w) in enumerate(level_hw):
        anc = Y._level_anchors(lv)
        gain = torch.tensor([w, h, w, h], dtype=torch.float32)
        t = targets[:, 2:6].float() * gain
        r = t[:, None, 2:4] / anc[None]                                              # (N, 3, 2)
        m = torch.max(r, 1.0 / r).max(2)[0]
        ok = (m <= thr) if ratio_le else (m < thr)
        inv = gain[:2] - t[:, :2]
        lt = (lambda v: v % 1.0 <= half) if half_le else (lambda v: v % 1.0 < half)
        gt = (lambda v: v >= one) if border_ge else (lambda v: v > one)
        cond = [torch.ones(N, dtype=torch.bool), lt(t[:, 0]) & gt(t[:, 0]), lt(t[:, 1]) & gt(t[:, 1]), lt(inv[:, 0]) & gt(inv[:, 0]), lt(inv[:, 1]) & gt(inv[:, 1])]
        cands = []
        order = [(oi, a) for a in range(3) for oi in range(5)] if anchor_major else [(oi, a) for oi in range(5) for a in range(3)]
        for oi, a in order:
            ox, oy = Y.OFFSETS[oi]
            gi = (t[:, 0] - ox).to(torch.int64).clamp(0, w - 1)
            gj = (t[:, 1] - oy).to(torch.int64).clamp(0, h - 1)
            for n in torch.nonzero(ok[:, a] & cond[oi]).flatten().tolist():
                cands.append((int(targets[n, 0]), a, int(gj[n]), int(gi[n]), n))
        out.append(cands)
    return out


def y7_assign(preds, targets, cands, img_size, nc, dtype=torch.float64, topn=20, round_k=False, claimants_only=False):
    """Y.simota_assign restated on whole tensors, ties to the lower list index, with the mutants' switches (top-`topn`, dynamic k rounded,
    conflict argmin over the claimants only).  Returns (matched lists per level, info per image with ground truths): IoU sums, k, the three
    margins of the module docstring, the contested candidates, the straddling duplicate pairs and whether torch.topk broke them the same
    way."""
    matched = [[] for _ in preds]
    info = {}
    for b in range(preds[0].shape[0]):
        rows = [n for n in range(targets.shape[0]) if int(targets[n, 0]) == b]
        ent = [(lv,) + e for lv in range(len(preds)) for e in cands[lv] if e[0] == b]          # (lv, b, a, gj, gi, n)
        if not rows or not ent:
            continue
        tgt = targets[rows]
        txywh = tgt[:, 2:6].to(dtype) * img_size
        txyxy = torch.cat((txywh[:, :2] - txywh[:, 2:] / 2, txywh[:, :2] + txywh[:, 2:] / 2), 1)
        e = torch.tensor(ent)
        v = torch.stack([preds[lv][b, a, gj, gi] for lv, _, a, gj, gi, _ in ent])
        anc = torch.stack([Y._level_anchors(lv)[a] for lv, _, a, _, _, _ in ent])
        stride = torch.tensor([Y.STRIDES_LOSS[lv] for lv, *_ in ent], dtype=dtype)[:, None]
        grid = torch.stack((e[:, 4], e[:, 3]), 1).to(dtype)
        pxy = (v[:, :2].sigmoid() * 2.0 - 0.5 + grid) * stride
        pwh = (v[:, 2:4].sigmoid() * 2) ** 2 * anc * stride
        boxes = torch.cat((pxy - pwh / 2, pxy + pwh / 2), 1)
        G, Cn = txyxy.shape[0], boxes.shape[0]
        lt, rb = torch.max(txyxy[:, None, :2], boxes[None, :, :2]), torch.min(txyxy[:, None, 2:], boxes[None, :, 2:])
        inter = (rb - lt).clamp(min=0).prod(2)
        area_t = ((txyxy[:, 2] - txyxy[:, 0]) * (txyxy[:, 3] - txyxy[:, 1]))[:, None]
        area_p = ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))[None]
        iou = inter / (area_t + area_p - inter)
        sums = torch.topk(iou, min(topn, Cn), dim=1)[0].sum(1)
        ks = torch.clamp((sums.round() if round_k else sums).int(), min=1)
        onehot = F.one_hot(tgt[:, 1].long(), nc).to(dtype)[:, None, :].expand(G, Cn, nc)
        y = (v[:, 5:].to(dtype).sigmoid()[None] * v[:, 4:5].sigmoid()[None]).expand(G, Cn, nc).sqrt()
        cost = F.binary_cross_entropy_with_logits(torch.log(y / (1 - y)), onehot, reduction="none").sum(-1) + 3.0 * (-torch.log(iou + 1e-8))
        cellkey = ((e[:, 0] * 3 + e[:, 2]) * 4096 + e[:, 3]) * 4096 + e[:, 4]
        match = torch.zeros(G, Cn, dtype=torch.bool)
        k_margin, gap_margin, straddles, topk_agrees = [], [], 0, True
        for g in range(G):
            k = min(int(ks[g]), Cn)
            order = torch.argsort(cost[g], stable=True)
            match[g, order[:k]] = True
            if set(torch.topk(cost[g], k=k, largest=False)[1].tolist()) != set(order[:k].tolist()):
                topk_agrees = False
            s = float(sums[g])
            k_margin.append(abs(s - max(2.0, round(s))) if not round_k else 0.0)
            if k < Cn:
                i, j = int(order[k - 1]), int(order[k])
                gap = float(cost[g, j] - cost[g, i])
                if gap == 0.0 and int(cellkey[i]) == int(cellkey[j]):
                    straddles += 1                                            # one cell twice: bit-identical columns, decided by list order
                else:
                    gap_margin.append(gap)
        claims = match.sum(0)
        contested = torch.nonzero(claims > 1).flatten().tolist()
        gt_of = torch.full((Cn,), -1, dtype=torch.long)
        con_margin = []
        for cidx in range(Cn):
            if claims[cidx] == 1:
                gt_of[cidx] = int(torch.nonzero(match[:, cidx]).flatten()[0])
            elif claims[cidx] > 1:
                col = cost[:, cidx]
                two = torch.sort(col)[0][:2]
                con_margin.append(float(two[1] - two[0]))
                if claimants_only:
                    col = torch.where(match[:, cidx], col, torch.full_like(col, float("inf")))
                gt_of[cidx] = int(torch.argmin(col))
        for cidx in range(Cn):
            if gt_of[cidx] >= 0:
                lv, cb, a, gj, gi, _ = ent[cidx]
                matched[lv].append((cb, a, gj, gi, rows[int(gt_of[cidx])]))
        info[b] = dict(G=G, C=Cn, sums=sums, ks=ks, iou=iou, k_margin=k_margin, gap_margin=gap_margin, con_margin=con_margin, contested=contested,
                       straddles=straddles, topk_agrees=topk_agrees, gt_of=gt_of, ent=ent, boxes=boxes, txyxy=txyxy)
    return matched, info


def y7_margins(c: Y7Case, outs=None, targets=None):
    """The admissibility condition of the module docstring on one case: dict(same: float32 and float64 assign identically, margin: the
    smallest margin (float64), diff: the largest float32-vs-float64 difference of an IoU sum, a k / k+1 gap or a contested gap,
    straddles, topk_agrees, info: the float64 run's)."""
    if outs is None:
        outs, targets = y7_inputs(c)
    cands = Y.loss_candidates(targets, c.levels)
    m64, i64 = y7_assign(y7_preds(outs, torch.float64), targets, cands, c.img_size, c.nc, torch.float64)
    m32, i32 = y7_assign(y7_preds(outs, torch.float32), targets, cands, c.img_size, c.nc, torch.float32)
    same = m64 == m32
    diff, margin, straddles, agrees = 0.0, float("inf"), 0, True
    for b, a in i64.items():
        z = i32[b]
        diff = max(diff, float((a["sums"] - z["sums"].double()).abs().max()))
        for key in ("gap_margin", "con_margin"):
            if len(a[key]) == len(z[key]):
                diff = max([diff] + [abs(p - q) for p, q in zip(a[key], z[key])])
            else:
                same = False
        margin = min([margin] + a["k_margin"] + a["gap_margin"] + a["con_margin"])
        straddles += a["straddles"]
        agrees = agrees and a["topk_agrees"] and z["topk_agrees"]
    return dict(same=same, margin=margin, diff=diff, straddles=straddles, topk_agrees=agrees, info=i64, cands=cands, matched=m64)


def y7_entry_ious(c: Y7Case, outs, targets, matched):
    """per level the clamped CIoU of every matched entry, float64, in list order (what yolo7_loss writes into the objectness target)"""
    preds = y7_preds(outs, torch.float64)
    res = []
    for lv, m in enumerate(matched):
        if not m:
            res.append(torch.zeros(0, dtype=torch.float64))
            continue
        h, w = c.levels[lv]
        b, a, gj, gi = (torch.tensor([e[k] for e in m]) for k in range(4))
        tt = targets[[e[4] for e in m]]
        pp = preds[lv][b, a, gj, gi]
        xy = pp[:, :2].sigmoid() * 2.0 - 0.5
        wh = (pp[:, 2:4].sigmoid() * 2) ** 2 * Y._level_anchors(lv)[a]
        tbox = tt[:, 2:6] * torch.tensor([w, h, w, h], dtype=torch.float64)
        tbox = torch.cat((tbox[:, :2] - torch.stack([gi, gj], 1).double(), tbox[:, 2:]), 1)
        res.append(Y._ciou_xywh(torch.cat((xy, wh), 1), tbox).clamp(0))
    return res


def y7_objectness_targets(c: Y7Case, outs, targets, matched, first_wins=False):
    """per level the objectness target map (B, 3, h, w) float64: of the entries that name a cell the LAST in list order wins (index_put on
    the CPU); `first_wins` is the mutant."""
    vals = y7_entry_ious(c, outs, targets, matched)
    maps = []
    for lv, m in enumerate(matched):
        t = torch.zeros(c.B, 3, *c.levels[lv], dtype=torch.float64)
        seen = set()
        for k, (b, a, gj, gi, _) in enumerate(m):
            if first_wins and (b, a, gj, gi) in seen:
                continue
            seen.add((b, a, gj, gi))
            t[b, a, gj, gi] = vals[lv][k]
        maps.append(t)
    return maps


def y7_duplicates(matched):
    """cells matched through more than one list entry: {(level, image, anchor, gj, gi): [list positions]}"""
    d = {}
    for lv, m in enumerate(matched):
        for k, e in enumerate(m):
            d.setdefault((lv,) + tuple(e[:4]), []).append(k)
    return {k: v for k, v in d.items() if len(v) > 1}


@functools.lru_cache(maxsize=None)
def y7_reference(name):
    """The float64 oracle (ties to the lower list index, the kernel's rule) on one case, computed once: candidates (float32 decisions),
    matched lists, the four loss items, the gradient w.r.t. the head rows (B, A, ld) and the objectness target maps."""
    c = y7_case(name)
    outs, targets = y7_inputs(c)
    o64 = [o.double().requires_grad_(True) for o in outs]
    items = Y.yolo7_loss(o64, targets, c.img_size, c.nc, c.input_hw, c.smoothing, dtype=torch.float64, ties="lower")
    items[0].backward()
    cands = Y.loss_candidates(targets, c.levels)
    matched = Y.simota_assign(y7_preds(outs, torch.float64), targets, cands, c.img_size, c.nc, torch.float64, "lower")
    return dict(case=c, outs=outs, targets=targets, cands=cands, matched=matched, items=torch.stack([v.detach().reshape(()) for v in items]),
                grad=y7_rows([o.grad for o in o64], c.ld), tobj=y7_objectness_targets(c, outs, targets, matched))


def y7_groups(c: Y7Case):
    """column groups of the head rows: {name: column indices} for box (0:4 of every anchor), objectness (4), classes (5:), padding"""
    na = 5 + c.nc
    box = [a * na + k for a in range(3) for k in range(4)]
    obj = [a * na + 4 for a in range(3)]
    cls = [a * na + 5 + k for a in range(3) for k in range(c.nc)]
    return dict(box=box, obj=obj, cls=cls, pad=list(range(3 * na, c.ld)))


def y7_level_slices(c: Y7Case):
    out, a_off = [], 0
    for h, w in c.levels:
        out.append(slice(a_off, a_off + h * w))
        a_off += h * w
    return out


# ----------------------------------------------------------------------------------------------------------------------------------------
# CenterNet loss
# ----------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class CnCase:
    name: str
    B: int
    h: int
    w: int
    nc: int
    K: int
    seed: int
    special: tuple = ()

    @property
    def nc_pad(self):
        return (self.nc + 7) & ~7

    @property
    def ld(self):
        return self.nc_pad + 16


CN_SCALE = 64.0
CN_REDUCE_SPAN = 256 * 256            # cn_reduce_kernel: at most 256 workgroups of 256 threads
CN_GRAD_SPAN = 4096 * 256             # cn_grad_kernel: at most 4096
CN_CASES = (
    CnCase("5x7_nc1_k1", 2, 5, 7, 1, 1, 11),
    CnCase("16x16_nc3_k30", 3, 16, 16, 3, 30, 12, ("indices", "heat_edges", "clamp")),
    CnCase("32x24_nc20_k30", 2, 32, 24, 20, 30, 13, ("clamp",)),
    CnCase("32x24_nc80_k30", 2, 32, 24, 80, 30, 14),                 # npix * nc = 122 880: second iteration of cn_reduce_kernel
    CnCase("64x64_nc80_k30", 4, 64, 64, 80, 30, 15),                 # npix * ld = 1 572 864: second iteration of cn_grad_kernel
)
CLAMP_LOGITS = (12.0, -12.0, 9.3, -9.3, 9.2, -9.2)   # sigmoid(+-9.3) lies outside [1e-4, 1 - 1e-4] by 9 %, sigmoid(+-9.2) inside by 1 %


def cn_case(name) -> CnCase:
    return next(c for c in CN_CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def cn_inputs(name):
    """(pred (B, h, w, nc + 4) float32, targets [heat, reg, wh, mask, idx]).  `indices`: image 0 has four objects on one index, mask zeros
    between ones and the indices 0 and A - 1; image 1 an all-zero mask; image 2 a full one.  `heat_edges`: targets of exactly 1 and of the
    float just below 1 next to each other.  `clamp`: logits of CLAMP_LOGITS on cells whose target is 1 and on cells whose target is < 1."""
    c = cn_case(name)
    g = torch.Generator().manual_seed(c.seed)
    pred = torch.randn(c.B, c.h, c.w, c.nc + 4, generator=g) * 2.0
    heat, reg, wh, mask, idx = C.synth_targets(c.B, c.h, c.w, c.nc, c.K, seed=c.seed)
    A = c.h * c.w
    if "indices" in c.special:
        mask.zero_()
        reg, wh = torch.rand(c.B, c.K, 2, generator=g), torch.rand(c.B, c.K, 2, generator=g) * 8 + 1
        idx = torch.randint(0, A, (c.B, c.K), generator=g)
        idx[0, [1, 4, 5, 9]] = 77                                     # four objects on one index ...
        idx[0, 0], idx[0, 11] = 0, A - 1
        mask[0, [0, 1, 4, 5, 7, 9, 11]] = 1.0                         # ... zeros between the ones
        idx[0, 2] = 77                                                # (a masked-out object on the shared index)
        mask[2] = 1.0                                                 # image 1: nothing, image 2: the full table
        idx[2, 20:23] = idx[2, 3]
    if "heat_edges" in c.special:
        below = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
        heat[0, 3, 3, 0], heat[0, 3, 4, 0], heat[0, 3, 5, 0] = 1.0, below, 1.0
        heat[1, 8, 8, 2], heat[1, 8, 9, 2] = below, below
    if "clamp" in c.special:
        pos = torch.nonzero(heat == 1.0)
        neg = torch.nonzero(heat < 0.5)
        assert len(pos) >= 1 and len(neg) >= len(CLAMP_LOGITS)
        for k, v in enumerate(CLAMP_LOGITS):
            b, y, x, ch = pos[k % len(pos)].tolist()
            if k >= len(pos):                                         # not enough centres: plant one more
                b, y, x, ch = neg[-1 - k].tolist()
                heat[b, y, x, ch] = 1.0
            pred[b, y, x, ch] = v
            b, y, x, ch = neg[k * 7 % len(neg)].tolist()
            pred[b, y, x, ch] = v
    return pred, [heat, reg, wh, mask, idx]


def cn_rows(c: CnCase, pred):
    """the engine's head rows (B, h * w, ld): heat map in 0 .. nc, the loss's "reg" pair at nc_pad, its "wh" pair at nc_pad + 8"""
    flat = pred.reshape(c.B, c.h * c.w, c.nc + 4)
    rows = torch.zeros(c.B, c.h * c.w, c.ld, dtype=pred.dtype)
    rows[..., :c.nc], rows[..., c.nc_pad:c.nc_pad + 2], rows[..., c.nc_pad + 8:c.nc_pad + 10] = flat[..., :c.nc], flat[..., c.nc:c.nc + 2], flat[..., c.nc + 2:]
    return rows


def cn_groups(c: CnCase):
    used = list(range(c.nc)) + [c.nc_pad, c.nc_pad + 1, c.nc_pad + 8, c.nc_pad + 9]
    return dict(heat=list(range(c.nc)), a=[c.nc_pad, c.nc_pad + 1], b=[c.nc_pad + 8, c.nc_pad + 9], pad=[k for k in range(c.ld) if k not in used])


def cn_loss(pred, targets, nc, hm_weight=1.0, wh_weight=0.1, off_weight=1.0, single_den=False, clamp_passes=False, scatter_once=False):
    """C.combined_loss restated with the mutants' switches: L1 denominator sum(mask) instead of twice it, the gradient passed outside the
    clamp, objects on a shared index gathered once."""
    heat_t, reg_t, wh_t, mask, idx = targets
    p = torch.sigmoid(pred[..., :nc])
    cl = torch.clamp(p, min=1e-4, max=1.0 - 1e-4)
    heat = p + (cl - p).detach() if clamp_passes else cl
    pos, neg = torch.eq(heat_t, 1).float(), torch.lt(heat_t, 1).float()
    num_pos = pos.sum()
    pos_loss = (torch.log(heat) * torch.pow(1 - heat, 2) * pos).sum()
    neg_loss = (torch.log(1 - heat) * torch.pow(heat, 2) * torch.pow(1 - heat_t, 4) * neg).sum()
    hm = -neg_loss if float(num_pos) == 0 else -(pos_loss + neg_loss) / num_pos
    m1 = mask.clone()
    if scatter_once:
        for b in range(idx.shape[0]):
            seen = set()
            for k in range(idx.shape[1]):
                if m1[b, k] != 0 and int(idx[b, k]) in seen:
                    m1[b, k] = 0
                if m1[b, k] != 0:
                    seen.add(int(idx[b, k]))

    def l1(feat, true):
        f = feat.reshape(feat.shape[0], -1, feat.shape[3])
        gth = torch.gather(f, 1, idx.unsqueeze(2).long().expand(idx.shape[0], idx.shape[1], f.shape[2]))
        m = mask.unsqueeze(2).expand_as(gth).float()
        mm = m1.unsqueeze(2).expand_as(gth).float()
        den = (mask.float().sum() if single_den else m.sum()) + 1e-4
        return ((gth * mm - true * mm).abs() if scatter_once else (gth * m - true * m).abs()).sum() / den

    off, wh = l1(pred[..., nc:nc + 2], reg_t), l1(pred[..., -2:], wh_t)
    return hm_weight * hm + off_weight * off + wh_weight * wh, hm, off, wh


@functools.lru_cache(maxsize=None)
def cn_reference(name, **mutant):
    """float64: (items (4,), gradient w.r.t. the head rows (B, h * w, ld)); without a mutant from oracle/centernet_ref.combined_loss itself"""
    c = cn_case(name)
    pred, targets = cn_inputs(name)
    p64 = pred.double().requires_grad_(True)
    t64 = [targets[0].double(), targets[1].double(), targets[2].double(), targets[3].double(), targets[4]]
    items = cn_loss(p64, t64, c.nc, **mutant) if mutant else C.combined_loss(p64, t64, c.nc)
    items[0].backward()
    return torch.stack([v.detach().reshape(()) for v in items]), cn_rows(c, p64.grad)


# ----------------------------------------------------------------------------------------------------------------------------------------
# CenterNet target drawing
# ----------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class DrawCase:
    name: str
    H: int
    W: int
    nc: int
    K: int
    seed: int


DRAW_CASES = (DrawCase("24x40_nc80", 24, 40, 80, 10, 21), DrawCase("8x8_nc1", 8, 8, 1, 10, 22))
DRAW_IMAGES = ("stack", "edges", "random", "empty", "stack_reversed")


def draw_case(name) -> DrawCase:
    return next(c for c in DRAW_CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def draw_inputs(name):
    """labels (5, K, 5) float32 [class id, cx, cy, w, h], counts (5,).  Image `stack`: a full table (K = 10) of overlapping boxes of one
    class, ten sizes, centres within a cell or two; `edges`: a box three times the map (clipped on all four sides), boxes whose integer
    width / height truncates to 0, a centre in the last row and last column, class nc - 1; `random`; `empty`; `stack_reversed`: the stack
    in reverse order (the maximum merge must not depend on it)."""
    c = draw_case(name)
    g = torch.Generator().manual_seed(c.seed)
    lab = torch.zeros(len(DRAW_IMAGES), c.K, 5)
    counts = torch.zeros(len(DRAW_IMAGES), dtype=torch.int32)
    cls = min(3, c.nc - 1)
    for k in range(c.K):                                               # sizes from a cell to most of the map
        s = 0.08 + 0.085 * k
        lab[0, k] = torch.tensor([cls, 0.45 + 0.02 * float(torch.rand(1, generator=g)), 0.55 + 0.03 * float(torch.rand(1, generator=g)), s, s * 0.9])
    counts[0] = c.K
    last = c.nc - 1
    lab[1, 0] = torch.tensor([last, 0.5, 0.5, 3.0, 3.0])
    lab[1, 1] = torch.tensor([0, 0.3, 0.6, 0.5 / c.W, 0.4])           # width truncates to 0
    lab[1, 2] = torch.tensor([last, 0.7, 0.2, 0.5, 0.5 / c.H])         # height truncates to 0
    lab[1, 3] = torch.tensor([last, 0.6, 0.7, 0.4 / c.W, 0.4 / c.H])   # both
    lab[1, 4] = torch.tensor([0, (c.W - 0.25) / c.W, (c.H - 0.25) / c.H, 0.45, 0.4])        # centre in the last row and column
    lab[1, 5] = torch.tensor([last, 0.25 / c.W, 0.25 / c.H, 0.3, 0.3])                      # and in the first
    counts[1] = 6
    n = 7
    lab[2, :n, 0] = torch.randint(0, c.nc, (n,), generator=g).float()
    lab[2, :n, 1:3] = torch.rand(n, 2, generator=g) * 0.9 + 0.05
    lab[2, :n, 3:5] = torch.rand(n, 2, generator=g) * 0.5 + 0.03
    counts[2] = n
    lab[4] = lab[0].flip(0)
    counts[4] = c.K
    return lab, counts


def draw(label, feature_hw, nc, max_num_boxes, round_radius=False, sum_merge=False):
    """C.generate_targets restated with the mutants' switches: the radius rounded instead of truncated, Gaussians summed instead of merged
    by maximum."""
    H, W = feature_hw
    label = np.array(label, dtype=np.float32, copy=True)
    cc = label[:, 2:]
    rows = np.concatenate((cc[:, 0:1] - cc[:, 2:3] / 2, cc[:, 1:2] - cc[:, 3:4] / 2, cc[:, 0:1] + cc[:, 2:3] / 2, cc[:, 1:2] + cc[:, 3:4] / 2, label[:, 1:2]), -1)
    rows = rows[:max_num_boxes]
    hm = np.zeros((H, W, nc), dtype=np.float32)
    reg, wh = np.zeros((max_num_boxes, 2), dtype=np.float32), np.zeros((max_num_boxes, 2), dtype=np.float32)
    mask, ind = np.zeros((max_num_boxes,), dtype=np.float32), np.zeros((max_num_boxes,), dtype=np.float32)
    for j, item in enumerate(rows):
        item[:4:2] = item[:4:2] * W
        item[1:4:2] = item[1:4:2] * H
        xmin, ymin, xmax, ymax, cid = item
        cid = cid.astype(np.int32)
        h, w = int(ymax - ymin), int(xmax - xmin)
        r = C.gaussian_radius((h, w))
        radius = max(0, int(round(r)) if round_radius else int(r))
        ctr = np.array([(xmin + xmax) / 2, (ymin + ymax) / 2], dtype=np.float32)
        ci = ctr.astype(np.int32)
        d = 2 * radius + 1
        m = (d - 1.0) / 2.0
        yy, xx = np.ogrid[-m:m + 1, -m:m + 1]
        gk = np.exp(-(xx * xx + yy * yy) / (2 * (d / 6) * (d / 6)))
        gk[gk < np.finfo(gk.dtype).eps * gk.max()] = 0
        x, y = int(ci[0]), int(ci[1])
        left, right, top, bottom = min(x, radius), min(W - x, radius + 1), min(y, radius), min(H - y, radius + 1)
        if right + left > 0 and top + bottom > 0:
            mg = gk[radius - top:radius + bottom, radius - left:radius + right].astype(np.float32)
            view = hm[y - top:y + bottom, x - left:x + right, cid]
            hm[y - top:y + bottom, x - left:x + right, cid] = view + mg if sum_merge else np.maximum(view, mg)
        reg[j] = ctr - ci
        wh[j] = np.array([w, h], dtype=np.float32)
        mask[j] = 1
        ind[j] = ci[1] * W + ci[0]
    return hm, reg, wh, mask, ind


def _as_label6(rows5):
    rows5 = np.asarray(rows5, dtype=np.float32)
    return np.concatenate((np.zeros((len(rows5), 1), np.float32), rows5), 1)


def draw_geometry(c: DrawCase, row5):
    """(x, y, radius, integer h, integer w) of one label row, as the oracle computes them"""
    l = np.asarray(row5, dtype=np.float32)
    xmin, xmax = (l[1] - l[3] / 2) * np.float32(c.W), (l[1] + l[3] / 2) * np.float32(c.W)
    ymin, ymax = (l[2] - l[4] / 2) * np.float32(c.H), (l[2] + l[4] / 2) * np.float32(c.H)
    h, w = int(ymax - ymin), int(xmax - xmin)
    return int(np.float32((xmin + xmax) / 2)), int(np.float32((ymin + ymax) / 2)), max(0, int(C.gaussian_radius((h, w)))), h, w


@functools.lru_cache(maxsize=None)
def draw_reference(name, **mutant):
    """per image (heat, reg, wh, mask, ind) from oracle/centernet_ref.generate_targets (or the mutant restatement)"""
    c = draw_case(name)
    lab, counts = draw_inputs(name)
    fn = (lambda l: draw(l, (c.H, c.W), c.nc, c.K, **mutant)) if mutant else (lambda l: C.generate_targets(l, (c.H, c.W), c.nc, c.K))
    return [fn(_as_label6(lab[b, :int(counts[b])].numpy())) for b in range(lab.shape[0])]


# ----------------------------------------------------------------------------------------------------------------------------------------
# SSD target encoding
# ----------------------------------------------------------------------------------------------------------------------------------------
SSD_NC, SSD_NMAX, SSD_THR = 20, 6, 0.5
SSD_PRIOR_SETS = ("all_8732", "slice_300")
SSD_IMAGES = ("empty", "one", "full", "whole_image", "slivers", "mirrored", "outside")


@functools.lru_cache(maxsize=None)
def ssd_priors(which):
    p = S.priors()
    assert p.shape == (8732, 4)
    return p if which == "all_8732" else np.ascontiguousarray(p[::29][:300])      # every scale; 7 x 300 rows end inside a 256-thread group


def _iou64(priors, row5):
    """the oracle's float64 IoU of one label row [class, cx, cy, w, h] (float32 corners) with every prior"""
    l = np.asarray(row5, dtype=np.float32)
    box = np.array([l[1] - l[3] / 2, l[2] - l[4] / 2, l[1] + l[3] / 2, l[2] + l[4] / 2], dtype=np.float32).astype(np.float64)
    wh = np.maximum(np.minimum(priors[:, 2:4], box[2:]) - np.maximum(priors[:, :2], box[:2]), 0)
    inter = wh[:, 0] * wh[:, 1]
    return inter / ((box[2] - box[0]) * (box[3] - box[1]) + (priors[:, 2] - priors[:, 0]) * (priors[:, 3] - priors[:, 1]) - inter)


def _mirrored_pair(priors):
    """two different boxes of a prior's size, shifted left / right of its centre by the same amount, whose oracle IoUs with that prior are
    bit-equal and above the threshold: the first prior (largest first) and shift for which float32 / float64 rounding keeps the symmetry"""
    area = (priors[:, 2] - priors[:, 0]) * (priors[:, 3] - priors[:, 1])
    inside = (priors.min(1) > 0.02) & (priors.max(1) < 0.98)
    for p in np.argsort(-area, kind="stable"):
        if not inside[p]:
            continue
        x0, y0, x1, y1 = (float(v) for v in priors[p])
        for d in (1 / 64, 1 / 128, 1 / 32):
            a = np.array([3, (x0 + x1) / 2 + d, (y0 + y1) / 2, x1 - x0, y1 - y0], dtype=np.float32)
            b = np.array([7, (x0 + x1) / 2 - d, (y0 + y1) / 2, x1 - x0, y1 - y0], dtype=np.float32)
            ia, ib = _iou64(priors, a), _iou64(priors, b)
            if ia[p] == ib[p] and ia[p] > SSD_THR:
                return int(p), a, b
    raise AssertionError("no prior keeps the mirror symmetry in floating point")


def _sliver_pair(priors):
    """two thin boxes no prior overlaps above the threshold whose best prior is the same prior (found by search over positions)"""
    for k in range(200):
        cx, cy = 0.31 + 0.003 * k, 0.47
        a = np.array([2, cx, cy, 0.004, 0.30], dtype=np.float32)
        b = np.array([9, cx + 0.002, cy + 0.01, 0.005, 0.28], dtype=np.float32)
        ia, ib = _iou64(priors, a), _iou64(priors, b)
        if ia.max() <= SSD_THR and ib.max() <= SSD_THR and ia.argmax() == ib.argmax() and ia.max() > 0 and ia[ia.argmax()] != ib[ib.argmax()]:
            return int(ia.argmax()), a, b
    raise AssertionError("no sliver pair shares its best prior")


@functools.lru_cache(maxsize=None)
def ssd_inputs(which):
    """labels (7, SSD_NMAX, 5) float32 [class id, cx, cy, w, h], counts (7,), notes (the priors the constructed images aim at)"""
    pri = ssd_priors(which)
    g = torch.Generator().manual_seed(31 + len(pri))
    lab = np.zeros((len(SSD_IMAGES), SSD_NMAX, 5), np.float32)
    counts = np.zeros(len(SSD_IMAGES), np.int32)

    def rand_rows(n):
        r = np.zeros((n, 5), np.float32)
        r[:, 0] = torch.randint(0, SSD_NC, (n,), generator=g).numpy()
        r[:, 1:3] = (torch.rand(n, 2, generator=g) * 0.6 + 0.2).numpy()
        r[:, 3:5] = (torch.rand(n, 2, generator=g) * 0.35 + 0.05).numpy()
        return r

    lab[1, :1], counts[1] = rand_rows(1), 1
    lab[2], counts[2] = rand_rows(SSD_NMAX), SSD_NMAX
    lab[3, 0], counts[3] = np.array([5, 0.5, 0.5, 1.0, 1.0], np.float32), 1
    sp, a, b = _sliver_pair(pri)
    lab[4, 0], lab[4, 1], counts[4] = a, b, 2
    mp, a, b = _mirrored_pair(pri)
    lab[5, 0], lab[5, 1], counts[5] = a, b, 2
    lab[6, 0], counts[6] = np.array([4, 1.5, 1.5, 0.1, 0.1], np.float32), 1          # outside the image: IoU 0 with every prior
    return lab, counts, dict(sliver_prior=sp, mirror_prior=mp)


def ssd_encode(label, anchors, nc, overlap_threshold=0.5, variance=(0.1, 0.1, 0.2, 0.2), force_always=False, last_on_ties=False):
    """S.generate_targets restated with the mutants' switches: every box's best prior is forced onto that box even when a prior exceeds the
    threshold (the matching rule of other SSD implementations), the last ground truth on ties of the per-prior argmax."""
    label = np.array(label, dtype=np.float32, copy=True)
    anchors = np.asarray(anchors, dtype=np.float32)
    variance = np.asarray(variance, dtype=np.float32)
    A = anchors.shape[0]
    label[:, 1] += 1
    cls = label[:, 1].astype(np.int32)
    c = label[:, 2:]
    coord = np.concatenate((c[:, 0:1] - c[:, 2:3] / 2, c[:, 1:2] - c[:, 3:4] / 2, c[:, 0:1] + c[:, 2:3] / 2, c[:, 1:2] + c[:, 3:4] / 2), -1)
    assignment = np.zeros((A, 4 + 1 + nc + 1), dtype=np.float32)
    assignment[:, 4] = 1.0
    if len(coord) == 0:
        return assignment
    enc, forced = [], []
    for box in coord.astype(np.float64):
        wh = np.maximum(np.minimum(anchors[:, 2:4], box[2:]) - np.maximum(anchors[:, :2], box[:2]), 0)
        inter = wh[:, 0] * wh[:, 1]
        iou = inter / ((box[2] - box[0]) * (box[3] - box[1]) + (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1]) - inter)
        e = np.zeros((A, 5))
        mask = iou > overlap_threshold
        if not mask.any():
            mask[iou.argmax()] = True
        e[:, -1][mask] = iou[mask]
        if force_always:
            e[iou.argmax(), -1] = 2.0
        aa = anchors[mask]
        a_center, a_wh = (aa[:, 0:2] + aa[:, 2:4]) * 0.5, aa[:, 2:4] - aa[:, 0:2]
        e[:, :2][mask] = 0.5 * (box[:2] + box[2:]) - a_center
        e[:, :2][mask] /= a_wh
        e[:, :2][mask] /= variance[:2]
        e[:, 2:4][mask] = np.log((box[2:] - box[:2]) / a_wh)
        e[:, 2:4][mask] /= variance[2:4]
        enc.append(e)
    enc = np.stack(enc)
    score = enc[:, :, -1]
    best = score.max(0)
    idx = (len(score) - 1 - score[::-1].argmax(0)) if last_on_ties else score.argmax(0)
    m = best > 0
    idx = idx[m]
    assignment[:, :4][m] = enc[:, m, :][idx, np.arange(len(idx)), :4]
    assignment[:, 4][m] = 0
    assignment[:, 5:-1][m] = np.eye(nc + 1)[cls][idx, 1:]
    assignment[:, -1][m] = 1
    return assignment


@functools.lru_cache(maxsize=None)
def ssd_reference(which, **mutant):
    """(7, A, 4 + 21 + 1) float32 from oracle/ssd_ref.generate_targets per image (or the mutant restatement)"""
    pri = ssd_priors(which)
    lab, counts, _ = ssd_inputs(which)
    fn = (lambda l: ssd_encode(l, pri, SSD_NC, SSD_THR, **mutant)) if mutant else (lambda l: S.generate_targets(l, pri, SSD_NC, SSD_THR))
    return np.stack([fn(_as_label6(lab[b, :counts[b]])) for b in range(len(counts))])
