"""numpy restatement of csrc/box_fusion.hip: Weighted Boxes Fusion (Solovyev et al., 2021) as this project pins it,
float32 with every step one rounded operation in the order written here.  It is the specification of ``cvx_det_fuse_wbf``; the reference
has no counterpart.  The map and the clamp of a row are ``det_tta_restatement.map_boxes`` and the overlap is ``tiled_restatement.overlaps``,
both imported: the same bits as ``cvx_det_fuse_views``.

Per frame:
  candidates  the rows r < counts[s] of the slots s = k * B + f, k the source; ordinal s * K + r.  A count outside [0, K] contributes
              nothing and adds 1 to the overflow word.  More than FUSE_CAP rows: count -1, zero outputs, overflow + 1.  A row is skipped
              when its raw score is below ``skip_score`` or its mapped and clamped box does not have x2 > x1 and y2 > y1 (zero width or
              height; a NaN corner).  Its weighted score is s = score * weights[k].
  order       class ascending (the bits of the fp32 class, which order like the value for the non-negative classes the tails emit), then
              s descending (its bits), then ordinal ascending.  ``class_agnostic``: one segment, (s, ordinal) alone.
  clusters    a segment is walked in order; candidate j joins the cluster c of its segment with the largest IoU(fused_c, box_j) that is
              strictly above ``iou_thr``, the lowest c among equals (a NaN never matches), else it opens one.
              open:   fused = box_j, sw = s_j, sx = s_j * box_j, n = 1, smax = s_j, first = ordinal_j, class = class_j
              update: sw = sw + s_j, sx = sx + s_j * box_j, n += 1, fused = sx / sw
  score       m = fminf((float)n, W), W = the fp32 sum of the weights in index order.  avg: ((sw / (float)n) * m) / W; max: (smax * m) / W;
              without ``rescale`` sw / (float)n or smax.
  emit        the clusters of the frame by (score descending, first ascending), the first ``max_det``: [fused, score, class], source =
              first, members = n.

``match="first"`` (for the tests alone) compares a candidate with each cluster's first box instead of its fused box."""
import functools

import numpy as np

import det_tta_restatement as DR
from det_tta_restatement import map_boxes
from tiled_restatement import overlaps

FUSE_CAP = 8192
MAX_SOURCES = 32
F32 = np.float32


def area_of(box):
    return ((box[..., 2] - box[..., 0]) * (box[..., 3] - box[..., 1])).astype(F32)


def fuse_wbf(rows, counts, view_map, frame_hw, weights=None, iou_thr=0.55, skip_score=0.0, conf="avg", rescale=True, class_agnostic=False,
             max_det=300, match="fused"):
    """rows (S * B, K, 6) float32, counts (S * B), view_map (S * B, 4) float32, frame_hw (B, 2), weights (S) ->
    (rows (B, max_det, 6) float32, counts (B) int32, source (B, max_det) int32, members (B, max_det) int32, overflow int)"""
    rows, view_map = np.asarray(rows, F32), np.asarray(view_map, F32)
    counts, frame_hw = np.asarray(counts, np.int64), np.asarray(frame_hw, np.int64)
    SB, K = rows.shape[:2]
    B = len(frame_hw)
    S = SB // B
    assert S * B == SB and 1 <= S <= MAX_SOURCES and view_map.shape == (SB, 4) and conf in ("avg", "max") and match in ("fused", "first")
    weights = np.ones(S, F32) if weights is None else np.asarray(weights, F32)
    assert weights.shape == (S,)
    W = F32(0)
    for w in weights:
        W = F32(W + w)
    thr, skip = F32(iou_thr), F32(skip_score)
    out_rows = np.zeros((B, max_det, 6), F32)
    out_counts = np.zeros(B, np.int32)
    out_source = np.full((B, max_det), -1, np.int32)
    out_members = np.zeros((B, max_det), np.int32)
    overflow = 0
    for f in range(B):
        ordinals = []
        for k in range(S):
            s = k * B + f
            if counts[s] < 0 or counts[s] > K:
                overflow += 1
                continue
            ordinals += [s * K + r for r in range(int(counts[s]))]
        if len(ordinals) > FUSE_CAP:
            out_counts[f] = -1
            overflow += 1
            continue
        if not ordinals:
            continue
        ordinals = np.array(ordinals, np.int64)
        cand = rows.reshape(SB * K, 6)[ordinals]
        box = map_boxes(cand, view_map[ordinals // K], frame_hw[f, 0], frame_hw[f, 1])
        keep = ~(cand[:, 4] < skip) & (box[:, 2] > box[:, 0]) & (box[:, 3] > box[:, 1])
        cand, box, ordinals = cand[keep], box[keep], ordinals[keep]
        if not len(cand):
            continue
        s_w = (cand[:, 4] * weights[ordinals // K // B]).astype(F32)
        cls = cand[:, 5].copy()
        cls_bits = np.zeros(len(cand), np.uint64) if class_agnostic else cls.view(np.uint32).astype(np.uint64)
        order = np.lexsort((ordinals, np.uint64(0xFFFFFFFF) - s_w.view(np.uint32).astype(np.uint64), cls_bits))
        box, s_w, cls, cls_bits, ordinals = box[order], s_w[order], cls[order], cls_bits[order], ordinals[order]
        source = ordinals // K // B
        n = len(box)
        area = area_of(box)
        clusters = []                                              # of the frame, in creation order: dicts
        a = 0
        while a < n:
            e = a
            while e < n and cls_bits[e] == cls_bits[a]:
                e += 1
            L = e - a
            fused, probe = np.zeros((L, 4), F32), np.zeros((L, 4), F32)     # probe: what a candidate is compared with
            seg = []
            for j in range(a, e):
                best = -1
                if seg:
                    v = overlaps(box[j], area[j], probe[:len(seg)], area_of(probe[:len(seg)]), "iou")
                    hit = v > thr                                  # a NaN compares false
                    if hit.any():
                        best = int(np.argmax(np.where(hit, v, F32(-1))))       # the first of the largest: ties to the older cluster
                if best < 0:
                    c = dict(sw=s_w[j], sx=(s_w[j] * box[j]).astype(F32), n=1, smax=s_w[j], first=int(ordinals[j]), cls=cls[j],
                             seen=1 << int(source[j]), at=len(seg))
                    fused[len(seg)] = probe[len(seg)] = box[j]
                    seg.append(c)
                else:
                    c = seg[best]
                    c["sw"] = F32(c["sw"] + s_w[j])
                    c["sx"] = (c["sx"] + (s_w[j] * box[j]).astype(F32)).astype(F32)
                    c["n"] += 1
                    c["seen"] |= 1 << int(source[j])
                    fused[best] = (c["sx"] / c["sw"]).astype(F32)
                    if match == "fused":
                        probe[best] = fused[best]
            for c in seg:
                c["box"] = fused[c["at"]].copy()
                nf = F32(c["n"])
                base = F32(c["sw"] / nf) if conf == "avg" else c["smax"]
                c["score"] = F32(F32(base * np.fmin(nf, W)) / W) if rescale else base
            clusters += seg
            a = e
        key = [((0xFFFFFFFF - int(np.asarray(c["score"], F32).view(np.uint32))) << 32, c["first"]) for c in clusters]
        emit = sorted(range(len(clusters)), key=lambda i: key[i])[:max_det]
        for r, i in enumerate(emit):
            c = clusters[i]
            out_rows[f, r, :4], out_rows[f, r, 4], out_rows[f, r, 5] = c["box"], c["score"], c["cls"]
            out_source[f, r], out_members[f, r] = c["first"], c["n"]
        out_counts[f] = len(emit)
    return out_rows, out_counts, out_source, out_members, overflow


# ---- the seeded inputs of the kernel tests (tests/test_box_fusion_gpu.py), here so that the CPU suite can check what they assume -------------
IDENTITY = np.array([1, 0, 1, 0], F32)
WEIGHTS = {1: np.array([1.5], F32), 3: np.array([1.0, 2.0, 0.5], F32), 6: np.array([1.0, 0.75, 2.0, 1.25, 0.5, 1.0], F32)}
WBF_IOU = 0.55


@functools.lru_cache(maxsize=None)
def wbf_case(B, S, seed=3, k_in=16):
    """The recipe of ``det_tta_restatement.fuse_case`` -- copies of its four base boxes written in each source's own coordinates, the
    inverse of a flipped or scaled map (``VIEW_GEOMETRY``), scores from a small set so that ties occur, three classes; with B = 3 frame 1
    is empty -- with a jitter of up to 13.5 pixels a corner, so that the overlaps of a box with its cluster lie on both sides of
    ``WBF_IOU`` and chains form.  (rows, counts, view_map, frame_hw, weights); shared and never modified."""
    rng = np.random.RandomState(seed + 100 * B + S)
    SB = S * B
    counts = rng.randint(5, k_in + 1, SB).astype(np.int32)
    counts[0] = k_in
    if B > 1:
        counts[np.arange(S) * B + 1] = 0
    vmap, rows = np.zeros((SB, 4), F32), np.zeros((SB, k_in, 6), F32)
    for k in range(S):
        z, flip = DR.VIEW_GEOMETRY[k]
        for b in range(B):
            s = k * B + b
            fh, fw = (int(v) for v in DR.FRAME_HW[b])
            left, top = (fw - fw * z) / 2, (fh - fh * z) / 2
            vmap[s] = [-1 / z, (fw - left) / z, 1 / z, -top / z] if flip else [1 / z, -left / z, 1 / z, -top / z]
            for r in range(k_in):                                   # rows past the count are filled too: they are not candidates
                box = DR.BASE[rng.randint(4)] + rng.randint(-9, 10, 4).astype(F32) * F32(1.5)
                x1, x2 = ((box[[0, 2]] - vmap[s, 1]) / vmap[s, 0])[::-1 if flip else 1]
                y1, y2 = (box[[1, 3]] - vmap[s, 3]) / vmap[s, 2]
                rows[s, r] = [x1, y1, x2, y2, rng.choice([0.9, 0.75, 0.5, 0.25]), rng.randint(3)]
    return frozen(rows, counts, vmap, DR.FRAME_HW[:B], WEIGHTS[S])


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def grid_boxes(n, size=6.0, pitch=10.0, per_row=32):
    """n disjoint boxes on a grid"""
    k = np.arange(n)
    x, y = (k % per_row) * pitch, (k // per_row) * pitch
    return np.stack([x, y, x + size, y + size], 1).astype(F32)


STRIDE_HW = np.array([[400, 400]], np.int32)
STRIDE_K = 48


def in_slots(boxes, scores, classes, S, K):
    """rows (S, K, 6) and counts of one frame: the rows dealt to the S sources in turn"""
    rows, counts = np.zeros((S, K, 6), F32), np.zeros(S, np.int32)
    for i, (b, s, c) in enumerate(zip(boxes, scores, classes)):
        k = i % S
        rows[k, counts[k]] = [*b, s, c]
        counts[k] += 1
    assert counts.max() <= K
    return rows, counts


@functools.lru_cache(maxsize=None)
def stride_case(kind, n):
    """one class in one frame over three sources.  ``disjoint``: n boxes that overlap nothing -- n clusters, the cluster index crosses the
    wave's 64 lanes; ``copies``: n near-copies of one box -- one cluster of n members; ``mixed`` (n ignored): 70 disjoint boxes with
    falling scores, then a near-copy of box 66 -- candidate 70 must match cluster 66.  (rows, counts, view_map, frame_hw, weights)"""
    rng = np.random.RandomState(31 + n)
    if kind == "disjoint":
        boxes = grid_boxes(n)
        scores = rng.choice([0.9, 0.6, 0.3], n)
    elif kind == "copies":
        boxes = np.array([100, 100, 220, 200], F32) + rng.randint(-4, 5, (n, 4)).astype(F32) * F32(0.5)
        scores = rng.choice([0.9, 0.6, 0.3], n)
    else:
        boxes = np.concatenate([grid_boxes(70), grid_boxes(70)[66:67] + np.array([0.25, 0, 0.25, 0], F32)])
        scores = np.concatenate([0.95 - 0.005 * np.arange(70), [0.1]])
    rows, counts = in_slots(boxes, scores, np.full(len(boxes), 2.0), 3, STRIDE_K)
    return frozen(rows, counts, np.tile(IDENTITY, (3, 1)), STRIDE_HW, np.ones(3, F32))


@functools.lru_cache(maxsize=None)
def classes_case(n_classes):
    """one frame whose candidates fall into ``n_classes`` classes with gaps between the indices (class 3 * i + (i % 2)): more segments than
    the 16 waves of the workgroup, the last third of them of a single candidate, the others of several overlapping ones"""
    rng = np.random.RandomState(17 + n_classes)
    boxes, scores, classes = [], [], []
    for i in range(n_classes):
        members = 1 if 3 * i >= 2 * n_classes else int(rng.randint(2, 7))
        base = np.array([20, 20, 120, 110], F32) + F32(i)
        for _ in range(members):
            boxes.append(base + rng.randint(-3, 4, 4).astype(F32) + (F32(150) if rng.rand() < 0.3 else F32(0)))
            scores.append(rng.choice([0.9, 0.7, 0.5, 0.3]))
            classes.append(3 * i + (i % 2))
    order = rng.permutation(len(boxes))
    rows, counts = in_slots(np.array(boxes)[order], np.array(scores)[order], np.array(classes, F32)[order], 2, 128)
    return frozen(rows, counts, np.tile(IDENTITY, (2, 1)), STRIDE_HW, np.array([1.0, 1.5], F32))


@functools.lru_cache(maxsize=None)
def capacity_case(extra):
    """``det_tta_restatement.capacity_case``: 8192 + extra disjoint candidates of one class in frame 1 of 2, eight sources"""
    rows, counts, vmap, frame_hw = DR.capacity_case(extra)
    return rows, counts, vmap, frame_hw, np.ones(8, F32)
