"""numpy restatement of csrc/det_tta.hip, float32 with the kernels' operations in the kernels' order.  It is the
specification of ``cvx_det_tta_inputs`` -- the resize of seg_tta_restatement inside a rectangle, the pad around it, the mirror -- and of
``cvx_det_fuse_views``: a rounded product and a rounded add per corner, the corners re-ordered, the clamp, the (score desc, ordinal asc)
key, the greedy pass under IoU (tiled_restatement's arithmetic, imported), the members of each kept row, the vote and the scores.

A view is ``(h, w, top, left, flip)``."""
import functools

import numpy as np

from seg_tta_restatement import resize_plane_stack
from tiled_restatement import overlaps

FUSE_CAP = 8192
PAD = np.float32(128.0) / np.float32(255.0)


def view_rect(H, W, h, w, flip):
    """the view of content size (h, w), in the middle of an (H, W) input"""
    return (h, w, (H - h) // 2, (W - w) // 2, flip)


def tta_inputs(images, views, pad=PAD, slots=None):
    """images (B, 3, H, W) -> (slots, 3, H, W) float32, slot k * B + b; the slots no view names are left NaN"""
    images = np.asarray(images, np.float32)
    B, C, H, W = images.shape
    out = np.full((len(views) * B if slots is None else slots, C, H, W), np.nan, np.float32)
    for k, (h, w, top, left, flip) in enumerate(views):
        slot = np.full((B, C, H, W), np.float32(pad), np.float32)
        slot[:, :, top:top + h, left:left + w] = resize_plane_stack(images, h, w)
        out[k * B:(k + 1) * B] = slot[..., ::-1] if flip else slot          # the resize first, the mirror second
    return out


def map_boxes(cand, vmap, fh, fw):
    """cand (n, 6) rows, vmap (n, 4) [ax, cx, ay, cy] of each row's slot -> (n, 4) boxes in the picture"""
    zero = np.float32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        tx1 = (cand[:, 0] * vmap[:, 0]).astype(np.float32) + vmap[:, 1]
        tx2 = (cand[:, 2] * vmap[:, 0]).astype(np.float32) + vmap[:, 1]
        ty1 = (cand[:, 1] * vmap[:, 2]).astype(np.float32) + vmap[:, 3]
        ty2 = (cand[:, 3] * vmap[:, 2]).astype(np.float32) + vmap[:, 3]
    box = np.empty((len(cand), 4), np.float32)
    box[:, 0] = np.fmin(np.fmax(np.fmin(tx1, tx2), zero), np.float32(fw))
    box[:, 1] = np.fmin(np.fmax(np.fmin(ty1, ty2), zero), np.float32(fh))
    box[:, 2] = np.fmin(np.fmax(np.fmax(tx1, tx2), zero), np.float32(fw))
    box[:, 3] = np.fmin(np.fmax(np.fmax(ty1, ty2), zero), np.float32(fh))
    return box


def fuse_views(rows, counts, view_map, frame_hw, threshold=0.5, class_agnostic=False, mode="vote", score_mode="max", max_det=300):
    """rows (V * B, K, 6) float32, counts (V * B), view_map (V * B, 4) float32, frame_hw (B, 2) ->
    (rows (B, max_det, 6) float32, counts (B) int32, source (B, max_det) int32, members (B, max_det) int32, overflow int)"""
    rows, view_map = np.asarray(rows, np.float32), np.asarray(view_map, np.float32)
    counts, frame_hw = np.asarray(counts, np.int64), np.asarray(frame_hw, np.int64)
    S, K = rows.shape[:2]
    B = len(frame_hw)
    V = S // B
    assert V * B == S and view_map.shape == (S, 4) and mode in ("nms", "vote") and score_mode in ("max", "views")
    thr = np.float32(threshold)
    out_rows = np.zeros((B, max_det, 6), np.float32)
    out_counts = np.zeros(B, np.int32)
    out_source = np.full((B, max_det), -1, np.int32)
    out_members = np.zeros((B, max_det), np.int32)
    overflow = 0
    for f in range(B):
        ordinals = []
        for k in range(V):
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
        cand = rows.reshape(S * K, 6)[ordinals]
        key = ((np.uint64(0xFFFFFFFF) - cand[:, 4].view(np.uint32).astype(np.uint64)) << np.uint64(32)) | ordinals.astype(np.uint64)
        order = np.argsort(key, kind="stable")
        cand, ordinals = cand[order], ordinals[order]
        n = len(cand)
        box = map_boxes(cand, view_map[ordinals // K], frame_hw[f, 0], frame_hw[f, 1])
        area = ((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])).astype(np.float32)
        score, cls, view = cand[:, 4], cand[:, 5], ordinals // K // B
        removed = np.zeros(n, bool)
        kept = []
        for i in range(n):
            if len(kept) >= max_det:
                break
            if removed[i]:
                continue
            kept.append(i)
            hit = overlaps(box[i], area[i], box[i + 1:], area[i + 1:], "iou") > thr          # a NaN compares false: it never suppresses
            if not class_agnostic:
                hit &= cls[i + 1:] == cls[i]
            removed[i + 1:] |= hit
        for r, i in enumerate(kept):
            iou = overlaps(box[i], area[i], box, area, "iou")
            hit = iou > thr
            if not class_agnostic:
                hit &= cls == cls[i]
            hit[i] = True
            members = np.flatnonzero(hit)
            own = box[i].copy()
            if mode == "vote":
                wt, acc = np.float32(0), np.zeros(4, np.float32)
                for j in members:                                   # sorted order; every operation rounded on its own
                    w = score[i] if j == i else np.float32(iou[j] * score[j])
                    wt = np.float32(wt + w)
                    acc = (acc + (w * box[j]).astype(np.float32)).astype(np.float32)
                if len(members) > 1 and wt > 0:
                    own = (acc / wt).astype(np.float32)
            out_rows[f, r, :4] = own
            if score_mode == "views":
                m = len(set(view[members].tolist()))
                out_rows[f, r, 4] = np.float32(np.float32(score[i] * np.float32(m)) / np.float32(V))
            else:
                out_rows[f, r, 4] = score[i]
            out_rows[f, r, 5] = cls[i]
            out_source[f, r] = ordinals[i]
            out_members[f, r] = len(members)
        out_counts[f] = len(kept)
    return out_rows, out_counts, out_source, out_members, overflow


def view_map(views, input_hw, terms):
    """(V * B, 4) float32 [ax, cx, ay, cy], slot k * B + b, in float64 from the tail's (px, py, gx, gy), each (B), rounded once"""
    H, W = input_hw
    px, py, gx, gy = (np.asarray(t, np.float64) for t in terms)
    out = []
    for h, w, top, left, flip in views:
        rx, ry = W / w, H / h
        if flip:
            ax, cx = np.full_like(gx, -rx), gx * ((W - px - left) * rx - px)
        else:
            ax, cx = np.full_like(gx, rx), gx * (px * (rx - 1.0) - left * rx)
        out.append(np.stack((ax, cx, np.full_like(gy, ry), gy * (py * (ry - 1.0) - top * ry)), 1))
    return np.concatenate(out).astype(np.float32)


# ---- the seeded inputs of the kernel tests (tests/test_det_tta_gpu.py), here so that the CPU suite can check what they assume ------------------
K_IN = 16
FUSE_SEED = 7
FRAME_HW = np.array([[120, 150], [64, 64], [140, 160]], np.int32)
BASE = np.array([[20, 20, 70, 80], [60, 30, 120, 90], [10, 70, 60, 118], [90, 60, 150, 125]], np.float32)
# per view: the zoom s, whether it is mirrored; the "network" is the picture itself (px = py = 0, gx = gy = 1, W = the picture's width)
VIEW_GEOMETRY = [(1.0, False), (0.75, True), (0.5, False), (0.875, True), (0.625, False), (1.0, True)]


@functools.lru_cache(maxsize=None)
def fuse_case(B, V, seed=FUSE_SEED, k_in=K_IN, empty_frame=True):
    """(rows (V * B, k_in, 6), counts, view_map (V * B, 4)) for the first B frames of FRAME_HW: jittered copies of a few base boxes,
    written in each view's own coordinates (the inverse of its map), scores from a small set so that ties occur, three classes.  With
    ``empty_frame`` and B > 1, frame 1 has no candidates.  Shared and never modified."""
    rng = np.random.RandomState(seed + 100 * B + V)
    S = V * B
    counts = rng.randint(5, k_in + 1, S).astype(np.int32)
    counts[0] = k_in
    if empty_frame and B > 1:
        counts[np.arange(V) * B + 1] = 0
    vmap = np.zeros((S, 4), np.float32)
    rows = np.zeros((S, k_in, 6), np.float32)
    for k in range(V):
        z, flip = VIEW_GEOMETRY[k]
        for b in range(B):
            s = k * B + b
            fh, fw = (int(v) for v in FRAME_HW[b])
            left, top = (fw - fw * z) / 2, (fh - fh * z) / 2
            vmap[s] = [-1 / z, (fw - left) / z, 1 / z, -top / z] if flip else [1 / z, -left / z, 1 / z, -top / z]
            for r in range(k_in):                                   # rows past the count are filled too: they are not candidates
                box = BASE[rng.randint(4)] + rng.randint(-6, 7, 4).astype(np.float32) * np.float32(0.75)
                x1, x2 = ((box[[0, 2]] - vmap[s, 1]) / vmap[s, 0])[::-1 if flip else 1]
                y1, y2 = (box[[1, 3]] - vmap[s, 3]) / vmap[s, 2]
                rows[s, r] = [x1, y1, x2, y2, rng.choice([0.9, 0.75, 0.5, 0.25]), rng.randint(3)]
    for a in (rows, counts, vmap):
        a.setflags(write=False)
    return rows, counts, vmap


WORD_K = 64
WORD_FRAME_HW = np.array([[140, 200]], np.int32)


@functools.lru_cache(maxsize=None)
def word_case(n):
    """n candidates of one frame, filled view by view into three views of 64: one, two and three 64-bit words per matrix row"""
    rows, _, vmap = fuse_case(1, 3, seed=11, k_in=WORD_K)
    counts = np.array([min(WORD_K, max(0, n - WORD_K * s)) for s in range(3)], np.int32)
    counts.setflags(write=False)
    return rows, counts, vmap


@functools.lru_cache(maxsize=None)
def capacity_case(extra):
    """8192 + extra disjoint candidates in frame 1 of 2, frame 0 empty: 8 views with blocks of 1025 rows, seven hold 1024 and the eighth
    1024 + extra"""
    K, rng = 1025, np.random.RandomState(5)
    k = np.arange(8 * K)
    boxes = np.stack([(k % 128) * 4, (k // 128) * 4, (k % 128) * 4 + 2, (k // 128) * 4 + 2], 1).astype(np.float32)
    rows = np.zeros((16, K, 6), np.float32)
    rows[1::2] = np.concatenate([boxes, rng.choice([0.9, 0.6, 0.3], (8 * K, 1)), np.zeros((8 * K, 1))], 1).astype(np.float32).reshape(8, K, 6)
    counts = np.zeros(16, np.int32)
    counts[1::2] = [K - 1] * 7 + [K - 1 + extra]
    vmap = np.tile(np.array([1, 0, 1, 0], np.float32), (16, 1))
    frame_hw = np.array([[10, 10], [400, 600]], np.int32)
    for a in (rows, counts, vmap, frame_hw):
        a.setflags(write=False)
    return rows, counts, vmap, frame_hw
