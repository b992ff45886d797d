"""numpy restatement of csrc/tiles.hip, float32 with the kernels' operations in the kernels' order: the crop of a tile
into its slot (byte / 255, pad 128 / 255) and the merge across the slots of a frame -- one fp32 add per coordinate, the clamp to the frame,
the (score desc, ordinal asc) key, the greedy pass under IoU (oracle.nms_ref's arithmetic) or IoS."""
import numpy as np

MERGE_CAP = 8192
PAD = np.float32(128.0) / np.float32(255.0)


def tiles(jobs, slots, H, W, swap_rb=False):
    """jobs: (frame (h, w, 3) uint8, y0, x0, th, tw, out) -> (slots, 3, H, W) float32; the slots no job names are left NaN"""
    out = np.full((slots, 3, H, W), np.nan, np.float32)
    for frame, y0, x0, th, tw, slot in jobs:
        h, w = frame.shape[:2]
        out[slot] = PAD
        ys, xs = np.arange(max(min(th, H), 0)), np.arange(max(min(tw, W), 0))
        ys, xs = ys[(y0 + ys >= 0) & (y0 + ys < h)], xs[(x0 + xs >= 0) & (x0 + xs < w)]          # a bad job reads nothing outside its frame
        crop = frame[np.ix_(y0 + ys, x0 + xs)]
        if swap_rb:
            crop = crop[..., ::-1]
        out[slot][:, ys[:, None], xs[None, :]] = crop.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return out


def overlaps(box, area, others, other_areas, metric):
    """metric(box, others) in float32, every operation rounded on its own; 0 / 0 is NaN"""
    w = np.fmax(np.float32(0), np.fmin(box[2], others[:, 2]) - np.fmax(box[0], others[:, 0]))
    h = np.fmax(np.float32(0), np.fmin(box[3], others[:, 3]) - np.fmax(box[1], others[:, 1]))
    inter = (w * h).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        if metric == "iou":
            total = (area + other_areas).astype(np.float32)
            return (inter / (total - inter).astype(np.float32)).astype(np.float32)
        return (inter / np.fmin(area, other_areas)).astype(np.float32)


def merge(rows, counts, slot_map, frame_hw, metric="ios", threshold=0.5, class_agnostic=False, max_det=300):
    """rows (slots, K, 6) float32, counts (slots), slot_map (slots, 4) [frame, x0, y0, 0], frame_hw (frames, 2) ->
    (rows (frames, max_det, 6) float32, counts (frames) int32, source (frames, max_det) int32, overflow int)"""
    rows = np.asarray(rows, np.float32)
    counts, slot_map, frame_hw = np.asarray(counts, np.int64), np.asarray(slot_map, np.int64), np.asarray(frame_hw, np.int64)
    S, K = rows.shape[:2]
    F = len(frame_hw)
    thr = np.float32(threshold)
    out_rows = np.zeros((F, max_det, 6), np.float32)
    out_counts = np.zeros(F, np.int32)
    out_source = np.full((F, max_det), -1, np.int32)
    overflow = 0
    for f in range(F):
        ordinals = []
        for s in range(S):
            if slot_map[s, 0] != f:
                continue
            if counts[s] < 0 or counts[s] > K:
                overflow += 1
                continue
            ordinals += [s * K + r for r in range(int(counts[s]))]
        if len(ordinals) > MERGE_CAP:
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
        slot = ordinals // K
        fh, fw = np.float32(frame_hw[f, 0]), np.float32(frame_hw[f, 1])
        ox, oy = slot_map[slot, 1].astype(np.float32), slot_map[slot, 2].astype(np.float32)
        box = np.empty((len(cand), 4), np.float32)
        box[:, 0] = np.fmin(np.fmax(cand[:, 0] + ox, np.float32(0)), fw)
        box[:, 1] = np.fmin(np.fmax(cand[:, 1] + oy, np.float32(0)), fh)
        box[:, 2] = np.fmin(np.fmax(cand[:, 2] + ox, np.float32(0)), fw)
        box[:, 3] = np.fmin(np.fmax(cand[:, 3] + oy, np.float32(0)), fh)
        area = ((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])).astype(np.float32)
        cls = cand[:, 5]
        removed = np.zeros(len(cand), bool)
        kept = 0
        for i in range(len(cand)):
            if kept >= max_det:
                break
            if removed[i]:
                continue
            out_rows[f, kept, :4], out_rows[f, kept, 4], out_rows[f, kept, 5] = box[i], cand[i, 4], cls[i]
            out_source[f, kept] = ordinals[i]
            kept += 1
            hit = overlaps(box[i], area[i], box[i + 1:], area[i + 1:], metric) > thr          # a NaN compares false: it never suppresses
            if not class_agnostic:
                hit &= cls[i + 1:] == cls[i]
            removed[i + 1:] |= hit
        out_counts[f] = kept
    return out_rows, out_counts, out_source, overflow
