"""Host restatement of the detector diagnostics (computervision.pytorch_amd/det_diag.py, csrc/det_diag.hip) in plain sequential Python /
numpy: the confusion matrix rule (the project's statement of Ultralytics' ``ConfusionMatrix.process_batch`` with the ties decided), the
confidence curves with their mean, smoothing and arg max -- one numpy operation per rounding -- and the miss rates of the reference's
``log_average_miss_rate`` (core/metrics/mAP.py:34-70).  Nothing here touches a GPU or the package under test.

THE CONFUSION RULE, per image, with ``nc`` classes, a confidence ``conf`` and an overlap threshold ``iou``:

1. A detection is (cls, score, l, t, r, b) as the evaluation reads it back from the writers' text: integer corners, and the score
   ``float(str(score)[:6])`` (or the float32 itself without quantisation).  A class outside [0, nc) is counted as bad and the box takes
   part in nothing, for a detection or a ground truth.  A detection takes part only if ``score >= conf``; the others count nowhere.
2. The overlap of a detection and a ground truth of ANY class is ``iw * ih / ua`` on integers with the +1 pixel convention (one
   division), 0 when they do not meet.  A pair is a candidate when ``overlap > iou``.
3. Each detection chooses its candidate of largest overlap, the lowest ground-truth index on a tie.  Difficult ground truths are
   candidates too.
4. A detection that chose a difficult ground truth counts nowhere.
5. Each non-difficult ground truth keeps one winner among the detections that chose it: the largest overlap, the lowest row on a tie.
   The winner adds 1 to ``confusion[cls_det, cls_gt]``.
6. Every other detection that takes part adds 1 to ``confusion[cls_det, nc]`` -- no candidate, or it lost its ground truth; a loser is
   NOT tried on its second choice.  Every non-difficult ground truth without a winner adds 1 to ``confusion[nc, cls_gt]``.
7. ``images_per_class[c]`` counts the images with at least one non-difficult ground truth of ``c``."""
import math

import numpy as np

FLAG_FP = 0
REF_POINTS = np.logspace(-2.0, 0.0, num=9)


def overlap(det_box, gt_box):
    l, t, r, b = det_box
    gl, gt, gr, gb = gt_box
    iw = min(r, gr) - max(l, gl) + 1
    ih = min(b, gb) - max(t, gt) + 1
    if iw <= 0 or ih <= 0:
        return 0.0
    ua = (r - l + 1) * (b - t + 1) + (gr - gl + 1) * (gb - gt + 1) - iw * ih
    return iw * ih / ua


def confusion(dets, gts, nc, conf=0.25, iou=0.45):
    """dets[image] = [(cls, score, l, t, r, b), ...] in row order, gts[image] = [(cls, l, t, r, b, difficult), ...].  Returns the matrix
    (nc + 1, nc + 1) int64 [predicted, true], images_per_class, the bad class indices, and what the tests count: detections below
    ``conf``, dropped for a difficult choice, matched off the diagonal, that lost their ground truth, and ties met."""
    m = np.zeros((nc + 1, nc + 1), np.int64)
    images = np.zeros(nc, np.int64)
    seen = dict(bad_class=0, below_conf=0, difficult_choice=0, off_diagonal=0, lost=0, gt_tie=0, row_tie=0)
    for det, gt in zip(dets, gts):
        valid_gt = []
        for g, obj in enumerate(gt):
            if 0 <= obj[0] < nc:
                valid_gt.append(g)
            else:
                seen["bad_class"] += 1
        for c in sorted({gt[g][0] for g in valid_gt if not gt[g][5]}):
            images[c] += 1
        chosen = {}                                                    # ground truth -> [(overlap, row)]
        took_part = []
        for row, d in enumerate(det):
            if not 0 <= d[0] < nc:
                seen["bad_class"] += 1
                continue
            if not d[1] >= conf:
                seen["below_conf"] += 1
                continue
            best, best_ov = -1, iou
            for g in valid_gt:
                ov = overlap(d[2:6], gt[g][1:5])
                if ov > iou and ov == best_ov:
                    seen["gt_tie"] += 1
                if ov > best_ov:
                    best, best_ov = g, ov
            if best >= 0 and gt[best][5]:
                seen["difficult_choice"] += 1
                continue
            took_part.append(row)
            if best >= 0:
                chosen.setdefault(best, []).append((best_ov, row))
        winners = {}
        for g, cands in chosen.items():
            top = max(ov for ov, _ in cands)
            rows_at_top = [row for ov, row in cands if ov == top]
            seen["row_tie"] += len(rows_at_top) > 1
            seen["lost"] += len(cands) - 1
            winners[min(rows_at_top)] = g
        for row in took_part:
            if row in winners:
                g = winners[row]
                m[det[row][0], gt[g][0]] += 1
                seen["off_diagonal"] += det[row][0] != gt[g][0]
            else:
                m[det[row][0], nc] += 1
        for g in valid_gt:
            if not gt[g][5] and g not in winners.values():
                m[nc, gt[g][0]] += 1
    return dict(confusion=m, images_per_class=images, **seen)


def score_value(score, quantize):
    """the fp64 number a float32 record score is compared by: the 4-decimal text's value when quantised"""
    s = np.asarray(score, np.float32).astype(np.float64)
    return np.rint(s * 1e4) / 1e4 if quantize else s


def smooth(y, window):
    """moving average with edge replication; the sum runs in ascending j"""
    y = np.asarray(y, np.float64)
    n = len(y)
    total = np.zeros(n)
    for j in range(window):
        total = total + y[np.clip(np.arange(n) - window // 2 + j, 0, n - 1)]
    return total / float(window)


def first_max(y):
    best = 0
    for i in range(1, len(y)):
        if y[i] > y[best]:
            best = i
    return best


def conf_curves(records, gt_per_class, points, window, quantize=True):
    """records[c] = (score float32, prec, rec, flag) of class c in get_map's order (score descending).  The step function: at x_k the
    precision / recall of the last record that reaches x_k."""
    nc = len(records)
    grid = np.arange(points).astype(np.float64) / float(points - 1)
    p, r = np.ones((nc, points)), np.zeros((nc, points))
    for c, (score, prec, rec, _) in enumerate(records):
        value = score_value(score, quantize)
        for k in range(points):
            n_k = int(np.count_nonzero(value >= grid[k]))
            if n_k:
                p[c, k], r[c, k] = prec[n_k - 1], rec[n_k - 1]
    f1 = r * p * 2 / np.where((p + r) == 0, 1, (p + r))
    with_gt = [c for c in range(nc) if gt_per_class[c] > 0]
    mean = np.zeros(points)
    for c in with_gt:
        mean = mean + f1[c]
    if with_gt:
        mean = mean / float(len(with_gt))
    mean_smooth = smooth(mean, window)
    best_per_class = np.array([first_max(smooth(f1[c], window)) for c in range(nc)], np.int64)
    return dict(conf_grid=grid, precision=p, recall=r, f1=f1, mean_f1=mean, mean_f1_smooth=mean_smooth, best_index=first_max(mean_smooth),
                best_index_per_class=best_per_class)


def fp_cumsum(flag):
    """the running count of FLAG_FP records: get_map's ``fp`` after its cumulative sum"""
    return np.cumsum(np.asarray(flag) == FLAG_FP).astype(np.int64)


def miss_rates(rec, fp_cum, n_images):
    """the nine values ``log_average_miss_rate`` averages, for one class: rec and the running FP count per record in get_map's order"""
    rec = np.asarray(rec, np.float64)
    out = np.ones(len(REF_POINTS))
    if len(rec) == 0 or n_images <= 0:
        return out
    fppi = np.asarray(fp_cum, np.int64) / float(n_images)
    mr = 1 - rec
    for i, ref in enumerate(REF_POINTS):
        at = np.where(fppi <= ref)[0]
        if len(at):
            out[i] = mr[at[-1]]
    return out


def lamr(mr9, n_records, n_images):
    """0 for a class without a record (as the reference returns), nan for a class no image holds"""
    if n_images <= 0:
        return float("nan")
    if n_records == 0:
        return 0.0
    return math.exp(np.mean(np.log(np.maximum(1e-10, mr9))))


def flags_per_class(dets, flags, nc):
    """the flat (image, row) flags of ``det_eval_restatement.get_map`` -> per class in its order (score descending, stable)"""
    out, i = [], 0
    flat = []
    for img, per in enumerate(dets):
        for row, d in enumerate(per):
            flat.append((d[0], d[1], flags[i]))
            i += 1
    for c in range(nc):
        mine = [(s, f) for cls, s, f in flat if cls == c]
        mine.sort(key=lambda x: float(x[0]), reverse=True)
        out.append(np.array([f for _, f in mine], np.int64))
    return out


def scores_per_class(dets, nc):
    out = []
    for c in range(nc):
        mine = [d[1] for per in dets for d in per if d[0] == c]
        mine.sort(key=float, reverse=True)
        out.append(np.array(mine, np.float64))
    return out


def planted_case():
    """One image, nc = 3, conf 0.25, iou 0.45, holding every case the confusion rule distinguishes, and the matrix derived by hand.

    ground truths                                   detections (row: class, score, box)
    g0 (0; 10,10,19,19)                             r0 (0, .90; 12,10,21,19)    80 / 120 with g0 AND with g1: the lower index, g0 -> [0, 0]
    g1 (0; 14,10,23,19)   nobody's choice           r1 (1, .80; 40,40,49,49)    on g2, the lower row of two                      -> [1, 1]
    g2 (1; 40,40,49,49)                             r2 (1, .95; 40,40,49,49)    the same box, a HIGHER score, the higher row     -> [1, bg]
    g3 (2; 60,10,69,19)   difficult                 r3 (2, .70; 60,10,69,19)    chose the difficult g3                           -> nowhere
    g4 (2; 60,40,69,49)                             r4 (0, .10; 10,10,19,19)    below conf (it would take g0 from r0 otherwise)  -> nowhere
    A  (0; 10,110,29,129)                           r5 (1, .60; 60,40,69,49)    on g4, of class 2                                -> [1, 2]
    B  (1; 20,110,39,129)                           r6 (0, .90; 10,110,29,129)  A's box                                          -> [0, 0]
                                                    r7 (1, .90; 14,110,33,129)  320 / 480 with A, 280 / 520 with B: chooses A, loses
                                                                                to r6 and is NOT given B                         -> [1, bg]
                                                    r8 (2, .50; 200,200,210,210) overlaps nothing                                -> [2, bg]
    missed: g1 -> [bg, 0], B -> [bg, 1]; the difficult g3 is not counted.  A greedy one-to-one matching would give B to r7: [1, 1] = 2."""
    gt = np.array([[[0, 10, 10, 19, 19, 0], [0, 14, 10, 23, 19, 0], [1, 40, 40, 49, 49, 0], [2, 60, 10, 69, 19, 1], [2, 60, 40, 69, 49, 0],
                    [0, 10, 110, 29, 129, 0], [1, 20, 110, 39, 129, 0]]], np.int32)
    rows = np.array([[[12, 10, 21, 19, .90, 0], [40, 40, 49, 49, .80, 1], [40, 40, 49, 49, .95, 1], [60, 10, 69, 19, .70, 2], [10, 10, 19, 19, .10, 0],
                      [60, 40, 69, 49, .60, 1], [10, 110, 29, 129, .90, 0], [14, 110, 33, 129, .90, 1], [200, 200, 210, 210, .50, 2]]], np.float32)
    want = np.array([[2, 0, 0, 0],
                     [0, 1, 1, 2],
                     [0, 0, 0, 1],
                     [1, 1, 0, 0]], np.int64)
    return (rows, np.array([9], np.int32), gt, np.array([7], np.int32)), want, np.array([1, 1, 1], np.int64)


def seeded_case(seed, B, nc, K, G, size=96, counts=None, gt_counts=None):
    """Seeded rows (B, K, 6) / counts / gt (B, G, 6) / gt_counts: every slot is filled, so the counts may be set freely afterwards.  Two
    thirds of the detections are a ground truth of their image moved by at most 2 pixels (nine in ten of those with its class), scores
    come half from a grid of 12 values and half from [0.001, 1); one ground truth in four is difficult."""
    rs = np.random.RandomState(seed)
    gt = np.zeros((B, G, 6), np.int32)
    lt = rs.randint(0, size - 8, (B, G, 2))
    gt[..., 0] = rs.randint(0, nc, (B, G))
    gt[..., 1:3] = lt
    gt[..., 3:5] = np.minimum(lt + rs.randint(1, 24, (B, G, 2)), size)
    gt[..., 5] = rs.rand(B, G) < 0.25
    rows = np.zeros((B, K, 6), np.float32)
    lt = rs.randint(0, size - 8, (B, K, 2))
    box = np.concatenate((lt, lt + rs.randint(1, 24, (B, K, 2))), 2)
    cls = rs.randint(0, nc, (B, K))
    if G:
        pick = rs.randint(0, G, (B, K))
        near = rs.rand(B, K) < 0.66
        own = np.take_along_axis(gt, pick[..., None], 1)
        box = np.where(near[..., None], own[..., 1:5] + rs.randint(-2, 3, (B, K, 4)), box)
        cls = np.where(near & (rs.rand(B, K) < 0.9), own[..., 0], cls)
    rows[..., :4] = box.astype(np.float32) + rs.rand(B, K, 4).astype(np.float32) * 0.99
    rows[..., 4] = np.where(rs.rand(B, K) < 0.5, (rs.randint(1, 13, (B, K)) / 12.5).astype(np.float32),
                            rs.uniform(0.001, 1.0, (B, K)).astype(np.float32))
    rows[..., 5] = cls
    counts = rs.randint(0, K + 1, B).astype(np.int32) if counts is None else np.asarray(counts, np.int32)
    gt_counts = rs.randint(0, G + 1, B).astype(np.int32) if gt_counts is None else np.asarray(gt_counts, np.int32)
    return rows, counts, gt, gt_counts
