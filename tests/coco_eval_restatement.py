"""Host restatement of pycocotools' ``COCOeval(cocoGt, cocoDt, 'bbox')`` -- ``evaluate()``, ``accumulate()``, ``summarize()`` -- in plain
sequential numpy, for the device COCO metric (computervision.pytorch_amd/coco_eval.py, csrc/coco_eval.hip).  pycocotools is not
installed where this project is built, so this file IS the reference the kernels are held to; tests/test_coco_eval_cpu.py holds it to
answers derived by hand.  It is written loop by loop, as pycocotools runs, and calls ``evaluate_img`` once per maxDet.  Nothing here
touches a GPU or the package under test.

Ground truth: dicts with ``image``, ``category``, ``bbox`` [x, y, w, h] (doubles), ``area``, ``iscrowd``; ids are 1 .. N in list order
(the reference's ``preprocess_gt`` numbers them from 0, which makes pycocotools read a match with annotation 0 as "unmatched": not
reproduced).  Detections: dicts with ``image``, ``category``, ``bbox``, ``score``; area = w * h, ids 1 .. N in list order."""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)            # as they come out: not exact multiples of 0.05
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
AREA_LBL = ["all", "small", "medium", "large"]


def bbox_iou(d, g, crowd):
    """maskApi's bbIou for one pair, in doubles"""
    dx, dy, dw, dh = (float(v) for v in d)
    gx, gy, gw, gh = (float(v) for v in g)
    w = min(dx + dw, gx + gw) - max(dx, gx)
    if w <= 0:
        return 0.0
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if h <= 0:
        return 0.0
    i = w * h
    u = dw * dh if crowd else dw * dh + gw * gh - i
    return i / u


def compute_iou(gt, dt):
    """COCOeval.computeIoU of one (image, category): detections by -score (stable), the first 100; (D, G) doubles"""
    if len(gt) == 0 and len(dt) == 0:
        return []
    inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in inds][:MAX_DETS[-1]]
    ious = np.zeros((len(dt), len(gt)))
    for j, d in enumerate(dt):
        for k, g in enumerate(gt):
            ious[j, k] = bbox_iou(d["bbox"], g["bbox"], int(g["iscrowd"]))
    return ious


def evaluate_img(gt, dt, ious, a_rng, max_det):
    """COCOeval.evaluateImg of one (image, category, area range, maxDet); None when the pair is empty"""
    if len(gt) == 0 and len(dt) == 0:
        return None
    g_ignore = [1 if (g["iscrowd"] or g["area"] < a_rng[0] or g["area"] > a_rng[1]) else 0 for g in gt]
    gtind = np.argsort(g_ignore, kind="mergesort")
    gt = [gt[i] for i in gtind]
    dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
    dt = [dt[i] for i in dtind[:max_det]]
    iscrowd = [int(g["iscrowd"]) for g in gt]
    ious = ious[:, gtind] if len(ious) > 0 else ious
    T, G, D = len(IOU_THRS), len(gt), len(dt)
    gtm = np.zeros((T, G), np.int64)
    dtm = np.zeros((T, D), np.int64)
    gt_ig = np.array([g_ignore[i] for i in gtind], np.int64)
    dt_ig = np.zeros((T, D), np.int64)
    if len(ious) > 0:
        for tind, t in enumerate(IOU_THRS):
            for dind in range(D):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = gt_ig[m]
                dtm[tind, dind] = gt[m]["id"]
                gtm[tind, m] = dt[dind]["id"]
    a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, D))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return dict(dt_ids=[d["id"] for d in dt], dt_matches=dtm, gt_matches=gtm, dt_scores=[d["score"] for d in dt], gt_ignore=gt_ig,
                dt_ignore=dt_ig, gt_ids=[g["id"] for g in gt])


def prepare(gts, dts):
    """ids, areas and the (image, category) lists, as COCO.loadRes and COCOeval._prepare leave them"""
    gts = [dict(g, id=i + 1, ignore=int(g["iscrowd"])) for i, g in enumerate(gts)]
    dts = [dict(d, id=i + 1, area=float(d["bbox"][2]) * float(d["bbox"][3])) for i, d in enumerate(dts)]
    by_gt, by_dt = {}, {}
    for g in gts:
        by_gt.setdefault((g["image"], g["category"]), []).append(g)
    for d in dts:
        by_dt.setdefault((d["image"], d["category"]), []).append(d)
    return by_gt, by_dt


def evaluate(gts, dts, images, num_classes):
    """COCOeval.evaluate: eval_imgs[k][a][m][i] for the images in ascending id order"""
    by_gt, by_dt = prepare(gts, dts)
    images = sorted(images)
    out = []
    for k in range(num_classes):
        ious = {i: compute_iou(by_gt.get((i, k), []), by_dt.get((i, k), [])) for i in images}
        out.append([[[evaluate_img(by_gt.get((i, k), []), by_dt.get((i, k), []), ious[i], a_rng, m) for i in images]
                     for m in MAX_DETS] for a_rng in AREA_RNG])
    return out


def accumulate(eval_imgs, num_classes):
    """COCOeval.accumulate -> precision (T, R, K, A, M), recall (T, K, A, M), npig (K, A)"""
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), num_classes, len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    npig_all = np.zeros((K, A), np.int64)
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(MAX_DETS):
                E = [e for e in eval_imgs[k][a][m] if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["dt_scores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dtm = np.concatenate([e["dt_matches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dt_ignore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gt_ignore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                npig_all[k, a] = npig
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, REC_THRS, side="left")
                    for ri, pi in enumerate(inds_r):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall, npig_all


SUMMARY = [(1, None, "all", 100), (1, .5, "all", 100), (1, .75, "all", 100), (1, None, "small", 100), (1, None, "medium", 100),
           (1, None, "large", 100), (0, None, "all", 1), (0, None, "all", 10), (0, None, "all", 100), (0, None, "small", 100),
           (0, None, "medium", 100), (0, None, "large", 100)]


def summarize(precision, recall):
    """COCOeval.summarize -> (stats (12), the twelve printed lines)"""
    stats, lines = np.zeros(12), []
    for n, (ap, iou_thr, area, max_det) in enumerate(SUMMARY):
        a, m = AREA_LBL.index(area), MAX_DETS.index(max_det)
        s = precision if ap == 1 else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, a, m] if ap == 1 else s[:, :, a, m]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        stats[n] = mean_s
        lines.append(summary_line(ap, iou_thr, area, max_det, mean_s))
    return stats, lines


def summary_line(ap, iou_thr, area, max_det, value):
    fmt = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
    title = 'Average Precision' if ap == 1 else 'Average Recall'
    kind = '(AP)' if ap == 1 else '(AR)'
    iou = '{:0.2f}:{:0.2f}'.format(IOU_THRS[0], IOU_THRS[-1]) if iou_thr is None else '{:0.2f}'.format(iou_thr)
    return fmt.format(title, kind, iou, area, max_det, value)


def coco_eval(gts, dts, images, num_classes):
    """The whole thing -> dict(stats, lines, precision, recall, npig, eval_imgs)"""
    eval_imgs = evaluate(gts, dts, images, num_classes)
    precision, recall, npig = accumulate(eval_imgs, num_classes)
    stats, lines = summarize(precision, recall)
    return dict(stats=stats, lines=lines, precision=precision, recall=recall, npig=npig, eval_imgs=eval_imgs)


def detection_masks(eval_imgs, dts, num_classes):
    """Per detection (list order) the rank within its (image, category) list and the 40-bit matched / ignored masks (bit a * 10 + t) of
    the maxDet = 100 evaluation: what ``cvx_coco_match`` records.  A detection past the first 100 has rank >= 100 and empty masks."""
    n = len(dts)
    rank, matched, ignored = np.full(n, -1, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    per = {}
    for i, d in enumerate(dts):
        per.setdefault((d["image"], d["category"]), []).append(i)
    for idx in per.values():
        order = np.argsort([-dts[i]["score"] for i in idx], kind="mergesort")
        for r, j in enumerate(order):
            rank[idx[j]] = r
    M = MAX_DETS.index(100)
    for k in range(num_classes):
        for a in range(len(AREA_RNG)):
            for e in eval_imgs[k][a][M]:
                if e is None:
                    continue
                for j, did in enumerate(e["dt_ids"]):
                    for t in range(len(IOU_THRS)):
                        if e["dt_matches"][t, j]:
                            matched[did - 1] |= 1 << (a * 10 + t)
                        if e["dt_ignore"][t, j]:
                            ignored[did - 1] |= 1 << (a * 10 + t)
    return rank, matched, ignored


# ---- the conversions around the COCOeval call -------------------------------------------------------------------------------------------
def voc_to_coco_gt(gts):
    """``preprocess_gt`` (core/metrics/mAP.py:837-902) on per-image lists of (cls, l, t, r, b, difficult): xywh from the corners as
    doubles, area = w * h - 10, iscrowd = difficult (categories as indices, images as indices)"""
    out = []
    for img, per in enumerate(gts):
        for cls, l, t, r, b, difficult in per:
            l, t, r, b = float(l), float(t), float(r), float(b)
            out.append(dict(image=img, category=int(cls), bbox=[l, t, r - l, b - t], area=(r - l) * (b - t) - 10.0, iscrowd=int(difficult)))
    return out


def voc_to_coco_dt(dets):
    """``preprocess_dr`` (:905-927) on per-image lists of (cls, score, l, t, r, b) as the text files hold them"""
    out = []
    for img, per in enumerate(dets):
        for cls, score, l, t, r, b in per:
            l, t, r, b = float(l), float(t), float(r), float(b)
            out.append(dict(image=img, category=int(cls), bbox=[l, t, r - l, b - t], score=float(score)))
    return out


def detections_from_rows(rows, counts, truncate=False, quantize=False):
    """NMS rows (B, K, 6) [x1, y1, x2, y2, score, cls] float32 with FINAL boxes -> the detection list the reference's ``evaluate_on_coco``
    writers make of them: ``[float(left), float(top), float(right - left), float(bottom - top)]`` on numpy float32 (the differences are
    taken in float32), ``float(score)``.  ``truncate`` / ``quantize``: the VOC writers' ``int()`` and ``str(score)[:6]`` first."""
    out = []
    for b in range(len(counts)):
        for r in range(int(counts[b])):
            x1, y1, x2, y2, s, c = (np.float32(v) for v in rows[b][r])
            if truncate:
                x1, y1, x2, y2 = (np.float32(int(v)) for v in (x1, y1, x2, y2))
            if quantize:
                text = str(s)[:6]
                assert "e" not in text, f"score {s!r} prints in scientific notation"
                s = np.float32(float(text))
            out.append(dict(image=b, category=int(c), bbox=[float(x1), float(y1), float(x2 - x1), float(y2 - y1)], score=float(s)))
    return out


def ground_truth_from_arrays(gt, gt_counts):
    """(B, G, 7) float64 [cls, x, y, w, h, area, iscrowd] -> the annotation list"""
    return [dict(image=b, category=int(gt[b][g][0]), bbox=[float(v) for v in gt[b][g][1:5]], area=float(gt[b][g][5]), iscrowd=int(gt[b][g][6]))
            for b in range(len(gt_counts)) for g in range(int(gt_counts[b]))]


def arrays_from_lists(gts, dts, n_images):
    """annotation / detection lists -> one device-shaped batch: rows (N, K, 6) float32 [x, y, x + w, y + h, score, cls], counts, gt
    (N, G, 7) float64, gt_counts.  Only for lists whose corners and scores are float32 values with x + w exact (the fixture's are)."""
    per_d, per_g = [[] for _ in range(n_images)], [[] for _ in range(n_images)]
    for d in dts:
        per_d[d["image"]].append(d)
    for g in gts:
        per_g[g["image"]].append(g)
    K, G = max(1, max(len(p) for p in per_d)), max(1, max(len(p) for p in per_g))
    rows, gt = np.zeros((n_images, K, 6), np.float32), np.zeros((n_images, G, 7), np.float64)
    for i in range(n_images):
        for r, d in enumerate(per_d[i]):
            x, y, w, h = d["bbox"]
            row = np.array([x, y, x + w, y + h, d["score"], d["category"]], np.float32)
            assert float(row[2] - row[0]) == w and float(row[3] - row[1]) == h and float(row[0]) == x and float(row[1]) == y, d
            assert float(row[4]) == d["score"], d
            rows[i, r] = row
        for j, g in enumerate(per_g[i]):
            gt[i, j] = [g["category"]] + list(g["bbox"]) + [g["area"], g["iscrowd"]]
    counts = np.array([len(p) for p in per_d], np.int32)
    gt_counts = np.array([len(p) for p in per_g], np.int32)
    return rows, counts, gt, gt_counts


def fixture_lists(z):
    """tests/golden/coco_inputs_ref.npz -> (gts, dts, n_images) of the COCO-style cases (images 0 .. n - 1, in (image, row) order)"""
    gts = [dict(image=int(r[0]), category=int(r[1]), bbox=[float(v) for v in r[2:6]], area=float(r[6]), iscrowd=int(r[7])) for r in z["coco_gt"]]
    dts = [dict(image=int(r[0]), category=int(r[1]), bbox=[float(v) for v in r[2:6]], score=float(r[6])) for r in z["coco_dt"]]
    return gts, dts, int(z["coco_n_images"])
