"""Host restatement of the VOC mAP evaluation (computervision.pytorch_amd/det_eval.py, csrc/det_eval.hip) in plain Python / numpy: the
reference's writers (core/algorithms/yolo_v8.py:286-296: ``class str(score)[:6] int(l) int(t) int(r) int(b)``) and its ``get_map`` /
``voc_ap`` (core/metrics/mAP.py:107-148, 302-834) written out literally and SEQUENTIALLY -- one loop over the sorted detections with
``used`` flags, as the reference runs it -- without the text files in between.  Nothing here touches a GPU or the package under test."""
import numpy as np

FLAG_FP, FLAG_TP, FLAG_NEITHER = 0, 1, 2


def score_text(x):
    """the writers' ``str(scores[i])[:6]`` of a float32 score"""
    return str(np.float32(x))[:6]


def undo_letterbox_f32(boxes, input_hw, image_hw, letterbox):
    """core/utils/boxes.py:undo_letterbox on (k, 4) float32 boxes (numpy float32 in-place operations with Python-float constants)"""
    box = np.asarray(boxes, dtype=np.float32).reshape(-1, 4).copy()
    in_h, in_w = (float(v) for v in input_hw)
    img_h, img_w = (float(v) for v in image_hw)
    if letterbox:
        gain = max(img_h / in_h, img_w / in_w)
        pad_top = (in_h - img_h / gain) // 2
        pad_left = (in_w - img_w / gain) // 2
        box[:, 0::2] -= pad_left
        box[:, 1::2] -= pad_top
        box *= gain
    else:
        box[:, 0::2] *= img_w / in_w
        box[:, 1::2] *= img_h / in_h
    return box


def detections_from_rows(rows, counts, quantize=True):
    """NMS rows (B, K, 6) [x1, y1, x2, y2, score, cls] with FINAL float boxes -> per image a list of (cls, score, l, t, r, b) as the
    reference reads them back from its text: float(str(score)[:6]) and int() of every coordinate."""
    out = []
    for b in range(len(counts)):
        dets = []
        for r in range(int(counts[b])):
            x1, y1, x2, y2, s, c = rows[b][r]
            if quantize:
                text = score_text(s)
                assert "e" not in text, f"score {s!r} prints in scientific notation"
                s = float(text)
            else:
                s = float(np.float32(s))
            dets.append((int(c), s, int(np.float32(x1)), int(np.float32(y1)), int(np.float32(x2)), int(np.float32(y2))))
        out.append(dets)
    return out


def ground_truth_from_arrays(gt, gt_counts):
    """(B, G, 6) [cls, l, t, r, b, difficult] -> per image a list of tuples"""
    return [[tuple(int(v) for v in gt[b][g]) for g in range(int(gt_counts[b]))] for b in range(len(gt_counts))]


def voc_ap(rec, prec):
    """mAP.py:107-148"""
    rec, prec = list(rec), list(prec)
    rec.insert(0, 0.0)
    rec.append(1.0)
    mrec = rec[:]
    prec.insert(0, 0.0)
    prec.append(0.0)
    mpre = prec[:]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    i_list = []
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            i_list.append(i)
    ap = 0.0
    for i in i_list:
        ap += ((mrec[i] - mrec[i - 1]) * mpre[i])
    return ap


def get_map(dets, gts, num_classes, min_overlap=0.5, score_threshold=0.5):
    """dets[image] = [(cls, score, l, t, r, b), ...] in row order, gts[image] = [(cls, l, t, r, b, difficult), ...] in file order; the
    images in the reference's sorted-id order.  Returns mAP, the per-class arrays of DetectionEvaluator.results(), the per-class
    (prec, rec) curves, the flag of every detection in (image, row) order, and per detection the matched ground truth and IoU."""
    n_img = len(dets)
    gt_counter = [0] * num_classes
    for boxes in gts:
        for cls, _, _, _, _, difficult in boxes:
            if not difficult:
                gt_counter[cls] += 1
    used = [[False] * len(boxes) for boxes in gts]
    flags = [[FLAG_FP] * len(d) for d in dets]
    detail = [[(-1, -1.0, 0)] * len(d) for d in dets]            # (ground truth index, ovmax, ground truths that reach ovmax)
    ap = np.zeros(num_classes)
    out = {k: np.zeros(num_classes) for k in ("precision", "recall", "f1")}
    tp_count, n_det = np.zeros(num_classes, np.int64), np.zeros(num_classes, np.int64)
    curves = []
    for c in range(num_classes):
        bounding = [(d[1], img, row) for img in range(n_img) for row, d in enumerate(dets[img]) if d[0] == c]
        bounding.sort(key=lambda x: float(x[0]), reverse=True)
        nd = len(bounding)
        n_det[c] = nd
        tp, fp = [0] * nd, [0] * nd
        thr_idx = 0
        for idx, (score, img, row) in enumerate(bounding):
            if score >= score_threshold:
                thr_idx = idx
            bb = [float(v) for v in dets[img][row][2:6]]
            ovmax, gt_match, reach = -1, -1, 0
            for g, obj in enumerate(gts[img]):
                if obj[0] == c:
                    bbgt = [float(v) for v in obj[1:5]]
                    bi = [max(bb[0], bbgt[0]), max(bb[1], bbgt[1]), min(bb[2], bbgt[2]), min(bb[3], bbgt[3])]
                    iw = bi[2] - bi[0] + 1
                    ih = bi[3] - bi[1] + 1
                    if iw > 0 and ih > 0:
                        ua = (bb[2] - bb[0] + 1) * (bb[3] - bb[1] + 1) + (bbgt[2] - bbgt[0] + 1) * (bbgt[3] - bbgt[1] + 1) - iw * ih
                        ov = iw * ih / ua
                        if ov == ovmax:
                            reach += 1
                        if ov > ovmax:
                            ovmax, gt_match, reach = ov, g, 1
            detail[img][row] = (gt_match, float(ovmax), reach)
            if ovmax >= min_overlap:
                if not gts[img][gt_match][5]:
                    if not used[img][gt_match]:
                        tp[idx] = 1
                        used[img][gt_match] = True
                        flags[img][row] = FLAG_TP
                    else:
                        fp[idx] = 1
                else:
                    flags[img][row] = FLAG_NEITHER
            else:
                fp[idx] = 1
        cumsum = 0
        for idx, val in enumerate(fp):
            fp[idx] += cumsum
            cumsum += val
        cumsum = 0
        for idx, val in enumerate(tp):
            tp[idx] += cumsum
            cumsum += val
        tp_count[c] = tp[-1] if nd else 0
        rec = [float(tp[idx]) / np.maximum(gt_counter[c], 1) for idx in range(nd)]
        prec = [float(tp[idx]) / np.maximum(fp[idx] + tp[idx], 1) for idx in range(nd)]
        ap[c] = voc_ap(rec[:], prec[:])
        if nd:
            r, p = np.array(rec), np.array(prec)
            f1 = r * p * 2 / np.where((p + r) == 0, 1, (p + r))
            out["f1"][c], out["recall"][c], out["precision"][c] = f1[thr_idx], rec[thr_idx], prec[thr_idx]
        curves.append((np.array(prec, dtype=np.float64), np.array(rec, dtype=np.float64)))
    gt_classes = [c for c in range(num_classes) if gt_counter[c] > 0]
    m = sum(ap[c] for c in gt_classes) / len(gt_classes) if gt_classes else 0.0
    res = dict(mAP=float(m), n_classes=len(gt_classes), ap=ap, tp=tp_count, n_det=n_det, n_gt=np.array(gt_counter, np.int64), **out)
    return dict(res=res, curves=curves, flags=[f for per in flags for f in per], detail=detail)


def random_case(seed, B=3, nc=4, max_det=16, G=6, size=64):
    """Seeded rows / counts / gt / gt_counts with coordinates in 0 .. size, so that ties, shared ground truths and touching boxes are
    frequent: half of the detections are a ground truth of the image moved by at most 2 pixels, scores come from a grid of 12 values."""
    rs = np.random.RandomState(seed)
    gt = np.zeros((B, G, 6), np.int32)
    gt_counts = rs.randint(0, G + 1, B).astype(np.int32)
    for b in range(B):
        for g in range(gt_counts[b]):
            l, t = rs.randint(0, size - 8, 2)
            w, h = rs.randint(1, 24, 2)
            gt[b, g] = (rs.randint(0, nc), l, t, min(l + w, size), min(t + h, size), rs.rand() < 0.25)
    rows = np.zeros((B, max_det, 6), np.float32)
    counts = rs.randint(0, max_det + 1, B).astype(np.int32)
    for b in range(B):
        for r in range(counts[b]):
            if gt_counts[b] and rs.rand() < 0.5:
                g = gt[b, rs.randint(0, gt_counts[b])]
                box = g[1:5] + rs.randint(-2, 3, 4)
                cls = g[0] if rs.rand() < 0.9 else rs.randint(0, nc)
            else:
                l, t = rs.randint(0, size - 8, 2)
                box = (l, t, l + rs.randint(1, 24), t + rs.randint(1, 24))
                cls = rs.randint(0, nc)
            rows[b, r, :4] = np.asarray(box, np.float32) + rs.rand(4).astype(np.float32) * 0.99        # int() cuts the fraction
            rows[b, r, 4] = np.float32(rs.randint(1, 13) / 12.5) if rs.rand() < 0.5 else np.float32(rs.uniform(0.001, 1.0))
            rows[b, r, 5] = cls
    return rows, counts, gt, gt_counts


def fixture_inputs(z):
    """tests/golden/det_map_ref.npz -> (dets, gts) lists for ``get_map`` and the same data as one device-shaped batch
    (rows (N, 16, 6) float32, counts, gt (N, 6, 6) int32, gt_counts): scores k / 10000 as float32, integer boxes."""
    n = int(z["n_images"])
    dets, gts = [[] for _ in range(n)], [[] for _ in range(n)]
    for img, cls, k, l, t, r, b in z["dets"].tolist():
        dets[img].append((cls, float(score_text(np.float32(k / 10000))), l, t, r, b))
    for img, cls, l, t, r, b, difficult in z["gts"].tolist():
        gts[img].append((cls, l, t, r, b, difficult))
    K, G = max(len(d) for d in dets), max(len(g) for g in gts)
    rows, gt = np.zeros((n, K, 6), np.float32), np.zeros((n, G, 6), np.int32)
    ks = [[] for _ in range(n)]
    for img, cls, k, l, t, r, b in z["dets"].tolist():
        rows[img, len(ks[img])] = (l, t, r, b, np.float32(k / 10000), cls)
        ks[img].append(k)
    for img in range(n):
        for g, box in enumerate(gts[img]):
            gt[img, g] = box
    counts = np.array([len(d) for d in dets], np.int32)
    gt_counts = np.array([len(g) for g in gts], np.int32)
    return dets, gts, (rows, counts, gt, gt_counts)
