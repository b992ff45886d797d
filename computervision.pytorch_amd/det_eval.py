"""VOC mAP of a detector, accumulated on the device: the reference's ``get_map(0.5, ...)`` (core/metrics/mAP.py:302-834) without the
text files its ``evaluate_on_voc`` writers exchange with it.

``DetectionEvaluator.add_batch`` is one ``cvx_det_match`` launch per batch (csrc/det_eval.hip): it takes the NMS rows and counts as
``cvx_nms`` leaves them on the device, maps and truncates the boxes, cuts the scores to the reference's text precision, decides TP / FP /
neither per detection and appends the records to a flat device buffer.  ``results()`` orders the records once (one stable ``torch.sort`` of
an int64 key: plumbing, once per evaluation), runs ``cvx_det_ap`` and makes the only host read.

Order matters where scores tie: the reference sorts its detection files by image id before it reads them (``dr_files_list.sort()``) and
keeps that order among equal scores.  ``add_batch`` keeps (call order, image order, row order), so THE CALLER FEEDS THE IMAGES IN SORTED-ID
ORDER to reproduce the reference's tie-breaks.

Not reproduced: scores below 1e-4 (the reference's text is scientific notation there; ``results()`` raises if one was seen -- the
writers use ``conf_threshold=0.001``), the plots and ``images-optional``.  The log-average miss rate is in ``det_diag.py``, with the
confusion matrix and the confidence curves (``evaluate_detector(diagnostics=)``).
"""
import os

import numpy as np
import torch

from . import _lib as L
from . import coco_eval
from .det_records import MAX_GT, MAX_ROWS, RecordEvaluator, check_batch, default_capacity, record_order  # noqa: F401 (old import paths)

FLAG_FP, FLAG_TP, FLAG_NEITHER = 0, 1, 2


def quantize_scores(x):
    """What ``float(str(np.float32(x))[:6])`` keeps of float32 scores in [1e-4, 1], as float32 -- the rule ``cvx_det_match`` applies on the
    device, in numpy.  k = rint(x * 1e4) in fp64 (the product is exact); the text is k / 1e4 itself when that rounds back to x (a 4-decimal
    number within half an ulp of x is the shortest round-trip text), otherwise it is longer and the cut truncates: floor(x * 1e4) / 1e4."""
    x = np.asarray(x, dtype=np.float32)
    p = x.astype(np.float64) * 1e4
    k = np.rint(p)
    exact = (k / 1e4).astype(np.float32) == x
    return np.where(exact, x, (np.floor(p) / 1e4).astype(np.float32)).astype(np.float32)


def letterbox_box_map(image_hw: torch.Tensor, input_hw, letterbox: bool) -> torch.Tensor:
    """(B, 2) original (h, w) on the device -> (B, 4) float32 [px, py, gx, gy] for box-map mode 1, the constants of
    ``core.utils.boxes.undo_letterbox``: computed in fp64 as Python does, rounded to fp32 where numpy's in-place ops round them."""
    in_h, in_w = float(input_hw[0]), float(input_hw[1])
    hw = image_hw.to(torch.float64)
    img_h, img_w = hw[:, 0], hw[:, 1]
    if letterbox:
        gain = torch.maximum(img_h / in_h, img_w / in_w)
        pad_top = torch.floor((in_h - img_h / gain) / 2)
        pad_left = torch.floor((in_w - img_w / gain) / 2)
        out = torch.stack((pad_left, pad_top, gain, gain), 1)
    else:
        zero = torch.zeros_like(img_h)
        out = torch.stack((zero, zero, img_w / in_w, img_h / in_h), 1)
    return out.to(torch.float32).contiguous()


def correct_boxes_device(boxes: torch.Tensor, input_hw, image_hw: torch.Tensor, letterbox: bool) -> torch.Tensor:
    """``yolo_correct_boxes`` (core/utils/image_process.py:161-181) as the YOLOv7 / SSD wrappers' ``_correct_boxes`` run it, for a device
    batch: boxes (B, K, 4) normalised corners float32, image_hw (B, 2) -> corners in original-image pixels.  The same float32 operations in
    the same order; the per-image constants are computed in fp64, as Python computes them, and rounded to fp32 where numpy rounds them."""
    H, W = float(input_hw[0]), float(input_hw[1])
    xy = (boxes[..., 0:2] + boxes[..., 2:4]) / 2
    wh = boxes[..., 2:4] - boxes[..., 0:2]
    hw = image_hw.to(torch.float64)
    ih, iw = hw[:, 0], hw[:, 1]
    if letterbox:
        scale = torch.maximum(ih / H, iw / W)
        top = torch.floor((H - ih / scale) / 2).to(torch.float32).view(-1, 1)
        left = torch.floor((W - iw / scale) / 2).to(torch.float32).view(-1, 1)
        s = scale.to(torch.float32).view(-1, 1)
        cx, cy = xy[..., 0] * W - left, xy[..., 1] * H - top
        bw, bh = wh[..., 0] * W, wh[..., 1] * H
        return torch.stack(((cx - bw / 2) * s, (cy - bh / 2) * s, (cx + bw / 2) * s, (cy + bh / 2) * s), -1)
    out = torch.stack((xy[..., 0] - wh[..., 0] / 2, xy[..., 1] - wh[..., 1] / 2, xy[..., 0] + wh[..., 0] / 2, xy[..., 1] + wh[..., 1] / 2), -1)
    out[..., 0::2] *= iw.to(torch.float32).view(-1, 1, 1)
    out[..., 1::2] *= ih.to(torch.float32).view(-1, 1, 1)
    return out


def reverse_letterbox_device(boxes: torch.Tensor, input_hw, image_hw: torch.Tensor) -> torch.Tensor:
    """``reverse_letter_box(xywh=False)`` (core/utils/image_process.py:100-129) as ``CenterNetA._finish`` runs it, for a device batch:
    boxes (B, K, 4) normalised corners float32 -> original-image pixels, the same float32 operations in the same order."""
    H, W = input_hw[0], input_hw[1]
    nb = boxes.clone()
    nb[..., 0::2] *= W
    nb[..., 1::2] *= H
    hw = image_hw.to(torch.float64)
    scale = torch.maximum(hw[:, 0] / H, hw[:, 1] / W)
    top = torch.floor((H - hw[:, 0] / scale) / 2).to(torch.float32).view(-1, 1)
    left = torch.floor((W - hw[:, 1] / scale) / 2).to(torch.float32).view(-1, 1)
    nb[..., 0] -= left
    nb[..., 2] -= left
    nb[..., 1] -= top
    nb[..., 3] -= top
    nb *= scale.to(torch.float32).view(-1, 1, 1)
    return nb


def pack_rows(per_image, device):
    """A list of (n_i, 6) device tensors [x1, y1, x2, y2, score, cls] -> (rows (B, max n_i, 6), counts (B) int32), zero padded.  The counts
    come from the shapes, which the caller's tail has already read: no further host read."""
    n = [int(t.shape[0]) for t in per_image]
    rows = torch.zeros(len(per_image), max(n + [1]), 6, dtype=torch.float32, device=device)
    for b, t in enumerate(per_image):
        if n[b]:
            rows[b, :n[b]] = t
    return rows, torch.tensor(n, dtype=torch.int32, device=device)


class DetectionEvaluator(RecordEvaluator):
    """Device-side ``get_map``.  ``max_det``: the most rows per image a batch may carry; ``capacity``: the records the whole evaluation may
    append (images x rows).  ``quantize_scores=True`` is the reference's ``str(score)[:6]``."""
    _ENTRIES = ("cvx_det_match", "cvx_det_ap")
    _low_score_message = ("scores below 1e-4: the reference writes them in scientific notation and reads back their first 6 characters, "
                          "which is not reproduced; evaluate with conf_threshold >= 0.001")

    def __init__(self, num_classes, max_det, capacity, device, min_overlap=0.5, score_threshold=0.5, quantize_scores=True):
        super().__init__(num_classes, max_det, capacity, device)
        self.min_overlap, self.score_threshold, self.quantize = float(min_overlap), float(score_threshold), bool(quantize_scores)

    def _columns(self):
        self.rec_flag = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
        self.gt_per_class = torch.zeros(self.num_classes, dtype=torch.int64, device=self.device)
        return self.rec_flag, self.gt_per_class

    def add_batch(self, rows, counts, gt, gt_counts, box_map=None):
        """rows (B, K, 6) float32 and counts (B) int32 as ``engine.nms`` returns them (K <= max_det); gt (B, G, 6) int32
        [cls, l, t, r, b, difficult] and gt_counts (B) int32; ``box_map`` None: the boxes are final (mode 0), or (B, 4) float32
        [px, py, gx, gy] (mode 1, ``letterbox_box_map``).  One launch pair, no host read."""
        self._buffers()
        rows, counts, gt, gt_counts, box_map = check_batch(rows, counts, gt, gt_counts, box_map, self.max_det, self.rec_score.device)
        B, K, G = int(rows.shape[0]), int(rows.shape[1]), int(gt.shape[1])
        self._cache = None
        L.check(L.load().cvx_det_match(L.ptr(rows), L.ptr(counts), B, K, 0 if box_map is None else 1, L.ptr(box_map), L.ptr(gt) if G else None,
                                       L.ptr(gt_counts), G, self.num_classes, self.min_overlap, int(self.quantize), L.ptr(self.rec_score),
                                       L.ptr(self.rec_class), L.ptr(self.rec_flag), self.capacity, L.ptr(self.state), L.ptr(self.gt_per_class),
                                       L.stream_ptr(self.device)), "cvx_det_match")

    def _reduce(self):
        """Order the records as get_map does, run cvx_det_ap; everything stays on the device."""
        self._buffers()
        nc, cap, dev = self.num_classes, self.capacity, self.device
        order, cls, seg_off = record_order(self.rec_class, self.rec_score, nc)
        score, flag = self.rec_score[order].contiguous(), self.rec_flag[order].contiguous()
        prec = torch.zeros(cap, dtype=torch.float64, device=dev)
        rec = torch.zeros(cap, dtype=torch.float64, device=dev)
        stats = torch.zeros(nc * 8 + 8, dtype=torch.float64, device=dev)
        L.check(L.load().cvx_det_ap(L.ptr(score), L.ptr(flag), L.ptr(seg_off), L.ptr(self.gt_per_class), nc, self.score_threshold,
                                    int(self.quantize), L.ptr(prec), L.ptr(rec), L.ptr(stats), L.stream_ptr(dev)), "cvx_det_ap")
        return dict(order=order, cls=cls, seg_off=seg_off, score=score, flag=flag, prec=prec, rec=rec, stats=stats)

    def results(self):
        """The single host read: mAP and per class ``ap / precision / recall / f1`` (the last three at ``score_threshold``) and the counts
        ``tp / n_det / n_gt``.  Raises ``CvxError`` if a batch overflowed (NMS count -1, no room left in ``capacity``), a class index was out
        of range or a score was below 1e-4."""
        if self._cache is None:
            dev = self._reduce()
            nc = self.num_classes
            host = torch.cat((self.state.to(torch.float64), dev["stats"])).cpu().numpy()        # counters < 2^53: exact as doubles
            cursor = self._check_counters(host)
            s = host[4:4 + nc * 8].reshape(nc, 8)
            self._cache = dict(device=dev, n_records=cursor, res={
                "mAP": float(host[4 + nc * 8]), "n_classes": int(host[4 + nc * 8 + 1]),
                "ap": s[:, 0].copy(), "precision": s[:, 1].copy(), "recall": s[:, 2].copy(), "f1": s[:, 3].copy(),
                "tp": s[:, 4].astype(np.int64), "n_det": s[:, 5].astype(np.int64), "n_gt": s[:, 6].astype(np.int64)})
        return self._cache["res"]

    def device_records(self):
        """What ``_reduce`` left on the device, after ``results()`` has checked the counters: ``score`` / ``flag`` / ``prec`` / ``rec`` per
        record in get_map's order (class ascending, score descending, stable), ``seg_off`` (nc + 1) the first record of each class,
        ``order`` / ``cls`` / ``stats``.  No host read of its own; ``det_diag.DetectionDiagnostics.results`` reads its curves from these."""
        self.results()
        return self._cache["device"]

    def curves(self):
        """Per class (prec, rec) float64 arrays, one entry per detection in get_map's order (a second host read, for the report)."""
        self.results()
        dev = self._cache["device"]
        off = dev["seg_off"].cpu().numpy()
        prec, rec = dev["prec"].cpu().numpy(), dev["rec"].cpu().numpy()
        return [(prec[off[c]:off[c + 1]], rec[off[c]:off[c + 1]]) for c in range(self.num_classes)]

    def records(self):
        """(score, class, flag) numpy arrays in append order (image, row) -- for tests and debugging."""
        self.results()
        n = self._cache["n_records"]
        return self.rec_score[:n].cpu().numpy(), self.rec_class[:n].cpu().numpy(), self.rec_flag[:n].cpu().numpy()

    def write_report(self, path, class_names):
        """``results/results.txt`` as get_map writes it: the classes in name order, per class with a ground truth the AP line and the
        '%.2f' precision / recall lists, the mean, the ground-truth counts, and the detection counts of every detected class."""
        res = self.results()
        text = format_report(res, self.curves(), class_names)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
        return text


def format_report(res, curves, class_names):
    """The text of get_map's results.txt from per-class results and curves (shared with the tests' restatement)."""
    nc = len(res["ap"])
    assert len(class_names) >= nc
    by_name = sorted(range(nc), key=lambda c: class_names[c])
    out = ["# AP and precision/recall per class\n"]
    for c in by_name:
        if res["n_gt"][c] <= 0:
            continue
        prec, rec = curves[c]
        out.append("{0:.2f}%".format(res["ap"][c] * 100) + " = " + class_names[c] + " AP " + "\n Precision: " + str(['%.2f' % v for v in prec])
                   + "\n Recall :" + str(['%.2f' % v for v in rec]) + "\n\n")
    if not any(res["n_gt"][c] > 0 for c in range(nc)):
        return "".join(out)                                  # get_map returns before the other sections ("No class detected")
    out.append("\n# metrics of all classes\n")
    out.append("metrics = {0:.2f}%".format(res["mAP"] * 100) + "\n")
    out.append("\n# Number of ground-truth objects per class\n")
    for c in by_name:
        if res["n_gt"][c] > 0:
            out.append(class_names[c] + ": " + str(int(res["n_gt"][c])) + "\n")
    out.append("\n# Number of detected objects per class\n")
    for c in by_name:
        if res["n_det"][c] > 0:
            tp = int(res["tp"][c]) if res["n_gt"][c] > 0 else 0
            out.append(class_names[c] + ": " + str(int(res["n_det"][c])) + " (tp:" + str(tp) + ", fp:" + str(int(res["n_det"][c]) - tp) + ")\n")
    return "".join(out)


def class_names(dataset_cfg, num_classes):
    """The dataset's class names when it has ``num_classes`` of them (VOC), otherwise the indices as text"""
    names = list(dataset_cfg.get("classes", []))
    return names if len(names) == num_classes else [str(c) for c in range(num_classes)]


def evaluate_detector(evaluator_rows, dataloader, num_classes, device, map_out_root, class_names, max_det, capacity=None, coco_metric=False,
                      diagnostics=None):
    """The loop the four ``evaluate_on_voc`` methods share.  ``evaluator_rows(images, meta)`` -> (rows, counts, box_map or None) on the
    device.  ``capacity`` defaults to batches x batch size x min(max_det, 1024) records.  Writes ``<map_out_root>/results/results.txt`` and
    returns the ``results()`` dict.  ``coco_metric``: the same pass also feeds a ``CocoEvaluator`` what ``get_coco_map`` (mAP.py:930-959)
    reads from the writers' text files -- truncated boxes, cut scores, the ground truth as ``preprocess_gt`` converts it; its results are
    the ``"coco"`` entry and its twelve lines go to ``<map_out_root>/coco_results.txt``.  ``diagnostics``: a ``det_diag.DetDiagnostics`` --
    the same rows also feed a ``DetectionDiagnostics`` (one more launch per batch); its results are the ``"diagnostics"`` entry and its
    three files go to ``<map_out_root>/results/``.  With None nothing of it is allocated or launched."""
    if diagnostics is not None:
        from . import det_diag
        if not isinstance(diagnostics, det_diag.DetDiagnostics):
            raise ValueError(f"diagnostics: a det_diag.DetDiagnostics or None, got {type(diagnostics).__name__}")
    ev = coco = diag = None
    for images, meta in dataloader:
        rows, counts, box_map = evaluator_rows(images, meta)
        if ev is None:
            if capacity is None:
                capacity = default_capacity(dataloader, rows.shape[0], max_det, "evaluate_on_voc")
            ev = DetectionEvaluator(num_classes, max_det, capacity, rows.device)
            if coco_metric:
                coco = coco_eval.CocoEvaluator(num_classes, max_det, capacity, rows.device, truncate_boxes=True, quantize_scores=True)
            if diagnostics is not None:
                diag = det_diag.DetectionDiagnostics(num_classes, max_det, rows.device, diagnostics)
        ev.add_batch(rows, counts, meta["gt"], meta["gt_counts"], box_map)
        if diag is not None:
            diag.add_batch(rows, counts, meta["gt"], meta["gt_counts"], box_map)
        if coco is not None:
            coco.add_batch(rows, counts, coco_eval.voc_gt_to_coco(meta["gt"]), meta["gt_counts"], box_map)
    if ev is None:
        raise L.CvxError("evaluate_on_voc: the dataloader yielded no batch")
    res = ev.results()
    ev.write_report(os.path.join(map_out_root, "results", "results.txt"), class_names)
    print("metrics = {0:.2f}%".format(res["mAP"] * 100))
    if coco is not None:
        res = dict(res, coco=coco.results())
        coco_eval.write_summary(coco, map_out_root)
    if diag is not None:
        res = dict(res, diagnostics=diag.results(ev))
        diag.write_report(os.path.join(map_out_root, "results"), class_names)
        print("recommended conf_threshold = {0:.4f}".format(res["diagnostics"]["best_conf"]))
    return res
