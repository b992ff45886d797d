"""The COCO detection metric (AP@[.5:.95], AP50, AP75, APs/m/l, AR1/10/100, ARs/m/l) of a detector, accumulated on the device:
pycocotools' ``COCOeval(cocoGt, cocoDt, 'bbox')`` as the reference calls it (``get_coco_map``, core/metrics/mAP.py:930-959, and every
detector's ``evaluate_on_coco``), without the JSON files in between.  pycocotools is not a dependency: the algorithm is restated in
tests/coco_eval_restatement.py and the kernels are held to that restatement bit for bit.

``CocoEvaluator.add_batch`` is one ``cvx_coco_match`` launch per batch (csrc/coco_eval.hip): it takes the NMS rows and counts as
``cvx_nms`` leaves them on the device, orders each image's rows by class and score, cuts each class to 100 and runs COCOeval's greedy
matching for the 4 area ranges x 10 IoU thresholds.  ``results()`` orders the records once (one stable ``torch.sort``), runs
``cvx_coco_accumulate`` and ``cvx_coco_summarize`` and makes the only host read.

Order matters where scores tie: COCOeval visits the images in ascending id order and keeps that order among equal scores.  ``add_batch``
keeps (call order, image order, row order), so THE CALLER FEEDS THE IMAGES IN SORTED-ID ORDER.

Classes are indices: category ids and the annotation JSON stay outside.  Not reproduced: the reference's ``preprocess_gt`` numbers the
annotations from 0 in ``os.listdir`` order, which makes pycocotools read a match with annotation 0 as "unmatched" -- which annotation
that is depends on the directory order.  Here every match counts.
"""
import os

import numpy as np
import torch

from . import _lib as L
from .det_records import MAX_GT, MAX_ROWS, RecordEvaluator, check_batch, default_capacity, record_order  # noqa: F401 (old import paths)

IOU_THRS = np.linspace(.5, .95, 10)         # the doubles as numpy makes them: not exact multiples of 0.05
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_LABELS = ("all", "small", "medium", "large")
# (AP?, IoU text, area, maxDets) of the twelve numbers, pycocotools' order
SUMMARY = ((1, "0.50:0.95", "all", 100), (1, "0.50", "all", 100), (1, "0.75", "all", 100), (1, "0.50:0.95", "small", 100),
           (1, "0.50:0.95", "medium", 100), (1, "0.50:0.95", "large", 100), (0, "0.50:0.95", "all", 1), (0, "0.50:0.95", "all", 10),
           (0, "0.50:0.95", "all", 100), (0, "0.50:0.95", "small", 100), (0, "0.50:0.95", "medium", 100), (0, "0.50:0.95", "large", 100))


def summary_lines(stats):
    """The twelve lines COCOeval.summarize prints"""
    fmt = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
    return [fmt.format('Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', iou, area, max_det, float(v))
            for (ap, iou, area, max_det), v in zip(SUMMARY, stats)]


def voc_gt_to_coco(gt: torch.Tensor) -> torch.Tensor:
    """(B, G, 6) int32 [cls, l, t, r, b, difficult] -> (B, G, 7) float64 [cls, x, y, w, h, area, iscrowd] as ``preprocess_gt``
    (core/metrics/mAP.py:871-876) converts the VOC text: xywh from the corners, area = w * h - 10, iscrowd = difficult"""
    g = gt.to(torch.float64)
    w, h = g[..., 3] - g[..., 1], g[..., 4] - g[..., 2]
    return torch.stack((g[..., 0], g[..., 1], g[..., 2], w, h, w * h - 10.0, g[..., 5]), -1).contiguous()


class CocoEvaluator(RecordEvaluator):
    """Device-side ``COCOeval``.  ``max_det``: the most rows per image a batch may carry; ``capacity``: the records the whole evaluation
    may append (images x rows).  ``truncate_boxes`` / ``quantize_scores``: the VOC writers' ``int()`` and ``str(score)[:6]``, for the
    metric ``get_coco_map`` computes from their text files."""
    _ENTRIES = ("cvx_coco_match", "cvx_coco_accumulate")
    _low_score_message = ("unusable scores: below 1e-4 with quantize_scores (the reference writes them in scientific notation and reads back "
                          "their first 6 characters), negative or NaN without")

    def __init__(self, num_classes, max_det, capacity, device, truncate_boxes=False, quantize_scores=False):
        super().__init__(num_classes, max_det, capacity, device)
        self.truncate, self.quantize = bool(truncate_boxes), bool(quantize_scores)

    def _columns(self):
        dev, cap = self.device, self.capacity
        self.rec_rank = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.rec_matched = torch.zeros(cap, dtype=torch.int64, device=dev)
        self.rec_ignored = torch.zeros(cap, dtype=torch.int64, device=dev)
        self.npig = torch.zeros(self.num_classes, 4, dtype=torch.int64, device=dev)
        # pinned and kept: the two copies do not wait on the host (the first batch of an evaluation allocates here)
        self._thrs_host = (torch.from_numpy(IOU_THRS).pin_memory(), torch.from_numpy(REC_THRS).pin_memory())
        self.iou_thrs = self._thrs_host[0].to(dev, non_blocking=True)
        self.rec_thrs = self._thrs_host[1].to(dev, non_blocking=True)
        return self.rec_rank, self.rec_matched, self.rec_ignored, self.npig

    def add_batch(self, rows, counts, gt, gt_counts, box_map=None):
        """rows (B, K, 6) float32 and counts (B) int32 as ``engine.nms`` returns them (K <= max_det); gt (B, G, 7) float64
        [cls, x, y, w, h, area, iscrowd] and gt_counts (B) int32; ``box_map`` None: the boxes are final (mode 0), or (B, 4) float32
        [px, py, gx, gy] (mode 1, ``det_eval.letterbox_box_map``).  One launch pair, no host read."""
        self._buffers()
        rows, counts, gt, gt_counts, box_map = check_batch(rows, counts, gt, gt_counts, box_map, self.max_det, self.rec_score.device,
                                                           torch.float64, 7)
        B, K, G = int(rows.shape[0]), int(rows.shape[1]), int(gt.shape[1])
        self._cache = None
        L.check(L.load().cvx_coco_match(L.ptr(rows), L.ptr(counts), B, K, 0 if box_map is None else 1, L.ptr(box_map), int(self.truncate),
                                        int(self.quantize), L.ptr(gt) if G else None, L.ptr(gt_counts), G, self.num_classes,
                                        L.ptr(self.iou_thrs), L.ptr(self.rec_score), L.ptr(self.rec_class), L.ptr(self.rec_rank),
                                        L.ptr(self.rec_matched), L.ptr(self.rec_ignored), self.capacity, L.ptr(self.state), L.ptr(self.npig),
                                        L.stream_ptr(self.device)), "cvx_coco_match")

    def _reduce(self):
        """Order the records as COCOeval.accumulate does, run cvx_coco_accumulate and cvx_coco_summarize; everything stays on the device."""
        self._buffers()
        nc, dev = self.num_classes, self.device
        order, _, seg_off = record_order(self.rec_class, self.rec_score, nc)
        rank, matched, ignored = self.rec_rank[order].contiguous(), self.rec_matched[order].contiguous(), self.rec_ignored[order].contiguous()
        precision = torch.empty(10, 101, nc, 4, 3, dtype=torch.float64, device=dev)
        recall = torch.empty(10, nc, 4, 3, dtype=torch.float64, device=dev)
        stats = torch.empty(12, dtype=torch.float64, device=dev)
        lib, st = L.load(), L.stream_ptr(dev)
        L.check(lib.cvx_coco_accumulate(L.ptr(rank), L.ptr(matched), L.ptr(ignored), L.ptr(seg_off), L.ptr(self.npig), nc, L.ptr(self.rec_thrs),
                                        L.ptr(precision), L.ptr(recall), st), "cvx_coco_accumulate")
        L.check(lib.cvx_coco_summarize(L.ptr(precision), L.ptr(recall), nc, L.ptr(stats), st), "cvx_coco_summarize")
        return precision, recall, stats

    def results(self):
        """The single host read: ``stats`` (12, pycocotools' order), ``precision`` (10, 101, nc, 4, 3), ``recall`` (10, nc, 4, 3), ``npig``
        (nc, 4) and ``n_records``.  Raises ``CvxError`` if a batch overflowed (NMS count -1, no room left in ``capacity``), a class index was
        out of range or a score was unusable."""
        if self._cache is None:
            precision, recall, stats = self._reduce()
            nc = self.num_classes
            host = torch.cat((self.state.to(torch.float64), self.npig.reshape(-1).to(torch.float64), stats, recall.reshape(-1),
                              precision.reshape(-1))).cpu().numpy()                              # counters < 2^53: exact as doubles
            cursor = self._check_counters(host)
            o = 4
            npig = host[o:o + nc * 4].astype(np.int64).reshape(nc, 4)
            o += nc * 4
            st = host[o:o + 12].copy()
            o += 12
            rc = host[o:o + recall.numel()].reshape(tuple(recall.shape)).copy()
            o += recall.numel()
            self._cache = dict(stats=st, precision=host[o:].reshape(tuple(precision.shape)).copy(), recall=rc, npig=npig, n_records=cursor)
        return self._cache

    def records(self):
        """(score, class, rank, matched, ignored) numpy arrays in append order (image, row) -- for tests and debugging."""
        n = self.results()["n_records"]
        return tuple(t[:n].cpu().numpy() for t in (self.rec_score, self.rec_class, self.rec_rank, self.rec_matched, self.rec_ignored))

    def summary_text(self):
        """The twelve lines of COCOeval.summarize, newline-terminated"""
        return "".join(line + "\n" for line in summary_lines(self.results()["stats"]))


def evaluate_detector_coco(evaluator_rows, dataloader, num_classes, map_out_root, max_det, capacity=None):
    """The loop the four ``evaluate_on_coco`` methods share.  ``evaluator_rows(images, meta)`` -> (rows, counts, box_map or None) on the
    device; ``meta`` carries ``gt_coco`` (B, G, 7) float64 and ``gt_counts``.  Writes ``<map_out_root>/coco_results.txt``, prints its twelve
    lines and returns the ``results()`` dict."""
    ev = None
    for images, meta in dataloader:
        rows, counts, box_map = evaluator_rows(images, meta)
        if ev is None:
            if capacity is None:
                capacity = default_capacity(dataloader, rows.shape[0], max_det, "evaluate_on_coco")
            ev = CocoEvaluator(num_classes, max_det, capacity, rows.device)
        ev.add_batch(rows, counts, meta["gt_coco"], meta["gt_counts"], box_map)
    if ev is None:
        raise L.CvxError("evaluate_on_coco: the dataloader yielded no batch")
    res = ev.results()
    write_summary(ev, map_out_root)
    return res


def write_summary(ev, map_out_root):
    text = ev.summary_text()
    os.makedirs(map_out_root, exist_ok=True)
    with open(os.path.join(map_out_root, "coco_results.txt"), "w") as f:
        f.write(text)
    print(text, end="")
    return text


def check_coco_arguments(subset, dataloader):
    """What every ``evaluate_on_coco`` checks before it touches the model"""
    if subset != "val":
        raise ValueError(f"evaluate_on_coco evaluates subset 'val' only, got {subset}")
    if dataloader is None:
        raise L.CvxError("evaluate_on_coco reads no dataset from disk: pass dataloader= yielding (images, dict(image_hw, gt_coco, gt_counts)) "
                         "on the device over the COCO-val pictures in sorted-image-id order")
