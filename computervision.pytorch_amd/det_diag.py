"""Diagnostics of a detector beside its VOC mAP, accumulated on the device: the confusion matrix at one (confidence, IoU) pair, precision /
recall / F1 against the confidence threshold with the threshold that maximises the smoothed mean F1, and the log-average miss rate of the
reference's ``get_map`` (``log_average_miss_rate``, core/metrics/mAP.py:34-70, called at :634-636).

``DetectionDiagnostics.add_batch`` is one ``cvx_det_confusion`` launch per batch (csrc/det_diag.hip) on the rows ``DetectionEvaluator``
takes; ``results(evaluator)`` runs ``cvx_det_conf_curves`` once on the records the evaluator's ``cvx_det_ap`` left on the device and makes
one host read beside the evaluator's.  The matching rule of the matrix is Ultralytics' ``ConfusionMatrix.process_batch`` with the ties
decided -- the project's own rule, written out in tests/det_diag_restatement.py and in include/cvx_engine.h.  The curves are step
functions: at ``conf_grid[k]`` they hold the exact precision / recall / F1 a user gets with ``conf_threshold = conf_grid[k]`` (not
Ultralytics' linear interpolation).

Not built: the COCO path, TIDE-style error types, matrices at several thresholds in one pass, plots.
"""
import math
import os

import numpy as np
import torch

from . import _lib as L
from .det_records import MAX_ROWS, check_batch

MAX_POINTS, MAX_WINDOW = 4096, 65535
REF_POINTS = np.logspace(-2.0, 0.0, num=9)       # the reference's nine FPPI points, computed by numpy: no pow on the device


class DetDiagnostics:
    """The spec: ``conf`` and ``iou`` of the confusion matrix (a pair matches when its overlap is strictly above ``iou``), the number of
    grid ``points`` of the confidence curves over [0, 1] and the odd ``smooth_window`` of the moving average the best threshold is read
    from."""

    def __init__(self, conf=0.25, iou=0.45, points=1001, smooth_window=101):
        if isinstance(conf, bool) or isinstance(iou, bool) or not isinstance(conf, (int, float)) or not isinstance(iou, (int, float)):
            raise ValueError("conf and iou are numbers")
        if not (0.0 <= float(conf) <= 1.0):
            raise ValueError(f"conf {conf}: a confidence in [0, 1]")
        if not (0.0 <= float(iou) < 1.0):
            raise ValueError(f"iou {iou}: an overlap threshold in [0, 1)")
        if isinstance(points, bool) or not isinstance(points, int) or not (2 <= points <= MAX_POINTS):
            raise ValueError(f"points {points}: an integer in 2 .. {MAX_POINTS}")
        if isinstance(smooth_window, bool) or not isinstance(smooth_window, int) or not (1 <= smooth_window <= MAX_WINDOW) or smooth_window % 2 == 0:
            raise ValueError(f"smooth_window {smooth_window}: an odd integer in 1 .. {MAX_WINDOW}")
        self.conf, self.iou, self.points, self.smooth_window = float(conf), float(iou), points, smooth_window

    def __repr__(self):
        return f"DetDiagnostics(conf={self.conf}, iou={self.iou}, points={self.points}, smooth_window={self.smooth_window})"


def curve_words(num_classes, points):
    """8-byte words of ``cvx_det_conf_curves``' output: precision, recall, f1 (nc, P) each, mean f1 and its smoothing (P) each, the miss
    rates (nc, 9), the best indices (nc + 1)"""
    return 3 * num_classes * points + 2 * points + 10 * num_classes + 1


def conf_curves(records, gt_per_class, images_per_class, num_classes, quantize, points, window):
    """One ``cvx_det_conf_curves`` call: ``records`` the dictionary of ``DetectionEvaluator.device_records()`` (``score`` float32,
    ``prec`` / ``rec`` float64, ``flag`` int32, ``seg_off`` int64 (nc + 1)), ``gt_per_class`` and ``images_per_class`` (nc) int64, all on
    one device.  Returns the output buffer as int64 words on the device; ``unpack_curves`` splits it on the host.  No host read."""
    dev = records["score"].device
    if dev.type != "cuda":
        raise L.CvxError("conf_curves runs on an MI355X only (cvx_det_conf_curves): there is no CPU path")
    nc = int(num_classes)
    want = (("score", torch.float32), ("prec", torch.float64), ("rec", torch.float64), ("flag", torch.int32), ("seg_off", torch.int64))
    for name, dtype in want:
        t = records[name]
        if t.dtype != dtype or t.device != dev or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"records[{name!r}]: a contiguous 1-d {dtype} tensor on {dev}")
    n = int(records["score"].numel())
    if records["seg_off"].numel() != nc + 1 or any(int(records[k].numel()) != n for k in ("prec", "rec", "flag")):
        raise ValueError("records: seg_off holds nc + 1 offsets; score, prec, rec and flag one entry per record")
    for t in (gt_per_class, images_per_class):
        if t.dtype != torch.int64 or t.numel() != nc or t.device != dev or not t.is_contiguous():
            raise ValueError("gt_per_class and images_per_class: (nc) int64 on the records' device")
    spec = DetDiagnostics(points=points, smooth_window=window)
    words = curve_words(nc, spec.points)
    out = torch.zeros(words, dtype=torch.float64, device=dev)
    ref = torch.from_numpy(REF_POINTS).to(dev)
    L.check(L.load().cvx_det_conf_curves(L.ptr(records["score"]), L.ptr(records["prec"]), L.ptr(records["rec"]), L.ptr(records["flag"]),
                                         L.ptr(records["seg_off"]), L.ptr(gt_per_class), L.ptr(images_per_class), nc, int(bool(quantize)),
                                         spec.points, spec.smooth_window, L.ptr(ref), L.ptr(out), words, L.stream_ptr(dev)), "cvx_det_conf_curves")
    return out.view(torch.int64)


def unpack_curves(words, num_classes, points):
    """the host copy of ``conf_curves``' words (numpy int64) -> precision, recall, f1 (nc, P), mean_f1, mean_f1_smooth (P), mr9 (nc, 9)
    float64 and best_index_per_class (nc), best_index"""
    nc, P = int(num_classes), int(points)
    words = np.ascontiguousarray(words, dtype=np.int64)
    assert words.size == curve_words(nc, P)
    f = words.view(np.float64)
    plane = nc * P
    best = words[3 * plane + 2 * P + 9 * nc:]
    return dict(precision=f[:plane].reshape(nc, P).copy(), recall=f[plane:2 * plane].reshape(nc, P).copy(),
                f1=f[2 * plane:3 * plane].reshape(nc, P).copy(), mean_f1=f[3 * plane:3 * plane + P].copy(),
                mean_f1_smooth=f[3 * plane + P:3 * plane + 2 * P].copy(), mr9=f[3 * plane + 2 * P:3 * plane + 2 * P + 9 * nc].reshape(nc, 9).copy(),
                best_index_per_class=best[:nc].copy(), best_index=int(best[nc]))


def lamr_from_mr9(mr9, n_records, images_per_class):
    """The end of ``log_average_miss_rate`` on the host: exp(mean(log(max(1e-10, .)))) of a class's nine miss rates; 0 for a class without
    a record, as the reference returns; nan for a class no image holds (the reference never reaches it)."""
    out = np.full(len(mr9), np.nan)
    for c in range(len(mr9)):
        if images_per_class[c] > 0:
            out[c] = math.exp(np.mean(np.log(np.maximum(1e-10, mr9[c])))) if n_records[c] > 0 else 0.0
    return out


def _mean_of(values, keep):
    return float(np.mean(values[keep])) if keep.any() else 0.0


class DetectionDiagnostics:
    """The accumulator: ``max_det`` the most rows per image a batch may carry.  ``quantize_scores`` as ``DetectionEvaluator``'s."""

    def __init__(self, num_classes, max_det, device, spec=None, quantize_scores=True):
        if not (0 < int(max_det) <= MAX_ROWS):
            raise ValueError(f"max_det {max_det}: cvx_det_confusion holds 1 .. {MAX_ROWS} rows per image")
        if int(num_classes) <= 0:
            raise ValueError("num_classes is positive")
        spec = DetDiagnostics() if spec is None else spec
        if not isinstance(spec, DetDiagnostics):
            raise ValueError(f"spec: a DetDiagnostics, got {type(spec).__name__}")
        self.num_classes, self.max_det, self.spec, self.quantize = int(num_classes), int(max_det), spec, bool(quantize_scores)
        self.device = torch.device(device)
        self._alloc = False
        self._cache = None

    def _buffers(self):
        if self.device.type != "cuda":
            raise L.CvxError("DetectionDiagnostics runs on an MI355X only (cvx_det_confusion / cvx_det_conf_curves): there is no CPU path")
        if not self._alloc:
            nc = self.num_classes
            # one block: [state (4), images_per_class (nc), confusion ((nc + 1)^2)] -- one fill to reset, one copy to read
            self._block = torch.zeros(4 + nc + (nc + 1) * (nc + 1), dtype=torch.int64, device=self.device)
            self.state, self.images_per_class, self.matrix = self._block[:4], self._block[4:4 + nc], self._block[4 + nc:].view(nc + 1, nc + 1)
            self._alloc = True

    def reset(self):
        self._cache = None
        if self._alloc:
            self._block.zero_()

    def add_batch(self, rows, counts, gt, gt_counts, box_map=None):
        """The arguments of ``DetectionEvaluator.add_batch``, with its checks.  One launch, no host read."""
        self._buffers()
        rows, counts, gt, gt_counts, box_map = check_batch(rows, counts, gt, gt_counts, box_map, self.max_det, self._block.device)
        B, K, G = int(rows.shape[0]), int(rows.shape[1]), int(gt.shape[1])
        self._cache = None
        L.check(L.load().cvx_det_confusion(L.ptr(rows), L.ptr(counts), B, K, 0 if box_map is None else 1, L.ptr(box_map), L.ptr(gt) if G else None,
                                           L.ptr(gt_counts), G, self.num_classes, self.spec.conf, self.spec.iou, int(self.quantize),
                                           L.ptr(self.matrix), L.ptr(self.images_per_class), L.ptr(self.state), L.stream_ptr(self.device)),
                "cvx_det_confusion")

    def _split(self, host):
        nc = self.num_classes
        seen, skipped, bad = (int(v) for v in host[:3])
        if skipped:
            raise L.CvxError(f"DetectionDiagnostics: {skipped} image(s) skipped: an NMS count of -1 (more candidates than cvx_nms sorts) or a "
                             "count past its block")
        if bad:
            raise L.CvxError(f"DetectionDiagnostics: {bad} class indices outside [0, {nc})")
        return seen, host[4:4 + nc].copy(), host[4 + nc:4 + nc + (nc + 1) * (nc + 1)].reshape(nc + 1, nc + 1).copy()

    def confusion(self):
        """The matrix alone, (nc + 1, nc + 1) int64 [predicted, true] with background last (one host read).  Raises as ``results``."""
        self._buffers()
        return self._split(self._block.cpu().numpy())[2]

    def results(self, evaluator):
        """``evaluator``: the ``DetectionEvaluator`` that was fed the same batches.  Raises ``CvxError`` on skipped images or class indices
        out of range.  One host read beside the evaluator's."""
        if self._cache is not None and self._cache[0] is evaluator:       # add_batch and reset drop it
            return self._cache[1]
        self._buffers()
        nc, spec = self.num_classes, self.spec
        if evaluator.num_classes != nc or evaluator.quantize != self.quantize:
            raise ValueError("results: the evaluator has this accumulator's num_classes and quantize_scores")
        ev = evaluator.results()
        records = evaluator.device_records()
        words = conf_curves(records, evaluator.gt_per_class, self.images_per_class, nc, self.quantize, spec.points, spec.smooth_window)
        host = torch.cat((self._block, words)).cpu().numpy()
        n_block = self._block.numel()
        _, images, matrix = self._split(host[:n_block])
        res = unpack_curves(host[n_block:], nc, spec.points)
        grid = np.arange(spec.points).astype(np.float64) / float(spec.points - 1)
        k = res["best_index"]
        with_gt = np.asarray(ev["n_gt"]) > 0
        lamr = lamr_from_mr9(res["mr9"], ev["n_det"], images)
        res.update(confusion=matrix, images_per_class=images, conf=spec.conf, iou=spec.iou, conf_grid=grid, best_conf=float(grid[k]),
                   best_conf_per_class=grid[res["best_index_per_class"]], precision_at_best=res["precision"][:, k].copy(),
                   recall_at_best=res["recall"][:, k].copy(), f1_at_best=res["f1"][:, k].copy(), lamr=lamr, n_gt=np.asarray(ev["n_gt"]).copy())
        res.update(mean_precision_at_best=_mean_of(res["precision_at_best"], with_gt), mean_recall_at_best=_mean_of(res["recall_at_best"], with_gt),
                   mean_f1_at_best=_mean_of(res["f1_at_best"], with_gt), mean_lamr=_mean_of(lamr, with_gt & ~np.isnan(lamr)))
        self._cache = (evaluator, res)
        return res

    def write_report(self, directory, class_names, evaluator=None):
        """``confusion_matrix.csv``, ``confidence_curves.csv`` and ``diagnostics.txt`` into ``directory``, from ``results(evaluator)`` or,
        without an evaluator, from the last ``results`` call; returns the three paths"""
        if evaluator is None and self._cache is None:
            raise L.CvxError("write_report: call results(evaluator) first, or pass evaluator=")
        res = self._cache[1] if evaluator is None else self.results(evaluator)
        os.makedirs(directory, exist_ok=True)
        paths = []
        for name, text in (("confusion_matrix.csv", format_confusion_csv(res["confusion"], class_names)),
                           ("confidence_curves.csv", format_curves_csv(res, class_names)),
                           ("diagnostics.txt", format_diagnostics(res, class_names))):
            paths.append(os.path.join(directory, name))
            with open(paths[-1], "w") as f:
                f.write(text)
        return paths


def _csv_name(name):
    return '"' + name.replace('"', '""') + '"' if any(ch in name for ch in ',"\n') else name


def format_confusion_csv(confusion, class_names):
    """header ``pred\\true``, the names, ``background``; then one line per predicted class and the background line (missed ground truths)"""
    nc = confusion.shape[0] - 1
    assert len(class_names) >= nc
    names = [_csv_name(class_names[c]) for c in range(nc)] + ["background"]
    out = [",".join(["pred\\true"] + names) + "\n"]
    for p in range(nc + 1):
        out.append(",".join([names[p]] + [str(int(v)) for v in confusion[p]]) + "\n")
    return "".join(out)


def format_curves_csv(res, class_names):
    """``conf, mean_f1, mean_f1_smooth``, then ``<name>_p, <name>_r, <name>_f1`` per class; one line per grid point, every number as
    ``repr`` writes a Python float (round trip)"""
    nc = res["f1"].shape[0]
    assert len(class_names) >= nc
    head = ["conf", "mean_f1", "mean_f1_smooth"]
    for c in range(nc):
        head += [_csv_name(class_names[c] + "_" + k) for k in ("p", "r", "f1")]
    out = [",".join(head) + "\n"]
    for k in range(len(res["conf_grid"])):
        line = [res["conf_grid"][k], res["mean_f1"][k], res["mean_f1_smooth"][k]]
        for c in range(nc):
            line += [res["precision"][c, k], res["recall"][c, k], res["f1"][c, k]]
        out.append(",".join(repr(float(v)) for v in line) + "\n")
    return "".join(out)


def format_diagnostics(res, class_names):
    """The recommended threshold; per class with a ground truth (in name order) its own best threshold, P / R / F1 at the recommended one,
    LAMR and images; the ten largest off-diagonal cells of the matrix (largest first, then predicted, then true index)."""
    nc = res["f1"].shape[0]
    assert len(class_names) >= nc
    names = list(class_names[:nc]) + ["background"]
    out = ["# detector diagnostics\n",
           "recommended conf_threshold = {0:.4f} (first maximum of the mean F1 over {1} classes, smoothed; mean F1 {2:.4f}, smoothed {3:.4f})\n".format(
               res["best_conf"], int((res["n_gt"] > 0).sum()), res["mean_f1"][res["best_index"]], res["mean_f1_smooth"][res["best_index"]]),
           "at it: mean precision {0:.4f}, mean recall {1:.4f}, mean F1 {2:.4f}; mean LAMR {3:.4f}\n".format(
               res["mean_precision_at_best"], res["mean_recall_at_best"], res["mean_f1_at_best"], res["mean_lamr"]),
           "\n# per class: own best conf | precision recall F1 at the recommended conf | LAMR | images\n"]
    for c in sorted(range(nc), key=lambda c: class_names[c]):
        if res["n_gt"][c] <= 0:
            continue
        out.append("{0}: {1:.4f} | {2:.4f} {3:.4f} {4:.4f} | {5:.4f} | {6}\n".format(
            class_names[c], res["best_conf_per_class"][c], res["precision_at_best"][c], res["recall_at_best"][c], res["f1_at_best"][c],
            res["lamr"][c], int(res["images_per_class"][c])))
    out.append("\n# confusion matrix at conf {0:.4f}, IoU {1:.2f}: largest off-diagonal cells (predicted -> true: count)\n".format(res["conf"], res["iou"]))
    m = res["confusion"]
    cells = [(-int(m[p, t]), p, t) for p in range(nc + 1) for t in range(nc + 1) if p != t and m[p, t] > 0]
    for neg, p, t in sorted(cells)[:10]:
        out.append("{0} -> {1}: {2}\n".format(names[p], names[t], -neg))
    return "".join(out)
