"""What the detection metrics share on the host (``det_eval.py``, ``coco_eval.py``, ``det_diag.py``; it imports none of them): the size
limits of csrc/det_common.h, the argument checks of a batch, the default capacity, the order in which the per-class kernels read the
records, and the base of the two evaluators that append records -- their constructor checks, lazy allocation, ``reset`` and the counter
check."""
import torch

from . import _lib as L

MAX_ROWS, MAX_GT = 16384, 1024


def check_batch(rows, counts, gt, gt_counts, box_map, max_det, device, gt_dtype=torch.int32, gt_width=6):
    """The argument checks of every ``add_batch``; the ground truth is (B, G, 6) int32 (VOC) or (B, G, 7) float64 (COCO).  Returns the
    five arguments contiguous."""
    if rows.dim() != 3 or rows.shape[2] != 6 or rows.dtype != torch.float32 or not (0 < int(rows.shape[1]) <= max_det):
        raise ValueError(f"rows: (B, K <= {max_det}, 6) float32, got {tuple(rows.shape)} {rows.dtype}")
    B = int(rows.shape[0])
    G = int(gt.shape[1]) if gt.dim() == 3 else -1
    if G < 0 or gt.shape[0] != B or (G and gt.shape[2] != gt_width) or gt.dtype != gt_dtype or G > MAX_GT:
        raise ValueError(f"gt: (B, G <= {MAX_GT}, {gt_width}) {str(gt_dtype).replace('torch.', '')}, got {tuple(gt.shape)} {gt.dtype}")
    if counts.dtype != torch.int32 or gt_counts.dtype != torch.int32 or counts.numel() != B or gt_counts.numel() != B:
        raise ValueError("counts and gt_counts: (B) int32")
    if box_map is not None and (box_map.dtype != torch.float32 or tuple(box_map.shape) != (B, 4)):
        raise ValueError("box_map: (B, 4) float32 [px, py, gx, gy]")
    for t in (rows, counts, gt, gt_counts, box_map):
        if t is not None and t.device != device:
            raise ValueError("add_batch: every tensor lives on the evaluator's device")
    return rows.contiguous(), counts.contiguous(), gt.contiguous(), gt_counts.contiguous(), None if box_map is None else box_map.contiguous()


def default_capacity(dataloader, batch, max_det, who):
    """batches x batch size x min(max_det, 1024) records"""
    if not hasattr(dataloader, "__len__"):
        raise L.CvxError(f"{who}: a dataloader without len() needs capacity= (the records of the whole evaluation)")
    return len(dataloader) * int(batch) * min(int(max_det), 1024)


def record_order(rec_class, rec_score, num_classes):
    """The order of get_map and of COCOeval.accumulate: class ascending, score descending, equal scores in append order (image, row).
    One stable sort of an int64 key -- the class in the high bits, the inverted score bits below -- so unwritten slots
    (class == num_classes) sort behind every class.  Returns ``order``, the sorted class column and ``seg_off`` (nc + 1), the first
    record of each class."""
    key = (rec_class.to(torch.int64) << 32) | (0xFFFFFFFF - rec_score.view(torch.int32).to(torch.int64))
    key, order = torch.sort(key, stable=True)
    cls = (key >> 32).contiguous()
    seg_off = torch.searchsorted(cls, torch.arange(num_classes + 1, dtype=torch.int64, device=cls.device)).contiguous()
    return order, cls, seg_off


class RecordEvaluator:
    """Base of ``DetectionEvaluator`` and ``CocoEvaluator``: ``rec_score`` / ``rec_class`` and the four counters of ``state`` (cursor,
    overflow, low score, bad class).  A subclass names its entries (``_ENTRIES``: the match entry first), allocates its further record
    columns and counters in ``_columns`` (returning them: ``reset`` zeroes them) and words ``_low_score_message``."""
    _ENTRIES = ()

    def __init__(self, num_classes, max_det, capacity, device):
        if not (0 < int(max_det) <= MAX_ROWS):
            raise ValueError(f"max_det {max_det}: {self._ENTRIES[0]} holds 1 .. {MAX_ROWS} rows per image")
        if int(num_classes) <= 0 or int(capacity) <= 0:
            raise ValueError("num_classes and capacity are positive")
        self.num_classes, self.max_det, self.capacity = int(num_classes), int(max_det), int(capacity)
        self.device = torch.device(device)
        self._alloc = False
        self._cache = None

    def _buffers(self):
        if self.device.type != "cuda":
            raise L.CvxError(f"{type(self).__name__} runs on an MI355X only ({' / '.join(self._ENTRIES)}): there is no CPU path")
        if not self._alloc:
            self.rec_score = torch.zeros(self.capacity, dtype=torch.float32, device=self.device)
            self.rec_class = torch.empty(self.capacity, dtype=torch.int32, device=self.device)
            self.state = torch.zeros(4, dtype=torch.int64, device=self.device)
            self._zeroed = (self.rec_score, self.state) + tuple(self._columns())
            self._alloc = True
            self.reset()

    def reset(self):
        self._cache = None
        if self._alloc:
            self.rec_class.fill_(self.num_classes)       # unwritten slots sort behind every class
            for t in self._zeroed:
                t.zero_()

    def _check_counters(self, host):
        """host[:4]: ``state`` as the single host read brought it.  Raises what ``results()`` raises; returns the cursor."""
        cursor, overflow, low, bad = (int(v) for v in host[:4])
        name = type(self).__name__
        if overflow:
            raise L.CvxError(f"{name}: {overflow} image(s) dropped: an NMS count of -1 (more candidates than cvx_nms sorts), a "
                             f"count past its block, or more than capacity={self.capacity} records")
        if bad:
            raise L.CvxError(f"{name}: {bad} class indices outside [0, {self.num_classes})")
        if low:
            raise L.CvxError(f"{name}: {low} " + self._low_score_message)
        return cursor
