"""Tracking evaluation on the device (csrc/track_eval.hip): ``TrackingEvaluator`` scores the track ids that
``track.Tracker`` hands out against ground-truth identities -- CLEAR-MOT (MOTA, MOTP, misses, false positives, identity switches,
fragmentations, mostly tracked / partly tracked / mostly lost) and the identity measures (IDF1, IDP, IDR).  The state of ``streams``
independent evaluations lives in device memory; ``add_frames`` is one ``cvx_mot_frames`` launch with no host read, ``get_results`` one
``cvx_mot_summary`` and the one host read.  The rules are in include/cvx_engine.h and restated in numpy in
tests/track_eval_restatement.py.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

from . import _lib as L

FRAME_CAP, MAX_GT_IDS, MAX_TRACK_IDS = 1024, 1024, 4096      # CVX_MOT_FRAME_CAP, CVX_MOT_MAX_GT_IDS, CVX_MOT_MAX_TRACK_IDS
HEADER_WORDS, TABLE_WORDS = 16, 24                           # CVX_MOT_HEADER_WORDS, CVX_MOT_TABLE_WORDS
# the columns of cvx_mot_summary's table
TABLE = ("frames", "objects", "hypotheses", "matches", "misses", "false_positives", "switches", "fragmentations", "cost", "mostly_tracked",
         "partially_tracked", "mostly_lost", "idtp", "flag_nan", "flag_dup_row", "flag_dup_gt", "flag_identity", "flag_track", "flag_frame",
         "flag_excess", "identities", "tracks", "reserved0", "reserved1")
assert len(TABLE) == TABLE_WORDS
SCORES = ("mota", "motp", "idf1", "idp", "idr")


class MotParams(C.Structure):
    """struct cvx_mot_params"""
    _fields_ = [("iou", C.c_float), ("class_agnostic", C.c_int32), ("max_gt_ids", C.c_int32), ("max_track_ids", C.c_int32), ("reserved", C.c_int32 * 2)]


def state_bytes(max_gt_ids: int, max_track_ids: int) -> int:
    """one stream's state block: the header, five int32 per identity, the c matrix; rounded up to 8 bytes"""
    return (8 * HEADER_WORDS + 20 * max_gt_ids + 4 * max_gt_ids * max_track_ids + 7) & ~7


def _ratio(a: int, b: int) -> float:
    return float(a) / float(b) if b else float("nan")


def results_of(row) -> dict:
    """The scores of one row of the table, in double from the integer sums; a score without a denominator is NaN."""
    r = {name: int(v) for name, v in zip(TABLE, row)}
    obj, hyp, tp = r["objects"], r["hypotheses"], r["idtp"]
    return {"mota": 1.0 - _ratio(r["misses"] + r["false_positives"] + r["switches"], obj), "motp": 1.0 - _ratio(r["cost"], 65536 * r["matches"]),
            "idf1": _ratio(2 * tp, obj + hyp), "idp": _ratio(tp, hyp), "idr": _ratio(tp, obj),
            "num_frames": r["frames"], "num_objects": obj, "num_hypotheses": hyp, "num_matches": r["matches"], "num_misses": r["misses"],
            "num_false_positives": r["false_positives"], "num_switches": r["switches"], "num_fragmentations": r["fragmentations"],
            "mostly_tracked": r["mostly_tracked"], "partially_tracked": r["partially_tracked"], "mostly_lost": r["mostly_lost"],
            "idtp": tp, "idfp": hyp - tp, "idfn": obj - tp}


def flags_of(row) -> dict:
    return {name[5:]: int(v) for name, v in zip(TABLE, row) if name.startswith("flag_")}


def format_report(results: dict) -> str:
    """``get_results()`` as text: one line per stream and one for all of them"""
    ints = [k for k in results["overall"] if k not in SCORES]
    lines = ["# tracking evaluation: CLEAR-MOT (Bernardin & Stiefelhagen 2008) and the identity measures (Ristani et al. 2016)",
             "# motp is the mean IoU of the matches; a score without a denominator is nan",
             " ".join(["stream"] + list(SCORES) + ints)]
    for name, r in [(str(k), r) for k, r in enumerate(results["streams"])] + [("overall", results["overall"])]:
        lines.append(" ".join([name] + [f"{r[k]:.6f}" for k in SCORES] + [str(r[k]) for k in ints]))
    return "\n".join(lines) + "\n"


class TrackingEvaluator:
    """``streams`` independent tracking evaluations on ``device``; stream means what it means for ``track.Tracker``.  ``iou``: the gate of a
    pair; ``max_gt_ids`` (<= 1024) and ``max_track_ids`` (<= 4096) bound the identities and the track ids, and size the state."""

    def __init__(self, device, streams: int = 1, iou: float = 0.5, class_agnostic: bool = False, max_gt_ids: int = MAX_GT_IDS,
                 max_track_ids: int = MAX_TRACK_IDS):
        if int(streams) != streams or not 1 <= int(streams) <= 65535:
            raise ValueError("TrackingEvaluator: streams is an integer in [1, 65535]")
        if not 0.0 <= float(iou) <= 1.0:
            raise ValueError(f"TrackingEvaluator: iou = {iou} lies outside [0, 1]")
        if int(max_gt_ids) != max_gt_ids or not 1 <= int(max_gt_ids) <= MAX_GT_IDS:
            raise ValueError(f"TrackingEvaluator: max_gt_ids is an integer in [1, {MAX_GT_IDS}]")
        if int(max_track_ids) != max_track_ids or not 1 <= int(max_track_ids) <= MAX_TRACK_IDS:
            raise ValueError(f"TrackingEvaluator: max_track_ids is an integer in [1, {MAX_TRACK_IDS}]")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.CvxError(f"TrackingEvaluator runs on an MI355X only (device {self.device}): there is no CPU path")
        self.streams, self.iou, self.class_agnostic = int(streams), float(iou), bool(class_agnostic)
        self.max_gt_ids, self.max_track_ids = int(max_gt_ids), int(max_track_ids)
        self._c_params = MotParams(self.iou, int(self.class_agnostic), self.max_gt_ids, self.max_track_ids)
        lib = L.load()
        self.stream_bytes = state_bytes(self.max_gt_ids, self.max_track_ids)
        need = int(lib.cvx_mot_state_bytes(self.streams, self.max_gt_ids, self.max_track_ids))
        if need != self.streams * self.stream_bytes:
            raise L.CvxError(f"cvx_mot_state_bytes = {need}: the library's state layout is not this binding's")
        self.state = torch.zeros(need, dtype=torch.uint8, device=self.device)
        self.workspace = torch.empty(int(lib.cvx_mot_workspace_bytes(self.streams)), dtype=torch.uint8, device=self.device)
        self.table = torch.zeros(self.streams + 1, TABLE_WORDS, dtype=torch.int64, device=self.device)
        self._results = None

    def add_frames(self, rows: torch.Tensor, counts: torch.Tensor, ids: torch.Tensor, gt: torch.Tensor, gt_counts: torch.Tensor,
                   frame_stream: Optional[torch.Tensor] = None) -> None:
        """``cvx_mot_frames``: rows (B, K, 6) fp32, counts (B) int32 and ids (B, K) int32 as ``predict_batch(..., tracker=)`` leaves them, the
        frames in time order; gt (B, G <= 1024, 6) fp32 ``[x1, y1, x2, y2, cls, identity]`` and gt_counts (B) int32; ``frame_stream`` (B)
        int32 names each frame's stream (None: all stream 0).  Everything on the device.  No host read."""
        if not (torch.is_tensor(rows) and rows.is_cuda):
            raise L.CvxError("TrackingEvaluator.add_frames runs on an MI355X only: there is no CPU path")
        if rows.dim() != 3 or rows.shape[2] != 6 or rows.dtype != torch.float32 or rows.shape[0] <= 0 or rows.shape[1] <= 0 or rows.device != self.device:
            raise ValueError(f"rows: (B, K, 6) float32 on {self.device}, got {tuple(rows.shape)} {rows.dtype} on {rows.device}")
        B, K = int(rows.shape[0]), int(rows.shape[1])
        if not torch.is_tensor(ids) or ids.dtype != torch.int32 or tuple(ids.shape) != (B, K) or ids.device != rows.device:
            raise ValueError("ids: (B, K) int32 on the rows' device")
        if (not torch.is_tensor(gt) or gt.dim() != 3 or gt.shape[0] != B or gt.shape[2] != 6 or gt.dtype != torch.float32 or gt.device != rows.device
                or not 1 <= gt.shape[1] <= FRAME_CAP):
            raise ValueError(f"gt: (B, G <= {FRAME_CAP}, 6) float32 on the rows' device")
        for name, t in (("counts", counts), ("gt_counts", gt_counts)) + ((("frame_stream", frame_stream),) if frame_stream is not None else ()):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.numel() != B or t.device != rows.device:
                raise ValueError(f"{name}: (B) int32 on the rows' device")
        rows, counts, ids, gt, gt_counts = rows.contiguous(), counts.contiguous(), ids.contiguous(), gt.contiguous(), gt_counts.contiguous()
        frame_stream = None if frame_stream is None else frame_stream.contiguous()
        self._results = None
        with torch.cuda.device(self.device):
            L.check(L.load().cvx_mot_frames(L.ptr(rows), L.ptr(counts), L.ptr(ids), B, K, L.ptr(gt), L.ptr(gt_counts), int(gt.shape[1]),
                                            L.ptr(frame_stream), self.streams, C.byref(self._c_params), L.ptr(self.state), L.ptr(self.workspace),
                                            self.workspace.numel(), L.stream_ptr(self.device)), "cvx_mot_frames")

    def reset(self, stream: Optional[int] = None) -> None:
        """Forgets one stream, or all: a memset."""
        self._results = None
        if stream is None:
            self.state.zero_()
            return
        if not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream {stream} outside [0, {self.streams})")
        n = self.stream_bytes
        self.state[int(stream) * n:(int(stream) + 1) * n].zero_()

    def summary_table(self) -> np.ndarray:
        """``cvx_mot_summary`` and ONE host read: the table (streams + 1, 24) int64, its last row the sum over the streams"""
        with torch.cuda.device(self.device):
            L.check(L.load().cvx_mot_summary(L.ptr(self.state), self.streams, self.max_gt_ids, self.max_track_ids, L.ptr(self.table),
                                             L.stream_ptr(self.device)), "cvx_mot_summary")
        return self.table.cpu().numpy()

    def get_results(self) -> dict:
        """ONE host read.  ``{"streams": [dict per stream], "overall": dict}`` with ``mota``, ``motp`` (the mean IoU of the matches), ``idf1``,
        ``idp``, ``idr``, ``num_frames``, ``num_objects``, ``num_hypotheses``, ``num_matches``, ``num_misses``, ``num_false_positives``,
        ``num_switches``, ``num_fragmentations``, ``mostly_tracked``, ``partially_tracked``, ``mostly_lost``, ``idtp``, ``idfp``, ``idfn``.
        Raises ``CvxError`` when anything was skipped: a NaN box, a repeated id or identity in a frame, an id or identity out of range, a bad
        count or stream, more than 1024 hypotheses in a frame."""
        table = self.summary_table()
        flags = flags_of(table[-1])
        if any(flags.values()):
            raise L.CvxError(f"TrackingEvaluator: inputs were skipped, nothing is truncated silently: {flags}")
        self._results = {"streams": [results_of(r) for r in table[:-1]], "overall": results_of(table[-1])}
        return self._results

    def write_report(self, path) -> str:
        """``get_results()`` (the last one, if no frame came since) as text to ``path``; returns the path"""
        res = self._results if self._results is not None else self.get_results()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(format_report(res))
        return str(path)

    def state_block(self, stream: int = 0) -> np.ndarray:
        """ONE host read: the raw state block of ``stream`` (uint8), laid out as include/cvx_engine.h says"""
        if not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream {stream} outside [0, {self.streams})")
        n = self.stream_bytes
        return self.state[int(stream) * n:(int(stream) + 1) * n].cpu().numpy()
