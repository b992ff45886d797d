"""Multi-object tracking on the device video path (csrc/track.hip): ``Tracker`` owns the state of ``streams``
independent trackers in device memory and gives every detection row of a batch of frames a track id in one ``cvx_track_update`` launch,
with no host read.  A ByteTrack-style tracker -- two association stages by score, constant-velocity prediction with an alpha-beta update,
greedy IoU association; the rules are in include/cvx_engine.h and restated in numpy in tests/track_restatement.py.  ``TrackModel`` swaps in
a Kalman motion model and a minimum-cost association, each optional (section 7ad, tests/track_model_restatement.py).  There is no CPU path."""
from __future__ import annotations

import ctypes as C
import numbers
from typing import Optional

import numpy as np
import torch

from . import _lib as L

TRACK_CAP = 1024                    # tracks per stream (CVX_TRACK_CAP)
# struct cvx_track_stream, include/cvx_engine.h: all zero is "no tracks, frame 0, next id 0"
STREAM_DTYPE = np.dtype([("frame", "<i4"), ("next_id", "<i4"), ("n_tracks", "<i4"), ("reserved", "<i4"), ("id", "<i4", (TRACK_CAP,)),
                         ("hits", "<i4", (TRACK_CAP,)), ("miss", "<i4", (TRACK_CAP,)), ("cls", "<f4", (TRACK_CAP,)), ("p", "<f4", (TRACK_CAP, 4)),
                         ("v", "<f4", (TRACK_CAP, 4))])
assert STREAM_DTYPE.itemsize == 16 + 48 * TRACK_CAP
EXT_BYTES = 16 * TRACK_CAP          # per stream: float cov[CVX_TRACK_CAP][4], (Pxx, Pxv, Pvv, reserved) of the track in the same slot
MOTIONS = {"alpha_beta": 0, "kalman": 1}     # CVX_TRACK_MOTION_*
ASSIGNS = {"greedy": 0, "optimal": 1}        # CVX_TRACK_ASSIGN_*
OPTIMAL_MAX_DET = 4096                       # CVX_TRACK_OPTIMAL_MAX_DET
DEFAULTS = dict(high=0.5, new_score=0.6, iou_high=0.2, iou_low=0.5, alpha=0.75, beta=0.25, min_hits=3, max_age=30, class_agnostic=False)


class TrackParams(C.Structure):
    """struct cvx_track_params"""
    _fields_ = [("high", C.c_float), ("new_score", C.c_float), ("iou_high", C.c_float), ("iou_low", C.c_float), ("alpha", C.c_float),
                ("beta", C.c_float), ("min_hits", C.c_int32), ("max_age", C.c_int32), ("class_agnostic", C.c_int32), ("reserved", C.c_int32)]


class TrackModelStruct(C.Structure):
    """struct cvx_track_model"""
    _fields_ = [("motion", C.c_int32), ("assign", C.c_int32), ("q_pos", C.c_float), ("q_vel", C.c_float), ("r_pos", C.c_float),
                ("init_pos", C.c_float), ("init_vel", C.c_float), ("min_scale", C.c_float)]


class TrackModel:
    """The motion model and the association of a ``Tracker``.  ``motion``: ``"alpha_beta"`` (fixed gains ``alpha``,
    ``beta``) or ``"kalman"``: a constant-velocity Kalman filter per corner coordinate whose gains follow from a covariance that grows
    while a track is lost; ``alpha`` and ``beta`` are then ignored.  Its noise is ByteTrack's, relative to the box height (``min_scale``
    pixels at the least): ``q_pos`` and ``q_vel`` per frame (std_weight_position, std_weight_velocity), ``r_pos`` of a detection, and a
    new track starts at ``init_pos * r_pos`` and ``init_vel * q_vel``.  ``assign``: ``"greedy"`` by descending IoU, or ``"optimal"``: the
    one-to-one matching with the most pairs and, among those, the least sum of 1 - IoU, in both association stages (at most 4096 rows per
    frame).  ``TrackModel()`` is alpha-beta and greedy: the results of ``Tracker`` without a model, through the other entry point."""

    def __init__(self, motion: str = "alpha_beta", assign: str = "greedy", q_pos: float = 1 / 20, q_vel: float = 1 / 160, r_pos: float = 1 / 20,
                 init_pos: float = 2.0, init_vel: float = 10.0, min_scale: float = 1.0):
        if motion not in MOTIONS:
            raise ValueError(f"motion: one of {sorted(MOTIONS)}, got {motion!r}")
        if assign not in ASSIGNS:
            raise ValueError(f"assign: one of {sorted(ASSIGNS)}, got {assign!r}")
        weights = dict(q_pos=q_pos, q_vel=q_vel, r_pos=r_pos, init_pos=init_pos, init_vel=init_vel)
        for name, v in weights.items():
            if not (isinstance(v, numbers.Real) and np.isfinite(np.float32(v)) and float(v) >= 0.0):
                raise ValueError(f"{name} is a finite number >= 0, got {v!r}")
        if not (isinstance(min_scale, numbers.Real) and np.isfinite(np.float32(min_scale)) and np.float32(min_scale) > 0.0):
            raise ValueError(f"min_scale is a finite number > 0, got {min_scale!r}")
        self.motion, self.assign, self.min_scale = motion, assign, float(min_scale)
        for name, v in weights.items():
            setattr(self, name, float(v))

    def __repr__(self):
        return (f"TrackModel(motion={self.motion!r}, assign={self.assign!r}, q_pos={self.q_pos}, q_vel={self.q_vel}, r_pos={self.r_pos}, "
                f"init_pos={self.init_pos}, init_vel={self.init_vel}, min_scale={self.min_scale})")

    @staticmethod
    def of(value) -> Optional["TrackModel"]:
        """None, a ``TrackModel`` or a dict of its keywords -> None or the ``TrackModel``"""
        if value is None or isinstance(value, TrackModel):
            return value
        if isinstance(value, dict):
            return TrackModel(**value)
        raise ValueError(f"model: None, a TrackModel or a dict of its keywords, got {type(value).__name__}")

    def check_rows(self, max_det: int) -> None:
        """``ValueError`` when frames of ``max_det`` rows are more than the association takes: a shape check, nothing is read"""
        if self.assign == "optimal" and max_det > OPTIMAL_MAX_DET:
            raise ValueError(f"rows: assign='optimal' takes at most {OPTIMAL_MAX_DET} rows per frame, got K = {max_det}")

    def struct(self) -> TrackModelStruct:
        return TrackModelStruct(MOTIONS[self.motion], ASSIGNS[self.assign], self.q_pos, self.q_vel, self.r_pos, self.init_pos, self.init_vel,
                                self.min_scale)


def check_params(**params) -> dict:
    """The parameters of ``Tracker`` with the defaults filled in; ``ValueError`` for an unknown name or a value outside its range."""
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise ValueError(f"Tracker: unknown parameter(s) {sorted(unknown)}; known: {sorted(DEFAULTS)}")
    p = {**DEFAULTS, **params}
    for name in ("high", "new_score", "iou_high", "iou_low"):
        if not 0.0 <= float(p[name]) <= 1.0:
            raise ValueError(f"Tracker: {name} = {p[name]} lies outside [0, 1]")
    for name in ("alpha", "beta"):
        if not np.isfinite(float(p[name])):
            raise ValueError(f"Tracker: {name} = {p[name]} is not a number")
    if int(p["min_hits"]) != p["min_hits"] or int(p["min_hits"]) < 1:
        raise ValueError("Tracker: min_hits is an integer >= 1")
    if int(p["max_age"]) != p["max_age"] or int(p["max_age"]) < 0:
        raise ValueError("Tracker: max_age is an integer >= 0")
    return p


class Tracker:
    """``streams`` independent trackers on ``device``.  The parameters (``high``, ``new_score``, ``iou_high``, ``iou_low``, ``alpha``,
    ``beta``, ``min_hits``, ``max_age``, ``class_agnostic``) default to ``DEFAULTS``.  ``model``: None for the alpha-beta filter and the
    greedy association through ``cvx_track_update``, or a ``TrackModel`` (or a dict of its keywords) for ``cvx_track_update_model``; the
    tracker then also owns the extension block with the covariances.  Under ``motion="kalman"`` ``alpha`` and ``beta`` are ignored."""

    def __init__(self, device, streams: int = 1, model=None, **params):
        self.params = check_params(**params)
        self.model = TrackModel.of(model)
        if int(streams) != streams or not 1 <= int(streams) <= 65535:
            raise ValueError("Tracker: streams is an integer in [1, 65535]")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.CvxError(f"Tracker runs on an MI355X only (device {self.device}): there is no CPU path")
        self.streams = int(streams)
        p = self.params
        self._c_params = TrackParams(p["high"], p["new_score"], p["iou_high"], p["iou_low"], p["alpha"], p["beta"], int(p["min_hits"]),
                                     int(p["max_age"]), int(bool(p["class_agnostic"])), 0)
        need = int(L.load().cvx_track_state_bytes(self.streams))
        if need != self.streams * STREAM_DTYPE.itemsize:
            raise L.CvxError(f"cvx_track_state_bytes({self.streams}) = {need}: the library's state layout is not this binding's")
        self.state = torch.zeros(need, dtype=torch.uint8, device=self.device)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.ext = None
        if self.model is not None:
            self._c_model = self.model.struct()
            need = int(L.load().cvx_track_ext_bytes(self.streams))
            if need != self.streams * EXT_BYTES:
                raise L.CvxError(f"cvx_track_ext_bytes({self.streams}) = {need}: the library's extension layout is not this binding's")
            self.ext = torch.zeros(need, dtype=torch.uint8, device=self.device)

    def update(self, rows: torch.Tensor, counts: torch.Tensor, frame_stream: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``cvx_track_update`` (``cvx_track_update_model`` with a model): rows (B, K, 6) fp32 and counts (B) int32 as ``det_to_image`` / ``merge_tiles`` leave them, the frames in time
        order; ``frame_stream`` (B) int32 on the device names each frame's stream (None: all stream 0).  Returns ids (B, K) int32 on the
        device, -1 where a row has no track (yet).  No host read.  ``assign="optimal"`` takes K <= 4096."""
        if self.model is not None and torch.is_tensor(rows) and rows.dim() == 3:
            self.model.check_rows(int(rows.shape[1]))
        if not (torch.is_tensor(rows) and rows.is_cuda):
            raise L.CvxError("Tracker.update runs on an MI355X only: there is no CPU path")
        if rows.dim() != 3 or rows.shape[2] != 6 or rows.dtype != torch.float32 or rows.shape[0] <= 0 or rows.shape[1] <= 0 or rows.device != self.device:
            raise ValueError(f"rows: (B, K, 6) float32 on {self.device}, got {tuple(rows.shape)} {rows.dtype} on {rows.device}")
        B, K = int(rows.shape[0]), int(rows.shape[1])
        if counts.dtype != torch.int32 or counts.numel() != B or counts.device != rows.device:
            raise ValueError("counts: (B) int32 on the rows' device")
        if frame_stream is not None and (not torch.is_tensor(frame_stream) or frame_stream.dtype != torch.int32 or frame_stream.numel() != B
                                         or frame_stream.device != rows.device):
            raise ValueError("frame_stream: (B) int32 on the rows' device")
        rows, counts = rows.contiguous(), counts.contiguous()
        frame_stream = None if frame_stream is None else frame_stream.contiguous()
        ids = torch.empty(B, K, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            if self.model is None:
                L.check(L.load().cvx_track_update(L.ptr(rows), L.ptr(counts), B, K, L.ptr(frame_stream), self.streams, C.byref(self._c_params),
                                                  L.ptr(self.state), L.ptr(ids), L.ptr(self.overflow), L.stream_ptr(self.device)), "cvx_track_update")
            else:
                L.check(L.load().cvx_track_update_model(L.ptr(rows), L.ptr(counts), B, K, L.ptr(frame_stream), self.streams, C.byref(self._c_params),
                                                        C.byref(self._c_model), L.ptr(self.state), L.ptr(self.ext), L.ptr(ids), L.ptr(self.overflow),
                                                        L.stream_ptr(self.device)), "cvx_track_update_model")
        return ids

    def reset(self, stream: Optional[int] = None) -> None:
        """Forgets the tracks, the frame count, the ids and the covariances of one stream, or of all (and then the overflow word too): memsets."""
        if stream is None:
            self.state.zero_()
            self.overflow.zero_()
            if self.ext is not None:
                self.ext.zero_()
            return
        if not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream {stream} outside [0, {self.streams})")
        n = STREAM_DTYPE.itemsize
        self.state[int(stream) * n:(int(stream) + 1) * n].zero_()
        if self.ext is not None:
            self.ext[int(stream) * EXT_BYTES:(int(stream) + 1) * EXT_BYTES].zero_()

    def tracks(self, stream: int = 0) -> dict:
        """ONE host read: the live tracks of ``stream`` sorted by id, as numpy arrays ``id`` (n) int32, ``box`` (n, 4) float32 (the position
        after the last update), ``velocity`` (n, 4) float32 per frame, ``cls`` (n) float32, ``hits`` and ``miss`` (n) int32; also ``frame``
        and ``next_id``.  Under ``motion="kalman"`` also ``cov`` (n, 3) float32, (Pxx, Pxv, Pvv) of each track, with a second host read."""
        if not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream {stream} outside [0, {self.streams})")
        n = STREAM_DTYPE.itemsize
        s = self.state[int(stream) * n:(int(stream) + 1) * n].cpu().numpy().view(STREAM_DTYPE)[0]
        live = min(max(int(s["n_tracks"]), 0), TRACK_CAP)
        order = np.argsort(s["id"][:live], kind="stable")
        out = {"id": s["id"][:live][order].copy(), "box": s["p"][:live][order].copy(), "velocity": s["v"][:live][order].copy(),
                "cls": s["cls"][:live][order].copy(), "hits": s["hits"][:live][order].copy(), "miss": s["miss"][:live][order].copy(),
                "frame": int(s["frame"]), "next_id": int(s["next_id"])}
        if self.model is not None and self.model.motion == "kalman":
            cov = self.ext[int(stream) * EXT_BYTES:(int(stream) + 1) * EXT_BYTES].cpu().numpy().view("<f4").reshape(TRACK_CAP, 4)
            out["cov"] = cov[:live, :3][order].copy()
        return out

    def overflowed(self) -> int:
        """ONE host read: how often a frame was dropped (a bad count or stream) or a birth skipped because a stream held ``TRACK_CAP`` tracks."""
        return int(self.overflow.item())
