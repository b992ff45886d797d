"""CPU: sliding-window segmentation's host side -- the numpy restatement of the stitch (tests/seg_tiled_restatement.py) on hand-derived
cases, the new symbol and structs, and the surface that needs no GPU.

The strip cases use constant logits per tile (a 1 x 1 feature map), so the blended value of class c at a pixel is just the sum of
weight * logit over the covering tiles and every expectation below is worked out by hand from the weight rule
``min(dy + 1, th - dy) * min(dx + 1, tw - dx)``.  A tile's weight falls towards ITS borders: in the overlap [4, 8) of two 1 x 8 tiles at
x = 0 and x = 4 the left tile weighs 4, 3, 2, 1 and the right one 1, 2, 3, 4."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import seg_tiled_restatement as SR
from computervision.pytorch_amd import LIB_PATH, CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import render as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def constant_slot(nc, cls, value=1.0):
    """the rows of a slot with a 1 x 1 feature map: class ``cls`` = value, the others 0"""
    rows = np.zeros((1, nc), np.float32)
    if cls is not None:
        rows[0, cls] = value
    return rows


STRIP = dict(frame_hw=(1, 12), tiles=[(0, 0, 1, 8), (0, 4, 1, 8)], nc=3, lh=1, lw=1, NH=1, NW=8)


def test_strip_grid_is_what_tile_grid_gives():
    # stride 8 - int(8 * 0.5) = 4: 0 fits (0 + 8 < 12), 4 does not (4 + 8 >= 12), and the last tile sits at 12 - 8 = 4
    assert R.tile_grid(1, 12, (1, 8), 0.5) == STRIP["tiles"]


def test_mean_ties_in_the_overlap_go_to_the_lower_class():
    slots = [constant_slot(3, 1), constant_slot(3, 2)]
    # [0, 4): only tile A, class 1.  [4, 8): 1 * 1 for class 1 and 1 * 1 for class 2, a tie: the lower class.  [8, 12): only tile B
    assert SR.stitch(rows_per_slot=slots, weight="mean", **STRIP).tolist() == [[1] * 8 + [2] * 4]
    acc = SR.accumulate(rows_per_slot=slots, weight="mean", **STRIP)
    assert acc[1, 0].tolist() == [1] * 8 + [0] * 4 and acc[2, 0].tolist() == [0] * 4 + [1] * 8 and not acc[0].any()


def test_linear_weights_by_hand():
    assert SR.tile_weight(1, 8, "linear").tolist() == [[1, 2, 3, 4, 4, 3, 2, 1]]
    assert SR.tile_weight(3, 5, "linear").tolist() == [[1, 2, 3, 2, 1], [2, 4, 6, 4, 2], [1, 2, 3, 2, 1]]
    assert SR.tile_weight(2, 2, "mean").tolist() == [[1, 1], [1, 1]]
    with pytest.raises(ValueError):
        SR.tile_weight(2, 2, "gauss")


def test_linear_switch_falls_strictly_inside_the_overlap():
    slots = [constant_slot(3, 1), constant_slot(3, 2)]
    # overlap [4, 8): class 1 has 4, 3, 2, 1 (tile A, dx = 4 .. 7), class 2 has 1, 2, 3, 4 (tile B, dx = 0 .. 3): 4 > 1, 3 > 2, 2 < 3, 1 < 4
    acc = SR.accumulate(rows_per_slot=slots, weight="linear", **STRIP)
    assert acc[1, 0].tolist() == [1, 2, 3, 4, 4, 3, 2, 1, 0, 0, 0, 0] and acc[2, 0].tolist() == [0, 0, 0, 0, 1, 2, 3, 4, 4, 3, 2, 1]
    assert SR.stitch(rows_per_slot=slots, weight="linear", **STRIP).tolist() == [[1] * 6 + [2] * 6]


def test_linear_class_one_wins_throughout_the_overlap():
    # tile A says class 1 with logit 5: 20, 15, 10, 5 against tile B's 1, 2, 3, 4 -- class 1 throughout the overlap, class 2 begins at x = 8
    slots = [constant_slot(3, 1, 5.0), constant_slot(3, 2)]
    acc = SR.accumulate(rows_per_slot=slots, weight="linear", **STRIP)
    assert acc[1, 0, 4:8].tolist() == [20, 15, 10, 5] and acc[2, 0, 4:8].tolist() == [1, 2, 3, 4]
    assert SR.stitch(rows_per_slot=slots, weight="linear", **STRIP).tolist() == [[1] * 8 + [2] * 4]
    # the other way round the switch moves to the overlap's first pixel: 4, 3, 2, 1 against 5, 10, 15, 20
    slots = [constant_slot(3, 1), constant_slot(3, 2, 5.0)]
    assert SR.stitch(rows_per_slot=slots, weight="linear", **STRIP).tolist() == [[1] * 4 + [2] * 8]


def test_equal_logits_give_class_zero_everywhere():
    for weight in SR.WEIGHTS:
        for value in (0.0, 0.75):
            slots = [np.full((1, 3), value, np.float32)] * 2
            assert not SR.stitch(rows_per_slot=slots, weight=weight, **STRIP).any()


def test_two_dimensional_weights_and_row_major_order():
    # a 3 x 3 frame, 2 x 2 tiles at stride 1: the centre pixel is covered by all four tiles, with weight 1 in each of them
    tiles = R.tile_grid(3, 3, (2, 2), 0.5)
    assert tiles == [(0, 0, 2, 2), (0, 1, 2, 2), (1, 0, 2, 2), (1, 1, 2, 2)]
    slots = [constant_slot(4, c, v) for c, v in ((0, 1.0), (1, 1.0), (2, 1.0), (3, 2.0))]
    got = SR.stitch((3, 3), tiles, slots, 4, 1, 1, 2, 2, "linear")
    # every 2 x 2 tile weighs 1 everywhere.  (0, 0): tile 0 only.  (0, 1): tiles 0 and 1 tie, class 0.  (1, 1): all four, class 3 has 2.
    # (1, 0): tiles 0 and 2 tie, class 0.  (1, 2): tiles 1 (1) and 3 (2).  (2, 1): tiles 2 (1) and 3 (2).  (0, 2): tile 1.  (2, 0): tile 2.
    assert got.tolist() == [[0, 0, 1], [0, 3, 3], [2, 3, 3]]


def test_a_frame_smaller_than_the_tile_uses_its_own_extent_in_the_weight():
    # network input 1 x 8, frame 1 x 5: one tile of extent 5 -- weights 1, 2, 3, 2, 1 (not 1, 2, 3, 4, 4) -- and the taps of a FULL input:
    # a 1 x 2 feature map at scale 2 / 8 has lam = max((dx + .5) / 4 - .5, 0) = 0, 0, .125, .375, .625 at dx = 0 .. 4
    tiles = R.tile_grid(1, 5, (1, 8), 0.2)
    assert tiles == [(0, 0, 1, 5)]
    rows = np.array([[8.0, 0.0], [0.0, 8.0]], np.float32)                 # feature pixel 0: class 0 = 8, pixel 1: class 1 = 8
    acc = SR.accumulate((1, 5), tiles, [rows], 2, 1, 2, 1, 8, "linear")
    assert acc[0, 0].tolist() == [8, 16, 21, 10, 3] and acc[1, 0].tolist() == [0, 0, 3, 6, 5]
    assert SR.stitch((1, 5), tiles, [rows], 2, 1, 2, 1, 8, "linear").tolist() == [[0, 0, 0, 0, 1]]
    assert SR.slot_logits(rows, 2, 1, 2, 1, 8, 1, 5)[1, 0].tolist() == [0, 0, 1, 3, 5]


def test_confusion_ignores_targets_outside_the_classes_and_overlay_blends():
    labels = np.array([[0, 1, 2], [2, 2, 1]], np.uint8)
    target = np.array([[0, 1, 1], [2, 255, 3]], np.uint8)
    want = np.zeros((3, 3), np.int64)
    want[0, 0] = want[1, 1] = want[1, 2] = want[2, 2] = 1                  # (255 -> 2) and (3 -> 1) are not counted
    got = SR.confusion(labels, target, 3)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    lut = np.array([[0, 0, 0], [128, 0, 0], [1, 255, 3]], np.uint8)
    frame = np.full((2, 3, 3), 2, np.uint8)
    out = SR.overlay(frame, labels, lut)
    # (2 + 0) / 2 = 1; (2 + 128) / 2 = 65; (2 + 1) / 2 = 1.5 -> 2 (even), (2 + 255) / 2 = 128.5 -> 128 (even), (2 + 3) / 2 = 2.5 -> 2 (even)
    assert out[0, 0].tolist() == [1, 1, 1] and out[0, 1].tolist() == [65, 1, 1] and out[0, 2].tolist() == [2, 128, 2]
    assert np.array_equal(SR.overlay(frame, labels, lut, bgr=True), out[..., ::-1])


def test_slot_chunks_are_equal_but_for_the_last():
    assert R.slot_chunks(30, 16) == [(0, 15), (15, 30)] and R.slot_chunks(9, 4) == [(0, 3), (3, 6), (6, 9)]
    assert R.slot_chunks(7, 4) == [(0, 4), (4, 7)] and R.slot_chunks(10, 4) == [(0, 4), (4, 8), (8, 10)] and R.slot_chunks(5, 16) == [(0, 5)] and R.slot_chunks(8, 4) == [(0, 4), (4, 8)]
    for slots in range(1, 70):
        for b in range(1, 20):
            chunks = R.slot_chunks(slots, b)
            sizes = [c1 - c0 for c0, c1 in chunks]
            assert chunks[0][0] == 0 and chunks[-1][1] == slots and all(a[1] == c[0] for a, c in zip(chunks, chunks[1:]))
            assert max(sizes) <= b and len(chunks) == -(-slots // b) and len(set(sizes[:-1])) <= 1 and 1 <= sizes[-1] <= sizes[0]
    with pytest.raises(ValueError):
        R.slot_chunks(4, 0)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_new_symbol_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    assert "cvx_seg_stitch" in declared and "cvx_seg_stitch" in L.PROTOTYPES and (lib is None or hasattr(lib, "cvx_seg_stitch"))
    assert len(L.PROTOTYPES["cvx_seg_stitch"][1]) == 23
    assert "cvx_seg_tile_frame" in header and "cvx_seg_map" in header
    assert R.SEG_TILE_FRAME_DTYPE.itemsize == 24 and R.SEG_MAP_DTYPE.itemsize == 16
    assert R.SEG_TILE_FRAME_DTYPE.names == ("first_slot", "ny", "nx", "y_off", "x_off", "reserved")
    assert "\"seg_tiles.hip\"" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert os.path.exists(os.path.join(ROOT, "computervision.pytorch_amd", "csrc", "seg_tiles.hip"))


# ---- surface ------------------------------------------------------------------------------------------------------------------------------
def test_segment_tiled_surface():
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    from core.trainer.segmentation_trainer import SegmentationMetrics
    from scripts import detect
    keywords = inspect.signature(DeeplabV3PlusA.segment_tiled).parameters
    assert list(keywords)[:3] == ["self", "model", "frames"]
    assert [keywords[k].default for k in ("overlap", "weight", "batch_size", "draw", "bgr", "targets", "metrics", "sync")] == \
        [0.2, "linear", 16, True, False, None, None, False]
    assert not hasattr(DeeplabV3PlusA, "predict_tiled")                     # the detectors' name stays theirs
    assert list(inspect.signature(DeeplabV3PlusA.segment_frames).parameters)[:4] == ["self", "model", "frames", "batch_size"]
    assert callable(detect.segment_video) and callable(detect.segment_frames)
    algo = DeeplabV3PlusA(DeeplabV3PlusConfig(), "cpu")
    frame = torch.zeros(200, 300, 3, dtype=torch.uint8)
    with pytest.raises(CvxError):                                           # no CPU path
        algo.segment_tiled(None, [frame])
    with pytest.raises(CvxError):
        algo.segment_frames(None, [frame], 2)
    with pytest.raises(CvxError):                                           # and detect_frames(tiled=...) keeps refusing DeepLab
        algo.detect_frames(None, [frame], 2, tiled={"overlap": 0.25})
    m = SegmentationMetrics(3)
    counts = m.add_labels_counts("cpu")
    assert counts is m.counts and counts.dtype == torch.int64 and tuple(counts.shape) == (3, 3) and not counts.any()
    counts[1, 2] += 5
    assert m.add_labels_counts("cpu") is counts and m.fold()[1, 2] == 5 and not m.counts.any()


def test_stitch_segmentation_refuses_host_tensors_and_bad_arguments():
    frames = [torch.zeros(20, 30, 3, dtype=torch.uint8)]
    rows = torch.zeros(1, 8 * 12, 4)
    good = dict(nc=3, level_hw=(8, 12), net_hw=(32, 48), tile_batch=None)
    with pytest.raises(CvxError):                                           # there is no CPU path
        R.stitch_segmentation(frames, rows, **good)
    for bad in (dict(weight="gauss"), dict(nc=257), dict(nc=0), dict(nc=5),            # nc 5 > ld 4
                dict(level_hw=(8, 13)),                                                  # 8 * 13 rows expected, 96 given
                dict(targets=[torch.zeros(20, 30, dtype=torch.uint8)]),                  # targets without counts
                dict(counts=torch.zeros(3, 3, dtype=torch.int64))):
        with pytest.raises(ValueError):
            R.stitch_segmentation(frames, rows, **{**good, **bad})
    with pytest.raises(ValueError):
        R.stitch_segmentation(frames, rows.double(), **good)
    with pytest.raises(ValueError):
        R.stitch_segmentation(frames, rows[0], **good)
    with pytest.raises(ValueError):                                         # the LDS histogram holds 128 x 128 entries
        R.stitch_segmentation(frames, torch.zeros(1, 96, 136), **{**good, "nc": 129}, targets=[torch.zeros(20, 30, dtype=torch.uint8)],
                              counts=torch.zeros(129, 129, dtype=torch.int64))
