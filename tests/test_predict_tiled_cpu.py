"""CPU: tiled prediction's host side -- ``tile_grid`` by hand and by property, the numpy restatement of the merge (tests/tiled_restatement.py)
on hand-derived cases, the new symbols, and the algorithm surface that needs no GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import tiled_restatement as TR
from computervision.pytorch_amd import LIB_PATH, CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import render as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- tile_grid ----------------------------------------------------------------------------------------------------------------------------
def test_tile_grid_by_hand():
    # stride 64 - int(64 * 0.25) = 48: 0 fits (0 + 64 < 100), 48 does not (112 >= 100), the last tile sits at 100 - 64 = 36
    assert R.tile_grid(100, 100, (64, 64), 0.25) == [(0, 0, 64, 64), (0, 36, 64, 64), (36, 0, 64, 64), (36, 36, 64, 64)]
    # smaller than the tile in one axis: one tile of the frame's own extent there
    assert R.tile_grid(40, 100, (64, 64), 0.25) == [(0, 0, 40, 64), (0, 36, 40, 64)]
    assert R.tile_grid(100, 64, (64, 64), 0.25) == [(0, 0, 64, 64), (36, 0, 64, 64)]
    # smaller in both, and the exact fit
    assert R.tile_grid(20, 30, (32, 48), 0.25) == [(0, 0, 20, 30)]
    assert R.tile_grid(64, 64, (64, 64), 0.25) == [(0, 0, 64, 64)]
    # overlap 0: stride = tile; 0, 64 (64 + 64 < 150), then 150 - 64 = 86; an exact multiple emits no start twice
    assert [t[1] for t in R.tile_grid(10, 150, (64, 64), 0.0)] == [0, 64, 86]
    assert [t[1] for t in R.tile_grid(10, 128, (64, 64), 0.0)] == [0, 64]
    # rectangular tiles: strides 32 - 8 = 24 and 48 - 12 = 36
    assert R.tile_grid(37, 53, (32, 48), 0.25) == [(0, 0, 32, 48), (0, 5, 32, 48), (5, 0, 32, 48), (5, 5, 32, 48)]
    assert [t[0] for t in R.tile_grid(96, 10, (32, 48), 0.25)] == [0, 24, 48, 64]


def test_tile_grid_refuses_bad_overlaps():
    for overlap in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            R.tile_grid(100, 100, (64, 64), overlap)
    with pytest.raises(ValueError):
        R.tile_grid(0, 100, (64, 64), 0.2)


def test_tile_grid_covers_the_frame_and_stays_inside():
    rng = np.random.RandomState(0)
    for _ in range(300):
        h, w = int(rng.randint(1, 400)), int(rng.randint(1, 400))
        TH, TW = int(rng.randint(1, 130)), int(rng.randint(1, 130))
        overlap = float(rng.choice([0.0, 0.1, 0.2, 0.25, 0.5, 0.9]))
        if TH - int(TH * overlap) < 1 or TW - int(TW * overlap) < 1:
            continue
        grid = R.tile_grid(h, w, (TH, TW), overlap)
        seen = np.zeros((h, w), bool)
        for y0, x0, th, tw in grid:
            assert 0 <= y0 and 0 <= x0 and y0 + th <= h and x0 + tw <= w
            assert th == min(TH, h) and tw == min(TW, w)
            seen[y0:y0 + th, x0:x0 + tw] = True
        assert seen.all(), (h, w, TH, TW, overlap)
        assert len(set(grid)) == len(grid) and grid == sorted(grid)          # no start twice; row-major


# ---- the restatement's merge on hand-derived cases ----------------------------------------------------------------------------------------
FRAME_HW = [[100, 200]]


def blocks(per_slot, K=4):
    rows = np.zeros((len(per_slot), K, 6), np.float32)
    for s, r in enumerate(per_slot):
        rows[s, :len(r)] = r
    return rows, np.array([len(r) for r in per_slot], np.int32)


def test_merge_partial_box_goes_under_ios_and_stays_under_iou():
    # an object at [70, 10, 130, 50] of the frame: the tile over x in [0, 96) sees its left 26 columns, the tile at x0 = 64 all of it.
    # inter = 26 * 40 = 1040 = the smaller area: IoS = 1 > 0.5; IoU = 1040 / (1040 + 2400 - 1040) = 0.433 < 0.5
    rows, counts = blocks([[[70, 10, 96, 50, 0.6, 3]], [[6, 10, 66, 50, 0.9, 3]]])
    slot_map = [[0, 0, 0, 0], [0, 64, 0, 0]]
    out, n, src, ov = TR.merge(rows, counts, slot_map, FRAME_HW, "ios", 0.5)
    assert n.tolist() == [1] and src[0, :2].tolist() == [4, -1] and ov == 0
    assert out[0, 0].tolist() == [70, 10, 130, 50, np.float32(0.9), 3] and not out[0, 1:].any()
    out, n, src, ov = TR.merge(rows, counts, slot_map, FRAME_HW, "iou", 0.5)
    assert n.tolist() == [2] and src[0, :3].tolist() == [4, 0, -1]
    assert out[0, 1].tolist() == [70, 10, 96, 50, np.float32(0.6), 3]


def test_merge_class_aware_against_agnostic():
    rows, counts = blocks([[[10, 10, 50, 50, 0.9, 1], [10, 10, 50, 50, 0.8, 2]]])
    assert TR.merge(rows, counts, [[0, 0, 0, 0]], FRAME_HW, "ios", 0.5, class_agnostic=False)[1].tolist() == [2]
    out, n, src, _ = TR.merge(rows, counts, [[0, 0, 0, 0]], FRAME_HW, "ios", 0.5, class_agnostic=True)
    assert n.tolist() == [1] and out[0, 0, 5] == 1 and src[0, :2].tolist() == [0, -1]


def test_merge_equal_scores_the_lower_ordinal_wins():
    rows, counts = blocks([[[0, 0, 1, 1, 0.9, 0]], [[10, 10, 50, 50, 0.5, 1]], [[0, 10, 40, 50, 0.5, 1]]])
    slot_map = [[0, 150, 50, 0], [0, 0, 0, 0], [0, 10, 0, 0]]          # slots 1 and 2 hold the same frame box with the same score
    out, n, src, _ = TR.merge(rows, counts, slot_map, FRAME_HW, "iou", 0.5)
    assert n.tolist() == [2] and src[0, :3].tolist() == [0, 4, -1]
    rows[1, 0], rows[2, 0] = rows[2, 0].copy(), rows[1, 0].copy()      # the other way round: still the lower ordinal
    slot_map[1], slot_map[2] = slot_map[2], slot_map[1]
    assert TR.merge(rows, counts, slot_map, FRAME_HW, "iou", 0.5)[2][0, :3].tolist() == [0, 4, -1]


def test_merge_max_det_cut_clamp_and_bad_counts():
    disjoint = [[20 * k, 0, 20 * k + 10, 10, 0.1 * (k + 1), 0] for k in range(5)]
    rows, counts = blocks([disjoint[:3], disjoint[3:]], K=4)
    out, n, src, ov = TR.merge(rows, counts, [[0, 0, 0, 0], [0, 0, 0, 0]], FRAME_HW, "ios", 0.5, max_det=3)
    assert n.tolist() == [3] and src[0].tolist() == [5, 4, 2] and out.shape == (1, 3, 6)          # scores 0.5, 0.4, 0.3
    # clamping to the frame (h 100, w 200), after the slot offset
    rows, counts = blocks([[[-5, -3, 250, 120, 0.9, 0]], [[150, 90, 190, 99, 0.8, 0]]])
    out, n, _, _ = TR.merge(rows, counts, [[0, 0, 0, 0], [0, 30, 20, 0]], FRAME_HW, "iou", 0.5)
    assert n.tolist() == [2] and out[0, 0, :4].tolist() == [0, 0, 200, 100] and out[0, 1, :4].tolist() == [180, 100, 200, 100]
    # a count outside [0, K] contributes nothing and is flagged; a frame without slots is empty
    rows, counts = blocks([disjoint[:2], disjoint[2:4]])
    counts[1] = -1
    out, n, src, ov = TR.merge(rows, counts, [[1, 0, 0, 0], [1, 0, 0, 0]], [[100, 200], [100, 200]], "ios", 0.5)
    assert n.tolist() == [0, 2] and ov == 1 and (src[0] == -1).all() and not out[0].any()
    counts[1] = 5
    assert TR.merge(rows, counts, [[1, 0, 0, 0], [1, 0, 0, 0]], [[100, 200], [100, 200]], "ios", 0.5)[3] == 1


def test_merge_degenerate_box_does_not_suppress():
    # two copies of a box without area: inter = 0 and the smaller area = 0, 0 / 0 is NaN, and NaN > threshold is false -- under both metrics
    rows, counts = blocks([[[10, 10, 10, 20, 0.9, 0], [10, 10, 10, 20, 0.8, 0]]])
    for metric in ("ios", "iou"):
        assert TR.merge(rows, counts, [[0, 0, 0, 0]], FRAME_HW, metric, 0.0)[1].tolist() == [2]
    # capacity: one candidate too many is flagged with count -1, never truncated
    many = np.zeros((2, 4097, 6), np.float32)
    many[..., 2:5] = 1
    out, n, _, ov = TR.merge(many, [4096, 4096], [[0, 0, 0, 0]] * 2, FRAME_HW, "ios", 0.5, max_det=2)
    assert n.tolist() == [1] and ov == 0
    out, n, _, ov = TR.merge(many, [4096, 4097], [[0, 0, 0, 0]] * 2, FRAME_HW, "ios", 0.5, max_det=2)
    assert n.tolist() == [-1] and ov == 1 and not out.any()


# ---- ABI and surface ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name in ("cvx_tiles_u8_to_nchw", "cvx_det_merge_tiles", "cvx_det_merge_workspace_bytes"):
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
    assert len(L.PROTOTYPES["cvx_tiles_u8_to_nchw"][1]) == 7 and len(L.PROTOTYPES["cvx_det_merge_tiles"][1]) == 18
    assert len(L.PROTOTYPES["cvx_det_merge_workspace_bytes"][1]) == 1
    assert "cvx_tile_job" in header and R.TILE_JOB_DTYPE.itemsize == 40
    assert "tiles.hip" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_predict_tiled_on_the_four_detectors_and_not_on_deeplab():
    from configs import CenternetConfig, SsdConfig, Yolo7Config, Yolo8DetConfig
    from core.algorithms.centernet import CenterNetA
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    from core.algorithms.ssd import Ssd
    from core.algorithms.yolo_v7 import YOLOv7
    from core.algorithms.yolo_v8 import YOLOv8
    from scripts import detect
    frame = torch.zeros(200, 300, 3, dtype=torch.uint8)
    for cls, cfg in ((YOLOv8, Yolo8DetConfig), (YOLOv7, Yolo7Config), (Ssd, SsdConfig), (CenterNetA, CenternetConfig)):
        algo = cls(cfg(), "cpu")
        with pytest.raises(CvxError):                                       # no CPU path
            algo.predict_tiled(None, [frame])
        with pytest.raises(CvxError):
            algo.detect_frames(None, [frame], 2, tiled={"overlap": 0.25})
    assert "tiled" in inspect.signature(YOLOv8.detect_frames).parameters and "tiled" in inspect.signature(detect.detect_frames).parameters
    assert "tiled" in inspect.signature(detect.detect_video).parameters
    keywords = inspect.signature(YOLOv8.predict_tiled).parameters
    assert [keywords[k].default for k in ("overlap", "full_frame", "match", "match_threshold", "class_agnostic", "max_det", "conf_threshold",
                                          "batch_size", "draw", "sync")] == [0.2, True, "ios", 0.5, False, 300, None, 32, False, True]
    assert not hasattr(DeeplabV3PlusA, "predict_tiled")                     # stitching logits is another feature


def test_merge_tiles_refuses_host_tensors():
    rows, counts = torch.zeros(2, 4, 6), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(CvxError):
        R.merge_tiles(rows, counts, torch.zeros(2, 4, dtype=torch.int32), torch.ones(1, 2, dtype=torch.int32))
    with pytest.raises(CvxError):
        R.TileBatch([torch.zeros(20, 30, 3, dtype=torch.uint8)], (32, 48))
