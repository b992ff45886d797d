"""CPU: the COCO metric's host side.  pycocotools is not installed, so the sequential restatement (tests/coco_eval_restatement.py) is held
to answers derived by hand here; the VOC -> COCO conversion is held to what the reference's ``preprocess_gt`` / ``preprocess_dr`` made of
the fixture (tests/golden/coco_inputs_ref.npz, written by tools/make_coco_fixture.py); then the new symbols and the algorithm surface
that needs no GPU.

Every precision is ``tp / (fp + tp + np.spacing(1))``: a lone true positive has precision 1 / (1 + 2^-52) = 0.9999999999999998, not 1, so
"AP 1.0" below is ONE = that double, to 1e-15 for the mean's rounding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import coco_eval_restatement as C
import det_eval_restatement as R
from computervision.pytorch_amd import LIB_PATH, CvxError, coco_eval
from computervision.pytorch_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1.0 / (1.0 + np.spacing(1))
EPS = 1e-15


def gt(image, category, box, area=None, iscrowd=0):
    return dict(image=image, category=category, bbox=[float(v) for v in box], area=float(box[2] * box[3] if area is None else area), iscrowd=iscrowd)


def dt(image, category, box, score):
    return dict(image=image, category=category, bbox=[float(v) for v in box], score=float(score))


def test_thresholds_as_numpy_makes_them():
    assert np.array_equal(coco_eval.IOU_THRS, C.IOU_THRS) and np.array_equal(coco_eval.REC_THRS, C.REC_THRS)
    assert C.IOU_THRS[0] == 0.5 and C.IOU_THRS[5] == 0.75 and C.IOU_THRS[8] != 0.9       # 0.8999999999999999
    assert C.AREA_RNG == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]


def test_perfect_detections():
    """three images, two classes, every detection its ground truth's own box, small and medium ones only: all twelve are 1.0 apart from
    the -1 of the empty "large" bin"""
    gts = [gt(0, 0, (10, 10, 20, 20)), gt(0, 1, (50, 50, 40, 40)), gt(1, 0, (5, 5, 8, 8)), gt(2, 1, (0, 0, 50, 60))]
    dts = [dt(g["image"], g["category"], g["bbox"], 0.9 - 0.1 * i) for i, g in enumerate(gts)]
    out = C.coco_eval(gts, dts, range(3), 2)
    want = np.array([ONE] * 5 + [-1.0] + [1.0] * 5 + [-1.0])      # maxDets cuts per (image, category), each of which has one detection
    assert np.abs(out["stats"] - want).max() <= EPS, out["stats"]
    assert out["lines"][0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000"
    assert out["lines"][5] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000"


def test_one_ground_truth_tp_then_fp_and_fp_then_tp():
    """TP (score .9) then FP (.8): tp = [1, 1], fp = [0, 1], rc = [1, 1], pr = [ONE, 1 / 2]; every recall threshold finds index 0: 101
    points of ONE, AP = ONE at each of the ten thresholds.
    FP (.9) then TP (.8): tp = [0, 1], fp = [1, 1], rc = [0, 1], pr = [0, 1 / (2 + 2^-52) = 0.5 exactly -- 2 + 2^-52 rounds to 2]; the
    envelope lifts pr[0] to 0.5; threshold 0 finds index 0, the other 100 find index 1: 101 points of 0.5, AP = 101 * 0.5 / 101 = 0.5
    exactly (the sum of 1010 halves is exact)."""
    g = [gt(0, 0, (10, 10, 20, 20))]
    hit, miss = (10, 10, 20, 20), (100, 100, 20, 20)
    out = C.coco_eval(g, [dt(0, 0, hit, .9), dt(0, 0, miss, .8)], [0], 1)
    assert abs(out["stats"][0] - ONE) <= EPS and np.array_equal(out["precision"][:, :, 0, 0, 2], np.full((10, 101), ONE))
    out = C.coco_eval(g, [dt(0, 0, miss, .9), dt(0, 0, hit, .8)], [0], 1)
    assert out["stats"][0] == 0.5 and np.array_equal(out["precision"][:, :, 0, 0, 2], np.full((10, 101), 0.5))
    assert out["stats"][6] == 0.0 and out["stats"][7] == 1.0           # AR1: the first detection is the miss; AR10 has both


def test_iou_off_the_threshold():
    """IoU 70 / 100 to the lone ground truth: the double 0.7 is <= linspace's fifth value (also the double 0.7), so thresholds 0 .. 4
    match (the walk skips a ground truth only when its IoU is < the threshold) and 5 .. 9 do not: AP = 5 / 10 * ONE"""
    assert 70 / 100 == C.IOU_THRS[4] and int((C.IOU_THRS <= 70 / 100).sum()) == 5
    out = C.coco_eval([gt(0, 0, (0, 0, 10, 10))], [dt(0, 0, (0, 0, 7, 10), .9)], [0], 1)
    assert C.bbox_iou((0, 0, 7, 10), (0, 0, 10, 10), 0) == 0.7
    assert np.array_equal(out["precision"][:5, :, 0, 0, 2], np.full((5, 101), ONE)) and not out["precision"][5:, :, 0, 0, 2].any()
    assert abs(out["stats"][0] - 0.5 * ONE) <= EPS and abs(out["stats"][1] - ONE) <= EPS and out["stats"][2] == 0.0


def test_crowd_box_absorbs_two_detections():
    """two detections inside a crowd box (IoU = intersection / detection area = 1) outscore the true positive: both match the crowd box,
    are ignored, and the AP stays ONE; with iscrowd = 0 the second of them is a false positive ahead of the true positive"""
    normal = gt(0, 0, (200, 200, 20, 20))
    dts = [dt(0, 0, (12, 12, 10, 10), .95), dt(0, 0, (30, 30, 10, 10), .9), dt(0, 0, (200, 200, 20, 20), .5)]
    out = C.coco_eval([gt(0, 0, (10, 10, 40, 40), iscrowd=1), normal], dts, [0], 1)
    e = out["eval_imgs"][0][0][2][0]
    assert e["dt_ignore"][:, :2].all() and e["dt_matches"][:, :2].all() and not e["dt_ignore"][:, 2].any()
    assert abs(out["stats"][0] - ONE) <= EPS and out["npig"][0, 0] == 1
    out = C.coco_eval([gt(0, 0, (10, 10, 40, 40)), normal], dts, [0], 1)
    assert out["stats"][0] < 0.6


def test_area_boundaries_are_inclusive():
    """area 1024 is small and medium, area 9216 is medium and large; a detection's own area decides only when it is unmatched"""
    gts = [gt(0, 0, (0, 0, 32, 32)), gt(0, 1, (100, 100, 96, 96))]
    dts = [dt(0, 0, (0, 0, 32, 32), .9), dt(0, 1, (100, 100, 96, 96), .8)]
    out = C.coco_eval(gts, dts, [0], 2)
    assert out["npig"].tolist() == [[1, 1, 1, 0], [1, 0, 1, 1]]
    assert np.abs(out["stats"][[3, 4, 5, 9, 10, 11]] - [ONE, ONE, ONE, 1, 1, 1]).max() <= EPS
    out = C.coco_eval([gt(0, 0, (0, 0, 32, 32), area=1024.5)], dts[:1], [0], 1)
    assert out["npig"].tolist() == [[1, 0, 1, 0]]
    assert out["stats"][3] == -1 and abs(out["stats"][4] - ONE) <= EPS     # matched: the detection takes the ground truth's flag


def test_top_100_cut():
    """100 misses outscore the hit: it is detection 101 of its (image, category) and never evaluated; with 99 misses it is the 100th"""
    g = [gt(0, 0, (500, 500, 20, 20))]
    misses = [dt(0, 0, (10 * i, 0, 5, 5), 0.9 - 0.001 * i) for i in range(100)]
    hit = dt(0, 0, (500, 500, 20, 20), 0.1)
    out = C.coco_eval(g, misses + [hit], [0], 1)
    assert out["stats"][0] == 0.0 and out["stats"][8] == 0.0
    assert C.detection_masks(out["eval_imgs"], misses + [hit], 1)[0][-1] == 100
    out = C.coco_eval(g, misses[:99] + [hit], [0], 1)
    assert out["stats"][8] == 1.0 and out["stats"][7] == 0.0 and abs(out["stats"][0] - 1 / (100 + np.spacing(1))) <= EPS


def test_equal_iou_goes_to_the_later_ground_truth():
    gts = [gt(0, 0, (10, 10, 10, 10)), gt(0, 0, (14, 10, 10, 10))]
    dts = [dt(0, 0, (12, 10, 10, 10), .9), dt(0, 0, (12, 10, 10, 10), .8)]
    assert C.bbox_iou(dts[0]["bbox"], gts[0]["bbox"], 0) == C.bbox_iou(dts[0]["bbox"], gts[1]["bbox"], 0) > 0.65
    e = C.coco_eval(gts, dts, [0], 1)["eval_imgs"][0][0][2][0]
    assert e["dt_matches"][0].tolist() == [2, 1] and e["gt_matches"][0].tolist() == [2, 1]      # ids: the first detection took gt 2
    assert e["dt_matches"][4].tolist() == [0, 0]                                                # 2 / 3 < 0.7


@pytest.fixture(scope="module")
def fixture(gold):
    z = gold("coco_inputs_ref.npz")
    gts, dts, n = C.fixture_lists(z)
    return z, gts, dts, n, C.coco_eval(gts, dts, range(n), int(z["num_classes"]))


def test_max_det_prefix_property_on_the_fixture(fixture):
    """the greedy walk never looks ahead: evaluateImg at maxDet = m is the first m detections of evaluateImg at maxDet = 100 -- what
    cvx_coco_match relies on when it walks once and records the rank"""
    z, gts, dts, n, out = fixture
    checked = 0
    for k in range(int(z["num_classes"])):
        for a in range(4):
            for i in range(n):
                full = out["eval_imgs"][k][a][2][i]
                for mi, m in enumerate(C.MAX_DETS[:2]):
                    cut = out["eval_imgs"][k][a][mi][i]
                    assert (full is None) == (cut is None)
                    if full is None:
                        continue
                    assert cut["dt_ids"] == full["dt_ids"][:m] and cut["dt_scores"] == full["dt_scores"][:m]
                    assert np.array_equal(cut["dt_matches"], full["dt_matches"][:, :m]) and np.array_equal(cut["dt_ignore"], full["dt_ignore"][:, :m])
                    assert np.array_equal(cut["gt_ignore"], full["gt_ignore"])
                    checked += len(full["dt_ids"]) > m
    assert checked > 50
    assert (out["stats"] > 0).all() and 0.03 < out["stats"][0] < 0.95


def test_voc_conversion_equals_the_reference(fixture, gold):
    """the restatement's and the package's VOC -> COCO conversions against the arrays the reference's preprocess_gt / preprocess_dr made
    of the 40-image case, exactly (its annotation ids, numbered from 0 in os.listdir order, are not compared)"""
    z = fixture[0]
    vz = gold("det_map_ref.npz")
    dets, gts, (_, _, gt_arr, gt_counts) = R.fixture_inputs(vz)
    cg, cd = C.voc_to_coco_gt(gts), C.voc_to_coco_dt(dets)
    got_gt = np.array([[g["image"], g["category"] + 1] + g["bbox"] + [g["area"], g["iscrowd"]] for g in cg], np.float64)
    got_dt = np.array([[d["image"], d["category"] + 1] + d["bbox"] + [d["score"]] for d in cd], np.float64)
    assert np.array_equal(got_gt, z["ref_gt"][:, :8]) and np.array_equal(got_dt, z["ref_dt"])
    assert sorted(z["ref_gt"][:, 8].tolist()) == list(range(len(cg)))
    dev = coco_eval.voc_gt_to_coco(torch.from_numpy(gt_arr)).numpy()         # what evaluate_on_voc(coco_metric=True) feeds the kernel
    assert dev.dtype == np.float64
    flat = np.concatenate([np.concatenate((np.full((int(c), 1), i, np.float64), dev[i, :int(c)]), 1) for i, c in enumerate(gt_counts)])
    flat[:, 1] += 1
    assert np.array_equal(flat, z["ref_gt"][:, :8])
    n_ref = len(z["ref_gt"])
    assert len(z["coco_gt"]) > n_ref and (z["coco_gt"][:, 7] == 1).sum() > (z["ref_gt"][:, 7] == 1).sum()


def test_summary_lines():
    stats = np.array([0.5, 0.25, 0.125, -1, 1, 0.0624, 0.1, 0.2, 0.3, 0.4, 0.5, 0.9996])
    lines = coco_eval.summary_lines(stats)
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.500"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.250"
    assert lines[2] == " Average Precision  (AP) @[ IoU=0.75      | area=   all | maxDets=100 ] = 0.125"
    assert lines[3] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = -1.000"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.100"
    assert lines[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 1.000"
    want = [C.summary_line(ap, thr, area, m, v) for (ap, thr, area, m), v in zip(C.SUMMARY, stats)]
    assert lines == want


def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name in ("cvx_coco_match", "cvx_coco_accumulate", "cvx_coco_summarize"):
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
    assert [len(L.PROTOTYPES[n][1]) for n in ("cvx_coco_match", "cvx_coco_accumulate", "cvx_coco_summarize")] == [22, 10, 5]
    assert "coco_eval.hip" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_evaluate_on_coco_on_the_four_detectors(tmp_path):
    import inspect
    from configs import CenternetConfig, SsdConfig, Yolo7Config, Yolo8DetConfig
    from core.algorithms.centernet import CenterNetA
    from core.algorithms.ssd import Ssd
    from core.algorithms.yolo_v7 import YOLOv7
    from core.algorithms.yolo_v8 import YOLOv8
    for cls, cfg in ((YOLOv8, Yolo8DetConfig), (YOLOv7, Yolo7Config), (Ssd, SsdConfig), (CenterNetA, CenternetConfig)):
        algo = cls(cfg(), "cpu")
        with pytest.raises(CvxError):                                       # no dataset reader: the data source is injected
            algo.evaluate_on_coco(None, str(tmp_path), "val")
        with pytest.raises(ValueError):
            algo.evaluate_on_coco(None, str(tmp_path), "test", dataloader=[])
        assert inspect.signature(algo.evaluate_on_voc).parameters["coco_metric"].default is False


def test_evaluator_arguments():
    with pytest.raises(ValueError):
        coco_eval.CocoEvaluator(20, 20000, 100, "cpu")
    ev = coco_eval.CocoEvaluator(20, 300, 100, "cpu")
    with pytest.raises(CvxError):                                           # no CPU path
        ev.results()
    with pytest.raises(CvxError):
        ev.add_batch(torch.zeros(1, 4, 6), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, 7, dtype=torch.float64), torch.zeros(1, dtype=torch.int32))
