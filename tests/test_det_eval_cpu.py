"""CPU: the VOC mAP evaluation's host side -- the sequential restatement (tests/det_eval_restatement.py) against what the reference's
``get_map`` made of the fixture (tests/golden/det_map_ref.npz, written by tools/make_map_fixture.py), the report text, the score
quantisation rule against ``str(np.float32(x))[:6]``, the new symbols and the algorithm surface that needs no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import det_eval_restatement as R
from computervision.pytorch_amd import LIB_PATH, CvxError, det_eval
from computervision.pytorch_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture(gold):
    z = gold("det_map_ref.npz")
    dets, gts, _ = R.fixture_inputs(z)
    return z, R.get_map(dets, gts, len(z["names"]))


def test_restatement_equals_the_reference_on_the_fixture(fixture):
    """curves bit for bit (the same fp64 divisions), tp_cum recovered from rec * n_gt exactly; AP and mAP to 1e-9: the two sums may differ
    in order only, n < 2^20 terms of at most 1 each, error <= n * 2^-53 < 1.2e-10"""
    z, out = fixture
    res, off = out["res"], z["curve_off"]
    gt_classes = z["gt_classes"].tolist()
    assert gt_classes == [c for c in range(len(z["names"])) if res["n_gt"][c] > 0] and res["n_classes"] == len(gt_classes)
    for c in gt_classes:
        prec, rec = out["curves"][c]
        assert np.array_equal(rec, z["rec"][off[c]:off[c + 1]]) and np.array_equal(prec, z["prec"][off[c]:off[c + 1]]), c
        tp_cum = np.rint(z["rec"][off[c]:off[c + 1]] * res["n_gt"][c])
        assert np.array_equal(tp_cum / res["n_gt"][c], rec)                 # the recovery is exact
        assert (int(tp_cum[-1]) if len(tp_cum) else 0) == res["tp"][c] and len(tp_cum) == res["n_det"][c]
        print(f"class {c}: AP {res['ap'][c]!r} against {z['ap'][c]!r}")
        assert abs(res["ap"][c] - z["ap"][c]) <= 1e-9
    print(f"mAP {res['mAP']!r} against {float(z['mAP'])!r}")
    assert abs(res["mAP"] - float(z["mAP"])) <= 1e-9
    assert 0.05 < res["mAP"] < 0.95


def test_report_text_matches_the_reference(fixture):
    z, out = fixture
    assert det_eval.format_report(out["res"], out["curves"], z["names"].tolist()) == str(z["results_txt"])


def test_score_quantisation_rule():
    """200 000 seeded float32 values in [1e-3, 1), a third of them within 2 ulp of a 4-decimal number (where the rule's two branches
    meet), and every k / 1e4 itself: the rule gives float(str(np.float32(x))[:6])"""
    rs = np.random.RandomState(0)
    x = rs.uniform(1e-3, 1.0, 200000).astype(np.float32)
    grid = (rs.randint(10, 10000, 70000) / 1e4).astype(np.float32)
    near = grid.copy()
    for _ in range(2):
        near = np.nextafter(near, np.where(rs.rand(near.size) < 0.5, np.float32(0), np.float32(2)).astype(np.float32))
    every = (np.arange(10, 10000) / 1e4).astype(np.float32)
    x = np.concatenate((x, grid, near, every, np.array([1e-3, 1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(0))], np.float32)))
    x = x[(x >= np.float32(1e-3)) & (x <= 1)]
    assert x.size >= 100000
    texts = [str(v)[:6] for v in x]
    assert not any("e" in t for t in texts)
    want = np.array([float(t) for t in texts])
    got = det_eval.quantize_scores(x)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(np.rint(got.astype(np.float64) * 1e4) / 1e4, want)       # the fp64 value the threshold test of cvx_det_ap uses
    assert (got != x).mean() > 0.5 and (got == x).sum() >= every.size                # both branches taken


def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name in ("cvx_det_match", "cvx_det_ap"):
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
    assert len(L.PROTOTYPES["cvx_det_match"][1]) == 19 and len(L.PROTOTYPES["cvx_det_ap"][1]) == 11
    assert "det_eval.hip" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_evaluate_on_voc_on_the_four_detectors(tmp_path):
    from configs import CenternetConfig, SsdConfig, Yolo7Config, Yolo8DetConfig
    from core.algorithms.centernet import CenterNetA
    from core.algorithms.ssd import Ssd
    from core.algorithms.yolo_v7 import YOLOv7
    from core.algorithms.yolo_v8 import YOLOv8
    for cls, cfg in ((YOLOv8, Yolo8DetConfig), (YOLOv7, Yolo7Config), (Ssd, SsdConfig), (CenterNetA, CenternetConfig)):
        algo = cls(cfg(), "cpu")
        with pytest.raises(CvxError):                                       # no dataset reader: the data source is injected
            algo.evaluate_on_voc(None, str(tmp_path), "val")
        with pytest.raises(ValueError):
            algo.evaluate_on_voc(None, str(tmp_path), "train", dataloader=[])


def test_evaluator_arguments():
    with pytest.raises(ValueError):
        det_eval.DetectionEvaluator(20, 20000, 100, "cpu")
    ev = det_eval.DetectionEvaluator(20, 300, 100, "cpu")
    with pytest.raises(CvxError):                                           # no CPU path
        ev.results()
