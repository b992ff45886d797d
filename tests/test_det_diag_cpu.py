"""CPU: the detector diagnostics' host side -- the restatement (tests/det_diag_restatement.py) against what the reference's
``log_average_miss_rate`` made of the fixtures (tests/golden/det_lamr_ref.npz, written by tools/make_lamr_fixture.py), the confusion rule
against a matrix derived by hand, its coverage of the mAP fixture and its invariants, the curves against the evaluator restatement's
values at 0.5, the smoothing by hand, the report text, the new symbols and the surface that needs no GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import det_diag_restatement as D
import det_eval_restatement as R
from computervision.pytorch_amd import LIB_PATH, CvxError, det_diag, det_eval
from computervision.pytorch_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture(gold):
    z = gold("det_map_ref.npz")
    dets, gts, _ = R.fixture_inputs(z)
    nc = len(z["names"])
    return z, dets, gts, nc, R.get_map(dets, gts, nc)


def test_lamr_equals_the_reference_exactly(fixture, gold):
    """the same fp64 operations in the same order: equality, no tolerance"""
    z, dets, gts, nc, out = fixture
    ref = gold("det_lamr_ref.npz")
    flags = D.flags_per_class(dets, out["flags"], nc)
    images = D.confusion(dets, gts, nc)["images_per_class"]
    assert np.array_equal(images, ref["images_per_class"])
    got = np.full(nc, np.nan)
    mr9 = np.ones((nc, 9))
    for c in range(nc):
        rec = out["curves"][c][1]
        mr9[c] = D.miss_rates(rec, D.fp_cumsum(flags[c]), images[c])
        got[c] = D.lamr(mr9[c], len(rec), images[c])
        print(f"class {c}: LAMR {got[c]!r} against {float(ref['lamr'][c])!r}")
    gt_classes = z["gt_classes"].tolist()
    assert len(gt_classes) == 5
    for c in gt_classes:
        assert got[c] == ref["lamr"][c], c
    assert got[0] == 0.922941540779515 and got[3] == 0.7903844105080718
    person = z["names"].tolist().index("person")
    assert out["res"]["n_gt"][person] > 0 and out["res"]["n_det"][person] == 0 and got[person] == 0.0 == ref["lamr"][person]
    assert np.isnan(got[5]) and np.isnan(ref["lamr"][5])                  # "boat": detections, no image holds one
    # the package's host end on the same nine values
    assert np.array_equal(det_diag.lamr_from_mr9(mr9, out["res"]["n_det"], images), got, equal_nan=True)
    assert np.array_equal(det_diag.REF_POINTS, D.REF_POINTS)
    off = ref["edge_off"]
    for i, name in enumerate(ref["edge_names"].tolist()):
        rec, fp, n = ref["edge_rec"][off[i]:off[i + 1]], ref["edge_fp_cum"][off[i]:off[i + 1]], int(ref["edge_n_images"][i])
        mine = D.lamr(D.miss_rates(rec, fp, n), len(rec), n)
        print(f"{name}: LAMR {mine!r} against {float(ref['edge_lamr'][i])!r}")
        assert mine == ref["edge_lamr"][i], name
    # the hundred-image case sits on both ends of the reference points: 1 / 100 qualifies for the first, 100 / 100 for the last
    i = ref["edge_names"].tolist().index("hundred_images")
    fp = ref["edge_fp_cum"][off[i]:off[i + 1]]
    assert 1 in fp and 100 in fp and 101 in fp
    assert np.array_equal(D.miss_rates(ref["edge_rec"][off[i]:off[i + 1]], fp, 100)[[0, 8]], [1 - 0.25, 1 - 0.5])


def test_confusion_rule_on_the_planted_image():
    (rows, counts, gt, gt_counts), want, images = D.planted_case()
    out = D.confusion(R.detections_from_rows(rows, counts), R.ground_truth_from_arrays(gt, gt_counts), 3, 0.25, 0.45)
    assert np.array_equal(out["confusion"], want) and np.array_equal(out["images_per_class"], images)
    assert D.overlap((14, 110, 33, 129), (10, 110, 29, 129)) == 320 / 480 and D.overlap((14, 110, 33, 129), (20, 110, 39, 129)) == 280 / 520
    assert 280 / 520 > 0.45                                               # B is a candidate of r7 and still missed
    assert out["confusion"][1, 1] == 1 and out["confusion"][3, 1] == 1 and out["confusion"][1, 3] == 2    # greedy one-to-one: 2, 0, 1
    assert D.overlap((12, 10, 21, 19), (10, 10, 19, 19)) == D.overlap((12, 10, 21, 19), (14, 10, 23, 19)) == 80 / 120
    assert (out["gt_tie"], out["row_tie"], out["difficult_choice"], out["below_conf"], out["off_diagonal"], out["lost"]) == (1, 1, 1, 1, 1, 2)


def test_the_map_fixture_covers_the_rule(fixture):
    z, dets, gts, nc, out = fixture
    conf = D.confusion(dets, gts, nc, 0.25, 0.45)
    m = conf["confusion"]
    print({k: v for k, v in conf.items() if k not in ("confusion", "images_per_class")})
    assert conf["off_diagonal"] == 14 and conf["difficult_choice"] == 20 and conf["below_conf"] == 80    # confirmed by this restatement
    assert conf["lost"] > 0 and conf["gt_tie"] > 0 and conf["bad_class"] == 0
    assert m[:nc, :nc].sum() - np.trace(m[:nc, :nc]) == 14
    n_gt, n_det = out["res"]["n_gt"], out["res"]["n_det"]
    for c in range(nc):
        assert (m[nc, c] > 0) == (n_gt[c] > 0), c                         # every class with a ground truth has missed ones
        assert (m[c, nc] > 0) == (n_det[c] > 0), c                        # every detected class has background false positives
    assert np.array_equal(m[:, :nc].sum(0), n_gt)


@pytest.mark.parametrize("seed", range(8))
def test_confusion_invariants(seed):
    nc, conf_thr = 4, 0.25
    rows, counts, gt, gt_counts = R.random_case(seed) if seed % 2 else D.seeded_case(seed, 3, nc, 16, 6)
    dets, gts = R.detections_from_rows(rows, counts), R.ground_truth_from_arrays(gt, gt_counts)
    out = D.confusion(dets, gts, nc, conf_thr, 0.45)
    m = out["confusion"]
    n_gt = R.get_map(dets, gts, nc)["res"]["n_gt"]
    assert np.array_equal(m[:, :nc].sum(0), n_gt) and m[nc, nc] == 0
    reach = np.zeros(nc, np.int64)
    for per in dets:
        for d in per:
            reach[d[0]] += d[1] >= conf_thr
    assert reach.sum() - m[:nc].sum() == out["difficult_choice"]
    dropped = reach - m[:nc].sum(1)
    assert (dropped >= 0).all() and dropped.sum() == out["difficult_choice"]
    assert sum(len(per) for per in dets) - reach.sum() == out["below_conf"]


def test_curves_at_one_half_are_the_evaluators_values(fixture):
    z, dets, gts, nc, out = fixture
    flags = D.flags_per_class(dets, out["flags"], nc)
    scores = D.scores_per_class(dets, nc)
    records = [(scores[c], out["curves"][c][0], out["curves"][c][1], flags[c]) for c in range(nc)]
    cur = D.conf_curves(records, out["res"]["n_gt"], 1001, 101)
    assert cur["conf_grid"][500] == 0.5 and cur["conf_grid"][0] == 0.0 and cur["conf_grid"][1000] == 1.0
    reaching = 0
    for c in range(nc):
        got = (cur["precision"][c, 500], cur["recall"][c, 500], cur["f1"][c, 500])
        if len(scores[c]) and scores[c][0] >= 0.5:
            reaching += 1
            assert got == (out["res"]["precision"][c], out["res"]["recall"][c], out["res"]["f1"][c]), c
        else:
            assert got == (1.0, 0.0, 0.0), c
    assert 0 < reaching < nc
    # a step function that never rises in recall as the threshold grows, and ends on (1, 0, 0) above the largest score
    assert (np.diff(cur["recall"], axis=1) <= 0).all()
    assert 0 <= cur["best_index"] <= 1000 and cur["mean_f1_smooth"][cur["best_index"]] == cur["mean_f1_smooth"].max()


def test_smoothing_by_hand():
    y = np.array([0.0, 0.25, 1.0, 0.5, 0.75])
    assert np.array_equal(D.smooth(y, 1), y)
    # a window of 9 over 4 points: out[i] = (y[0] * (5 - i) + y[1] + y[2] + y[3] * (2 + i)) / 9 with y = 0, 1, 2, 3
    assert np.array_equal(D.smooth(np.array([0.0, 1.0, 2.0, 3.0]), 9), np.array([9.0, 12.0, 15.0, 18.0]) / 9.0)
    assert np.array_equal(D.smooth(np.array([1.0, 0.0, 0.0]), 3), np.array([2.0, 1.0, 0.0]) / 3.0)
    assert D.first_max(np.array([0.0, 1.0, 1.0, 0.0])) == 1 and D.first_max(np.array([2.0, 2.0])) == 0
    assert np.array_equal(D.smooth(np.array([0.0, 1.0, 0.0, 1.0, 0.0]), 3), np.array([1.0, 1.0, 2.0, 1.0, 1.0]) / 3.0)
    assert D.first_max(D.smooth(np.array([0.0, 1.0, 0.0, 1.0, 0.0]), 3)) == 2
    assert D.first_max(D.smooth(np.array([0.0, 1.0, 0.0, 0.0, 1.0, 0.0]), 3)) == 0      # every smoothed value is 1 / 3: the first wins


def small_result():
    """two classes, three grid points, written by hand"""
    return dict(confusion=np.array([[3, 1, 2], [0, 4, 0], [5, 6, 0]], np.int64), images_per_class=np.array([7, 9], np.int64), conf=0.25, iou=0.45,
                conf_grid=np.array([0.0, 0.5, 1.0]), precision=np.array([[0.5, 0.75, 1.0], [0.25, 1.0, 1.0]]),
                recall=np.array([[1.0, 0.5, 0.0], [0.5, 0.25, 0.0]]), f1=np.array([[0.625, 0.6, 0.0], [0.125, 0.4, 0.0]]),
                mean_f1=np.array([0.375, 0.5, 0.0]), mean_f1_smooth=np.array([0.375, 0.5, 0.0]), best_index=1, best_conf=0.5,
                best_index_per_class=np.array([0, 1], np.int64), best_conf_per_class=np.array([0.0, 0.5]),
                precision_at_best=np.array([0.75, 1.0]), recall_at_best=np.array([0.5, 0.25]), f1_at_best=np.array([0.6, 0.4]),
                mean_precision_at_best=0.875, mean_recall_at_best=0.375, mean_f1_at_best=0.5, lamr=np.array([0.5, 0.0]), mean_lamr=0.25,
                n_gt=np.array([8, 10], np.int64))


def test_report_text_by_hand():
    res, names = small_result(), ["dog", "cat, big"]
    assert det_diag.format_confusion_csv(res["confusion"], names) == ('pred\\true,dog,"cat, big",background\n'
                                                                      'dog,3,1,2\n'
                                                                      '"cat, big",0,4,0\n'
                                                                      'background,5,6,0\n')
    assert det_diag.format_curves_csv(res, names) == ('conf,mean_f1,mean_f1_smooth,dog_p,dog_r,dog_f1,"cat, big_p","cat, big_r","cat, big_f1"\n'
                                                      '0.0,0.375,0.375,0.5,1.0,0.625,0.25,0.5,0.125\n'
                                                      '0.5,0.5,0.5,0.75,0.5,0.6,1.0,0.25,0.4\n'
                                                      '1.0,0.0,0.0,1.0,0.0,0.0,1.0,0.0,0.0\n')
    assert det_diag.format_diagnostics(res, names) == (
        "# detector diagnostics\n"
        "recommended conf_threshold = 0.5000 (first maximum of the mean F1 over 2 classes, smoothed; mean F1 0.5000, smoothed 0.5000)\n"
        "at it: mean precision 0.8750, mean recall 0.3750, mean F1 0.5000; mean LAMR 0.2500\n"
        "\n# per class: own best conf | precision recall F1 at the recommended conf | LAMR | images\n"
        "cat, big: 0.5000 | 1.0000 0.2500 0.4000 | 0.0000 | 9\n"
        "dog: 0.0000 | 0.7500 0.5000 0.6000 | 0.5000 | 7\n"
        "\n# confusion matrix at conf 0.2500, IoU 0.45: largest off-diagonal cells (predicted -> true: count)\n"
        "background -> cat, big: 6\n"
        "background -> dog: 5\n"
        "dog -> background: 2\n"
        "dog -> cat, big: 1\n")
    many = dict(res, confusion=np.arange(144).reshape(12, 12), n_gt=np.zeros(11, np.int64), f1=np.zeros((11, 3)))
    tail = det_diag.format_diagnostics(many, [str(i) for i in range(11)]).split("count)\n")[1].splitlines()
    assert len(tail) == 10 and tail[0] == "background -> 10: 142" and tail[1] == "background -> 9: 141"


def test_unpack_curves_layout():
    nc, P = 2, 3
    words = np.arange(det_diag.curve_words(nc, P), dtype=np.float64)
    assert words.size == 3 * nc * P + 2 * P + 10 * nc + 1 == 45
    raw = words.view(np.int64).copy()
    raw[-3:] = [2, 0, 1]
    out = det_diag.unpack_curves(raw, nc, P)
    assert out["precision"].tolist() == [[0, 1, 2], [3, 4, 5]] and out["recall"][1].tolist() == [9, 10, 11] and out["f1"][0].tolist() == [12, 13, 14]
    assert out["mean_f1"].tolist() == [18, 19, 20] and out["mean_f1_smooth"].tolist() == [21, 22, 23]
    assert out["mr9"].shape == (2, 9) and out["mr9"][0, 0] == 24 and out["mr9"][1, 8] == 41
    assert out["best_index_per_class"].tolist() == [2, 0] and out["best_index"] == 1


def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name in ("cvx_det_confusion", "cvx_det_conf_curves"):
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
    assert len(L.PROTOTYPES["cvx_det_confusion"][1]) == 17 and len(L.PROTOTYPES["cvx_det_conf_curves"][1]) == 15
    assert "det_diag.hip" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "#define CVX_ABI_VERSION 6" in header                           # additive


def test_spec_and_accumulator_arguments():
    spec = det_diag.DetDiagnostics()
    assert (spec.conf, spec.iou, spec.points, spec.smooth_window) == (0.25, 0.45, 1001, 101)
    for bad in (dict(conf=-0.1), dict(conf=1.5), dict(conf="0.3"), dict(iou=1.0), dict(iou=-1), dict(points=1), dict(points=4097), dict(points=10.0),
                dict(smooth_window=0), dict(smooth_window=100), dict(smooth_window=3.0), dict(smooth_window=65537), dict(conf=True)):
        with pytest.raises(ValueError):
            det_diag.DetDiagnostics(**bad)
    with pytest.raises(ValueError):
        det_diag.DetectionDiagnostics(20, 20000, "cpu")
    with pytest.raises(ValueError):
        det_diag.DetectionDiagnostics(0, 300, "cpu")
    with pytest.raises(ValueError):
        det_diag.DetectionDiagnostics(20, 300, "cpu", spec=(0.25, 0.45))
    import torch
    acc = det_diag.DetectionDiagnostics(20, 300, "cpu")
    rows, counts = torch.zeros(1, 4, 6), torch.zeros(1, dtype=torch.int32)
    gt, gt_counts = torch.zeros(1, 2, 6, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(CvxError):                                           # no CPU path
        acc.add_batch(rows, counts, gt, gt_counts)
    with pytest.raises(CvxError):
        acc.confusion()
    with pytest.raises(CvxError):
        acc.results(det_eval.DetectionEvaluator(20, 300, 100, "cpu"))
    with pytest.raises(CvxError):
        acc.write_report("unused", [str(c) for c in range(20)])
    acc.reset()


def test_evaluate_on_voc_takes_diagnostics_on_the_four_detectors_and_the_ensemble(tmp_path):
    from computervision.pytorch_amd import box_fusion
    from configs import CenternetConfig, SsdConfig, Yolo7Config, Yolo8DetConfig
    from core.algorithms.centernet import CenterNetA
    from core.algorithms.ssd import Ssd
    from core.algorithms.yolo_v7 import YOLOv7
    from core.algorithms.yolo_v8 import YOLOv8
    assert inspect.signature(det_eval.evaluate_detector).parameters["diagnostics"].default is None
    assert inspect.signature(box_fusion.DetEnsemble.evaluate_on_voc).parameters["diagnostics"].default is None

    class Model:
        def eval(self):
            return self

    for cls, cfg in ((YOLOv8, Yolo8DetConfig), (YOLOv7, Yolo7Config), (Ssd, SsdConfig), (CenterNetA, CenternetConfig)):
        assert inspect.signature(cls.evaluate_on_voc).parameters["diagnostics"].default is None
        algo = cls(cfg(), "cpu")
        with pytest.raises(CvxError, match="yielded no batch"):             # the keyword is taken; the empty loader is what stops it
            algo.evaluate_on_voc(Model(), str(tmp_path), "val", dataloader=[], diagnostics=det_diag.DetDiagnostics(conf=0.3))
        with pytest.raises(ValueError, match="DetDiagnostics"):
            algo.evaluate_on_voc(Model(), str(tmp_path), "val", dataloader=[], diagnostics=0.3)
    assert not os.path.exists(os.path.join(tmp_path, "results"))
