"""One batch of 260 images through the three accumulators of the detection metrics -- ``DetectionEvaluator``, ``CocoEvaluator`` and
``DetectionDiagnostics`` -- against their restatements.  The record base of an image is a workgroup sum over the images before it
(csrc/det_common.h: det_record_base) whose threads stride by 256: past 256 images the second stride runs, which no other test
reaches.  And the same case split at image 130: the cursor handed from one batch to the next, at a boundary that is not image 0.
The assertions are the three files' own ``check_against`` / ``check_results``."""
import numpy as np
import pytest
import torch

import det_diag_restatement as D
import det_eval_restatement as R
import test_coco_eval_gpu as TC
import test_det_diag_gpu as TD
import test_det_eval_gpu as TV
from computervision.pytorch_amd import coco_eval, det_diag, det_eval

pytestmark = pytest.mark.gpu
B, NC, K, G = 260, 4, 4, 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def case():
    arrays = D.seeded_case(7, B, NC, K, G)
    assert arrays[0].shape == (B, K, 6) and arrays[2].shape == (B, G, 6)
    return arrays


@pytest.fixture(scope="module")
def coco_gt(case):
    return coco_eval.voc_gt_to_coco(torch.from_numpy(case[2])).numpy()


def accumulators(dev):
    return (det_eval.DetectionEvaluator(NC, K, B * K, dev),
            coco_eval.CocoEvaluator(NC, K, B * K, dev, truncate_boxes=True, quantize_scores=True),
            det_diag.DetectionDiagnostics(NC, K, dev, det_diag.DetDiagnostics(points=101, smooth_window=11)))


def feed(dev, case, coco_gt, pieces):
    voc, coco, diag = accumulators(dev)
    for idx in pieces:
        rows, counts, gt, gt_counts = TV.on(dev, *[a[idx] for a in case])
        voc.add_batch(rows, counts, gt, gt_counts)
        coco.add_batch(rows, counts, TV.on(dev, coco_gt[idx])[0], gt_counts)
        diag.add_batch(rows, counts, gt, gt_counts)
    return voc, coco, diag


def test_one_batch_of_260_images_through_the_three_accumulators(dev, case, coco_gt):
    rows, counts, gt, gt_counts = case
    voc, coco, diag = feed(dev, case, coco_gt, [np.arange(B)])

    want = R.get_map(R.detections_from_rows(rows, counts), R.ground_truth_from_arrays(gt, gt_counts), NC)
    flags = np.array(want["flags"])
    print(f"VOC restatement: {(flags == 1).sum()} TP, {(flags == 0).sum()} FP, {(flags == 2).sum()} neither, mAP {want['res']['mAP']!r}")
    assert ((flags == 1).sum(), (flags == 0).sum(), (flags == 2).sum()) == (77, 406, 28) and abs(want["res"]["mAP"] - 0.116) < 5e-4
    TV.check_against(voc, want, NC)
    score, cls, _ = voc.records()
    flat = [d for per in R.detections_from_rows(rows, counts) for d in per]
    assert cls.tolist() == [d[0] for d in flat] and np.array_equal(score, np.array([d[1] for d in flat]).astype(np.float32))

    cwant = TC.restate(rows, counts, coco_gt, gt_counts, NC, truncate=True, quantize=True)
    assert (cwant["stats"] > 0).sum() == 8
    TC.check_against(coco, cwant)

    spec = diag.spec
    dwant = TD.restate(NC, rows, counts, gt, gt_counts, spec)
    assert (np.diag(dwant["confusion"])[:NC] >= 16).all()
    TD.check_results(diag.results(voc), dwant)


def test_split_at_image_130_equals_the_one_batch(dev, case, coco_gt):
    whole = feed(dev, case, coco_gt, [np.arange(B)])
    split = feed(dev, case, coco_gt, [np.arange(130), np.arange(130, B)])
    for one, two in zip(whole[:2], split[:2]):
        for x, y in zip(one.records(), two.records()):
            assert len(x) == int(case[1].sum()) and np.array_equal(x, y)
    rw, rs = whole[0].results(), split[0].results()
    for k in ("ap", "precision", "recall", "f1", "tp", "n_det", "n_gt"):
        assert np.array_equal(rw[k], rs[k]), k                              # bit for bit
    assert rw["mAP"] == rs["mAP"]
    for (p1, r1), (p2, r2) in zip(whole[0].curves(), split[0].curves()):
        assert np.array_equal(p1, p2) and np.array_equal(r1, r2)
    for k in ("stats", "precision", "recall", "npig"):
        assert np.array_equal(whole[1].results()[k], split[1].results()[k]), k
