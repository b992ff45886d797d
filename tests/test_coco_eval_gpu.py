"""MI355X: ``cvx_coco_match`` + ``cvx_coco_accumulate`` + ``cvx_coco_summarize`` through ``CocoEvaluator`` against the sequential
restatement of COCOeval (tests/coco_eval_restatement.py) on the fixture (tests/golden/coco_inputs_ref.npz); batch splitting; box-map mode
1 against ``undo_letterbox`` with the truncate / quantize flags; the overflow counters; ``evaluate_on_coco`` of YOLOv8 and CenterNet end
to end against the restatement fed with the same rows pulled to the host; ``evaluate_on_voc(coco_metric=True)``."""
import os

import numpy as np
import pytest
import torch

import coco_eval_restatement as C
from computervision.pytorch_amd import CvxError, coco_eval, det_eval
from core.utils.boxes import undo_letterbox

pytestmark = pytest.mark.gpu
STAT_TOL = 1e-9      # the bound the VOC test gives AP: the means differ in summation order only, < 2^17 terms of at most 1 each


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def on(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def restate(rows, counts, gt, gt_counts, nc, **kw):
    """the restatement's answer for final rows: results and the per-detection records in (image, row) order"""
    dts, gts = C.detections_from_rows(rows, counts, **kw), C.ground_truth_from_arrays(gt, gt_counts)
    out = C.coco_eval(gts, dts, range(len(counts)), nc)
    out["masks"] = C.detection_masks(out["eval_imgs"], dts, nc)
    out["dts"] = dts
    return out


def check_against(ev, want):
    """records, npig, precision and recall exact; the twelve stats to STAT_TOL"""
    res = ev.results()
    score, cls, rank, matched, ignored = ev.records()
    assert cls.tolist() == [d["category"] for d in want["dts"]]
    assert np.array_equal(score, np.array([d["score"] for d in want["dts"]]).astype(np.float32))
    assert np.array_equal(rank, want["masks"][0]) and np.array_equal(matched, want["masks"][1]) and np.array_equal(ignored, want["masks"][2])
    assert np.array_equal(res["npig"], want["npig"])
    assert np.array_equal(res["recall"], want["recall"])
    assert np.array_equal(res["precision"], want["precision"])
    d = np.abs(res["stats"] - want["stats"]).max()
    print(f"stats {res['stats'].tolist()}: max difference {d:.3e}")
    assert d <= STAT_TOL
    assert ev.summary_text().splitlines() == want["lines"]


@pytest.fixture(scope="module")
def fixture(gold):
    z = gold("coco_inputs_ref.npz")
    gts, dts, n = C.fixture_lists(z)
    nc = int(z["num_classes"])
    arrays = C.arrays_from_lists(gts, dts, n)
    assert arrays[0].shape[0] == 40 and 100 < arrays[0].shape[1] <= 128 and arrays[2].shape[1] <= 16 and nc == 6
    return nc, arrays, restate(*arrays, nc)


def feed(dev, nc, arrays, pieces, **kw):
    n, K = arrays[0].shape[:2]
    ev = coco_eval.CocoEvaluator(nc, K, n * K, dev, **kw)
    for idx in np.array_split(np.arange(n), pieces):
        ev.add_batch(*on(dev, *[a[idx] for a in arrays]))
    return ev


def test_fixture_against_the_restatement(dev, fixture):
    nc, arrays, want = fixture
    assert (want["masks"][0] >= 100).sum() >= 10 and (want["stats"] > 0).all()
    check_against(feed(dev, nc, arrays, 1), want)


def test_batch_splitting_is_bit_identical(dev, fixture):
    nc, arrays, want = fixture
    whole = feed(dev, nc, arrays, 1)
    for pieces in (3, 40):
        split = feed(dev, nc, arrays, pieces)
        for x, y in zip(whole.records(), split.records()):
            assert np.array_equal(x, y)
        for k in ("stats", "precision", "recall", "npig"):
            assert np.array_equal(whole.results()[k], split.results()[k]), (pieces, k)
    split.reset()
    split.add_batch(*on(dev, *[a[:3] for a in arrays]))
    check_against(split, restate(*[a[:3] for a in arrays], nc))


@pytest.mark.parametrize("letterbox,truncate,quantize", [(True, False, False), (False, True, True), (True, True, False), (False, False, True)])
def test_box_map_mode_1_and_the_flags(dev, letterbox, truncate, quantize):
    """float boxes in network pixels, four original sizes, 110 rows of class 0 in image 0: mode 1 on the raw rows == mode 0 on
    undo_letterbox's float32 boxes == the restatement on them.  Every ground truth is a detection's own final box (truncated when the
    kernel truncates) moved by a fraction of a pixel, so most IoUs sit between 0.5 and 1 where the ten thresholds cut"""
    nc, B, K, G = 3, 4, 128, 16
    rs = np.random.RandomState(5 + 2 * truncate + quantize)
    image_hw = np.array([[375, 500], [500, 333], [97, 640], [128, 128]], np.int64)
    rows = np.zeros((B, K, 6), np.float32)
    lt = rs.uniform(0, 100, (B, K, 2)).astype(np.float32)
    rows[..., 0:2] = lt
    rows[..., 2:4] = lt + rs.uniform(4, 27, (B, K, 2)).astype(np.float32)
    rows[..., 4] = rs.uniform(0.001, 1, (B, K)).astype(np.float32)
    rows[..., 4][rs.rand(B, K) < 0.2] = np.float32(0.25)                        # equal scores, in and across images
    rows[..., 5] = rs.randint(0, nc, (B, K))
    rows[0, :110, 5] = 0
    counts = np.array([K, K - 3, 40, 17], np.int32)
    final = rows.copy()
    for b in range(B):
        final[b, :, :4] = undo_letterbox(rows[b], (128, 128), image_hw[b], letterbox)[0]
    gt = np.zeros((B, G, 7), np.float64)
    for b in range(B):
        for g in range(G):
            r = rs.randint(0, counts[b])
            x1, y1, x2, y2 = (float(int(v)) if truncate else float(v) for v in final[b, r, :4])
            x, y, w, h = x1 + rs.randint(-8, 9) / 8, y1 + rs.randint(-8, 9) / 8, x2 - x1 + rs.randint(-8, 9) / 8, y2 - y1 + rs.randint(-8, 9) / 8
            gt[b, g] = [final[b, r, 5], x, y, w, h, w * h * (1 if g % 5 else 40), rs.rand() < 0.2]
    gt_counts = np.array([G, G - 1, G, 5], np.int32)
    kw = dict(truncate_boxes=truncate, quantize_scores=quantize)
    box_map = det_eval.letterbox_box_map(torch.from_numpy(image_hw).to(dev), (128, 128), letterbox)
    ev1 = coco_eval.CocoEvaluator(nc, K, B * K, dev, **kw)
    ev1.add_batch(*on(dev, rows, counts, gt, gt_counts), box_map)
    ev0 = coco_eval.CocoEvaluator(nc, K, B * K, dev, **kw)
    ev0.add_batch(*on(dev, final, counts, gt, gt_counts))
    want = restate(final, counts, gt, gt_counts, nc, truncate=truncate, quantize=quantize)
    check_against(ev0, want)
    check_against(ev1, want)
    assert 0.02 < want["stats"][0] < 0.98 and (want["masks"][0] >= 100).any() and want["npig"][:, 1:].sum(0).all()


def test_overflow_counters_raise_at_results(dev, fixture):
    nc, arrays, _ = fixture
    rows, counts, gt, gt_counts = [a[:3].copy() for a in arrays]
    counts[1] = -1                                                              # cvx_nms: more candidates than its sort holds
    ev = coco_eval.CocoEvaluator(nc, rows.shape[1], 3 * rows.shape[1], dev)
    ev.add_batch(*on(dev, rows, counts, gt, gt_counts))
    with pytest.raises(CvxError, match="dropped"):
        ev.results()
    rows, counts, gt, gt_counts = [a[:3].copy() for a in arrays]
    ev = coco_eval.CocoEvaluator(nc, rows.shape[1], int(counts.sum()) - 1, dev)          # no room left for the last image
    ev.add_batch(*on(dev, rows, counts, gt, gt_counts))
    with pytest.raises(CvxError, match="dropped"):
        ev.results()
    rows[0, 0, 5] = nc
    ev = coco_eval.CocoEvaluator(nc, rows.shape[1], 3 * rows.shape[1], dev)
    ev.add_batch(*on(dev, rows, counts, gt, gt_counts))
    with pytest.raises(CvxError, match="class indices"):
        ev.results()


class TinyLoader:
    """two batches of two images in memory: (images, meta) on the device"""

    def __init__(self, images, **meta):
        self.items = [(images[i:i + 2], {k: v[i:i + 2] for k, v in meta.items()}) for i in (0, 2)]

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def coco_ground_truth_near(final_rows, counts, G, seed):
    """ground truths made from every third detection's own box, moved by up to a pixel in eighths; one in four a crowd box"""
    rs = np.random.RandomState(seed)
    B = len(counts)
    gt, gt_counts = np.zeros((B, G, 7), np.float64), np.zeros(B, np.int32)
    for b in range(B):
        for r in range(0, min(int(counts[b]), 3 * G), 3):
            x1, y1, x2, y2 = (float(v) for v in final_rows[b, r, :4])
            x, y, w, h = x1 + rs.randint(-8, 9) / 8, y1 + rs.randint(-8, 9) / 8, x2 - x1 + rs.randint(-8, 9) / 8, y2 - y1 + rs.randint(-8, 9) / 8
            gt[b, gt_counts[b]] = [final_rows[b, r, 5], x, y, w, h, w * h, rs.rand() < 0.25]
            gt_counts[b] += 1
    return gt, gt_counts


def voc_ground_truth_near(final_rows, counts, G, seed):
    rs = np.random.RandomState(seed)
    B = len(counts)
    gt, gt_counts = np.zeros((B, G, 6), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        for r in range(0, min(int(counts[b]), 3 * G), 3):
            box = [int(v) + int(rs.randint(-2, 3)) for v in final_rows[b, r, :4]]
            gt[b, gt_counts[b]] = [int(final_rows[b, r, 5])] + box + [int(rs.rand() < 0.25)]
            gt_counts[b] += 1
    return gt, gt_counts


def check_result(res, want):
    for k in ("npig", "recall", "precision"):
        assert np.array_equal(res[k], want[k]), k
    print(f"stats {res['stats'].tolist()}")
    assert np.abs(res["stats"] - want["stats"]).max() <= STAT_TOL


def test_yolov8_evaluate_on_coco_and_coco_metric_end_to_end(dev, tmp_path):
    """seed-0 YOLOv8-n, nc = 20, 128 x 128, class biases raised by 3 as in the VOC test (16 detections per image on the CPU oracle).
    ``evaluate_on_coco`` against the restatement on the unrounded final boxes; ``evaluate_on_voc(coco_metric=True)`` returns the VOC
    numbers of ``coco_metric=False`` unchanged, beside the COCO metric of the truncated boxes and cut scores"""
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8
    from computervision.pytorch_amd import engine as E
    from oracle import synth
    cfg = Yolo8DetConfig()
    cfg.dataset.num_classes, cfg.arch.input_size = 20, (3, 128, 128)
    algo = YOLOv8(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    raised = [k for k in sd if ".cv3." in k and k.endswith(".2.bias")]
    assert len(raised) == 3
    for k in raised:
        sd[k] += 3.0
    model.load_state_dict(sd)
    images = synth.images(4, 128, 128, seed=1).to(dev)
    image_hw = np.array([[375, 500], [500, 333], [128, 128], [97, 200]], np.int64)
    with torch.no_grad():
        y = torch.cat([model(images[i:i + 2])[0] for i in (0, 2)])
    rows, _, counts = E.nms(y, 0.001, algo.iou_threshold, algo.max_det)
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    print(f"YOLOv8-n detections above 0.001: {counts.tolist()}")
    assert 16 <= int(counts.sum()) <= 256
    final = rows.copy()
    for b in range(4):
        final[b, :, :4] = undo_letterbox(rows[b], (128, 128), image_hw[b], algo.letterbox_image)[0]
    gt_coco, gt_counts = coco_ground_truth_near(final, counts, 6, seed=2)
    gt_voc, gt_counts_voc = voc_ground_truth_near(final, counts, 6, seed=2)
    assert np.array_equal(gt_counts, gt_counts_voc)
    t_hw, t_coco, t_voc, t_counts = on(dev, image_hw, gt_coco, gt_voc, gt_counts)

    res = algo.evaluate_on_coco(model, str(tmp_path / "coco"), "val", dataloader=TinyLoader(images, image_hw=t_hw, gt_coco=t_coco, gt_counts=t_counts))
    want = restate(final, counts, gt_coco, gt_counts, 20)
    check_result(res, want)
    assert res["stats"][0] > 0 and res["n_records"] == int(counts.sum())
    assert open(tmp_path / "coco" / "coco_results.txt").read().splitlines() == want["lines"]

    loader = TinyLoader(images, image_hw=t_hw, gt=t_voc, gt_counts=t_counts)
    plain = algo.evaluate_on_voc(model, str(tmp_path / "a"), "val", dataloader=loader)
    both = algo.evaluate_on_voc(model, str(tmp_path / "b"), "val", dataloader=loader, coco_metric=True)
    assert "coco" not in plain and sorted(both) == sorted(list(plain) + ["coco"])
    for k, v in plain.items():
        assert np.array_equal(both[k], v), k
    assert open(tmp_path / "a" / "results" / "results.txt").read() == open(tmp_path / "b" / "results" / "results.txt").read()
    assert not os.path.exists(tmp_path / "a" / "coco_results.txt")
    conv = coco_eval.voc_gt_to_coco(t_voc).cpu().numpy()
    want = restate(final, counts, conv, gt_counts, 20, truncate=True, quantize=True)
    check_result(both["coco"], want)
    assert open(tmp_path / "b" / "coco_results.txt").read().splitlines() == want["lines"]


def test_centernet_evaluate_on_coco_end_to_end(dev, tmp_path):
    """seed-0 CenterNet DLA-34 at 128 x 128, nc = 20, the size head's bias raised by 6 as in the VOC test (about 70 detections per image)"""
    from configs import CenternetConfig
    from core.algorithms.centernet import CenterNetA
    from oracle import synth
    cfg = CenternetConfig()
    cfg.dataset.num_classes, cfg.arch.input_size = 20, (3, 128, 128)
    algo = CenterNetA(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["backbone.reg.2.bias"] += 6.0
    model.load_state_dict(sd)
    images = synth.images(4, 128, 128, seed=1).to(dev)
    image_hw = np.array([[375, 500], [500, 333], [128, 128], [97, 200]], np.int64)
    final, counts = [], []
    with torch.no_grad():
        for b in range(4):                                                   # the wrapper's own per-image host tail
            boxes, scores, classes = algo._finish(algo.decode_raw(model.forward_raw(images[b:b + 1]), 32, 32, 0.001), 0, *image_hw[b].tolist())
            rows = np.zeros((algo.K, 6), np.float32)
            rows[:len(boxes)] = np.concatenate((boxes, scores[:, None], classes[:, None].astype(np.float32)), 1)
            final.append(rows)
            counts.append(len(boxes))
    final, counts = np.stack(final), np.array(counts, np.int32)
    print(f"CenterNet detections above 0.001: {counts.tolist()}")
    assert 100 <= int(counts.sum()) < 4 * algo.K
    gt_coco, gt_counts = coco_ground_truth_near(final, counts, 6, seed=3)
    t_hw, t_coco, t_counts = on(dev, image_hw, gt_coco, gt_counts)
    res = algo.evaluate_on_coco(model, str(tmp_path), "val", dataloader=TinyLoader(images, image_hw=t_hw, gt_coco=t_coco, gt_counts=t_counts))
    check_result(res, restate(final, counts, gt_coco, gt_counts, 20))
    assert res["stats"][0] > 0
