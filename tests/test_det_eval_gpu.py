"""MI355X: ``cvx_det_match`` + ``cvx_det_ap`` through ``DetectionEvaluator`` against the reference's ``get_map`` on the fixture
(tests/golden/det_map_ref.npz) and against the sequential restatement (tests/det_eval_restatement.py) on seeded random cases; batch
splitting; box-map mode 1 against ``undo_letterbox``; the device restatements of the inverse letterbox maps; ``evaluate_on_voc`` of YOLOv8
and CenterNet end to end against the restatement fed with the same rows pulled to the host."""
import os

import numpy as np
import pytest
import torch

import det_eval_restatement as R
from computervision.pytorch_amd import CvxError, det_eval
from core.utils.boxes import undo_letterbox

pytestmark = pytest.mark.gpu
AP_TOL = 1e-9        # the two sums differ in order only: n < 2^20 terms of at most 1 each, error <= n * 2^-53 < 1.2e-10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def on(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def evaluate(dev, nc, rows, counts, gt, gt_counts, box_map=None, capacity=None, **kw):
    ev = det_eval.DetectionEvaluator(nc, rows.shape[1], capacity or rows.shape[0] * rows.shape[1], dev, **kw)
    ev.add_batch(*on(dev, rows, counts, gt, gt_counts), None if box_map is None else on(dev, box_map)[0])
    return ev


def check_against(ev, want, nc):
    """flags, counts and curves exact; AP, mAP and the thresholded values to AP_TOL"""
    res, wres = ev.results(), want["res"]
    _, _, flags = ev.records()
    assert flags.tolist() == want["flags"]
    for k in ("tp", "n_det", "n_gt"):
        assert np.array_equal(res[k], wres[k]), k
    assert res["n_classes"] == wres["n_classes"]
    for c, (prec, rec) in enumerate(ev.curves()):
        assert np.array_equal(prec, want["curves"][c][0]) and np.array_equal(rec, want["curves"][c][1]), c
    for k in ("ap", "precision", "recall", "f1"):
        d = np.abs(res[k] - wres[k]).max()
        print(f"{k}: max difference {d:.3e}")
        assert d <= AP_TOL, (k, res[k], wres[k])
    print(f"mAP {res['mAP']!r} against {wres['mAP']!r}")
    assert abs(res["mAP"] - wres["mAP"]) <= AP_TOL


def test_fixture_of_the_reference(dev, gold, tmp_path):
    z = gold("det_map_ref.npz")
    names = z["names"].tolist()
    dets, gts, arrays = R.fixture_inputs(z)
    ev = evaluate(dev, len(names), *arrays)
    check_against(ev, R.get_map(dets, gts, len(names)), len(names))
    res, off = ev.results(), z["curve_off"]
    for c in z["gt_classes"].tolist():                                     # the reference's own captures
        prec, rec = ev.curves()[c]
        assert np.array_equal(rec, z["rec"][off[c]:off[c + 1]]) and np.array_equal(prec, z["prec"][off[c]:off[c + 1]])
        assert abs(res["ap"][c] - z["ap"][c]) <= AP_TOL
    assert abs(res["mAP"] - float(z["mAP"])) <= AP_TOL
    text = ev.write_report(str(tmp_path / "results" / "results.txt"), names)
    assert text == str(z["results_txt"]) == open(tmp_path / "results" / "results.txt").read()


@pytest.mark.parametrize("seed", range(20))
def test_random_cases_against_the_restatement(dev, seed):
    nc = 4
    rows, counts, gt, gt_counts = R.random_case(seed)
    if seed == 19:                       # the row block cvx_nms can return at most: the kernel's large-LDS path
        rows = np.concatenate((rows, np.zeros((3, 16384 - 16, 6), np.float32)), 1)
    want = R.get_map(R.detections_from_rows(rows, counts), R.ground_truth_from_arrays(gt, gt_counts), nc)
    ev = evaluate(dev, nc, rows, counts, gt, gt_counts, capacity=48)
    check_against(ev, want, nc)
    score, cls, _ = ev.records()
    flat = [d for per in R.detections_from_rows(rows, counts) for d in per]
    assert cls.tolist() == [d[0] for d in flat] and np.array_equal(score, np.array([d[1] for d in flat]).astype(np.float32))


def test_empty_image_and_overflow(dev):
    nc = 4
    rows, counts, gt, gt_counts = R.random_case(3, B=1)
    counts[:] = 0
    ev = evaluate(dev, nc, rows, counts, gt, gt_counts)
    check_against(ev, R.get_map([[]], R.ground_truth_from_arrays(gt, gt_counts), nc), nc)
    assert ev.results()["n_det"].sum() == 0 and ev.results()["mAP"] == 0.0
    rows, counts, gt, gt_counts = R.random_case(4)
    counts[1] = -1                                                          # cvx_nms: more candidates than its sort holds
    with pytest.raises(CvxError, match="dropped"):
        evaluate(dev, nc, rows, counts, gt, gt_counts).results()
    rows, counts, gt, gt_counts = R.random_case(4)
    counts[:] = 16
    with pytest.raises(CvxError, match="dropped"):                          # no room left
        evaluate(dev, nc, rows, counts, gt, gt_counts, capacity=40).results()
    rows[0, 0, 4] = 5e-5
    with pytest.raises(CvxError, match="below 1e-4"):
        evaluate(dev, nc, rows, counts, gt, gt_counts).results()


def test_two_batches_equal_one(dev):
    nc = 4
    a, b = R.random_case(31), R.random_case(32)
    whole = evaluate(dev, nc, *[np.concatenate((x, y)) for x, y in zip(a, b)], capacity=96)
    split = det_eval.DetectionEvaluator(nc, 16, 96, dev)
    split.add_batch(*on(dev, *a))
    split.add_batch(*on(dev, *b))
    rw, rs = whole.results(), split.results()
    for x, y in zip(whole.records(), split.records()):
        assert np.array_equal(x, y)
    for k in ("ap", "precision", "recall", "f1", "tp", "n_det", "n_gt"):
        assert np.array_equal(rw[k], rs[k]), k                              # bit for bit
    assert rw["mAP"] == rs["mAP"] and rw["n_det"].sum() > 20
    for (p1, r1), (p2, r2) in zip(whole.curves(), split.curves()):
        assert np.array_equal(p1, p2) and np.array_equal(r1, r2)
    split.reset()
    split.add_batch(*on(dev, *a))
    check_against(split, R.get_map(R.detections_from_rows(a[0], a[1]), R.ground_truth_from_arrays(a[2], a[3]), nc), nc)


@pytest.mark.parametrize("letterbox", [True, False])
def test_box_map_mode_1_is_undo_letterbox(dev, letterbox):
    """float boxes in network pixels, four original sizes: mode 1 on the raw rows == mode 0 on undo_letterbox's float32 boxes == the
    restatement on their int() -- every ground truth is a detection's own truncated box grown by one pixel on one side, so a coordinate
    that is off by one changes an IoU across 0.5 or 1.0 somewhere among 1024 detections"""
    nc, B, K, G = 3, 4, 256, 64
    rs = np.random.RandomState(5)
    image_hw = np.array([[375, 500], [500, 333], [97, 640], [128, 128]], np.int64)
    rows = np.zeros((B, K, 6), np.float32)
    lt = rs.uniform(0, 100, (B, K, 2)).astype(np.float32)
    rows[..., 0:2] = lt
    rows[..., 2:4] = lt + rs.uniform(1, 27, (B, K, 2)).astype(np.float32)
    rows[..., 4] = rs.uniform(0.001, 1, (B, K)).astype(np.float32)
    rows[..., 5] = rs.randint(0, nc, (B, K))
    counts = np.array([K, K - 3, K, 17], np.int32)
    final = rows.copy()
    for b in range(B):
        final[b, :, :4] = undo_letterbox(rows[b], (128, 128), image_hw[b], letterbox)[0]
        assert np.array_equal(final[b, :, :4], R.undo_letterbox_f32(rows[b, :, :4], (128, 128), image_hw[b], letterbox))
    gt = np.zeros((B, G, 6), np.int32)
    for b in range(B):
        for g in range(G):
            r = rs.randint(0, counts[b])
            box = [int(v) for v in final[b, r, :4]]
            box[rs.randint(0, 4)] += rs.randint(-1, 2)
            gt[b, g] = [int(rows[b, r, 5])] + box + [0]
    gt_counts = np.full(B, G, np.int32)
    box_map = det_eval.letterbox_box_map(torch.from_numpy(image_hw).to(dev), (128, 128), letterbox)
    ev1 = det_eval.DetectionEvaluator(nc, K, B * K, dev)
    ev1.add_batch(*on(dev, rows, counts, gt, gt_counts), box_map)
    ev0 = evaluate(dev, nc, final, counts, gt, gt_counts)
    want = R.get_map(R.detections_from_rows(final, counts), R.ground_truth_from_arrays(gt, gt_counts), nc)
    check_against(ev0, want, nc)
    check_against(ev1, want, nc)
    assert 50 < ev1.results()["tp"].sum() < counts.sum()


@pytest.mark.parametrize("letterbox", [True, False])
def test_inverse_maps_restated_on_the_device(dev, letterbox):
    """``correct_boxes_device`` against the YOLOv7 / SSD wrappers' numpy ``_correct_boxes`` and ``reverse_letterbox_device`` against
    ``CenterNetA._finish``'s operations, bit for bit"""
    from configs import CenternetConfig, SsdConfig
    from core.algorithms.centernet import CenterNetA
    from core.algorithms.ssd import Ssd
    cfg = SsdConfig()
    cfg.decode.letterbox_image = letterbox
    ssd = Ssd(cfg, dev)
    rs = np.random.RandomState(6)
    image_hw = np.array([[375, 500], [500, 333], [97, 640]], np.int64)
    lt = rs.uniform(0, 0.8, (3, 50, 2)).astype(np.float32)
    boxes = np.concatenate((lt, lt + rs.uniform(0.01, 0.2, (3, 50, 2)).astype(np.float32)), 2)
    got = det_eval.correct_boxes_device(torch.from_numpy(boxes).to(dev), (300, 300), torch.from_numpy(image_hw).to(dev), letterbox).cpu().numpy()
    for b in range(3):
        o = boxes[b]
        xy, wh = (o[:, 0:2] + o[:, 2:4]) / 2, o[:, 2:4] - o[:, 0:2]
        assert np.array_equal(got[b], ssd._correct_boxes(xy, wh, [300, 300], [int(image_hw[b, 0]), int(image_hw[b, 1])]))
    if letterbox:
        ccfg = CenternetConfig()
        ccfg.arch.input_size = (3, 128, 160)
        algo = CenterNetA(ccfg, dev)
        got = det_eval.reverse_letterbox_device(torch.from_numpy(boxes).to(dev), algo.input_size, torch.from_numpy(image_hw).to(dev)).cpu().numpy()
        for b in range(3):
            out = dict(counts=torch.tensor([50]), keep=torch.arange(50).view(1, 50), boxes=torch.from_numpy(boxes[b:b + 1]),
                       scores=torch.zeros(1, 50), classes=torch.zeros(1, 50))
            assert np.array_equal(got[b], algo._finish(out, 0, int(image_hw[b, 0]), int(image_hw[b, 1]))[0])


class TinyLoader:
    """two batches of two images in memory: (images, dict(image_hw, gt, gt_counts)) on the device"""

    def __init__(self, images, image_hw, gt, gt_counts):
        self.items = [(images[i:i + 2], dict(image_hw=image_hw[i:i + 2], gt=gt[i:i + 2], gt_counts=gt_counts[i:i + 2])) for i in (0, 2)]

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def ground_truth_near(final_rows, counts, G, seed):
    """ground truths made from every third detection's own truncated box, moved by up to 2 pixels; one in four difficult"""
    rs = np.random.RandomState(seed)
    B = len(counts)
    gt, gt_counts = np.zeros((B, G, 6), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        for r in range(0, min(int(counts[b]), 3 * G), 3):
            box = [int(v) + int(rs.randint(-2, 3)) for v in final_rows[b, r, :4]]
            gt[b, gt_counts[b]] = [int(final_rows[b, r, 5])] + box + [int(rs.rand() < 0.25)]
            gt_counts[b] += 1
    return gt, gt_counts


def test_yolov8_evaluate_on_voc_end_to_end(dev, tmp_path):
    """seed-0 YOLOv8-n, nc = 20, 128 x 128, conf_threshold 0.001 as the reference sets it.  The random-init class biases
    (-10.2 / -8.8 / -7.4 per level) leave no score above 0.001; raised by 3 the CPU oracle keeps 16 detections per image, 64 in all."""
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8
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
    from computervision.pytorch_amd import engine as E
    with torch.no_grad():
        y = torch.cat([model(images[i:i + 2])[0] for i in (0, 2)])
    rows, _, counts = E.nms(y, 0.001, algo.iou_threshold, algo.max_det)
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    total = int(counts.sum())
    print(f"YOLOv8-n detections above 0.001: {counts.tolist()}")
    assert 0 < total < 4 * algo.max_det and 16 <= total <= 256              # 64 on the CPU oracle
    final = rows.copy()
    for b in range(4):
        final[b, :, :4] = undo_letterbox(rows[b], (128, 128), image_hw[b], algo.letterbox_image)[0]
    gt, gt_counts = ground_truth_near(final, counts, 6, seed=2)
    loader = TinyLoader(images, *on(dev, image_hw, gt, gt_counts))
    res = algo.evaluate_on_voc(model, str(tmp_path), "val", dataloader=loader)
    want = R.get_map(R.detections_from_rows(final, counts), R.ground_truth_from_arrays(gt, gt_counts), 20)
    for k in ("tp", "n_det", "n_gt"):
        assert np.array_equal(res[k], want["res"][k]), k
    for k in ("ap", "precision", "recall", "f1"):
        assert np.abs(res[k] - want["res"][k]).max() <= AP_TOL, k
    assert abs(res["mAP"] - want["res"]["mAP"]) <= AP_TOL and res["tp"].sum() > 0
    from configs.dataset_cfg import VOC_CFG
    assert open(os.path.join(tmp_path, "results", "results.txt")).read() == det_eval.format_report(want["res"], want["curves"], VOC_CFG["classes"])


def test_centernet_evaluate_on_voc_end_to_end(dev, tmp_path):
    """seed-0 CenterNet DLA-34 at 128 x 128 (the size of its forward fixture), nc = 20: random-init scores are about 0.5 everywhere, so
    every image has K = 100 peaks above 0.001.  The random-init size head (the "reg" head, as the reference's decode reads it) gives -0.01,
    which the decode clamps to boxes of zero size that no ground truth two pixels away overlaps by half; its bias raised by 6 makes
    boxes six feature cells wide, of which the DIoU-NMS keeps 72 / 64 / 65 / 67 on the CPU oracle, 18 of them true positives here."""
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
    total = int(counts.sum())
    print(f"CenterNet detections above 0.001: {counts.tolist()}")
    assert 0 < total < 4 * algo.K and total >= 100
    gt, gt_counts = ground_truth_near(final, counts, 6, seed=3)
    loader = TinyLoader(images, *on(dev, image_hw, gt, gt_counts))
    res = algo.evaluate_on_voc(model, str(tmp_path), "val", dataloader=loader)
    want = R.get_map(R.detections_from_rows(final, counts), R.ground_truth_from_arrays(gt, gt_counts), 20)
    for k in ("tp", "n_det", "n_gt"):
        assert np.array_equal(res[k], want["res"][k]), k
    for k in ("ap", "precision", "recall", "f1"):
        assert np.abs(res[k] - want["res"][k]).max() <= AP_TOL, k
    assert abs(res["mAP"] - want["res"]["mAP"]) <= AP_TOL and res["tp"].sum() > 0
