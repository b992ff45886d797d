"""MI355X: ``cvx_det_confusion`` + ``cvx_det_conf_curves`` through ``DetectionDiagnostics`` against the sequential restatement
(tests/det_diag_restatement.py) and the reference's LAMR (tests/golden/det_lamr_ref.npz): the fixture, sizes around the workgroup and the
LDS rounding, the planted image, box-map mode 1, skipped images and bad classes, batch splitting, hand-built records, no host read in
``add_batch``, and ``evaluate_on_voc(diagnostics=)`` of YOLOv8 and of a one-member ensemble end to end.  No tolerance anywhere: tables are
equal as integers, curves as fp64 bit patterns; each check prints its mismatch count first."""
import os

import numpy as np
import pytest
import torch

import det_diag_restatement as D
import det_eval_restatement as R
from computervision.pytorch_amd import CvxError, det_diag, det_eval
from core.utils.boxes import undo_letterbox

pytestmark = pytest.mark.gpu
FILES = ("confusion_matrix.csv", "confidence_curves.csv", "diagnostics.txt")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def on(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def same_bits(name, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = int(np.count_nonzero(got.view(np.int64) != want.view(np.int64))) if got.dtype == np.float64 else int(np.count_nonzero(got != want))
    print(f"{name}: {bad} of {got.size} differ")
    assert bad == 0, name


def accumulate(dev, nc, rows, counts, gt, gt_counts, spec, box_map=None, quantize=True, evaluator=True):
    diag = det_diag.DetectionDiagnostics(nc, rows.shape[1], dev, spec, quantize_scores=quantize)
    ev = det_eval.DetectionEvaluator(nc, rows.shape[1], rows.shape[0] * rows.shape[1], dev, quantize_scores=quantize) if evaluator else None
    t = on(dev, rows, counts, gt, gt_counts) + [None if box_map is None else on(dev, box_map)[0]]
    diag.add_batch(*t)
    if ev is not None:
        ev.add_batch(*t)
    return diag, ev


def restate(nc, rows, counts, gt, gt_counts, spec, quantize=True):
    """everything ``results()`` returns, from the two restatements"""
    dets, gts = R.detections_from_rows(rows, counts, quantize), R.ground_truth_from_arrays(gt, gt_counts)
    conf = D.confusion(dets, gts, nc, spec.conf, spec.iou)
    gm = R.get_map(dets, gts, nc)
    flags, scores = D.flags_per_class(dets, gm["flags"], nc), D.scores_per_class(dets, nc)
    records = [(scores[c], gm["curves"][c][0], gm["curves"][c][1], flags[c]) for c in range(nc)]
    want = D.conf_curves(records, gm["res"]["n_gt"], spec.points, spec.smooth_window, quantize)
    images = conf["images_per_class"]
    want["mr9"] = np.stack([D.miss_rates(records[c][2], D.fp_cumsum(flags[c]), images[c]) for c in range(nc)])
    want["lamr"] = np.array([D.lamr(want["mr9"][c], len(scores[c]), images[c]) for c in range(nc)])
    want.update(confusion=conf["confusion"], images_per_class=images, n_gt=gm["res"]["n_gt"])
    return want


def check_results(res, want):
    for k in ("confusion", "images_per_class", "best_index_per_class"):
        same_bits(k, res[k], want[k])
    for k in ("conf_grid", "precision", "recall", "f1", "mean_f1", "mean_f1_smooth", "mr9"):
        same_bits(k, res[k], want[k])
    print(f"best index {res['best_index']} against {want['best_index']}")
    assert res["best_index"] == want["best_index"] and res["best_conf"] == want["conf_grid"][want["best_index"]]
    assert np.array_equal(res["lamr"], want["lamr"], equal_nan=True), (res["lamr"], want["lamr"])
    k = want["best_index"]
    same_bits("f1_at_best", res["f1_at_best"], want["f1"][:, k].copy())
    same_bits("best_conf_per_class", res["best_conf_per_class"], want["conf_grid"][want["best_index_per_class"]])
    with_gt = want["n_gt"] > 0
    if with_gt.any():
        assert res["mean_f1_at_best"] == float(np.mean(want["f1"][:, k][with_gt]))
        assert res["mean_precision_at_best"] == float(np.mean(want["precision"][:, k][with_gt]))
    keep = with_gt & ~np.isnan(want["lamr"])
    assert res["mean_lamr"] == (float(np.mean(want["lamr"][keep])) if keep.any() else 0.0)


def test_fixture_of_the_reference(dev, gold, tmp_path):
    z, ref = gold("det_map_ref.npz"), gold("det_lamr_ref.npz")
    names = z["names"].tolist()
    nc = len(names)
    _, _, arrays = R.fixture_inputs(z)
    assert arrays[0].shape[0] == 40 and arrays[0].shape[1] <= 16 and arrays[2].shape == (40, 6, 6)         # one batch
    spec = det_diag.DetDiagnostics()
    diag, ev = accumulate(dev, nc, *arrays, spec)
    res = diag.results(ev)
    want = restate(nc, *arrays, spec)
    check_results(res, want)
    same_bits("confusion()", diag.confusion(), want["confusion"])
    for c in z["gt_classes"].tolist():                                     # the reference's own LAMR
        print(f"class {c}: LAMR {res['lamr'][c]!r} against {float(ref['lamr'][c])!r}")
        assert res["lamr"][c] == ref["lamr"][c]
    assert np.isnan(res["lamr"][5]) and np.array_equal(res["images_per_class"], ref["images_per_class"])
    m = res["confusion"]
    assert m[:nc, :nc].sum() - np.trace(m[:nc, :nc]) == 14 and np.array_equal(m[:, :nc].sum(0), ev.results()["n_gt"])
    paths = diag.write_report(str(tmp_path / "results"), names)
    assert [os.path.basename(p) for p in paths] == list(FILES)
    assert open(paths[0]).read() == det_diag.format_confusion_csv(want["confusion"], names)
    assert open(paths[1]).read() == det_diag.format_curves_csv(res, names) and open(paths[1]).read().count("\n") == 1002
    text = open(paths[2]).read()
    assert text == det_diag.format_diagnostics(res, names) and "recommended conf_threshold = {0:.4f}".format(want["conf_grid"][want["best_index"]]) in text


SIZES = [(1, 0, 1), (255, 1, 4), (256, 2, 80), (257, 3, 4), (600, 64, 80), (64, 64, 1)]


@pytest.mark.parametrize("K,G,nc", SIZES)
def test_sizes_around_the_workgroup(dev, K, G, nc):
    """five images: full, no detection, no ground truth, neither, and a full one with a single ground truth"""
    counts, gt_counts = [K, 0, (K + 1) // 2, 0, K], [G, G, 0, 0, min(G, 1)]
    arrays = D.seeded_case(100 + K, 5, nc, K, max(G, 1), counts=counts, gt_counts=gt_counts)
    if G == 0:
        arrays = (arrays[0], arrays[1], arrays[2][:, :0], arrays[3])
    spec = det_diag.DetDiagnostics(points=101, smooth_window=11)
    diag, ev = accumulate(dev, nc, *arrays, spec)
    res = diag.results(ev)
    check_results(res, restate(nc, *arrays, spec))
    assert res["confusion"].sum() > 0 or K == 1


def test_the_largest_block_takes_the_large_lds_path(dev):
    """K = 16384 rows and G = 1024 ground truths, about 100 KB of LDS: one image with 300 rows against all 1024 ground truths, one with
    every row against 3.  (``cvx_det_match`` does not hold this pair, so the matrix is checked alone.)"""
    nc = 4
    rows, counts, gt, gt_counts = D.seeded_case(19, 2, nc, 16384, 1024, size=512, counts=[300, 16384], gt_counts=[1024, 3])
    spec = det_diag.DetDiagnostics()
    diag, _ = accumulate(dev, nc, rows, counts, gt, gt_counts, spec, evaluator=False)
    want = D.confusion(R.detections_from_rows(rows, counts), R.ground_truth_from_arrays(gt, gt_counts), nc, spec.conf, spec.iou)
    same_bits("confusion", diag.confusion(), want["confusion"])
    same_bits("images_per_class", diag.images_per_class.cpu().numpy(), want["images_per_class"])
    assert want["confusion"][:nc, :nc].sum() > 50 and want["lost"] > 0


def test_planted_image_alone_and_last_in_a_batch(dev):
    (rows, counts, gt, gt_counts), want, images = D.planted_case()
    spec = det_diag.DetDiagnostics(conf=0.25, iou=0.45)
    diag, _ = accumulate(dev, 3, rows, counts, gt, gt_counts, spec, evaluator=False)
    same_bits("alone", diag.confusion(), want)
    same_bits("images", diag.images_per_class.cpu().numpy(), images)
    a = D.seeded_case(7, 2, 3, 9, 7)
    batch = [np.concatenate((x, y)) for x, y in zip(a, (rows, counts, gt, gt_counts))]
    diag, ev = accumulate(dev, 3, *batch, spec)
    res = diag.results(ev)
    before = D.confusion(R.detections_from_rows(a[0], a[1]), R.ground_truth_from_arrays(a[2], a[3]), 3, 0.25, 0.45)
    same_bits("last of a batch", res["confusion"], before["confusion"] + want)
    check_results(res, restate(3, *batch, spec))


@pytest.mark.parametrize("letterbox", [True, False])
def test_box_map_mode_1_is_undo_letterbox(dev, letterbox):
    """the data of test_det_eval_gpu's box-map test: mode 1 on the raw rows == mode 0 on undo_letterbox's float32 boxes == the
    restatement on their int()"""
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
            gt[b, g] = [int(rows[b, r, 5]) if rs.rand() < 0.8 else rs.randint(0, nc)] + box + [int(rs.rand() < 0.2)]
    gt_counts = np.full(B, G, np.int32)
    box_map = det_eval.letterbox_box_map(torch.from_numpy(image_hw).to(dev), (128, 128), letterbox).cpu().numpy()
    spec = det_diag.DetDiagnostics(points=101, smooth_window=11)
    want = restate(nc, final, counts, gt, gt_counts, spec)
    d1, e1 = accumulate(dev, nc, rows, counts, gt, gt_counts, spec, box_map=box_map)
    d0, e0 = accumulate(dev, nc, final, counts, gt, gt_counts, spec)
    check_results(d0.results(e0), want)
    check_results(d1.results(e1), want)
    m = want["confusion"]
    assert np.trace(m[:nc, :nc]) > 50 and m[:nc, :nc].sum() > np.trace(m[:nc, :nc])


def test_skipped_image_and_bad_classes(dev):
    nc = 4
    rows, counts, gt, gt_counts = D.seeded_case(41, 3, nc, 16, 6, counts=[16, 16, 16], gt_counts=[6, 6, 6])
    counts[1] = -1                                                          # cvx_nms: more candidates than its sort holds
    rows[0, 0, 4:6] = (0.99, nc)
    gt[2, 0, 0] = nc
    spec = det_diag.DetDiagnostics()
    diag, ev = accumulate(dev, nc, rows, counts, gt, gt_counts, spec)
    keep = [0, 2]
    want = D.confusion(R.detections_from_rows(rows[keep], counts[keep]), R.ground_truth_from_arrays(gt[keep], gt_counts[keep]), nc, spec.conf, spec.iou)
    assert want["bad_class"] == 2
    same_bits("state", diag.state.cpu().numpy(), np.array([2, 1, 2, 0], np.int64))
    same_bits("the other cells", diag.matrix.cpu().numpy(), want["confusion"])
    same_bits("images", diag.images_per_class.cpu().numpy(), want["images_per_class"])
    with pytest.raises(CvxError):
        diag.results(ev)
    with pytest.raises(CvxError, match="skipped"):
        diag.confusion()
    counts[1] = 17                                                          # past its block
    gt_counts[0] = 7
    diag, _ = accumulate(dev, nc, rows, counts, gt, gt_counts, spec, evaluator=False)
    same_bits("state", diag.state.cpu().numpy()[:2], np.array([1, 2], np.int64))
    rows[0, 0, 5], counts[1], gt_counts[0] = 0, 16, 6
    diag, _ = accumulate(dev, nc, rows, counts, gt, gt_counts, spec, evaluator=False)
    with pytest.raises(CvxError, match="class indices"):
        diag.confusion()


def test_scores_as_they_are_and_cut_to_the_text(dev):
    """conf = 0.7 and a third of the scores float32(0.7) = 0.699999988...: cut to the text they are '0.7' and take part, as they are they
    stay below the threshold"""
    nc = 4
    rows, counts, gt, gt_counts = D.seeded_case(61, 4, nc, 64, 6, counts=[64, 64, 0, 33], gt_counts=[6, 0, 6, 3])
    rows[..., 4][np.random.RandomState(62).rand(4, 64) < 0.33] = np.float32(0.7)
    spec = det_diag.DetDiagnostics(conf=0.7, iou=0.3, points=11, smooth_window=3)
    got = {}
    for quantize in (True, False):
        diag, ev = accumulate(dev, nc, rows, counts, gt, gt_counts, spec, quantize=quantize)
        got[quantize] = diag.results(ev)
        check_results(got[quantize], restate(nc, rows, counts, gt, gt_counts, spec, quantize))
    assert got[True]["confusion"][:nc].sum() >= got[False]["confusion"][:nc].sum() + 30


def test_two_batches_equal_one_and_reset_clears(dev):
    nc = 4
    a, b = D.seeded_case(31, 3, nc, 16, 6), D.seeded_case(32, 3, nc, 16, 6)
    spec = det_diag.DetDiagnostics(points=101, smooth_window=11)
    whole = [np.concatenate((x, y)) for x, y in zip(a, b)]
    d1, e1 = accumulate(dev, nc, *whole, spec)
    d2 = det_diag.DetectionDiagnostics(nc, 16, dev, spec)
    e2 = det_eval.DetectionEvaluator(nc, 16, 96, dev)
    for part in (a, b):
        d2.add_batch(*on(dev, *part))
        e2.add_batch(*on(dev, *part))
    r1, r2 = d1.results(e1), d2.results(e2)
    for k in ("confusion", "images_per_class", "precision", "recall", "f1", "mean_f1", "mean_f1_smooth", "mr9", "best_index_per_class"):
        same_bits(k, r2[k], r1[k])
    assert r1["best_index"] == r2["best_index"] and r1["confusion"].sum() > 20
    same_bits("state", d2.state.cpu().numpy(), np.array([6, 0, 0, 0], np.int64))
    d2.reset()
    assert int(d2._block.abs().sum()) == 0
    e2.reset()
    d2.add_batch(*on(dev, *a))
    e2.add_batch(*on(dev, *a))
    check_results(d2.results(e2), restate(nc, *a, spec))


def hand_built_records(seed):
    """six classes with 0, 1, 255, 256, 257 and 513 records: the chunk boundaries of the scan and of the binary search.  Class 1: one record
    at 0.3; class 2: every score 0.7, records but no ground truth and no image; class 3: scores on the tenths (0.3 and 0.7 as float32 lie
    on either side of the decimal); class 4: seeded scores, one image; class 5: thousandths and seeded scores."""
    rs = np.random.RandomState(seed)
    lengths = [0, 1, 255, 256, 257, 513]
    gt_per_class = np.array([3, 2, 0, 0, 0, 0], np.int64)                     # classes 3 .. 5: their true positives and three more
    images = np.array([2, 1, 0, 30, 1, 100], np.int64)
    scores = [np.zeros(0, np.float32), np.array([0.3], np.float32), np.full(255, 0.7, np.float32),
              (rs.randint(0, 11, 256) / 10).astype(np.float32), rs.uniform(0.001, 1.0, 257).astype(np.float32),
              np.concatenate(((rs.randint(1, 1001, 300) / 1000).astype(np.float32), rs.uniform(0.001, 1.0, 213).astype(np.float32)))]
    records = []
    for c, n in enumerate(lengths):
        s = np.sort(scores[c])[::-1].copy()
        # true positives gather at the high scores, so that F1 peaks inside the grid; one record in ten is neither
        flag = np.where(rs.rand(n) < s.astype(np.float64) ** 2, 1, np.where(rs.rand(n) < 0.9, 0, 2)).astype(np.int32)
        flag[:1] = 1                                                        # the best record is a true positive: recall > 0 from there on
        if c >= 3:
            gt_per_class[c] = int((flag == 1).sum()) + 3
        tp, fp = np.cumsum(flag == 1), np.cumsum(flag == 0)
        rec = tp / float(max(gt_per_class[c], 1))
        prec = tp / np.maximum(tp + fp, 1).astype(np.float64)
        records.append((s, prec, rec, flag))
    return records, gt_per_class, images


@pytest.mark.parametrize("quantize", [True, False])
@pytest.mark.parametrize("points,window", [(2, 1), (11, 3), (11, 101), (1001, 101)])
def test_curves_on_hand_built_records(dev, points, window, quantize):
    records, gt_per_class, images = hand_built_records(3)
    nc = len(records)
    seg_off = np.concatenate(([0], np.cumsum([len(r[0]) for r in records]))).astype(np.int64)
    score, prec, rec, flag = (np.concatenate([r[i] for r in records]) for i in range(4))
    t = on(dev, score, prec, rec, flag, seg_off, gt_per_class, images)
    words = det_diag.conf_curves(dict(score=t[0], prec=t[1], rec=t[2], flag=t[3], seg_off=t[4]), t[5], t[6], nc, quantize, points, window)
    got = det_diag.unpack_curves(words.cpu().numpy(), nc, points)
    want = D.conf_curves(records, gt_per_class, points, window, quantize)
    for k in ("precision", "recall", "f1", "mean_f1", "mean_f1_smooth", "best_index_per_class"):
        same_bits(k, got[k], want[k])
    assert got["best_index"] == want["best_index"]
    mr9 = np.stack([D.miss_rates(records[c][2], D.fp_cumsum(records[c][3]), images[c]) for c in range(nc)])
    same_bits("mr9", got["mr9"], mr9)
    assert (mr9[0] == 1).all() and (mr9[2] == 1).all() and (mr9[3] < 1).any() and (mr9[5] < 1).any()
    assert got["precision"][0].tolist() == [1.0] * points and got["f1"][0].tolist() == [0.0] * points
    if points == 11:                                                        # float32(0.3) >= 0.3 > float32(0.7): the cut score decides
        assert (got["recall"][1, 3] > 0) and (got["recall"][1, 4] == 0)
        assert (got["recall"][2, 7] > 0) == quantize
    lamr = det_diag.lamr_from_mr9(got["mr9"], [len(r[0]) for r in records], images)
    assert np.array_equal(lamr, [D.lamr(mr9[c], len(records[c][0]), images[c]) for c in range(nc)], equal_nan=True)
    assert lamr[0] == 0.0 and np.isnan(lamr[2])


def test_add_batch_makes_no_host_read(dev):
    nc = 4
    arrays = D.seeded_case(51, 3, nc, 16, 6)
    spec = det_diag.DetDiagnostics()
    diag = det_diag.DetectionDiagnostics(nc, 16, dev, spec)
    t = on(dev, *arrays)
    diag.add_batch(*t)                                                      # first use: the code object, the buffers
    diag.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=dev).item()
            flags = False
        except RuntimeError:
            flags = True
        print(f"set_sync_debug_mode('error') flags a read-back on this build: {flags}")
        diag.add_batch(*t)
        diag.add_batch(*t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    want = D.confusion(R.detections_from_rows(arrays[0], arrays[1]), R.ground_truth_from_arrays(arrays[2], arrays[3]), nc, spec.conf, spec.iou)
    same_bits("twice the batch", diag.confusion(), 2 * want["confusion"])


class TinyLoader:
    """two batches of two images in memory: (images, dict(image_hw, gt, gt_counts)) on the device"""

    def __init__(self, images, image_hw, gt, gt_counts):
        self.items = [(images[i:i + 2], dict(image_hw=image_hw[i:i + 2], gt=gt[i:i + 2], gt_counts=gt_counts[i:i + 2])) for i in (0, 2)]

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


@pytest.fixture(scope="module")
def yolov8(dev):
    """seed-0 YOLOv8-n, nc = 20, 128 x 128, the class biases raised by 3 as in test_det_eval_gpu: scores sit just above 0.001"""
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8
    from oracle import synth
    cfg = Yolo8DetConfig()
    cfg.dataset.num_classes, cfg.arch.input_size = 20, (3, 128, 128)
    algo = YOLOv8(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for k in [k for k in sd if ".cv3." in k and k.endswith(".2.bias")]:
        sd[k] += 3.0
    model.load_state_dict(sd)
    images = synth.images(4, 128, 128, seed=1).to(dev)
    image_hw = np.array([[375, 500], [500, 333], [128, 128], [97, 200]], np.int64)
    return algo, model, images, image_hw


def ground_truth_near(final_rows, counts, G, seed, nc):
    """ground truths made from every third detection's own truncated box, moved by up to 2 pixels; one in four difficult, one in four of
    another class"""
    rs = np.random.RandomState(seed)
    B = len(counts)
    gt, gt_counts = np.zeros((B, G, 6), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        for r in range(0, min(int(counts[b]), 3 * G), 3):
            box = [int(v) + int(rs.randint(-2, 3)) for v in final_rows[b, r, :4]]
            cls = int(final_rows[b, r, 5]) if rs.rand() < 0.75 else int(rs.randint(0, nc))
            gt[b, gt_counts[b]] = [cls] + box + [int(rs.rand() < 0.25)]
            gt_counts[b] += 1
    return gt, gt_counts


def evaluate_both_ways(evaluate, tmp_path, spec, nc=20):
    """``evaluate(root, diagnostics)`` with and without the spec: the files, the invariants, the untouched rest"""
    res = evaluate(str(tmp_path / "with"), spec)
    plain = evaluate(str(tmp_path / "plain"), None)
    assert "diagnostics" not in plain and sorted(res) == sorted(list(plain) + ["diagnostics"])
    for k, v in plain.items():
        assert np.array_equal(np.asarray(res[k]), np.asarray(v), equal_nan=True), k
    assert open(tmp_path / "with" / "results" / "results.txt", "rb").read() == open(tmp_path / "plain" / "results" / "results.txt", "rb").read()
    for name in FILES:
        assert os.path.getsize(tmp_path / "with" / "results" / name) > 0 and not os.path.exists(tmp_path / "plain" / "results" / name)
    d = res["diagnostics"]
    m = d["confusion"]
    reaching = int(m[:nc].sum())
    print(f"detections that reach conf {spec.conf} and count: {reaching}; matched {int(m[:nc, :nc].sum())}; recommended conf {d['best_conf']}")
    assert reaching > 0, "no detection reaches conf: the test shows nothing"
    assert np.array_equal(m[:, :nc].sum(0), res["n_gt"]) and m[nc, nc] == 0
    assert d["precision"].shape == (nc, spec.points) and 0 <= d["best_index"] < spec.points
    return res


def test_yolov8_evaluate_on_voc_with_diagnostics_end_to_end(dev, yolov8, tmp_path):
    from computervision.pytorch_amd import engine as E
    from configs.dataset_cfg import VOC_CFG
    algo, model, images, image_hw = yolov8
    with torch.no_grad():
        y = torch.cat([model(images[i:i + 2])[0] for i in (0, 2)])
    rows, _, counts = E.nms(y, 0.001, algo.iou_threshold, algo.max_det)
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    final = rows.copy()
    for b in range(4):
        final[b, :, :4] = undo_letterbox(rows[b], (128, 128), image_hw[b], algo.letterbox_image)[0]
    gt, gt_counts = ground_truth_near(final, counts, 6, seed=2, nc=20)
    loader = TinyLoader(images, *on(dev, image_hw, gt, gt_counts))
    spec = det_diag.DetDiagnostics(conf=0.001, points=101, smooth_window=11)
    res = evaluate_both_ways(lambda root, diag: algo.evaluate_on_voc(model, root, "val", dataloader=loader, diagnostics=diag), tmp_path, spec)
    want = restate(20, final, counts, gt, gt_counts, spec)
    check_results(res["diagnostics"], want)
    assert want["confusion"][:20, :20].sum() > 0
    assert open(tmp_path / "with" / "results" / "confusion_matrix.csv").read() == det_diag.format_confusion_csv(want["confusion"], VOC_CFG["classes"])


def test_one_member_ensemble_evaluate_on_voc_with_diagnostics(dev, yolov8, tmp_path):
    from computervision.pytorch_amd import box_fusion
    algo, model, images, image_hw = yolov8
    ens = box_fusion.DetEnsemble([(algo, model)])
    tail = ens._evaluation_tails("evaluate_on_voc")
    t_hw = torch.from_numpy(image_hw).to(dev)
    parts = [tail(images[i:i + 2], dict(image_hw=t_hw[i:i + 2])) for i in (0, 2)]
    assert all(p[2] is None for p in parts)
    K = max(int(p[0].shape[1]) for p in parts)
    final = np.zeros((4, K, 6), np.float32)
    for j, p in enumerate(parts):
        final[2 * j:2 * j + 2, :p[0].shape[1]] = p[0].cpu().numpy()
    counts = np.concatenate([p[1].cpu().numpy() for p in parts]).astype(np.int32)
    print("fused rows per image", counts.tolist())
    assert counts.min() >= 1
    gt, gt_counts = ground_truth_near(final, counts, 6, seed=4, nc=20)
    loader = TinyLoader(images, *on(dev, image_hw, gt, gt_counts))
    spec = det_diag.DetDiagnostics(conf=0.001, points=101, smooth_window=11)
    res = evaluate_both_ways(lambda root, diag: ens.evaluate_on_voc(root, "val", dataloader=loader, diagnostics=diag), tmp_path, spec)
    check_results(res["diagnostics"], restate(20, final, counts, gt, gt_counts, spec))
