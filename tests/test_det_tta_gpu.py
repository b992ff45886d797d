"""MI355X: scale and flip test-time augmentation for the detectors.  The two launches of csrc/det_tta.hip (``cvx_det_tta_inputs``,
``cvx_det_fuse_views``) against the numpy restatement (tests/det_tta_restatement.py), bit for bit, and the surfaces -- ``predict_batch``,
``detect_frames``, ``evaluate_on_voc``, ``evaluate_on_coco`` with ``tta=`` -- end to end against the same wrapper steps with the
restatement's fusion on the host."""
import numpy as np
import pytest
import torch

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import coco_eval, det_eval
from computervision.pytorch_amd import det_tta as T
from computervision.pytorch_amd import render as R
import det_tta_restatement as DR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def on(dev, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def pictures(shapes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


# ---- 1. the input kernel ------------------------------------------------------------------------------------------------------------------
ZOOMS = [1.0, 0.83, 0.67, 0.5]
FLIPS = {"off": [False] * 4, "on": [True] * 4, "mixed": [False, True, True, False]}


@pytest.mark.parametrize("flips", sorted(FLIPS))
@pytest.mark.parametrize("input_hw", [(40, 56), (41, 37)])          # 16-byte stores, and a width that allows none
def test_input_kernel_equals_the_restatement(dev, input_hw, flips):
    H, W = input_hw
    B = 2
    images = np.random.RandomState(H).rand(B, 3, H, W).astype(np.float32)
    sizes = [(int(np.floor(H * z + 0.5)), int(np.floor(W * z + 0.5)), f) for z, f in zip(ZOOMS, FLIPS[flips])]
    views = [DR.view_rect(H, W, *s) for s in sizes]
    table = T.view_table(sizes, (H, W))
    assert [tuple(r)[:5] for r in table.tolist()] == [(h, w, t, l, int(f)) for h, w, t, l, f in views]
    slots = len(views) * B + 1                                       # one slot no view names stays as it was
    out = torch.full((slots, 3, H, W), -7.0, dtype=torch.float32, device=dev)
    got = T.tta_inputs(torch.from_numpy(images).to(dev), table, out=out)
    assert got is out
    got = got.cpu().numpy()
    want = DR.tta_inputs(images, views, slots=slots)
    assert (got[-1] == -7.0).all() and np.isnan(want[-1]).all()
    for s in range(slots - 1):
        assert same_bits(got[s], want[s]), s
    if not FLIPS[flips][0]:                                          # the identity view equals its input
        assert same_bits(got[:B], images)
    assert (got[B:2 * B, :, 0, :] == DR.PAD).all()                   # the first row of a smaller view is padding
    fresh = T.tta_inputs(torch.from_numpy(images).to(dev), table, pad=0.25).cpu().numpy()
    assert fresh.shape == (slots - 1, 3, H, W) and (fresh[B:2 * B, :, 0, :] == 0.25).all()


def test_det_tta_inputs_are_the_table_of_its_views(dev):
    tta = T.DetTTA()
    images = np.random.RandomState(1).rand(2, 3, 64, 96).astype(np.float32)
    views = [DR.view_rect(64, 96, *s) for s in tta.views((64, 96))]
    assert same_bits(tta.inputs(torch.from_numpy(images).to(dev)).cpu().numpy(), DR.tta_inputs(images, views))


# ---- 2. the fusion kernel -----------------------------------------------------------------------------------------------------------------
def check_fuse(got, want):
    rows, counts, source, members, overflow = (t.cpu().numpy() for t in got)
    assert counts.tolist() == want[1].tolist() and overflow.tolist() == [want[4]]
    assert np.array_equal(source, want[2]) and np.array_equal(members, want[3]) and same_bits(rows, want[0])


@pytest.mark.parametrize("max_det", [5, 300])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("V", [1, 3, 6])
@pytest.mark.parametrize("B", [1, 3])
def test_fuse_kernel_equals_the_restatement(dev, B, V, agnostic, max_det):
    """both modes and both score modes of every case; with B = 3, frame 1 has no candidates"""
    rows, counts, vmap = DR.fuse_case(B, V)
    hw = DR.FRAME_HW[:B]
    device = on(dev, [rows, counts, vmap, hw])
    for mode in ("nms", "vote"):
        for score in ("max", "views"):
            want = DR.fuse_views(rows, counts, vmap, hw, 0.5, agnostic, mode, score, max_det)
            assert want[4] == 0 and want[1][0] >= 2 and (B == 1 or want[1][1] == 0)
            check_fuse(T.fuse_views(*device, 0.5, agnostic, mode, score, max_det), want)


@pytest.mark.parametrize("mode", ["nms", "vote"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_fuse_kernel_across_a_mask_word_edge(dev, n, mode):
    """n candidates of one frame over three views of 64: one, two and three 64-bit words per matrix row; a kept row gathers members from
    the matrix's row behind it and from its column before it"""
    rows, counts, vmap = DR.word_case(n)
    want = DR.fuse_views(rows, counts, vmap, DR.WORD_FRAME_HW, 0.5, False, mode, "views", 300)
    check_fuse(T.fuse_views(*on(dev, [rows, counts, vmap, DR.WORD_FRAME_HW]), 0.5, False, mode, "views", 300), want)


def test_fuse_kernel_flags_a_bad_count(dev):
    rows, counts, vmap = DR.fuse_case(3, 3)
    d_rows, _, d_map, d_hw = on(dev, [rows, counts, vmap, DR.FRAME_HW])
    for bad in (-1, DR.K_IN + 1):
        c = counts.copy()
        c[3] = bad                                                   # view 1 of frame 0
        want = DR.fuse_views(rows, c, vmap, DR.FRAME_HW, 0.5, False, "vote", "max", 300)
        assert want[4] == 1 and not np.isin(want[2][0], np.arange(3 * DR.K_IN, 4 * DR.K_IN)).any() and want[1][0] >= 2
        check_fuse(T.fuse_views(d_rows, torch.from_numpy(c).to(dev), d_map, d_hw, 0.5, False, "vote", "max", 300), want)
    before = torch.full((1,), 5, dtype=torch.int32, device=dev)      # a word the caller hands in is added to
    assert T.fuse_views(d_rows, torch.from_numpy(c).to(dev), d_map, d_hw, overflow=before)[4].tolist() == [6]


@pytest.mark.parametrize("extra", [0, 1])
def test_fuse_kernel_capacity(dev, extra):
    """exactly 8192 disjoint candidates in a frame pass; 8193 give count -1 and overflow 1 -- flagged, never truncated"""
    rows, counts, vmap, frame_hw = DR.capacity_case(extra)
    want = DR.fuse_views(rows, counts, vmap, frame_hw, 0.5, False, "vote", "max", 300)
    assert want[1].tolist() == [0, -1 if extra else 300] and want[4] == extra
    got = T.fuse_views(*on(dev, [rows, counts, vmap, frame_hw]), 0.5, False, "vote", "max", 300)
    check_fuse(got, want)
    if extra:
        with pytest.raises(CvxError):                                # the one host read refuses a dropped frame
            R.read_detections(*R.det_to_image(got[0], got[1]))


def test_fuse_views_validates_its_arguments(dev):
    rows, counts, vm, hw = on(dev, [np.zeros((4, 4, 6), np.float32), np.zeros(4, np.int32), np.zeros((4, 4), np.float32), np.ones((2, 2), np.int32)])
    for bad in (dict(fuse="wbf"), dict(score="mean"), dict(threshold=1.5), dict(max_det=0), dict(max_det=T.FUSE_CAP + 1)):
        with pytest.raises(ValueError):
            T.fuse_views(rows, counts, vm, hw, **bad)
    for args in ((rows[..., :5], counts, vm, hw), (rows, counts.long(), vm, hw), (rows, counts, vm[:2], hw), (rows, counts, vm.double(), hw),
                 (rows, counts, vm, hw.float()), (rows[:3], counts[:3], vm[:3], hw), (rows, counts, vm.cpu(), hw)):
        with pytest.raises(ValueError):
            T.fuse_views(*args)
    with pytest.raises(ValueError):
        T.tta_inputs(torch.zeros(1, 3, 40, 56, device=dev), T.view_table([(40, 56, False)], (40, 56)), out=torch.zeros(1, 3, 40, 48, device=dev))
    assert T.fuse_views(rows, counts, vm, hw)[1].tolist() == [0, 0]


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def yolov8(dev):
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8
    cfg = Yolo8DetConfig()
    cfg.dataset.num_classes, cfg.arch.input_size = 20, (3, 128, 128)
    algo = YOLOv8(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for k in [k for k in sd if ".cv3." in k and k.endswith(".2.bias")]:
        sd[k] += 3.0                                           # random-init class biases leave no score above 0.001 (tests/test_det_eval_gpu.py)
    model.load_state_dict(sd)
    return algo, model


def detector(name, dev):
    if name == "yolo7":
        from configs import Yolo7Config
        from core.algorithms.yolo_v7 import YOLOv7
        cfg = Yolo7Config()
        cfg.arch.input_size, cfg.train.pretrained = (3, 160, 224), False
        return YOLOv7(cfg, dev), 0.2
    if name == "ssd":
        from configs import SsdConfig
        from core.algorithms.ssd import Ssd
        cfg = SsdConfig()
        cfg.train.pretrained = False
        return Ssd(cfg, dev), 0.07
    from configs import CenternetConfig
    from core.algorithms.centernet import CenterNetA
    cfg = CenternetConfig()
    cfg.arch.input_size = (3, 128, 128)
    return CenterNetA(cfg, dev), 0.3


def compose(algo, model, x, image_hw, conf, tta, max_det=None):
    """the expectation: the wrapper's own steps -- the views, the class's tail on the B slots of each view, ``det_to_image``, the blocks
    padded to one width -- with the restatement's fusion on the host.  Returns the restatement's five outputs and the per-slot counts."""
    B, (H, W) = int(x.shape[0]), (int(v) for v in x.shape[2:])
    views = tta.inputs(x)
    vmap = tta.view_map(image_hw, (H, W), terms=algo._box_map_terms(image_hw, (H, W))).cpu().numpy()
    rows_of = algo._evaluation_rows(model)
    parts, bad = [], np.zeros(B, bool)
    for k in range(tta.n_views):
        rows, counts, box_map = rows_of(views[k * B:(k + 1) * B], {"image_hw": image_hw}, conf)
        c = counts.cpu().numpy()
        bad |= (c < 0) | (c > rows.shape[1])
        rows, counts, _ = R.det_to_image(rows, counts, box_map)
        parts.append((rows.cpu().numpy(), counts.cpu().numpy()))
    K = max(p[0].shape[1] for p in parts)
    rows = np.zeros((tta.n_views * B, K, 6), np.float32)
    for k, (r, _) in enumerate(parts):
        rows[k * B:(k + 1) * B, :r.shape[1]] = r
    counts = np.concatenate([p[1] for p in parts])
    thr = tta.iou if tta.iou is not None else getattr(algo, "iou_threshold", None) or algo.nms_threshold
    out = DR.fuse_views(rows, counts, vmap, image_hw.cpu().numpy(), thr, tta.class_agnostic, tta.fuse_mode, tta.score,
                        tta.max_det if max_det is None else max_det)
    assert not bad.any()
    return out, counts


def compose_frames(algo, model, frames, conf, tta):
    input_hw, letterbox = algo._predict_input()
    fb = R.FrameBatch(frames, input_hw, letterbox)
    return compose(algo, model, fb.network_input(), fb.image_hw, conf, tta)


FRAME_SHAPES = [(200, 300), (97, 128), (128, 128)]
TTAS = [dict(), dict(fuse="nms", iou=0.6, score="views", class_agnostic=True, max_det=7)]


@pytest.mark.parametrize("params", TTAS, ids=["default", "nms"])
def test_yolov8_predict_batch_equals_the_composition(dev, yolov8, params):
    algo, model = yolov8
    tta = T.DetTTA(**params)
    frames = on(dev, pictures(FRAME_SHAPES, 41))
    want, slot_counts = compose_frames(algo, model, frames, 0.001, tta)
    print("YOLOv8-n views: rows per slot", slot_counts.tolist(), "fused per frame", want[1].tolist(), "largest member count", int(want[3].max()))
    assert want[4] == 0 and want[1].min() > 0
    rows, counts = algo.predict_batch(model, frames, conf_threshold=0.001, sync=False, tta=tta)
    assert rows.is_cuda and rows.shape == (3, tta.max_det, 6) and counts.tolist() == want[1].tolist()
    assert same_bits(rows.cpu().numpy(), want[0])
    triples = algo.predict_batch(model, frames, conf_threshold=0.001, sync=True, tta=tta)
    for f, (boxes, scores, classes) in enumerate(triples):
        n = int(want[1][f])
        assert same_bits(boxes, want[0][f, :n, :4]) and same_bits(scores, want[0][f, :n, 4]) and np.array_equal(classes, want[0][f, :n, 5].astype(np.int64))


def test_yolov7_predict_batch_equals_the_composition(dev):
    """the tail without a box map: its rows are final boxes, and the view map undoes ``correct_boxes_device``"""
    algo, conf = detector("yolo7", dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    tta = T.DetTTA()
    frames = on(dev, pictures([(224, 314), (85, 119)], 42))
    want, slot_counts = compose_frames(algo, model, frames, conf, tta)
    print("YOLOv7 views: rows per slot", slot_counts.tolist(), "fused per frame", want[1].tolist(), "overflow", want[4])
    rows, counts = algo.predict_batch(model, frames, conf_threshold=conf, sync=False, tta=tta)
    assert counts.tolist() == want[1].tolist() and same_bits(rows.cpu().numpy(), want[0])


@pytest.mark.parametrize("name", ["yolo8", "yolo7", "ssd", "centernet"])
def test_one_plain_view_is_plain_predict_batch(dev, yolov8, name):
    """``DetTTA(scales=(1.0,), flips=(False,), fuse="nms", iou=1.0)`` suppresses nothing (no IoU exceeds 1) and maps through a = 1, c = 0:
    its rows are plain ``predict_batch``'s rows bit for bit -- in the fusion's own order, (score descending, row ascending), where the
    tails of YOLOv7 and SSD go class by class; the first ``max_det`` = 300 of them; and with the fusion's clamp to the picture, which a
    box of the plain path may overhang."""
    if name == "yolo8":
        (algo, model), conf = yolov8, 0.001
    else:
        algo, conf = detector(name, dev)
        torch.manual_seed(0)
        model = algo.build_model()[0].to(dev).eval()
    (H, W), _ = algo._predict_input()
    shapes = [(H * 7 // 5, W * 7 // 5), (H // 2 + 5, W // 2 + 7)]
    frames = on(dev, pictures(shapes, 43))
    plain_rows, plain_counts = (t.cpu().numpy() for t in algo.predict_batch(model, frames, conf_threshold=conf, sync=False))
    tta = T.DetTTA(scales=(1.0,), flips=(False,), fuse="nms", iou=1.0)
    rows, counts = (t.cpu().numpy() for t in algo.predict_batch(model, frames, conf_threshold=conf, sync=False, tta=tta))
    print(f"{name}: plain rows per frame above {conf}: {plain_counts.tolist()}, through one plain view {counts.tolist()}")
    assert plain_counts.sum() > 0 and rows.shape == (2, 300, 6)
    zero = np.float32(0)
    for f, (h, w) in enumerate(shapes):
        n = int(plain_counts[f])
        p = plain_rows[f, :n]
        key = ((np.uint64(0xFFFFFFFF) - p[:, 4].view(np.uint32).astype(np.uint64)) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        p = p[np.argsort(key, kind="stable")][:300].copy()
        p[:, :4] = p[:, :4] * np.float32(1) + zero                   # a = 1, c = 0: the bits stay, but for a -0
        p[:, [0, 2]] = np.fmin(np.fmax(p[:, [0, 2]], zero), np.float32(w))
        p[:, [1, 3]] = np.fmin(np.fmax(p[:, [1, 3]], zero), np.float32(h))
        assert counts[f] == len(p) and same_bits(rows[f, :len(p)], p) and not rows[f, len(p):].any(), (name, f)


def test_detect_frames_paints_what_predict_batch_paints(dev, yolov8):
    from scripts import detect
    algo, model = yolov8
    tta = T.DetTTA()
    host = pictures(FRAME_SHAPES + [(64, 90), (150, 140)], 44)
    direct = on(dev, host)
    configured, algo.conf_threshold = algo.conf_threshold, 0.001     # detect_frames predicts at the configured confidence
    try:
        rows3, counts3 = algo.predict_batch(model, direct[:3], draw=True, sync=False, tta=tta)
        algo.predict_batch(model, direct[3:], draw=True, sync=False, tta=tta)
        video = on(dev, host)
        batches = list(detect.detect_frames(algo, model, iter(video), 3, tta=tta))
    finally:
        algo.conf_threshold = configured
    torch.cuda.synchronize()
    assert [len(b) for b in batches] == [3, 2] and all(f is v for f, v in zip([f for b in batches for f in b], video))
    painted = 0
    for b in range(5):
        assert torch.equal(video[b], direct[b]), b
        painted += int((direct[b].cpu().numpy() != host[b]).any())
    print("frames painted", painted, "rows per frame", counts3.tolist())
    assert painted > 0
    with pytest.raises(CvxError):
        detect.detect_frames(algo, model, iter(video), 3, tiled={}, tta=tta)


# ---- 4. the evaluations -------------------------------------------------------------------------------------------------------------------
class Loader:
    """two batches of two images: (images, meta) on the device.  With ``arm``, torch's synchronisation check is on from the first batch
    to the end of the iteration, and ``flagged`` says whether this build's check raises on a read-back at all."""

    def __init__(self, images, arm=False, **meta):
        self.items = [(images[i:i + 2], {k: v[i:i + 2] for k, v in meta.items()}) for i in (0, 2)]
        self.arm, self.flagged = arm, None

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        if not self.arm:
            yield from self.items
            return
        torch.cuda.set_sync_debug_mode("error")
        try:
            try:
                torch.ones(1, device=self.items[0][0].device).item()
                self.flagged = False
            except RuntimeError:
                self.flagged = True
            yield from self.items
        finally:
            torch.cuda.set_sync_debug_mode("default")


def ground_truths(final_rows, counts, G, seed):
    """VOC and COCO ground truths made from every third fused row's own box, moved a little; one in four difficult / a crowd"""
    rs = np.random.RandomState(seed)
    B = len(counts)
    voc, coco, n = np.zeros((B, G, 6), np.int32), np.zeros((B, G, 7), np.float64), np.zeros(B, np.int32)
    for b in range(B):
        for r in range(0, min(int(counts[b]), 3 * G), 3):
            x1, y1, x2, y2 = (float(v) for v in final_rows[b, r, :4])
            hard = int(rs.rand() < 0.25)
            voc[b, n[b]] = [int(final_rows[b, r, 5])] + [int(v) + int(rs.randint(-2, 3)) for v in (x1, y1, x2, y2)] + [hard]
            x, y, w, h = x1 + rs.randint(-8, 9) / 8, y1 + rs.randint(-8, 9) / 8, x2 - x1 + rs.randint(-8, 9) / 8, y2 - y1 + rs.randint(-8, 9) / 8
            coco[b, n[b]] = [final_rows[b, r, 5], x, y, w, h, w * h, hard]
            n[b] += 1
    return voc, coco, n


def same_results(got, want):
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v), equal_nan=True), k


def test_yolov8_evaluations_equal_the_evaluators_on_the_composition(dev, yolov8, tmp_path):
    from oracle import synth
    algo, model = yolov8
    tta = T.DetTTA()
    images = synth.images(4, 128, 128, seed=1).to(dev)
    image_hw = torch.tensor([[375, 500], [500, 333], [128, 128], [97, 200]], device=dev)
    max_det = min(algo.eval_max_det, 8192)
    batches = [compose(algo, model, images[i:i + 2], image_hw[i:i + 2], 0.001, tta, max_det)[0] for i in (0, 2)]      # also every first use
    fused, counts = np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])
    print("fused rows per image", counts.tolist(), "largest member count", max(int(b[3].max()) for b in batches))
    assert counts.min() > 0 and all(b[4] == 0 for b in batches)
    voc, coco, n = ground_truths(fused, counts, 6, seed=2)
    t_voc, t_coco, t_n = on(dev, [voc, coco, n])
    capacity = 4 * max_det
    ev, cv = det_eval.DetectionEvaluator(20, algo.eval_max_det, capacity, dev), coco_eval.CocoEvaluator(20, algo.eval_max_det, capacity, dev)
    for j, i in enumerate((0, 2)):
        r, c = on(dev, [batches[j][0], batches[j][1]])
        ev.add_batch(r, c, t_voc[i:i + 2], t_n[i:i + 2], None)
        cv.add_batch(r, c, t_coco[i:i + 2], t_n[i:i + 2], None)
    want_voc, want_coco = ev.results(), cv.results()
    assert want_voc["tp"].sum() > 0 and want_coco["stats"][0] > 0
    torch.cuda.synchronize()
    loader = Loader(images, arm=True, image_hw=image_hw, gt=t_voc, gt_counts=t_n)
    try:
        res = algo.evaluate_on_voc(model, str(tmp_path / "voc"), "val", dataloader=loader, capacity=capacity, tta=tta)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loader.flagged, "torch.cuda.set_sync_debug_mode('error') does not flag a read-back on this build"
    same_results(res, want_voc)
    loader = Loader(images, arm=True, image_hw=image_hw, gt_coco=t_coco, gt_counts=t_n)
    try:
        res = algo.evaluate_on_coco(model, str(tmp_path / "coco"), "val", dataloader=loader, capacity=capacity, tta=tta)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loader.flagged
    same_results(res, want_coco)
    assert (tmp_path / "coco" / "coco_results.txt").read_text() == cv.summary_text()


def test_centernet_evaluation_equals_the_evaluator_on_the_composition(dev, tmp_path):
    """a tail whose rows are final boxes, through ``evaluate_on_voc``: CenterNet at 128 x 128, the size head's bias raised by 6 as in
    tests/test_det_eval_gpu.py"""
    from oracle import synth
    from configs import CenternetConfig
    from core.algorithms.centernet import CenterNetA
    cfg = CenternetConfig()
    cfg.dataset.num_classes, cfg.arch.input_size = 20, (3, 128, 128)
    algo = CenterNetA(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["backbone.reg.2.bias"] += 6.0
    model.load_state_dict(sd)
    tta = T.DetTTA(scales=(1.0, 0.75), flips=(False, True))
    images = synth.images(4, 128, 128, seed=1).to(dev)
    image_hw = torch.tensor([[375, 500], [500, 333], [128, 128], [97, 200]], device=dev)
    max_det = min(algo.eval_max_det, 8192)
    batches = [compose(algo, model, images[i:i + 2], image_hw[i:i + 2], 0.001, tta, max_det)[0] for i in (0, 2)]
    fused, counts = np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])
    print("CenterNet fused rows per image", counts.tolist())
    assert counts.min() > 0
    voc, _, n = ground_truths(fused, counts, 6, seed=3)
    t_voc, t_n = on(dev, [voc, n])
    ev = det_eval.DetectionEvaluator(algo.num_classes, algo.eval_max_det, 4 * max_det, dev)
    for j, i in enumerate((0, 2)):
        ev.add_batch(*on(dev, [batches[j][0], batches[j][1]]), t_voc[i:i + 2], t_n[i:i + 2], None)
    res = algo.evaluate_on_voc(model, str(tmp_path), "val", dataloader=Loader(images, image_hw=image_hw, gt=t_voc, gt_counts=t_n), capacity=4 * max_det,
                               tta=tta)
    same_results(res, ev.results())
