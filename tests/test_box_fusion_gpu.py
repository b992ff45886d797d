"""MI355X: Weighted Boxes Fusion and the detector ensemble.  The launch of csrc/box_fusion.hip (``cvx_det_fuse_wbf``) against the numpy
restatement (tests/box_fusion_restatement.py), bit for bit, and the surfaces -- ``predict_batch(..., tta=DetTTA(fusion=WBF()))``,
``DetEnsemble.predict_batch``, ``.evaluate_on_voc``, ``.evaluate_on_coco`` -- end to end against the same steps with the restatement's
fusion on the host.  The fixtures follow tests/test_det_tta_gpu.py: YOLOv8-n at 128 x 128 with the class biases raised, CenterNet at
128 x 128 with the size head's bias raised."""
import numpy as np
import pytest
import torch

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import box_fusion as BF
from computervision.pytorch_amd import coco_eval, det_eval
from computervision.pytorch_amd import det_tta as T
from computervision.pytorch_amd import render as R
import box_fusion_restatement as BR

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


def check_fuse(got, want):
    rows, counts, source, members, overflow = (t.cpu().numpy() for t in got)
    assert counts.tolist() == want[1].tolist() and overflow.tolist() == [want[4]]
    assert np.array_equal(source, want[2]) and np.array_equal(members, want[3]) and same_bits(rows, want[0])


def both(dev, case, **kw):
    """the kernel and the restatement on one case (rows, counts, view_map, frame_hw, weights); returns the restatement's outputs"""
    rows, counts, vmap, hw, weights = case
    kw.setdefault("iou", BR.WBF_IOU)
    want = BR.fuse_wbf(rows, counts, vmap, hw, weights, kw["iou"], **{k: v for k, v in kw.items() if k != "iou"})
    check_fuse(BF.fuse_wbf(*on(dev, [rows, counts, vmap, hw]), weights=weights, **kw), want)
    return want


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_det", [5, 300])
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("S", [1, 3, 6])
@pytest.mark.parametrize("B", [1, 3])
def test_kernel_equals_the_restatement(dev, B, S, agnostic, max_det):
    """both confidences with and without the rescaling; unequal weights, flipped and scaled maps; with B = 3, frame 1 has no candidates"""
    for conf in ("avg", "max"):
        for rescale in (False, True):
            want = both(dev, BR.wbf_case(B, S), conf=conf, rescale=rescale, class_agnostic=agnostic, max_det=max_det)
            assert want[4] == 0 and want[1][0] >= 2 and (B == 1 or want[1][1] == 0)


@pytest.mark.parametrize("kind", ["disjoint", "copies"])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_kernel_across_the_lane_stride(dev, n, kind):
    """n disjoint boxes: n clusters, the cluster index crosses the 64 lanes of the walking wave once and twice; n near-copies: one cluster
    of n members"""
    want = both(dev, BR.stride_case(kind, n))
    assert want[1].tolist() == [n if kind == "disjoint" else 1]


def test_candidate_70_matches_cluster_66(dev):
    want = both(dev, BR.stride_case("mixed", 0), conf="max", rescale=False)
    assert want[1].tolist() == [70] and want[3][0, 66] == 2


@pytest.mark.parametrize("n_classes", [17, 40])
def test_more_segments_than_waves(dev, n_classes):
    """17 and 40 classes in one frame, the indices with gaps, a third of the segments of one candidate"""
    want = both(dev, BR.classes_case(n_classes))
    assert len(set(want[0][0, :want[1][0], 5].tolist())) == n_classes
    both(dev, BR.classes_case(n_classes), class_agnostic=True, conf="max")


@pytest.mark.parametrize("extra", [0, 1])
def test_kernel_capacity(dev, extra):
    """exactly 8192 disjoint candidates in a frame pass -- 8192 clusters of one class, walked by one wave --; 8193 give count -1 and
    overflow 1: flagged, never truncated"""
    case = BR.capacity_case(extra)
    want = both(dev, case)
    assert want[1].tolist() == [0, -1 if extra else 300] and want[4] == extra
    if extra:
        got = BF.fuse_wbf(*on(dev, case[:4]))
        with pytest.raises(CvxError):                                # the one host read refuses a dropped frame
            R.read_detections(*R.det_to_image(got[0], got[1]))


def test_kernel_flags_a_bad_count_and_adds_to_a_callers_word(dev):
    rows, counts, vmap, hw, weights = BR.wbf_case(3, 3)
    for bad in (-1, rows.shape[1] + 1):
        c = counts.copy()
        c[3] = bad                                                   # source 1 of frame 0
        want = both(dev, (rows, c, vmap, hw, weights))
        assert want[4] == 1 and not np.isin(want[2][0], np.arange(3 * rows.shape[1], 4 * rows.shape[1])).any() and want[1][0] >= 2
    before = torch.full((1,), 5, dtype=torch.int32, device=dev)
    got = BF.fuse_wbf(*on(dev, [rows, c, vmap, hw]), weights=weights, overflow=before)
    assert got[4] is before and before.tolist() == [6]


def test_two_calls_give_the_same_bits(dev):
    case = BR.wbf_case(3, 6)
    device = on(dev, case[:4])
    first = [t.cpu().numpy() for t in BF.fuse_wbf(*device, weights=case[4], class_agnostic=True)]
    again = [t.cpu().numpy() for t in BF.fuse_wbf(*device, weights=case[4], class_agnostic=True)]
    assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
               for a, b in zip(first, again))


def test_fuse_wbf_validates_its_arguments(dev):
    rows, counts, vm, hw = on(dev, [np.zeros((4, 4, 6), np.float32), np.zeros(4, np.int32), np.zeros((4, 4), np.float32), np.ones((2, 2), np.int32)])
    for bad in (dict(conf="mean"), dict(iou=1.5), dict(skip_score=-0.5), dict(max_det=0), dict(max_det=BF.FUSE_CAP + 1), dict(weights=[1.0]),
                dict(weights=[1.0, 0.0]), dict(weights=[1.0, float("inf")]), dict(weights=torch.ones(2, device=dev))):
        with pytest.raises(ValueError):
            BF.fuse_wbf(rows, counts, vm, hw, **bad)
    for args in ((rows[..., :5], counts, vm, hw), (rows, counts.long(), vm, hw), (rows, counts, vm[:2], hw), (rows, counts, vm.double(), hw),
                 (rows, counts, vm, hw.float()), (rows[:3], counts[:3], vm[:3], hw), (rows, counts, vm.cpu(), hw)):
        with pytest.raises(ValueError):
            BF.fuse_wbf(*args)
    many = on(dev, [np.zeros((33, 4, 6), np.float32), np.zeros(33, np.int32), np.zeros((33, 4), np.float32), np.ones((1, 2), np.int32)])
    with pytest.raises(ValueError):                                  # more than 32 sources
        BF.fuse_wbf(*many)
    assert BF.fuse_wbf(rows, counts, vm, hw)[1].tolist() == [0, 0]


# ---- 2. end to end ------------------------------------------------------------------------------------------------------------------------
def yolov8_model(algo, dev, seed):
    torch.manual_seed(seed)
    model = algo.build_model()[0].to(dev).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for k in [k for k in sd if ".cv3." in k and k.endswith(".2.bias")]:
        sd[k] += 3.0                                           # random-init class biases leave no score above 0.001 (tests/test_det_eval_gpu.py)
    model.load_state_dict(sd)
    return model


@pytest.fixture(scope="module")
def yolov8(dev):
    """the detector and two sets of weights"""
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8
    cfg = Yolo8DetConfig()
    cfg.dataset.num_classes, cfg.arch.input_size = 20, (3, 128, 128)
    algo = YOLOv8(cfg, dev)
    return algo, yolov8_model(algo, dev, 0), yolov8_model(algo, dev, 1)


@pytest.fixture(scope="module")
def centernet(dev):
    from configs import CenternetConfig
    from core.algorithms.centernet import CenterNetA
    cfg = CenternetConfig()
    cfg.dataset.num_classes, cfg.arch.input_size = 20, (3, 128, 128)
    algo = CenterNetA(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["backbone.reg.2.bias"] += 6.0                           # the size head's bias, as in tests/test_det_eval_gpu.py
    model.load_state_dict(sd)
    return algo, model


def detector(name, dev):
    if name == "yolo7":
        from configs import Yolo7Config
        from core.algorithms.yolo_v7 import YOLOv7
        cfg = Yolo7Config()
        cfg.arch.input_size, cfg.train.pretrained = (3, 160, 224), False
        return YOLOv7(cfg, dev), 0.2
    from configs import SsdConfig
    from core.algorithms.ssd import Ssd
    cfg = SsdConfig()
    cfg.train.pretrained = False
    return Ssd(cfg, dev), 0.07


def padded(parts):
    """[(rows (B, K_k, 6), counts (B))] numpy -> (rows (S * B, K, 6), counts (S * B)), slot k * B + b"""
    B, K = parts[0][0].shape[0], max(p[0].shape[1] for p in parts)
    rows = np.zeros((len(parts) * B, K, 6), np.float32)
    for k, (r, _) in enumerate(parts):
        rows[k * B:(k + 1) * B, :r.shape[1]] = r
    return rows, np.concatenate([p[1] for p in parts])


def tail_rows(rows_of, x, image_hw, conf):
    """a tail's rows as final boxes, on the host; no frame may be flagged"""
    rows, counts, box_map = rows_of(x, {"image_hw": image_hw}, conf)
    c = counts.cpu().numpy()
    assert not ((c < 0) | (c > rows.shape[1])).any()
    rows, counts, _ = R.det_to_image(rows, counts, box_map)
    return rows.cpu().numpy(), counts.cpu().numpy()


def wbf_of(fusion, rows, counts, vmap, hw, weights, max_det):
    return BR.fuse_wbf(rows, counts, vmap, hw, weights, fusion.iou, fusion.skip_score, fusion.conf, fusion.rescale, fusion.class_agnostic, max_det)


def compose_views(algo, model, x, image_hw, conf, tta, max_det=None):
    """the expectation of ``DetTTA(fusion=WBF())``: the wrapper's own steps -- the views, the class's tail on the B slots of each view,
    ``det_to_image``, the blocks padded to one width -- with the restatement's fusion on the host"""
    B, (H, W) = int(x.shape[0]), (int(v) for v in x.shape[2:])
    views = tta.inputs(x)
    vmap = tta.view_map(image_hw, (H, W), terms=algo._box_map_terms(image_hw, (H, W))).cpu().numpy()
    rows_of = algo._evaluation_rows(model)
    rows, counts = padded([tail_rows(rows_of, views[k * B:(k + 1) * B], image_hw, conf) for k in range(tta.n_views)])
    return wbf_of(tta.fusion, rows, counts, vmap, image_hw.cpu().numpy(), tta.fusion.weights, tta.max_det if max_det is None else max_det)


def compose_members(parts, image_hw, weights, fusion, max_det=None):
    """the expectation of ``DetEnsemble``: the members' final rows padded to one width, identity maps, the restatement's fusion"""
    rows, counts = padded(parts)
    vmap = np.tile(BR.IDENTITY, (len(rows), 1))
    return wbf_of(fusion, rows, counts, vmap, image_hw.cpu().numpy(), weights, fusion.max_det if max_det is None else max_det)


def member_input(algo, frames):
    input_hw, letterbox = algo._predict_input()
    fb = R.FrameBatch(frames, input_hw, letterbox)
    return fb.network_input(), fb.image_hw


FRAME_SHAPES = [(200, 300), (97, 128), (128, 128)]
FUSIONS = [dict(), dict(iou=0.6, skip_score=0.002, conf="max", rescale=False, weights=[2.0, 1.0, 0.5], class_agnostic=True)]


def check_predictions(predict, want, max_det):
    """``predict(sync)``: the device rows against the expectation, then the triples of the one host read"""
    rows, counts = predict(False)
    assert rows.is_cuda and rows.shape == (len(want[1]), max_det, 6) and counts.tolist() == want[1].tolist()
    assert same_bits(rows.cpu().numpy(), want[0])
    for f, (boxes, scores, classes) in enumerate(predict(True)):
        n = int(want[1][f])
        assert same_bits(boxes, want[0][f, :n, :4]) and same_bits(scores, want[0][f, :n, 4]) and np.array_equal(classes, want[0][f, :n, 5].astype(np.int64))


@pytest.mark.parametrize("params", FUSIONS, ids=["default", "weighted"])
def test_yolov8_tta_with_wbf_equals_the_composition(dev, yolov8, params):
    algo, model, _ = yolov8
    tta = T.DetTTA(fusion=BF.WBF(**params), max_det=40 if params else 300)
    frames = on(dev, pictures(FRAME_SHAPES, 41))
    x, image_hw = member_input(algo, frames)
    want = compose_views(algo, model, x, image_hw, 0.001, tta)
    print("YOLOv8-n views through WBF: fused per frame", want[1].tolist(), "largest member count", int(want[3].max()))
    assert want[4] == 0 and want[1].min() > 0 and want[3].max() >= 2
    check_predictions(lambda sync: algo.predict_batch(model, frames, conf_threshold=0.001, sync=sync, tta=tta), want, tta.max_det)


def test_centernet_tta_with_wbf_equals_the_composition(dev, centernet):
    """a tail whose rows are final boxes, and whose boxes stay inside the picture: many clusters of several members across two views"""
    algo, model = centernet
    tta = T.DetTTA(scales=(1.0, 0.75), flips=(False, True), fusion=BF.WBF(weights=[1.0, 0.5]))
    frames = on(dev, pictures(FRAME_SHAPES, 48))
    x, image_hw = member_input(algo, frames)
    want = compose_views(algo, model, x, image_hw, 0.3, tta)
    print("CenterNet views through WBF: fused per frame", want[1].tolist(), "largest member count", int(want[3].max()))
    assert want[4] == 0 and want[1].min() >= 2 and want[3].max() >= 2
    check_predictions(lambda sync: algo.predict_batch(model, frames, conf_threshold=0.3, sync=sync, tta=tta), want, tta.max_det)


def test_two_yolov8_weights_ensemble_equals_the_composition(dev, yolov8):
    algo, m1, m2 = yolov8
    fusion = BF.WBF(max_det=100)
    ens = BF.DetEnsemble([(algo, m1), (algo, m2, 2.0)], fusion)
    frames = on(dev, pictures(FRAME_SHAPES, 45))
    x, image_hw = member_input(algo, frames)
    parts = [tail_rows(algo._evaluation_rows(m), x, image_hw, 0.001) for m in (m1, m2)]
    want = compose_members(parts, image_hw, [1.0, 2.0], fusion)
    print("two YOLOv8-n: rows per member", [p[1].tolist() for p in parts], "fused", want[1].tolist(), "largest member count", int(want[3].max()))
    assert want[4] == 0 and want[1].min() > 0
    check_predictions(lambda sync: ens.predict_batch(frames, conf_threshold=0.001, sync=sync), want, 100)


def test_ensemble_behind_a_tta_fuses_twice(dev, yolov8):
    """each member fuses its own views as the DetTTA says -- here by the vote of cvx_det_fuse_views --, then the ensemble fuses the members"""
    import det_tta_restatement as DR
    algo, m1, m2 = yolov8
    tta, fusion = T.DetTTA(scales=(1.0, 0.75), flips=(False, True), max_det=50), BF.WBF()
    ens = BF.DetEnsemble([(algo, m1), (algo, m2)], fusion, tta=tta)
    frames = on(dev, pictures(FRAME_SHAPES[:2], 46))
    x, image_hw = member_input(algo, frames)
    views = tta.inputs(x)
    vmap = tta.view_map(image_hw, (128, 128), terms=algo._box_map_terms(image_hw, (128, 128))).cpu().numpy()
    parts = []
    for m in (m1, m2):
        rows, counts = padded([tail_rows(algo._evaluation_rows(m), views[k * 2:(k + 1) * 2], image_hw, 0.001) for k in range(2)])
        voted = DR.fuse_views(rows, counts, vmap, image_hw.cpu().numpy(), getattr(algo, "iou_threshold", None) or algo.nms_threshold, False, "vote", "max", 50)
        parts.append((voted[0], voted[1]))
    want = compose_members(parts, image_hw, [1.0, 1.0], fusion)
    assert want[1].min() > 0
    rows, counts = ens.predict_batch(frames, conf_threshold=0.001, sync=False)
    assert counts.tolist() == want[1].tolist() and same_bits(rows.cpu().numpy(), want[0])


def test_yolov8_and_centernet_ensemble_mixes_tails_and_box_maps(dev, yolov8, centernet):
    """a tail that reports through a box map and one whose rows are final boxes, each on its own network batch"""
    (y8, m1, _), (cn, mc) = yolov8, centernet
    fusion = BF.WBF(iou=0.5, class_agnostic=True, max_det=100)
    ens = BF.DetEnsemble([(y8, m1, 1.5), (cn, mc)], fusion)
    frames = on(dev, pictures(FRAME_SHAPES, 47))
    parts = []
    for algo, model in ((y8, m1), (cn, mc)):
        x, image_hw = member_input(algo, frames)
        parts.append(tail_rows(algo._evaluation_rows(model), x, image_hw, 0.001))
    want = compose_members(parts, image_hw, [1.5, 1.0], fusion)
    print("YOLOv8-n + CenterNet: rows per member", [p[1].tolist() for p in parts], "fused", want[1].tolist(), "largest member count", int(want[3].max()))
    assert want[4] == 0 and all(p[1].min() > 0 for p in parts)
    check_predictions(lambda sync: ens.predict_batch(frames, conf_threshold=0.001, sync=sync), want, 100)
    drawn = [f.clone() for f in frames]
    ens.predict_batch(drawn, conf_threshold=0.001, draw=True, sync=False)
    assert any(not torch.equal(a, b) for a, b in zip(drawn, frames))


@pytest.mark.parametrize("name", ["yolo8", "centernet", "yolo7", "ssd"])
def test_one_member_is_plain_predict_batch(dev, yolov8, centernet, name):
    """a one-member ensemble under ``WBF(iou=1.0, rescale=False)`` fuses nothing (no IoU exceeds 1): its rows are plain ``predict_batch``'s
    bit for bit -- in the fusion's order, (score descending, row ascending); clamped to the picture; without the rows the clamp leaves no
    area; the first ``max_det`` = 300 of them"""
    if name == "yolo8":
        (algo, model, _), conf = yolov8, 0.001
    elif name == "centernet":
        (algo, model), conf = centernet, 0.3
    else:
        algo, conf = detector(name, dev)
        torch.manual_seed(0)
        model = algo.build_model()[0].to(dev).eval()
    (H, W), _ = algo._predict_input()
    shapes = [(H * 7 // 5, W * 7 // 5), (H // 2 + 5, W // 2 + 7)]
    frames = on(dev, pictures(shapes, 43))
    plain_rows, plain_counts = (t.cpu().numpy() for t in algo.predict_batch(model, frames, conf_threshold=conf, sync=False))
    ens = BF.DetEnsemble([(algo, model)], BF.WBF(iou=1.0, rescale=False))
    rows, counts = (t.cpu().numpy() for t in ens.predict_batch(frames, conf_threshold=conf, sync=False))
    print(f"{name}: plain rows per frame above {conf}: {plain_counts.tolist()}, through a one-member ensemble {counts.tolist()}")
    assert plain_counts.sum() > 0 and rows.shape == (2, 300, 6)
    zero = np.float32(0)
    for f, (h, w) in enumerate(shapes):
        n = int(plain_counts[f])
        p = plain_rows[f, :n].copy()
        p[:, :4] = p[:, :4] * np.float32(1) + zero                   # a = 1, c = 0: the bits stay, but for a -0
        p[:, [0, 2]] = np.fmin(np.fmax(p[:, [0, 2]], zero), np.float32(w))
        p[:, [1, 3]] = np.fmin(np.fmax(p[:, [1, 3]], zero), np.float32(h))
        p[:, 4] = p[:, 4] * np.float32(1)
        ordinal = np.arange(n, dtype=np.uint64)[(p[:, 2] > p[:, 0]) & (p[:, 3] > p[:, 1])]
        p = p[ordinal.astype(np.int64)]
        key = ((np.uint64(0xFFFFFFFF) - p[:, 4].view(np.uint32).astype(np.uint64)) << np.uint64(32)) | ordinal
        p = p[np.argsort(key, kind="stable")][:300]
        assert counts[f] == len(p) and same_bits(rows[f, :len(p)], p) and not rows[f, len(p):].any(), (name, f)


# ---- 3. the evaluations -------------------------------------------------------------------------------------------------------------------
class Loader:
    """two batches of two images: (images, meta) on the device; torch's synchronisation check is on from the first batch to the end of the
    iteration, and ``flagged`` says whether this build's check raises on a read-back at all (tests/test_det_tta_gpu.py)"""

    def __init__(self, images, **meta):
        self.items = [(images[i:i + 2], {k: v[i:i + 2] for k, v in meta.items()}) for i in (0, 2)]
        self.flagged = None

    def __len__(self):
        return len(self.items)

    def __iter__(self):
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


def test_ensemble_evaluations_equal_the_evaluators_on_the_composition(dev, yolov8, centernet, tmp_path):
    from oracle import synth
    """YOLOv8-n with weight 2 and CenterNet, both at 128 x 128 (with the random YOLOv8 weights of the tests every box overhangs the picture
    and a frame's rows fold into one; CenterNet's carry the weight)"""
    (algo, m1, _), (cn, mc) = yolov8, centernet
    members = [(algo, m1), (cn, mc)]
    assert algo._predict_input() == cn._predict_input()
    fusion = BF.WBF()
    ens = BF.DetEnsemble([(algo, m1, 2.0), (cn, mc)], fusion)
    images = synth.images(4, 128, 128, seed=1).to(dev)
    image_hw = torch.tensor([[375, 500], [500, 333], [128, 128], [97, 200]], device=dev)
    max_det = min(ens.eval_max_det, 8192)
    batches = []
    for i in (0, 2):
        parts = [tail_rows(a._evaluation_rows(m), images[i:i + 2], image_hw[i:i + 2], 0.001) for a, m in members]
        batches.append(compose_members(parts, image_hw[i:i + 2], [2.0, 1.0], fusion, max_det))
    fused, counts = np.concatenate([b[0] for b in batches]), np.concatenate([b[1] for b in batches])
    print("fused rows per image", counts.tolist(), "largest member count", max(int(b[3].max()) for b in batches))
    assert counts.min() >= 2 and all(b[4] == 0 for b in batches)
    voc, coco, n = ground_truths(fused, counts, 6, seed=2)
    t_voc, t_coco, t_n = on(dev, [voc, coco, n])
    capacity = 4 * max_det
    ev, cv = det_eval.DetectionEvaluator(20, ens.eval_max_det, capacity, dev), coco_eval.CocoEvaluator(20, ens.eval_max_det, capacity, dev)
    for j, i in enumerate((0, 2)):
        r, c = on(dev, [batches[j][0], batches[j][1]])
        ev.add_batch(r, c, t_voc[i:i + 2], t_n[i:i + 2], None)
        cv.add_batch(r, c, t_coco[i:i + 2], t_n[i:i + 2], None)
    want_voc, want_coco = ev.results(), cv.results()
    assert want_voc["tp"].sum() > 0 and want_coco["stats"][0] > 0
    torch.cuda.synchronize()
    loader = Loader(images, image_hw=image_hw, gt=t_voc, gt_counts=t_n)
    try:
        res = ens.evaluate_on_voc(str(tmp_path / "voc"), "val", dataloader=loader, capacity=capacity)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loader.flagged, "torch.cuda.set_sync_debug_mode('error') does not flag a read-back on this build"
    same_results(res, want_voc)
    loader = Loader(images, image_hw=image_hw, gt_coco=t_coco, gt_counts=t_n)
    try:
        res = ens.evaluate_on_coco(str(tmp_path / "coco"), "val", dataloader=loader, capacity=capacity)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loader.flagged
    same_results(res, want_coco)
    assert (tmp_path / "coco" / "coco_results.txt").read_text() == cv.summary_text()
