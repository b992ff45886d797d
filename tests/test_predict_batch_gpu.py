"""MI355X: batched prediction on the device.  The four launches (``cvx_letterbox_batch_u8_to_nchw``, ``cvx_det_to_image``,
``cvx_draw_detections``, ``cvx_seg_overlay``) against the per-image entry, host ``undo_letterbox`` and the numpy restatement
(tests/render_restatement.py), and ``predict_batch`` / ``detect_frames`` of the five algorithm classes end to end.  Every comparison is
byte- or bit-exact: the rules are integer work or single rounded fp32 operations."""
import numpy as np
import pytest
import torch

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import engine as E
from computervision.pytorch_amd import render as R
from computervision.pytorch_amd.augment import DeviceAugmenter, identity_lut
from computervision.pytorch_amd.det_eval import letterbox_box_map
from core.utils.boxes import undo_letterbox
from core.utils.image_process import images_to_batch
import render_restatement as RS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def pictures(shapes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def on(dev, arrays):
    return [torch.from_numpy(a).to(dev) for a in arrays]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def stretched(frames, hw):
    """the validation loader's tensor for jobs that stretch each picture over the whole canvas (bicubic, / 255)"""
    H, W = hw
    params = [{"jobs": [dict(ih=int(f.shape[0]), iw=int(f.shape[1]), nh=H, nw=W, dx=0, dy=0, flip=0, quad=-1, rect=(0, 0, W, H))],
               "lut": identity_lut()} for f in frames]
    none = [[np.zeros((0, 5), np.float32)] for _ in frames]
    return DeviceAugmenter((H, W), train=False).apply(params, [[f] for f in frames], none, fmt="padded")[0]


# ---- 1. batched letterbox ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap_rb", [False, True])
@pytest.mark.parametrize("letterbox", [True, False])
def test_batched_letterbox_equals_the_per_image_entry(dev, letterbox, swap_rb):
    H, W = 64, 96
    frames = on(dev, pictures([(37, 53), (130, 70), (64, 96), (1, 200), (3, 200)], 1))
    if letterbox:           # 1 x 200 collapses to 0 rows at this size: both entries refuse it; the batch goes on without it
        with pytest.raises(CvxError):
            E.letterbox_u8(frames[3], torch.empty(3, H, W, device=dev), letterbox=True)
        with pytest.raises(CvxError):
            R.letterbox_batch(frames, (H, W), letterbox=True, swap_rb=swap_rb)
        frames = frames[:3] + frames[4:]
    got = R.letterbox_batch(frames, (H, W), letterbox=letterbox, swap_rb=swap_rb)
    want = images_to_batch(frames, (H, W), dev, letterbox=letterbox, swap_rb=swap_rb)
    assert got.shape == want.shape == (len(frames), 3, H, W)
    for i in range(len(frames)):
        assert torch.equal(got[i].view(torch.int32), want[i].view(torch.int32)), i


# ---- 2. rows to image coordinates -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letterbox", [True, False])
def test_det_to_image_equals_host_undo_letterbox(dev, letterbox):
    input_hw, K = (128, 160), 300
    image_hw = np.array([[375, 500], [60, 45], [500, 333], [128, 160]], np.int64)          # up, down, portrait, same size
    rng = np.random.RandomState(3)
    rows = rng.uniform(-20, 180, (4, K, 6)).astype(np.float32)
    rows[..., 4] = rng.uniform(0, 1, (4, K))
    rows[..., 5] = rng.randint(0, 80, (4, K))
    for counts, overflow in (([0, 1, K, 17], 0), ([5, -1, K, 17], 1), ([5, 2, K + 1, -1], 2)):
        counts = np.array(counts, np.int32)
        r, c = on(dev, [rows, counts])
        bm = letterbox_box_map(torch.from_numpy(image_hw).to(dev), input_hw, letterbox)
        out, n, ov = R.det_to_image(r, c, bm)
        out, n, ov = out.cpu().numpy(), n.cpu().numpy(), ov.cpu().numpy()
        good = np.where((counts < 0) | (counts > K), 0, counts)
        assert n.tolist() == good.tolist() and ov.tolist() == [overflow]
        for b in range(4):
            box, conf, cls = undo_letterbox(rows[b, :good[b]], input_hw, image_hw[b], letterbox)
            assert same_bits(out[b, :good[b], :4], box) and same_bits(out[b, :good[b], 4], conf)
            assert np.array_equal(out[b, :good[b], 5].astype(np.int64), cls) and not out[b, good[b]:].any()
    out, n, ov = R.det_to_image(r, c, None)                                               # final boxes: copied
    assert same_bits(out[0, :5].cpu().numpy(), rows[0, :5]) and n.tolist() == [5, 2, 0, 0]


# ---- 3. drawing -------------------------------------------------------------------------------------------------------------------------
def draw_case(h, w, many, seed):
    rng = np.random.RandomState(seed)
    rows = [
        [w + 50, h + 50, w + 90, h + 80, 0.5, 3],             # wholly outside the frame
        [-300, -300, -200, -250, 0.7, 4],                     # outside, with its tag
        [-7.6, -3.2, 12.9, 9.4, 0.99949997, 0],               # negative and fractional coordinates
        [w - 9.5, h - 6.5, w + 30.2, h + 11.9, 0.0625, 19],   # beyond both edges; its tag is cut at the right edge and at the bottom
        [w // 2, 4, w // 2, h - 3, 1.0, 79],                  # x0 == x1
        [20, h - 4, 10, h - 9, 0.9, 5],                       # inverted
        [float("nan"), 2, 9, 9, 0.9, 5],
    ]
    for k in range(5):                                        # mutually overlapping
        rows.append([6 + 3 * k, 8 + 2 * k, w - 12 + 2 * k, h - 14 + 3 * k, 0.25 + 0.1 * k, [0, 19, 79, 7, 250][k]])
    for _ in range(many):
        x, y = rng.uniform(-10, w), rng.uniform(-10, h)
        rows.append([x, y, x + rng.uniform(-2, 40), y + rng.uniform(-2, 40), rng.uniform(0, 1), rng.randint(0, 80)])
    return np.array(rows, np.float32)


@pytest.mark.parametrize("thickness,font_scale", [(2, 2), (1, 1), (3, 1)])
def test_draw_detections_equals_the_restatement(dev, thickness, font_scale):
    shapes = [(37, 53), (64, 64), (130, 70), (40, 40)]
    per_frame = [draw_case(37, 53, 0, 1), draw_case(64, 64, 0, 2), draw_case(130, 70, 300, 3), np.zeros((0, 6), np.float32)]    # the last: no box
    K = max(len(r) for r in per_frame)
    assert K > 256                                             # more than one chunk of the LDS list
    rows = np.zeros((4, K, 6), np.float32)
    for b, r in enumerate(per_frame):
        rows[b, :len(r)] = r
    counts = np.array([len(r) for r in per_frame], np.int32)
    rows[3, :4] = draw_case(40, 40, 0, 4)[7:11]                 # rows past the count are not drawn
    host = pictures(shapes, 5)
    # frame 1: a row stride larger than w * 3 and a multiple of 4 (the dword stores); 53 * 3 and 70 * 3 are not (the byte stores)
    padded = torch.zeros(64, 64 * 3 + 16, dtype=torch.uint8, device=dev)
    frames = on(dev, host)
    frames[1] = padded[:, :64 * 3].view(64, 64, 3)
    frames[1].copy_(torch.from_numpy(host[1]))
    before_pad = padded.clone()
    r, c = on(dev, [rows, counts])
    R.draw_detections(frames, r, c, thickness=thickness, font_scale=font_scale)
    torch.cuda.synchronize()
    for b in range(4):
        want, painted = RS.draw(host[b], rows[b], counts[b], thickness=thickness, font_scale=font_scale)
        got = frames[b].cpu().numpy()
        assert np.array_equal(got[~painted], host[b][~painted]), b       # untouched outside the painted pixels
        assert np.array_equal(got, want), (b, np.argwhere((got != want).any(2))[:5])
        assert painted.any() == (b != 3)
    assert torch.equal(padded[:, 64 * 3:], before_pad[:, 64 * 3:])      # the bytes between the rows


# ---- 4. segmentation overlay ------------------------------------------------------------------------------------------------------------
OVERLAY_TIES = {21: ((5, 11), (20, 3)), 5: ((1, 3), (4, 2)), 3: ((1, 2), (2, 0))}


@pytest.mark.parametrize("nc,ld", [(3, 4), (5, 5), (21, 24)])          # the vector path, the scalar path, the production padding
@pytest.mark.parametrize("bgr", [False, True])
def test_seg_overlay_equals_the_restatement(dev, bgr, nc, ld):
    lh, lw, NH, NW = 9, 9, 33, 33
    (t0, t1), (t2, t3) = OVERLAY_TIES[nc]
    rng = np.random.RandomState(7)
    logits = (rng.randint(-64, 64, (4, lh * lw, ld)) / 8.0).astype(np.float32)
    logits[0, :20, t0] = logits[0, :20, t1] = 9.0              # exact ties between two classes (and with themselves in the mix)
    logits[1, 30:60, :nc] = 1.0                                 # every class ties: class 0
    logits[1, 60:70, t2] = logits[1, 60:70, t3] = 10.0
    logits[2:, :, nc:] = 100.0                                  # the padding columns are not classes
    # up and down from 33 x 33 with row strides 123 and 81 (the byte path); stride 132 (three dwords per thread); a thread with one pixel
    shapes = [(50, 41), (20, 27), (24, 44), (3, 1)]
    host = pictures(shapes, 8)
    host[0][0, :8] = [[0, 1, 2], [3, 4, 5], [128, 129, 130], [131, 255, 254], [7, 6, 5], [64, 65, 66], [67, 192, 193], [194, 195, 0]]
    frames = on(dev, host)
    assert [f.stride(0) % 4 for f in frames[:3]] == [3, 1, 0] and all(f.data_ptr() % 4 == 0 for f in frames)
    lut = R.palette(nc)
    R.seg_overlay(frames, torch.from_numpy(logits).to(dev), nc, (lh, lw), (NH, NW), bgr=bgr)
    torch.cuda.synchronize()
    parities, classes = set(), set()
    for b in range(4):
        want = RS.seg_overlay(host[b], logits[b], nc, lh, lw, NH, NW, lut, bgr=bgr)
        got = frames[b].cpu().numpy()
        assert np.array_equal(got, want), (b, np.argwhere((got != want).any(2))[:5])
        cls = RS.argmax_lowest(RS.logits_at_network_size(logits[b], nc, lh, lw, NH, NW), 0)[RS.nearest_index(shapes[b][0], NH)][:, RS.nearest_index(shapes[b][1], NW)]
        parities |= set(((host[b].astype(int) + lut[cls].astype(int)) % 4).reshape(-1).tolist())
        classes |= set(np.unique(cls).tolist())
        if nc == 21 and b < 2:
            assert len(np.unique(cls)) > 3
    assert parities == {0, 1, 2, 3}
    if nc < 21:
        assert classes == set(range(nc))


# ---- 5. YOLOv8 end to end ---------------------------------------------------------------------------------------------------------------
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
    return cfg, algo, model


FRAME_SHAPES = [(97, 200), (150, 111), (128, 128)]


def triples_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert same_bits(g[0], w[0]) and same_bits(g[1], w[1]) and np.array_equal(g[2], w[2]) and g[2].dtype == np.int64


@pytest.mark.parametrize("letterbox", [True, False])
def test_yolov8_predict_batch_equals_the_per_image_path(dev, yolov8, letterbox):
    from core.algorithms.yolo_v8 import YOLOv8
    cfg, _, model = yolov8
    cfg.decode.letterbox_image = letterbox
    algo = YOLOv8(cfg, dev)
    cfg.decode.letterbox_image = True
    frames = on(dev, pictures(FRAME_SHAPES, 11))
    x = images_to_batch(frames, (128, 128), dev, letterbox=True) if letterbox else stretched(frames, (128, 128))
    with torch.no_grad():
        y = model(x)[0]
    want = [undo_letterbox(r.cpu().numpy(), (128, 128), s, letterbox) for r, s in zip(algo.non_max_suppression(y, 0.001), FRAME_SHAPES)]
    print("YOLOv8-n detections per frame:", [len(w[1]) for w in want])
    assert sum(len(w[1]) for w in want) > 0
    triples_equal(algo.predict_batch(model, frames, conf_threshold=0.001, sync=True), want)
    rows, counts = algo.predict_batch(model, frames, conf_threshold=0.001, sync=False)
    assert rows.is_cuda and counts.tolist() == [len(w[1]) for w in want]


# ---- 6. the other detectors -------------------------------------------------------------------------------------------------------------
def other_detector(name, dev):
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
        return Ssd(cfg, dev), 0.05
    from configs import CenternetConfig
    from core.algorithms.centernet import CenterNetA
    cfg = CenternetConfig()
    cfg.arch.input_size = (3, 128, 128)
    return CenterNetA(cfg, dev), 0.3


@pytest.mark.parametrize("name", ["yolo7", "ssd", "centernet"])
def test_predict_batch_equals_the_evaluation_rows(dev, name):
    """the expectation: the class's own ``_evaluation_rows`` at the same confidence on the batch the per-image helper builds, through host
    ``undo_letterbox`` where the tail hands out a box map (these three tails return final boxes and no map)"""
    algo, conf = other_detector(name, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    input_hw, letterbox = algo._predict_input()
    frames = on(dev, pictures(FRAME_SHAPES, 12))
    x = images_to_batch(frames, input_hw, dev, letterbox=True) if letterbox else stretched(frames, input_hw)
    image_hw = torch.tensor(FRAME_SHAPES, dtype=torch.int32, device=dev)
    rows, counts, box_map = algo._evaluation_rows(model)(x, {"image_hw": image_hw}, conf)
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    print(f"{name}: detections per frame above {conf}: {counts.tolist()}")
    want = []
    for b, n in enumerate(counts):
        r = rows[b, :n]
        want.append(undo_letterbox(r, input_hw, FRAME_SHAPES[b], letterbox) if box_map is not None
                    else (r[:, :4].copy(), r[:, 4].copy(), r[:, 5].astype(np.int64)))
    triples_equal(algo.predict_batch(model, frames, conf_threshold=conf, sync=True), want)


# ---- 7. DeepLab -------------------------------------------------------------------------------------------------------------------------
def test_deeplab_predict_batch_equals_forward_rows_and_the_restatement(dev):
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    cfg = DeeplabV3PlusConfig()
    cfg.arch.input_size, cfg.arch.backbone_pretrained = (3, 97, 129), False
    algo = DeeplabV3PlusA(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    shapes = [(50, 41), (120, 150)]
    host = pictures(shapes, 13)
    frames = on(dev, host)
    with torch.no_grad():
        want_rows = model.forward_rows(stretched(frames, (97, 129))).clone()
    lh, lw = model._last_engine.graph.level_hw[0]
    rows = algo.predict_batch(model, frames, draw=True)
    torch.cuda.synchronize()
    assert torch.equal(rows.view(torch.int32), want_rows.view(torch.int32))
    z = want_rows.cpu().numpy()
    for b in range(2):
        want = RS.seg_overlay(host[b], z[b], algo.num_classes, lh, lw, 97, 129, R.palette(algo.num_classes))
        assert np.array_equal(frames[b].cpu().numpy(), want), b


# ---- 8. no host wait --------------------------------------------------------------------------------------------------------------------
def test_predict_batch_and_detect_frames_do_not_synchronise(dev, yolov8):
    from scripts import detect
    _, algo, model = yolov8
    host = pictures(FRAME_SHAPES + [(64, 90), (33, 47)], 14)
    algo.predict_batch(model, on(dev, host[:3]), conf_threshold=0.001, draw=True, sync=False)      # first use: code objects, palette, engines
    algo.predict_batch(model, on(dev, host[3:]), conf_threshold=0.001, draw=True, sync=False)
    once, video = on(dev, host[:3]), on(dev, host)
    algo.conf_threshold, saved = 0.001, algo.conf_threshold
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=dev).item()
            caught = False
        except RuntimeError:
            caught = True
        if not caught:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a read-back on this build")
        rows, counts = algo.predict_batch(model, once, draw=True, sync=False)
        batches = list(detect.detect_frames(algo, model, iter(video), 3))
    finally:
        torch.cuda.set_sync_debug_mode("default")
        algo.conf_threshold = saved
    torch.cuda.synchronize()
    assert [len(b) for b in batches] == [3, 2] and all(f is v for f, v in zip([f for b in batches for f in b], video))
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    assert counts.sum() > 0
    for b in range(3):
        want, _ = RS.draw(host[b], rows[b], counts[b])
        assert np.array_equal(once[b].cpu().numpy(), want), b
        assert np.array_equal(video[b].cpu().numpy(), want), b         # the same pictures through detect_frames
    clean = on(dev, host[3:])
    r2, c2 = algo.predict_batch(model, clean, conf_threshold=0.001, sync=False)
    for b in range(2):
        want, _ = RS.draw(host[3 + b], r2[b].cpu().numpy(), int(c2[b]))
        assert np.array_equal(video[3 + b].cpu().numpy(), want), b
