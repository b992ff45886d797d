"""MI355X: ``cvx_soft_nms`` against its numpy restatement (tests/soft_nms_restatement.py) -- rows, anchor indices and counts bit for bit,
no tolerance -- and against ``cvx_nms_variant`` itself in hard mode; then the YOLOv8, YOLOv7 and SSD tails with ``cfg.decode.soft_nms`` set.
tests/test_soft_nms_cpu.py shows, from the restatement alone, what each seeded case was built to catch."""
import numpy as np
import pytest
import torch

import eval_tail_cases as T
import soft_nms_restatement as S
from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import det_eval
from computervision.pytorch_amd import engine as E
from computervision.pytorch_amd import soft_nms as SN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check(got, want, max_det):
    """(rows, index, counts) of a launch against the restatement: the kept part bit for bit, zeros behind it"""
    rows, index, counts = (t.cpu().numpy() for t in got)
    assert rows.shape == (len(want), max_det, 6) and index.shape == (len(want), max_det)
    for b, ref in enumerate(want):
        if ref is None:
            assert counts[b] == -1, (b, counts[b])
            assert not rows[b].any() and not index[b].any()
            continue
        k = int(counts[b])
        assert k == len(ref[1]), (b, k, len(ref[1]))
        assert np.array_equal(index[b, :k].astype(np.int64), ref[1]), b
        assert np.array_equal(bits(rows[b, :k]), bits(ref[0])), b
        assert not rows[b, k:].any() and not index[b, k:].any(), b


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in T.nms_cases()])
def test_hard_mode_is_cvx_nms_variant_vanilla(dev, name):
    """method = hard, per class: rows, indices and counts of ``engine.nms(..., variant="vanilla")`` itself, byte for byte -- the overflow
    case (counts = -1) and the corner-box case included"""
    c = T.nms_case(name)
    y = torch.from_numpy(c.pred).to(dev)
    want = E.nms(y, c.conf, c.iou, c.max_det, variant="vanilla", boxes_xyxy=c.xyxy)
    got = E.nms(y, c.conf, c.iou, c.max_det, boxes_xyxy=c.xyxy, soft=SN.SoftNMS("hard"))
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.cpu().numpy().view(np.int32), w.cpu().numpy().view(np.int32))
    assert [int(v) for v in got[2].cpu()] == [-1 if b in c.overflow else len(r[1]) for b, r in enumerate(T.nms_reference(c, "vanilla"))]


@pytest.mark.parametrize("method", ["linear", "gaussian"])
@pytest.mark.parametrize("name", [c.name for c in S.soft_cases()])
def test_soft_sweep(dev, name, method):
    c = S.soft_case(name)
    y = torch.from_numpy(c.pred).to(dev)
    for agnostic in c.agnostic:
        soft = SN.SoftNMS(method, sigma=c.sigma, min_score=c.min_score, class_agnostic=agnostic)
        want = S.soft_reference(c, method, agnostic)
        print(f"{name} {method} agnostic={agnostic}: candidates {c.n}, emitted {[len(r[1]) for r in want]}")
        check(SN.soft_nms(y, c.conf, soft, c.iou, c.max_det), want, c.max_det)


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_max_det_below_at_and_above_the_number_emitted(dev, method, agnostic):
    c = S.soft_case("long_segments_700x3")
    y = torch.from_numpy(c.pred).to(dev)
    emitted = len(S.soft_reference(c, method, agnostic)[0][1])
    assert 7 < emitted < c.max_det
    soft = SN.SoftNMS(method, class_agnostic=agnostic)
    for max_det in (1, 7, emitted - 1, emitted, emitted + 1):
        check(SN.soft_nms(y, c.conf, soft, c.iou, max_det), S.soft_reference(c, method, agnostic, max_det), max_det)


def test_iou_of_soft_nms_overrides_the_callers(dev):
    c = S.soft_case("edge_n129")
    y = torch.from_numpy(c.pred).to(dev)
    got = E.nms(y, c.conf, 0.9, c.max_det, soft=SN.SoftNMS("linear", iou=c.iou))
    check(got, S.soft_reference(c, "linear", False), c.max_det)


def test_overflow_and_corner_boxes(dev):
    """the two front-end paths the clustered cases do not take: more than 16384 candidates (count -1, rows zero, the other block intact)
    and rows 0..3 taken as corners"""
    over = T.nms_case("large_a_overflow")
    y = torch.from_numpy(over.pred).to(dev)
    want = S.soft_nms_restated(over.pred, over.conf, 0.3, 512, "gaussian", overflow=over.overflow)
    check(SN.soft_nms(y, over.conf, SN.SoftNMS("gaussian"), 0.3, 512), want, 512)
    xy = T.nms_case("xyxy_clipped")
    y = torch.from_numpy(xy.pred).to(dev)
    for method in ("linear", "gaussian"):
        want = S.soft_nms_restated(xy.pred, xy.conf, 0.3, 256, method, xyxy=True)
        check(SN.soft_nms(y, xy.conf, SN.SoftNMS(method), 0.3, 256, boxes_xyxy=True), want, 256)


def test_two_calls_give_the_same_bytes(dev):
    c = S.soft_case("mass_ties")
    y = torch.from_numpy(c.pred).to(dev)
    for agnostic in (False, True):
        soft = SN.SoftNMS("gaussian", class_agnostic=agnostic)
        first = [t.cpu().numpy() for t in SN.soft_nms(y, c.conf, soft, c.iou, c.max_det)]
        again = [t.cpu().numpy() for t in SN.soft_nms(y, c.conf, soft, c.iou, c.max_det)]
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(first, again))


def test_the_entry_refuses_bad_arguments(dev):
    lib = E.L.load()
    y = torch.zeros(1, 5, 64, device=dev)
    rows, index, counts = torch.zeros(1, 8, 6, device=dev), torch.zeros(1, 8, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.cvx_soft_nms_workspace_bytes(1, 64)), dtype=torch.uint8, device=dev)

    def call(conf=0.25, iou=0.5, max_det=8, method=2, sigma=0.5, min_score=0.001, flags=0):
        return lib.cvx_soft_nms(E.L.ptr(y), 1, 64, 1, conf, iou, max_det, method, sigma, min_score, flags, E.L.ptr(rows), E.L.ptr(index), E.L.ptr(counts),
                                E.L.ptr(ws), ws.numel(), E.L.stream_ptr(dev))

    assert call() == 0
    for bad in (dict(conf=1.5), dict(iou=-0.1), dict(sigma=0.01), dict(sigma=11.0), dict(min_score=1.0), dict(min_score=-0.1), dict(max_det=0),
                dict(max_det=16385), dict(method=3), dict(method=-1), dict(flags=0x400), dict(flags=3)):
        assert call(**bad) != 0, bad
        with pytest.raises(CvxError):
            E.L.check(call(**bad), "cvx_soft_nms")
    torch.cuda.synchronize()


# ---- 2. the plugin layer -------------------------------------------------------------------------------------------------------------------
class Seen(list):
    pass


@pytest.fixture
def nms_seen(monkeypatch):
    """every ``engine.nms`` call the test makes: (y, conf threshold, keywords)"""
    real, seen = E.nms, Seen()

    def nms(y, conf_thres, *args, **kw):
        seen.append((y, conf_thres, dict(kw)))
        return real(y, conf_thres, *args, **kw)

    monkeypatch.setattr(E, "nms", nms)
    return seen


@pytest.fixture
def soft_calls(monkeypatch):
    """how often ``soft_nms.soft_nms`` (the only caller of ``cvx_soft_nms``) ran"""
    real, calls = SN.soft_nms, []

    def soft_nms(*args, **kw):
        calls.append(1)
        return real(*args, **kw)

    monkeypatch.setattr(SN, "soft_nms", soft_nms)
    return calls


def images(dev, n, hw, seed, mirrored=False):
    """``mirrored``: the second picture is the first one mirrored -- under random weights the scores of unrelated pictures can lie so far
    apart that no one threshold leaves both between 100 and 1000 candidates"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, hw[0], hw[1], generator=g)
    if mirrored:
        x[1] = x[0].flip(-1)
    return x.to(dev)


def threshold_for(scores, inclusive=False):
    """scores (B, N) of the images' anchors -> a confidence threshold that leaves every image between 100 and 1000 candidates, from the
    observed scores (random weights tie many of them): of the values that do -- zero and every score that occurs -- the one that leaves the
    most.  ``inclusive``: a candidate has score >= the threshold (YOLOv7), else > it."""
    B, N = scores.shape
    values = torch.unique(torch.cat((scores.flatten(), scores.new_zeros(1))))
    ascending = torch.sort(scores, 1).values
    n = N - torch.searchsorted(ascending, values.expand(B, -1).contiguous(), right=not inclusive)         # (B, values)
    fits = ((n >= 100) & (n <= 1000)).all(0)
    assert bool(fits.any()), ("no threshold leaves every image between 100 and 1000 candidates; the images' 100th and 1000th largest scores:",
                              torch.sort(scores, 1, descending=True).values[:, [99, 999]].tolist())
    at = int(torch.nonzero(fits)[0])
    conf, n = float(values[at]), n[:, at].tolist()
    assert n == ((scores >= conf) if inclusive else (scores > conf)).sum(1).tolist() and all(100 <= v <= 1000 for v in n), (conf, n)
    return conf, n


def yolov8(dev, soft):
    from configs import Yolo8DetConfig
    from core.algorithms.yolo_v8 import YOLOv8
    cfg = Yolo8DetConfig()
    cfg.dataset.num_classes, cfg.arch.input_size, cfg.decode.soft_nms = 20, (3, 128, 128), soft
    algo = YOLOv8(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for k in [k for k in sd if ".cv3." in k and k.endswith(".2.bias")]:
        sd[k] += 3.0                                           # random-init class biases leave no score above 0.001 (tests/test_det_eval_gpu.py)
    model.load_state_dict(sd)
    return algo, model


def yolov7(dev, soft):
    from configs import Yolo7Config
    from core.algorithms.yolo_v7 import YOLOv7
    cfg = Yolo7Config()
    cfg.arch.input_size, cfg.train.pretrained, cfg.decode.soft_nms = (3, 160, 224), False, soft
    algo = YOLOv7(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    # under the reference's initialisation (weights N(0, 0.02), biases 0) the head rows vanish and every anchor scores sigmoid(0)^2 = 0.25:
    # seeded head biases give every (level, anchor) its own objectness, class and box, and larger head weights let the picture through
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(7)
    heads = [k for k in sd if k.startswith("yolo_head_")]
    assert len(heads) == 6
    for k in heads:
        sd[k] = torch.randn(sd[k].shape, generator=g).to(sd[k]) if k.endswith(".bias") else sd[k] * 1000.0
    model.load_state_dict(sd)
    return algo, model


def ssd(dev, soft):
    from configs import SsdConfig
    from core.algorithms.ssd import Ssd
    cfg = SsdConfig()
    cfg.train.pretrained, cfg.decode.soft_nms = False, soft
    algo = Ssd(cfg, dev)
    torch.manual_seed(0)
    return algo, algo.build_model()[0].to(dev).eval()


@pytest.mark.parametrize("soft", [dict(method="linear"), dict(method="gaussian")], ids=["linear", "gaussian"])
def test_yolov8_tail(dev, nms_seen, soft):
    algo, model = yolov8(dev, soft)
    x = images(dev, 2, (128, 128), 61)
    image_hw = torch.tensor([[200, 300], [128, 128]], dtype=torch.int32, device=dev)
    with torch.no_grad():
        preds = model(x)
    y = preds[0] if isinstance(preds, (list, tuple)) else preds
    conf, n = threshold_for(y[:, 4:].max(1).values)
    expect = SN.SoftNMS(**soft)
    want = S.soft_nms_restated(y.cpu().numpy(), conf, algo.iou_threshold, algo.max_det, expect.method, sigma=expect.sigma, min_score=expect.min_score)
    print(f"YOLOv8-n {soft}: conf {conf:.4f}, candidates {n}, emitted {[len(r[1]) for r in want]}")
    out = algo.non_max_suppression(preds, conf)
    assert all(np.array_equal(bits(o.cpu().numpy()), bits(r[0])) for o, r in zip(out, want))
    rows, counts, box_map = algo._evaluation_rows(model)(x, {"image_hw": image_hw}, conf)
    y_tail = nms_seen[-1][0]                                        # the decode output of that forward
    assert all(isinstance(kw.get("soft"), SN.SoftNMS) and kw["soft"].method == expect.method for _, _, kw in nms_seen) and len(nms_seen) == 2
    want = S.soft_nms_restated(y_tail.cpu().numpy(), conf, algo.iou_threshold, algo.max_det, expect.method, sigma=expect.sigma,
                               min_score=expect.min_score)
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    for b, r in enumerate(want):
        assert counts[b] == len(r[1]) and np.array_equal(bits(rows[b, :counts[b]]), bits(r[0])) and not rows[b, counts[b]:].any()
    assert box_map is not None


@pytest.mark.parametrize("soft", [dict(method="linear"), dict(method="gaussian", class_agnostic=True)], ids=["linear", "gaussian_agnostic"])
def test_yolov7_tail(dev, nms_seen, soft):
    algo, model = yolov7(dev, soft)
    x = images(dev, 2, (160, 224), 62, mirrored=True)
    image_hw = torch.tensor([[200, 300], [160, 224]], dtype=torch.int32, device=dev)
    expect = SN.SoftNMS(**soft)

    def restated(y, conf):
        """the (n, 7) rows nms_device promises: the restatement at the next float below conf (>= conf), classes ascending, then its order"""
        thr = float(np.nextafter(np.float32(conf), np.float32(-1.0)))
        out = []
        for rows, anchors in S.soft_nms_restated(y.cpu().numpy(), thr, algo.nms_threshold, T.NMS_CAP, expect.method, sigma=expect.sigma,
                                                 min_score=expect.min_score, class_agnostic=expect.class_agnostic):
            order = np.argsort(rows[:, 5], kind="stable")
            rows, anchors = rows[order], anchors[order]
            out.append((np.concatenate((rows[:, :5], np.ones((len(rows), 1), np.float32), rows[:, 5:6]), 1), anchors))
        return out

    with torch.no_grad():
        model(x)
    dec, y = algo.decode_rows(model, model.last_rows)
    conf, n = threshold_for(y[:, 4:].max(1).values, inclusive=True)
    want = restated(y, conf)
    print(f"YOLOv7 {soft}: conf {conf:.4f}, candidates {n}, emitted {[len(r[1]) for r in want]}")
    for (det, idx), (rows, anchors) in zip(algo.nms_device(y, dec, conf), want):
        assert np.array_equal(bits(det.cpu().numpy()), bits(rows)) and np.array_equal(idx.cpu().numpy(), anchors)
        assert np.array_equal(bits((det[:, 4] * det[:, 5]).cpu().numpy()), bits(rows[:, 4]))       # obj_conf * class_conf is the decayed score
    del nms_seen[:]
    rows, counts, box_map = algo._evaluation_rows(model)(x, {"image_hw": image_hw}, conf)
    assert box_map is None and nms_seen and all(kw.get("soft") is algo.soft_nms for _, _, kw in nms_seen)
    want = restated(nms_seen[-1][0], conf)
    boxes = torch.zeros(2, rows.shape[1], 4, device=dev)
    for b, (r, _) in enumerate(want):
        boxes[b, :len(r)] = torch.from_numpy(r[:, :4]).to(dev)
    boxes = det_eval.correct_boxes_device(boxes, algo.input_image_size, image_hw, algo.letterbox_image).cpu().numpy()
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    for b, (r, _) in enumerate(want):
        k = int(counts[b])
        assert k == len(r) and np.array_equal(bits(rows[b, :k, :4]), bits(boxes[b, :k]))
        assert np.array_equal(bits(rows[b, :k, 4]), bits(r[:, 4])) and np.array_equal(rows[b, :k, 5], r[:, 6])


@pytest.mark.parametrize("soft", [dict(method="linear"), dict(method="gaussian")], ids=["linear", "gaussian"])
def test_ssd_tail(dev, nms_seen, soft):
    algo, model = ssd(dev, soft)
    x = images(dev, 2, (300, 300), 63, mirrored=True)
    image_hw = torch.tensor([[200, 300], [300, 300]], dtype=torch.int32, device=dev)
    expect = SN.SoftNMS(**soft)
    with torch.no_grad():
        preds = model(x)
    priors = torch.from_numpy(algo.anchors).to(dev)
    boxes, prob = E.ssd_decode(preds[0], preds[1], priors, algo.variance[::2].tolist())
    conf, n = threshold_for(prob[:, :, 1:].reshape(2, -1))
    boxes_h, prob_h = boxes.cpu().numpy(), prob.cpu().numpy()

    def restated(b):
        """classes ascending, each (class, image) block through the restatement: [x1, y1, x2, y2, label, score] and (prior, class column)"""
        det, pairs = [np.zeros((0, 6), np.float32)], [np.zeros((0, 2), np.int64)]
        for c in range(1, algo.num_classes + 1):
            block = np.concatenate((boxes_h[b].T, prob_h[b, :, c][None]), 0)
            rows, anchors = S.soft_nms_image(block, conf, algo.nms_threshold, T.NMS_CAP, expect.method, sigma=expect.sigma, min_score=expect.min_score,
                                             xyxy=True)
            det.append(np.concatenate((rows[:, :4], np.full((len(rows), 1), c - 1, np.float32), rows[:, 4:5]), 1))
            pairs.append(np.stack((anchors, np.full(len(anchors), c, np.int64)), 1))
        return np.concatenate(det), np.concatenate(pairs)

    want = [restated(b) for b in range(2)]
    print(f"SSD {soft}: conf {conf:.4f}, candidates {n}, emitted {[len(w[0]) for w in want]}")
    for (det, pairs), (rows, pr) in zip(algo.decode_device(preds, conf), want):
        assert np.array_equal(bits(det.cpu().numpy()), bits(rows)) and np.array_equal(pairs.cpu().numpy(), pr)
    assert nms_seen and all(kw.get("soft") is algo.soft_nms and kw.get("boxes_xyxy") for _, _, kw in nms_seen)
    rows, counts, box_map = algo._evaluation_rows(model)(x, {"image_hw": image_hw}, conf)
    assert box_map is None
    padded = torch.zeros(2, rows.shape[1], 4, device=dev)
    for b, (r, _) in enumerate(want):
        padded[b, :len(r)] = torch.from_numpy(r[:, :4]).to(dev)
    corrected = det_eval.correct_boxes_device(padded, algo.input_image_size, image_hw, algo.letterbox_image).cpu().numpy()
    rows, counts = rows.cpu().numpy(), counts.cpu().numpy()
    for b, (r, _) in enumerate(want):
        k = int(counts[b])
        assert k == len(r) and np.array_equal(bits(rows[b, :k, :4]), bits(corrected[b, :k]))
        assert np.array_equal(bits(rows[b, :k, 4]), bits(r[:, 5])) and np.array_equal(rows[b, :k, 5], r[:, 4])


def test_refusals(dev):
    from configs import CenternetConfig, SsdConfig
    from core.algorithms.centernet import CenterNetA
    from core.algorithms.ssd import Ssd
    cfg = SsdConfig()
    cfg.decode.soft_nms = dict(method="gaussian", class_agnostic=True)
    with pytest.raises(CvxError, match="class_agnostic"):
        Ssd(cfg, dev)
    cfg = CenternetConfig()
    cfg.decode.soft_nms = dict(method="linear")
    with pytest.raises(CvxError, match="not built for CenterNet"):
        CenterNetA(cfg, dev)


def test_without_the_option_cvx_soft_nms_never_runs(dev, soft_calls, nms_seen):
    for build, hw, conf in ((yolov8, (128, 128), 0.001), (yolov7, (160, 224), 0.2), (ssd, (300, 300), 0.07)):
        algo, model = build(dev, None)
        assert algo.soft_nms is None
        x = images(dev, 1, hw, 64)
        image_hw = torch.tensor([[hw[0], hw[1]]], dtype=torch.int32, device=dev)
        before = len(nms_seen)
        rows, counts, _ = algo._evaluation_rows(model)(x, {"image_hw": image_hw}, conf)
        assert len(nms_seen) > before and int(counts.sum()) > 0, build.__name__
    assert soft_calls == [] and all("soft" not in kw or kw["soft"] is None for _, _, kw in nms_seen)
    E.nms(torch.from_numpy(S.soft_case("edge_n65").pred).to(dev), 0.25, 0.3, 64, soft=SN.SoftNMS("linear"))
    assert soft_calls == [1]                                       # the counter does count
