"""CPU: multi-scale / flip test-time augmentation's host side -- the numpy restatement of the fusion (tests/seg_tta_restatement.py) on
hand-derived strips, the ``view_size`` rule and the validation, the new symbols and struct, and the surface that needs no GPU.

The strips use a 1 x 2 logit level under a 1 x 8 output: scale 2 / 8, so the source coordinate (x + .5) / 4 - .5 clamps to 0 for x = 0, 1,
gives lam = .125, .375, .625, .875 for x = 2 .. 5 and sits on the last feature pixel for x = 6, 7.  A class that is 8 at feature pixel 0 and 0
at pixel 1 therefore reads 8, 8, 7, 5, 3, 1, 0, 0 along the strip, and its mirror image 0, 0, 1, 3, 5, 7, 8, 8 (all exact in fp32)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import render_restatement as RS
import seg_tta_restatement as TR
from computervision.pytorch_amd import LIB_PATH, CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import seg_tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def level(*pixels):
    """rows (1, len(pixels), nc) of a 1 x len(pixels) logit level from one list of class logits per feature pixel"""
    return np.array([pixels], np.float32)


LEFT_RIGHT = (level([8, 0], [0, 8]), 1, 2, False)        # class 0 at the left, class 1 at the right


def test_the_strip_reads_as_derived():
    z = TR.view_logits(LEFT_RIGHT, 2, 1, 8)
    assert z[0, 0, 0].tolist() == [8, 8, 7, 5, 3, 1, 0, 0] and z[0, 1, 0].tolist() == [0, 0, 1, 3, 5, 7, 8, 8]
    assert TR.labels_logits([LEFT_RIGHT], 2, 1, 8).tolist() == [[[0, 0, 0, 0, 1, 1, 1, 1]]]


def test_the_second_view_alone_moves_the_switch():
    # a second view that is 3 for class 0 everywhere (a 1 x 1 level): 11, 11, 10, 8, 6, 4, 3, 3 against 0, 0, 1, 3, 5, 7, 8, 8 -- at x = 4 the
    # first view alone says class 1 (3 < 5), both together class 0 (6 > 5)
    views = [LEFT_RIGHT, (level([3, 0]), 1, 1, False)]
    acc = TR.fuse_logits(views, 2, 1, 8)
    assert acc[0, 0, 0].tolist() == [11, 11, 10, 8, 6, 4, 3, 3] and acc[0, 1, 0].tolist() == [0, 0, 1, 3, 5, 7, 8, 8]
    assert TR.labels_logits(views, 2, 1, 8).tolist() == [[[0, 0, 0, 0, 0, 1, 1, 1]]]
    assert TR.labels_logits(views[::-1], 2, 1, 8).tolist() == [[[0, 0, 0, 0, 0, 1, 1, 1]]]          # exact sums: the order does not matter here


@pytest.mark.parametrize("mode", ["logits", "prob"])
def test_a_mirrored_view_is_read_at_the_mirrored_column(mode):
    fuse = TR.labels_logits if mode == "logits" else (lambda *a: TR.labels_prob(*a)[0])
    flat = (level([0, 0, 0]), 1, 1, False)                       # says nothing: the mirrored view alone decides
    seen = level([0, 8, 0], [0, 0, 8])                           # what the network saw in the MIRRORED picture: class 1 left, class 2 right
    # even width 8: un-mirrored the view reads 1, 1, 1, 1, 2, 2, 2, 2; the picture's column x is the view's column 7 - x
    assert fuse([(seen, 1, 2, False)], 3, 1, 8).tolist() == [[[1, 1, 1, 1, 2, 2, 2, 2]]]
    assert fuse([flat, (seen, 1, 2, True)], 3, 1, 8).tolist() == [[[2, 2, 2, 2, 1, 1, 1, 1]]]
    # odd width 5: scale 2 / 5, lam = 0, .1, .5, .9 and the last pixel; the middle column is a tie (4 against 4) and goes to the lower
    # class whichever way the view is read, so the mirror of 1, 1, 1, 2, 2 is 2, 2, 1, 1, 1 and not 2, 2, 2, 1, 1
    assert fuse([(seen, 1, 2, False)], 3, 1, 5).tolist() == [[[1, 1, 1, 2, 2]]]
    assert fuse([flat, (seen, 1, 2, True)], 3, 1, 5).tolist() == [[[2, 2, 1, 1, 1]]]


def test_equal_logits_give_class_zero_everywhere():
    for value in (0.0, 0.75):
        views = [(np.full((2, 6, 4), value, np.float32), 2, 3, False), (np.full((2, 2, 4), value, np.float32), 1, 2, True)]
        assert not TR.labels_logits(views, 3, 7, 9).any()
        labels, p, margin = TR.labels_prob(views, 3, 7, 9)
        assert not labels.any() and np.allclose(p, 1 / 3) and not margin.any()


def test_one_view_is_the_arg_max_of_the_plain_up_sampling():
    rows = np.random.RandomState(3).standard_normal((2, 5 * 7, 8)).astype(np.float32)
    want = np.stack([RS.argmax_lowest(RS.logits_at_network_size(rows[b], 6, 5, 7, 19, 30), 0) for b in range(2)])
    assert np.array_equal(TR.labels_logits([(rows, 5, 7, False)], 6, 19, 30), want) and np.unique(want).size == 6
    assert np.array_equal(TR.labels_prob([(rows, 5, 7, False)], 6, 19, 30)[0], want)          # the softmax keeps the order of one view
    z = TR.view_logits((rows, 5, 7, True), 6, 19, 30)
    assert np.array_equal(z[1, :, :, ::-1], RS.logits_at_network_size(rows[1], 6, 5, 7, 19, 30))


def test_the_two_modes_can_disagree():
    # one confident view for class 0 (10 against 0) and two mild ones for class 1 (2 against 0): the logits sum to 10 against 4, the
    # probabilities to 1.0000 + .1192 + .1192 = 1.2384 against .0000 + .8808 + .8808 = 1.7616
    views = [(level([10, 0]), 1, 1, False), (level([0, 2]), 1, 1, False), (level([0, 2]), 1, 1, True)]
    assert TR.fuse_logits(views, 2, 2, 3)[0, :, 0, 0].tolist() == [10, 4]
    assert not TR.labels_logits(views, 2, 2, 3).any()
    labels, p, margin = TR.labels_prob(views, 2, 2, 3)
    assert labels.all() and np.allclose(p[0, :, 0, 0], [1.2384 / 3, 1.7616 / 3], atol=2e-5) and np.allclose(margin, (1.7616 - 1.2384) / 3, atol=4e-5)


def test_inputs_restatement_resizes_first_and_mirrors_second():
    x = np.random.RandomState(4).rand(2, 3, 6, 9).astype(np.float32)
    same = TR.tta_inputs(x, 6, 9, True)
    assert np.array_equal(same[:2], x) and np.array_equal(same[2:], x[..., ::-1])              # lam == 0 at every tap: a bit-exact copy
    out = TR.tta_inputs(x, 9, 14, True)
    assert out.shape == (4, 3, 9, 14) and np.array_equal(out[2:], out[:2, ..., ::-1])
    want = torch.nn.functional.interpolate(torch.from_numpy(x), size=(9, 14), mode="bilinear", align_corners=False).numpy()
    assert np.allclose(out[:2], want, atol=1e-6)
    ramp = np.array([[[[0, 8]]]], np.float32)
    assert TR.tta_inputs(ramp, 1, 8, True)[:, 0, 0].tolist() == [[0, 0, 1, 3, 5, 7, 8, 8], [8, 8, 7, 5, 3, 1, 0, 0]]


def test_confusion_skips_targets_outside_the_classes():
    labels = np.array([[[0, 1, 2], [2, 2, 1]]], np.uint8)
    target = np.array([[[0, 1, 1], [2, 255, -100]]], np.int64)
    want = np.zeros((3, 3), np.int64)
    want[0, 0] = want[1, 1] = want[1, 2] = want[2, 2] = 1
    assert np.array_equal(TR.confusion(labels, target, 3), want)


# ---- the view rule and the validation -------------------------------------------------------------------------------------------------------
def test_view_size_rule():
    assert [T.view_size(513, s) for s in (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)] == [257, 385, 513, 641, 770, 898]
    assert (T.view_size(65, 0.75), T.view_size(97, 0.75), T.view_size(65, 1.5), T.view_size(97, 1.5)) == (49, 73, 98, 146)
    assert T.view_size(65, 0.5) == 33 and T.view_size(66, 0.5) == 33
    for n, s in ((64, 0.5), (33, 0.98), (100, 0.3)):                    # 32, 32, 30
        with pytest.raises(ValueError):
            T.view_size(n, s)
    tta = T.SegTTA((0.75, 1.0, 1.5), flip=True)
    assert tta.view_sizes(65, 97) == [(49, 73), (65, 97), (98, 146)] and tta.n_views == 6 and tta.mode == "prob"
    with pytest.raises(ValueError):
        T.SegTTA((0.5, 1.0)).view_sizes(64, 97)


def test_seg_tta_validates_its_arguments():
    assert T.SegTTA().scales == (1.0,) and T.SegTTA().flip is False and T.SegTTA([1, 2], True, "logits").n_views == 4
    assert T.SegTTA([1.0] * 16).n_views == 16 and T.SegTTA([1.0] * 8, flip=True).n_views == 16
    for bad in (dict(scales=[1.0] * 17), dict(scales=[1.0] * 9, flip=True), dict(scales=(1.0, 0.0)), dict(scales=(-0.5,)), dict(scales=()),
                dict(scales=(float("inf"),)), dict(scales=(float("nan"),)), dict(mode="mean"), dict(mode=1)):
        with pytest.raises(ValueError):
            T.SegTTA(**bad)


def test_fuse_refuses_host_tensors_and_bad_arguments():
    view = T.SegView(torch.zeros(2, 6, 4), (2, 3), False)
    good = dict(nc=3, ld=4, out_hw=(7, 9))
    with pytest.raises(CvxError):                                           # there is no CPU path
        T.fuse([view], **good)
    with pytest.raises(CvxError):
        T.tta_inputs(torch.zeros(1, 3, 40, 40), (33, 33))
    with pytest.raises(CvxError):
        T.SegTTA().run(None, torch.zeros(1, 3, 40, 40))
    for bad in (dict(mode="mean"), dict(nc=257, ld=260), dict(nc=0), dict(nc=5), dict(out_hw=(0, 9)), dict(probs=True, mode="logits"),
                dict(targets=torch.zeros(2, 7, 9, dtype=torch.long)), dict(counts=torch.zeros(3, 3, dtype=torch.long)), dict(labels=False)):
        with pytest.raises(ValueError):
            T.fuse([view], **{**good, **bad})
    with pytest.raises(ValueError):
        T.fuse([], **good)
    with pytest.raises(ValueError):
        T.fuse([view] * 17, **good)


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name, n_args in (("cvx_seg_tta_inputs", 10), ("cvx_seg_fuse", 13)):
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
        assert len(L.PROTOTYPES[name][1]) == n_args
    assert "typedef struct cvx_seg_view" in header
    assert L.SEG_VIEW_DTYPE.itemsize == 24 and L.SEG_VIEW_DTYPE.names == ("rows", "lh", "lw", "flip", "reserved")
    assert [L.SEG_VIEW_DTYPE.fields[n][1] for n in L.SEG_VIEW_DTYPE.names] == [0, 8, 12, 16, 20]
    assert "\"seg_tta.hip\"" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert os.path.exists(os.path.join(ROOT, "computervision.pytorch_amd", "csrc", "seg_tta.hip"))


# ---- surface ----------------------------------------------------------------------------------------------------------------------------------
def test_surface_and_defaults(tmp_path, monkeypatch):
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    from core.trainer import segmentation_trainer as ST

    def defaults(fn, names):
        p = inspect.signature(fn).parameters
        return [p[n].default for n in names]

    assert defaults(DeeplabV3PlusA.evaluate_on_voc, ("subset", "dataloader", "scales", "flip", "fuse")) == ["val", None, None, False, "prob"]
    assert defaults(DeeplabV3PlusA.predict_tensor, ("scales", "flip", "fuse")) == [None, False, "prob"]
    assert defaults(DeeplabV3PlusA.predict_labels, ("scales", "flip", "fuse", "probs")) == [(1.0,), False, "prob", False]
    assert defaults(T.SegTTA.__init__, ("scales", "flip", "mode")) == [(1.0,), False, "prob"]
    assert defaults(T.fuse, ("targets", "counts", "probs")) == [None, None, False]
    assert list(inspect.signature(ST.fused_evaluation_tta).parameters) == ["model", "metrics", "dataloader", "device", "tta"]
    algo = DeeplabV3PlusA(DeeplabV3PlusConfig(), "cpu")
    images = torch.zeros(1, 3, 65, 97)
    with pytest.raises(CvxError):                                           # no CPU path
        algo.predict_labels(None, images)
    with pytest.raises(CvxError):
        algo.predict_tensor(None, images, flip=True)
    with pytest.raises(CvxError):
        algo.evaluate_on_voc(None, str(tmp_path), dataloader=[], scales=(0.75, 1.0))
    with pytest.raises(CvxError):
        algo.evaluate_on_voc(None, str(tmp_path), dataloader=[], flip=True)
    with pytest.raises(ValueError):                                         # a bad mode is refused before anything runs
        algo.evaluate_on_voc(None, str(tmp_path), dataloader=[], flip=True, fuse="mean")
    # the defaults still take the old path: the plain fused evaluation, with the criterion
    calls = []

    def plain(model, criterion, metrics, dataloader, device):
        calls.append((model, type(criterion).__name__, dataloader))
        return {"Loss": 0.5, "Overall Acc": 0.1, "Mean Acc": 0.2, "FreqW Acc": 0.3, "Mean IoU": 0.4}

    def tta(*a, **k):
        raise AssertionError("evaluate_on_voc() with its defaults must not take the augmented path")

    monkeypatch.setattr(ST, "fused_evaluation", plain)
    monkeypatch.setattr(ST, "fused_evaluation_tta", tta)
    loader = [object()]
    path = algo.evaluate_on_voc("the model", str(tmp_path), dataloader=loader)
    assert calls == [("the model", "SegLoss", loader)]
    assert open(path, encoding="utf-8").read() == "Overall Acc: 0.1\nMean Acc: 0.2\nFreqW Acc: 0.3\nMean IoU: 0.4"


# ---- what the GPU test of mode 1 assumes about its own inputs -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", TR.PROB_CASES, ids=lambda c: f"nc{c[0]}-ld{c[1]}-{c[2][0]}x{c[2][1]}-k{c[3]}-b{c[4]}")
def test_few_pixels_of_the_seeded_cases_have_a_label_within_rounding(case):
    """tests/test_seg_tta_gpu.py compares mode 1's labels where the float64 top-2 margin exceeds 2e-5 and asserts that less than 1 % of the
    pixels are left out; that is a property of the seeded inputs alone, shown here"""
    nc, ld, out_hw, n_views, batch = case
    views, _ = TR.fuse_case(*case)
    labels, p, margin = TR.labels_prob(views, nc, *out_hw)
    share = float((margin <= TR.MARGIN).mean())
    print(f"{case}: {share * 100:.3f} % of {margin.size} pixels have a margin <= {TR.MARGIN}, classes present {np.unique(labels).size}")
    assert share < 0.01 and np.unique(labels).size == nc and np.allclose(p.sum(1), 1.0, atol=1e-12)
