"""CPU: scale and flip test-time augmentation for the detectors, the host side -- the numpy restatement of the two kernels
(tests/det_tta_restatement.py) on hand-derived cases, the view map, what the seeded GPU cases assume about themselves, the validation, the
new symbols and struct, and the surface that needs no GPU.

The hand-derived vote: A = [0, 0, 8, 8] with score 0.5 from view 0 and C = [0, 0, 8, 4] with score 0.25 from view 1, both of class 1, under
the identity map.  IoU = 32 / 64 = 0.5, above the threshold 0.25.  A is kept; its members in sorted order are A itself (weight 0.5) and C
(weight 0.5 * 0.25 = 0.125): Wt = 0.625, X = 0.5 * A + 0.125 * C = [0, 0, 5, 4.5], and the voted box is [0, 0, 8, 4.5 / 0.625 = 7.2] -- every
intermediate is exact in fp32, so the one rounding is the last division's."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import det_tta_restatement as DR
from computervision.pytorch_amd import LIB_PATH, CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import det_eval
from computervision.pytorch_amd import det_tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = [1, 0, 1, 0]
HW = np.array([[20, 20]], np.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def two_views(row0, row1, maps=(IDENTITY, IDENTITY)):
    """one frame, two views with one row each"""
    rows = np.zeros((2, 4, 6), np.float32)
    rows[0, 0], rows[1, 0] = row0, row1
    return rows, np.array([1, 1], np.int32), np.array(maps, np.float32)


A, C = [0, 0, 8, 8, 0.5, 1], [0, 0, 8, 4, 0.25, 1]


# ---- the fusion, by hand ----------------------------------------------------------------------------------------------------------------------
def test_two_views_vote_as_derived():
    rows, counts, vmap = two_views(A, C)
    out, n, source, members, overflow = DR.fuse_views(rows, counts, vmap, HW, 0.25, False, "vote", "max", 5)
    assert n.tolist() == [1] and overflow == 0 and source[0].tolist() == [0, -1, -1, -1, -1] and members[0].tolist() == [2, 0, 0, 0, 0]
    assert np.array_equal(bits(out[0, 0]), bits([0, 0, 8, np.float32(4.5) / np.float32(0.625), 0.5, 1])) and abs(float(out[0, 0, 3]) - 7.2) < 1e-6
    assert not out[0, 1:].any()
    plain = DR.fuse_views(rows, counts, vmap, HW, 0.25, False, "nms", "max", 5)
    assert plain[0][0, 0].tolist() == [0, 0, 8, 8, 0.5, 1] and plain[1].tolist() == [1] and plain[3][0, 0] == 2       # the same members, no vote
    above = DR.fuse_views(rows, counts, vmap, HW, 0.5, False, "vote", "max", 5)                                        # 0.5 > 0.5 is false
    assert above[1].tolist() == [2] and above[3][0, :2].tolist() == [1, 1] and above[0][0, 0].tolist() == [0, 0, 8, 8, 0.5, 1]


def test_other_classes_do_not_vote_unless_agnostic():
    rows, counts, vmap = two_views(A, C[:5] + [2])
    out, n, source, members, _ = DR.fuse_views(rows, counts, vmap, HW, 0.25, False, "vote", "max", 5)
    assert n.tolist() == [2] and source[0, :2].tolist() == [0, 4] and members[0, :2].tolist() == [1, 1]
    assert out[0, 0].tolist() == [0, 0, 8, 8, 0.5, 1] and out[0, 1].tolist() == [0, 0, 8, 4, 0.25, 2]
    out, n, _, members, _ = DR.fuse_views(rows, counts, vmap, HW, 0.25, True, "vote", "max", 5)
    assert n.tolist() == [1] and members[0, 0] == 2 and np.array_equal(bits(out[0, 0, :4]), bits([0, 0, 8, np.float32(4.5) / np.float32(0.625)]))


def test_a_member_before_the_kept_row_votes_too():
    # three views, one row each, sorted D = [0, 4, 8, 8] (0.5), A = [0, 0, 8, 8] (0.25), C = [0, 0, 8, 4] (0.125).  D is kept and removes A
    # (IoU 0.5); C does not touch D and is kept.  A, though removed, is a member of C and lies BEFORE it in sorted order: it votes first
    rows = np.zeros((3, 4, 6), np.float32)
    rows[0, 0], rows[1, 0], rows[2, 0] = [0, 4, 8, 8, 0.5, 1], [0, 0, 8, 8, 0.25, 1], [0, 0, 8, 4, 0.125, 1]
    out, n, _, members, _ = DR.fuse_views(rows, np.array([1, 1, 1], np.int32), np.array([IDENTITY] * 3, np.float32), HW, 0.25, False, "vote", "max", 5)
    assert n.tolist() == [2] and members[0, :2].tolist() == [2, 2]
    wt = np.float32(0.125) + np.float32(0.125)                      # C's vote: A first (0.5 * 0.25), then C itself (0.125)
    want = (np.float32(0.125) * np.array([0, 0, 8, 8], np.float32) + np.float32(0.125) * np.array([0, 0, 8, 4], np.float32)) / wt
    assert want.tolist() == [0, 0, 8, 6] and out[0, 1, :4].tolist() == [0, 0, 8, 6]


@pytest.mark.parametrize("W", [8, 9])
def test_a_flipped_view_comes_back_mirrored(W):
    """an off-centre box [1, 2, 3, 5] of a W-wide picture is [W - 3, 2, W - 1, 5] in the mirrored view; the flipped full-size map is
    a = -1, c = W, and the corners come back in order.  The pixels agree: column 1 of the picture is column W - 2 of the mirrored slot."""
    rows, counts, vmap = two_views([W - 3, 2, W - 1, 5, 0.5, 0], [0, 0, 0, 0, 0, 0], ([-1, W, 1, 0], IDENTITY))
    counts = np.array([1, 0], np.int32)
    out, n, _, _, _ = DR.fuse_views(rows, counts, vmap, np.array([[6, W]], np.int32), 0.5, False, "vote", "max", 3)
    assert n.tolist() == [1] and out[0, 0].tolist() == [1, 2, 3, 5, 0.5, 0]
    img = np.zeros((1, 3, 6, W), np.float32)
    img[..., 1] = 1.0
    slots = DR.tta_inputs(img, [(6, W, 0, 0, False), (6, W, 0, 0, True)])
    assert np.array_equal(slots[0], img[0]) and np.flatnonzero(slots[1, 0, 0]).tolist() == [W - 2]
    # the object's own view map for the mirrored full-size view of an unpadded picture
    vm = T.DetTTA(scales=(1.0,), flips=(True,)).view_map(torch.tensor([[40, 8 * W]]), (40, 8 * W), False)
    assert vm.tolist() == [[-1, 8 * W, 1, 0]]


def test_a_lone_row_keeps_its_bits():
    lone = [0.1, 0.7, 9.3, 7.9, 0.7, 0]
    rows, counts, vmap = two_views(lone, [12, 12, 19, 19, 0.9, 0])
    out, n, _, members, _ = DR.fuse_views(rows, counts, vmap, HW, 0.5, False, "vote", "max", 3)
    assert n.tolist() == [2] and members[0, :2].tolist() == [1, 1]
    assert np.array_equal(bits(out[0, 1]), bits(lone)) and np.array_equal(bits(out[0, 0]), bits([12, 12, 19, 19, 0.9, 0]))
    s = np.float32(0.7)
    assert any((s * np.float32(v)) / s != np.float32(v) for v in lone[:4])          # the quotient would not have kept them


def test_views_scores():
    rows, counts, vmap = two_views(A, C)
    both = DR.fuse_views(rows, counts, vmap, HW, 0.25, False, "vote", "views", 5)
    assert both[0][0, 0, 4] == np.float32(0.5) and both[1].tolist() == [1]                      # m = V = 2
    apart = DR.fuse_views(rows, counts, vmap, HW, 0.5, False, "nms", "views", 5)
    assert apart[0][0, :2, 4].tolist() == [0.25, 0.125] and apart[1].tolist() == [2]            # m = 1 of 2 views: half the score, the order stays
    rows2 = rows.copy()
    rows2[0, 1] = C                                                                             # two members, one view
    same_view = DR.fuse_views(rows2, np.array([2, 0], np.int32), vmap, HW, 0.25, False, "vote", "views", 5)
    assert same_view[3][0, 0] == 2 and same_view[0][0, 0, 4] == np.float32(0.25)


def test_a_bad_count_is_flagged_and_contributes_nothing():
    rows, _, vmap = two_views(A, C)
    for bad in (-1, 5):
        out, n, source, _, overflow = DR.fuse_views(rows, np.array([1, bad], np.int32), vmap, HW, 0.25, False, "vote", "max", 5)
        assert overflow == 1 and n.tolist() == [1] and source[0, 0] == 0 and out[0, 0].tolist() == [0, 0, 8, 8, 0.5, 1]


@pytest.mark.parametrize("extra", [0, 1])
def test_capacity(extra):
    rows, counts, vmap, frame_hw = DR.capacity_case(extra)
    assert counts.sum() == DR.FUSE_CAP + extra and counts.max() <= rows.shape[1]
    out, n, source, members, overflow = DR.fuse_views(rows, counts, vmap, frame_hw, 0.5, False, "vote", "max", 300)
    assert n.tolist() == [0, -1 if extra else 300] and overflow == extra
    if extra:                                                                                   # flagged, never truncated
        assert not out.any() and (source == -1).all() and not members.any()
    else:
        assert (members[1] == 1).all() and (source[1] // 1025 % 2 == 1).all() and (source[1] % 1025 < 1024).all()


# ---- the inputs, by hand ----------------------------------------------------------------------------------------------------------------------
def test_a_view_is_the_resize_inside_the_pad():
    rng = np.random.RandomState(0)
    img = rng.rand(2, 3, 12, 10).astype(np.float32)
    views = [DR.view_rect(12, 10, 12, 10, False), DR.view_rect(12, 10, 6, 5, False), DR.view_rect(12, 10, 6, 5, True)]
    out = DR.tta_inputs(img, views, slots=7)
    assert np.array_equal(bits(out[:2]), bits(img)) and np.isnan(out[6]).all()                  # the identity view; an unnamed slot
    top, left = 3, 2
    assert views[1] == (6, 5, top, left, False)
    inner = out[2:4, :, top:top + 6, left:left + 5]
    # exactly half the size: the taps fall half way between two pixels, lam = 0.5 on both axes -- the mean of a 2 x 2 block, up to rounding
    assert np.allclose(inner, img.reshape(2, 3, 6, 2, 5, 2).mean((3, 5)), atol=1e-6)
    frame = out[2:4].copy()
    frame[:, :, top:top + 6, left:left + 5] = DR.PAD
    assert (frame == DR.PAD).all()
    assert np.array_equal(bits(out[4:6]), bits(out[2:4][..., ::-1]))
    assert (out[4:6, :, top, 10 - left - 5:10 - left] == out[2:4, :, top, left:left + 5][..., ::-1]).all()


# ---- the view map -----------------------------------------------------------------------------------------------------------------------------
def test_the_identity_view_maps_exactly():
    hw = torch.tensor([[375, 500], [333, 97], [1080, 1920], [41, 37]])
    for letterbox in (True, False):
        vm = T.DetTTA(scales=(1.0, 0.83), flips=(False, True)).view_map(hw, (160, 224), letterbox)
        assert vm.shape == (8, 4) and vm.dtype == torch.float32 and vm[:4].tolist() == [[1, 0, 1, 0]] * 4
        assert (vm[4:, 0] < -1).all() and (vm[4:, 2] > 1).all()


def test_the_default_terms_are_the_box_map():
    hw = torch.tensor([[375, 500], [333, 97], [1080, 1920], [41, 37]])
    for letterbox in (True, False):
        terms = torch.stack(T.box_map_terms(hw, (160, 224), letterbox), 1)
        assert terms.dtype == torch.float64 and torch.equal(terms.float(), det_eval.letterbox_box_map(hw, (160, 224), letterbox))


@pytest.mark.parametrize("letterbox", [True, False])
def test_view_map_round_trip(letterbox):
    """A box of the picture pushed forward in float64 -- picture -> network (x / gx + px) -> view (x * s + left) -> mirror (W - x) ->
    reported ((x - px) * gx) -- and brought back through the fp32 map in fp32 (a rounded product, a rounded add) returns within 1e-2 pixel.
    The bound, for coordinates below 4096 and zooms from 0.5 (|a| <= 2; |c| < 3 * 4096 since c = gx * (W - px - left) / s - gx * px is at
    most one mirrored picture width over s plus one offset): one fp32 ulp is at most 2^-11 = 4.9e-4 for values below 8192 and 2^-10 below
    16384.  Rounding x_rep: 2^-12 * |a| <= 4.9e-4; rounding a: 2^-24 relative of |a * x_rep| < 8192, 4.9e-4; the product's rounding 4.9e-4;
    rounding c: at most 2^-11 (half an ulp below 16384), 4.9e-4; the add's rounding, the result below 4096: 2.4e-4.  Together below 2.3e-3,
    and 1e-2 leaves a factor four."""
    H, W = 160, 224
    tta = T.DetTTA(scales=(1.0, 0.83, 0.67, 0.5, 0.91), flips=(False, True, False, True, True))
    sizes = [(375, 499), (333, 97), (1081, 1919), (41, 37), (2999, 4001)]
    hw = torch.tensor(sizes)
    vm = tta.view_map(hw, (H, W), letterbox).numpy()
    px, py, gx, gy = (t.numpy() for t in T.box_map_terms(hw, (H, W), letterbox))
    rng = np.random.RandomState(3)
    worst = 0.0
    for k, ((h, w, flip), (_, _, top, left, _, _)) in enumerate(zip(tta.views((H, W)), T.view_table(tta.views((H, W)), (H, W)).tolist())):
        for b, (ih, iw) in enumerate(sizes):
            x = np.sort(rng.rand(64, 2) * iw, 1)
            y = np.sort(rng.rand(64, 2) * ih, 1)
            xv = (x / gx[b] + px[b]) * (w / W) + left
            yv = (y / gy[b] + py[b]) * (h / H) + top
            if flip:
                xv = (W - xv)[:, ::-1]
            xr, yr = ((xv - px[b]) * gx[b]).astype(np.float32), ((yv - py[b]) * gy[b]).astype(np.float32)
            a = vm[k * len(sizes) + b]
            bx = np.sort((xr * a[0]).astype(np.float32) + a[1], 1)
            by = (yr * a[2]).astype(np.float32) + a[3]
            worst = max(worst, np.abs(bx - x).max(), np.abs(by - y).max())
    print("view_map round trip, letterbox", letterbox, "worst", worst)
    assert worst < 1e-2


def test_the_restatement_states_the_same_map():
    tta = T.DetTTA()
    hw = torch.tensor([[375, 499], [333, 97]])
    H, W = 128, 160
    views = [DR.view_rect(H, W, h, w, f) for h, w, f in tta.views((H, W))]
    want = DR.view_map(views, (H, W), [t.numpy() for t in T.box_map_terms(hw, (H, W), True)])
    assert np.array_equal(bits(tta.view_map(hw, (H, W), True).numpy()), bits(want))


# ---- the seeded cases of the GPU test bite ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("V", [3, 6])
@pytest.mark.parametrize("B", [1, 3])
def test_the_seeded_case_bites(B, V, agnostic):
    rows, counts, vmap = DR.fuse_case(B, V)
    hw = DR.FRAME_HW[:B]
    vote = DR.fuse_views(rows, counts, vmap, hw, 0.5, agnostic, "vote", "views", 300)
    plain = DR.fuse_views(rows, counts, vmap, hw, 0.5, agnostic, "nms", "max", 300)
    assert vote[4] == 0 and np.array_equal(vote[1], plain[1]) and np.array_equal(vote[2], plain[2]) and np.array_equal(vote[3], plain[3])
    alone = np.zeros(B, np.int64)
    for k in range(V):                                              # what each view keeps on its own
        c = np.zeros_like(counts)
        c[k * B:(k + 1) * B] = counts[k * B:(k + 1) * B]
        alone += DR.fuse_views(rows, c, vmap, hw, 0.5, agnostic, "nms", "max", 300)[1]
    for f in range(B):
        n = int(vote[1][f])
        if B > 1 and f == 1:
            assert n == 0
            continue
        assert 2 <= n < alone[f], (n, alone[f])                     # a suppression across views: the union of the views' own results is larger
        several = vote[0][f, :n, 4] > plain[0][f, :n, 4] / V * np.float32(1.5)
        assert several.any() and (vote[3][f, :n] > 1).any()         # a kept row with members from two or more views
        assert (bits(vote[0][f, :n, :4]) != bits(plain[0][f, :n, :4])).any()          # a voted box that differs from its own
    ties = rows[..., 4][np.arange(K := rows.shape[1])[None, :] < counts[:, None]]
    assert len(np.unique(ties)) < len(ties)                         # tied scores: the ordinal decides


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_the_word_cases_reach_the_words_they_name(n):
    rows, counts, vmap = DR.word_case(n)
    assert counts.sum() == n and counts.tolist() == [min(64, max(0, n - 64 * s)) for s in range(3)]
    out = DR.fuse_views(rows, counts, vmap, DR.WORD_FRAME_HW, 0.5, False, "vote", "max", 300)
    assert out[4] == 0 and 1 <= out[1][0] <= n
    if n == 129:                                                    # members on both sides of a word edge
        assert out[3][0].max() > 8


# ---- validation -------------------------------------------------------------------------------------------------------------------------------
def test_det_tta_validates_its_arguments():
    d = T.DetTTA()
    assert (d.scales, d.flips, d.fuse_mode, d.iou, d.score, d.class_agnostic, d.max_det) == ((1.0, 0.83, 0.67), (False, True, False), "vote", None, "max",
                                                                                               False, 300)
    assert d.pad == 128 / 255 and d.n_views == 3 and T.DetTTA([1.0] * 8, [False] * 8).n_views == 8
    for bad in (dict(scales=(1.0,)), dict(scales=(), flips=()), dict(scales=[1.0] * 9, flips=[False] * 9), dict(scales=(1.0, 0.0, 0.5)),
                dict(scales=(1.0, -0.5, 0.5)), dict(scales=(1.0, float("nan"), 0.5)), dict(scales=(1.0, float("inf"), 0.5)), dict(fuse="wbf"),
                dict(score="mean"), dict(iou=1.5), dict(iou=-0.1), dict(max_det=0), dict(max_det=8193), dict(pad=float("nan"))):
        with pytest.raises(ValueError):
            T.DetTTA(**bad)
    with pytest.raises(ValueError, match="predict_tiled"):          # zooms above 1 are refused, with a pointer
        T.DetTTA(scales=(1.0, 1.25, 0.67))
    assert d.views((128, 160)) == [(128, 160, False), (106, 133, True), (86, 107, False)]
    assert T.view_size(64, 0.5) == 32 and T.view_table(d.views((128, 160)), (128, 160)).tolist()[1] == (106, 133, 11, 13, 1, 0)
    with pytest.raises(ValueError):                                 # 31 pixels of content
        T.view_size(62, 0.5)
    with pytest.raises(ValueError):
        d.views((128, 47))
    with pytest.raises(ValueError):
        d.fuse(None, None, None, None)                              # no threshold of its own and none handed in


def test_the_entries_refuse_host_tensors_and_bad_arguments():
    table = T.view_table([(40, 56, False)], (40, 56))
    with pytest.raises(CvxError):                                   # there is no CPU path
        T.tta_inputs(torch.zeros(1, 3, 40, 56), table)
    with pytest.raises(CvxError):
        T.DetTTA().inputs(torch.zeros(1, 3, 64, 64))
    with pytest.raises(CvxError):
        T.fuse_views(torch.zeros(2, 4, 6), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4), torch.ones(1, 2, dtype=torch.int32))
    for bad in ([(41, 56, False)], [(40, 0, False)], [], [(40, 56, False)] * 9):
        with pytest.raises(ValueError):
            T.view_table(bad, (40, 56))


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name, n_args in (("cvx_det_tta_inputs", 9), ("cvx_det_fuse_views", 20)):
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
        assert len(L.PROTOTYPES[name][1]) == n_args
    assert "typedef struct cvx_det_view" in header
    assert L.DET_VIEW_DTYPE.itemsize == 24 and L.DET_VIEW_DTYPE.names == ("h", "w", "top", "left", "flip", "reserved")
    assert [L.DET_VIEW_DTYPE.fields[n][1] for n in L.DET_VIEW_DTYPE.names] == [0, 4, 8, 12, 16, 20]
    assert "\"det_tta.hip\"" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert os.path.exists(os.path.join(ROOT, "computervision.pytorch_amd", "csrc", "det_tta.hip"))


# ---- surface ----------------------------------------------------------------------------------------------------------------------------------
def test_surface_and_defaults(monkeypatch):
    from configs import CenternetConfig, Yolo8DetConfig
    from core.algorithms.base import Detector, FramePredictor
    from core.algorithms.centernet import CenterNetA
    from core.algorithms.yolo_v8 import YOLOv8
    from scripts import detect

    for fn in (Detector.predict_batch, Detector.evaluate_on_voc, Detector.evaluate_on_coco, FramePredictor.detect_frames, detect.detect_frames,
               detect.detect_video):
        assert inspect.signature(fn).parameters["tta"].default is None, fn
    assert "tta" not in inspect.signature(Detector.predict_tiled).parameters

    algo = YOLOv8(Yolo8DetConfig(), "cpu")
    with pytest.raises(CvxError):                                   # no CPU path, with or without augmentation
        algo.predict_batch(None, [], tta=T.DetTTA())
    with pytest.raises(CvxError, match="not built"):                # augmented tiles
        algo.detect_frames(None, [], 2, tiled={}, tta=T.DetTTA())
    with pytest.raises(ValueError):
        algo._augmented(None, "vote")

    # tta=None is the old code path: the class's own callable, untouched, and DetTTA.wrap is never entered
    def no_wrap(*a, **k):
        raise AssertionError("tta=None must not take the augmented path")

    def rows_of(*a, **k):
        raise AssertionError("not called here")

    monkeypatch.setattr(T.DetTTA, "wrap", no_wrap)
    monkeypatch.setattr(algo, "_evaluation_rows", lambda model: rows_of)
    assert algo._augmented("the model", None) is rows_of and algo._augmented("the model", None, 100) is rows_of
    monkeypatch.undo()

    # with one, evaluate_on_voc / evaluate_on_coco hand min(eval_max_det, 8192) on
    seen = []
    monkeypatch.setattr(T.DetTTA, "wrap", lambda self, detector, rows_of, max_det=None: seen.append((detector, max_det)) or rows_of)
    monkeypatch.setattr(algo, "_evaluation_rows", lambda model: rows_of)
    assert algo._augmented("the model", T.DetTTA(), min(algo.eval_max_det, 8192)) is rows_of and seen == [(algo, min(algo.max_det, 8192))]

    # the hook: the class's own map terms; CenterNet's tail undoes a letterbox whatever the configuration says
    hw = torch.tensor([[375, 500]])
    cn = CenterNetA(CenternetConfig(), "cpu")
    cn.letterbox_image = False
    assert torch.equal(torch.stack(cn._box_map_terms(hw, (128, 128))), torch.stack(T.box_map_terms(hw, (128, 128), True)))
    algo.letterbox_image = False
    assert torch.equal(torch.stack(algo._box_map_terms(hw, (128, 128))), torch.stack(T.box_map_terms(hw, (128, 128), False)))
