"""CPU: Weighted Boxes Fusion and the detector ensemble, the host side -- the numpy restatement of the kernel
(tests/box_fusion_restatement.py) on hand-derived cases, what the seeded GPU cases assume about themselves, the validation, the new
symbols, and the surface that needs no GPU.

The hand-derived chain, one class, three sources, weights 1, iou 0.5, the identity map: A = [0, 0, 100, 100] with score 0.9,
B = [25, 0, 125, 100] with 0.8, C = [45, 0, 145, 100] with 0.7.  IoU(A, B) = 75 / 125 = 0.6, so B joins A: sw = 1.7, the fused x1 =
(0.9 * 0 + 0.8 * 25) / 1.7 = 20 / 1.7 = 11.76..., x2 = 100 + 20 / 1.7.  IoU(A, C) = 55 / 145 = 0.379 -- C does not overlap the first box
enough --, but IoU(fused AB, C) = (111.76 - 45) / (145 - 11.76) = 66.76 / 133.24 = 0.501: C joins the evolving box.  One cluster of three,
score ((2.4 / 3) * 3) / 3."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import box_fusion_restatement as BR
import det_tta_restatement as DR
from computervision.pytorch_amd import LIB_PATH, CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import box_fusion as BF
from computervision.pytorch_amd import det_tta as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
HW = np.array([[200, 200]], np.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def one_each(*rows, K=4):
    """one frame, a source per row, the identity map"""
    S = len(rows)
    block = np.zeros((S, K, 6), F32)
    for k, r in enumerate(rows):
        block[k, 0] = r
    return block, np.ones(S, np.int32), np.tile(BR.IDENTITY, (S, 1))


A, B, C = [0, 0, 100, 100, 0.9, 1], [25, 0, 125, 100, 0.8, 1], [45, 0, 145, 100, 0.7, 1]


# ---- the rules, by hand -----------------------------------------------------------------------------------------------------------------------
def test_the_chain_fuses_through_the_evolving_box():
    rows, counts, vmap = one_each(A, B, C)
    out, n, source, members, overflow = BR.fuse_wbf(rows, counts, vmap, HW, iou_thr=0.5)
    assert n.tolist() == [1] and overflow == 0 and source[0, 0] == 0 and members[0, 0] == 3 and (source[0, 1:] == -1).all()
    sw = F32(F32(F32(0.9) + F32(0.8)) + F32(0.7))
    x1 = F32(F32(F32(F32(0.8) * F32(25)) + F32(F32(0.7) * F32(45))) / sw)
    x2 = F32(F32(F32(F32(F32(0.9) * F32(100)) + F32(F32(0.8) * F32(125))) + F32(F32(0.7) * F32(145))) / sw)
    assert bits(out[0, 0, [0, 2]]).tolist() == bits([x1, x2]).tolist() and out[0, 0, 1] == 0
    assert abs(float(out[0, 0, 3]) - 100) < 1e-4 and out[0, 0, 5] == 1
    assert bits(out[0, 0, 4]) == bits(F32(F32(F32(sw / F32(3)) * F32(3)) / F32(3))) and abs(float(out[0, 0, 4]) - 0.8) < 1e-6
    fused_ab = np.array([20 / 1.7, 0, 100 + 20 / 1.7, 100])
    assert abs((fused_ab[2] - 45) / (145 - fused_ab[0]) - 0.501) < 1e-3
    # against each cluster's first box the chain stays split, and so it does under the vote around NMS survivors
    first = BR.fuse_wbf(rows, counts, vmap, HW, iou_thr=0.5, match="first")
    assert first[1].tolist() == [2] and first[3][0, :2].tolist() == [2, 1] and first[2][0, :2].tolist() == [0, 8]
    vote = DR.fuse_views(rows, counts, vmap, HW, 0.5, False, "vote", "max", 300)
    assert vote[1].tolist() == [2]


def test_a_lone_box_keeps_its_bits():
    row = [10.3, 20.7, 50.1, 60.9, 0.37, 4]
    rows, counts, vmap = one_each(row, [0, 0, 0, 0, 0, 0])
    counts = np.array([1, 0], np.int32)
    out, n, source, members, _ = BR.fuse_wbf(rows, counts, vmap, HW)
    assert n.tolist() == [1] and members[0, 0] == 1 and source[0, 0] == 0
    assert bits(out[0, 0, :4]).tolist() == bits(row[:4]).tolist() and out[0, 0, 5] == 4
    assert bits(out[0, 0, 4]) == bits(F32(F32(F32(0.37) * F32(1)) / F32(2)))     # s * min(1, W) / W with W = 2 sources
    plain = BR.fuse_wbf(rows, counts, vmap, HW, rescale=False)[0]
    assert bits(plain[0, 0, 4]) == bits(F32(0.37))


def test_conf_and_rescale():
    rows, counts, vmap = one_each(A, B, C)
    s = [F32(0.9), F32(0.8), F32(0.7)]
    sw = F32(F32(s[0] + s[1]) + s[2])
    got = {(conf, rescale): BR.fuse_wbf(rows, counts, vmap, HW, iou_thr=0.5, conf=conf, rescale=rescale)[0][0, 0, 4]
           for conf in ("avg", "max") for rescale in (False, True)}
    assert bits(got["avg", False]) == bits(F32(sw / F32(3))) and bits(got["max", False]) == bits(s[0])
    assert bits(got["max", True]) == bits(F32(F32(s[0] * F32(3)) / F32(3)))
    # two of three sources agree: the confidence falls by a third
    two = BR.fuse_wbf(*one_each(A, B, [150, 150, 190, 190, 0.7, 1]), HW, iou_thr=0.5, conf="max")
    assert two[1].tolist() == [2] and bits(two[0][0, 0, 4]) == bits(F32(F32(s[0] * F32(2)) / F32(3)))
    assert bits(two[0][0, 1, 4]) == bits(F32(F32(s[2] * F32(1)) / F32(3))) and two[3][0, :2].tolist() == [2, 1]


def test_a_weight_of_two_on_one_source():
    rows, counts, vmap = one_each(A, B)
    out, n, source, members, _ = BR.fuse_wbf(rows, counts, vmap, HW, weights=[1.0, 2.0], iou_thr=0.5)
    # B's weighted score 1.6 leads: it opens the cluster, A joins it
    assert n.tolist() == [1] and source[0, 0] == 4 and members[0, 0] == 2
    sw = F32(F32(1.6) + F32(0.9))
    assert bits(out[0, 0, 0]) == bits(F32(F32(F32(F32(1.6) * F32(25)) + F32(F32(0.9) * F32(0))) / sw))
    assert bits(out[0, 0, 4]) == bits(F32(F32(F32(sw / F32(2)) * F32(2)) / F32(3)))      # m = min(2, W = 3)
    one = BR.fuse_wbf(*one_each(A), HW, weights=[0.5])
    assert bits(one[0][0, 0, 4]) == bits(F32(F32(F32(0.45) * F32(0.5)) / F32(0.5)))      # m = min(1, W = 0.5)


def test_skip_score_and_zero_area():
    rows, counts, vmap = one_each(A, B, C)
    out = BR.fuse_wbf(rows, counts, vmap, HW, iou_thr=0.5, skip_score=0.75)
    assert out[1].tolist() == [1] and out[3][0, 0] == 2                            # C is left out; 0.75 itself would stay
    assert BR.fuse_wbf(rows, counts, vmap, HW, iou_thr=0.5, skip_score=0.8)[3][0, 0] == 2
    flat = BR.fuse_wbf(*one_each(A, [30, 40, 30, 90, 0.95, 1], [30, 40, 80, 40, 0.95, 1], [250, 10, 300, 90, 0.95, 1]), HW, iou_thr=0.5)
    assert flat[1].tolist() == [1] and flat[2][0, 0] == 0 and flat[3][0, 0] == 1   # no width, no height, clamped to no width


def test_a_tie_goes_to_the_older_cluster():
    left, right, mid = [0, 0, 40, 40, 0.9, 0], [20, 0, 60, 40, 0.8, 0], [10, 0, 50, 40, 0.5, 0]      # IoU(left, right) = 1/3; mid: 0.6 with both
    out = BR.fuse_wbf(*one_each(left, right, mid), HW, iou_thr=0.5)
    assert out[1].tolist() == [2] and out[3][0, :2].tolist() == [2, 1] and out[2][0, :2].tolist() == [0, 4]
    out = BR.fuse_wbf(*one_each(right, left, mid), HW, iou_thr=0.5)                 # whichever came first in the walk -- by score -- wins
    assert out[2][0, :2].tolist() == [4, 0] and out[3][0, :2].tolist() == [2, 1]


def test_class_agnostic_merges_across_classes():
    other = [25, 0, 125, 100, 0.8, 3]
    apart = BR.fuse_wbf(*one_each(A, other), HW, iou_thr=0.5)
    assert apart[1].tolist() == [2] and apart[0][0, :2, 5].tolist() == [1, 3]
    merged = BR.fuse_wbf(*one_each(A, other), HW, iou_thr=0.5, class_agnostic=True)
    assert merged[1].tolist() == [1] and merged[3][0, 0] == 2 and merged[0][0, 0, 5] == 1      # the class of the first member


def test_an_empty_frame_a_bad_count_and_max_det():
    rows, counts, vmap = one_each(A, B, C)
    empty = BR.fuse_wbf(rows, np.zeros(3, np.int32), vmap, HW)
    assert empty[1].tolist() == [0] and not empty[0].any() and (empty[2] == -1).all() and not empty[3].any() and empty[4] == 0
    for bad in (-1, 5):
        out = BR.fuse_wbf(rows, np.array([1, bad, 1], np.int32), vmap, HW, iou_thr=0.5)
        assert out[4] == 1 and out[1].tolist() == [2] and out[2][0, :2].tolist() == [0, 8]     # B's slot contributes nothing
    cut = BR.fuse_wbf(*one_each(A, [150, 150, 190, 190, 0.95, 1]), HW, max_det=1)
    assert cut[1].tolist() == [1] and cut[0].shape == (1, 1, 6) and cut[2][0, 0] == 4


@pytest.mark.parametrize("extra", [0, 1])
def test_capacity(extra):
    rows, counts, vmap, frame_hw, weights = BR.capacity_case(extra)
    out = BR.fuse_wbf(rows, counts, vmap, frame_hw, weights, BR.WBF_IOU)
    assert out[1].tolist() == [0, -1 if extra else 300] and out[4] == extra
    if extra:
        assert not out[0].any() and (out[2] == -1).all() and not out[3].any()
    else:
        assert (out[3][1] == 1).all()


# ---- what the seeded GPU cases assume -----------------------------------------------------------------------------------------------------------
def test_the_seeded_cases_bite():
    differs = 0
    for Bn in (1, 3):
        for S in (1, 3, 6):
            rows, counts, vmap, hw, weights = BR.wbf_case(Bn, S)
            out = BR.fuse_wbf(rows, counts, vmap, hw, weights, BR.WBF_IOU)
            assert out[4] == 0 and out[1][0] >= 2 and (Bn == 1 or (out[1][1] == 0 and out[1][2] >= 2))
            assert S == 1 or out[3].max() >= 3
            first = BR.fuse_wbf(rows, counts, vmap, hw, weights, BR.WBF_IOU, match="first")
            differs += any(not np.array_equal(bits(a), bits(b)) for a, b in zip(out[:4], first[:4]))
    assert differs >= 1                                              # the re-matching against the evolving box decides somewhere


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_the_stride_cases_reach_the_lanes_they_name(n):
    args = BR.stride_case("disjoint", n)
    out = BR.fuse_wbf(*args[:4], args[4], BR.WBF_IOU)
    assert out[1].tolist() == [n] and (out[3][0, :n] == 1).all() and out[4] == 0
    args = BR.stride_case("copies", n)
    out = BR.fuse_wbf(*args[:4], args[4], BR.WBF_IOU)
    assert out[1].tolist() == [1] and out[3][0, 0] == n


def test_the_mixed_case_matches_cluster_66():
    args = BR.stride_case("mixed", 0)
    out = BR.fuse_wbf(*args[:4], args[4], BR.WBF_IOU, rescale=False, conf="max")
    assert out[1].tolist() == [70] and out[3][0, :70].tolist() == [1] * 66 + [2] + [1] * 3      # conf max: the clusters stay in score order


@pytest.mark.parametrize("n_classes", [17, 40])
def test_the_class_cases_have_more_segments_than_waves(n_classes):
    rows, counts, vmap, hw, weights = BR.classes_case(n_classes)
    out = BR.fuse_wbf(rows, counts, vmap, hw, weights, BR.WBF_IOU, max_det=300)
    classes = out[0][0, :out[1][0], 5]
    assert len(set(classes.tolist())) == n_classes > 16 and out[3].max() >= 2 and out[4] == 0
    present = sorted(set(classes.tolist()))
    assert max(np.diff(present)) > 1                                 # gaps between the class indices
    valid = np.concatenate([rows[k, :counts[k], 5] for k in range(2)])
    assert min((valid == c).sum() for c in present) == 1             # segments of a single candidate


# ---- validation -------------------------------------------------------------------------------------------------------------------------------
def test_wbf_validates_its_arguments():
    w = BF.WBF()
    assert (w.iou, w.skip_score, w.conf, w.rescale, w.weights, w.class_agnostic, w.max_det) == (0.55, 0.0, "avg", True, None, False, 300)
    assert BF.WBF(weights=[1, 2.5]).weights == (1.0, 2.5) and BF.WBF(weights=torch.tensor([2.0])).weights == (2.0,)
    for bad in (dict(iou=1.5), dict(iou=-0.1), dict(skip_score=-1.0), dict(skip_score=float("nan")), dict(conf="box_and_model_avg"), dict(max_det=0),
                dict(max_det=8193), dict(weights=[]), dict(weights=[1.0] * 33), dict(weights=[1.0, 0.0]), dict(weights=[1.0, -2.0]),
                dict(weights=[float("inf")]), dict(weights=[float("nan")]), dict(weights=[1e-60])):
        with pytest.raises(ValueError):
            BF.WBF(**bad)


def test_det_tta_takes_a_fusion_and_is_otherwise_what_it_was():
    d = T.DetTTA()
    assert d.fusion is None
    assert (d.scales, d.flips, d.fuse_mode, d.iou, d.score, d.class_agnostic, d.max_det) == ((1.0, 0.83, 0.67), (False, True, False), "vote", None, "max",
                                                                                               False, 300)
    assert inspect.signature(T.DetTTA).parameters["fusion"].default is None
    w = BF.WBF(weights=[1, 2, 1])
    assert T.DetTTA(fusion=w).fusion is w and T.DetTTA(fusion=BF.WBF()).fusion.weights is None
    for bad in (dict(fusion="wbf"), dict(fusion=BF.WBF(weights=[1, 2])), dict(fuse="wbf"), dict(fuse="wbf", fusion=BF.WBF())):
        with pytest.raises(ValueError):
            T.DetTTA(**bad)
    with pytest.raises(CvxError):                                   # no threshold is asked for, and there is no CPU path
        T.DetTTA(fusion=w).fuse(torch.zeros(3, 4, 6), torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4), torch.ones(1, 2, dtype=torch.int32))


def test_fuse_wbf_refuses_host_tensors():
    with pytest.raises(CvxError):
        BF.fuse_wbf(torch.zeros(2, 4, 6), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4), torch.ones(1, 2, dtype=torch.int32))


def test_det_ensemble_validates_its_members():
    from configs import CenternetConfig, DeeplabV3PlusConfig, Yolo8DetConfig
    from core.algorithms.centernet import CenterNetA
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    from core.algorithms.yolo_v8 import YOLOv8
    y8, cn = YOLOv8(Yolo8DetConfig(), "cpu"), CenterNetA(CenternetConfig(), "cpu")
    same = CenternetConfig()
    same.dataset.num_classes = y8.num_classes
    cn_same = CenterNetA(same, "cpu")
    ens = BF.DetEnsemble([(y8, "m1"), (y8, "m2", 2.0), (cn_same, "m3")], tta=T.DetTTA())
    assert ens.weights == (1.0, 2.0, 1.0) and isinstance(ens.fusion, BF.WBF) and ens.num_classes == y8.num_classes
    assert ens.eval_max_det == max(y8.eval_max_det, cn_same.eval_max_det)
    bad_lists = [[], [(y8, "m")] * 33, [(y8,)], [(y8, "m", 1.0, 2)], [(y8, "m", 0.0)], [(y8, "m", float("nan"))], [("yolo", "m")],
                 [(DeeplabV3PlusA(DeeplabV3PlusConfig(), "cpu"), "m")]]
    if cn.num_classes != y8.num_classes:
        bad_lists.append([(y8, "m"), (cn, "m")])
    for members in bad_lists:
        with pytest.raises(ValueError):
            BF.DetEnsemble(members)
    for more in (dict(fusion="wbf"), dict(fusion=BF.WBF(weights=[1.0])), dict(tta="vote")):
        with pytest.raises(ValueError):
            BF.DetEnsemble([(y8, "m")], **more)
    with pytest.raises(CvxError):                                   # there is no CPU path
        BF.DetEnsemble([(y8, None)]).predict_batch([])
    with pytest.raises(CvxError):                                   # no dataset is read from disk
        BF.DetEnsemble([(y8, None)]).evaluate_on_voc("out")
    with pytest.raises(ValueError):
        BF.DetEnsemble([(y8, None)]).evaluate_on_voc("out", subset="train", dataloader=[])
    with pytest.raises(ValueError):
        BF.DetEnsemble([(y8, None)]).evaluate_on_coco("out", subset="test", dataloader=[])
    same.arch.input_size = (3, y8._predict_input()[0][0] + 32, y8._predict_input()[0][1])
    other_size = CenterNetA(same, "cpu")
    assert other_size._predict_input() != y8._predict_input()       # the loader's images have one network size
    for evaluate in ("evaluate_on_voc", "evaluate_on_coco"):
        with pytest.raises(ValueError, match="network size"):
            getattr(BF.DetEnsemble([(y8, torch.nn.Identity()), (other_size, torch.nn.Identity())]), evaluate)("out", dataloader=[])
    assert list(inspect.signature(BF.DetEnsemble.predict_batch).parameters)[1:] == ["frames", "conf_threshold", "draw", "sync", "tracker"]
    assert list(inspect.signature(BF.fuse_wbf).parameters) == ["rows", "counts", "view_map", "frame_hw", "weights", "iou", "skip_score", "conf", "rescale",
                                                               "class_agnostic", "max_det", "overflow"]


# ---- ABI --------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name, n_args in (("cvx_det_wbf_workspace_bytes", 1), ("cvx_det_fuse_wbf", 22)):
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
        assert len(L.PROTOTYPES[name][1]) == n_args
    assert "#define CVX_ABI_VERSION 6" in header and L.ABI_VERSION == 6
    assert "\"box_fusion.hip\"" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    source = open(os.path.join(ROOT, "computervision.pytorch_amd", "csrc", "box_fusion.hip")).read()
    assert "#pragma clang fp contract(off)" in source
