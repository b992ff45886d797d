"""CPU: Soft-NMS, the host side -- the numpy restatement of ``cvx_soft_nms`` (tests/soft_nms_restatement.py) against the hard-NMS oracle
and on hand-derived cases, what the seeded GPU cases assume about themselves, the mutants, the library's exp(-x), the new symbols, the
validation and the configuration field.

The hand-derived case, one class, iou 0.5, min_score 0.001: A = [0, 0, 100, 100] with score 0.9, B = [0, 0, 100, 50] with 0.8,
C = [0, 25, 100, 75] with 0.7.  IoU(A, B) = 5000 / 10000 = 0.5 exactly -- not above the threshold --, IoU(A, C) = 0.5 likewise, and
IoU(B, C) = 2500 / 7500 = 1/3.
linear: A leaves with 0.9 and decays nothing (0.5 > 0.5 is false); B leaves with 0.8; 1/3 is not above 0.5 either: C leaves with 0.7.
        At iou 0.4 A decays both by 1 - 0.5: B = 0.4, C = 0.35; B leaves second, C third with 0.35 untouched (1/3 is below 0.4).
gaussian, sigma 0.5: A decays both by E(0.25 / 0.5) = E(0.5): B = 0.8 E(0.5), C = 0.7 E(0.5).  B leaves second and decays C by
        E((1/3)^2 / 0.5) = E(2/9): C = (0.7 E(0.5)) E(fl(fl(1/3)^2 / 0.5))."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import eval_tail_cases as T
import soft_nms_restatement as S
from computervision.pytorch_amd import LIB_PATH, CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import soft_nms as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def block(boxes_xyxy, scores, classes, nc=2):
    """corner boxes as one block y (4 + nc, A)"""
    y = np.zeros((4 + nc, len(scores)), F32)
    y[:4] = np.asarray(boxes_xyxy, F32).T
    for a, (s, c) in enumerate(zip(scores, classes)):
        y[4 + c, a] = s
    return y


ABC = block([[0, 0, 100, 100], [0, 0, 100, 50], [0, 25, 100, 75]], [0.9, 0.8, 0.7], [1, 1, 1])


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in T.nms_cases()])
def test_hard_mode_equals_the_vanilla_oracle(name):
    c = T.nms_case(name)
    got = S.soft_nms_restated(c.pred, c.conf, c.iou, c.max_det, "hard", overflow=c.overflow, xyxy=c.xyxy)
    assert T.same_nms(got, T.nms_reference(c, "vanilla"))


def test_three_boxes_linear():
    rows, anchors = S.soft_nms_image(ABC, 0.25, 0.5, 10, "linear", xyxy=True)
    assert anchors.tolist() == [0, 1, 2] and np.array_equal(bits(rows[:, 4]), bits([0.9, 0.8, 0.7]))
    rows, anchors = S.soft_nms_image(ABC, 0.25, 0.4, 10, "linear", xyxy=True)
    half = F32(1.0) - F32(0.5)
    assert anchors.tolist() == [0, 1, 2] and np.array_equal(bits(rows[:, 4]), bits([F32(0.9), F32(0.8) * half, F32(0.7) * half]))
    assert np.array_equal(rows[:, 5], [1, 1, 1]) and np.array_equal(rows[:, :4], ABC[:4].T)
    np.testing.assert_allclose(rows[:, 4], [0.9, 0.4, 0.35], rtol=1e-6)


def test_three_boxes_gaussian():
    rows, anchors = S.soft_nms_image(ABC, 0.25, 0.5, 10, "gaussian", sigma=0.5, xyxy=True)
    e_half = S.exp_neg(F32(0.25) / F32(0.5))
    third = F32(2500) / (F32(5000) + F32(5000) - F32(2500))
    b = F32(0.8) * e_half
    c = (F32(0.7) * e_half) * S.exp_neg((third * third) / F32(0.5))
    assert anchors.tolist() == [0, 1, 2] and np.array_equal(bits(rows[:, 4]), bits([F32(0.9), b, c]))
    np.testing.assert_allclose(rows[:, 4], [0.9, 0.8 * math.exp(-0.5), 0.7 * math.exp(-0.5) * math.exp(-2 / 9)], rtol=2e-6)
    # a decay can change the order: with a tall score on C it overtakes B after A's pick
    y = ABC.copy()
    y[5, 2] = 0.85
    y[5, 1] = 0.8
    rows, anchors = S.soft_nms_image(y, 0.25, 0.5, 10, "gaussian", sigma=0.5, xyxy=True)
    assert anchors.tolist() == [0, 2, 1]


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("name", ["long_segments_700x3", "mass_ties", "duplicate_box"])
def test_linear_at_iou_1_returns_every_candidate_untouched(name, agnostic):
    c = S.soft_case(name)
    for x in c.pred:
        rows, anchors = S.soft_nms_image(x, c.conf, 1.0, T.NMS_CAP, "linear", class_agnostic=agnostic)
        box, sc, cls, cand = T._candidates(x, c.conf, False)
        assert np.array_equal(anchors, cand) and np.array_equal(bits(rows[:, 4]), bits(sc)) and np.array_equal(bits(rows[:, :4]), bits(box))


@pytest.mark.parametrize("method", ["linear", "gaussian"])
@pytest.mark.parametrize("name", [c.name for c in S.soft_cases()])
def test_a_segments_emissions_never_increase(name, method):
    c = S.soft_case(name)
    for agnostic in c.agnostic:
        for x in c.pred:
            stats = []
            rows, _ = S.soft_nms_image(x, c.conf, c.iou, c.max_det, method, sigma=c.sigma, min_score=c.min_score, class_agnostic=agnostic, stats=stats)
            assert all(bool((s["finals"][:-1] >= s["finals"][1:]).all()) for s in stats)
            assert bool((rows[:-1, 4] >= rows[1:, 4]).all()) and bool((rows[:, 4] > F32(c.min_score)).all())
            assert sum(s["emitted"] for s in stats) == len(rows)


# ---- what the seeded cases assume about themselves -----------------------------------------------------------------------------------------
def stats_of(c, method, agnostic, b=0):
    stats = []
    S.soft_nms_image(c.pred[b], c.conf, c.iou, c.max_det, method, sigma=c.sigma, min_score=c.min_score, class_agnostic=agnostic, stats=stats)
    return stats


def test_the_cases_are_what_their_names_say():
    names = {c.name for c in S.soft_cases()}
    assert {f"edge_n{n}" for n in (0, 1, 63, 64, 65, 129)} <= names
    assert S.soft_case("mixed_batch").n == (0, 1, 64, 700, 65)
    long = S.soft_case("long_segments_700x3")
    assert [s["length"] > 64 for s in stats_of(long, "linear", False)] == [True] * 3
    many = stats_of(S.soft_case("classes_300x40_of_80"), "gaussian", False)
    assert len(many) == 40 > 16 and S.soft_case("classes_300x40_of_80").pred.shape[1] == 84
    best = S.soft_case("classes_300x40_of_80").pred[0, 4:].max(1)
    assert int((best > 0.25).sum()) == 40 and not (best[1::2] > 0.25).any()           # every second class is empty
    ties = S.soft_case("mass_ties")
    sc = T._candidates(ties.pred[0], ties.conf, False)[1]
    assert len(np.unique(sc)) <= 8 and len(sc) == 900
    assert S.soft_case("agnostic_3000").n == (3000,) and S.soft_case("agnostic_3000").agnostic == (True,)
    assert {S.soft_case("sigma_0.05").sigma, S.soft_case("sigma_10").sigma} == {0.05, 10.0}


@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_most_candidates_are_decayed_several_times(method):
    """in the long cases; the clusters are tight enough (and iou = 0.3 low enough for linear)"""
    for name, agnostic in (("long_segments_700x3", False), ("long_segments_700x3", True), ("mass_ties", False), ("agnostic_3000", True)):
        decays = np.concatenate([s["decays"] for s in stats_of(S.soft_case(name), method, agnostic)])
        assert np.median(decays) >= 2, (name, agnostic, float(np.median(decays)))


def test_the_duplicate_is_decayed_to_zero_and_dropped_by_linear():
    c = S.soft_case("duplicate_box")
    _, i0, i1 = S.with_duplicate(T.clustered(515, 130, 3, 100))
    assert np.array_equal(c.pred[0, :4, i0], c.pred[0, :4, i1])
    for agnostic in (False, True):
        anchors = S.soft_reference(c, "linear", agnostic)[0][1]
        assert i0 in anchors and i1 not in anchors and len(anchors) == 99
        assert i1 in S.soft_reference(c, "gaussian", agnostic)[0][1]               # E(1 / sigma) > 0: the Gaussian keeps it


@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_min_score_stops_some_segments_early(method):
    c = S.soft_case("min_score_0.3")
    stats = stats_of(c, method, False)
    assert len(stats) == 6 and sum(s["left"] > 0 for s in stats) >= 2 and all(s["emitted"] > 0 for s in stats)
    rows = S.soft_reference(c, method, False)[0][0]
    assert 0 < len(rows) < 700 and bool((rows[:, 4] > F32(0.3)).all())


def test_sigma_at_its_ends_changes_the_result():
    lo, hi = S.soft_case("sigma_0.05"), S.soft_case("sigma_10")
    assert np.array_equal(lo.pred, hi.pred)
    assert not S.same(S.soft_reference(lo, "gaussian", False), S.soft_reference(hi, "gaussian", False))
    assert len(S.soft_reference(lo, "gaussian", False)[0][1]) < len(S.soft_reference(hi, "gaussian", False)[0][1]) == 300


# ---- the mutants: (switch, case, method, class_agnostic) -- each changes the expected output of the case it names ---------------------------
MUTANTS = (
    ("tie_high", "mass_ties", "gaussian", False),
    ("ge_iou", "duplicate_box_iou_1", "linear", False),      # at iou = 1.0 only the exact duplicate sits on the threshold
    ("cross_class", "long_segments_700x3", "gaussian", False),
    ("no_merge", "classes_300x40_of_80", "linear", False),
    ("ge_min", "min_score_exact", "linear", False),
    ("twice", "edge_n129", "gaussian", False),
)


@pytest.mark.parametrize("switch,name,method,agnostic", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_each_mutant_changes_a_case(switch, name, method, agnostic):
    c = S.soft_case(name)
    kw = dict(sigma=c.sigma, min_score=c.min_score, class_agnostic=agnostic)
    good = S.soft_reference(c, method, agnostic)
    bad = S.soft_nms_restated(c.pred, c.conf, c.iou, c.max_det, method, **kw, **{switch: True})
    assert not S.same(good, bad), switch
    if switch == "ge_iou":
        assert len(good[0][1]) == 100 and len(bad[0][1]) == 99
    if switch == "ge_min":      # B decays to 0.8f * 0.5f, and min_score is that very float: not above it, so the segment stops behind A
        assert good[0][1].tolist() == [0] and bad[0][1].tolist() == [0, 1]


def test_the_hand_case_is_the_seeded_one():
    c = S.soft_case("min_score_exact")
    assert np.array_equal(T._candidates(c.pred[0], c.conf, False)[0], ABC[:4].T) and c.min_score == float(F32(0.8) * F32(0.5))


# ---- E(x) ----------------------------------------------------------------------------------------------------------------------------------------
def test_exp_neg_is_within_1e_6_of_exp():
    """1e-6 is derived: the degree-6 Taylor polynomial on |r| <= ln2 / 2 truncates near 1e-7 relative, and six rounded multiply-add pairs
    and the reduction add a few steps of 6e-8"""
    x = np.linspace(0.0, 20.0, 100000).astype(F32)
    got = S.exp_neg(x).astype(np.float64)
    want = np.array([math.exp(-float(v)) for v in x])
    rel = np.abs(got - want) / want
    print("E(x): largest relative error on [0, 20]:", float(rel.max()))
    assert rel.max() < 1e-6
    assert S.exp_neg(F32(0)) == F32(1) and S.exp_neg(F32(80)) == 0 and S.exp_neg(F32(np.inf)) == 0 and S.exp_neg(F32(79.9)) > 0
    assert bool((np.diff(got) <= 0).all())


# ---- ABI, validation, configuration ----------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name, n_args in (("cvx_soft_nms_workspace_bytes", 2), ("cvx_soft_nms", 17)):
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
        assert len(L.PROTOTYPES[name][1]) == n_args
        args = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(args.split(",")) == n_args
    assert "\"soft_nms.hip\"" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    for text in ("CVX_SOFT_NMS_HARD = 0", "CVX_SOFT_NMS_LINEAR = 1", "CVX_SOFT_NMS_GAUSSIAN = 2", "#define CVX_SOFT_NMS_CLASS_AGNOSTIC 0x200"):
        assert text in header
    assert SN.METHODS == {"hard": 0, "linear": 1, "gaussian": 2} and SN.FLAG_CLASS_AGNOSTIC == 0x200 and SN.FLAG_BOXES_XYXY == 0x100


def test_soft_nms_validates_its_arguments():
    d = SN.SoftNMS()
    assert (d.method, d.sigma, d.iou, d.min_score, d.class_agnostic) == ("gaussian", 0.5, None, 0.001, False)
    for bad in (dict(method="soft"), dict(method=1), dict(sigma=0.01), dict(sigma=10.5), dict(sigma=float("nan")), dict(sigma="0.5"), dict(iou=-0.1),
                dict(iou=1.1), dict(iou=float("nan")), dict(min_score=1.0), dict(min_score=-0.001), dict(min_score=float("nan"))):
        with pytest.raises(ValueError):
            SN.SoftNMS(**bad)
    for good in (dict(sigma=0.05), dict(sigma=10), dict(iou=0.0), dict(iou=1), dict(min_score=0), dict(method="hard"), dict(method="linear", class_agnostic=1)):
        SN.SoftNMS(**good)
    assert SN.SoftNMS.of(None) is None and SN.SoftNMS.of(d) is d and SN.SoftNMS.of(dict(method="linear", iou=0.4)).iou == 0.4
    for bad in ("gaussian", 1, dict(methods="linear")):
        with pytest.raises((ValueError, TypeError)):
            SN.SoftNMS.of(bad)
    with pytest.raises(CvxError):                                   # there is no CPU path
        SN.soft_nms(torch.zeros(1, 6, 10), 0.25, d, 0.5)
    from computervision.pytorch_amd import engine as E
    with pytest.raises(CvxError):
        E.nms(torch.zeros(1, 6, 10), 0.25, 0.5, soft=d)


def test_the_field_defaults_to_none_and_reaches_the_wrappers():
    from configs import CenternetConfig, SsdConfig, Yolo7Config, Yolo8DetConfig
    from core.algorithms.centernet import CenterNetA
    from core.algorithms.ssd import Ssd
    from core.algorithms.yolo_v7 import YOLOv7
    from core.algorithms.yolo_v8 import YOLOv8
    for config, algo in ((Yolo8DetConfig, YOLOv8), (Yolo7Config, YOLOv7), (SsdConfig, Ssd)):
        cfg = config()
        assert cfg.decode.soft_nms is None and algo(cfg, "cpu").soft_nms is None
        cfg.decode.soft_nms = dict(method="linear", iou=0.4)
        got = algo(cfg, "cpu").soft_nms
        assert isinstance(got, SN.SoftNMS) and (got.method, got.iou) == ("linear", 0.4)
        cfg.decode.soft_nms = SN.SoftNMS("gaussian", sigma=2.0)
        assert algo(cfg, "cpu").soft_nms is cfg.decode.soft_nms
        cfg.decode.soft_nms = dict(method="soft")
        with pytest.raises(ValueError):
            algo(cfg, "cpu")
        del cfg.decode.soft_nms                                         # a configuration from before the field
        assert algo(cfg, "cpu").soft_nms is None
    cfg = SsdConfig()
    cfg.decode.soft_nms = dict(class_agnostic=True)
    with pytest.raises(CvxError, match="class_agnostic"):
        Ssd(cfg, "cpu")
    cfg = CenternetConfig()
    CenterNetA(cfg, "cpu")
    cfg.decode.soft_nms = dict(method="linear")
    with pytest.raises(CvxError, match="not built for CenterNet"):
        CenterNetA(cfg, "cpu")
