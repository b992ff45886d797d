"""CPU: the rules of SegLoss's options (class weights, label smoothing, OHEM) -- tests/seg_loss_restatement.py against
F.cross_entropy of the installed torch in float64 -- and the host side of the feature: refusals, config plumbing, seg_class_weights.
The kernels are held against the same restatement in tests/test_seg_loss_opts_gpu.py."""
import copy
import math

import pytest
import torch

import builder
from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd.deeplab import SegLoss, seg_class_weights
import seg_loss_restatement as R

SHAPES = [(2, 9, 12, 33, 45, 21), (1, 5, 6, 40, 48, 5), (2, 33, 33, 33, 33, 19), (3, 17, 12, 65, 45, 5)]
# (shape, seed, min_kept, thresh, valid pixels, kept pixels, pixels within 1e-4 of a threshold)
OHEM_CASES = [
    (SHAPES[0], 11, 200, 0.7, 2519, 2516, 1),
    (SHAPES[0], 11, 200, 1e-4, 2519, 400, 1),
    (SHAPES[1], 12, 100000, 0.7, 1593, 1593, 0),
    (SHAPES[2], 13, 300, 0.02, 1846, 1169, 1),
    (SHAPES[3], 14, 500, 0.3, 7431, 5632, 2),
    (SHAPES[3], 14, 500, 0.01, 7431, 1500, 1),
]


def case_logits(shape, seed):
    rows, t, w = R.make_case(shape, seed)
    return R.upsample(R.low_res_nchw(rows, shape), shape), t, w.double()


def band_count(res, thresh, width=1e-4):
    """valid pixels whose float64 key lies within ``width`` of theta_t or of theta_min (the rank-K pixel itself included)"""
    k = res["keys"][res["valid"]]
    near = (k - R.theta_of(thresh)).abs() <= width
    if math.isfinite(res["theta_min"]):
        near |= (k - res["theta_min"]).abs() <= width
    return int(near.sum())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_is_torchs_cross_entropy(shape, eps, weighted):
    z, t, w = case_logits(shape, shape[0] * 1000 + shape[3] + shape[5])
    w = w if weighted else None
    res = R.criterion(z, t, w, eps)
    loss, grad = R.torch_ce(z, t, w, eps)
    assert abs(float(res["loss"]) - float(loss)) <= 1e-12 * abs(float(loss))
    assert float((res["grad"] - grad).abs().max()) <= 1e-12
    assert bool((res["kept"] == res["valid"]).all())


@pytest.mark.parametrize("case", OHEM_CASES, ids=lambda c: f"{c[0][3]}x{c[0][4]}-k{c[2]}-t{c[3]}")
def test_ohem_is_torchs_call_on_the_kept_pixels(case):
    shape, seed, min_kept, thresh, n_valid, n_kept, n_band = case
    z, t, w = case_logits(shape, seed)
    ohem = dict(thresh=thresh, min_kept=min_kept)
    res = R.criterion(z, t, w, 0.1, ohem)
    K = min_kept * shape[0]
    assert int(res["valid"].sum()) == n_valid and int(res["kept"].sum()) == n_kept
    assert n_kept >= min(K, n_valid) and bool((res["kept"] <= res["valid"]).all())
    assert band_count(res, thresh) == n_band <= 2
    loss, grad = R.torch_ce(z, t, w, 0.1, kept=res["kept"])
    assert abs(float(res["loss"]) - float(loss)) <= 1e-12 * abs(float(loss))
    assert float((res["grad"] - grad).abs().max()) <= 1e-12
    # the choice of pixels does not depend on the weights or the smoothing
    assert bool((R.criterion(z, t, None, 0.0, ohem)["kept"] == res["kept"]).all())
    if n_valid < K:
        assert bool((res["kept"] == res["valid"]).all()) and res["theta_min"] == -math.inf


def test_rank_branch_keeps_exactly_the_k_largest():
    shape, seed, min_kept, thresh = OHEM_CASES[1][:4]
    z, t, w = case_logits(shape, seed)
    res = R.criterion(z, t, None, 0.0, dict(thresh=thresh, min_kept=min_kept))
    by_rank = res["valid"] & (res["keys"] >= res["theta_min"])
    assert int(by_rank.sum()) == min_kept * shape[0] == int(res["kept"].sum())   # no ties in random keys: rank K keeps K
    assert int((by_rank & ~(res["keys"] > R.theta_of(thresh))).sum()) == 396       # kept by the rank alone: target probability >= thresh


def test_constant_logits_keep_every_valid_pixel():
    shape = SHAPES[1]
    _, t, _ = R.make_case(shape, 5)
    z = torch.full((shape[0], shape[5], shape[3], shape[4]), 0.25, dtype=torch.float64)
    res = R.criterion(z, t, None, 0.0, dict(thresh=1e-3, min_kept=10))       # K = 10, every key is ln 5: all tied at rank K
    assert int(res["kept"].sum()) == int(res["valid"].sum()) > 10
    assert abs(float(res["loss"]) - math.log(shape[5])) < 1e-12


def test_no_valid_pixel_gives_nan_and_a_zero_gradient():
    z, t, _ = case_logits(SHAPES[1], 5)
    res = R.criterion(z, torch.full_like(t, -100), None, 0.1, dict(thresh=0.7, min_kept=10))
    assert math.isnan(float(res["loss"])) and float(res["grad"].abs().max()) == 0.0


def test_refusals():
    for kw in (dict(class_weights=[1.0] * 21), dict(label_smoothing=0.1), dict(ohem=dict(thresh=0.7, min_kept=10))):
        with pytest.raises(ValueError):
            SegLoss("focal", **kw)
        SegLoss("ce", **kw)
    for bad in ([1.0, -0.5, 1.0], [1.0, float("nan")], [1.0, float("inf")], [0.0, 0.0, 0.0], []):
        with pytest.raises(ValueError):
            SegLoss("ce", class_weights=bad)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            SegLoss("ce", label_smoothing=bad)
    for bad in (0.0, -0.2, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            SegLoss("ce", ohem=dict(thresh=bad, min_kept=10))
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError):
            SegLoss("ce", ohem=dict(thresh=0.7, min_kept=bad))
    SegLoss("ce", ohem=dict(thresh=1.0, min_kept=1))
    with pytest.raises(ValueError):
        SegLoss("nonsense", label_smoothing=0.1)
    # the length of the weights is checked where the class count is known: at the first call
    crit = SegLoss("ce", class_weights=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        crit.weights_on(torch.device("cpu"), 21)
    assert crit.weights_on(torch.device("cpu"), 3).tolist() == [1.0, 2.0, 3.0]


def test_the_plain_criterion_carries_no_options():
    for kind in ("focal", "ce"):
        crit = SegLoss(kind)
        assert not crit.has_options and crit.class_weights is None and crit.ohem is None and crit.label_smoothing == 0.0
        assert (crit.alpha, crit.gamma, crit.ignore_index) == (0.25, 2.0, -100)
    crit = SegLoss("ce", ohem=dict(thresh=0.7, min_kept=500))
    assert crit.has_options and crit.mode == 1 and crit.ohem == {"thresh": 0.7, "min_kept": 500}
    assert crit.ohem_theta == -math.log(0.7)
    assert math.copysign(1.0, SegLoss("ce", ohem=dict(thresh=1.0, min_kept=1)).ohem_theta) == 1.0     # +0.0: the sign bit would mean "off"
    with pytest.raises(CvxError):
        crit.ohem_keys()                                                    # not called yet


def test_build_loss_reads_the_options_from_cfg_loss():
    cfg, algo_cls, _ = builder.export_from_registry("deeplabv3plus")
    cfg = copy.deepcopy(cfg)
    assert not hasattr(cfg.loss, "class_weights") and not hasattr(cfg.loss, "label_smoothing") and not hasattr(cfg.loss, "ohem")
    assert not algo_cls(cfg, torch.device("cpu")).build_loss().has_options
    cfg.loss.loss_type = "ce"
    cfg.loss.class_weights = [0.5] + [1.0] * 20
    cfg.loss.label_smoothing = 0.1
    cfg.loss.ohem = dict(thresh=0.7, min_kept=1000)
    crit = algo_cls(cfg, torch.device("cpu")).build_loss()
    assert crit.mode == 1 and crit.has_options and crit.label_smoothing == 0.1 and crit.ohem == {"thresh": 0.7, "min_kept": 1000}
    assert crit.class_weights.tolist() == [0.5] + [1.0] * 20
    cfg.loss.loss_type = "focal"
    with pytest.raises(ValueError):
        algo_cls(cfg, torch.device("cpu")).build_loss()                      # options under focal
    cfg.loss.loss_type = "dice"
    with pytest.raises(CvxError):
        algo_cls(cfg, torch.device("cpu")).build_loss()


def test_seg_class_weights():
    counts = [600, 300, 100, 0]                                             # f = 0.6, 0.3, 0.1 among the counted pixels; class 3 never occurs
    w = seg_class_weights(counts, "median_freq")
    assert w.dtype == torch.float32 and w.tolist() == pytest.approx([0.5, 1.0, 3.0, 0.0], rel=1e-6)
    assert seg_class_weights(counts).tolist() == w.tolist()
    assert seg_class_weights([100, 300], "median_freq").tolist() == pytest.approx([2.0, 2.0 / 3.0], rel=1e-6)   # even count: the mean of the middle two
    w = seg_class_weights(counts, "enet")
    assert w.tolist() == pytest.approx([1 / math.log(1.62), 1 / math.log(1.32), 1 / math.log(1.12), 0.0], rel=1e-6)
    SegLoss("ce", class_weights=w)
    with pytest.raises(ValueError):
        seg_class_weights(counts, "inverse")
    with pytest.raises(ValueError):
        seg_class_weights([0, 0, 0])
