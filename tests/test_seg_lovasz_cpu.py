"""The Lovasz-Softmax rules (tests/seg_lovasz_restatement.py) against Berman's formulation written with torch.autograd, answers worked
out by hand, the condition on the inputs of tests/test_seg_lovasz_gpu.py (``order_sensitivity``), and the host side of
``SegLoss(lovasz=)``: the refusals, ``build_loss`` and the C ABI's entries.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import builder
from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd.deeplab import SegLoss, seg_lovasz_defaults
import seg_lovasz_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def jaccard_increments(fg_sorted):
    """The gradient of the Lovasz extension of the Jaccard loss w.r.t. the sorted errors (Berman et al., Algorithm 1)."""
    total = fg_sorted.sum()
    inter = total - fg_sorted.cumsum(0)
    union = total + (1.0 - fg_sorted).cumsum(0)
    jac = 1.0 - inter / union
    return torch.cat([jac[:1], jac[1:] - jac[:-1]])


def autograd_lovasz(logits, target, per_image, skip_absent, weights):
    """Sort, increments, dot product, (weighted) mean over the classes, mean over the groups -- under autograd; (value, d / d logits)."""
    x = logits.double().clone().requires_grad_(True)
    B, C, H, W = x.shape
    # the values are the restatement's bits (pixels with equal logits tie exactly, see softmax_tied), the derivative is torch.softmax's
    p = torch.softmax(x, dim=1)
    p = p + (R.softmax_tied(x.detach()) - p).detach()
    v = torch.ones(C, dtype=torch.float64) if weights is None else torch.as_tensor(weights).double()
    groups = [(p[b:b + 1], target[b:b + 1]) for b in range(B)] if per_image else [(p, target)]
    total = torch.zeros((), dtype=torch.float64)
    for pg, tg in groups:
        valid = ((tg != -100) & (tg >= 0) & (tg < C)).reshape(-1)
        probs = pg.permute(0, 2, 3, 1).reshape(-1, C)[valid]
        labels = tg.reshape(-1)[valid]
        num, den = torch.zeros((), dtype=torch.float64), 0.0
        for c in range(C):
            fg = (labels == c).double()
            if skip_absent and float(fg.sum()) == 0:
                continue
            if labels.numel() == 0:
                den += float(v[c])
                continue
            err = (fg - probs[:, c]).abs()
            es, perm = torch.sort(err, descending=True, stable=True)
            num = num + v[c] * torch.dot(es, jaccard_increments(fg[perm]))
            den += float(v[c])
        if den > 0:
            total = total + num / den
    value = total / len(groups)
    grad = torch.autograd.grad(value, x)[0] if value.requires_grad else torch.zeros_like(x)
    return value.detach(), grad


def full_logits(shape, rows):
    return R.upsample(R.low_res_nchw(rows, shape), shape)


@pytest.mark.parametrize("name", list(R.CONFIGS))
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_against_autograd(shape, name):
    rows, t, w = R.case(shape)
    assert int((t == 2).sum()) == 0 and int((t == 3).sum()) > 0                # one class is absent
    cfg = seg_lovasz_defaults(**R.config(name, w))
    logits = full_logits(shape, rows)
    got = R.lovasz(logits, t, **cfg)
    want_v, want_g = autograd_lovasz(logits, t, cfg["per_image"], cfg["skip_absent"], cfg["class_weights"])
    verr = abs(float(got["value"]) - float(want_v)) / abs(float(want_v))
    gerr = float((got["grad"] - want_g).abs().max() / want_g.abs().max())
    print(f"{name} {shape}: value {float(got['value']):.12f}, relative error {verr:.3g}; gradient relative error {gerr:.3g}")
    assert verr <= 1e-12 and gerr <= 1e-12
    G = shape[0] if cfg["per_image"] else 1
    assert tuple(got["stats"].shape) == (G, shape[5], 4)
    assert float(got["stats"][:, 2, 2].abs().max()) == 0.0                      # Y of the absent class
    assert float(got["stats"][..., 2].sum()) == float(got["valid"].sum())
    assert bool((got["grad"][~got["valid"][:, None].expand_as(got["grad"])] == 0).all())


def test_one_image_fully_ignored():
    shape = R.SHAPES[0]
    rows, t, w = R.case(shape)
    t = t.clone()
    t[1] = -100
    logits = full_logits(shape, rows)
    for per_image in (True, False):
        for skip in (True, False):
            got = R.lovasz(logits, t, per_image=per_image, skip_absent=skip)
            want_v, want_g = autograd_lovasz(logits, t, per_image, skip, None)
            assert abs(float(got["value"]) - float(want_v)) <= 1e-12 * abs(float(want_v))
            assert float((got["grad"] - want_g).abs().max()) <= 1e-12 * float(want_g.abs().max())
            assert float(got["grad"][1].abs().max()) == 0.0
    # under per_image the ignored image contributes 0 and still counts
    both, alone = R.lovasz(logits, t, per_image=True), R.lovasz(logits[:1], t[:1], per_image=True)
    assert abs(float(both["value"]) - 0.5 * float(alone["value"])) < 1e-15
    # no valid pixel at all: value 0, gradient 0
    for skip in (True, False):
        r = R.lovasz(logits, torch.full_like(t, -100), skip_absent=skip)
        assert float(r["value"]) == 0.0 and float(r["grad"].abs().max()) == 0.0


def probs_to_logits(p1):
    """Two classes with p_1 as given: z = (0, logit(p_1))."""
    p1 = torch.tensor(p1, dtype=torch.float64)
    z = torch.zeros(1, 2, 1, p1.numel(), dtype=torch.float64)
    z[0, 1, 0] = torch.log(p1 / (1.0 - p1))
    return z


def test_three_pixels_by_hand():
    """Two classes, three pixels, p_1 = (0.8, 0.4, 0.3), targets (1, 0, 1).

    Class 1: f = (1, 0, 1), e = (0.2, 0.4, 0.7), G = 2.  Sorted: 0.7 (fg), 0.4 (bg), 0.2 (fg).
      k = 0, fg, I = 2, U = 2: Delta = 1/2.   k = 1, bg, I = 1, U = 2: Delta = 1 / (2 * 3) = 1/6.   k = 2, fg, I = 1, U = 3: Delta = 1/3.
      (J = 1/2, 2/3, 1.)   L_1 = 0.7 / 2 + 0.4 / 6 + 0.2 / 3 = 29/60.
    Class 0: f = (0, 1, 0), e = (0.2, 0.4, 0.7), G = 1.  Sorted: 0.7 (bg), 0.4 (fg), 0.2 (bg).
      k = 0, bg, I = 1, U = 1: Delta = 1 / (1 * 2) = 1/2.   k = 1, fg, U = 2: Delta = 1/2.   k = 2, bg, I = 0: Delta = 0.
      L_0 = 0.7 / 2 + 0.4 / 2 = 11/20.
    loss = (29/60 + 11/20) / 2 = 31/60.  h_1 = 1/2 * (-1/3, +1/6, -1/2) and h_0 = 1/2 * (0, -1/2, +1/2) at pixels 0, 1, 2."""
    z, t = probs_to_logits([0.8, 0.4, 0.3]), torch.tensor([[[1, 0, 1]]])
    r = R.lovasz(z, t)
    assert abs(float(r["stats"][0, 1, 3]) - 29 / 60) < 1e-15 and abs(float(r["stats"][0, 0, 3]) - 11 / 20) < 1e-15
    assert r["stats"][0, :, 2].tolist() == [1.0, 2.0]
    assert abs(float(r["value"]) - 31 / 60) < 1e-15
    assert torch.allclose(r["h"][0, 1, 0], torch.tensor([-1 / 6, 1 / 12, -1 / 4], dtype=torch.float64), rtol=0, atol=1e-16)
    assert torch.allclose(r["h"][0, 0, 0], torch.tensor([0.0, -1 / 4, 1 / 4], dtype=torch.float64), rtol=0, atol=1e-16)
    assert r["order"][(0, 1)].tolist() == [2, 1, 0]
    # the class weights enter as a weighted mean: v = (3, 1)
    rw = R.lovasz(z, t, class_weights=[3.0, 1.0])
    assert abs(float(rw["value"]) - (3 * 11 / 20 + 29 / 60) / 4) < 1e-15


def test_a_class_without_a_pixel_costs_its_largest_error():
    """G_c = 0 and skip_absent=False: I = 0 throughout, so only the first element of the order has Delta != 0 (Delta = 1): L_c = max p_c."""
    g = torch.Generator().manual_seed(4)
    z = torch.randn(2, 3, 4, 5, generator=g, dtype=torch.float64)
    t = torch.randint(0, 2, (2, 4, 5), generator=g)
    r = R.lovasz(z, t, skip_absent=False)
    p2 = torch.softmax(z, dim=1)[:, 2]
    assert float(r["stats"][0, 2, 2]) == 0.0 and abs(float(r["stats"][0, 2, 3]) - float(p2.max())) < 1e-15
    where = int(p2.reshape(-1).argmax())
    h2 = r["h"][:, 2].reshape(-1)
    assert abs(float(h2[where]) - 1.0 / 3.0) < 1e-15 and int((h2 != 0).sum()) == 1
    skipped = R.lovasz(z, t)                                                    # skip_absent: the class is left out, of the mean too
    assert float(skipped["stats"][0, 2, 3]) == 0.0 and float(skipped["h"][:, 2].abs().max()) == 0.0
    assert abs(float(skipped["value"]) - float(skipped["stats"][0, :2, 3].mean())) < 1e-15


def test_the_index_rule_decides_a_tie():
    """Two pixels, p_1 = 0.5 at both, targets (1, 0): class 1 has e = (0.5, 0.5) with flags (fg, bg).  Pixel 0 comes first: Delta = (1, 0).
    The other order would give Delta = (1/2, 1/2) -- the same value 0.5 and another gradient.  With the targets swapped the background pixel
    comes first: Delta = (1/2, 1/2)."""
    z = torch.zeros(1, 2, 1, 2, dtype=torch.float64)
    r = R.lovasz(z, torch.tensor([[[1, 0]]]))
    assert r["order"][(0, 1)].tolist() == [0, 1] and float(r["stats"][0, 1, 3]) == 0.5
    assert r["h"][0, 1, 0].tolist() == [-0.5, 0.0]                            # (1/2 classes) * s * Delta
    r = R.lovasz(z, torch.tensor([[[0, 1]]]))
    assert r["order"][(0, 1)].tolist() == [0, 1] and float(r["stats"][0, 1, 3]) == 0.5
    assert r["h"][0, 1, 0].tolist() == [0.25, -0.25]


def test_combination_with_a_base():
    shape = R.SHAPES[1]
    rows, t, w = R.case(shape)
    logits = full_logits(shape, rows)
    lov, base = R.lovasz(logits, t), R.criterion(logits, t)
    v, g = R.combine(base["loss"], base["grad"], lov, weight=0.5, base_weight=2.0)
    assert abs(float(v) - (2.0 * float(base["loss"]) + 0.5 * float(lov["value"]))) < 1e-15
    assert torch.equal(g, 2.0 * base["grad"] + 0.5 * lov["grad"])


CASES = R.gpu_cases()


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if not c[4]])
def test_the_gpu_cases_do_not_hang_on_the_order(name):
    """The gradient is not continuous in the order; the GPU file compares gradients only on inputs where the order taken from fp32 errors
    perturbed by a few ulp moves d / d rows by less than a tenth of its bound."""
    shape, rows, t, w, _ = CASES[name]
    configs = ["batch"] if name == "many" else (["batch", "per_image"] if name == "digits" else list(R.CONFIGS))
    for cname in configs:
        s = R.order_sensitivity(shape, R.config(cname, w), inputs=(rows, t))
        print(f"{name} {cname}: order sensitivity {s:.3g}")
        assert s < 1e-4, (name, cname, s)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[4]])
def test_the_tie_cases_tie_exactly(name):
    """The tie cases are exempt from the condition by construction: at most ten distinct errors per class, the same in fp32 and in float64,
    and the distinct ones far apart -- the index rule decides in both precisions."""
    shape, rows, t, w, _ = CASES[name]
    logits = R.full_logits(shape, rows, tied=True)
    assert float((logits - full_logits(shape, rows)).abs().max()) < 1e-15      # torch's upsampling of the constant, to rounding
    for per_image in (False, True):
        r = R.lovasz(logits, t, per_image=per_image, skip_absent=False)
        for (g, c), e in r["errors"].items():
            d64, d32 = np.unique(e), np.unique(e.astype(np.float32))
            assert len(d64) == len(d32) <= 10, (g, c, len(d64), len(d32))
            assert len(d64) >= (2 if c != 2 else 1) and (len(d64) < 2 or float(np.min(np.diff(d64) / d64[1:])) > 1e-4)   # class 2 is absent
            assert len(e) > 50 * len(d64)                                        # many exact ties


BAD = [dict(sigma=1.0), dict(kind="dice"), dict(weight=0.0), dict(weight=-1.0), dict(base_weight=-0.5), dict(weight=float("nan")),
       dict(base_weight=float("inf")), dict(class_weights=[1.0, -1.0, 1.0]), dict(class_weights=[1.0, float("nan")]),
       dict(class_weights=[0.0, 0.0, 0.0]), dict(alpha=0.5)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_constructor_refusals(bad):
    for loss_type in ("ce", "focal"):
        with pytest.raises(ValueError):
            SegLoss(loss_type, lovasz=bad)
    with pytest.raises(ValueError):
        seg_lovasz_defaults(**bad)


def test_constructor_and_config_surface():
    d = seg_lovasz_defaults()
    assert d == {"weight": 1.0, "base_weight": 1.0, "per_image": False, "skip_absent": True, "class_weights": None}
    assert not SegLoss("ce").has_lovasz and not SegLoss("ce", region=dict(kind="dice")).has_lovasz
    crit = SegLoss("ce", lovasz=dict(weight=0.7, base_weight=0.0, per_image=True))
    assert crit.has_lovasz and not crit.has_region and not crit.has_options and crit.region is None
    assert (crit.lovasz["weight"], crit.lovasz["base_weight"], crit.lovasz["per_image"]) == (0.7, 0.0, True)
    assert SegLoss("focal", lovasz={}).has_lovasz and SegLoss("focal", lovasz={}).mode == 0
    both = SegLoss("ce", class_weights=[1.0, 2.0], label_smoothing=0.1, ohem=dict(thresh=0.7, min_kept=10), lovasz=dict(class_weights=[2.0, 1.0]))
    assert both.has_lovasz and both.has_options and both.lovasz["class_weights"].tolist() == [2.0, 1.0]
    with pytest.raises(ValueError):                                             # the C struct has one selector
        SegLoss("ce", region=dict(kind="dice"), lovasz={})
    with pytest.raises(ValueError):                                             # lovasz is a keyword, not a region kind
        SegLoss("ce", region=dict(kind="lovasz"))
    with pytest.raises(ValueError):
        SegLoss("focal", class_weights=[1.0, 2.0], lovasz={})
    with pytest.raises(CvxError):                                               # no CPU path
        crit.op(torch.zeros(1, 4, 24), torch.zeros(1, 8, 8, dtype=torch.long), (2, 2), 1.0)
    with pytest.raises(CvxError):                                               # nothing to show before the first call
        crit.lovasz_sorted()
    c = crit._criterion_struct(torch.device("cpu"), 21, 4)
    assert (c.region, c.base, c.weight, c.base_weight, c.per_image, c.skip_absent) == (2, 0, 0.7, 0.0, 1, 1)
    assert SegLoss("focal", lovasz={})._criterion_struct(torch.device("cpu"), 21, 4).base == 1


def test_build_loss_reads_the_lovasz_config():
    cfg, algo_cls, _ = builder.export_from_registry("deeplabv3plus")
    assert not hasattr(cfg.loss, "lovasz")
    assert algo_cls(cfg, torch.device("cpu")).build_loss().has_lovasz is False
    cfg.loss.lovasz = dict(weight=0.5, per_image=True)
    crit = algo_cls(cfg, torch.device("cpu")).build_loss()
    assert crit.has_lovasz and (crit.lovasz["weight"], crit.lovasz["per_image"]) == (0.5, True)
    cfg.loss.lovasz = dict(weight=0.0)
    with pytest.raises(ValueError):
        algo_cls(cfg, torch.device("cpu")).build_loss()
    cfg.loss.lovasz = dict()
    cfg.loss.region = dict(kind="dice")
    with pytest.raises(ValueError):
        algo_cls(cfg, torch.device("cpu")).build_loss()


def test_the_new_entry_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(os.environ.get("CVX_LIB", os.path.join(ROOT, "computervision.pytorch_amd", "lib", "libcvx_engine.so")))
    name = "cvx_seg_criterion_lovasz_view"
    assert name in declared and name in L.PROTOTYPES and hasattr(lib, name) and len(L.PROTOTYPES[name][1]) == 3
    assert ctypes.sizeof(L.SegCriterion) == 128 == int(re.search(r"#define CVX_SEG_CRITERION_BYTES (\d+)", header).group(1))
    assert int(re.search(r"#define CVX_ABI_VERSION (\d+)", header).group(1)) == L.ABI_VERSION == 6 == L.load().cvx_abi_version()


def test_workspace_and_refusals_of_the_library():
    lib = L.load()
    B, nc, H, W = 16, 21, 513, 513
    dims = L.SegDims(24, B, nc, 129, 129, H, W)

    def crit(**kw):
        return L.SegCriterion(**dict(dict(ignore_index=-100, ohem_theta=-1.0, region=2, weight=1.0, skip_absent=1), **kw))

    def ws(d, c, for_eval):
        return int(lib.cvx_seg_criterion_workspace_bytes(ctypes.byref(d), ctypes.byref(c), for_eval))

    n = B * nc * H * W
    train, val = ws(dims, crit(base=2, base_weight=1.0), 0), ws(dims, crit(base=2, base_weight=1.0), 1)
    print(f"workspace at batch {B}, {H} x {W}, {nc} classes: training {train / 2 ** 30:.2f} GiB, value only {val / 2 ** 30:.2f} GiB")
    assert 2 * 8 * n + 4 * n < train < 2 * 8 * n + 4 * n + n + 64 * 2 ** 20      # two ping-pong buffers of key + payload, the gradient plane
    assert 2 * 5 * n < val < 2 * 5 * n + n + 64 * 2 ** 20                        # a one-byte payload and no plane
    assert ws(dims, crit(base=0), 0) > 0 and ws(dims, crit(base=0, per_image=1), 0) > 0
    # refused: base_weight that does not fit base, weight 0, more than 1024 classes, a group of 2^31 pixels or more, another selector
    assert ws(dims, crit(base=2), 0) == 0 and ws(dims, crit(base=0, base_weight=1.0), 0) == 0 and ws(dims, crit(base=0, weight=0.0), 0) == 0
    assert ws(L.SegDims(1032, 1, 1025, 2, 2, 4, 4), crit(base=0), 0) == 0
    huge = L.SegDims(8, 2, 2, 8, 8, 32768, 32768)                                # 2 x 2^30 pixels
    assert ws(huge, crit(base=0), 0) == 0 and ws(huge, crit(base=0, per_image=1), 0) > 0
    assert ws(dims, crit(base=0, region=3), 0) == 0
    offs = (ctypes.c_int64 * 3)()
    assert lib.cvx_seg_criterion_lovasz_view(ctypes.byref(dims), ctypes.byref(crit(base=0)), offs) == 0
    assert 0 < offs[2] < offs[0] < offs[1] < train and offs[0] % 256 == 0 and offs[1] - offs[0] >= 4 * n
    assert lib.cvx_seg_criterion_lovasz_view(ctypes.byref(dims), ctypes.byref(crit(base=0, region=1, alpha=0.5, beta=0.5, gamma=1.0)), offs) != 0
    assert math.isfinite(train)
