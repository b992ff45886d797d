"""MI355X: the region term of ``cvx_seg_criterion_loss`` (csrc/loss_seg.hip) -- Dice / Tversky / focal-Tversky region losses in the fused criterion
chain -- through ``SegLoss(region=)``: against torch float64 (tests/seg_region_restatement.py, which tests/test_seg_region_cpu.py holds
against autograd to 1e-12 on these inputs; the adjoint of the upsampling is torch's), against the existing entries by composition,
bit repeatability, the bad-label flag, the fused validation pass and ``SegTrainStep`` end to end.

Bounds: the project's.  Value 2e-5 relative; gradient 1e-3 relative in the max norm (one fp16 rounding of the scaled gradient);
``region_stats``: Y exact, I, P, T 1e-6 relative, element by element.  Every test prints what it measured."""
import contextlib
import math

import numpy as np
import pytest
import torch

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd.deeplab import SegLoss
import seg_region_restatement as R

pytestmark = pytest.mark.gpu

SCALE = 65536.0
TINY = (1, 3, 3, 7, 5, 2)
# OHEM_CASES[3] and [1] of tests/test_seg_loss_opts_gpu.py: (shape, seed, min_kept, thresh); both drop valid pixels
OHEM_IDENTITY = (R.SHAPES[2], 13, 300, 0.02)
OHEM_UPSAMPLED = (R.SHAPES[0], 11, 200, 1e-4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


_CASES, _REFS = {}, {}


def inputs(shape):
    if shape not in _CASES:
        if shape == TINY:
            g = torch.Generator().manual_seed(1)
            rows = torch.zeros(1, 9, 8)
            rows[..., :2] = torch.randn(1, 9, 2, generator=g) * 2
            t = torch.randint(0, 2, (1, 7, 5), generator=g)
            t[0, 0, 0] = -100
            _CASES[shape] = (rows, t, torch.tensor([0.5, 1.5]))
        else:
            _CASES[shape] = R.case(shape)
    return _CASES[shape]


def reference(shape, name):
    """float64, computed once per (shape, configuration): the region term alone and CE + region, each as (value, d / d rows), and the
    statistics."""
    if (shape, name) not in _REFS:
        rows, t, w = inputs(shape)
        logits = R.upsample(R.low_res_nchw(rows, shape), shape)
        reg = R.region(logits, t, **R.config(name, w))
        base = R.criterion(logits, t)
        both = R.combine(base["loss"], base["grad"], reg)
        _REFS[(shape, name)] = {"alone": (float(reg["value"]), R.to_rows_grad(reg["grad"], shape)),
                                "ce": (float(both[0]), R.to_rows_grad(both[1], shape)), "stats": reg["stats"]}
    return _REFS[(shape, name)]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def check_value_and_gradient(name, shape, loss, dpred, want):
    nc = shape[5]
    want_loss, want_grad = want
    got = dpred.float().cpu() / SCALE
    err, gerr = abs(float(loss) - want_loss) / abs(want_loss), rel(got[..., :nc].double(), want_grad)
    print(f"{name} {shape}: loss {float(loss):.8f} (float64 {want_loss:.8f}, relative error {err:.3g}), gradient relative error {gerr:.3g}")
    assert err < 2e-5, (float(loss), want_loss)
    assert gerr < 1e-3, gerr
    assert got.shape[2] == nc or float(got[..., nc:].abs().max()) == 0.0
    return err, gerr


def check_stats(name, crit, want, bound=1e-6):
    got = crit.region_stats.cpu()
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got[..., 2], want[..., 2])                              # Y: integers, exact
    worst = 0.0
    for q, label in ((0, "I"), (1, "P"), (3, "T")):
        e = float(((got[..., q] - want[..., q]).abs() / want[..., q].abs().clamp_min(1e-300)).max())
        worst = max(worst, e)
        assert bool(((got[..., q] - want[..., q]).abs() <= bound * want[..., q].abs()).all()), (label, e)
    print(f"{name}: region_stats I, P, T worst relative error {worst:.3g}")


def run_case(dev, shape, name):
    B, ih, iw, H, W, nc = shape
    rows, t, w = inputs(shape)
    ref = reference(shape, name)
    d_rows, d_t = rows.to(dev), t.to(dev)
    crit = SegLoss("ce", region=R.config(name, w))
    crit.nc = nc
    loss, dpred = crit.op(d_rows, d_t, (ih, iw), SCALE)
    check_value_and_gradient("ce + " + name, shape, loss, dpred, ref["ce"])
    check_stats(name, crit, ref["stats"])
    # rows whose stride is not a multiple of 8 floats: the scalar-load path of both pixel passes
    rows_odd = torch.zeros(B, ih * iw, nc + 1)
    rows_odd[..., :nc] = rows[..., :nc]
    loss_o, dpred_o = crit.op(rows_odd.to(dev), d_t, (ih, iw), SCALE)
    check_value_and_gradient("ce + " + name + ", ld = nc + 1", shape, loss_o, dpred_o, ref["ce"])
    check_stats(name + ", ld = nc + 1", crit, ref["stats"])
    # the region term alone: no base chain, a plain write of the gradient plane
    alone = SegLoss("ce", region=dict(R.config(name, w), base_weight=0.0))
    alone.nc = nc
    loss_a, dpred_a = alone.op(d_rows, d_t, (ih, iw), SCALE)
    check_value_and_gradient(name + " alone", shape, loss_a, dpred_a, ref["alone"])
    check_stats(name + " alone", alone, ref["stats"])


@pytest.mark.parametrize("name", list(R.CONFIGS))
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_gradient_and_stats_against_float64(dev, shape, name):
    run_case(dev, shape, name)


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_less_than_one_workgroup(dev, name):
    run_case(dev, TINY, name)


def ohem_inputs(case):
    shape, seed, min_kept, thresh = case
    rows, t, w = R.make_case(shape, seed)
    return shape, rows, t, w, dict(thresh=thresh, min_kept=min_kept)


COMPOSITIONS = {
    "ce+dice": (R.SHAPES[0], "ce", {}, dict(kind="dice", weight=0.7, base_weight=1.3)),
    "ce_weights_smoothing_ohem+tversky": (OHEM_UPSAMPLED, "ce", dict(weights=True, label_smoothing=0.1, ohem=True),
                                          dict(kind="tversky", gamma=0.75, per_image=True, weight=2.0, base_weight=0.5)),
    "focal+dice": (R.SHAPES[3], "focal", {}, dict(kind="dice", weight=1.5)),
}


def compose(dev, shape, rows, t, loss_type, base_kw, region):
    """(the compound criterion, its loss and dpred, the base alone, its loss and dpred, the region alone, its loss and dpred)"""
    B, ih, iw, H, W, nc = shape
    d_rows, d_t = rows.to(dev), t.to(dev)
    out = []
    for kw in (dict(base_kw, region=region), base_kw, dict(region=dict(region, base_weight=0.0))):
        crit = SegLoss(loss_type, **kw)
        crit.nc = nc
        loss, dpred = crit.op(d_rows, d_t, (ih, iw), SCALE)
        out += [crit, loss.clone(), dpred.clone()]
    return out


@pytest.mark.parametrize("name", list(COMPOSITIONS))
def test_composition_with_the_existing_entries(dev, name):
    case, loss_type, opts, region = COMPOSITIONS[name]
    if opts:
        shape, rows, t, w, ohem = ohem_inputs(case)
        base_kw = dict(class_weights=w, label_smoothing=opts["label_smoothing"], ohem=ohem)
    else:
        shape, base_kw = case, {}
        rows, t, w = R.case(shape)
    nc = shape[5]
    crit, loss, dpred, base, loss_b, dpred_b, alone, loss_a, dpred_a = compose(dev, shape, rows, t, loss_type, base_kw, region)
    bw = region.get("base_weight", 1.0)
    want = bw * float(loss_b) + float(loss_a)                                     # the region-alone criterion carries `weight` already
    err = abs(float(loss) - want) / abs(want)
    want_d = bw * dpred_b.float() + dpred_a.float()
    derr = rel(dpred.float(), want_d)
    print(f"{name}: loss {float(loss):.8f} = {bw} * {float(loss_b):.8f} + {float(loss_a):.8f} (relative error {err:.3g}); dpred relative error {derr:.3g}")
    assert err < 2e-5 and derr < 1e-3
    assert torch.equal(crit.region_stats, alone.region_stats)                     # OHEM selects for the base only: the sums run over all valid pixels
    if opts:
        assert torch.equal(crit.last_stats, base.last_stats) and float(crit.last_stats[0]) < float(crit.last_stats[1])   # pixels were dropped
        assert torch.equal(crit.ohem_keys(), base.ohem_keys())
    # two calls on the same inputs: the same bits
    B, ih, iw = shape[0], shape[1], shape[2]
    stats = crit.region_stats.clone()
    loss2, dpred2 = crit.op(rows.to(dev), t.to(dev), (ih, iw), SCALE)
    assert torch.equal(loss2.view(torch.int32), loss.view(torch.int32)) and torch.equal(dpred2.view(torch.int16), dpred.view(torch.int16))
    assert torch.equal(crit.region_stats.view(torch.int64), stats.view(torch.int64))
    loss3, dpred3 = alone.op(rows.to(dev), t.to(dev), (ih, iw), SCALE)
    assert torch.equal(loss3.view(torch.int32), loss_a.view(torch.int32)) and torch.equal(dpred3.view(torch.int16), dpred_a.view(torch.int16))


def test_a_pixel_ohem_drops_still_carries_the_region_gradient(dev):
    """Label resolution = logits resolution: the upsampling and its adjoint are the identity, so dpred is the per-pixel gradient."""
    shape, rows, t, w, ohem = ohem_inputs(OHEM_IDENTITY)
    B, ih, iw, H, W, nc = shape
    region = dict(kind="tversky", alpha=0.7, beta=0.3, gamma=2.0)
    crit, loss, dpred, base, loss_b, dpred_b, alone, loss_a, dpred_a = compose(dev, shape, rows, t, "ce", dict(class_weights=w, label_smoothing=0.1, ohem=ohem),
                                                                               region)
    keys, stats = crit.ohem_keys().cpu(), crit.last_stats.cpu()
    theta_t, theta_min = np.float32(abs(math.log(ohem["thresh"]))), np.float32(float(stats[2]))
    kn = keys.numpy()
    valid = kn >= 0
    kept = valid & ((kn > theta_t) | (kn >= theta_min))
    dropped = torch.from_numpy(valid & ~kept).reshape(B, ih * iw)
    assert int(kept.sum()) == int(stats[0]) and 0 < int(dropped.sum()) == int(stats[1]) - int(stats[0])
    comb, reg, bas = dpred.float().cpu()[..., :nc], dpred_a.float().cpu()[..., :nc], dpred_b.float().cpu()[..., :nc]
    assert float(bas[dropped].abs().max()) == 0.0                                  # the base term is gone there
    worst = float((comb[dropped] - reg[dropped]).abs().max() / comb.abs().max())
    print(f"{int(dropped.sum())} dropped pixels: region gradient max {float(reg[dropped].abs().max()):.4g}, compound - region there {worst:.3g} of the max norm")
    assert float(reg[dropped].abs().max()) > 0.0 and worst < 1e-3
    assert bool((comb[dropped].abs().amax(1) > 0).all())


@pytest.mark.parametrize("base_weight", [1.0, 0.0], ids=["with_base", "region_alone"])
@pytest.mark.parametrize("loss_type", ["ce", "focal"])
def test_bad_label_flag(dev, loss_type, base_weight):
    shape = R.SHAPES[1]
    B, ih, iw, H, W, nc = shape
    rows, t, _ = inputs(shape)
    crit = SegLoss(loss_type, region=dict(kind="dice", base_weight=base_weight))
    crit.nc = nc
    tb = t.clone()
    tb[0, H - 1, W - 1] = nc + 3
    with pytest.raises(CvxError):
        crit.op(rows.to(dev), tb.to(dev), (ih, iw), SCALE)
    crit.op(rows.to(dev), tb.to(dev), (ih, iw), SCALE, check=False)
    assert crit.bad_targets()
    loss, _ = crit.op(rows.to(dev), t.to(dev), (ih, iw), SCALE, check=False)
    assert not crit.bad_targets() and math.isfinite(float(loss))
    with pytest.raises(ValueError):                                                # the length is known at the first call
        SegLoss(loss_type, region=dict(kind="dice", class_weights=[1.0] * (nc + 1))).op(rows.to(dev), t.to(dev), (ih, iw), SCALE)


def test_more_classes_than_a_workgroup_has_threads(dev):
    """nc = 260 (> 256 threads, not a multiple of 8) against float64; beyond the limit of 1024 classes the entry refuses.

    The statistics' bound here is 1e-5, not the 1e-6 of the sums over many pixels: with 99 pixels and 260 classes I_c is the probability
    of ONE pixel, exp(z_t - lse) in fp32.  The logits reach |z| = 8 and more (ulp 9.5e-7); the three roundings of bilinear_mix and as
    many in the log-sum-exp put up to about 4 ulp = 3.8e-6 on each of z_t and lse, and expf adds 2e-7: 8e-6 relative on p, and no
    averaging over pixels.  (Measured: 1.1e-6.)"""
    shape = (1, 4, 5, 9, 11, 260)
    B, ih, iw, H, W, nc = shape
    rows, t, _ = R.make_case(shape, 21)
    logits = R.upsample(R.low_res_nchw(rows, shape), shape)
    reg = R.region(logits, t, kind="tversky")
    base = R.criterion(logits, t)
    v, g = R.combine(base["loss"], base["grad"], reg)
    crit = SegLoss("ce", region=dict(kind="tversky"))
    crit.nc = nc
    loss, dpred = crit.op(rows.to(dev), t.to(dev), (ih, iw), SCALE)
    check_value_and_gradient("ce + tversky, 260 classes", shape, loss, dpred, (float(v), R.to_rows_grad(g, shape)))
    check_stats("260 classes", crit, reg["stats"], bound=1e-5)
    big = SegLoss("ce", region=dict(kind="dice"))
    with pytest.raises(CvxError):
        big.op(torch.zeros(1, 4, 1032, device=dev), torch.zeros(1, 4, 4, dtype=torch.long, device=dev), (2, 2), SCALE)


@contextlib.contextmanager
def no_sync(dev):
    """Host synchronisation inside the block is an error, where this build of torch can flag one."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=dev).item()
            flagged = False
        except RuntimeError:
            flagged = True
        if not flagged:
            torch.cuda.set_sync_debug_mode("default")
        yield flagged
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_validation_pass(dev):
    from core.trainer.segmentation_trainer import SegmentationMetrics
    w = None
    slots = torch.zeros(4, device=dev)
    trained, batches = [], []
    for i, shape in enumerate((R.SHAPES[0], R.SHAPES[3])):
        rows, t, w = inputs(shape)
        batches.append((shape, rows.to(dev), t.to(dev), w))
    # nc differs between the two shapes: one metrics object and criterion per class count, two batches through each
    for i, (shape, d_rows, d_t, w) in enumerate(batches):
        B, ih, iw, H, W, nc = shape
        region = dict(kind="tversky", gamma=0.75, per_image=True, weight=0.8, base_weight=1.2)
        crit = SegLoss("ce", class_weights=w, label_smoothing=0.1, ohem=dict(thresh=0.7, min_kept=10), region=region)
        train = SegLoss("ce", class_weights=w, label_smoothing=0.1, region=region)                    # the training value without OHEM
        crit.nc = train.nc = nc
        flipped = torch.flip(d_t, dims=[2]).contiguous()
        want = [float(train.op(d_rows, tt, (ih, iw), SCALE)[0]) for tt in (d_t, flipped)]
        plain, fused = SegmentationMetrics(nc, device=dev), SegmentationMetrics(nc, device=dev)
        plain.add_rows(d_rows, d_t, (ih, iw), SegLoss("ce"), slots[3:4])
        plain.add_rows(d_rows, flipped, (ih, iw), SegLoss("ce"), slots[3:4])
        SegmentationMetrics(nc, device=dev).add_rows(d_rows, d_t, (ih, iw), crit, slots[3:4])     # the first call copies the class weights
        with no_sync(dev) as flagged:
            fused.add_rows(d_rows, d_t, (ih, iw), crit, slots[0:1])
            fused.add_rows(d_rows, flipped, (ih, iw), crit, slots[1:2])
        got = slots[:2].cpu().tolist()
        errs = [abs(g - v) / abs(v) for g, v in zip(got, want)]
        print(f"validation {shape}: slots {got}, training values {want}, relative errors {errs}, sync flagged: {flagged}")
        assert max(errs) < 2e-5
        assert torch.equal(fused.counts, plain.counts) and int(fused.counts.sum()) == 2 * int((d_t != -100).sum())
    # the region term alone and a focal base
    shape, d_rows, d_t, w = batches[0]
    B, ih, iw, H, W, nc = shape
    for loss_type, bw in (("focal", 1.0), ("ce", 0.0)):
        crit = SegLoss(loss_type, region=dict(kind="dice", base_weight=bw))
        crit.nc = nc
        want = float(crit.op(d_rows, d_t, (ih, iw), SCALE)[0])
        m = SegmentationMetrics(nc, device=dev)
        m.add_rows(d_rows, d_t, (ih, iw), crit, slots[2:3])
        assert abs(float(slots[2]) - want) < 2e-5 * abs(want), (loss_type, float(slots[2]), want)


def test_train_steps_end_to_end(dev, gold):
    from computervision.pytorch_amd.deeplab import DeepLabV3PlusR101, SegTrainStep
    from computervision.pytorch_amd.train import DynamicLossScale, FlatAdam
    g = gold("deeplab_train_97x129.npz")
    x, t = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["target"].astype(np.int64)).to(dev)
    torch.manual_seed(0)
    m = DeepLabV3PlusR101(21).to(dev).train()
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    crit = SegLoss("ce", region=dict(kind="dice"))
    sc = DynamicLossScale(dev, init_scale=4096.0)
    step = SegTrainStep(m, crit, FlatAdam(m, lr=1e-3), scaler=sc)
    losses = [step(x, t).clone()]                                               # the first step allocates
    held = (crit._ws.data_ptr(), crit._ws.numel(), crit.region_stats.data_ptr(), crit._bad.data_ptr())
    with no_sync(dev) as flagged:
        for _ in range(2):
            losses.append(step(x, t).clone())
    torch.cuda.synchronize()
    assert held == (crit._ws.data_ptr(), crit._ws.numel(), crit.region_stats.data_ptr(), crit._bad.data_ptr())
    losses = torch.cat(losses).cpu()
    stats = crit.region_stats.cpu()
    print(f"sync flagged: {flagged}; losses {losses.tolist()}; mean T of the present classes {float(stats[0, stats[0, :, 2] > 0, 3].mean()):.4f}")
    assert bool(torch.isfinite(losses).all()) and float(losses[-1]) < float(losses[0])
    n_valid = int(((t != -100) & (t >= 0) & (t < 21)).sum())
    assert int(stats[0, :, 2].sum()) == n_valid
    sc.poll()
    assert sc.skipped == 0 and not crit.bad_targets()
    moved = torch.stack([(p.detach() != before[k]).any() for k, p in m.named_parameters()]).cpu()
    still = [k for (k, _), mv in zip(m.named_parameters(), moved.tolist()) if not mv]
    assert not still, still
