"""MI355X: the options of ``cvx_seg_criterion_loss`` / ``cvx_seg_criterion_eval`` (csrc/loss_seg.hip) -- cross-entropy with class weights, label
smoothing and online hard example mining in the fused criterion chain -- against torch float64 and tests/seg_loss_restatement.py, and
``SegLoss(class_weights=, label_smoothing=, ohem=)`` end to end in ``SegTrainStep``.

Bounds.  Loss: 2e-5 relative, the bound the option-free criterion is held to.  Gradient: 1e-3 relative in the max norm, one fp16 rounding of the
scaled gradient.  OHEM keys: four times the distance E between torch's own fp32 and fp64 keys on the same inputs (E is measured in the
test from the two references, at most 1.3e-5 absolute on these cases; every test prints what it measured).  The selection itself is exact
on the device's own keys: no tolerance.  Against the float64 selection the device's mask may differ only at pixels whose float64 key lies
within 1e-4 of a threshold, and the restatement alone shows that at most 2 valid pixels do (tests/test_seg_loss_opts_cpu.py pins 1, 1,
0, 1, 2, 1 for the six cases)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd.deeplab import SegLoss
import seg_loss_restatement as R

pytestmark = pytest.mark.gpu

SCALE = 65536.0
SHAPES = [(2, 9, 12, 33, 45, 21), (1, 5, 6, 40, 48, 5), (2, 33, 33, 33, 33, 19), (3, 17, 12, 65, 45, 5)]
# (shape, seed, min_kept, thresh, valid, kept, weights and smoothing too)
OHEM_CASES = [
    (SHAPES[0], 11, 200, 0.7, 2519, 2516, True),
    (SHAPES[0], 11, 200, 1e-4, 2519, 400, False),
    (SHAPES[1], 12, 100000, 0.7, 1593, 1593, True),
    (SHAPES[2], 13, 300, 0.02, 1846, 1169, True),
    (SHAPES[3], 14, 500, 0.3, 7431, 5632, False),
    (SHAPES[3], 14, 500, 0.01, 7431, 1500, True),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def reference(shape, rows, t, weights, eps, kept=None):
    """torch float64: F.cross_entropy on F.interpolate(bilinear, align_corners=False) of the rows, the targets outside ``kept`` ignored;
    (loss, d loss / d rows as (B, ih*iw, nc))."""
    B, ih, iw, H, W, nc = shape
    low = R.low_res_nchw(rows, shape).requires_grad_(True)
    tt = t if kept is None else torch.where(kept, t, torch.full_like(t, -100))
    loss = F.cross_entropy(R.upsample(low, shape), tt, weight=None if weights is None else weights.double(), ignore_index=-100,
                           label_smoothing=eps, reduction="mean")
    loss.backward()
    return float(loss), low.grad.permute(0, 2, 3, 1).reshape(B, ih * iw, nc)


def check_value_and_gradient(name, shape, loss, dpred, want_loss, want_grad):
    nc = shape[5]
    got = dpred.float().cpu() / SCALE
    err, gerr = abs(float(loss) - want_loss) / abs(want_loss), rel(got[..., :nc].double(), want_grad)
    print(f"{name}: loss {float(loss):.8f} (float64 {want_loss:.8f}, relative error {err:.3g}), gradient relative error {gerr:.3g}")
    assert err < 2e-5, (float(loss), want_loss)
    assert gerr < 1e-3, gerr
    assert got.shape[2] == nc or float(got[..., nc:].abs().max()) == 0.0


CONFIGS = {"weights": (True, 0.0), "smoothing": (False, 0.1), "both": (True, 0.1)}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weights_and_smoothing_against_torch_fp64(dev, shape, config):
    B, ih, iw, H, W, nc = shape
    rows, t, w = R.make_case(shape, B * 1000 + H + nc)
    weighted, eps = CONFIGS[config]
    w = w if weighted else None
    want_loss, want_grad = reference(shape, rows, t, w, eps)
    crit = SegLoss("ce", class_weights=w, label_smoothing=eps)
    crit.nc = nc
    loss, dpred = crit.op(rows.to(dev), t.to(dev), (ih, iw), SCALE)
    check_value_and_gradient(config, shape, loss, dpred, want_loss, want_grad)
    stats = crit.last_stats.cpu()
    n_valid = int((t != -100).sum())
    assert stats[0] == stats[1] == n_valid and stats[2] == -math.inf
    assert abs(float(stats[3]) - float((w[t[t != -100]].double().sum() if weighted else n_valid))) <= 1e-9 * n_valid
    # rows whose stride is not a multiple of 8 floats take the scalar-load path of the pixel kernel: same numbers
    rows_odd = torch.zeros(B, ih * iw, nc + 1)
    rows_odd[..., :nc] = rows[..., :nc]
    loss_o, dpred_o = crit.op(rows_odd.to(dev), t.to(dev), (ih, iw), SCALE)
    check_value_and_gradient(config + ", ld = nc + 1", shape, loss_o, dpred_o, want_loss, want_grad)
    assert abs(float(loss_o) - float(loss)) <= 1e-6 * abs(float(loss)) and rel(dpred_o[..., :nc].float(), dpred[..., :nc].float()) < 1e-3
    # labels outside [0, nc) that are not the ignore index: flagged, the pixel is skipped
    tb = t.clone()
    tb[0, 0, 0] = nc + 3
    with pytest.raises(CvxError):
        crit.op(rows.to(dev), tb.to(dev), (ih, iw), SCALE)
    crit.op(rows.to(dev), tb.to(dev), (ih, iw), SCALE, check=False)
    assert crit.bad_targets()
    crit.op(rows.to(dev), t.to(dev), (ih, iw), SCALE, check=False)
    assert not crit.bad_targets()
    with pytest.raises(ValueError):
        SegLoss("ce", class_weights=[1.0] * (nc + 1)).op(rows.to(dev), t.to(dev), (ih, iw), SCALE)   # nc comes from ld: still the wrong length


def call_opts_entry(dev, rows, t, shape, weights=None, eps=0.0, theta=-1.0, k=0):
    """cvx_seg_criterion_loss with a cross-entropy base and exactly these options, no SegLoss in between"""
    B, ih, iw, H, W, nc = shape
    lib = L.load()
    ld = rows.shape[2]
    dims = L.SegDims(ld, B, nc, ih, iw, H, W)
    crit = L.SegCriterion(base=2, class_weight=weights.data_ptr() if weights is not None else None, label_smoothing=eps, ignore_index=-100,
                          ohem_theta=theta, ohem_min_kept=k)
    ws = torch.empty(int(lib.cvx_seg_criterion_workspace_bytes(ctypes.byref(dims), ctypes.byref(crit), 0)), dtype=torch.uint8, device=dev)
    loss, bad = torch.empty(1, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    dpred = torch.full((B, ih * iw, ld), float("nan"), dtype=torch.float16, device=dev)
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    L.check(lib.cvx_seg_criterion_loss(L.ptr(rows), ctypes.byref(dims), L.ptr(t), ctypes.byref(crit), SCALE, L.ptr(loss), L.ptr(dpred), L.ptr(bad),
                                       L.ptr(stats), None, L.ptr(ws), L.stream_ptr(dev)), "cvx_seg_criterion_loss")
    return loss, dpred, stats


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_no_option_reproduces_the_plain_entry_bit_for_bit(dev, shape):
    """unit class weights and zero smoothing go through the options kernel (Ce<true>) and reproduce SegLoss("ce"), the option-free kernel
    (Ce<false>), bit for bit"""
    B, ih, iw, H, W, nc = shape
    rows, t, _ = R.make_case(shape, B * 1000 + H + nc)
    ones = torch.ones(nc, device=dev)
    for r in (rows, torch.cat([rows[..., :nc], torch.zeros(B, ih * iw, 1)], 2).contiguous()):        # vector and scalar path
        d_rows, d_t = r.to(dev), t.to(dev)
        plain = SegLoss("ce")
        plain.nc = nc
        loss0, dpred0 = plain.op(d_rows, d_t, (ih, iw), SCALE)
        loss1, dpred1, stats = call_opts_entry(dev, d_rows, d_t, shape, weights=ones)
        assert torch.equal(loss0.view(torch.int32), loss1.view(torch.int32))
        assert torch.equal(dpred0.view(torch.int16), dpred1.view(torch.int16))
        assert stats[0] == stats[1] == stats[3] == int((t != -100).sum())


def torch_fp32_keys(shape, rows, t):
    z = R.upsample(R.low_res_nchw(rows, shape, torch.float32), shape)
    valid = t != -100
    ce = torch.logsumexp(z, 1) - z.gather(1, torch.where(valid, t, torch.zeros_like(t))[:, None])[:, 0]
    return torch.where(valid, ce.clamp_min(0), torch.full_like(ce, -1.0))


@pytest.mark.parametrize("case", OHEM_CASES, ids=lambda c: f"{c[0][3]}x{c[0][4]}-k{c[2]}-t{c[3]}")
def test_ohem(dev, case):
    shape, seed, min_kept, thresh, n_valid, n_kept, with_options = case
    B, ih, iw, H, W, nc = shape
    rows, t, w = R.make_case(shape, seed)
    w, eps = (w, 0.1) if with_options else (None, 0.0)
    ohem = dict(thresh=thresh, min_kept=min_kept)
    K = min_kept * B
    res = R.criterion(R.upsample(R.low_res_nchw(rows, shape), shape), t, w, eps, ohem)
    assert int(res["valid"].sum()) == n_valid and int(res["kept"].sum()) == n_kept
    theta_t = R.theta_of(thresh)
    k64 = res["keys"]
    band = res["valid"] & ((k64 - theta_t).abs() <= 1e-4)
    if math.isfinite(res["theta_min"]):
        band |= res["valid"] & ((k64 - res["theta_min"]).abs() <= 1e-4)
    assert int(band.sum()) <= 2                                       # from the restatement alone

    crit = SegLoss("ce", class_weights=w, label_smoothing=eps, ohem=ohem)
    crit.nc = nc
    d_rows, d_t = rows.to(dev), t.to(dev)
    loss, dpred = crit.op(d_rows, d_t, (ih, iw), SCALE)
    keys = crit.ohem_keys().cpu()
    stats = crit.last_stats.cpu().clone()
    loss, dpred = loss.cpu(), dpred.cpu()
    # 1. the keys against float64, within 4 x torch fp32's own distance to float64
    E = float((torch_fp32_keys(shape, rows, t).double() - k64).abs().max())
    kerr = float((keys.double() - k64).abs().max())
    print(f"keys: max |device - float64| {kerr:.3g}; torch fp32 against float64 E = {E:.3g}, bound {4 * E:.3g}")
    assert tuple(keys.shape) == (B, H, W) and bool(((keys == -1) == ~res["valid"]).all())
    assert kerr <= 4 * E
    # 2. the selection is exact on the device's own keys
    kn = keys.numpy()
    vk = np.sort(kn[kn >= 0])[::-1]
    assert stats[1] == len(vk) == n_valid
    if len(vk) >= K:
        theta_min = vk[K - 1]
        assert np.float32(float(stats[2])).view(np.uint32) == theta_min.view(np.uint32) and float(stats[2]) == float(theta_min)
    else:
        theta_min = np.float32(-np.inf)
        assert float(stats[2]) == -math.inf
    mask = (kn >= 0) & ((kn > np.float32(theta_t)) | (kn >= theta_min))
    assert int(stats[0]) == int(mask.sum()) >= min(K, n_valid)
    # 3. loss and gradient against torch float64 on the device's kept set
    kept = torch.from_numpy(mask)
    want_loss, want_grad = reference(shape, rows, t, w, eps, kept)
    check_value_and_gradient("ohem", shape, loss, dpred, want_loss, want_grad)
    assert abs(float(stats[3]) - float((w.double()[t[kept]].sum() if w is not None else mask.sum()))) <= 1e-9 * n_valid
    # 4. the device's mask against the float64 mask: they may differ inside the band only
    differ = kept != res["kept"]
    print(f"kept {int(mask.sum())} (float64 {n_kept}), {int(differ.sum())} pixels differ, {int(band.sum())} in the band")
    assert bool((differ <= band).all())
    # 5. repeatability, also on the scalar path's own run
    loss2, dpred2 = crit.op(d_rows, d_t, (ih, iw), SCALE)
    assert torch.equal(loss2.cpu().view(torch.int32), loss.view(torch.int32)) and torch.equal(dpred2.cpu().view(torch.int16), dpred.view(torch.int16))
    assert torch.equal(crit.last_stats.cpu().view(torch.int64), stats.view(torch.int64))
    rows_odd = torch.zeros(B, ih * iw, nc + 1)
    rows_odd[..., :nc] = rows[..., :nc]
    loss_o, dpred_o = crit.op(rows_odd.to(dev), d_t, (ih, iw), SCALE)
    assert torch.equal(crit.ohem_keys().cpu(), keys)                   # the same taps, the same class order: the same keys
    check_value_and_gradient("ohem, ld = nc + 1", shape, loss_o, dpred_o, want_loss, want_grad)


def test_ohem_with_constant_logits_keeps_every_valid_pixel(dev):
    shape = SHAPES[1]
    B, ih, iw, H, W, nc = shape
    _, t, _ = R.make_case(shape, 5)
    rows = torch.full((B, ih * iw, 8), 0.25)
    crit = SegLoss("ce", ohem=dict(thresh=1e-3, min_kept=10))               # K = 10; every key is the same number: all tied at rank K
    crit.nc = nc
    loss, dpred = crit.op(rows.to(dev), t.to(dev), (ih, iw), SCALE)
    stats, keys = crit.last_stats.cpu(), crit.ohem_keys().cpu()
    n_valid = int((t != -100).sum())
    assert stats[0] == stats[1] == n_valid > 10
    assert len(torch.unique(keys[keys >= 0])) == 1 and float(stats[2]) == float(keys[keys >= 0][0])
    assert abs(float(loss) - math.log(nc)) < 2e-5 * math.log(nc)


def test_all_targets_ignored(dev):
    shape = SHAPES[1]
    B, ih, iw, H, W, nc = shape
    rows, t, w = R.make_case(shape, 5)
    t = torch.full_like(t, -100)
    for ohem in (None, dict(thresh=0.7, min_kept=10)):
        crit = SegLoss("ce", class_weights=w, label_smoothing=0.1, ohem=ohem)
        crit.nc = nc
        loss, dpred = crit.op(rows.to(dev), t.to(dev), (ih, iw), SCALE)
        assert math.isnan(float(loss)) and float(dpred.float().abs().max()) == 0.0
        assert crit.last_stats.cpu()[[0, 1, 3]].tolist() == [0.0, 0.0, 0.0]


# the last shape: nc = 91 is the first class count whose nc * nc cells miss the LDS histogram, so the evaluation kernel counts in the global matrix
EVAL_SHAPES = [(SHAPES[0], 0), (SHAPES[3], 0), ((1, 3, 3, 9, 11, 91), 96), ((1, 3, 3, 9, 11, 91), 92)]


@pytest.mark.parametrize("shape,ld", EVAL_SHAPES, ids=["x".join(map(str, s)) + (f"-ld{ld}" if ld else "") for s, ld in EVAL_SHAPES])
def test_eval_opts(dev, shape, ld):
    from core.trainer.segmentation_trainer import SegmentationMetrics
    B, ih, iw, H, W, nc = shape
    rows, t, w = R.make_case(shape, B * 1000 + H + nc)
    if ld:
        rows = torch.cat([rows[..., :nc], torch.zeros(B, ih * iw, ld - nc)], 2).contiguous()
    want_loss, _ = reference(shape, rows, t, w, 0.1)
    d_rows, d_t = rows.to(dev), t.to(dev)
    slots = torch.zeros(2, device=dev)
    plain, opts = SegmentationMetrics(nc, device=dev), SegmentationMetrics(nc, device=dev)
    plain.add_rows(d_rows, d_t, (ih, iw), SegLoss("ce"), slots[0:1])
    opts.add_rows(d_rows, d_t, (ih, iw), SegLoss("ce", class_weights=w, label_smoothing=0.1, ohem=dict(thresh=0.7, min_kept=10)), slots[1:2])
    assert torch.equal(plain.counts, opts.counts) and int(opts.counts.sum()) == int((t != -100).sum())
    err = abs(float(slots[1]) - want_loss) / want_loss
    print(f"validation value {float(slots[1]):.8f} (float64 {want_loss:.8f}, relative error {err:.3g}); plain {float(slots[0]):.8f}")
    assert err < 2e-5
    assert abs(float(slots[0]) - reference(shape, rows, t, None, 0.0)[0]) < 2e-5 * float(slots[0])


def test_train_steps_end_to_end(dev, gold):
    from computervision.pytorch_amd.deeplab import DeepLabV3PlusR101, SegTrainStep
    from computervision.pytorch_amd.train import DynamicLossScale, FlatAdam
    from core.trainer.segmentation_trainer import SegmentationMetrics
    g = gold("deeplab_train_97x129.npz")
    x, t = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["target"].astype(np.int64)).to(dev)
    torch.manual_seed(0)
    m = DeepLabV3PlusR101(21).to(dev).train()
    w = torch.rand(21, generator=torch.Generator().manual_seed(1)) + 0.1
    crit = SegLoss("ce", class_weights=w, label_smoothing=0.1, ohem=dict(thresh=0.7, min_kept=500))
    sc = DynamicLossScale(dev, init_scale=4096.0)
    step = SegTrainStep(m, crit, FlatAdam(m, lr=1e-3), scaler=sc)
    losses, stats = [step(x, t).clone()], [crit.last_stats.clone()]          # the first step allocates and copies the weights
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=dev).item()
            flagged = False
        except RuntimeError:
            flagged = True
        if not flagged:
            torch.cuda.set_sync_debug_mode("default")                         # this build does not flag a read-back: the steps run unguarded
        for _ in range(5):
            losses.append(step(x, t).clone())
            stats.append(crit.last_stats.clone())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    losses, stats = torch.cat(losses).cpu(), torch.stack(stats).cpu()
    print(f"sync flagged: {flagged}; losses {losses.tolist()}; kept {stats[:, 0].tolist()} of {stats[:, 1].tolist()}")
    assert bool(torch.isfinite(losses).all()) and float(losses[-1]) < float(losses[0])
    n_valid = int(((t != -100) & (t >= 0) & (t < 21)).sum())
    assert bool((stats[:, 1] == n_valid).all())
    assert bool((stats[:, 0] >= min(1000, n_valid)).all()) and bool((stats[:, 0] <= n_valid).all())
    sc.poll()
    assert sc.skipped == 0 and not crit.bad_targets()
    m.eval()
    metrics, slot = SegmentationMetrics(21, device=dev), torch.zeros(1, device=dev)
    with torch.no_grad():
        rows = m.forward_rows(x)
    metrics.add_rows(rows, t, m._last_engine.graph.level_hw[0], crit, slot)
    assert math.isfinite(float(slot)) and float(slot) > 0 and int(metrics.counts.sum()) == n_valid
