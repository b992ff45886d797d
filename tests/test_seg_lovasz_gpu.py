"""MI355X: the Lovasz-Softmax term of ``cvx_seg_criterion_loss`` / ``cvx_seg_criterion_eval`` (csrc/loss_seg.hip, csrc/lovasz_sort.h) through
``SegLoss(lovasz=)``: value, gradient and statistics against float64 (tests/seg_lovasz_restatement.py, which tests/test_seg_lovasz_cpu.py
holds against Berman's formulation under autograd), the device-wide sort itself from ``lovasz_sorted()`` (exact), ties, all four digit
passes, many classes, the edge cases, composition with the existing entries, bit repeatability, the fused validation pass and
``SegTrainStep`` end to end.

Bounds: the project's (tests/test_seg_region_gpu.py).  Value 2e-5 relative; gradient 1e-3 relative in the max norm (one fp16 rounding of
the scaled gradient); Y_c exact; L_c 1e-6 relative.  The gradient is not continuous in the order of the errors: tests/test_seg_lovasz_cpu.py
asserts for every input used here that the order taken from fp32 errors moved by a few ulp changes d / d rows by less than 1e-4 (the tie
cases tie exactly instead).  The sort tile is 1024 elements: SHAPES[3] has 7459 valid pixels in its batch group (8 tiles, the last ragged)
and about 2490 per image (3 tiles).  Every test prints what it measured."""
import contextlib
import math

import numpy as np
import pytest
import torch

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd.deeplab import SegLoss
import seg_lovasz_restatement as R

pytestmark = pytest.mark.gpu

SCALE = 65536.0
CASES = R.gpu_cases()
# OHEM_CASES[3] and [1] of tests/test_seg_loss_opts_gpu.py: (shape, seed, min_kept, thresh); both drop valid pixels
OHEM_IDENTITY = (R.SHAPES[2], 13, 300, 0.02)
OHEM_UPSAMPLED = (R.SHAPES[0], 11, 200, 1e-4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


_REFS, _KEY_ERR = {}, {}


def reference_of(shape, rows, t, cfg, tied=False):
    logits = R.full_logits(shape, rows, tied)
    lov = R.lovasz(logits, t, **cfg)
    base = R.criterion(logits, t)
    both = R.combine(base["loss"], base["grad"], lov)
    return {"alone": (float(lov["value"]), R.to_rows_grad(lov["grad"], shape)), "ce": (float(both[0]), R.to_rows_grad(both[1], shape)),
            "stats": lov["stats"], "order": lov["order"], "errors": lov["errors"], "valid": lov["valid"]}


def reference(name, cname):
    """float64, computed once per (case, configuration)"""
    if (name, cname) not in _REFS:
        shape, rows, t, w, tied = CASES[name]
        _REFS[(name, cname)] = reference_of(shape, rows, t, R.config(cname, w), tied)
    return _REFS[(name, cname)]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def check_value_and_gradient(label, shape, loss, dpred, want):
    nc = shape[5]
    want_loss, want_grad = want
    got = dpred.float().cpu() / SCALE
    err, gerr = abs(float(loss) - want_loss) / abs(want_loss), rel(got[..., :nc].double(), want_grad)
    print(f"{label} {shape}: loss {float(loss):.8f} (float64 {want_loss:.8f}, relative error {err:.3g}), gradient relative error {gerr:.3g}")
    assert err < 2e-5, (float(loss), want_loss)
    assert gerr < 1e-3, gerr
    assert got.shape[2] == nc or float(got[..., nc:].abs().max()) == 0.0


def check_stats(label, crit, want):
    got = crit.region_stats.cpu()
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(want.shape)
    assert float(got[..., :2].abs().max()) == 0.0
    assert torch.equal(got[..., 2], want[..., 2])                              # Y: integers, exact
    e = float(((got[..., 3] - want[..., 3]).abs() / want[..., 3].abs().clamp_min(1e-300)).max())
    print(f"{label}: L_c worst relative error {e:.3g}")
    assert bool(((got[..., 3] - want[..., 3]).abs() <= 1e-6 * want[..., 3].abs()).all()), e


def check_sorted(label, crit, t, cfg, ref, max_distinct=None):
    """The order itself, exact: per segment the keys do not increase, the payload indices are the group's valid pixels, equal keys carry
    ascending indices, the flag is t == c, and the length is the group's valid-pixel count (0 for a class the sort skips).  Returns the
    largest distance of a key from the float64 error of its pixel (test_keys_against_the_float64_errors holds it to its bound)."""
    keys, payload, segs = (x.cpu().numpy() for x in crit.lovasz_sorted())
    B, nc = t.shape[0], ref["stats"].shape[1]
    G = B if cfg.get("per_image") else 1
    skip = cfg.get("skip_absent", True)
    assert segs.shape == (G, nc, 2) and keys.dtype == np.uint32 and payload.dtype == np.uint32
    tt, vv = t.numpy().reshape(G, -1), ref["valid"].numpy().reshape(G, -1)
    worst = 0.0
    for g in range(G):
        valid_idx = np.nonzero(vv[g])[0]
        for c in range(nc):
            off, n = int(segs[g, c, 0]), int(segs[g, c, 1])
            assert off == (g * nc + c) * tt.shape[1]
            if skip and float(ref["stats"][g, c, 2]) == 0.0:
                assert n == 0
                continue
            assert n == valid_idx.size
            if n == 0:
                continue
            k, pl = keys[off:off + n], payload[off:off + n]
            idx, flag = (pl & np.uint32(0x7FFFFFFF)).astype(np.int64), (pl >> np.uint32(31)).astype(bool)
            assert bool((k[:-1] >= k[1:]).all())
            assert np.array_equal(np.sort(idx), valid_idx)
            tie = k[:-1] == k[1:]
            assert bool((idx[:-1][tie] < idx[1:][tie]).all())
            assert np.array_equal(flag, tt[g][idx] == c)
            e64 = np.empty(tt.shape[1])
            e64[ref["order"][(g, c)]] = ref["errors"][(g, c)]
            worst = max(worst, float(np.abs(k.view(np.float32).astype(np.float64) - e64[idx]).max()))
            if max_distinct is not None:
                assert len(np.unique(k)) <= max_distinct
    print(f"{label}: sorted view exact; keys within {worst:.3g} of the float64 errors")
    _KEY_ERR[label] = worst
    return worst


def live_view(crit):
    """(keys, payload, segments) with the two arrays cut down to the segments' lengths: past a segment's length the workspace holds
    whatever it held."""
    keys, payload, segs = crit.lovasz_sorted()
    spans = [(int(o), int(n)) for o, n in segs.reshape(-1, 2).cpu().tolist()]
    cut = lambda x: torch.cat([x[o:o + n] for o, n in spans]) if spans else x[:0]   # noqa: E731
    return cut(keys).clone(), cut(payload).clone(), segs.clone()


def run_case(dev, name, cname, max_distinct=None):
    shape, rows, t, w, tied = CASES[name]
    B, ih, iw, H, W, nc = shape
    cfg = R.config(cname, w)
    ref = reference(name, cname)
    d_rows, d_t = rows.to(dev), t.to(dev)
    crit = SegLoss("ce", lovasz=cfg)
    crit.nc = nc
    loss, dpred = crit.op(d_rows, d_t, (ih, iw), SCALE)
    label = f"{name} ce + lovasz {cname}"
    check_value_and_gradient(label, shape, loss, dpred, ref["ce"])
    check_stats(label, crit, ref["stats"])
    check_sorted(label, crit, t, cfg, ref, max_distinct)
    # rows whose stride is not a multiple of 8 floats: the scalar-load path of every pixel pass
    rows_odd = torch.zeros(B, ih * iw, nc + 1)
    rows_odd[..., :nc] = rows[..., :nc]
    loss_o, dpred_o = crit.op(rows_odd.to(dev), d_t, (ih, iw), SCALE)
    check_value_and_gradient(label + ", ld = nc + 1", shape, loss_o, dpred_o, ref["ce"])
    check_stats(label + ", ld = nc + 1", crit, ref["stats"])
    check_sorted(label + ", ld = nc + 1", crit, t, cfg, ref, max_distinct)
    # the term alone: no base chain, a plain write of the gradient plane
    alone = SegLoss("ce", lovasz=dict(cfg, base_weight=0.0))
    alone.nc = nc
    loss_a, dpred_a = alone.op(d_rows, d_t, (ih, iw), SCALE)
    check_value_and_gradient(f"{name} lovasz {cname} alone", shape, loss_a, dpred_a, ref["alone"])
    check_stats(label + " alone", alone, ref["stats"])
    check_sorted(label + " alone", alone, t, cfg, ref, max_distinct)


@pytest.mark.parametrize("cname", list(R.CONFIGS))
@pytest.mark.parametrize("name", ["shape0", "shape1", "shape2", "shape3"])
def test_value_gradient_stats_and_order_against_float64(dev, name, cname):
    run_case(dev, name, cname)


KEY_CASES = ([(n, c) for n in ("shape0", "shape1", "shape2", "shape3", "tiny") for c in R.CONFIGS]
             + [(n, c) for n in ("ties_constant", "ties_five", "digits") for c in ("batch", "per_image")] + [("many", "batch")]
             + [("shape0_image1_ignored", c) for c in ("batch", "per_image", "per_image_all")])


@pytest.mark.parametrize("name,cname", KEY_CASES)
def test_keys_against_the_float64_errors(dev, name, cname):
    """Each key within 1e-6 of the float64 error of its pixel, on every case of this file.  The keys kernel takes its interpolation weights
    from a source coordinate formed in double for this: with the fp32 coordinate the other kernels share, the weight carries half an
    ulp of a number of magnitude 8 .. 16 and the keys of SHAPES[0] and SHAPES[3], whose upsampling ratio is not a power of two, were
    1.4e-6 and 2.6e-6 off (2.7e-7 where the ratio is 1/8)."""
    shape, rows, t, w, tied = CASES[name]
    cfg = R.config(cname, w)
    crit = SegLoss("ce", lovasz=dict(cfg, base_weight=0.0))
    crit.nc = shape[5]
    crit.op(rows.to(dev), t.to(dev), (shape[1], shape[2]), SCALE)
    worst = check_sorted(f"{name} {cname} keys", crit, t, cfg, reference(name, cname))
    assert worst < 1e-6, worst


@pytest.mark.parametrize("cname", list(R.CONFIGS))
def test_a_segment_far_smaller_than_a_sort_tile(dev, cname):
    run_case(dev, "tiny", cname)


@pytest.mark.parametrize("cname", ["batch", "per_image"])
@pytest.mark.parametrize("name", ["ties_constant", "ties_five"])
def test_ties_follow_the_index_rule(dev, name, cname):
    """Exact ties, in fp32 and in float64 alike: the order is the index rule (and, for "five", the order of a few distinct values)."""
    run_case(dev, name, cname, max_distinct=10)


@pytest.mark.parametrize("cname", ["batch", "per_image"])
def test_every_digit_pass_and_the_cluster_at_key_zero(dev, cname):
    shape, rows, t, w, _ = CASES["digits"]
    run_case(dev, "digits", cname)
    crit = SegLoss("ce", lovasz=dict(R.config(cname, w), base_weight=0.0))
    crit.nc = shape[5]
    crit.op(rows.to(dev), t.to(dev), (shape[1], shape[2]), SCALE)
    keys, _, segs = (x.cpu().numpy() for x in crit.lovasz_sorted())
    live = np.concatenate([keys[o:o + n] for o, n in segs.reshape(-1, 2)])
    pos = live[live > 0].view(np.float32)
    print(f"digits {cname}: {live.size} keys, {int((live == 0).sum())} exactly 0, the others from {pos.min():.3g} to {pos.max():.3g}")
    assert int((live == 0).sum()) > 100 and float(pos.min()) < 1e-20 and float(pos.max()) > 0.99
    for shift in (0, 8, 16, 24):                                               # every pass has more than one digit to order
        assert len(np.unique((live >> np.uint32(shift)) & np.uint32(255))) > 8


def test_more_classes_than_a_workgroup_has_threads(dev):
    """nc = 260 on 99 pixels, the case of tests/test_seg_region_gpu.py; beyond 1024 classes the entry refuses."""
    run_case(dev, "many", "batch")
    big = SegLoss("ce", lovasz={})
    with pytest.raises(CvxError):
        big.op(torch.zeros(1, 4, 1032, device=dev), torch.zeros(1, 4, 4, dtype=torch.long, device=dev), (2, 2), SCALE)


def test_edge_cases(dev):
    shape, rows, t, w, _ = CASES["shape0"]
    B, ih, iw, H, W, nc = shape
    d_rows = rows.to(dev)
    # an absent class: skipped under skip_absent (length 0 in the view), sorted without
    for skip in (True, False):
        crit = SegLoss("ce", lovasz=dict(skip_absent=skip, base_weight=0.0))
        crit.nc = nc
        crit.op(d_rows, t.to(dev), (ih, iw), SCALE)
        segs, stats = crit.lovasz_sorted()[2].cpu(), crit.region_stats.cpu()
        n_valid = int((t != -100).sum())
        assert float(stats[0, 2, 2]) == 0.0 and int(segs[0, 2, 1]) == (0 if skip else n_valid) and int(segs[0, 3, 1]) == n_valid
        assert (float(stats[0, 2, 3]) == 0.0) == skip
    # an image with every pixel ignored, under per_image (both settings of skip_absent), and in the batch group
    t1 = CASES["shape0_image1_ignored"][2]
    assert int((t1[1] != -100).sum()) == 0
    for cfg in (dict(per_image=True), dict(per_image=True, skip_absent=False), dict()):
        ref = reference_of(shape, rows, t1, cfg)
        crit = SegLoss("ce", lovasz=dict(cfg, base_weight=0.0))
        crit.nc = nc
        loss, dpred = crit.op(d_rows, t1.to(dev), (ih, iw), SCALE)
        check_value_and_gradient(f"image 1 ignored, {cfg}", shape, loss, dpred, ref["alone"])
        check_stats(f"image 1 ignored, {cfg}", crit, ref["stats"])
        check_sorted(f"image 1 ignored, {cfg}", crit, t1, cfg, ref)
        assert float(dpred[1].float().abs().max()) == 0.0
    # no valid pixel at all: the value is the base's and the term adds no gradient
    none = torch.full_like(t, -100).to(dev)
    for cfg in (dict(), dict(per_image=True, skip_absent=False)):
        alone = SegLoss("ce", lovasz=dict(cfg, base_weight=0.0))
        base, both = SegLoss("focal"), SegLoss("focal", lovasz=cfg)
        alone.nc = base.nc = both.nc = nc
        loss_a, dpred_a = alone.op(d_rows, none, (ih, iw), SCALE)
        loss_b, dpred_b = base.op(d_rows, none, (ih, iw), SCALE)
        loss, dpred = both.op(d_rows, none, (ih, iw), SCALE)
        print(f"no valid pixel, {cfg}: lovasz alone {float(loss_a)}, focal {float(loss_b)}, focal + lovasz {float(loss)}")
        assert float(loss_a) == 0.0 and float(dpred_a.float().abs().max()) == 0.0
        assert float(loss) == float(loss_b) == 0.0 and float(dpred.float().abs().max()) == 0.0 == float(dpred_b.float().abs().max())
        assert float(alone.region_stats.abs().max()) == 0.0 and int(alone.lovasz_sorted()[2][..., 1].abs().max()) == 0


@pytest.mark.parametrize("base_weight", [1.0, 0.0], ids=["with_base", "lovasz_alone"])
@pytest.mark.parametrize("loss_type", ["ce", "focal"])
def test_bad_label_flag(dev, loss_type, base_weight):
    shape, rows, t, _, _ = CASES["shape1"]
    B, ih, iw, H, W, nc = shape
    crit = SegLoss(loss_type, lovasz=dict(base_weight=base_weight))
    crit.nc = nc
    tb = t.clone()
    tb[0, H - 1, W - 1] = nc + 3
    with pytest.raises(CvxError):
        crit.op(rows.to(dev), tb.to(dev), (ih, iw), SCALE)
    loss_bad, _ = crit.op(rows.to(dev), tb.to(dev), (ih, iw), SCALE, check=False)
    assert crit.bad_targets()
    tskip = tb.clone()
    tskip[0, H - 1, W - 1] = -100                                               # the bad label is skipped: the value is that of an ignored pixel
    loss_skip, _ = crit.op(rows.to(dev), tskip.to(dev), (ih, iw), SCALE, check=False)
    assert not crit.bad_targets() and math.isfinite(float(loss_skip))
    assert torch.equal(loss_bad.view(torch.int32), loss_skip.view(torch.int32))
    with pytest.raises(ValueError):                                                # the length is known at the first call
        SegLoss(loss_type, lovasz=dict(class_weights=[1.0] * (nc + 1))).op(rows.to(dev), t.to(dev), (ih, iw), SCALE)


def ohem_inputs(case):
    shape, seed, min_kept, thresh = case
    rows, t, w = R.make_case(shape, seed)
    return shape, rows, t, w, dict(thresh=thresh, min_kept=min_kept)


COMPOSITIONS = {
    "ce+lovasz": (R.SHAPES[0], "ce", {}, dict(weight=0.7, base_weight=1.3)),
    "ce_weights_smoothing_ohem+lovasz_per_image": (OHEM_UPSAMPLED, "ce", dict(label_smoothing=0.1), dict(per_image=True)),
    "focal+lovasz": (R.SHAPES[3], "focal", {}, dict(weight=1.5)),
}


def compose(dev, shape, rows, t, loss_type, base_kw, lovasz):
    """(the compound criterion, its loss and dpred, the base alone, its loss and dpred, the term alone, its loss and dpred)"""
    B, ih, iw, H, W, nc = shape
    d_rows, d_t = rows.to(dev), t.to(dev)
    out = []
    for kw in (dict(base_kw, lovasz=lovasz), base_kw, dict(lovasz=dict(lovasz, base_weight=0.0))):
        crit = SegLoss(loss_type, **kw)
        crit.nc = nc
        loss, dpred = crit.op(d_rows, d_t, (ih, iw), SCALE)
        out += [crit, loss.clone(), dpred.clone()]
    return out


@pytest.mark.parametrize("name", list(COMPOSITIONS))
def test_composition_with_the_existing_entries(dev, name):
    case, loss_type, opts, lovasz = COMPOSITIONS[name]
    if opts:
        shape, rows, t, w, ohem = ohem_inputs(case)
        base_kw = dict(class_weights=w, label_smoothing=opts["label_smoothing"], ohem=ohem)
    else:
        shape, base_kw = case, {}
        rows, t, w = R.case(shape)
    crit, loss, dpred, base, loss_b, dpred_b, alone, loss_a, dpred_a = compose(dev, shape, rows, t, loss_type, base_kw, lovasz)
    bw = lovasz.get("base_weight", 1.0)
    want = bw * float(loss_b) + float(loss_a)                                     # the term-alone criterion carries `weight` already
    err = abs(float(loss) - want) / abs(want)
    derr = rel(dpred.float(), bw * dpred_b.float() + dpred_a.float())
    print(f"{name}: loss {float(loss):.8f} = {bw} * {float(loss_b):.8f} + {float(loss_a):.8f} (relative error {err:.3g}); dpred relative error {derr:.3g}")
    assert err < 1e-7 and derr < 1e-3
    assert torch.equal(crit.region_stats, alone.region_stats)                     # OHEM selects for the base only: the order runs over all valid pixels
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(live_view(crit), live_view(alone)))
    if opts:
        assert torch.equal(crit.last_stats, base.last_stats) and float(crit.last_stats[0]) < float(crit.last_stats[1])   # pixels were dropped
        assert torch.equal(crit.ohem_keys(), base.ohem_keys())


def test_a_pixel_ohem_drops_carries_exactly_the_lovasz_gradient(dev):
    """Label resolution = logits resolution: the upsampling and its adjoint are the identity, so dpred is the per-pixel gradient."""
    shape, rows, t, w, ohem = ohem_inputs(OHEM_IDENTITY)
    B, ih, iw, H, W, nc = shape
    crit, loss, dpred, base, loss_b, dpred_b, alone, loss_a, dpred_a = compose(dev, shape, rows, t, "ce", dict(class_weights=w, label_smoothing=0.1, ohem=ohem),
                                                                               dict(per_image=True))
    keys, stats = crit.ohem_keys().cpu(), crit.last_stats.cpu()
    theta_t, theta_min = np.float32(abs(math.log(ohem["thresh"]))), np.float32(float(stats[2]))
    kn = keys.numpy()
    valid = kn >= 0
    kept = valid & ((kn > theta_t) | (kn >= theta_min))
    dropped = torch.from_numpy(valid & ~kept).reshape(B, ih * iw)
    assert int(kept.sum()) == int(stats[0]) and 0 < int(dropped.sum()) == int(stats[1]) - int(stats[0])
    comb, lov, bas = dpred.cpu()[..., :nc], dpred_a.cpu()[..., :nc], dpred_b.cpu()[..., :nc]
    assert float(bas[dropped].float().abs().max()) == 0.0                         # the base term is gone there
    print(f"{int(dropped.sum())} dropped pixels: lovasz gradient max {float(lov[dropped].float().abs().max()):.4g} (scaled)")
    assert float(lov[dropped].float().abs().max()) > 0.0
    assert torch.equal(comb[dropped].view(torch.int16), lov[dropped].view(torch.int16))


@pytest.mark.parametrize("cname", ["batch", "per_image_all"])
def test_two_calls_give_the_same_bits(dev, cname):
    shape, rows, t, w, _ = CASES["shape3"]
    B, ih, iw, H, W, nc = shape
    for kw in (dict(), dict(base_weight=0.0)):
        crit = SegLoss("ce", lovasz=dict(R.config(cname, w), **kw))
        crit.nc = nc
        loss, dpred = crit.op(rows.to(dev), t.to(dev), (ih, iw), SCALE)
        first = [loss.clone(), dpred.clone(), crit.region_stats.clone()] + list(live_view(crit))
        crit._ws[4096:].fill_(0xAB)                                                # nothing of the first call is left to lean on
        loss2, dpred2 = crit.op(rows.to(dev), t.to(dev), (ih, iw), SCALE)
        second = [loss2, dpred2, crit.region_stats] + list(live_view(crit))
        for a, b in zip(first, second):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


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
    slots = torch.zeros(3, device=dev)
    for name in ("shape0", "shape3"):
        shape, rows, t, w, _ = CASES[name]
        B, ih, iw, H, W, nc = shape
        d_rows, d_t = rows.to(dev), t.to(dev)
        flipped = torch.flip(d_t, dims=[2]).contiguous()
        for loss_type, kw in (("ce", dict(class_weights=w, label_smoothing=0.1, lovasz=dict(per_image=True, weight=0.8, base_weight=1.2))),
                              ("focal", dict(lovasz={})), ("ce", dict(lovasz=dict(base_weight=0.0, skip_absent=False)))):
            crit, train = SegLoss(loss_type, **kw), SegLoss(loss_type, **kw)
            crit.nc = train.nc = nc
            want = torch.cat([train.op(d_rows, tt, (ih, iw), SCALE)[0].clone() for tt in (d_t, flipped)])
            plain, fused = SegmentationMetrics(nc, device=dev), SegmentationMetrics(nc, device=dev)
            plain.add_rows(d_rows, d_t, (ih, iw), SegLoss("ce"), slots[2:3])
            plain.add_rows(d_rows, flipped, (ih, iw), SegLoss("ce"), slots[2:3])
            SegmentationMetrics(nc, device=dev).add_rows(d_rows, d_t, (ih, iw), crit, slots[2:3])     # the first call allocates and copies the weights
            held = (crit._ws_eval.data_ptr(), crit.region_stats.data_ptr())
            with no_sync(dev) as flagged:
                fused.add_rows(d_rows, d_t, (ih, iw), crit, slots[0:1])
                fused.add_rows(d_rows, flipped, (ih, iw), crit, slots[1:2])
            print(f"validation {name} {loss_type}: slots {slots[:2].tolist()}, training values {want.tolist()}, sync flagged: {flagged}")
            assert torch.equal(slots[:2].view(torch.int32), want.view(torch.int32))
            assert held == (crit._ws_eval.data_ptr(), crit.region_stats.data_ptr()) and crit._ws is None
            assert crit._ws_eval.numel() < train._ws.numel() * 0.6
            assert torch.equal(fused.counts, plain.counts) and int(fused.counts.sum()) == 2 * int((d_t != -100).sum())
            assert torch.equal(crit.region_stats, train.region_stats)


def test_train_steps_end_to_end(dev, gold):
    from computervision.pytorch_amd.deeplab import DeepLabV3PlusR101, SegTrainStep
    from computervision.pytorch_amd.train import DynamicLossScale, FlatAdam
    g = gold("deeplab_train_97x129.npz")
    x, t = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["target"].astype(np.int64)).to(dev)
    torch.manual_seed(0)
    m = DeepLabV3PlusR101(21).to(dev).train()
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    crit = SegLoss("ce", lovasz={})
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
    print(f"sync flagged: {flagged}; losses {losses.tolist()}; mean L_c of the present classes {float(stats[0, stats[0, :, 2] > 0, 3].mean()):.4f}")
    assert bool(torch.isfinite(losses).all())
    n_valid = int(((t != -100) & (t >= 0) & (t < 21)).sum())
    assert int(stats[0, :, 2].sum()) == n_valid
    sc.poll()
    assert sc.skipped == 0 and not crit.bad_targets()
    moved = torch.stack([(p.detach() != before[k]).any() for k, p in m.named_parameters()]).cpu()
    still = [k for (k, _), mv in zip(m.named_parameters(), moved.tolist()) if not mv]
    assert not still, still
