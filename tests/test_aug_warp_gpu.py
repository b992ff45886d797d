"""GPU (MI355X): stage 2 of the device augmentation -- ``cvx_aug_warp_mix`` and ``cvx_aug_boxes_warp`` through ``DeviceAugmenter.apply(warp=...)``
against the host restatement (tests/aug_warp_restatement.py on tests/aug_restatement.py), in all four target formats, and
``DeviceAugLoader(close_after=...)`` in front of ``Yolo8Trainer``.

Every comparison of kernel output is bit-exact, and can be: stage 1 is bit-exact against its own restatement (tests/test_augment_gpu.py), and
stage 2 is a fixed sequence of single rounded fp32 operations (the kernel file is compiled with contraction off; fp32 division is correctly
rounded) that numpy repeats on float32 arrays.  Output 64 x 96 (1.5 tiles wide, 4 tiles tall) and 50 x 70 (a multiple of neither side of the
64 x 16 tile); sources are the synthetic pictures of aug_restatement.py.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aug_restatement as R  # noqa: E402
import aug_warp_restatement as WR  # noqa: E402
from computervision.pytorch_amd.augment import DeviceAugLoader, DeviceAugmenter  # noqa: E402

F = np.float32
SRC = {"a": R.synth_picture(37, 53, 11), "b": R.synth_picture(64, 48, 12), "c": R.synth_picture(96, 96, 13), "d": R.synth_picture(5, 7, 14),
       "e": R.synth_picture(96, 96, 15)}
LUT = R.make_lut((1.05, 1.3, 0.8))
NO_BOXES = np.zeros((0, 5), F)
SIZES = [(64, 96), (50, 70)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def plain(src, nh, nw, dx, dy, hw, flip=0):
    ih, iw = SRC[src].shape[:2]
    return [dict(ih=ih, iw=iw, nh=nh, nw=nw, dx=dx, dy=dy, flip=flip, quad=-1, rect=(0, 0, hw[1], hw[0]))], [src]


def mosaic(srcs, sizes, fx, fy, flips, hw):
    h, w = hw
    cx, cy = int(w * fx), int(h * fy)
    rects = [(0, 0, cx, cy), (0, cy, cx, h), (cx, cy, w, h), (cx, 0, w, cy)]
    jobs = []
    for q, (s, (nh, nw), f) in enumerate(zip(srcs, sizes, flips)):
        ih, iw = SRC[s].shape[:2]
        jobs.append(dict(ih=ih, iw=iw, nh=nh, nw=nw, dx=cx - nw if q <= 1 else cx, dy=cy - nh if q in (0, 3) else cy, flip=f, quad=q, rect=rects[q]))
    return jobs, list(srcs)


def warp_of(Ms, s=None, partner=None, r=None):
    """hand-made matrices -> what ``apply(warp=...)`` takes; the float64 inverse is made here, once, for the device and the restatement"""
    M = np.asarray(Ms, np.float64).reshape(-1, 3, 3)
    B = len(M)
    r = np.ones(B, F) if r is None else np.asarray(r, F)
    return {"M": M, "Minv": np.linalg.inv(M), "s": np.ones(B) if s is None else np.asarray(s, np.float64),
            "partner": np.full(B, -1) if partner is None else np.asarray(partner), "r": r, "r1": F(1) - r}


def prepare(dev, outputs, boxes=None):
    """hand-made jobs -> the arguments of ``apply``, the pictures uploaded"""
    params = [{"jobs": jobs, "lut": lut} for (jobs, _), lut in outputs]
    srcs = [[torch.from_numpy(SRC[s]).to(dev) for s in keys] for (_, keys), _ in outputs]
    if boxes is None:
        boxes = [[NO_BOXES] * len(jobs) for (jobs, _), _ in outputs]
    return params, srcs, boxes


def run(dev, outputs, hw, boxes=None, warp=None, fmt="yolo7", **kw):
    apply_kw = {k: kw.pop(k) for k in ("max_boxes", "exact") if k in kw}
    aug = DeviceAugmenter(hw, **kw)
    images, targets = aug.apply(*prepare(dev, outputs, boxes), fmt=fmt, warp=warp, **apply_kw)
    return images, targets, aug


def canvases_of(outputs, hw):
    """stage 1's canvases by its own restatement, (B, 3, H, W) fp32"""
    return np.stack([R.to_tensor(R.render(jobs, [SRC[k] for k in keys], lut, hw[0], hw[1])) for (jobs, keys), lut in outputs])


def labels_of(outputs, boxes, hw):
    """stage 1's labels per canvas by its own restatement, rows [cls, cx, cy, w, h]"""
    rows = R.targets([list(zip(jobs, bs)) for ((jobs, _), _), bs in zip(outputs, boxes)], hw[0], hw[1])
    return [rows[rows[:, 0] == i, 1:] for i in range(len(outputs))]


# ---- 1. images: one canvas, five matrices, two sizes --------------------------------------------------------------
def image_matrix(name, hw):
    h, w = hw
    return {"identity": np.eye(3),
            "integer_shift": np.array([[1, 0, 7], [0, 1, -5], [0, 0, 1]], np.float64),
            "rotation_zoom_shear": WR.matrix((0, 0, 17, 1.2, 6, -4, 0.53, 0.46), h, w),
            "zoom_below_half": WR.matrix((0, 0, -8, 0.4, 0, 0, 0.5, 0.5), h, w),
            "perspective": WR.matrix((0.003, -0.002, 5, 0.9, 2, 1, 0.52, 0.49), h, w)}[name]


@functools.lru_cache(maxsize=None)
def single_canvas(hw):
    outputs = [(plain("a", 40, 58, 10, 7, hw) if hw == (64, 96) else plain("a", 40, 58, 5, 4, hw), LUT)]
    return outputs, canvases_of(outputs, hw)


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["identity", "integer_shift", "rotation_zoom_shear", "zoom_below_half", "perspective"])
def test_warped_image_equals_the_restatement_bit_for_bit(dev, name, hw):
    outputs, canvases = single_canvas(hw)
    warp = warp_of(image_matrix(name, hw))
    images, rows, aug = run(dev, outputs, hw, warp=warp)
    assert images.shape == (1, 3) + hw and images.dtype == torch.float32 and images.device == dev and rows.shape == (0, 6)
    got = images.cpu().numpy()
    ref = WR.warp_mix(canvases, warp["Minv"])
    grey = float((ref[0, 0] == WR.GREY).mean())
    print(f"{name} {hw}: {int((got != ref).sum())} differing values of {ref.size}, border share {grey:.2f}")
    assert np.array_equal(got, ref)
    assert aug.last_warp is warp
    if name == "identity":
        stage1, _, aug1 = run(dev, outputs, hw)
        assert torch.equal(images, stage1) and np.array_equal(got, canvases) and aug1.last_warp is None
    if name == "integer_shift":
        assert np.array_equal(got[0, :, :hw[0] - 5, 7:], canvases[0, :, 5:, :hw[1] - 7]) and (got[0, :, :, :7] == WR.GREY).all()
    if name == "zoom_below_half":
        assert grey > 0.5
    if name in ("rotation_zoom_shear", "perspective"):
        assert 0.02 < grey < 0.6 and not np.array_equal(got, canvases)


# ---- 2. batches: MixUp inside the batch ----------------------------------------------------------------------------
def test_batch_of_three_with_a_canvas_that_is_output_and_partner(dev):
    hw = (64, 96)
    m = mosaic("cabe", [(50, 40), (30, 33), (41, 77), (60, 61)], 0.3, 0.7, [0, 1, 0, 0], hw)
    outputs = [(plain("a", 40, 58, 10, 7, hw), LUT), (m, R.make_lut((0.95, 0.6, 1.2))), (plain("b", 50, 37, 30, 9, hw, flip=1), R.identity_lut())]
    Ms = [WR.matrix((0.001, 0, 10, 1.1, 3, 0, 0.5, 0.55), *hw), WR.matrix((0, 0.002, -20, 0.8, 0, 5, 0.45, 0.5), *hw), np.eye(3)]
    warp = warp_of(Ms, partner=[1, -1, 1], r=[0.53, 1.0, 0.4375])
    images, _, _ = run(dev, outputs, hw, warp=warp)
    canvases = canvases_of(outputs, hw)
    ref = WR.warp_mix(canvases, warp["Minv"], warp["partner"], warp["r"], warp["r1"])
    got = images.cpu().numpy()
    assert np.array_equal(got, ref)
    own = WR.warp_mix(canvases, warp["Minv"])
    assert np.array_equal(got[1], own[1]) and not np.array_equal(got[0], own[0]) and not np.array_equal(got[2], canvases[2])
    assert np.array_equal(got[2], canvases[2] * F(0.4375) + own[1] * (F(1) - F(0.4375)))       # each canvas through its own matrix


def test_mutual_pair(dev):
    hw = (50, 70)
    outputs = [(plain("a", 40, 58, 5, 4, hw), LUT), (plain("c", 45, 60, -3, 8, hw, flip=1), LUT)]
    Ms = [WR.matrix((0, 0, 30, 0.9, 0, 0, 0.5, 0.5), *hw), WR.matrix((0.002, 0.001, -12, 1.3, 4, 4, 0.55, 0.45), *hw)]
    warp = warp_of(Ms, partner=[1, 0], r=[0.47, 0.61])
    images, _, _ = run(dev, outputs, hw, warp=warp)
    ref = WR.warp_mix(canvases_of(outputs, hw), warp["Minv"], warp["partner"], warp["r"], warp["r1"])
    assert np.array_equal(images.cpu().numpy(), ref) and not np.array_equal(ref[0], ref[1])


# ---- 3. boxes -------------------------------------------------------------------------------------------------------
def box_batch(hw=(64, 96)):
    """five outputs: 300 boxes (two chunks of the scan) with a partner that has none; a mosaic with the first as partner; no boxes, partner
    the mosaic; a few boxes, no partner; no boxes, no partner"""
    m = mosaic("cabe", [(50, 40), (30, 33), (41, 77), (60, 61)], 0.3, 0.7, [1, 0, 0, 1], hw)
    outputs = [(plain("c", 80, 90, -5, -9, hw, flip=1), LUT), (m, LUT), (plain("a", 40, 58, 10, 7, hw), LUT), (plain("b", 60, 45, 20, 2, hw), LUT),
               (plain("d", 33, 20, 60, 25, hw), LUT)]
    boxes = [[R.synth_boxes(96, 96, 300, 21)], [R.synth_boxes(*SRC[k].shape[:2], 7, 22 + i) for i, k in enumerate(m[1])], [NO_BOXES],
             [R.synth_boxes(64, 48, 6, 27)], [NO_BOXES]]
    eights = [(0.001, -0.001, 12, 0.9, 3, -2, 1.0, 0.15), (0, 0.002, -25, 0.7, 0, 6, 0.3, 0.6), (0, 0, 5, 1.4, 0, 0, 0.5, 0.5),
              (-0.002, 0, 40, 1.2, -5, 5, 0.6, 0.4), (0, 0, 0, 1, 0, 0, 0.5, 0.5)]
    warp = warp_of([WR.matrix(e, *hw) for e in eights], s=[e[3] for e in eights], partner=[2, 0, 1, -1, -1], r=[0.5, 0.45, 0.6, 1, 1])
    return outputs, boxes, warp


@functools.lru_cache(maxsize=None)
def box_reference():
    hw = (64, 96)
    outputs, boxes, warp = box_batch(hw)
    stage1 = labels_of(outputs, boxes, hw)
    per = WR.boxes_per_output(stage1, warp["M"], warp["s"].astype(F), warp["partner"], *hw)
    return stage1, per


def test_compact_formats(dev):
    hw = (64, 96)
    outputs, boxes, warp = box_batch(hw)
    stage1, per = box_reference()
    ref = WR.compact(per)
    n_src = [sum(len(b) for b in bs) for bs in boxes]
    kept1, kept = [len(s) for s in stage1], [len(k) for k in per]
    print("source boxes", n_src, "after stage 1", kept1, "after stage 2 (own + partner)", kept)
    assert kept1[0] > 256 and kept1[2] == 0 and kept1[4] == 0 and kept[4] == 0 and 0 < kept[2] <= kept1[1]
    assert 0 < kept[0] < kept1[0] and kept[1] == kept[2] + kept[0]           # some dropped; output 1 carries canvas 0's boxes behind its own
    _, t7, aug = run(dev, outputs, hw, boxes, warp, fmt="yolo7")
    assert t7.device == dev and int(aug.last_count.item()) == len(ref) == t7.shape[0]
    assert np.array_equal(t7.cpu().numpy(), ref)
    assert np.array_equal(ref[:, 0], np.sort(ref[:, 0]))
    _, t8, _ = run(dev, outputs, hw, boxes, warp, fmt="yolo8")
    assert t8["batch_idx"].shape == (len(ref),) and t8["cls"].shape == (len(ref), 1) and t8["bboxes"].shape == (len(ref), 4)
    assert np.array_equal(torch.cat((t8["batch_idx"][:, None], t8["cls"], t8["bboxes"]), 1).cpu().numpy(), ref)
    _, pad, _ = run(dev, outputs, hw, boxes, warp, fmt="yolo7", exact=False)       # no read-back: all rows, unused ones carry image -1
    rows = n_src[0] + n_src[2] + n_src[1] + n_src[0] + n_src[2] + n_src[1] + n_src[3] + n_src[4]
    assert pad.shape == (rows, 6) and np.array_equal(pad[:len(ref)].cpu().numpy(), ref) and bool((pad[len(ref):, 0] == -1).all())
    assert not pad[len(ref):, 1:].any()


def test_padded_format_and_overflow(dev):
    hw = (64, 96)
    outputs, boxes, warp = box_batch(hw)
    _, per = box_reference()
    kept = [len(k) for k in per]
    _, (labels, counts), aug = run(dev, outputs, hw, boxes, warp, fmt="padded")
    cap = 300 + 28                                                             # the largest n_i + n_p(i) of source boxes: output 1
    ref_labels, ref_counts, ref_over = WR.padded(per, cap)
    assert labels.shape == (5, cap, 5) and counts.dtype == torch.int32 and ref_over == 0 and int(aug.last_overflow.item()) == 0
    assert np.array_equal(counts.cpu().numpy(), ref_counts) and counts.cpu().tolist() == kept and aug.last_count is counts
    assert np.array_equal(labels.cpu().numpy(), ref_labels)                    # order, values and the zero fill
    cap = kept[2] + 1                                                          # outputs 0 and 1 overflow, 2 and 3 do not
    _, (labels, counts), aug = run(dev, outputs, hw, boxes, warp, fmt="padded", max_boxes=cap)
    ref_labels, ref_counts, ref_over = WR.padded(per, cap)
    assert ref_over == 1 and int(aug.last_overflow.item()) != 0 and counts.cpu().tolist() == [cap, cap, kept[2], min(kept[3], cap), 0]
    assert np.array_equal(labels.cpu().numpy(), ref_labels) and np.array_equal(counts.cpu().numpy(), ref_counts)


def sync_debug(dev):
    """whether torch.cuda.set_sync_debug_mode("error") flags a read-back on this build"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=dev).item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def apply_without_sync(dev, aug, outputs, boxes, warp, fmt):
    """a first call for the library, the priors and the code objects, then the call under the debug mode where the build has it"""
    args = prepare(dev, outputs, boxes)
    aug.apply(*args, fmt=fmt, warp=warp)
    if not sync_debug(dev):
        print("set_sync_debug_mode('error') flags nothing on this build: plain call")
        return aug.apply(*args, fmt=fmt, warp=warp)
    torch.cuda.set_sync_debug_mode("error")
    try:
        return aug.apply(*args, fmt=fmt, warp=warp)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def algorithm(name, dev, hw=None, max_boxes=None):
    import builder
    cfg, alg_cls, _ = builder.export_from_registry(name)
    if hw is not None:
        cfg.arch.input_size = (3,) + tuple(hw)
    if max_boxes is not None:
        cfg.train.max_num_boxes = max_boxes
    return alg_cls(cfg, dev)


def target_batch(hw):
    """three outputs: boxes and a partner without any; a mosaic whose partner is the first; no boxes, no partner"""
    h, w = hw
    m = mosaic("cabe", [(h // 2, w // 2), (h // 3, w // 2), (h // 2, w // 2), (h // 2, w // 3)], 0.45, 0.55, [1, 0, 0, 1], hw)
    outputs = [(plain("c", h - 20, w - 20, 10, 5, hw, flip=1), LUT), (m, LUT), (plain("a", h // 2, w // 2, 5, 9, hw), LUT)]
    boxes = [[R.synth_boxes(96, 96, 9, 31)], [R.synth_boxes(*SRC[k].shape[:2], 3, 32 + i) for i, k in enumerate(m[1])], [NO_BOXES]]
    eights = [(0, 0, 8, 0.6, 2, -2, 0.8, 0.4), (0.0005, 0, -10, 1.1, 0, 3, 0.4, 0.5), (0, 0, 0, 1, 0, 0, 0.5, 0.5)]
    warp = warp_of([WR.matrix(e, h, w) for e in eights], s=[e[3] for e in eights], partner=[2, 0, -1], r=[0.5, 0.55, 1])
    per = WR.boxes_per_output(labels_of(outputs, boxes, hw), warp["M"], warp["s"].astype(F), warp["partner"], h, w)
    return outputs, boxes, warp, per


def test_ssd_targets_never_overflow_and_do_not_synchronise(dev):
    hw = (300, 300)
    outputs, boxes, warp, per = target_batch(hw)
    kept = [len(k) for k in per]
    print("kept per output", kept)
    assert kept[0] > 0 and kept[1] > kept[0] and kept[2] == 0
    ssd = algorithm("ssd", dev)
    aug = DeviceAugmenter(hw, target=ssd)
    images, y_true = apply_without_sync(dev, aug, outputs, boxes, warp, "ssd")
    ref_labels, ref_counts, _ = WR.padded(per, 9 + 12)                         # the largest n_i + n_p(i) of source boxes
    ref = ssd.encode_targets(torch.from_numpy(ref_labels).to(dev), torch.from_numpy(ref_counts).to(dev))
    assert y_true.shape == (3, 8732, 4 + 21 + 1) and torch.equal(y_true, ref)
    assert aug.last_count.cpu().tolist() == kept and int(aug.last_overflow.item()) == 0       # every kept box has its row
    assert int(y_true[2, :, -1].sum()) == 0 and int(y_true[1, :, -1].sum()) > 0
    _, (labels, counts), _ = run(dev, outputs, hw, boxes, warp, fmt="padded")
    assert labels.shape == (3, 21, 5) and np.array_equal(labels.cpu().numpy(), ref_labels)


def test_centernet_keeps_the_first_k_and_does_not_synchronise(dev):
    hw = (128, 160)
    outputs, boxes, warp, per = target_batch(hw)
    kept = [len(k) for k in per]
    print("kept per output", kept)
    assert kept[1] > 4 and kept[2] == 0
    cn = algorithm("centernet", dev, hw, max_boxes=4)
    aug = DeviceAugmenter(hw, target=cn)
    _, got = apply_without_sync(dev, aug, outputs, boxes, warp, "centernet")
    ref_labels, ref_counts, ref_over = WR.padded(per, 4)
    ref = cn.draw_targets(torch.from_numpy(ref_labels).to(dev), torch.from_numpy(ref_counts).to(dev))
    assert len(got) == 5 == len(ref)
    for name, g, r in zip(("heatmap", "reg", "wh", "reg_mask", "indices"), got, ref):
        assert g.shape == r.shape and g.dtype == r.dtype and torch.equal(g, r), name
    assert ref_over == 1 and int(aug.last_overflow.item()) != 0 and aug.last_count.cpu().tolist() == [min(k, 4) for k in kept]
    _, (labels, _), _ = run(dev, outputs, hw, boxes, warp, fmt="padded", max_boxes=4)
    assert np.array_equal(labels.cpu().numpy(), ref_labels)                    # the first K, in order


# ---- 4. the options off ------------------------------------------------------------------------------------------------
def test_options_off_is_the_augmenter_of_before(dev):
    hw = (64, 96)
    pictures = [torch.from_numpy(SRC[k]).to(dev) for k in "cab"]
    boxes = [R.synth_boxes(*SRC[k].shape[:2], 6, 50 + i) for i, k in enumerate("cab")]
    groups = [pictures[2], pictures[0], [pictures[1], pictures[2], pictures[0], pictures[1]]]
    bgroups = [boxes[2], boxes[0], [boxes[1], boxes[2], boxes[0], boxes[1]]]
    old, new = DeviceAugmenter(hw, mosaic=True, seed=5), DeviceAugmenter(hw, mosaic=True, seed=5, affine=None, mixup=0.0)
    for fmt in ("yolo7", "padded"):
        (ia, ta), (ib, tb) = old(groups, bgroups, fmt=fmt), new(groups, bgroups, fmt=fmt)
        assert torch.equal(ia, ib) and new.last_warp is None
        assert torch.equal(ta, tb) if fmt == "yolo7" else (torch.equal(ta[0], tb[0]) and torch.equal(ta[1], tb[1]))
    assert old.rng.rand() == new.rng.rand()
    on = DeviceAugmenter(hw, mosaic=True, seed=5, affine={}, mixup=1.0)
    ic, _ = on(groups, bgroups, fmt="yolo7")
    assert on.last_warp is not None and sorted(on.last_warp["partner"].tolist()) != [-1, -1, -1] and not torch.equal(ic, ia)
    assert bool(torch.isfinite(ic).all()) and 0.0 <= float(ic.min()) and float(ic.max()) <= 1.0


# ---- 5. the loader in front of the trainer --------------------------------------------------------------------------------
def test_yolo8_trainer_on_a_loader_that_closes_the_mosaic(dev, tmp_path):
    """batch 2 at 128 x 128 (the smallest input the trainer's tests pin; the graph takes multiples of 32): one step on an epoch with mosaic, warp
    and MixUp, then an epoch past close_after"""
    import builder
    hw = (128, 128)
    cfg, _, trainer_cls = builder.export_from_registry("yolo8_det")
    cfg.arch.input_size = (3,) + hw
    cfg.train.batch_size, cfg.train.epoch, cfg.train.pretrained = 2, 1, False
    cfg.train.save_path = str(tmp_path)
    cfg.engine.init_loss_scale = 1024.0
    sizes = [(37, 53), (64, 48), (96, 96), (80, 120), (50, 50)]
    source = [(torch.from_numpy(R.synth_picture(h, w, 30 + i)).to(dev), R.synth_boxes(h, w, 4 if i != 3 else 0, 40 + i)) for i, (h, w) in enumerate(sizes)]
    aug = DeviceAugmenter(hw, mosaic=True, mosaic_prob=1.0, seed=3, affine=dict(degrees=10, shear=2, perspective=0.0005), mixup=1.0)
    loader = DeviceAugLoader(source, 2, aug, length=1, fmt="yolo8", device=dev, close_after=1)
    torch.manual_seed(0)
    tr = trainer_cls(cfg, dev, dataloader=loader)
    before = tr.model.flat_params.clone()
    tr.train(max_iters=1)
    torch.cuda.synchronize()
    assert loader.epoch == 1 and tr.optimizer.device_step() == 1
    assert sorted(aug.last_warp["partner"].tolist()) == [0, 1]                  # mixup = 1.0, batch 2: each is the other's partner
    assert bool(torch.isfinite(tr.model.flat_params).all()) and not torch.equal(before, tr.model.flat_params)
    batches = []
    for batch in loader:                                                        # the second epoch: closed
        batches.append(batch)
        assert aug.last_warp is not None and aug.last_warp["partner"].tolist() == [-1, -1]
    assert loader.epoch == 2 and len(batches) == 1
    images, targets = batches[0]
    assert images.shape == (2, 3) + hw and bool(torch.isfinite(images).all())
    tr.model.train()
    values = [float(v) for v in tr.train_loop(batches[0], None)]
    print("loss values", values)
    assert values and all(np.isfinite(v) for v in values)
