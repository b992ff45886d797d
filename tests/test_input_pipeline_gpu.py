"""GPU (MI355X): the input pipeline of the SSD and CenterNet trainers and the validation path of all four detection trainers --
``cvx_aug_images_plain`` and ``cvx_aug_boxes_padded`` through ``DeviceAugmenter`` against the host restatement
(tests/input_pipeline_restatement.py on tests/aug_restatement.py) and the reference fixtures (tests/golden/aug_val_ref.npz, aug_ref.npz),
``fmt="ssd"`` / ``fmt="centernet"`` against ``Ssd.encode_targets`` / ``CenterNetA.draw_targets`` on the same rows, and ``DeviceAugLoader`` in
front of the trainers as ``dataloader=`` and ``val_dataloader=``.

Every comparison of kernel output is bit-exact, and can be: the image path without colour is integer arithmetic and one fp32 division
(``out == byte / 255``), the padded box kernel runs the compact kernel's device function, and the target kernels are deterministic functions
of the (labels, counts) they are handed.  Output 64 x 96 (H != W, 1.5 tiles wide, 4 tiles tall) unless a model fixes the size.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aug_restatement as R  # noqa: E402
import input_pipeline_restatement as P  # noqa: E402
from computervision.pytorch_amd.augment import DeviceAugLoader, DeviceAugmenter  # noqa: E402

H, W = 64, 96
SRC = {"a": R.synth_picture(37, 53, 11), "b": R.synth_picture(64, 48, 12), "c": R.synth_picture(96, 96, 13), "d": R.synth_picture(5, 7, 14),
       "e": R.synth_picture(96, 96, 15), "land": R.synth_picture(48, 120, 16), "same": R.synth_picture(64, 96, 17)}
LUT = R.make_lut((1.05, 1.3, 0.8))
NO_BOXES = np.zeros((0, 5), np.float32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def plain(src, nh, nw, dx, dy, flip=0, hw=(H, W)):
    ih, iw = SRC[src].shape[:2]
    return [dict(ih=ih, iw=iw, nh=nh, nw=nw, dx=dx, dy=dy, flip=flip, quad=-1, rect=(0, 0, hw[1], hw[0]))], [src]


def mosaic(srcs, sizes, fx, fy, flips, hw=(H, W)):
    """jobs placed as mosaic_body does (detection_dataset.py:248-263) around cuts at (fx, fy)"""
    h, w = hw
    cx, cy = int(w * fx), int(h * fy)
    rects = [(0, 0, cx, cy), (0, cy, cx, h), (cx, cy, w, h), (cx, 0, w, cy)]
    jobs = []
    for q, (s, (nh, nw), f) in enumerate(zip(srcs, sizes, flips)):
        ih, iw = SRC[s].shape[:2]
        jobs.append(dict(ih=ih, iw=iw, nh=nh, nw=nw, dx=cx - nw if q <= 1 else cx, dy=cy - nh if q in (0, 3) else cy, flip=f, quad=q, rect=rects[q]))
    return jobs, list(srcs)


def run(dev, outputs, boxes=None, fmt="yolo7", hw=(H, W), **kw):
    """outputs: [((jobs, source keys | arrays), lut)] -> DeviceAugmenter(**kw).apply on the device"""
    apply_kw = {k: kw.pop(k) for k in ("max_boxes", "exact") if k in kw}
    aug = DeviceAugmenter(hw, **kw)
    params = [{"jobs": jobs, "lut": lut} for (jobs, _), lut in outputs]
    srcs = [[torch.from_numpy(SRC[s] if isinstance(s, str) else s).to(dev) for s in keys] for (_, keys), _ in outputs]
    if boxes is None:
        boxes = [[NO_BOXES] * len(jobs) for (jobs, _), _ in outputs]
    images, targets = aug.apply(params, srcs, boxes, fmt=fmt, **apply_kw)
    return images, targets, aug


def as_bytes(image):
    return np.rint(image * 255).astype(np.int64).transpose(1, 2, 0)


# ---- 1. images without the colour transform --------------------------------------------------------------
VAL_SOURCES = {"upscale_bars_left_right": ["a"], "downscale_bars_top_bottom": ["land"], "identity": ["same"], "batch3_different_sizes": ["a", "land", "c"]}


@pytest.mark.parametrize("name", list(VAL_SOURCES))
def test_plain_images_equal_the_restatement_to_the_byte(dev, name):
    keys = VAL_SOURCES[name]
    aug = DeviceAugmenter((H, W), train=False)
    images, rows = aug([torch.from_numpy(SRC[k]).to(dev) for k in keys], [NO_BOXES] * len(keys), fmt="yolo7")
    assert images.shape == (len(keys), 3, H, W) and images.dtype == torch.float32 and images.device == dev and rows.shape == (0, 6)
    got = images.cpu().numpy()
    for i, k in enumerate(keys):
        jb = P.val_job(*SRC[k].shape[:2], H, W)
        ref = P.render_plain([jb], [SRC[k]], H, W)
        bad = np.argwhere(as_bytes(got[i]) != ref)
        print(f"{name}[{i}]: job {jb}, {len(bad)} differing bytes of {ref.size}")
        assert len(bad) == 0 and np.array_equal(got[i], R.to_tensor(ref))          # out == byte / 255 exactly
    if name == "identity":
        assert np.array_equal(as_bytes(got[0]), SRC["same"])                       # same size: the picture itself, which the HSV path would not return
    if name == "upscale_bars_left_right":
        assert jb["dx"] > 0 and jb["dy"] == 0 and jb["nh"] > jb["ih"] and (as_bytes(got[0])[:, :jb["dx"]] == 128).all()
    if name == "downscale_bars_top_bottom":
        assert jb["dy"] > 0 and jb["dx"] == 0 and jb["nw"] < jb["iw"] and (as_bytes(got[0])[:jb["dy"]] == 128).all()


def test_plain_images_share_the_flips_and_the_mosaic_composition(dev):
    """the template instance without colour, on hand-made training jobs: canvas flip with an overhang, and a mosaic with mirrored sources"""
    outputs = [(plain("c", 70, 90, 20, -9, flip=1), LUT), (mosaic("ecba", [(30, 52), (45, 40), (28, 31), (40, 70)], 0.5, 0.5, [1, 0, 1, 0]), LUT)]
    images, _, _ = run(dev, outputs, train=False)
    for i, ((jobs, keys), _) in enumerate(outputs):
        assert np.array_equal(images[i].cpu().numpy(), R.to_tensor(P.render_plain(jobs, [SRC[k] for k in keys], H, W)))


def test_plain_images_equal_the_validation_fixture(dev, gold):
    fh, fw, cases = P.load_val_cases(gold("aug_val_ref.npz"))
    assert (fh, fw) == (H, W)
    picked = [c for c in cases if c["image"] is not None]
    aug = DeviceAugmenter((H, W), train=False)
    images, _ = aug([torch.from_numpy(c["picture"]).to(dev) for c in picked], [NO_BOXES] * len(picked), fmt="yolo7")
    assert len(picked) == 3
    for i, c in enumerate(picked):
        assert np.array_equal(images[i].cpu().numpy(), R.to_tensor(c["image"]))    # the reference's 0...255 picture / 255


# ---- 2. the colour path is what it was ---------------------------------------------------------------------
def test_colour_path_unchanged(dev):
    outputs = [(plain("a", 40, 58, 10, 7), LUT), (mosaic("cabe", [(50, 40), (30, 33), (41, 77), (60, 61)], 0.3, 0.7, [0, 0, 0, 0]), R.make_lut((1.1, 0.3, 1.4)))]
    images, _, _ = run(dev, outputs)
    for i, ((jobs, keys), lut) in enumerate(outputs):
        ref = R.render(jobs, [SRC[k] for k in keys], lut, H, W)
        assert np.array_equal(images[i].cpu().numpy(), R.to_tensor(ref))
        assert not np.array_equal(ref, P.render_plain(jobs, [SRC[k] for k in keys], H, W))


# ---- 3. padded boxes = compact boxes, regrouped -------------------------------------------------------------
def padded_batch():
    """plain image with 300 boxes (two chunks of the scan), mosaic image, image without boxes, image whose boxes are all discarded"""
    m = mosaic("cabe", [(50, 40), (30, 33), (41, 77), (60, 61)], 0.3, 0.7, [1, 0, 0, 1])
    tiny_boxes = np.array([[10, 10, 18, 60, 3], [50, 5, 59, 90, 4], [0, 0, 9, 9, 5]], np.float32)       # 96 -> 10 pixels: under 1 px wide
    outputs = [(plain("c", 80, 90, -5, -9, flip=1), LUT), (m, LUT), (plain("a", 40, 58, 10, 7), LUT), (plain("c", 9, 10, 40, 30), LUT)]
    boxes = [[R.synth_boxes(96, 96, 300, 21)], [R.synth_boxes(*SRC[k].shape[:2], 7, 22 + i) for i, k in enumerate(m[1])], [NO_BOXES], [tiny_boxes]]
    return outputs, boxes


def test_padded_boxes_equal_compact_boxes_regrouped(dev):
    outputs, boxes = padded_batch()
    _, rows, _ = run(dev, outputs, boxes, fmt="yolo7")
    rows = rows.cpu().numpy()
    ref_rows = R.targets([list(zip(jobs, bs)) for ((jobs, _), _), bs in zip(outputs, boxes)], H, W)
    assert np.array_equal(rows, ref_rows)
    kept = [int((rows[:, 0] == b).sum()) for b in range(4)]
    print("kept per image", kept)
    assert 256 < kept[0] < 300 and 4 < kept[1] < 28 and kept[2] == 0 and kept[3] == 0
    _, (labels, counts), aug = run(dev, outputs, boxes, fmt="padded")
    assert labels.shape == (4, 300, 5) and labels.dtype == torch.float32 and counts.dtype == torch.int32 and labels.device == dev
    ref_labels, ref_counts, ref_over = P.regroup(rows, 4, 300)
    assert np.array_equal(counts.cpu().numpy(), ref_counts) and counts.cpu().tolist() == kept
    assert np.array_equal(labels.cpu().numpy(), ref_labels)                        # order, values and the zero fill
    assert ref_over == 0 and int(aug.last_overflow.item()) == 0 and aug.last_count is counts
    # a capacity below image 0's and image 1's kept count, above nothing else
    cap = kept[1] - 2
    _, (labels, counts), aug = run(dev, outputs, boxes, fmt="padded", max_boxes=cap)
    ref_labels, ref_counts, ref_over = P.regroup(rows, 4, cap)
    assert ref_over == 1 and int(aug.last_overflow.item()) != 0
    assert counts.cpu().tolist() == [cap, cap, 0, 0] and np.array_equal(counts.cpu().numpy(), ref_counts)
    assert np.array_equal(labels.cpu().numpy(), ref_labels)
    # only image 0 overflows: the others are what they were
    cap = kept[1] + 3
    _, (labels, counts), aug = run(dev, outputs, boxes, fmt="padded", max_boxes=cap)
    ref_labels, ref_counts, _ = P.regroup(rows, 4, cap)
    assert counts.cpu().tolist() == [cap, kept[1], 0, 0] and int(aug.last_overflow.item()) != 0
    assert np.array_equal(labels.cpu().numpy(), ref_labels) and not labels[1, kept[1]:].any()


# ---- 4. / 5. the target formats ------------------------------------------------------------------------------
def algorithm(name, dev, hw=None, max_boxes=None):
    import builder
    cfg, alg_cls, _ = builder.export_from_registry(name)
    if hw is not None:
        cfg.arch.input_size = (3,) + tuple(hw)
    if max_boxes is not None:
        cfg.train.max_num_boxes = max_boxes
    return alg_cls(cfg, dev)


def test_ssd_targets_equal_encode_targets_on_the_same_rows(dev):
    """SSD300, batch 3: plain, mosaic, an image without boxes"""
    hw = (300, 300)
    m = mosaic("cabe", [(160, 150), (120, 140), (150, 170), (140, 200)], 0.45, 0.55, [1, 0, 0, 1], hw)
    outputs = [(plain("c", 250, 280, 10, 30, flip=1, hw=hw), LUT), (m, LUT), (plain("a", 200, 280, 5, 40, hw=hw), LUT)]
    boxes = [[R.synth_boxes(96, 96, 9, 31)], [R.synth_boxes(*SRC[k].shape[:2], 5, 32 + i) for i, k in enumerate(m[1])], [NO_BOXES]]
    ssd = algorithm("ssd", dev)
    images7, rows, _ = run(dev, outputs, boxes, fmt="yolo7", hw=hw)
    per_image = P.per_image_rows(rows.cpu().numpy(), 3)
    assert len(per_image[0]) > 0 and len(per_image[1]) > 0 and len(per_image[2]) == 0
    ref = ssd.encode_targets([torch.from_numpy(r) for r in per_image])
    images, y_true, aug = run(dev, outputs, boxes, fmt="ssd", hw=hw, target=ssd)
    assert y_true.shape == (3, 8732, 4 + 21 + 1) == ref.shape and y_true.device == dev
    assert torch.equal(y_true, ref) and torch.equal(images, images7)
    assert int(y_true[..., -1].sum()) > 0 and int(y_true[2, :, -1].sum()) == 0 and bool((y_true[2, :, 4] == 1).all())
    assert aug.last_count.cpu().tolist() == [len(r) for r in per_image] and int(aug.last_overflow.item()) == 0
    assert torch.equal(ssd.encode_targets(*run(dev, outputs, boxes, fmt="padded", hw=hw)[1]), ref)       # the device fast path of the class


def test_centernet_targets_equal_draw_targets_on_the_same_rows(dev):
    """128 x 160, K = 4: the plain image keeps more than four boxes and is cut to its first four"""
    hw = (128, 160)
    m = mosaic("cabe", [(70, 60), (50, 66), (60, 90), (64, 80)], 0.4, 0.5, [0, 1, 0, 0], hw)
    outputs = [(plain("c", 110, 140, 10, 9, hw=hw), LUT), (m, LUT), (plain("a", 100, 140, 5, 14, flip=1, hw=hw), LUT)]
    boxes = [[R.synth_boxes(96, 96, 9, 41)], [R.synth_boxes(*SRC[k].shape[:2], 1, 42 + i) for i, k in enumerate(m[1])], [R.synth_boxes(37, 53, 2, 47)]]
    cn = algorithm("centernet", dev, hw, max_boxes=4)
    _, rows, _ = run(dev, outputs, boxes, fmt="yolo7", hw=hw)
    per_image = P.per_image_rows(rows.cpu().numpy(), 3)
    print("kept per image", [len(r) for r in per_image])
    assert len(per_image[0]) > 4 and 0 < len(per_image[1]) <= 4 and 0 < len(per_image[2]) <= 4
    ref = cn.draw_targets([torch.from_numpy(r) for r in per_image])
    _, got, aug = run(dev, outputs, boxes, fmt="centernet", hw=hw, target=cn)
    assert len(got) == 5 == len(ref) and got[0].shape == (3, 32, 40, 20) and got[1].shape == (3, 4, 2)
    for name, g, r in zip(("heatmap", "reg", "wh", "reg_mask", "indices"), got, ref):
        assert g.shape == r.shape and g.dtype == r.dtype and torch.equal(g, r), name
    assert float(got[0].max()) == 1.0 and got[3].sum(1).cpu().tolist() == [4.0, float(len(per_image[1])), float(len(per_image[2]))]
    assert int(aug.last_overflow.item()) != 0 and aug.last_count.cpu().tolist() == [4, len(per_image[1]), len(per_image[2])]
    assert all(torch.equal(g, r) for g, r in zip(cn.draw_targets(*run(dev, outputs, boxes, fmt="padded", hw=hw, max_boxes=4)[1]), ref))


# ---- 6. validation boxes and targets ---------------------------------------------------------------------------
def test_validation_boxes_and_targets_equal_the_fixture(dev, gold):
    _, _, cases = P.load_val_cases(gold("aug_val_ref.npz"))
    pictures, boxes = [torch.from_numpy(c["picture"]).to(dev) for c in cases], [c["boxes"] for c in cases]
    ref = np.concatenate([np.concatenate([np.full((len(c["labels"]), 1), i, np.float32), c["labels"][:, 1:]], 1) for i, c in enumerate(cases)], 0)
    assert any(len(c["boxes"]) == 0 for c in cases) and len(ref) < sum(len(b) for b in boxes)
    images8, t8 = DeviceAugmenter((H, W), train=False)(pictures, boxes, fmt="yolo8")
    assert np.array_equal(torch.cat((t8["batch_idx"][:, None], t8["cls"], t8["bboxes"]), 1).cpu().numpy(), ref)
    _, t7 = DeviceAugmenter((H, W), train=False)(pictures, boxes, fmt="yolo7")
    assert np.array_equal(t7.cpu().numpy(), ref)
    ssd = algorithm("ssd", dev)
    aug = DeviceAugmenter((H, W), train=False, target=ssd)
    images, y_true = aug(pictures, boxes, fmt="ssd")
    assert torch.equal(y_true, ssd.encode_targets([torch.from_numpy(c["labels"]) for c in cases])) and torch.equal(images, images8)
    assert aug.last_count.cpu().tolist() == [len(c["labels"]) for c in cases]
    _, (labels, counts) = DeviceAugmenter((H, W), train=False)(pictures, boxes, fmt="padded")
    for i, c in enumerate(cases):
        n = len(c["labels"])
        assert int(counts[i]) == n and np.array_equal(labels[i, :n].cpu().numpy(), c["labels"][:, 1:]) and not labels[i, n:].any()


# ---- 7. the loader in front of the trainers ---------------------------------------------------------------------
class CountingSource:
    def __init__(self, items):
        self.items, self.visits = items, [0] * len(items)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        self.visits[i] += 1
        return self.items[i]


def picture_source(dev):
    sizes = [(37, 53), (64, 48), (96, 96), (80, 120), (50, 50)]
    return [(torch.from_numpy(R.synth_picture(h, w, 30 + i)).to(dev), R.synth_boxes(h, w, 4 if i != 3 else 0, 40 + i)) for i, (h, w) in enumerate(sizes)]


@pytest.mark.parametrize("name,hw,fmt", [("ssd", (300, 300), "ssd"), ("centernet", (128, 160), "centernet"), ("yolo8_det", (128, 128), "yolo8")])
def test_trainer_on_the_device_loaders(dev, tmp_path, name, hw, fmt):
    """batch 2, two iterations on a training DeviceAugLoader; evaluate_loop on a validation DeviceAugLoader that visits each picture once"""
    import builder
    cfg, alg_cls, trainer_cls = builder.export_from_registry(name)
    cfg.arch.input_size = (3,) + hw
    cfg.train.batch_size, cfg.train.epoch, cfg.train.pretrained = 2, 1, False
    cfg.train.save_path = str(tmp_path)
    if name == "yolo8_det":
        cfg.engine.init_loss_scale = 1024.0
    target = alg_cls(cfg, dev) if fmt in ("ssd", "centernet") else None
    source, val_source = picture_source(dev), CountingSource(picture_source(dev))
    train_loader = DeviceAugLoader(source, 2, DeviceAugmenter(hw, mosaic=True, mosaic_prob=0.5, seed=3, target=target), length=2, fmt=fmt, device=dev)
    val_loader = DeviceAugLoader(val_source, 2, DeviceAugmenter(hw, train=False, target=target), fmt=fmt, device=dev, drop_last=False)
    assert len(val_loader) == 3 and len(DeviceAugLoader(val_source, 2, DeviceAugmenter(hw, train=False, target=target), fmt=fmt, device=dev)) == 2
    torch.manual_seed(0)
    tr = trainer_cls(cfg, dev, dataloader=train_loader, val_dataloader=val_loader)
    assert tr.train_dataloader is train_loader and tr.val_dataloader is val_loader
    before = tr.model.flat_params.clone()
    tr.train(max_iters=2)
    torch.cuda.synchronize()
    assert tr.optimizer.device_step() == 2
    after = tr.model.flat_params
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    tr.model.train()
    values = [float(v) for v in tr.train_loop(next(iter(train_loader)), None)]
    print(name, "train values", values)
    assert values and all(np.isfinite(v) for v in values)
    val_source.visits = [0] * len(val_source)
    result = tr.evaluate_loop()
    print(name, result)
    assert np.isfinite(result["val_loss"]) and result["val_loss"] > 0 and val_source.visits == [1] * 5


# ---- 8. no host synchronisation ------------------------------------------------------------------------------------
def test_target_formats_do_not_synchronise(dev):
    ssd, cn = algorithm("ssd", dev), algorithm("centernet", dev, (128, 160), max_boxes=4)
    pictures = [torch.from_numpy(SRC[k]).to(dev) for k in "cab"]
    boxes = [R.synth_boxes(*SRC[k].shape[:2], 6, 50 + i) for i, k in enumerate("cab")]
    calls = [(DeviceAugmenter((H, W), seed=1, target=ssd), "ssd"), (DeviceAugmenter((H, W), train=False, target=ssd), "ssd"),
             (DeviceAugmenter((128, 160), seed=1, target=cn), "centernet"), (DeviceAugmenter((128, 160), train=False, target=cn), "centernet")]
    for aug, fmt in calls:                                                        # first use: library, priors, kernels' code objects
        aug(pictures, boxes, fmt=fmt)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=dev).item()
            caught = False
        except RuntimeError:
            caught = True
        if not caught:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a read-back on this build")
        results = [aug(pictures, boxes, fmt=fmt) for aug, fmt in calls]
        with pytest.raises(RuntimeError):                                         # the compact formats do read the count back (exact=True)
            DeviceAugmenter((H, W), seed=1)(pictures, boxes, fmt="yolo7")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(images).all()) for images, _ in results)
