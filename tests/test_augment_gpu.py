"""GPU (MI355X): ``cvx_aug_images`` / ``cvx_aug_boxes`` through ``DeviceAugmenter`` against the host restatement (tests/aug_restatement.py)
and the reference fixture (tests/golden/aug_ref.npz), and ``DeviceAugLoader`` feeding the two YOLO trainers.

Every comparison is bit-exact, and can be: the image path is integer arithmetic plus a handful of single fp32 operations in a fixed order
(the kernel file is compiled without contraction), ``out == byte / 255`` exactly, and the box path is the reference's fp32 operation
sequence.  Output 64 x 96 (H != W, 1.5 tiles wide, 4 tiles tall); sources 37 x 53, 64 x 48, 96 x 96 and a 5 x 7 one that is upscaled.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aug_restatement as R  # noqa: E402
from computervision.pytorch_amd.augment import DeviceAugLoader, DeviceAugmenter  # noqa: E402

H, W = 64, 96
SRC = {"a": R.synth_picture(37, 53, 11), "b": R.synth_picture(64, 48, 12), "c": R.synth_picture(96, 96, 13), "d": R.synth_picture(5, 7, 14),
       "e": R.synth_picture(96, 96, 15)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def plain(src, nh, nw, dx, dy, flip=0):
    ih, iw = SRC[src].shape[:2]
    return [dict(ih=ih, iw=iw, nh=nh, nw=nw, dx=dx, dy=dy, flip=flip, quad=-1, rect=(0, 0, W, H))], [src]


def mosaic(srcs, sizes, fx, fy, flips):
    """jobs placed as mosaic_body does (detection_dataset.py:248-263) around cuts at (fx, fy)"""
    cx, cy = int(W * fx), int(H * fy)
    rects = [(0, 0, cx, cy), (0, cy, cx, H), (cx, cy, W, H), (cx, 0, W, cy)]
    jobs = []
    for q, (s, (nh, nw), f) in enumerate(zip(srcs, sizes, flips)):
        ih, iw = SRC[s].shape[:2]
        jobs.append(dict(ih=ih, iw=iw, nh=nh, nw=nw, dx=cx - nw if q <= 1 else cx, dy=cy - nh if q in (0, 3) else cy, flip=f, quad=q, rect=rects[q]))
    return jobs, list(srcs)


LUT = R.make_lut((1.05, 1.3, 0.8))
MOSAIC_37 = mosaic("cabe", [(50, 40), (30, 33), (41, 77), (60, 61)], 0.3, 0.7, [0, 0, 0, 0])
MOSAIC_FLIP = mosaic("ecba", [(30, 52), (45, 40), (28, 31), (40, 70)], 0.5, 0.5, [1, 0, 1, 0])
IMAGE_CASES = {
    "plain": [(plain("a", 40, 58, 10, 7), LUT)],
    "canvas_flip_off_centre": [(plain("b", 50, 37, 3, 9, flip=1), LUT)],
    "negative_dy_overhang": [(plain("c", 80, 90, -5, -9), LUT)],
    "overhang_right_bottom_flipped": [(plain("c", 70, 90, 20, 10, flip=1), LUT)],
    "nw_61": [(plain("a", 43, 61, 17, 11), LUT)],
    "shrink_more_than_2x": [(plain("c", 30, 40, 31, 20), LUT)],
    "upscale_5x7": [(plain("d", 50, 70, 13, 6), LUT)],
    "mosaic_cuts_03_07": [(MOSAIC_37, LUT)],
    "mosaic_source_flipped": [(MOSAIC_FLIP, LUT)],
    "identity_lut": [(plain("c", 60, 85, 4, 2), R.identity_lut())],
    "extreme_lut": [(plain("a", 40, 58, 10, 7), R.make_lut((0.9, 1.7, 0.6))), (MOSAIC_37, R.make_lut((1.1, 0.3, 1.4)))],
    "batch3_mixed": [(plain("b", 50, 37, 30, 9, flip=1), LUT), (MOSAIC_FLIP, R.make_lut((0.95, 0.6, 1.2))), (plain("d", 33, 20, 60, 25), R.identity_lut())],
}


def run(dev, outputs, boxes=None, fmt="yolo7", exact=True):
    """outputs: [((jobs, source keys | arrays), lut)] -> DeviceAugmenter.apply on the device"""
    aug = DeviceAugmenter((H, W))
    params = [{"jobs": jobs, "lut": lut} for (jobs, _), lut in outputs]
    srcs = [[torch.from_numpy(SRC[s] if isinstance(s, str) else s).to(dev) for s in keys] for (_, keys), _ in outputs]
    if boxes is None:
        boxes = [[np.zeros((0, 5), np.float32)] * len(jobs) for (jobs, _), _ in outputs]
    images, targets = aug.apply(params, srcs, boxes, fmt=fmt, exact=exact)
    return images, targets, aug


@pytest.mark.parametrize("name", list(IMAGE_CASES))
def test_images_equal_the_restatement_to_the_byte(dev, name):
    outputs = IMAGE_CASES[name]
    images, _, _ = run(dev, outputs)
    assert images.shape == (len(outputs), 3, H, W) and images.dtype == torch.float32 and images.device == dev
    got = images.cpu().numpy()
    for i, ((jobs, keys), lut) in enumerate(outputs):
        ref_bytes = R.render(jobs, [SRC[k] for k in keys], lut, H, W)
        got_bytes = np.rint(got[i] * 255).astype(np.int64).transpose(1, 2, 0)
        bad = np.argwhere(got_bytes != ref_bytes)
        print(f"{name}[{i}]: {len(bad)} differing bytes of {ref_bytes.size}" + (f", first at {bad[0]}: {got_bytes[tuple(bad[0])]} vs {ref_bytes[tuple(bad[0])]}" if len(bad) else ""))
        assert len(bad) == 0
        assert np.array_equal(got[i], R.to_tensor(ref_bytes))                   # out == byte / 255 exactly
    if name == "identity_lut":
        (jobs, keys), lut = outputs[0]
        jb = jobs[0]
        pasted = R.paste(np.full((H, W, 3), 128, np.uint8), R.resize_cubic(SRC[keys[0]], (jb["nw"], jb["nh"])), jb["dx"], jb["dy"])
        same = (R.hsv2rgb(R.rgb2hsv(pasted)) == pasted).all(-1)                 # where HSV round-trips, the output is the pasted picture
        assert same.mean() > 0.2 and np.array_equal(np.rint(got[0] * 255).astype(np.uint8).transpose(1, 2, 0)[same], pasted[same])


def test_images_equal_the_reference_fixture(dev, gold):
    """the two pictures the reference's own get_random_data / mosaic_for_voc composed (with the restated pixel primitives)"""
    fh, fw, cases = R.load_cases(gold("aug_ref.npz"))
    assert (fh, fw) == (H, W)
    picked = [c for c in cases if c["image"] is not None]
    outputs = [((c["jobs"], [R.synth_picture(int(s[0]), int(s[1]), int(k)) for s, k in zip(c["sizes"], c["src_seeds"])]), c["lut"]) for c in picked]
    images, _, _ = run(dev, outputs)
    assert {int(c["mosaic"]) for c in picked} == {0, 1}
    for i, c in enumerate(picked):
        assert np.array_equal(images[i].cpu().numpy(), R.to_tensor(c["image"]))


def test_boxes_equal_the_reference_fixture_bit_for_bit(dev, gold):
    """every fixture case as one output image of ONE launch, plus an image whose boxes are all filtered out; targets, count and order"""
    _, _, cases = R.load_cases(gold("aug_ref.npz"))
    outputs = [((c["jobs"], [np.zeros((j["ih"], j["iw"], 3), np.uint8) for j in c["jobs"]]), c["lut"]) for c in cases]
    boxes = [c["job_boxes"] for c in cases]
    tiny = plain("c", 9, 10, 40, 30)                                              # 96 -> 10 pixels: these boxes end up under 1 px wide
    tiny_boxes = np.array([[10, 10, 18, 60, 3], [50, 5, 59, 90, 4], [0, 0, 9, 9, 5]], np.float32)
    at = 6
    outputs.insert(at, (tiny, LUT))
    boxes.insert(at, [tiny_boxes])
    assert len(R.targets([[(tiny[0][0], tiny_boxes)]], H, W)) == 0
    ref = []
    for k, c in enumerate(cases):
        lab = c["labels"].copy()
        lab[:, 0] = k + (k >= at)                                                # its output index in this launch
        ref.append(lab)
    ref = np.concatenate(ref, 0)
    n_in = sum(len(b) for bs in boxes for b in bs)
    assert any(len(c["boxes"]) == 0 for c in cases) and len(ref) < n_in
    _, t7, aug = run(dev, outputs, boxes, fmt="yolo7")
    assert t7.device == dev and int(aug.last_count.item()) == len(ref) == t7.shape[0]
    assert np.array_equal(t7.cpu().numpy(), ref)
    assert np.array_equal(ref[:, 0], np.sort(ref[:, 0]))                          # grouped by image, box order within
    _, t8, _ = run(dev, outputs, boxes, fmt="yolo8")
    assert set(t8) == {"batch_idx", "cls", "bboxes"} and all(v.device == dev for v in t8.values())
    assert t8["batch_idx"].shape == (len(ref),) and t8["cls"].shape == (len(ref), 1) and t8["bboxes"].shape == (len(ref), 4)
    assert np.array_equal(torch.cat((t8["batch_idx"][:, None], t8["cls"], t8["bboxes"]), 1).cpu().numpy(), ref)
    _, pad, aug = run(dev, outputs, boxes, fmt="yolo7", exact=False)              # no read-back: all rows, unused ones carry image -1
    assert pad.shape == (n_in, 6) and np.array_equal(pad[:len(ref)].cpu().numpy(), ref) and bool((pad[len(ref):, 0] == -1).all())


def test_boxes_merge_equals_reference_merge_bboxes(dev, gold):
    """merge_bboxes alone: jobs that leave integer boxes where they are (picture = canvas), cuts at the fixture's"""
    g = gold("aug_ref.npz")
    cx, cy = (int(v) for v in g["merge_cut"])
    rects = [(0, 0, cx, cy), (0, cy, cx, H), (cx, cy, W, H), (cx, 0, W, cy)]
    jobs = [dict(ih=H, iw=W, nh=H, nw=W, dx=0, dy=0, flip=0, quad=q, rect=rects[q]) for q in range(4)]
    blank = np.zeros((H, W, 3), np.uint8)
    _, t, _ = run(dev, [((jobs, [blank] * 4), LUT)], [[g["merge_in"][q] for q in range(4)]])
    m = g["merge_out"]
    x1, y1, x2, y2 = (m[:, i] / np.float32(d) for i, d in zip(range(4), (W, H, W, H)))
    bw, bh = x2 - x1, y2 - y1
    ref = np.stack([np.zeros_like(x1), m[:, 4], x1 + bw / np.float32(2), y1 + bh / np.float32(2), bw, bh], 1).astype(np.float32)
    assert 0 < len(ref) < 40 and np.array_equal(t.cpu().numpy(), ref)


def test_no_boxes_at_all(dev):
    images, t, aug = run(dev, IMAGE_CASES["plain"])
    assert t.shape == (0, 6) and int(aug.last_count.item()) == 0


# ---- the loader in front of the trainers -----------------------------------------------------------------
def picture_source(dev, n=5):
    sizes = [(37, 53), (64, 48), (96, 96), (80, 120), (50, 50)]
    return [(torch.from_numpy(R.synth_picture(h, w, 30 + i)).to(dev), R.synth_boxes(h, w, 4 if i != 3 else 0, 40 + i)) for i, (h, w) in enumerate(sizes[:n])]


def host_copy(batch):
    images, targets = batch
    return images.cpu(), ({k: v.cpu().clone() for k, v in targets.items()} if isinstance(targets, dict) else targets.cpu().clone())


@pytest.mark.parametrize("name,hw,fmt", [("yolo8_det", (128, 128), "yolo8"), ("yolo7", (160, 224), "yolo7")])
def test_loader_feeds_the_trainer(dev, tmp_path, name, hw, fmt):
    """batch 2, max_iters = 2: the trainer over DeviceAugLoader ends on the same parameters, bit for bit, as the trainer fed the same augmented
    tensors by its ordinary injected-loader path (host tensors, as a DataLoader hands them over)"""
    import builder

    def trainer(loader, sub):
        cfg, _, trainer_cls = builder.export_from_registry(name)
        cfg.arch.input_size = (3,) + hw
        cfg.train.batch_size, cfg.train.epoch, cfg.train.pretrained = 2, 1, False
        cfg.train.save_path = str(tmp_path / sub)
        if name == "yolo8_det":
            cfg.engine.init_loss_scale = 1024.0
        torch.manual_seed(0)
        return trainer_cls(cfg, dev, dataloader=loader)

    source = picture_source(dev)

    def loader():
        return DeviceAugLoader(source, 2, DeviceAugmenter(hw, mosaic=True, mosaic_prob=0.5, seed=3), length=2, fmt=fmt, device=dev)

    batches = list(loader())
    assert len(batches) == 2
    for images, targets in batches:
        assert images.shape == (2, 3) + hw and images.device == dev and 0.0 <= float(images.min()) and float(images.max()) <= 1.0
        rows = targets if fmt == "yolo7" else torch.cat((targets["batch_idx"][:, None], targets["cls"], targets["bboxes"]), 1)
        assert rows.device == dev and rows.shape[1] == 6 and rows.shape[0] > 0
        assert bool(((rows[:, 2:] >= 0) & (rows[:, 2:] <= 1)).all()) and bool((rows[:, 0] < 2).all())
    tr = trainer(loader(), "device")
    tr.train(max_iters=2)
    tr2 = trainer([host_copy(b) for b in batches], "host")
    tr2.train(max_iters=2)
    torch.cuda.synchronize()
    assert tr.optimizer.device_step() == 2 == tr2.optimizer.device_step()
    assert torch.equal(tr.model.flat_params, tr2.model.flat_params)
    tr.model.train()
    tr2.model.train()
    v1 = [float(v) for v in tr.train_loop(batches[0], None)]
    v2 = [float(v) for v in tr2.train_loop(host_copy(batches[0]), None)]
    assert all(np.isfinite(v) for v in v1) and v1 == v2, (v1, v2)
