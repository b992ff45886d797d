"""Writes tests/golden/aug_ref.npz: the REAL reference ``DetectionDataset.__getitem__`` (core/data/detection_dataset.py:60-130) and what it
calls -- ``get_random_data``, ``mosaic_for_voc``, ``mosaic_body``, ``merge_bboxes`` -- run unbound on a namespace ``self`` over seeded
synthetic pictures and boxes, with every drawn parameter recorded.

    python tools/make_aug_golden.py /path/to/ComputerVision.pytorch

``detection_dataset.py`` imports ``cv2``, ``pycocotools`` and ``torchvision``; none of them is needed to be real here, so stand-in modules
are registered first.  The stand-in ``cv2`` implements ``resize`` / ``flip`` / ``cvtColor`` / ``split`` / ``merge`` / ``LUT`` by the
restatement in tests/aug_restatement.py and records its arguments; ``cv2_paste`` (the reference's own) is wrapped to record the paste
position, ``read_image`` / ``_parse_xml`` serve the synthetic data, and ``np.random.shuffle`` is the identity (the device path keeps box
order).  So the fixture pins, against the reference's code: the order of the random draws, the ``int()`` truncations, paste positions,
flips, LUT construction, the quadrant composition, the box arithmetic, ``merge_bboxes`` and the label normalisation.  It does NOT pin the
pixel primitives against OpenCV's bytes.  Mosaic cases use square pictures, where the reference's rows/columns swap (:224) is invisible.

Per case ``c<k>_``: ``seed``, ``mosaic`` (0 | 1), ``sizes`` (J, 2) (ih, iw) and ``src_seeds`` (J,) of the pictures in job order (regenerate
them with ``aug_restatement.synth_picture``), ``boxes`` (n, 5) source boxes of all jobs and
``box_start`` (J + 1,), ``params`` (J, 6) (nh, nw, dx, dy, flip, quad), ``cut`` (2,), ``lut`` (3, 256), ``labels`` (m, 6) fp32
[0, cls, cx, cy, w, h] as ``__getitem__`` returns them, and for the cases listed in ``image_cases`` ``image`` (H, W, 3) uint8, the picture
handed to ``to_tensor``.  ``merge_in`` (4, 10, 5) / ``merge_cut`` / ``merge_out``: ``merge_bboxes`` alone on boxes anywhere on the canvas (through
the data set's own geometry it never drops a box).
"""
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aug_restatement as R  # noqa: E402

H, W = 64, 96
NOTE = ("reference DetectionDataset code run with a stand-in cv2 (tests/aug_restatement.py): geometry, draw order, LUTs, box arithmetic and "
        "merge_bboxes are the reference's own; the pixel primitives (bicubic resize, RGB<->HSV) are NOT checked against OpenCV's bytes")


def install_stand_ins(log):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_CUBIC, cv2.INTER_NEAREST, cv2.COLOR_RGB2HSV, cv2.COLOR_HSV2RGB = 2, 0, 41, 55
    cv2.COLOR_BGR2RGB, cv2.COLOR_BGR2GRAY, cv2.IMREAD_COLOR, cv2.IMREAD_IGNORE_ORIENTATION, cv2.BORDER_CONSTANT = 4, 6, 1, 128, 0

    def resize(src, dsize, interpolation):
        assert interpolation == cv2.INTER_CUBIC
        log.append(("resize", tuple(int(v) for v in dsize)))
        return R.resize_cubic(src, dsize)

    def flip(img, code):
        log.append(("flip", img.shape[:2]))
        return R.flip(img, code)

    def cvt(img, code):
        return {cv2.COLOR_RGB2HSV: R.rgb2hsv, cv2.COLOR_HSV2RGB: R.hsv2rgb}[code](img)

    def lut(img, table):
        log.append(("lut", np.array(table)))
        return table[img]

    cv2.resize, cv2.flip, cv2.cvtColor, cv2.LUT = resize, flip, cvt, lut
    cv2.split = lambda img: tuple(img[..., i] for i in range(img.shape[-1]))
    cv2.merge = lambda chans: np.stack(chans, -1)
    sys.modules["cv2"] = cv2
    coco = types.ModuleType("pycocotools.coco")
    coco.COCO = object
    sys.modules["pycocotools"], sys.modules["pycocotools.coco"] = types.ModuleType("pycocotools"), coco
    tv, tvt, tvf = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.ModuleType("torchvision.transforms.functional")

    def to_tensor(img):
        log.append(("to_tensor", np.array(img)))
        return img

    tvf.to_tensor = to_tensor
    tv.transforms, tvt.functional = tvt, tvf
    sys.modules["torchvision"], sys.modules["torchvision.transforms"], sys.modules["torchvision.transforms.functional"] = tv, tvt, tvf


def run_case(dd, log, seed, mosaic, pictures, boxes):
    """pictures / boxes: the data set (lists); item 0 is asked for.  Returns the fixture entries of the case."""
    DD = dd.DetectionDataset
    ns = types.SimpleNamespace(dataset_name="voc", mosaic=mosaic, mosaic_prob=2.0, epoch_now=-1, epoch_length=100, special_aug_ratio=0.7,
                               input_shape=[H, W], jitter=0.3, hue=0.1, sat=0.7, val=0.4, train=True,
                               voc_images=list(range(len(pictures))), xml_paths=list(range(len(pictures))))
    served = []

    def read_image(key):
        served.append(key)
        return pictures[key].copy()

    dd.read_image = read_image
    ns._parse_xml = lambda key: [[float(v) for v in row] for row in boxes[key]]
    for name in ("get_random_data", "mosaic_for_voc", "mosaic_body", "merge_bboxes"):
        setattr(ns, name, types.MethodType(getattr(DD, name), ns))
    del log[:]
    np.random.seed(seed)
    random.seed(seed)
    _, labels = DD.__getitem__(ns, 0)
    sizes = [(n[1][1], n[1][0]) for n in log if n[0] == "resize"]
    pastes = [n[1] for n in log if n[0] == "paste"]
    luts = [n[1] for n in log if n[0] == "lut"]
    image = [n[1] for n in log if n[0] == "to_tensor"][0]
    assert len(sizes) == len(pastes) == len(served) == (4 if mosaic else 1) and len(luts) == 3
    # flips in call order: a mosaic picture is mirrored before its resize, a plain canvas after its paste
    flips, pending = [], False
    for n in log:
        if n[0] == "flip":
            pending = True
            if not mosaic:
                flips.append(1)
        elif n[0] == "resize" and mosaic:
            flips.append(int(pending))
            pending = False
    if not mosaic and not flips:
        flips = [0]
    params = np.array([[nh, nw, dx, dy, f, (q if mosaic else -1)] for q, ((nh, nw), (dx, dy), f) in enumerate(zip(sizes, pastes, flips))], np.int32)
    bx = [np.asarray(boxes[k], np.float32).reshape(-1, 5) for k in served]
    cut = (params[2, 2], params[2, 3]) if mosaic else (0, 0)                 # quadrant 2 is pasted at (cutx, cuty)
    return {"seed": np.int64(seed), "mosaic": np.int64(mosaic), "sizes": np.array([pictures[k].shape[:2] for k in served], np.int32),
            "served": np.array(served, np.int32), "boxes": np.concatenate(bx, 0), "box_start": np.cumsum([0] + [len(b) for b in bx]).astype(np.int32),
            "params": params, "cut": np.array(cut, np.int32), "lut": np.stack(luts).astype(np.uint8), "labels": np.asarray(labels, np.float32)}, image


def main():
    ref_root = os.path.abspath(sys.argv[1])
    log = []
    install_stand_ins(log)
    sys.path.insert(0, ref_root)
    import core.data.detection_dataset as dd
    assert os.path.abspath(dd.__file__).startswith(ref_root)
    real_paste = dd.cv2_paste

    def paste(img1, img2, x, y):
        log.append(("paste", (int(x), int(y))))
        return real_paste(img1, img2, x, y)

    dd.cv2_paste = paste
    np.random.shuffle = lambda x: None                                         # deviation 1: boxes keep their order
    arrays = {"note": np.array(NOTE), "input_shape": np.array([H, W], np.int32)}
    plain_sources = [(37, 53), (64, 48), (96, 96), (5, 7)]
    cases, image_cases = [], []
    k = 0
    for si, (h, w) in enumerate(plain_sources):
        for seed in ([0, 1, 20, 53] if si == 2 else [0, 1, 2]):                   # 1040 and 1073 draw a negative dy (overhang)
            pic, box = R.synth_picture(h, w, 100 + si), R.synth_boxes(h, w, 6 if (si, seed) != (1, 2) else 0, 200 + 10 * si + seed)
            entry, image = run_case(dd, log, 1000 + 10 * si + seed, False, [pic], [box])
            entry["src_seeds"] = np.array([100 + si], np.int32)
            if (si, seed) == (2, 20):
                entry["image"] = image
                image_cases.append(k)
            cases.append(entry)
            k += 1
    for seed in range(5):
        sizes = [(96, 96), (48, 48), (96, 96), (37, 37), (64, 64), (96, 96)]
        pics = [R.synth_picture(h, w, 300 + i) for i, (h, w) in enumerate(sizes)]
        boxes = [R.synth_boxes(h, w, (0 if i == 1 and seed == 0 else 7), 400 + 10 * seed + i) for i, (h, w) in enumerate(sizes)]
        entry, image = run_case(dd, log, 2000 + seed, True, pics, boxes)
        entry["src_seeds"] = (300 + entry["served"]).astype(np.int32)
        if seed == 0:
            entry["image"] = image
            image_cases.append(k)
        cases.append(entry)
        k += 1
    # coverage the tests rely on
    plain = [c for c in cases if not c["mosaic"]]
    assert any(c["params"][0, 4] for c in plain) and any(not c["params"][0, 4] for c in plain)
    assert any(c["params"][0, 3] < 0 or c["params"][0, 2] < 0 for c in plain), "no overhanging paste"
    assert any(len(c["labels"]) < len(c["boxes"]) for c in plain) and any(len(c["boxes"]) == 0 for c in plain)
    straddle = dropped = False
    for c in (c for c in cases if c["mosaic"]):
        outputs = []
        for j in range(4):
            nh, nw, dx, dy, f, q = (int(v) for v in c["params"][j])
            cx, cy = (int(v) for v in c["cut"])
            rect = [(0, 0, cx, cy), (0, cy, cx, H), (cx, cy, W, H), (cx, 0, W, cy)][j]
            jb = dict(ih=int(c["sizes"][j, 0]), iw=int(c["sizes"][j, 1]), nh=nh, nw=nw, dx=dx, dy=dy, flip=f, quad=q, rect=rect)
            b = R.boxes_of_job(jb, c["boxes"][c["box_start"][j]:c["box_start"][j + 1]], H, W, merge=False)
            merged = R.boxes_of_job(jb, c["boxes"][c["box_start"][j]:c["box_start"][j + 1]], H, W)
            dropped |= len(merged) < len(b)
            straddle |= bool(((b[:, 0] <= cx) & (b[:, 2] >= cx) & (b[:, 1] <= cy) & (b[:, 3] >= cy)).any())
    assert straddle and not dropped            # the reference pastes each picture against the cuts, so merge_bboxes never drops one of ITS boxes
    # ... therefore merge_bboxes on its own: boxes anywhere on the canvas, through the reference's unbound method
    rng = np.random.RandomState(7)
    cutx, cuty = 40, 30
    groups = []
    for q in range(4):
        x1, y1 = rng.randint(0, W - 4, 10), rng.randint(0, H - 4, 10)
        groups.append(np.stack([x1, y1, np.minimum(x1 + rng.randint(2, 60, 10), W), np.minimum(y1 + rng.randint(2, 40, 10), H),
                                rng.randint(0, 20, 10)], 1).astype(np.float32))
    merged = dd.DetectionDataset.merge_bboxes(None, [g.astype(np.float64) for g in groups], cutx, cuty)
    assert 0 < len(merged) < 40
    arrays["merge_in"], arrays["merge_cut"] = np.stack(groups), np.array([cutx, cuty], np.int32)
    arrays["merge_out"] = np.array(merged, np.float32).reshape(-1, 5)
    for i, c in enumerate(cases):
        for key, v in c.items():
            arrays[f"c{i}_{key}"] = v
    arrays["n_cases"], arrays["image_cases"] = np.int64(len(cases)), np.array(image_cases, np.int32)
    path = os.path.join(ROOT, "tests", "golden", "aug_ref.npz")
    np.savez_compressed(path, **arrays)
    print(path, len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
