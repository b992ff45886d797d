"""Writes tests/golden/aug_val_ref.npz: the REAL reference ``DetectionDataset.__getitem__`` with ``train=False`` (core/data/detection_dataset.py:60-130
around ``get_random_data(random=False)``, :137-166) run unbound on a namespace ``self`` over seeded synthetic pictures and boxes.

    python tools/make_aug_val_golden.py /path/to/ComputerVision.pytorch

Same method as tools/make_aug_golden.py, whose stand-in modules are reused: the stand-in ``cv2`` resizes by the restatement in
tests/aug_restatement.py and records its arguments, ``cv2_paste`` (the reference's own) is wrapped to record the paste position, and
``np.random.shuffle`` is the identity (the device path keeps box order).  So the fixture pins, against the reference's code: the validation
geometry (``scale = min(w / iw, h / ih)``, the ``int()`` truncations, the centred paste), that nothing is flipped or colour-transformed, the
box arithmetic with its clamps and the ``w > 1 && h > 1`` filter, and the label normalisation.  It does NOT pin the bicubic resize against
OpenCV's bytes (the standing of DESIGN.md section 7f).  The tool also checks that the validation path draws no random number.

Per case ``c<k>_``: ``sizes`` (1, 2) (ih, iw), ``src_seeds`` (1,) (regenerate the picture with ``aug_restatement.synth_picture``), ``boxes``
(n, 5) source boxes, ``box_start`` (2,), ``params`` (1, 6) (nh, nw, dx, dy, flip = 0, quad = -1), ``labels`` (m, 6) fp32 [0, cls, cx, cy, w, h] as
``__getitem__`` returns them, and for the cases listed in ``image_cases`` ``image`` (H, W, 3) uint8: the picture handed to ``to_tensor``,
which the reference holds as float32 in 0...255 (checked here to be whole numbers; ``to_tensor`` does not divide float input).
"""
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import aug_restatement as R  # noqa: E402
from make_aug_golden import install_stand_ins  # noqa: E402

H, W = 64, 96
NOTE = ("reference DetectionDataset(train=False) code run with a stand-in cv2 (tests/aug_restatement.py): geometry, paste position, box arithmetic, "
        "clamps, the w > 1 && h > 1 filter and the label normalisation are the reference's own; the bicubic resize is NOT checked against "
        "OpenCV's bytes; images are stored as uint8, the reference holds them as float32 in 0...255")
# (ih, iw): upscaled with bars left and right, landscape with bars top and bottom, portrait, exactly the output size, a large landscape
SOURCES = [(37, 53), (48, 120), (120, 48), (64, 96), (150, 200)]
IMAGE_SOURCES = (0, 1, 2)


def edge_boxes(ih, iw):
    """one box that reaches past the picture on every side (clamped to the canvas where the picture touches it), one a source pixel
    wide and one a source pixel tall (under 1 px after a downscale, and never over 1 px by more than the scale)"""
    return np.array([[-6, -5, iw + 9, ih + 7, 1], [10, 5, 11, ih - 4, 2], [3, 20, iw - 5, 21, 3]], np.float32)


def run_case(dd, log, picture, boxes):
    DD = dd.DetectionDataset
    ns = types.SimpleNamespace(dataset_name="voc", mosaic=False, mosaic_prob=0.0, epoch_now=-1, epoch_length=100, special_aug_ratio=0.7,
                               input_shape=[H, W], jitter=0.3, hue=0.1, sat=0.7, val=0.4, train=False, voc_images=[0], xml_paths=[0])
    dd.read_image = lambda key: picture.copy()
    ns._parse_xml = lambda key: [[float(v) for v in row] for row in boxes]
    ns.get_random_data = types.MethodType(DD.get_random_data, ns)
    del log[:]
    np.random.seed(77)
    random.seed(77)
    before, before_py = np.random.get_state()[1].copy(), random.getstate()
    _, labels = DD.__getitem__(ns, 0)
    assert np.array_equal(np.random.get_state()[1], before) and random.getstate() == before_py, "the validation path drew a random number"
    kinds = [n[0] for n in log]
    assert kinds.count("resize") == 1 and kinds.count("paste") == 1 and kinds.count("to_tensor") == 1
    assert "flip" not in kinds and "lut" not in kinds
    (nw, nh), = [n[1] for n in log if n[0] == "resize"]
    (dx, dy), = [n[1] for n in log if n[0] == "paste"]
    image, = [n[1] for n in log if n[0] == "to_tensor"]
    assert image.dtype == np.float32 and image.shape == (H, W, 3) and np.array_equal(image, image.astype(np.uint8))
    b = np.asarray(boxes, np.float32).reshape(-1, 5)
    return {"sizes": np.array([picture.shape[:2]], np.int32), "boxes": b, "box_start": np.array([0, len(b)], np.int32),
            "params": np.array([[nh, nw, dx, dy, 0, -1]], np.int32), "labels": np.asarray(labels, np.float32)}, image.astype(np.uint8)


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
    np.random.shuffle = lambda x: None                                         # boxes keep their order (deviation 1 of augment.py)
    arrays = {"note": np.array(NOTE), "input_shape": np.array([H, W], np.int32)}
    cases, image_cases = [], []
    for si, (ih, iw) in enumerate(SOURCES):
        for variant in (0, 1):                                                   # seeded boxes + the edge boxes; no boxes at all
            if variant == 1 and si != 1:
                continue
            boxes = np.concatenate([R.synth_boxes(ih, iw, 5, 600 + si), edge_boxes(ih, iw)], 0) if variant == 0 else np.zeros((0, 5), np.float32)
            entry, image = run_case(dd, log, R.synth_picture(ih, iw, 500 + si), boxes)
            entry["src_seeds"] = np.array([500 + si], np.int32)
            if variant == 0 and si in IMAGE_SOURCES:
                entry["image"] = image
                image_cases.append(len(cases))
            cases.append(entry)
    # coverage the tests rely on
    clamped = discarded = False
    for c in cases:
        nh, nw, dx, dy = (int(v) for v in c["params"][0, :4])
        ih, iw = (int(v) for v in c["sizes"][0])
        b = c["boxes"]
        if len(b):
            x2, y2 = b[:, 2] * np.float32(nw) / np.float32(iw) + dx, b[:, 3] * np.float32(nh) / np.float32(ih) + dy
            x1, y1 = b[:, 0] * np.float32(nw) / np.float32(iw) + dx, b[:, 1] * np.float32(nh) / np.float32(ih) + dy
            clamped |= bool(((x2 > W) | (y2 > H) | (x1 < 0) | (y1 < 0)).any())
            discarded |= len(c["labels"]) < len(b)
    assert clamped and discarded
    geo = {tuple(int(v) for v in c["params"][0, :4]) for c in cases}
    assert any(dx > 0 and dy == 0 for _, _, dx, dy in geo) and any(dy > 0 and dx == 0 for _, _, dx, dy in geo) and (H, W, 0, 0) in geo
    assert any(int(c["params"][0, 0]) > int(c["sizes"][0, 0]) for c in cases), "no upscaled picture"
    for i, c in enumerate(cases):
        for key, v in c.items():
            arrays[f"c{i}_{key}"] = v
    arrays["n_cases"], arrays["image_cases"] = np.int64(len(cases)), np.array(image_cases, np.int32)
    path = os.path.join(ROOT, "tests", "golden", "aug_val_ref.npz")
    np.savez_compressed(path, **arrays)
    print(path, len(cases), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
