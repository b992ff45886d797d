"""Host restatement (numpy) of what ``csrc/augment.hip`` computes, shared by tests/test_augment_cpu.py, tests/test_augment_gpu.py and
tools/make_aug_golden.py (whose stand-in ``cv2`` is built from the pixel primitives here).

Pixel primitives, each in the integer / fp32 form the kernel uses (one rounded fp32 operation per step, no fused multiply-add):

* ``resize_cubic``  OpenCV's INTER_CUBIC on uint8: ``fx = float((x + .5) * iw / nw - .5)`` in double, ``sx = floor(fx)``, the four Keys weights
  (A = -0.75) in fp32 rounded to int16 as ``rint(w * 2048)``, taps ``sx-1 .. sx+2`` clamped to the picture, both passes exact in integers,
  byte = ``clamp((v + 2^21) >> 22)``;
* ``rgb2hsv`` OpenCV's 8-bit integer form with the ``sdiv`` / ``hdiv`` tables (12-bit shift); ``hsv2rgb`` its float form, bytes by round-half-even;
* ``paste`` cv2_paste's clipping; ``flip`` a horizontal mirror.

They are NOT checked against OpenCV's bytes (OpenCV is not available where the fixture is made); the geometry, draw order, LUTs and box
arithmetic around them are pinned against the reference's own code by tests/golden/aug_ref.npz.
"""
import numpy as np

F = np.float32


def cubic_taps(n_dst, n_src):
    """first tap (n_dst,) int64 and Q11 weights (n_dst, 4) int64 of a resize n_src -> n_dst"""
    r = np.arange(n_dst, dtype=np.float64)
    f = ((r + 0.5) * float(n_src) / float(n_dst) - 0.5).astype(F)
    fl = np.floor(f)
    t = f - fl
    A = F(-0.75)
    t1, u = t + F(1), F(1) - t
    c0 = ((A * t1 - F(5) * A) * t1 + F(8) * A) * t1 - F(4) * A
    c1 = ((A + F(2)) * t - (A + F(3))) * t * t + F(1)
    c2 = ((A + F(2)) * u - (A + F(3))) * u * u + F(1)
    c3 = F(1) - c0 - c1 - c2
    w = np.stack([np.rint(c * F(2048)) for c in (c0, c1, c2, c3)], 1)
    assert w.dtype == F
    return fl.astype(np.int64) - 1, w.astype(np.int64)


def resize_cubic(img, dsize):
    """cv2.resize(img, dsize=(nw, nh), interpolation=INTER_CUBIC) for uint8 HWC"""
    nw, nh = int(dsize[0]), int(dsize[1])
    ih, iw = img.shape[:2]
    sx, wx = cubic_taps(nw, iw)
    sy, wy = cubic_taps(nh, ih)
    src = img.astype(np.int64)
    hor = np.zeros((ih, nw, img.shape[2]), np.int64)
    for k in range(4):
        hor += wx[None, :, k, None] * src[:, np.clip(sx + k, 0, iw - 1), :]
    ver = np.zeros((nh, nw, img.shape[2]), np.int64)
    for j in range(4):
        ver += wy[:, j, None, None] * hor[np.clip(sy + j, 0, ih - 1)]
    assert np.abs(ver).max(initial=0) < 2 ** 31 - 2 ** 21            # the kernel accumulates in int32
    return np.clip((ver + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def flip(img, code=1):
    assert code == 1
    return np.ascontiguousarray(img[:, ::-1])


_I = np.arange(1, 256, dtype=np.float64)
SDIV = np.concatenate(([0], np.rint((255 << 12) / _I))).astype(np.int64)
HDIV = np.concatenate(([0], np.rint((180 << 12) / (6.0 * _I)))).astype(np.int64)


def rgb2hsv(img):
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    v = np.maximum(r, np.maximum(g, b))
    diff = v - np.minimum(r, np.minimum(g, b))
    s = (diff * SDIV[v] + 2048) >> 12
    num = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (num * HDIV[diff] + 2048) >> 12
    h = h + np.where(h < 0, 180, 0)
    return np.stack([np.clip(h, 0, 255), np.clip(s, 0, 255), v], -1).astype(np.uint8)


def _sat_u8(x):
    assert x.dtype == F
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def hsv2rgb(img):
    hb, sb, vb = (img[..., i] for i in range(3))
    hf = hb.astype(F) * (F(6) / F(180))
    sf, vf = sb.astype(F) / F(255), vb.astype(F) / F(255)
    while (hf >= F(6)).any():
        hf = np.where(hf >= F(6), hf - F(6), hf)
    sector = np.floor(hf).astype(np.int64)
    hf = hf - sector.astype(F)
    bad = (sector < 0) | (sector >= 6)
    sector, hf = np.where(bad, 0, sector), np.where(bad, F(0), hf)
    tab = [vf, vf * (F(1) - sf), vf * (F(1) - sf * hf), vf * (F(1) - sf * (F(1) - hf))]
    table = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])      # (b, g, r) per sector
    tabs = np.stack(tab, -1)
    out = []
    for ch in (2, 1, 0):                                                                       # r, g, b
        x = np.take_along_axis(tabs, table[sector, ch][..., None], -1)[..., 0]
        out.append(_sat_u8(np.where(sb == 0, vf, x) * F(255)))
    return np.stack(out, -1)


def colour(img, lut):
    """detection_dataset.py:197-205 with lut = (3, 256) uint8 (hue, sat, val)"""
    hsv = rgb2hsv(img)
    hsv = np.stack([lut[i][hsv[..., i]] for i in range(3)], -1)
    return hsv2rgb(hsv)


def paste(canvas, img, x, y):
    """cv2_paste (core/utils/image_process.py:132-158) for pictures that meet the canvas"""
    h1, w1 = canvas.shape[:2]
    h2, w2 = img.shape[:2]
    xmin, ymin, xmax, ymax = max(x, 0), max(y, 0), min(w1, x + w2), min(h1, y + h2)
    if xmax > xmin and ymax > ymin:
        canvas[ymin:ymax, xmin:xmax] = img[ymin - y:ymax - y, xmin - x:xmax - x]
    return canvas


def identity_lut():
    return np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def make_lut(r):
    """detection_dataset.py:200-203"""
    r = np.asarray(r, np.float64)
    x = np.arange(0, 256, dtype=r.dtype)
    return np.stack([((x * r[0]) % 180).astype(np.uint8), np.clip(x * r[1], 0, 255).astype(np.uint8), np.clip(x * r[2], 0, 255).astype(np.uint8)])


def render(jobs, sources, lut, H, W):
    """One output image as bytes (H, W, 3).  jobs: dicts with ih, iw, nh, nw, dx, dy, flip, quad, rect; sources: uint8 HWC arrays."""
    out = np.zeros((H, W, 3), np.uint8)
    for jb, src in zip(jobs, sources):
        assert src.shape[:2] == (jb["ih"], jb["iw"])
        mosaic = jb["quad"] >= 0
        pic = flip(src) if (mosaic and jb["flip"]) else src
        canvas = paste(np.full((H, W, 3), 128, np.uint8), resize_cubic(pic, (jb["nw"], jb["nh"])), jb["dx"], jb["dy"])
        if not mosaic and jb["flip"]:
            canvas = flip(canvas)
        x0, y0, x1, y1 = jb["rect"]
        out[y0:y1, x0:x1] = canvas[y0:y1, x0:x1]
    return colour(out, lut)


def to_tensor(img):
    """TF.to_tensor: (H, W, 3) uint8 -> (3, H, W) fp32, a true division"""
    return np.ascontiguousarray(img.transpose(2, 0, 1)).astype(F) / F(255)


def boxes_of_job(jb, box, H, W, merge=True):
    """The box half for one job in fp32: rows (x1, y1, x2, y2, cls) that survive, before normalisation."""
    b = np.array(box, F).reshape(-1, 5).copy()
    if not len(b):
        return b
    mosaic = jb["quad"] >= 0
    iw, ih, nw, nh, dx, dy = (F(jb[k]) for k in ("iw", "ih", "nw", "nh", "dx", "dy"))
    if mosaic and jb["flip"]:
        b[:, [0, 2]] = iw - b[:, [2, 0]]
    b[:, [0, 2]] = b[:, [0, 2]] * nw / iw + dx
    b[:, [1, 3]] = b[:, [1, 3]] * nh / ih + dy
    if not mosaic and jb["flip"]:
        b[:, [0, 2]] = F(W) - b[:, [2, 0]]
    b[:, 0:2][b[:, 0:2] < 0] = 0
    b[:, 2][b[:, 2] > W] = W
    b[:, 3][b[:, 3] > H] = H
    b = b[np.logical_and(b[:, 2] - b[:, 0] > 1, b[:, 3] - b[:, 1] > 1)]
    assert b.dtype == F
    if not mosaic or not merge:
        return b
    q = jb["quad"]
    x0, y0, x1, y1 = jb["rect"]
    return merge_boxes(b, q, (x1 if q <= 1 else x0), (y1 if q in (0, 3) else y0))


def merge_boxes(b, q, cutx, cuty):
    """merge_bboxes (detection_dataset.py:405-449) for the boxes of quadrant q"""
    keep = []
    for row in b:
        bx1, by1, bx2, by2 = row[:4]
        sy, sx = by2 >= cuty and by1 <= cuty, bx2 >= cutx and bx1 <= cutx
        if q == 0:
            if by1 > cuty or bx1 > cutx:
                continue
            by2, bx2 = (cuty if sy else by2), (cutx if sx else bx2)
        elif q == 1:
            if by2 < cuty or bx1 > cutx:
                continue
            by1, bx2 = (cuty if sy else by1), (cutx if sx else bx2)
        elif q == 2:
            if by2 < cuty or bx2 < cutx:
                continue
            by1, bx1 = (cuty if sy else by1), (cutx if sx else bx1)
        else:
            if by1 > cuty or bx2 < cutx:
                continue
            by2, bx1 = (cuty if sy else by2), (cutx if sx else bx1)
        keep.append([bx1, by1, bx2, by2, row[4]])
    return np.array(keep, F).reshape(-1, 5)


def targets(outputs, H, W):
    """(N, 6) fp32 [image, cls, cx, cy, w, h] (detection_dataset.py:100-130 + the collate functions).  outputs: per output image a list of
    (job, boxes) pairs."""
    rows = []
    for i, pairs in enumerate(outputs):
        for jb, box in pairs:
            b = boxes_of_job(jb, box, H, W)
            if not len(b):
                continue
            b[:, [0, 2]] = b[:, [0, 2]] / F(W)
            b[:, [1, 3]] = b[:, [1, 3]] / F(H)
            b[:, 2:4] = b[:, 2:4] - b[:, 0:2]
            b[:, 0:2] = b[:, 0:2] + b[:, 2:4] / F(2)
            rows.append(np.concatenate([np.full((len(b), 1), i, F), b[:, 4:5], b[:, :4]], 1))
    return np.concatenate(rows, 0).astype(F) if rows else np.zeros((0, 6), F)


# ---- seeded synthetic data (the fixture stores seeds, not pictures) ----
def synth_picture(h, w, seed):
    """smooth colour ramps + a little noise, uint8 (h, w, 3)"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    chans = [(np.sin(xx * a + yy * b + c) * 100 + 128) for a, b, c in rng.uniform(0.05, 0.6, (3, 3))]
    return np.clip(np.stack(chans, -1) + rng.randint(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


def synth_boxes(h, w, n, seed):
    """n boxes (x1, y1, x2, y2, cls) fp32 inside an (h, w) picture; some thin, some touching the border"""
    rng = np.random.RandomState(seed)
    x1, y1 = rng.uniform(0, w * 0.8, n), rng.uniform(0, h * 0.8, n)
    bw, bh = rng.uniform(0.5, w * 0.7, n), rng.uniform(0.5, h * 0.7, n)
    b = np.stack([x1, y1, np.minimum(x1 + bw, w), np.minimum(y1 + bh, h), rng.randint(0, 20, n)], 1)
    return np.round(b).astype(np.float32) if n else np.zeros((0, 5), np.float32)


# ---- tests/golden/aug_ref.npz ----
def load_cases(g):
    """fixture -> list of dicts; jobs in the form draw_params returns"""
    H, W = (int(v) for v in g["input_shape"])
    cases = []
    for i in range(int(g["n_cases"])):
        c = {k: g[f"c{i}_{k}"] for k in ("seed", "mosaic", "sizes", "src_seeds", "boxes", "box_start", "params", "cut", "lut", "labels")}
        c["image"] = g[f"c{i}_image"] if i in g["image_cases"] else None
        cx, cy = (int(v) for v in c["cut"])
        rects = [(0, 0, cx, cy), (0, cy, cx, H), (cx, cy, W, H), (cx, 0, W, cy)] if c["mosaic"] else [(0, 0, W, H)]
        c["jobs"] = [dict(ih=int(s[0]), iw=int(s[1]), nh=int(p[0]), nw=int(p[1]), dx=int(p[2]), dy=int(p[3]), flip=int(p[4]), quad=int(p[5]), rect=r)
                     for s, p, r in zip(c["sizes"], c["params"], rects)]
        c["job_boxes"] = [c["boxes"][c["box_start"][j]:c["box_start"][j + 1]] for j in range(len(c["jobs"]))]
        cases.append(c)
    return H, W, cases
