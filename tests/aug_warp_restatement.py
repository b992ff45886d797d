"""Host restatement (numpy fp32) of stage 2 of the device augmentation -- ``cvx_aug_warp_mix`` and ``cvx_aug_boxes_warp`` in
``csrc/augment.hip`` -- shared by tests/test_aug_warp_cpu.py and tests/test_aug_warp_gpu.py.  The rules are the
project's own, modelled on YOLOv5's ``random_perspective``, ``box_candidates`` and ``mixup``; the kernels are held to this file bit for bit.

Every fp32 step is ONE rounded operation (numpy on float32 arrays does exactly that; the kernel file is compiled with contraction off), in
this order:

* matrix: ``M = T . Sh . R . P . C`` in float64 (``matrix``), ``M^-1`` inverted in float64; both and the zoom ``s`` are rounded to fp32 once;
* pixel ``(x, y)``, integer coordinates, no half-pixel shift: ``u' = (i0 x + i1 y) + i2``, ``v' = (i3 x + i4 y) + i5``,
  ``w = (i6 x + i7 y) + i8`` with ``i = M^-1``; ``u = u' / w``, ``v = v' / w``, always divided.  Unless ``-1 < u < W`` and ``-1 < v < H`` no
  tap can lie on the canvas and the value is the grey ``128 / 255`` itself (also for a NaN).  Otherwise ``x0 = floor(u)``, ``lx = u - x0``,
  likewise y; a tap outside the canvas is the grey; ``top = v00 (1 - lx) + v01 lx``, ``bot = v10 (1 - lx) + v11 lx``,
  ``value = top (1 - ly) + bot ly`` (two rounded products, then the rounded sum, at both levels);
* MixUp: ``out = own r + partner r1`` (two rounded products, one rounded sum), ``r1 = fp32(1) - r`` taken on the host; an output without a
  partner is ``own`` untouched;
* box ``[cls, cx, cy, w, h]``: ``pcx = cx W``, ``pw = w W``, ``x1 = pcx - pw / 2``, ``x2 = pcx + pw / 2`` (y alike); the corners ``(x1, y1),
  (x2, y2), (x1, y2), (x2, y1)`` through ``M`` like a pixel through ``M^-1``; min / max of the four, clipped to ``[0, W] x [0, H]``;
  ``w2 = X2 - X1``, ``w1 = x2 - x1``; kept iff ``w2 > min_wh``, ``h2 > min_wh``, ``(w2 h2) / ((w1 s) (h1 s)) > min_area_ratio`` and
  ``fmax(w2 / h2, h2 / w2) < max_aspect``; then ``X / W``, ``Y / H``, ``bw = X2 - X1``, ``cx = X1 + bw / 2``.
"""
import numpy as np

F = np.float32
GREY = F(128) / F(255)
CANDIDATES = dict(min_wh=2.0, min_area_ratio=0.1, max_aspect=100.0)


def matrix(eight, H, W):
    """float64 ``M`` of the eight numbers (p_x, p_y, degrees, zoom, shear_x degrees, shear_y degrees, t_x, t_y), YOLOv5's composition"""
    px, py, deg, s, shx, shy, tx, ty = (float(v) for v in eight)
    C = np.array([[1, 0, -W / 2], [0, 1, -H / 2], [0, 0, 1]], np.float64)
    P = np.array([[1, 0, 0], [0, 1, 0], [px, py, 1]], np.float64)
    a = np.deg2rad(deg)
    R = np.array([[s * np.cos(a), s * np.sin(a), 0], [-s * np.sin(a), s * np.cos(a), 0], [0, 0, 1]], np.float64)
    Sh = np.array([[1, np.tan(np.deg2rad(shx)), 0], [np.tan(np.deg2rad(shy)), 1, 0], [0, 0, 1]], np.float64)
    T = np.array([[1, 0, tx * W], [0, 1, ty * H], [0, 0, 1]], np.float64)
    return T @ Sh @ R @ P @ C


def project(m, x, y):
    """(x, y) fp32 arrays through the fp32 3 x 3 ``m`` with the divide"""
    m = np.asarray(m, np.float64).astype(F).reshape(9)
    assert x.dtype == F and y.dtype == F
    with np.errstate(all="ignore"):
        a = (m[0] * x + m[1] * y) + m[2]
        b = (m[3] * x + m[4] * y) + m[5]
        w = (m[6] * x + m[7] * y) + m[8]
        px, py = a / w, b / w
    assert px.dtype == F and py.dtype == F
    return px, py


def warp_image(canvas, minv):
    """canvas (3, H, W) fp32 seen through ``minv`` = M^-1 -> (3, H, W) fp32"""
    canvas = np.asarray(canvas)
    assert canvas.dtype == F
    _, H, W = canvas.shape
    yy, xx = np.mgrid[0:H, 0:W]
    u, v = project(minv, xx.astype(F), yy.astype(F))
    with np.errstate(all="ignore"):
        near = (u > F(-1)) & (u < F(W)) & (v > F(-1)) & (v < F(H))
    u, v = np.where(near, u, F(0)), np.where(near, v, F(0))
    xf, yf = np.floor(u), np.floor(v)
    lx, ly = u - xf, v - yf
    omx, omy = F(1) - lx, F(1) - ly
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    padded = np.full((3, H + 2, W + 2), GREY, F)                       # the canvas with a grey ring: index + 1
    padded[:, 1:-1, 1:-1] = canvas
    v00, v01 = padded[:, y0 + 1, x0 + 1], padded[:, y0 + 1, x0 + 2]
    v10, v11 = padded[:, y0 + 2, x0 + 1], padded[:, y0 + 2, x0 + 2]
    top = v00 * omx + v01 * lx
    bot = v10 * omx + v11 * lx
    out = top * omy + bot * ly
    assert out.dtype == F
    return np.where(near[None], out, GREY)


def warp_mix(canvases, minv, partner=None, r=None, r1=None):
    """canvases (B, 3, H, W) fp32; minv (B, 3, 3); partner (B,) with -1 for none; r, r1 (B,) fp32 -> the final batch"""
    B = len(canvases)
    warped = [warp_image(canvases[i], minv[i]) for i in range(B)]
    out = []
    for i in range(B):
        p = -1 if partner is None else int(partner[i])
        if p < 0:
            out.append(warped[i])
            continue
        assert p != i and p < B
        mixed = warped[i] * F(r[i]) + warped[p] * F(r1[i])
        assert mixed.dtype == F
        out.append(mixed)
    return np.stack(out)


def box_corners(labels, H, W):
    """[cls, cx, cy, w, h] normalised -> pixel corners x1, y1, x2, y2 (fp32)"""
    lab = np.asarray(labels, F).reshape(-1, 5)
    pcx, pcy, pw, ph = lab[:, 1] * F(W), lab[:, 2] * F(H), lab[:, 3] * F(W), lab[:, 4] * F(H)
    return pcx - pw / F(2), pcy - ph / F(2), pcx + pw / F(2), pcy + ph / F(2)


def warp_corners(labels, m, H, W):
    """the new box of every label: min / max of its four corners through ``m``, clipped -> X1, Y1, X2, Y2 (fp32)"""
    x1, y1, x2, y2 = box_corners(labels, H, W)
    xs, ys = zip(*(project(m, a, b) for a, b in ((x1, y1), (x2, y2), (x1, y2), (x2, y1))))
    X1, X2 = np.fmin(np.fmin(xs[0], xs[1]), np.fmin(xs[2], xs[3])), np.fmax(np.fmax(xs[0], xs[1]), np.fmax(xs[2], xs[3]))
    Y1, Y2 = np.fmin(np.fmin(ys[0], ys[1]), np.fmin(ys[2], ys[3])), np.fmax(np.fmax(ys[0], ys[1]), np.fmax(ys[2], ys[3]))
    clip = lambda a, hi: np.fmin(np.fmax(a, F(0)), F(hi))  # noqa: E731
    return clip(X1, W), clip(Y1, H), clip(X2, W), clip(Y2, H)


def candidates(w1, h1, w2, h2, s, min_wh=2.0, min_area_ratio=0.1, max_aspect=100.0):
    """the three tests, each as its own mask: (size, area, aspect)"""
    w1, h1, w2, h2, s = (np.asarray(a, F) for a in (w1, h1, w2, h2, s))
    with np.errstate(all="ignore"):
        size = (w2 > F(min_wh)) & (h2 > F(min_wh))
        area = (w2 * h2) / ((w1 * s) * (h1 * s)) > F(min_area_ratio)
        aspect = np.fmax(w2 / h2, h2 / w2) < F(max_aspect)
    return size, area, aspect


def warp_boxes(labels, m, s, H, W, **cand):
    """stage-1 labels (n, 5) of one canvas through its matrix -> the kept rows (k, 5) [cls, cx, cy, w, h] in order"""
    lab = np.asarray(labels, F).reshape(-1, 5)
    if not len(lab):
        return lab
    x1, y1, x2, y2 = box_corners(lab, H, W)
    X1, Y1, X2, Y2 = warp_corners(lab, m, H, W)
    size, area, aspect = candidates(x2 - x1, y2 - y1, X2 - X1, Y2 - Y1, F(s), **{**CANDIDATES, **cand})
    nx1, nx2, ny1, ny2 = X1 / F(W), X2 / F(W), Y1 / F(H), Y2 / F(H)
    bw, bh = nx2 - nx1, ny2 - ny1
    out = np.stack([lab[:, 0], nx1 + bw / F(2), ny1 + bh / F(2), bw, bh], 1)
    assert out.dtype == F
    return out[size & area & aspect]


def boxes_per_output(labels, m, s, partner, H, W, **cand):
    """labels: per canvas (n_i, 5) stage-1 rows -> per output the kept rows of its own canvas, then of its partner's"""
    kept = [warp_boxes(lab, m[i], s[i], H, W, **cand) for i, lab in enumerate(labels)]
    out = []
    for i in range(len(labels)):
        p = -1 if partner is None else int(partner[i])
        out.append(kept[i] if p < 0 else np.concatenate([kept[i], kept[p]], 0))
    return out


def compact(per_output):
    """(N', 6) rows [image, cls, cx, cy, w, h] in image order"""
    rows = [np.concatenate([np.full((len(k), 1), i, F), k], 1) for i, k in enumerate(per_output) if len(k)]
    return np.concatenate(rows, 0).astype(F) if rows else np.zeros((0, 6), F)


def padded(per_output, cap):
    """labels (B, cap, 5) with zero rows behind the kept ones, counts (B), overflow"""
    B = len(per_output)
    labels, counts, overflow = np.zeros((B, cap, 5), F), np.zeros(B, np.int32), 0
    for i, k in enumerate(per_output):
        n = min(len(k), cap)
        labels[i, :n], counts[i] = k[:n], n
        overflow |= int(len(k) > cap)
    return labels, counts, overflow
