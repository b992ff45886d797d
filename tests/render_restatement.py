"""numpy restatement of the drawing rules of csrc/render.hip, written in painter's order -- box 0 first, outline, tag,
text, later layers over earlier ones -- where the kernel walks the boxes backwards and stops at the first layer -- and of the overlay: nearest
index, the fp32 taps of bilinear.h with their single roundings, arg max, integer blend."""
import numpy as np

from computervision.pytorch_amd import render as R

COORD_LIMIT = 1048576


def trunc_coord(v):
    """int(): towards zero, far-away values clamped (a NaN class reads as the lower bound)"""
    v = np.float32(v)
    if v != v:
        return -COORD_LIMIT
    return int(np.trunc(min(max(v, np.float32(-COORD_LIMIT)), np.float32(COORD_LIMIT))))


def box_layers(h, w, row, thickness=2, font_scale=2):
    """(outline mask, tag mask, text mask) of one row [x1, y1, x2, y2, score, cls] on an (h, w) frame, or None when it paints nothing"""
    if any(np.float32(v) != np.float32(v) for v in row[:4]):
        return None
    x0, y0, x1, y1 = (trunc_coord(v) for v in row[:4])
    if x1 < x0 or y1 < y0:
        return None
    yy, xx = np.mgrid[0:h, 0:w]
    g, s = thickness // 2, (thickness + 1) // 2
    outer = (xx >= x0 - g) & (xx <= x1 + g) & (yy >= y0 - g) & (yy <= y1 + g)
    inner = (xx >= x0 + s) & (xx <= x1 - s) & (yy >= y0 + s) & (yy <= y1 - s)
    outline = outer & ~inner
    cls = min(max(trunc_coord(row[5]), 0), R.MAX_CLASS)
    label = R.format_label(cls, row[4])
    fs = font_scale
    tag_w, tag_h = (6 * len(label) + 1) * fs, 9 * fs
    tx, ty = x0, (y0 - tag_h if y0 - tag_h >= 0 else y0)
    tag = (xx >= tx) & (xx < tx + tag_w) & (yy >= ty) & (yy < ty + tag_h)
    text = np.zeros((h, w), bool)
    for k, ch in enumerate(label):
        for gy, bits in enumerate(R.FONT[ch]):
            for gx in range(5):
                if bits >> (4 - gx) & 1:
                    px, py = tx + fs + k * 6 * fs + gx * fs, ty + fs + gy * fs
                    text |= (xx >= px) & (xx < px + fs) & (yy >= py) & (yy < py + fs)
    return outline, tag, text, cls


def draw(frame, rows, count, lut=None, thickness=2, font_scale=2):
    """frame (h, w, 3) uint8 with rows[:count] painted, as a new array; also the mask of painted pixels"""
    lut = R.palette(256) if lut is None else np.asarray(lut, np.uint8)
    out = np.array(frame, copy=True)
    h, w = out.shape[:2]
    painted = np.zeros((h, w), bool)
    for row in np.asarray(rows, np.float32).reshape(-1, 6)[:max(int(count), 0)]:
        layers = box_layers(h, w, row, thickness, font_scale)
        if layers is None:
            continue
        outline, tag, text, cls = layers
        colour = lut[(cls + 1) % len(lut)].astype(np.int64)
        out[outline] = colour
        out[tag] = colour * 7 // 10
        out[text] = 0 if int(colour.sum()) > 382 else 255
        painted |= outline | tag | text
    return out, painted


def blend_half(a, b):
    """cv2.addWeighted(a, .5, b, .5, 0) on uint8: (a + b) / 2 rounded half to even"""
    s = np.asarray(a, np.int64) + np.asarray(b, np.int64)
    return ((s >> 1) + (s & (s >> 1) & 1)).astype(np.uint8)


def argmax_lowest(z, axis=0):
    """arg max with the lowest index winning a tie (strict > while walking up)"""
    z = np.asarray(z)
    best = np.take(z, 0, axis)
    arg = np.zeros(best.shape, np.int64)
    for c in range(1, z.shape[axis]):
        zc = np.take(z, c, axis)
        up = zc > best
        best = np.where(up, zc, best)
        arg = np.where(up, c, arg)
    return arg


def nearest_index(dst_size, src_size):
    """cv2.resize(..., INTER_NEAREST): source index per destination index"""
    scale = 1.0 / (float(dst_size) / float(src_size))
    return np.minimum(np.floor(np.arange(dst_size, dtype=np.float64) * scale).astype(np.int64), src_size - 1)


def _fma(a, b, c):
    """fp32 fused multiply-add, one rounding: the fp64 product of two fp32 is exact; the fp64 sum is rounded to odd (its error term from
    the two-sum decides), and rounding a 53-bit round-to-odd value to 24 bits equals rounding the exact value once"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def bilinear_taps(out_size, in_size):
    """bilinear.h:bilinear_src in fp32: (i0, i1, lam) per output index"""
    d = np.arange(out_size, dtype=np.float32)
    scale = np.float32(in_size) / np.float32(out_size)
    s = _fma(d + np.float32(0.5), scale, np.float32(-0.5))
    s = np.maximum(s, np.float32(0))
    a = np.minimum(s.astype(np.int64), in_size - 1)
    b = a + (a < in_size - 1)
    return a, b, (s - a.astype(np.float32)).astype(np.float32)


def bilinear_mix(v00, v01, v10, v11, lx, ly):
    one = np.float32(1)
    top = _fma(lx, v01, ((one - lx) * v00).astype(np.float32))
    bot = _fma(lx, v11, ((one - lx) * v10).astype(np.float32))
    return _fma(one - ly, top, (ly * bot).astype(np.float32))


def logits_at_network_size(rows, nc, lh, lw, NH, NW):
    """rows (lh * lw, ld) fp32 -> (nc, NH, NW) fp32, cvx_resize_bilinear_rows_to_nchw's numbers"""
    z = np.asarray(rows, np.float32).reshape(lh, lw, -1)[:, :, :nc]
    y0, y1, ly = bilinear_taps(NH, lh)
    x0, x1, lx = bilinear_taps(NW, lw)
    Y0, X0 = np.meshgrid(y0, x0, indexing="ij")
    Y1, X1 = np.meshgrid(y1, x1, indexing="ij")
    LY, LX = np.meshgrid(ly, lx, indexing="ij")
    out = bilinear_mix(z[Y0, X0], z[Y0, X1], z[Y1, X0], z[Y1, X1], LX[..., None], LY[..., None])
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def seg_overlay(frame, rows, nc, lh, lw, NH, NW, lut, bgr=False):
    """frame (h, w, 3) uint8 RGB with the class colours of the logits rows blended in, as a new array"""
    h, w = frame.shape[:2]
    classes = argmax_lowest(logits_at_network_size(rows, nc, lh, lw, NH, NW), 0)
    cls = classes[nearest_index(h, NH)][:, nearest_index(w, NW)]
    out = blend_half(frame, np.asarray(lut, np.uint8)[cls])
    return out[..., ::-1].copy() if bgr else out
