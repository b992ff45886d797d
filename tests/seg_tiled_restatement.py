"""numpy restatement of the logit stitch of csrc/seg_tiles.hip: numpy float32, the kernel's operations in the kernel's
order.  It is the specification of ``cvx_seg_stitch``; the fused multiply-add, the taps, the arg max and the blend are the ones of
tests/render_restatement.py, imported and not restated."""
import numpy as np

from render_restatement import _fma, argmax_lowest, bilinear_mix, bilinear_taps, blend_half

WEIGHTS = ("mean", "linear")


def slot_logits(rows, nc, lh, lw, NH, NW, th, tw):
    """rows (lh * lw, ld) fp32 of one slot -> (nc, th, tw): the logits at the tile-local pixels.  The taps are those of a full network
    input (scale lh / NH, lw / NW) whatever the tile's extent -- cvx_resize_bilinear_rows_to_nchw's numbers for that slot, cropped."""
    z = np.asarray(rows, np.float32).reshape(lh, lw, -1)[:, :, :nc]
    y0, y1, ly = (v[:th] for v in bilinear_taps(NH, lh))
    x0, x1, lx = (v[:tw] for v in bilinear_taps(NW, lw))
    Y0, X0 = np.meshgrid(y0, x0, indexing="ij")
    Y1, X1 = np.meshgrid(y1, x1, indexing="ij")
    LY, LX = np.meshgrid(ly, lx, indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):                  # an overflowed logit stays inf, 0 * inf is NaN: as in the kernel
        out = bilinear_mix(z[Y0, X0], z[Y0, X1], z[Y1, X0], z[Y1, X1], LX[..., None], LY[..., None])
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def tile_weight(th, tw, weight):
    """(th, tw) fp32: 1 for "mean"; for "linear" the integer min(dy + 1, th - dy) * min(dx + 1, tw - dx), exact in fp32"""
    if weight not in WEIGHTS:
        raise ValueError(weight)
    if weight == "mean":
        return np.ones((th, tw), np.float32)
    dy, dx = np.arange(th, dtype=np.int64), np.arange(tw, dtype=np.int64)
    w = np.minimum(dy + 1, th - dy)[:, None] * np.minimum(dx + 1, tw - dx)[None, :]
    assert w.max() < 2 ** 24
    return w.astype(np.float32)


def accumulate(frame_hw, tiles, rows_per_slot, nc, lh, lw, NH, NW, weight):
    """(nc, h, w) fp32: per pixel acc = fma(w_k, z_k, acc) from 0 over the covering tiles in the order of ``tiles`` (row-major, as
    ``render.tile_grid`` lists them; slot k holds tile k).  No division by the weight sum."""
    h, w = int(frame_hw[0]), int(frame_hw[1])
    assert len(tiles) == len(rows_per_slot)
    acc = np.zeros((nc, h, w), np.float32)
    for (y0, x0, th, tw), rows in zip(tiles, rows_per_slot):
        z = slot_logits(rows, nc, lh, lw, NH, NW, th, tw)
        wk = tile_weight(th, tw, weight)
        with np.errstate(invalid="ignore", over="ignore"):
            acc[:, y0:y0 + th, x0:x0 + tw] = _fma(wk[None], z, acc[:, y0:y0 + th, x0:x0 + tw])
    return acc


def stitch(frame_hw, tiles, rows_per_slot, nc, lh, lw, NH, NW, weight="linear"):
    """(h, w) uint8 labels: the arg max of the blended logits, the lowest class winning a tie"""
    return argmax_lowest(accumulate(frame_hw, tiles, rows_per_slot, nc, lh, lw, NH, NW, weight), 0).astype(np.uint8)


def overlay(frame, labels, lut, bgr=False):
    """frame (h, w, 3) uint8 RGB with the colours of ``labels`` blended in 50/50, as a new array (``bgr``: written as B, G, R)"""
    out = blend_half(frame, np.asarray(lut, np.uint8)[np.asarray(labels, np.int64)])
    return out[..., ::-1].copy() if bgr else out


def confusion(labels, target, nc):
    """(nc, nc) int64: confusion[target][label] over the pixels with target < nc"""
    labels, target = np.asarray(labels, np.int64).reshape(-1), np.asarray(target, np.int64).reshape(-1)
    keep = (target >= 0) & (target < nc)
    return np.bincount(target[keep] * nc + labels[keep], minlength=nc * nc).reshape(nc, nc).astype(np.int64)
