"""numpy restatement of csrc/seg_tta.hip: numpy float32, the kernels' operations in the kernels' order.  It is the
specification of ``cvx_seg_tta_inputs`` and of ``cvx_seg_fuse``: the input resize + mirror, the per-view logits z_k and mode 0 ("logits")
exactly; for mode 1 ("prob") it takes the float32 z_k and does the softmax and the mean in float64, and returns the float64 top-2 margin of
the mean probability per pixel, so a test can leave out the pixels whose label an fp32 rounding may decide.  The fused multiply-add, the
taps, the mix and the arg max are the ones of tests/render_restatement.py, imported and not restated.

A view is ``(rows, lh, lw, flip)``: rows (B, lh * lw, ld) fp32 as ``forward_rows`` leaves them."""
import functools

import numpy as np

from render_restatement import argmax_lowest, bilinear_mix, bilinear_taps


def resize_plane_stack(x, oh, ow):
    """x (..., h, w) fp32 -> (..., oh, ow): bilinear, align_corners=False, no antialiasing, the taps and the mix of bilinear.h"""
    x = np.asarray(x, np.float32)
    h, w = x.shape[-2:]
    y0, y1, ly = bilinear_taps(oh, h)
    x0, x1, lx = bilinear_taps(ow, w)
    Y0, X0 = np.meshgrid(y0, x0, indexing="ij")
    Y1, X1 = np.meshgrid(y1, x1, indexing="ij")
    LY, LX = np.meshgrid(ly, lx, indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        return bilinear_mix(x[..., Y0, X0], x[..., Y0, X1], x[..., Y1, X0], x[..., Y1, X1], LX, LY)


def tta_inputs(images, oh, ow, flip):
    """images (B, c, h, w) -> (B * (1 + flip), c, oh, ow): the resize first, the mirror second"""
    plain = resize_plane_stack(images, oh, ow)
    return np.concatenate([plain, plain[..., ::-1]]) if flip else plain


def view_logits(view, nc, oh, ow):
    """(B, nc, oh, ow) fp32: z_k -- one interpolation from the view's logit level to the output size (cvx_resize_bilinear_rows_to_nchw's
    numbers for that view), read at column ow - 1 - x for a flipped view"""
    rows, lh, lw, flip = view
    rows = np.asarray(rows, np.float32)
    z = rows.reshape(rows.shape[0], lh, lw, -1)[..., :nc].transpose(0, 3, 1, 2)
    out = resize_plane_stack(z, oh, ow)
    return np.ascontiguousarray(out[..., ::-1] if flip else out)


def fuse_logits(views, nc, oh, ow):
    """mode 0: (B, nc, oh, ow) fp32, acc = acc + z_k from 0, one rounded add per view in table order"""
    acc = None
    for v in views:
        z = view_logits(v, nc, oh, ow)
        with np.errstate(invalid="ignore", over="ignore"):
            acc = (np.zeros_like(z) + z if acc is None else acc + z).astype(np.float32)
    return acc


def fuse_prob(views, nc, oh, ow):
    """mode 1: (B, nc, oh, ow) float64, the mean over the views of softmax(z_k) -- z_k in fp32 as the kernel has it, the rest in float64"""
    total = None
    for v in views:
        z = view_logits(v, nc, oh, ow).astype(np.float64)
        e = np.exp(z - z.max(1, keepdims=True))
        p = e / e.sum(1, keepdims=True)
        total = p if total is None else total + p
    return total / len(views)


def labels_logits(views, nc, oh, ow):
    return argmax_lowest(fuse_logits(views, nc, oh, ow), 1).astype(np.uint8)


def labels_prob(views, nc, oh, ow):
    """(labels (B, oh, ow) uint8, mean probabilities (B, nc, oh, ow) float64, margin (B, oh, ow) float64: largest minus second largest)"""
    p = fuse_prob(views, nc, oh, ow)
    if nc == 1:
        return np.zeros(p[:, 0].shape, np.uint8), p, np.ones(p[:, 0].shape)
    top = np.sort(p, axis=1)
    return argmax_lowest(p, 1).astype(np.uint8), p, top[:, -1] - top[:, -2]


def confusion(labels, target, nc):
    """(nc, nc) int64: confusion[target][label] over the pixels with target in [0, nc)"""
    labels, target = np.asarray(labels, np.int64).reshape(-1), np.asarray(target, np.int64).reshape(-1)
    keep = (target >= 0) & (target < nc)
    return np.bincount(target[keep] * nc + labels[keep], minlength=nc * nc).reshape(nc, nc).astype(np.int64)


# ---- the seeded inputs of the kernel tests (tests/test_seg_tta_gpu.py), here so that the CPU suite can check what they assume ------------------
LEVELS = [(9 + (20 * k) // 15, 13 + (30 * k) // 15) for k in range(16)]          # (9, 13) .. (29, 43), all different
FUSE_SHAPES = [(3, 4), (5, 5), (21, 24)]                                         # the vector path, the scalar path, the production padding
FUSE_OUTPUTS = [(65, 97), (64, 50)]
FUSE_TABLES = [1, 2, 6, 16]
FUSE_BATCHES = [1, 3]


def table_geometry(n_views):
    """[(lh, lw, flip)]: n_views different levels spread over LEVELS, mixed flip flags (none for a single view)"""
    picks = [LEVELS[7]] if n_views == 1 else [LEVELS[(15 * k) // (n_views - 1)] for k in range(n_views)]
    return [(lh, lw, k % 3 == 1) for k, (lh, lw) in enumerate(picks)]


@functools.lru_cache(maxsize=None)
def fuse_case(nc, ld, out_hw, n_views, batch):
    """(views, targets): logits drawn directly as 3 * standard_normal with the padding columns past nc far above every class -- they must
    not be read as classes --, int64 targets in [0, nc + 2) with some -100 and 255.  Shared and never modified."""
    rng = np.random.RandomState(100000 + 1000 * nc + 100 * n_views + 10 * batch + out_hw[0])
    views = []
    for lh, lw, flip in table_geometry(n_views):
        rows = (3.0 * rng.standard_normal((batch, lh * lw, ld))).astype(np.float32)
        rows[..., nc:] = 100.0
        rows.setflags(write=False)
        views.append((rows, lh, lw, flip))
    targets = rng.randint(0, nc + 2, (batch,) + tuple(out_hw)).astype(np.int64)
    r = rng.rand(*targets.shape)
    targets[r < 0.05] = -100
    targets[r > 0.95] = 255
    targets.setflags(write=False)
    return views, targets


# mode 1 runs over every shape, output and table, with batch 3 at the (64, 50) output and 1 at (65, 97)
PROB_CASES = [(nc, ld, out_hw, n, 3 if out_hw == (64, 50) else 1) for nc, ld in FUSE_SHAPES for out_hw in FUSE_OUTPUTS for n in FUSE_TABLES]
MARGIN = 2e-5            # a label is compared where the float64 top-2 margin of the mean probability exceeds this: twice the bound on probs
