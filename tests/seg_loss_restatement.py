"""The rules of the weighted / smoothed / hard-pixel-mined cross-entropy (csrc/loss_seg.hip) restated in torch
float64, formula by formula and without F.cross_entropy, so that tests can hold both torch's call and the kernels against it.

    l_i   = (1 - eps) w_t (lse - z_t) + (eps / C) sum_c w_c (lse - z_c)
    loss  = sum_{i in S} l_i / sum_{i in S} w_{t_i}
    dl/dz = (1 - eps) w_t (p - onehot_t) + (eps / C) (W p - w),  p = exp(z - lse), W = sum_c w_c
    key_i = max(lse - z_t, 0);  K = min_kept * B;  theta_t = fp32(-ln thresh);  theta_min = K-th largest key of the valid pixels,
            -inf when there are fewer than K;  kept iff key > theta_t or key >= theta_min

Also the test inputs of tests/test_seg_loss_opts_*.py (the generator order of test_seg_loss_kernel_against_torch, then the weights)."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def make_case(shape, seed):
    """rows (B, ih*iw, ld) fp32 with ld = (nc+7)&~7, targets (B, H, W) int64 with about 15 % ignored (-100), weights (nc,) fp32."""
    B, ih, iw, H, W, nc = shape
    g = torch.Generator().manual_seed(seed)
    ld = (nc + 7) & ~7
    rows = torch.zeros(B, ih * iw, ld)
    rows[..., :nc] = torch.randn(B, ih * iw, nc, generator=g) * 2
    t = torch.randint(0, nc, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.15] = -100
    weights = torch.rand(nc, generator=g) + 0.1
    return rows, t, weights


def low_res_nchw(rows, shape, dtype=torch.float64):
    B, ih, iw, H, W, nc = shape
    return rows[..., :nc].reshape(B, ih, iw, nc).permute(0, 3, 1, 2).to(dtype).clone()


def upsample(low, shape):
    return F.interpolate(low, size=(shape[3], shape[4]), mode="bilinear", align_corners=False)


def theta_of(thresh):
    """fp32 rounding of the host double -ln thresh, as a python float"""
    return float(np.float32(abs(math.log(thresh))))


def criterion(logits, target, weights=None, eps=0.0, ohem=None, ignore_index=-100):
    """logits (B, C, H, W) float64, target (B, H, W) int64 -> dict(keys, theta_min, kept, valid, loss, grad): keys (B, H, W) with -1 at
    pixels that are not valid, kept / valid boolean masks, grad = d loss / d logits."""
    B, C, H, W = logits.shape
    z = logits.double()
    w = torch.ones(C, dtype=torch.float64) if weights is None else torch.as_tensor(weights).double()
    valid = (target != ignore_index) & (target >= 0) & (target < C)
    tc = torch.where(valid, target, torch.zeros_like(target))
    lse = torch.logsumexp(z, dim=1)
    zt = z.gather(1, tc[:, None])[:, 0]
    ce = lse - zt
    keys = torch.where(valid, ce.clamp_min(0.0), torch.full_like(ce, -1.0))
    theta_min = -math.inf
    kept = valid.clone()
    if ohem is not None:
        K = int(ohem["min_kept"]) * B
        vk = keys[valid]
        if vk.numel() >= K:
            theta_min = float(torch.sort(vk, descending=True).values[K - 1])
        kept = valid & ((keys > theta_of(ohem["thresh"])) | (keys >= theta_min))
    wt = w[tc]
    l = (1.0 - eps) * wt * ce + (eps / C) * (w[None, :, None, None] * (lse[:, None] - z)).sum(1)
    denom = (wt * kept).sum()
    loss = (l * kept).sum() / denom
    p = torch.exp(z - lse[:, None])
    onehot = F.one_hot(tc, C).permute(0, 3, 1, 2).double()
    g = (1.0 - eps) * wt[:, None] * (p - onehot) + (eps / C) * (w.sum() * p - w[None, :, None, None])
    grad = g * kept[:, None] / (denom if float(denom) > 0 else 1.0)
    return {"keys": keys, "theta_min": theta_min, "kept": kept, "valid": valid, "loss": loss, "grad": grad}


def torch_ce(logits, target, weights, eps, kept=None, ignore_index=-100):
    """F.cross_entropy of the installed torch, with the targets outside ``kept`` replaced by ignore_index; (loss, d loss / d logits)."""
    x = logits.clone().requires_grad_(True)
    t = target if kept is None else torch.where(kept, target, torch.full_like(target, ignore_index))
    loss = F.cross_entropy(x, t, weight=None if weights is None else torch.as_tensor(weights).to(x.dtype), ignore_index=ignore_index,
                           label_smoothing=eps, reduction="mean")
    grad = torch.autograd.grad(loss, x)[0] if bool((t != ignore_index).any()) else torch.zeros_like(x)
    return loss.detach(), grad
