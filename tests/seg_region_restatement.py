"""The rules of the Dice / Tversky / focal-Tversky region losses (csrc/loss_seg.hip) restated in torch float64,
formula by formula and without autograd, so that tests can hold both an independent autograd formulation and the kernels against it.

    valid pixels: t != ignore_index and 0 <= t < C; a group is the batch, or one image under per_image; sums over a group's valid pixels
    I_c = sum p_c y_c     P_c = sum p_c     Y_c = sum y_c                      p = softmax(z), y = one-hot(t)
    D_c = (1 - al - be) I_c + al P_c + be Y_c + smooth      T_c = (I_c + smooth) / D_c, 1 when D_c == 0       L_c = (1 - T_c)^gamma
    m_c = [Y_c > 0] with skip_absent, else 1;  v = class weights (ones when absent)
    group loss = sum_c m_c v_c L_c / sum_c m_c v_c, 0 when that denominator is 0;   region = mean of the group losses over the G groups
    k_c = (1/G) m_c v_c / sum m v (-gamma (1 - T_c)^(gamma - 1)), 0 where 1 - T_c <= 0
    a_c = k_c (D_c - (I_c + smooth)(1 - al - be)) / D_c^2       b_c = -k_c (I_c + smooth) al / D_c^2
    g_c = a_c y_c + b_c       d region / d z_k = p_k (g_k - sum_c p_c g_c) at a valid pixel, 0 elsewhere
    criterion = base_weight * base + weight * region

Also the inputs and the four configurations of tests/test_seg_region_*.py."""
import torch
import torch.nn.functional as F

from seg_loss_restatement import criterion, low_res_nchw, make_case, upsample  # noqa: F401  (the tests take them from here)

SHAPES = [(2, 9, 12, 33, 45, 21), (1, 5, 6, 40, 48, 5), (2, 33, 33, 33, 33, 19), (3, 17, 12, 65, 45, 5)]
# name -> the region= dict without weights; "class_weights": True stands for the case's weights (make_case's third output)
CONFIGS = {
    "dice": dict(kind="dice"),
    "tversky_g075_per_image_all": dict(kind="tversky", alpha=0.3, beta=0.7, gamma=0.75, smooth=1e-5, per_image=True, skip_absent=False),
    "tversky_g2_smooth0": dict(kind="tversky", alpha=0.7, beta=0.3, gamma=2.0, smooth=0.0),
    "dice_per_image_weights": dict(kind="dice", per_image=True, class_weights=True),
}


def case(shape):
    """make_case(shape, B*1000 + H + nc) with target class 2 remapped to 3: one class is absent."""
    B, ih, iw, H, W, nc = shape
    rows, t, w = make_case(shape, B * 1000 + H + nc)
    t = torch.where(t == 2, torch.full_like(t, 3), t)
    return rows, t, w


def config(name, weights):
    """The region= dict of configuration ``name`` for ``SegLoss`` (class_weights: the case's weights where the configuration has them)."""
    r = dict(CONFIGS[name])
    if r.get("class_weights"):
        r["class_weights"] = weights
    return r


def region(logits, target, kind="dice", alpha=None, beta=None, gamma=1.0, smooth=1.0, per_image=False, skip_absent=True, class_weights=None,
           ignore_index=-100, **_):
    """logits (B, C, H, W), target (B, H, W) int64 -> dict(value, stats (G, C, 4) = I, P, Y, T, grad = d region / d logits, valid)."""
    al, be = (0.5, 0.5) if kind == "dice" else (0.3 if alpha is None else alpha, 0.7 if beta is None else beta)
    z = logits.double()
    B, C, H, W = z.shape
    valid = (target != ignore_index) & (target >= 0) & (target < C)
    tc = torch.where(valid, target, torch.zeros_like(target))
    p = torch.exp(z - torch.logsumexp(z, dim=1, keepdim=True))
    vm = valid[:, None].double()
    y = F.one_hot(tc, C).permute(0, 3, 1, 2).double() * vm
    dims = (2, 3) if per_image else (0, 2, 3)
    I, P, Y = (p * y).sum(dims).reshape(-1, C), (p * vm).sum(dims).reshape(-1, C), y.sum(dims).reshape(-1, C)
    G = I.shape[0]
    D = (1.0 - al - be) * I + al * P + be * Y + smooth
    zero = D == 0
    Ds = torch.where(zero, torch.ones_like(D), D)
    T = torch.where(zero, torch.ones_like(D), (I + smooth) / Ds)
    om = (1.0 - T).clamp_min(0.0)
    pos = om > 0
    oms = torch.where(pos, om, torch.ones_like(om))
    L = torch.where(pos, oms ** gamma, torch.zeros_like(om))
    v = torch.ones(C, dtype=torch.float64) if class_weights is None else torch.as_tensor(class_weights).double()
    w = v[None] * ((Y > 0).double() if skip_absent else torch.ones_like(Y))
    den = w.sum(1, keepdim=True)
    live = den > 0
    dens = torch.where(live, den, torch.ones_like(den))
    group = torch.where(live[:, 0], (w * L).sum(1) / dens[:, 0], torch.zeros(G, dtype=torch.float64))
    value = group.sum() / G
    k = torch.where(pos & live & ~zero, (1.0 / G) * (w / dens) * (-gamma * oms ** (gamma - 1.0)), torch.zeros_like(om))
    a = k * (D - (I + smooth) * (1.0 - al - be)) / (Ds * Ds)
    b = -k * (I + smooth) * al / (Ds * Ds)
    if not per_image:
        a, b = a.expand(B, C), b.expand(B, C)
    g = a[:, :, None, None] * y + b[:, :, None, None]
    grad = p * (g - (p * g).sum(1, keepdim=True)) * vm
    return {"value": value, "stats": torch.stack([I, P, Y, T], dim=2), "grad": grad, "valid": valid}


def combine(base_value, base_grad, reg, weight=1.0, base_weight=1.0):
    """(value, gradient) of base_weight * base + weight * region; base_value / base_grad None: the region term alone."""
    if base_value is None or base_weight == 0.0:
        return weight * reg["value"], weight * reg["grad"]
    return base_weight * base_value + weight * reg["value"], base_weight * base_grad + weight * reg["grad"]


def focal(logits, target, alpha=0.25, gamma=2.0, ignore_index=-100):
    """FocalLoss() of the reference restated without autograd: alpha (1 - pt)^gamma ce, mean over ALL pixels; (value, gradient)."""
    z = logits.double()
    B, C, H, W = z.shape
    valid = (target != ignore_index) & (target >= 0) & (target < C)
    tc = torch.where(valid, target, torch.zeros_like(target))
    lse = torch.logsumexp(z, dim=1)
    ce = (lse - z.gather(1, tc[:, None])[:, 0]) * valid
    pt = torch.exp(-ce)
    om = (1.0 - pt).clamp_min(0.0)
    n = float(B * H * W)
    value = (alpha * om ** gamma * ce * valid).sum() / n
    coef = alpha * (om ** gamma + gamma * om ** (gamma - 1.0) * pt * ce) * valid
    p = torch.exp(z - lse[:, None])
    grad = coef[:, None] * (p - F.one_hot(tc, C).permute(0, 3, 1, 2).double()) / n
    return value, grad


def to_rows_grad(grad_full, shape):
    """The adjoint of the bilinear upsampling in float64: d / d logits (B, C, H, W) -> d / d rows as (B, ih*iw, nc)."""
    B, ih, iw, H, W, nc = shape
    low = torch.zeros(B, nc, ih, iw, dtype=torch.float64, requires_grad=True)
    upsample(low, shape).backward(grad_full)
    return low.grad.permute(0, 2, 3, 1).reshape(B, ih * iw, nc)
