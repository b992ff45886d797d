"""The rules of the Lovasz-Softmax term (csrc/loss_seg.hip, include/cvx_engine.h) restated in float64, formula by
formula and without autograd, so that tests can hold both Berman's formulation under autograd and the kernels against it.

    p = softmax(z); valid pixels: t != ignore_index and 0 <= t < C; a group is the batch, or one image under per_image; the pixel index
    inside a group is its linear (b, y, x) index.  Per group and class c, over the group's valid pixels:
    f = [t == c]    e = f ? 1 - p_c : p_c    G_c = sum f
    order: e descending, ties by ascending pixel index
    state before element k of that order: fb foreground and k - fb background elements; I = G_c - fb, U = G_c + (k - fb)
    Delta_k = 1 / U at a foreground element, I / (U (U + 1)) at a background one, 1 for the first element of a class with G_c = 0
    L_c = sum_k e_(k) Delta_k
    m_c = [G_c > 0] with skip_absent, else 1;  v = class weights (ones when absent)
    group loss = sum_c m_c v_c L_c / sum_c m_c v_c, 0 when that denominator is 0;   lovasz = mean of the group losses over the G groups
    h_c(pixel) = (1/G) m_c v_c / sum m v * s * Delta_rank, s = -1 where t == c, +1 elsewhere
    d lovasz / d z_k = p_k (h_k - sum_c p_c h_c) at a valid pixel, 0 elsewhere
    criterion = base_weight * base + weight * lovasz

``key`` replaces the value the ORDER is taken from (the errors in the sums stay float64): ``order_sensitivity`` takes it from float32(e)
and from float32(e) (1 + u) and reports how far the gradient w.r.t. the rows moves.

Also the inputs and the configurations of tests/test_seg_lovasz_*.py."""
import numpy as np
import torch

from seg_region_restatement import SHAPES, case, combine, criterion, focal, low_res_nchw, make_case, to_rows_grad, upsample  # noqa: F401

TINY = (1, 3, 3, 7, 5, 2)
MANY = (1, 4, 5, 9, 11, 260)
# name -> the lovasz= dict; "class_weights": True stands for the case's weights
CONFIGS = {"batch": {}, "per_image": dict(per_image=True), "per_image_all": dict(per_image=True, skip_absent=False),
           "batch_weights": dict(class_weights=True)}


def config(name, weights):
    r = dict(CONFIGS[name])
    if r.get("class_weights"):
        r["class_weights"] = weights
    return r


def tiny_case():
    g = torch.Generator().manual_seed(1)
    rows = torch.zeros(1, 9, 8)
    rows[..., :2] = torch.randn(1, 9, 2, generator=g) * 2
    t = torch.randint(0, 2, (1, 7, 5), generator=g)
    t[0, 0, 0] = -100
    return rows, t, torch.tensor([0.5, 1.5])


def tie_case(kind):
    """SHAPES[3] with logits that tie exactly, in fp32 and in float64 alike: every logit is 0 or a power of two, and the bilinear mix of
    four equal such values is that value to the bit in both precisions.  "constant": the same logits at every pixel, so every class's
    errors take two values (p_c and 1 - p_c) and the order is the index rule alone.  "five": every logit drawn from five values, the
    same over an image and different between the images, so a batch group has many exact ties across flags inside an image and an
    order between the images."""
    shape = SHAPES[3]
    B, ih, iw, H, W, nc = shape
    _, t, w = case(shape)
    ld = (nc + 7) & ~7
    rows = torch.zeros(B, ih * iw, ld)
    if kind == "constant":
        rows[..., :nc] = torch.tensor([0.5, -1.0, 2.0, 0.0, 1.0])
    else:
        g = torch.Generator().manual_seed(5)
        vals = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0])
        rows[..., :nc] = vals[torch.randint(0, 5, (B, 1, nc), generator=g)]
    return shape, rows, t, w


def digits_case():
    """SHAPES[2] as a confident network sees it: every pixel has a winning class -- its target at half of the valid pixels -- and every
    OTHER logit is lowered by an amount uniform in [0, 60].  The margins reach 60 and more: the errors run from about 1e-26 (and exact
    zeros, where p or 1 - p rounds to 0 in fp32) to 1, so every digit pass of the sort has work and key 0 is a dense cluster.
    The margin is made by lowering, not by raising: the device forms p = exp(z_c - lse) in fp32, and a winning logit of 60 would put
    half an ulp of lse, 1.9e-6, on every key of the pixel, which says nothing about the sort.  The identity shape for the same reason:
    the logits are the rows' own values, with no interpolation rounding."""
    shape = SHAPES[2]
    B, ih, iw, H, W, nc = shape
    rows, t, w = make_case(shape, 77)
    g = torch.Generator().manual_seed(78)
    n = B * ih * iw
    winner = torch.randint(0, nc, (n,), generator=g)
    tt = t.reshape(n)
    take = (torch.rand(n, generator=g) < 0.5) & (tt >= 0)
    winner = torch.where(take, tt, winner)
    amount = torch.rand(n, generator=g) * 60.0
    flat = rows.reshape(n, -1)
    lowered = flat[:, :nc] - amount[:, None]
    lowered[torch.arange(n), winner] = flat[torch.arange(n), winner]
    flat[:, :nc] = lowered
    return shape, rows, t, w


def many_case():
    rows, t, w = make_case(MANY, 21)
    return MANY, rows, t, w


def gpu_cases():
    """name -> (shape, rows, t, weights, tied): every input the GPU file uses.  tied: exempt from the order condition by construction."""
    out = {}
    for i, shape in enumerate(SHAPES):
        out[f"shape{i}"] = (shape,) + tuple(case(shape)) + (False,)
    rows, t, w = case(SHAPES[0])
    t = t.clone()
    t[1] = -100
    out["shape0_image1_ignored"] = (SHAPES[0], rows, t, w, False)
    out["tiny"] = (TINY,) + tuple(tiny_case()) + (False,)
    for kind in ("constant", "five"):
        out["ties_" + kind] = tie_case(kind) + (True,)
    out["digits"] = digits_case() + (False,)
    out["many"] = many_case() + (False,)
    return out


def full_logits(shape, rows, tied=False):
    """The float64 logits at label resolution.  tied: the rows are constant over each image and so are their bilinear mixes -- exactly, and
    to the bit on the device (four equal taps that are 0 or a power of two); torch's CPU upsampling sums four weighted taps and is an ulp
    off here and there, which would untie the reference, so the constant is broadcast instead."""
    if not tied:
        return upsample(low_res_nchw(rows, shape), shape)
    B, ih, iw, H, W, nc = shape
    assert bool((rows == rows[:, :1]).all())
    return rows[:, 0, :nc].double()[:, :, None, None].expand(B, nc, H, W).clone()


def softmax_tied(z):
    """exp(z - logsumexp z) of (B, C, H, W) float64 logits in which pixels with the same logits get the same bits (those of the first such
    pixel).  The upsampling repeats border pixels and the tie cases repeat everything; torch's vector and tail code paths round such twins
    differently, which would turn an exact tie -- where the index rule decides, as it does on the device -- into an order by rounding."""
    B, C, H, W = z.shape
    p = torch.exp(z - torch.logsumexp(z, dim=1, keepdim=True)).permute(0, 2, 3, 1).reshape(-1, C)
    _, first, inverse = np.unique(z.permute(0, 2, 3, 1).reshape(-1, C).numpy(), axis=0, return_index=True, return_inverse=True)
    return p[torch.from_numpy(first[inverse.reshape(-1)])].reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def prepare(logits, target, ignore_index=-100):
    z = logits.double()
    B, C, H, W = z.shape
    valid = (target != ignore_index) & (target >= 0) & (target < C)
    p = softmax_tied(z)
    return {"p": p.numpy(), "valid": valid.numpy(), "t": target.numpy(), "shape": (B, C, H, W)}


def lovasz(logits, target, per_image=False, skip_absent=True, class_weights=None, ignore_index=-100, key=None, prep=None, **_):
    """logits (B, C, H, W), target (B, H, W) int64 -> dict(value, stats (G, C, 4) = 0, 0, Y_c, L_c (0 for an absent class under
    skip_absent), grad = d lovasz / d logits, h, valid, order: {(g, c): the group's pixel indices in sorted order}, errors: {(g, c): e in
    that order}).  key(e) -> the values the order is taken from (default: e itself)."""
    q = prep or prepare(logits, target, ignore_index)
    p, valid, t = q["p"], q["valid"], q["t"]
    B, C, H, W = q["shape"]
    G = B if per_image else 1
    v = np.ones(C) if class_weights is None else np.asarray(torch.as_tensor(class_weights).double())
    stats = np.zeros((G, C, 4))
    h = np.zeros((B, C, H, W))
    group_losses, order, errors = [], {}, {}
    for g in range(G):
        sel = slice(g, g + 1) if per_image else slice(0, B)
        vm = valid[sel].reshape(-1)
        idx = np.nonzero(vm)[0]                                   # the group's valid pixels by their index inside the group
        tt = t[sel].reshape(-1)[idx]
        pg = np.moveaxis(p[sel], 1, 0).reshape(C, -1)[:, idx]    # (C, n)
        Gc = np.array([(tt == c).sum() for c in range(C)])
        m = (Gc > 0).astype(np.float64) if skip_absent else np.ones(C)
        mv = m * v
        den = mv.sum()
        hg = np.zeros((C, vm.size))
        L = np.zeros(C)
        for c in range(C):
            f = tt == c
            e = np.where(f, 1.0 - pg[c], pg[c])
            kv = e if key is None else key(e)
            o = np.lexsort((idx, -kv))                            # e descending, ties by ascending pixel index
            fs, es = f[o], e[o]
            k = np.arange(o.size)
            fb = np.cumsum(fs) - fs                               # foreground elements in front of element k
            I, U = Gc[c] - fb, Gc[c] + (k - fb)
            Us = np.where(U > 0, U, 1).astype(np.float64)
            delta = np.where(U <= 0, 1.0, np.where(fs, 1.0 / Us, I / (Us * (Us + 1.0))))
            L[c] = float((es * delta).sum())
            if den > 0:
                hg[c, idx[o]] = (1.0 / G) * mv[c] / den * np.where(fs, -1.0, 1.0) * delta
            order[(g, c)], errors[(g, c)] = idx[o], es
        group_losses.append(float((mv * L).sum() / den) if den > 0 else 0.0)
        stats[g, :, 2] = Gc
        stats[g, :, 3] = L * ((Gc > 0) if skip_absent else 1.0)
        h[sel] = np.moveaxis(hg.reshape(C, -1, H, W), 0, 1)
    pt, ht = torch.from_numpy(p), torch.from_numpy(h)
    grad = pt * (ht - (pt * ht).sum(1, keepdim=True)) * torch.from_numpy(valid)[:, None].double()
    return {"value": torch.tensor(sum(group_losses) / G, dtype=torch.float64), "stats": torch.from_numpy(stats), "grad": grad, "h": ht,
            "valid": torch.from_numpy(valid), "order": order, "errors": errors}


def order_sensitivity(shape, cfg, inputs=None, draws=8, seed=0, tied=False):
    """The largest change of d lovasz / d rows in the max norm, relative to its max norm, between the order taken from float32(e) and
    from float32(e) (1 + u), u uniform in +-4 * 2^-24 from a fixed seed, over ``draws`` draws.  inputs: (rows, t), default case(shape)."""
    rows, t = (inputs if inputs is not None else case(shape))[:2]
    logits = full_logits(shape, rows, tied)
    prep = prepare(logits, t)
    kw = {k: v for k, v in cfg.items() if k in ("per_image", "skip_absent", "class_weights")}

    def f32(e):
        return e.astype(np.float32).astype(np.float64)

    base = to_rows_grad(lovasz(logits, t, key=f32, prep=prep, **kw)["grad"], shape)
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(draws):
        def jitter(e):
            return f32(e) * (1.0 + rng.uniform(-4.0 * 2.0 ** -24, 4.0 * 2.0 ** -24, e.shape))
        moved = to_rows_grad(lovasz(logits, t, key=jitter, prep=prep, **kw)["grad"], shape)
        worst = max(worst, float((moved - base).abs().max() / base.abs().max().clamp_min(1e-300)))
    return worst
