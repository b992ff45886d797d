"""Host restatement of the segmentation training recipe (``cvx_seg_pipeline_aug``, csrc/seg_pipeline.hip) in numpy:
the rules of the header comment written out operation by operation.  ``evaluate(..., dt=np.float32)`` rounds every operation to fp32 in
the stated order and is what the kernel is held to bit for bit; ``dt=np.float64`` evaluates the same rules on the same fp32 coordinates
(their taps and lambdas taken as exact numbers, as tests/seg_pipeline_restatement.py does), and the distance between the two is the ``d``
the tests scale their bounds from.  Nothing here touches a GPU or the package under test."""
import numpy as np

from seg_pipeline_restatement import MEAN, STD, label_indices  # noqa: F401

BRIGHTNESS, CONTRAST, CONTRAST_LAST, SATURATION, HUE, BLUR = 1, 2, 4, 8, 16, 32
FILL = (124, 116, 104)
F32 = np.float32


def job(ih, iw, rh, rw, i=0, j=0, flip=0, cos=1.0, sin=0.0, flags=0, beta=0.0, alpha=1.0, sat=1.0, hue=0.0, blur_k=0, taps=()):
    """a hand-made job; the float fields are rounded to fp32 here, as the job table holds them"""
    taps = tuple(float(F32(t)) for t in taps)
    assert (blur_k > 0) == bool(flags & BLUR) and len(taps) >= blur_k
    return dict(ih=ih, iw=iw, rh=rh, rw=rw, i=i, j=j, flip=flip, cos=float(F32(cos)), sin=float(F32(sin)), flags=flags, beta=float(F32(beta)),
                alpha=float(F32(alpha)), sat=float(F32(sat)), hue=float(F32(hue)), blur_k=blur_k, taps=taps + (0.0,) * (9 - len(taps)))


def gaussian_taps(kernel, sigma):
    """torchvision ``_get_gaussian_kernel1d`` in float64, rounded to fp32"""
    half = (kernel - 1) * 0.5
    x = np.linspace(-half, half, kernel)
    pdf = np.exp(-0.5 * (x / sigma) ** 2)
    return (pdf / pdf.sum()).astype(F32)


# ---- step 1: geometry, always in fp32 ----------------------------------------------------------------------------------------------------------
def coords(jb, xs, ys, H, W):
    """(u, v, inside) of the output positions ``xs`` (columns) x ``ys`` (rows); any integers, the blur's halo lies outside the crop"""
    xs, ys = np.asarray(xs, np.int64)[None, :], np.asarray(ys, np.int64)[:, None]
    xf = (W - 1 - xs) if jb["flip"] else xs
    hw, hh = F32(W) * F32(0.5), F32(H) * F32(0.5)
    px = (xf.astype(F32) + F32(0.5)) - hw
    py = (ys.astype(F32) + F32(0.5)) - hh
    c, s = F32(jb["cos"]), F32(jb["sin"])
    u = ((c * px + s * py) + hw) + F32(jb["j"])
    v = ((c * py - s * px) + hh) + F32(jb["i"])
    assert u.dtype == F32 and v.dtype == F32
    inside = (u >= 0) & (u < F32(jb["rw"])) & (v >= 0) & (v < F32(jb["rh"]))
    return u, v, inside


def linear_tap(u, in_size, out_size):
    """(i0, i1, lambda fp32) of the continuous coordinate ``u`` of the resized axis: torch's source-index rule with u = dst + 0.5"""
    scale = F32(in_size) / F32(out_size)
    s = np.maximum(scale * u - F32(0.5), F32(0))
    a = np.minimum(np.clip(s, 0, 2.0 ** 30).astype(np.int64), in_size - 1)
    lam = np.clip(s - a.astype(F32), F32(0), F32(1))
    assert lam.dtype == F32
    return a, np.minimum(a + 1, in_size - 1), lam


def nearest_tap(u, in_size, out_size):
    scale = F32(in_size) / F32(out_size)
    a = np.floor((u - F32(0.5)) * scale)
    return np.clip(np.nan_to_num(a), 0, in_size - 1).astype(np.int64)


def mix4(p00, p01, p10, p11, lx, ly, dt):
    lx, ly = lx.astype(dt), ly.astype(dt)
    if dt is F32:
        wx0, wy0 = F32(1) - lx, F32(1) - ly
    else:
        wx0, wy0 = 1.0 - lx, 1.0 - ly
    top = wx0 * p00 + lx * p01
    bot = wx0 * p10 + lx * p11
    return wy0 * top + ly * bot


# ---- step 3: colour -----------------------------------------------------------------------------------------------------------------------------
def clip01(v, dt):
    return np.minimum(np.maximum(v, dt(0)), dt(1))


def rgb_to_hsv(r, g, b, dt):
    """hexcone: H in degrees [0, 360], S, V = max"""
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    d = mx - mn
    with np.errstate(all="ignore"):
        S = np.where(mx > 0, d / mx, dt(0))
        hr = dt(60) * ((g - b) / d)
        hr = np.where(hr < 0, hr + dt(360), hr)
        hg = dt(60) * ((b - r) / d) + dt(120)
        hb = dt(60) * ((r - g) / d) + dt(240)
    Hd = np.where(d == 0, dt(0), np.where(mx == r, hr, np.where(mx == g, hg, hb)))
    return Hd.astype(dt), S.astype(dt), mx


def hsv_to_rgb(Hd, S, V, dt):
    hh = Hd / dt(60)
    sector = hh.astype(np.int64)
    f = hh - sector.astype(dt)
    sector = np.where(sector >= 6, sector - 6, sector)
    p, q, t = V * (dt(1) - S), V * (dt(1) - S * f), V * (dt(1) - S * (dt(1) - f))
    r = np.choose(sector, [V, q, p, p, t, V])
    g = np.choose(sector, [t, V, V, q, p, p])
    b = np.choose(sector, [p, p, t, V, V, q])
    return r, g, b


def hsv_step(r, g, b, do_sat, sat, do_hue, hue, dt):
    Hd, S, V = rgb_to_hsv(r, g, b, dt)
    if do_sat:
        S = clip01(S * dt(sat), dt)
    if do_hue:
        Hd = Hd + dt(hue)
        Hd = np.where(Hd >= 360, Hd - dt(360), Hd)
        Hd = np.where(Hd < 0, Hd + dt(360), Hd)
    return hsv_to_rgb(Hd, S, V, dt)


def colour_plane(picture, jb, xs, ys, H, W, fill, dt):
    """steps 1-3 at the positions xs x ys of the extended plane: (3, len(ys), len(xs)) in [0, 1]"""
    u, v, inside = coords(jb, xs, ys, H, W)
    y0, y1, ly = linear_tap(v, jb["ih"], jb["rh"])
    x0, x1, lx = linear_tap(u, jb["iw"], jb["rw"])
    src = np.asarray(picture).astype(dt) / dt(255)
    rgb = [mix4(src[y0, x0, c], src[y0, x1, c], src[y1, x0, c], src[y1, x1, c], lx, ly, dt) for c in range(3)]
    fl = jb["flags"]
    if fl & BRIGHTNESS:
        rgb = [clip01(p + dt(F32(jb["beta"])), dt) for p in rgb]
    if fl & CONTRAST and not fl & CONTRAST_LAST:
        rgb = [clip01(p * dt(F32(jb["alpha"])), dt) for p in rgb]
    if fl & (SATURATION | HUE):
        rgb = list(hsv_step(rgb[0], rgb[1], rgb[2], bool(fl & SATURATION), F32(jb["sat"]), bool(fl & HUE), F32(jb["hue"]), dt))
    if fl & CONTRAST and fl & CONTRAST_LAST:
        rgb = [clip01(p * dt(F32(jb["alpha"])), dt) for p in rgb]
    out = np.stack([np.where(inside, rgb[c], dt(F32(fill[c])) / dt(255)) for c in range(3)])
    assert out.dtype == dt, out.dtype
    return out


def blur(plane, taps, k, dt):
    """step 4 on a (3, H + 2 r, W + 2 r) plane: horizontal pass, then vertical, both in tap order from the first product"""
    taps = [dt(F32(t)) for t in taps[:k]]
    n = plane.shape[2] - (k - 1)
    acc = taps[0] * plane[:, :, 0:n]
    for t in range(1, k):
        acc = acc + taps[t] * plane[:, :, t:t + n]
    m = acc.shape[1] - (k - 1)
    out = taps[0] * acc[:, 0:m]
    for t in range(1, k):
        out = out + taps[t] * acc[:, t:t + m]
    assert out.dtype == dt
    return out


def image(picture, jb, H, W, fill=FILL, dt=F32, normalise=True):
    """the (3, H, W) image of one job"""
    r = jb["blur_k"] // 2 if jb["flags"] & BLUR else 0
    plane = colour_plane(picture, jb, np.arange(-r, W + r), np.arange(-r, H + r), H, W, fill, dt)
    if r:
        plane = blur(plane, jb["taps"], jb["blur_k"], dt)
    if normalise:
        mean = np.asarray(MEAN, F32).astype(dt).reshape(3, 1, 1)
        std = np.asarray(STD, F32).astype(dt).reshape(3, 1, 1)
        plane = (plane - mean) / std
    assert plane.shape == (3, H, W) and plane.dtype == dt
    return np.ascontiguousarray(plane)


def targets(labels, jb, H, W, mode="bilinear", ignore_index=-100):
    """the (H, W) int64 targets of one job from the (h, w) class map (unlisted colours already mapped): steps 1-2, never blurred"""
    labels = np.asarray(labels, np.int64)
    u, v, inside = coords(jb, np.arange(W), np.arange(H), H, W)
    if mode == "bilinear":
        y0, y1, ly = linear_tap(v, jb["ih"], jb["rh"])
        x0, x1, lx = linear_tap(u, jb["iw"], jb["rw"])
        lab = labels.astype(F32)
        got = np.rint(mix4(lab[y0, x0], lab[y0, x1], lab[y1, x0], lab[y1, x1], lx, ly, F32)).astype(np.int64)
    else:
        got = labels[nearest_tap(v, jb["ih"], jb["rh"]), nearest_tap(u, jb["iw"], jb["rw"])]
    return np.where(inside, got, ignore_index)


def label_indices_or(mask, colormap, unlisted):
    """RGB2idx with a K-entry table where a colour that is not listed becomes ``unlisted``"""
    key = (mask[..., 0].astype(np.int64) * 256 + mask[..., 1]) * 256 + mask[..., 2]
    out = np.full(mask.shape[:2], unlisted, np.int64)
    for k, (r, g, b) in enumerate(colormap):
        out[key == (int(r) * 256 + int(g)) * 256 + int(b)] = k
    return out
