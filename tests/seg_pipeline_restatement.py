"""Host restatement of the segmentation input pipeline (computervision.pytorch_amd/seg_pipeline.py, csrc/seg_pipeline.hip) in numpy / torch-CPU:
the reference's transforms (core/data/segmentation_dataset.py:82-293) written out literally, the pin the kernel is held to
(``torch.nn.functional.interpolate`` on the CPU -- what torchvision 0.14.1's tensor resize calls; torchvision itself is not installed), and an
fp64 evaluation of the same formulas from which the tests take their bounds.  Nothing here touches a GPU or the package under test."""
import numpy as np
import torch
import torch.nn.functional as F

from aug_restatement import synth_picture  # noqa: F401  (the tests' pictures)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---- the random draws, literally ---------------------------------------------------------------------------------------------------
def resized_size(ih, iw, base):
    """torchvision ``_compute_resized_output_size`` for an int size: (h, w) of ``Resize(base)``"""
    short, long = (iw, ih) if iw <= ih else (ih, iw)
    new_short, new_long = base, int(base * long / short)
    return (new_long, new_short) if iw <= ih else (new_short, new_long)


def get_params(gen, h, w, th, tw):
    """torchvision ``RandomCrop.get_params`` (:614-637 of transforms.py in 0.14.1) with an explicit generator"""
    if h < th or w < tw:
        raise ValueError(f"Required crop size {(th, tw)} is larger than input image size {(h, w)}")
    if w == tw and h == th:
        return 0, 0, h, w
    i = torch.randint(0, h - th + 1, size=(1,), generator=gen).item()
    j = torch.randint(0, w - tw + 1, size=(1,), generator=gen).item()
    return i, j, th, tw


def draw(gen, pyrng, size, base, crop_hw, train=True):
    """Resize -> RandomCrop -> RandomHorizontalFlip of one item, in the order ``Compose`` calls them (:268-273)"""
    ih, iw = size
    H, W = crop_hw
    if not train:
        return dict(ih=ih, iw=iw, rh=H, rw=W, i=0, j=0, flip=0)
    rh, rw = resized_size(ih, iw, base)
    i, j, _, _ = get_params(gen, rh, rw, H, W)
    flip = 1 if pyrng.random() < 0.5 else 0
    return dict(ih=ih, iw=iw, rh=rh, rw=rw, i=i, j=j, flip=flip)


# ---- the pin: torch on the CPU ----------------------------------------------------------------------------------------------------------
def _crop_flip(t, job, H, W):
    t = t[..., job["i"]:job["i"] + H, job["j"]:job["j"] + W]
    return t.flip(-1) if job["flip"] else t


def image_torch(picture, job, H, W, normalise=True):
    """ToTensor -> Resize -> crop -> hflip -> Normalize of a uint8 (h, w, 3) picture in fp32: (3, H, W)"""
    x = torch.from_numpy(np.ascontiguousarray(picture)).permute(2, 0, 1).float().div(255)
    x = F.interpolate(x[None], size=(job["rh"], job["rw"]), mode="bilinear", align_corners=False)[0]
    x = _crop_flip(x, job, H, W).clone()
    if normalise:
        x.sub_(torch.tensor(MEAN).view(3, 1, 1)).div_(torch.tensor(STD).view(3, 1, 1))
    return x


def labels_torch(labels, job, H, W, mode="bilinear"):
    """what ``Resize`` does to the (h, w) int64 class map -- F.resize on an integer tensor: cast to fp32, interpolate bilinearly,
    torch.round, cast back -- then crop and hflip; ``mode="nearest"`` is F.interpolate(mode="nearest") instead"""
    t = torch.from_numpy(np.ascontiguousarray(labels)).long()[None, None].float()
    if mode == "bilinear":
        t = torch.round(F.interpolate(t, size=(job["rh"], job["rw"]), mode="bilinear", align_corners=False))
    else:
        t = F.interpolate(t, size=(job["rh"], job["rw"]), mode="nearest")
    return _crop_flip(t[0, 0].long(), job, H, W)


# ---- the same formulas in fp64 ------------------------------------------------------------------------------------------------------------
def taps(out_size, in_size):
    """torch's coordinate arithmetic, in fp32 as torch does it: scale = in / out, src = max(scale * (dst + 0.5) - 0.5, 0), the upper tap
    clamped to the last row / column.  Returns (i0, i1, lambda fp32)."""
    scale = np.float32(in_size) / np.float32(out_size)
    src = np.maximum(scale * (np.arange(out_size, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    assert src.dtype == np.float32
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    lam = np.clip(src - i0.astype(np.float32), np.float32(0), np.float32(1))
    return i0, i1, lam


def resize64(x, oh, ow):
    """bilinear resize of (..., h, w) in fp64 with the fp32 coordinates above (their lambdas taken as exact numbers)"""
    x = np.asarray(x, np.float64)
    y0, y1, ly = taps(oh, x.shape[-2])
    x0, x1, lx = taps(ow, x.shape[-1])
    ly, lx = ly.astype(np.float64)[:, None], lx.astype(np.float64)[None, :]
    top = x[..., y0, :][..., x0] * (1 - lx) + x[..., y0, :][..., x1] * lx
    bot = x[..., y1, :][..., x0] * (1 - lx) + x[..., y1, :][..., x1] * lx
    return top * (1 - ly) + bot * ly


def _crop_flip_np(a, job, H, W):
    a = a[..., job["i"]:job["i"] + H, job["j"]:job["j"] + W]
    return a[..., ::-1] if job["flip"] else a


def image64(picture, job, H, W, normalise=True):
    """image_torch's formulas in fp64 (mean and std are the fp32 numbers torch subtracts and divides by)"""
    x = resize64(np.asarray(picture, np.float64).transpose(2, 0, 1) / 255.0, job["rh"], job["rw"])
    x = _crop_flip_np(x, job, H, W)
    if normalise:
        x = (x - np.asarray(MEAN, np.float32).astype(np.float64).reshape(3, 1, 1)) / np.asarray(STD, np.float32).astype(np.float64).reshape(3, 1, 1)
    return np.ascontiguousarray(x)


def labels64(labels, job, H, W):
    """the interpolated (not yet rounded) class value of every output pixel in fp64"""
    return np.ascontiguousarray(_crop_flip_np(resize64(labels, job["rh"], job["rw"]), job, H, W))


def near_half(values, eps=1e-3):
    """pixels whose interpolated value lies within ``eps`` of a half-integer: torch.round may go either way there in fp32"""
    frac = values - np.floor(values)
    return np.abs(frac - 0.5) <= eps


# ---- masks -------------------------------------------------------------------------------------------------------------------------------------
def blocky_labels(h, w, seed, cell=8, nc=21):
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, nc, ((h + cell - 1) // cell, (w + cell - 1) // cell))
    return np.kron(coarse, np.ones((cell, cell), np.int64))[:h, :w].astype(np.int64)


def colour_mask(labels, colormap, unknown=()):
    """(h, w, 3) uint8 in the table's colours; the pixels listed in ``unknown`` get a colour the table does not hold"""
    m = np.asarray(colormap, np.uint8)[labels]
    for (y, x) in unknown:
        m[y, x] = (7, 9, 11)
    return m


def label_indices(mask, colormap):
    """RGB2idx (:70-79, :200-209) with a K-entry table: a colour that is not listed is class 0, as in the reference's 2^24-entry table"""
    key = (mask[..., 0].astype(np.int64) * 256 + mask[..., 1]) * 256 + mask[..., 2]
    out = np.zeros(mask.shape[:2], np.int64)
    for k, (r, g, b) in enumerate(colormap):
        out[key == (int(r) * 256 + int(g)) * 256 + int(b)] = k
    return out
