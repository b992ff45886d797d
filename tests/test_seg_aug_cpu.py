"""CPU: the host side of the segmentation training recipe -- the draws of ``DeviceSegAugmenter`` with and without a recipe, the ABI of
``cvx_seg_aug_job`` / ``cvx_seg_pipeline_aug``, the restatement (tests/seg_aug_restatement.py) against the existing one and against
``colorsys``, and the refusals."""
import colorsys
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import seg_aug_restatement as A
import seg_pipeline_restatement as S
from computervision.pytorch_amd import LIB_PATH, CvxError, seg_pipeline
from computervision.pytorch_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((37, 53), 33, (33, 33)), ((40, 29), 33, (33, 33)), ((33, 33), 33, (33, 33)), ((5, 7), 33, (33, 33)), ((48, 120), 48, (32, 48))]
RECIPE = dict(scale=(0.5, 2.0), rotate=dict(degrees=10, p=0.5),
              photometric=dict(brightness=32, contrast=(0.5, 1.5), saturation=(0.5, 1.5), hue=18, p=0.5),
              blur=dict(kernel=5, sigma=(0.1, 2.0), p=0.5), fill=(124, 116, 104))


class Recorder(random.Random):
    """a ``random.Random`` that notes which of its methods the code under test calls"""

    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def random(self):
        if not self.inside:
            self.calls.append("random")
        return super().random()

    inside = False

    def uniform(self, a, b):
        self.calls.append("uniform")
        return a + (b - a) * super().random()

    def randint(self, a, b):
        self.calls.append("randint")
        self.inside = True                   # a subclass that overrides random() has randint() draw through it: not the code under test's call
        try:
            return super().randint(a, b)
        finally:
            self.inside = False


def test_without_a_recipe_the_draws_are_draw_seg_params():
    """the class draws through draw_seg_params: the same results and the same generator states as the literal restatement, item after
    item; the torch generator is used (a recipe never touches it)"""
    rs = np.random.RandomState(1)
    sizes = [SHAPES[k][0] for k in rs.randint(0, 4, 60)]
    aug = seg_pipeline.DeviceSegAugmenter((33, 33), 33, seed=9)
    assert aug.recipe is None and aug.ignore_index == -100 and aug.unlisted == "class0"
    gen, py = torch.Generator().manual_seed(9), random.Random(9)
    seen = []
    aug.apply = lambda params, images, masks: seen.extend(params)            # the launch is not what this test is about
    for size in sizes:
        aug([torch.zeros(size + (3,), dtype=torch.uint8)], [torch.zeros(size, dtype=torch.uint8)])
    want = [S.draw(gen, py, size, 33, (33, 33)) for size in sizes]
    assert seen == want
    assert torch.equal(aug.gen.get_state(), gen.get_state()) and aug.pyrng.getstate() == py.getstate()
    assert set(seen[0]) == {"ih", "iw", "rh", "rw", "i", "j", "flip"}
    with pytest.raises(CvxError):                                            # too small a picture raises as before
        seg_pipeline.DeviceSegAugmenter((33, 40), 33, seed=0)([torch.zeros(40, 29, 3, dtype=torch.uint8)], [torch.zeros(40, 29, dtype=torch.uint8)])


def test_recipe_draws_ranges_order_and_determinism():
    recipe = seg_pipeline.check_recipe(RECIPE)
    H, W = 33, 33
    py_a, py_b = random.Random(4), random.Random(4)
    negative = rotated = blurred = 0
    flags_seen = 0
    for n in range(400):
        size = SHAPES[n % 4][0]
        p = seg_pipeline.draw_seg_aug_params(py_a, size, 33, (H, W), recipe)
        assert p == seg_pipeline.draw_seg_aug_params(py_b, size, 33, (H, W), recipe)
        base = seg_pipeline.resized_size(*size, 33)
        for got, v in zip((p["rh"], p["rw"]), base):
            assert max(1, int(v * 0.5 + 0.5)) <= got <= int(v * 2.0 + 0.5)
        assert min(0, p["rh"] - H) <= p["i"] <= max(0, p["rh"] - H) and min(0, p["rw"] - W) <= p["j"] <= max(0, p["rw"] - W)
        negative += p["i"] < 0 or p["j"] < 0
        assert p["flip"] in (0, 1)
        c, s = p["cos"], p["sin"]
        assert c == float(np.float32(c)) and s == float(np.float32(s)) and abs(c * c + s * s - 1) < 1e-6
        assert abs(s) <= np.sin(np.deg2rad(10)) + 1e-7 and c > 0
        rotated += s != 0.0
        fl = p["flags"]
        flags_seen |= fl
        assert not fl & A.BRIGHTNESS or abs(p["beta"]) <= 32 / 255 + 1e-7
        assert not fl & A.CONTRAST or 0.5 <= p["alpha"] <= 1.5
        assert not fl & A.SATURATION or 0.5 <= p["sat"] <= 1.5
        assert not fl & A.HUE or abs(p["hue"]) <= 18
        assert len(p["taps"]) == 9
        if fl & A.BLUR:
            blurred += 1
            taps = np.asarray(p["taps"], np.float64)
            assert p["blur_k"] == 5 and np.all(taps[5:] == 0) and np.all(taps[:5] >= 0) and taps[2] > 0 and np.allclose(taps[:5], taps[4::-1])
            # each tap is a float64 share of 1 rounded to fp32: half an ulp of a number below 1 is at most 2^-25
            assert abs(taps.sum() - 1.0) <= 5 * 2.0 ** -25
        else:
            assert p["blur_k"] == 0
    assert py_a.getstate() == py_b.getstate()
    assert negative > 40 and 120 < rotated < 280 and 120 < blurred < 280 and flags_seen == 63
    # the documented order of the draws for a seed where every coin comes up (p = 1)
    always = seg_pipeline.check_recipe(dict(RECIPE, rotate=dict(degrees=10, p=1.0), photometric=dict(RECIPE["photometric"], p=1.0),
                                            blur=dict(kernel=5, sigma=(0.1, 2.0), p=1.0)))
    rec = Recorder(2)
    seg_pipeline.draw_seg_aug_params(rec, (37, 53), 33, (H, W), always)
    assert rec.calls == (["uniform"] + ["random", "uniform"] + ["randint", "randint"] + ["random"] + ["random", "uniform"] + ["random"]
                         + ["random", "uniform"] * 3 + ["random", "uniform"])
    rec = Recorder(2)                                                        # every part off: origin and flip alone
    off = seg_pipeline.draw_seg_aug_params(rec, (5, 7), 8, (H, W), seg_pipeline.check_recipe({}))
    assert rec.calls == ["randint", "randint", "random"] and (off["rh"], off["rw"]) == (8, 11) and off["i"] <= 0 and off["j"] <= 0
    assert (off["cos"], off["sin"], off["flags"], off["blur_k"]) == (1.0, 0.0, 0, 0)
    # the taps are torchvision's: float64 normalisation, one rounding
    x = np.arange(-4, 5, dtype=np.float64)
    pdf = np.exp(-x * x / (2 * 1.3 ** 2))
    assert np.array_equal(seg_pipeline.gaussian_taps(9, 1.3), (pdf / pdf.sum()).astype(np.float32))
    assert np.array_equal(seg_pipeline.gaussian_taps(9, 1.3), A.gaussian_taps(9, 1.3))


def test_abi_of_the_recipe_job():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH)
    assert "cvx_seg_pipeline_aug" in declared and "cvx_seg_pipeline_aug" in L.PROTOTYPES and hasattr(lib, "cvx_seg_pipeline_aug")
    assert len(L.PROTOTYPES["cvx_seg_pipeline_aug"][1]) == 15
    body = re.search(r"typedef struct cvx_seg_aug_job \{(.*?)\} cvx_seg_aug_job;", header, re.S).group(1)
    size = {"const uint8_t*": 8, "int32_t": 4, "float": 4}
    offset, fields = 0, {}
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        ctype, names = re.match(r"(const uint8_t\*|int32_t|float)\s+(.*)", decl).groups()
        for name in [n.strip() for n in names.split(",")]:
            m = re.match(r"(\w+)(?:\[(\d+)\])?$", name)
            fields[m.group(1)] = offset
            offset += size[ctype] * int(m.group(2) or 1)
    dt = seg_pipeline.SEG_AUG_JOB_DTYPE
    assert offset == 128 == dt.itemsize
    assert fields == {name: dt.fields[name][1] for name in dt.names}
    assert [fields[k] for k in ("image", "mask", "ih", "mask_channels", "cos", "sin", "flags", "beta", "alpha", "sat", "hue", "blur_k", "taps",
                                "reserved")] == [0, 8, 16, 44, 48, 52, 56, 60, 64, 68, 72, 76, 80, 116]
    old = seg_pipeline.SEG_JOB_DTYPE                                          # the first 48 bytes are cvx_seg_job's
    assert all(dt.fields[k][1] == old.fields[k][1] for k in old.names if k != "reserved") and old.itemsize == 64
    for name, bit in (("BRIGHTNESS", 1), ("CONTRAST", 2), ("CONTRAST_LAST", 4), ("SATURATION", 8), ("HUE", 16), ("BLUR", 32)):
        assert re.search(rf"#define CVX_SEG_AUG_{name} {bit}\b", header) and getattr(seg_pipeline, "AUG_" + name) == bit == getattr(A, name)


@pytest.mark.parametrize("size,base,crop", SHAPES)
def test_neutral_job_of_the_restatement_is_the_old_pipeline(size, base, crop):
    """cos = 1, sin = 0, no flags, no blur, the origin inside: the fp32 restatement against image_torch -- equal where that path is
    bit-exact today (the identity resize), within 4 d elsewhere (d = |torch fp32 - fp64 restatement|, the rule of
    test_seg_pipeline_gpu.py) --, its fp64 form equal to image64, and the labels equal to labels_torch away from half-integers"""
    H, W = crop
    rh, rw = S.resized_size(*size, base)
    picture = S.synth_picture(size[0], size[1], seed=size[0])
    labels = S.blocky_labels(size[0], size[1], seed=60)
    for i, j, flip in ((0, 0, 0), (rh - H, rw - W, 1), ((rh - H) // 2, (rw - W) // 2, 1)):
        old = dict(ih=size[0], iw=size[1], rh=rh, rw=rw, i=i, j=j, flip=flip)
        jb = A.job(size[0], size[1], rh, rw, i, j, flip)
        got = A.image(picture, jb, H, W)
        want = S.image_torch(picture, old, H, W).numpy()
        exact = S.image64(picture, old, H, W)
        d = float(np.abs(exact - want.astype(np.float64)).max())
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{size} -> {rh} x {rw} at ({i}, {j}) flip {flip}: restatement - torch {err:.3e}, d {d:.3e}")
        assert err <= 4 * d
        if (size[0], size[1]) == (rh, rw):
            assert np.array_equal(got, want)
        assert np.array_equal(A.image(picture, jb, H, W, dt=np.float64), exact)
        for mode in ("bilinear", "nearest"):
            t = A.targets(labels, jb, H, W, mode)
            safe = ~S.near_half(S.labels64(labels, old, H, W)) if mode == "bilinear" else np.ones((H, W), bool)
            assert np.array_equal(t[safe], S.labels_torch(labels, old, H, W, mode=mode).numpy()[safe])


def test_colour_maths_against_colorsys():
    rs = np.random.RandomState(7)
    rgb = rs.rand(2000, 3)
    rgb[:50, 1] = rgb[:50, 0]                                                # ties of the maximum, greys, black and white
    rgb[50:100] = rgb[50:100, :1]
    rgb[100], rgb[101] = 0.0, 1.0
    Hd, Sv, V = A.rgb_to_hsv(rgb[:, 0], rgb[:, 1], rgb[:, 2], np.float64)
    want = np.array([colorsys.rgb_to_hsv(*p) for p in rgb])
    dh = np.abs(Hd / 360.0 - want[:, 0])
    assert np.minimum(dh, 1 - dh).max() < 1e-12 and np.abs(Sv - want[:, 1]).max() < 1e-12 and np.abs(V - want[:, 2]).max() < 1e-12
    hsv = rs.rand(2000, 3)
    hsv[:7, 0] = np.arange(7) / 6.0                                          # the sector borders, 360 degrees included
    back = np.stack(A.hsv_to_rgb(hsv[:, 0] * 360.0, hsv[:, 1], hsv[:, 2], np.float64), 1)
    assert np.abs(back - np.array([colorsys.hsv_to_rgb(*p) for p in hsv])).max() < 1e-12
    r, g, b = A.hsv_step(rgb[:, 0], rgb[:, 1], rgb[:, 2], True, 1.3, True, -200.0, np.float64)
    want = np.array([colorsys.hsv_to_rgb((h - 200.0 / 360.0) % 1.0, min(s * 1.3, 1.0), v) for h, s, v in
                     (colorsys.rgb_to_hsv(*p) for p in rgb)])
    assert np.abs(np.stack([r, g, b], 1) - want).max() < 1e-12


FULL = [dict(cos=np.cos(np.deg2rad(10)), sin=np.sin(np.deg2rad(10))), dict(flags=A.BRIGHTNESS, beta=0.11), dict(flags=A.CONTRAST, alpha=1.4),
        dict(flags=A.SATURATION, sat=1.45), dict(flags=A.HUE, hue=-17.0),
        dict(flags=63, beta=-0.08, alpha=0.6, sat=0.7, hue=15.0, blur_k=9, taps=A.gaussian_taps(9, 1.7), cos=np.cos(np.deg2rad(-7)),
             sin=np.sin(np.deg2rad(-7)))]


@pytest.mark.parametrize("k", range(len(FULL)))
def test_fp32_fp64_gap_of_the_full_pipeline(k):
    """d of the whole pipeline per case, printed: rounding noise (a handful of fp32 roundings of values below 2.7; the hue rotation
    divides by the chroma, so a nearly grey pixel amplifies its roundings) and nothing else"""
    picture = S.synth_picture(37, 53, seed=37)
    jb = A.job(37, 53, 40, 57, -3, 4, 1, **FULL[k])
    a, b = A.image(picture, jb, 33, 48), A.image(picture, jb, 33, 48, dt=np.float64)
    assert a.dtype == np.float32 and b.dtype == np.float64
    d = float(np.abs(a - b).max())
    print(f"case {k} {sorted(FULL[k])}: fp32 - fp64 {d:.3e}")
    assert d < 1e-3
    fill = (np.asarray(A.FILL, np.float64) / 255 - np.asarray(S.MEAN, np.float32)) / np.asarray(S.STD, np.float32)
    if not jb["flags"] & A.BLUR:
        outside = ~A.coords(jb, np.arange(48), np.arange(33), 33, 48)[2]
        assert outside.any() and np.abs(b[:, outside] - fill[:, None]).max() == 0.0     # padding is not distorted


def test_refusals():
    with pytest.raises(ValueError):
        seg_pipeline.DeviceSegAugmenter((33, 33), 33, train=False, recipe=RECIPE)
    with pytest.raises(ValueError):
        seg_pipeline.DeviceSegAugmenter((33, 33), 33, unlisted="ignore")                 # label_resize is bilinear by default
    with pytest.raises(ValueError):
        seg_pipeline.DeviceSegAugmenter((33, 33), 33, unlisted="void", label_resize="nearest")
    seg_pipeline.DeviceSegAugmenter((33, 33), 33, unlisted="ignore", label_resize="nearest", train=False)
    for kernel in (4, 11, 1):
        with pytest.raises(ValueError):
            seg_pipeline.DeviceSegAugmenter((33, 33), 33, recipe=dict(blur=dict(kernel=kernel, sigma=(0.1, 2.0), p=0.5)))
    with pytest.raises(ValueError):
        seg_pipeline.DeviceSegAugmenter((33, 33), 33, recipe=dict(zoom=(0.5, 2.0)))
    aug = seg_pipeline.DeviceSegAugmenter((33, 33), 33, seed=0, recipe=RECIPE)
    with pytest.raises(CvxError):                                            # no CPU path
        aug([torch.zeros(20, 20, 3, dtype=torch.uint8)], [torch.zeros(20, 20, dtype=torch.uint8)])
    with pytest.raises(CvxError):
        seg_pipeline.DeviceSegAugmenter((33, 33), 33, unlisted="ignore", label_resize="nearest")(
            [torch.zeros(40, 40, 3, dtype=torch.uint8)], [torch.zeros(40, 40, dtype=torch.uint8)])
    assert aug._aug_fields({}) == (1.0, 0.0, 0, 0.0, 1.0, 1.0, 0.0, 0, (0.0,) * 9)
    for bad in (dict(blur_k=4, flags=32, taps=(0.25,) * 4), dict(blur_k=3, flags=0, taps=(0.3,) * 3), dict(blur_k=5, flags=32, taps=(0.3,) * 3),
                dict(flags=64), dict(cos=float("nan")), dict(hue=400.0, flags=16)):
        with pytest.raises(CvxError):
            aug._aug_fields(bad)
