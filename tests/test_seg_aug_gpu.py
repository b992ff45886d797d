"""GPU: ``cvx_seg_pipeline_aug`` through ``DeviceSegAugmenter(recipe=...)`` -- neutral jobs against ``cvx_seg_pipeline`` (equal), full jobs
against the fp32 restatement (tests/seg_aug_restatement.py, equal), exact geometric identities, padding against torch on the CPU,
``unlisted="ignore"``, and the DeepLabv3+ trainer fed by a recipe loader."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_aug_restatement as A
import seg_pipeline_restatement as S
from computervision.pytorch_amd import seg_pipeline
from core.algorithms.segmentation_2d import voc_colormap

pytestmark = pytest.mark.gpu

SIZES = [(37, 53), (40, 29), (5, 7), (48, 120)]        # the pictures of test_seg_pipeline_gpu.SHAPES
LABEL_SEED = 60
CMAP = voc_colormap()
RECIPE = dict(scale=(0.5, 2.0), rotate=dict(degrees=10, p=0.5),
              photometric=dict(brightness=32, contrast=(0.5, 1.5), saturation=(0.5, 1.5), hue=18, p=0.5),
              blur=dict(kernel=5, sigma=(0.1, 2.0), p=0.5), fill=(124, 116, 104))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(dev):
    """per picture size: the picture, the colour mask with a few pixels of an unlisted colour, the labels it stands for (unlisted ->
    class 0) and their device copies"""
    out = {}
    for ih, iw in SIZES:
        raw = S.blocky_labels(ih, iw, seed=LABEL_SEED)
        unknown = [(0, 0), (ih - 1, iw - 1), (ih // 2, iw // 3)]
        mask = S.colour_mask(raw, CMAP, unknown)
        labels = S.label_indices(mask, CMAP)
        picture = S.synth_picture(ih, iw, seed=ih)
        out[(ih, iw)] = dict(picture=picture, mask=mask, labels=labels, unknown=unknown, d_picture=torch.from_numpy(picture).to(dev),
                             d_mask=torch.from_numpy(mask).to(dev), d_labels=torch.from_numpy(labels.astype(np.uint8)).to(dev))
    return out


def run(case, crop, jobs, colour=True, label_resize="bilinear", recipe=None, **kw):
    aug = seg_pipeline.DeviceSegAugmenter(crop, 33, colormap=CMAP if colour else None, label_resize=label_resize, recipe=recipe, **kw)
    images, targets = aug.apply(jobs, [case["d_picture"]] * len(jobs), [case["d_mask"] if colour else case["d_labels"]] * len(jobs))
    assert images.dtype == torch.float32 and targets.dtype == torch.int64
    assert tuple(images.shape) == (len(jobs), 3) + tuple(crop) and tuple(targets.shape) == (len(jobs),) + tuple(crop)
    return images.cpu(), targets.cpu()


def rot(deg):
    a = np.deg2rad(np.float64(deg))
    return dict(cos=np.cos(a), sin=np.sin(a))


# ---- 1. neutral jobs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,base,crop", [((37, 53), 33, (33, 33)), ((40, 29), 33, (33, 33)), ((5, 7), 33, (33, 33)), ((48, 120), 48, (32, 48)),
                                            ((48, 120), 80, (70, 37))])
def test_neutral_jobs_equal_cvx_seg_pipeline(cases, size, base, crop):
    """cos = 1, sin = 0, no flags, no blur, the origin in range: outputs and targets of the new entry equal the old entry's, both label
    modes, colour and index masks"""
    case, (H, W) = cases[size], crop
    rh, rw = S.resized_size(*size, base)
    mi, mj = rh - H, rw - W
    old = [dict(ih=size[0], iw=size[1], rh=rh, rw=rw, i=i, j=j, flip=f) for i, j, f in ((0, 0, 0), (mi, mj, 1), (mi // 2, mj // 2, 1), (mi, 0, 0))]
    old.append(dict(ih=size[0], iw=size[1], rh=H, rw=W, i=0, j=0, flip=0))                        # the validation job
    new = [A.job(**p) for p in old]
    for label_resize in ("bilinear", "nearest"):
        for colour in (True, False):
            want = run(case, crop, old, colour, label_resize)
            got = run(case, crop, new, colour, label_resize, recipe={})
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (label_resize, colour)
    assert int(want[1].min()) >= 0


# ---- 2. full jobs against the fp32 restatement -----------------------------------------------------------------------------------------------
T3, T9 = A.gaussian_taps(3, 0.8), A.gaussian_taps(9, 1.7)
ALL = dict(beta=-0.08, alpha=1.35, sat=0.7, hue=15.0)
SMALL = dict(rh=17, rw=24, i=-8, j=-4)                  # 37 x 53 at zoom 0.5 inside a 33 x 33 crop: padding on all four sides
FULL = {
    "37x53 in 33x33": ((37, 53), (33, 33), [
        dict(SMALL),                                                                              # zoom 0.5, padded
        dict(rh=66, rw=94, i=20, j=30, flip=1),                                                   # zoom 2.0
        dict(rh=33, rw=47, i=0, j=7, **rot(10)),
        dict(SMALL, flip=1, **rot(-10)),
        dict(rh=33, rw=47, i=0, j=3, flags=A.BRIGHTNESS, beta=0.11),
        dict(rh=33, rw=47, i=0, j=3, flags=A.CONTRAST, alpha=1.4),
        dict(rh=33, rw=47, i=0, j=3, flags=A.CONTRAST | A.CONTRAST_LAST, alpha=0.6),
        dict(rh=33, rw=47, i=0, j=3, flags=A.SATURATION, sat=1.45),
        dict(rh=33, rw=47, i=0, j=3, flags=A.HUE, hue=-17.0),
        dict(rh=33, rw=47, i=0, j=14, flags=31 - A.CONTRAST_LAST, **ALL),                         # all together, contrast first
        dict(rh=33, rw=47, i=0, j=14, flags=31, **ALL),                                           # ... contrast last
        dict(SMALL, flags=A.BLUR, blur_k=3, taps=T3),                                             # blur across the picture / fill border
        dict(SMALL, flags=A.BLUR, blur_k=9, taps=T9),
        dict(rh=33, rw=47, i=0, j=7, flags=A.BLUR, blur_k=9, taps=T9),                            # ... across the tile borders at 32
        dict(rh=40, rw=57, i=-3, j=20, flip=1, flags=63, blur_k=9, taps=T9, **ALL, **rot(-7)),
        dict(rh=33, rw=47, i=0, j=0),                                                             # no blur beside blurred images
    ]),
    "48x120 in 70x37": ((48, 120), (70, 37), [
        dict(rh=96, rw=240, i=10, j=100, flags=63, blur_k=9, taps=T9, **ALL, **rot(10)),
        dict(rh=24, rw=60, i=-20, j=11, flags=A.BLUR, blur_k=3, taps=T3),
        dict(rh=24, rw=60, i=-46, j=23, flip=1, flags=A.BLUR | A.HUE, hue=170.0, blur_k=9, taps=T9),
        dict(rh=48, rw=120, i=-11, j=-2, **rot(-10)),
    ]),
    "5x7 in 32x48": ((5, 7), (32, 48), [
        dict(rh=33, rw=46, i=1, j=-1, flags=A.BLUR | A.HUE | A.SATURATION, hue=-18.0, sat=1.5, blur_k=5, taps=A.gaussian_taps(5, 0.1), **rot(10)),
        dict(rh=66, rw=92, i=17, j=22, flip=1, flags=A.BLUR, blur_k=7, taps=A.gaussian_taps(7, 2.0)),
        dict(rh=16, rw=23, i=-9, j=-20, flags=31, **ALL),
    ]),
}


@pytest.mark.parametrize("name", list(FULL))
def test_full_jobs_equal_the_fp32_restatement(cases, name):
    """one launch per group, blurred and unblurred images side by side: every image equals the fp32 restatement bit for bit; so do the
    targets, bilinear from an index mask and nearest from a colour mask.  The fp32 - fp64 gap d of each job is printed."""
    size, crop, specs = FULL[name]
    case, (H, W) = cases[size], crop
    jobs = [A.job(size[0], size[1], **spec) for spec in specs]
    images, t_bilinear = run(case, crop, jobs, colour=False, recipe={})
    _, t_nearest = run(case, crop, jobs, colour=True, label_resize="nearest", recipe={})
    for n, jb in enumerate(jobs):
        want = A.image(case["picture"], jb, H, W)
        d = float(np.abs(want - A.image(case["picture"], jb, H, W, dt=np.float64)).max())
        err = float(np.abs(images[n].numpy() - want).max())
        outside = int((~A.coords(jb, np.arange(W), np.arange(H), H, W)[2]).sum())
        print(f"{name} job {n}: flags {jb['flags']} k {jb['blur_k']}: {outside} pixels outside, kernel - restatement {err:.3e}, d {d:.3e}")
        assert np.array_equal(images[n].numpy(), want), (n, specs[n], err)
        assert np.array_equal(t_bilinear[n].numpy(), A.targets(case["labels"], jb, H, W, "bilinear")), (n, specs[n])
        assert np.array_equal(t_nearest[n].numpy(), A.targets(case["labels"], jb, H, W, "nearest")), (n, specs[n])
    if name == "37x53 in 33x33":
        padded = ~A.coords(jobs[0], np.arange(W), np.arange(H), H, W)[2]
        assert padded[0].all() and padded[-1].all() and padded[:, 0].all() and padded[:, -1].all() and not padded[16, 16]
        assert (t_nearest[0].numpy()[padded] == -100).all() and (t_nearest[0].numpy()[~padded] >= 0).all()


# ---- 3. exact identities -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,crop,origin", [((37, 53), (33, 33), (0, 7)), ((48, 120), (70, 37), (-11, 40))])
def test_half_turn_is_a_flip_over_both_axes(cases, size, crop, origin):
    case = cases[size]
    rh, rw = S.resized_size(*size, 48)
    base = dict(rh=rh, rw=rw, i=origin[0], j=origin[1], flags=A.BRIGHTNESS | A.HUE, beta=0.05, hue=12.0)
    jobs = [A.job(size[0], size[1], **base), A.job(size[0], size[1], cos=-1.0, sin=0.0, **base), A.job(size[0], size[1], flip=1, **base),
            A.job(size[0], size[1], flip=1, cos=-1.0, sin=0.0, **base)]
    for label_resize in ("bilinear", "nearest"):
        x, t = run(case, crop, jobs, label_resize=label_resize, recipe={})
        for k in (0, 2):
            assert torch.equal(x[k + 1], torch.flip(x[k], (-2, -1))) and torch.equal(t[k + 1], torch.flip(t[k], (-2, -1)))
    assert not torch.equal(x[0], x[1])


def test_quarter_turns_are_rot90(cases):
    size, crop = (37, 53), (33, 33)
    base = dict(rh=33, rw=47, i=0, j=9, flags=A.SATURATION, sat=1.2)
    jobs = [A.job(*size, **base), A.job(*size, cos=0.0, sin=1.0, **base), A.job(*size, cos=0.0, sin=-1.0, **base)]
    for label_resize in ("bilinear", "nearest"):
        x, t = run(cases[size], crop, jobs, label_resize=label_resize, recipe={})
        assert torch.equal(x[1], torch.rot90(x[0], -1, (-2, -1))) and torch.equal(t[1], torch.rot90(t[0], -1, (-2, -1)))
        assert torch.equal(x[2], torch.rot90(x[0], 1, (-2, -1))) and torch.equal(t[2], torch.rot90(t[0], 1, (-2, -1)))
    assert not torch.equal(x[0], x[1])


# ---- 4. padding against torch -----------------------------------------------------------------------------------------------------------------
def padded_torch(picture, labels, jb, H, W, fill, ignore_index):
    """F.interpolate to (rh, rw), a canvas of fill / ignore_index around it, crop, flip, normalise: (3, H, W) fp32, (H, W) int64, inside"""
    rh, rw, i, j = jb["rh"], jb["rw"], jb["i"], jb["j"]
    x = torch.from_numpy(np.ascontiguousarray(picture)).permute(2, 0, 1).float().div(255)
    x = F.interpolate(x[None], size=(rh, rw), mode="bilinear", align_corners=False)[0]
    t = F.interpolate(torch.from_numpy(labels).float()[None, None], size=(rh, rw), mode="nearest")[0, 0].long()
    m = max(H, W) + max(abs(i), abs(j))                                      # margin of the canvas
    canvas = (torch.tensor(fill, dtype=torch.float32) / 255).view(3, 1, 1).repeat(1, rh + 2 * m, rw + 2 * m)
    canvas[:, m:m + rh, m:m + rw] = x
    tc = torch.full((rh + 2 * m, rw + 2 * m), ignore_index, dtype=torch.long)
    tc[m:m + rh, m:m + rw] = t
    inside = torch.zeros(rh + 2 * m, rw + 2 * m, dtype=torch.bool)
    inside[m:m + rh, m:m + rw] = True
    cut = [a[..., m + i:m + i + H, m + j:m + j + W] for a in (canvas, tc, inside)]
    if jb["flip"]:
        cut = [a.flip(-1) for a in cut]
    img = (cut[0].clone() - torch.tensor(S.MEAN).view(3, 1, 1)) / torch.tensor(S.STD).view(3, 1, 1)
    return img, cut[1], cut[2]


@pytest.mark.parametrize("size,crop,spec", [((37, 53), (33, 33), dict(rh=17, rw=24, i=-8, j=-4)),
                                            ((40, 29), (70, 37), dict(rh=45, rw=33, i=-10, j=-2, flip=1)),
                                            ((5, 7), (32, 48), dict(rh=9, rw=13, i=-11, j=-20)),
                                            ((48, 120), (70, 37), dict(rh=96, rw=240, i=60, j=220, flip=1))])
def test_padding_against_torch(cases, size, crop, spec):
    """label_resize="nearest".  Inside the picture the image is within 4 d of torch (d = max |torch fp32 - fp64 restatement| over the
    inside pixels, from the references alone; the rule of test_seg_pipeline_gpu.py) and the labels are exact; outside, the image is
    exactly (fill / 255 - mean) / std and the target exactly ignore_index."""
    case, (H, W) = cases[size], crop
    jb = A.job(size[0], size[1], **spec)
    fill, ignore = (124, 116, 104), -100
    x, t = run(case, crop, [jb], label_resize="nearest", recipe=dict(fill=fill))
    want, want_t, inside = padded_torch(case["picture"], case["labels"], jb, H, W, fill, ignore)
    assert bool(inside.any()) and bool((~inside).any())
    assert np.array_equal(inside.numpy(), A.coords(jb, np.arange(W), np.arange(H), H, W)[2])
    exact = A.image(case["picture"], jb, H, W, fill=fill, dt=np.float64)
    d = float(np.abs(exact - want.double().numpy())[:, inside.numpy()].max())
    err = float((x[0] - want)[:, inside].abs().max())
    print(f"{size} -> {jb['rh']} x {jb['rw']} at ({jb['i']}, {jb['j']}) in {crop}: kernel - torch {err:.3e}, d {d:.3e}")
    assert err <= 4 * d
    assert torch.equal(x[0][:, ~inside], want[:, ~inside])
    assert torch.equal(t[0], want_t) and bool((t[0][~inside] == ignore).all()) and bool((t[0][inside] >= 0).all())


# ---- 5. unlisted colours ----------------------------------------------------------------------------------------------------------------------
def test_unlisted_colours_become_ignore_index(cases):
    """the hand-placed pixels of an unlisted colour: ignore_index with unlisted="ignore" (with and without a recipe, training and
    validation), class 0 by default"""
    size, crop = (48, 120), (32, 48)
    case = cases[size]
    assert all(case["labels"][y, x] == 0 for y, x in case["unknown"])
    old = [dict(ih=48, iw=120, rh=48, rw=120, i=0, j=0, flip=0), dict(ih=48, iw=120, rh=48, rw=120, i=16, j=72, flip=1)]
    val = dict(ih=48, iw=120, rh=32, rw=48, i=0, j=0, flip=0)
    for ignore in (-100, 255):
        marked = A.label_indices_or(case["mask"], CMAP, ignore)
        assert int((marked == ignore).sum()) == 3
        _, t = run(case, crop, old, label_resize="nearest", unlisted="ignore", ignore_index=ignore)                # no recipe
        for job, got in zip(old, t):
            assert torch.equal(got, S.labels_torch(marked, job, 32, 48, mode="nearest"))
        assert int((t[0] == ignore).sum()) == 2 and int((t[1] == ignore).sum()) == 1 and t[0, 24, 40] == ignore and t[0, 0, 0] == ignore and t[1, 31, 0] == ignore
        _, tv = run(case, crop, [val], label_resize="nearest", unlisted="ignore", ignore_index=ignore, train=False)
        assert torch.equal(tv[0], S.labels_torch(marked, val, 32, 48, mode="nearest"))
        _, tr = run(case, crop, [A.job(**p) for p in old], label_resize="nearest", unlisted="ignore", ignore_index=ignore, recipe={})
        assert torch.equal(tr, t)
    _, t0 = run(case, crop, [A.job(**p) for p in old], label_resize="nearest", recipe={})
    assert torch.equal(t0, run(case, crop, old, label_resize="nearest")[1]) and t0[0, 0, 0] == 0 and int(t0.min()) == 0


# ---- 6. the trainer ---------------------------------------------------------------------------------------------------------------------------
def test_trainer_with_a_recipe_loader(dev):
    """DeeplabV3PlusTrainer at 97 x 129 fed by a recipe DeviceSegLoader whose source holds pictures smaller than the crop: a train step
    with a finite loss, no bad targets, ignore_index among the targets, and identical batches from a second loader with the seed"""
    import builder
    cfg, _, trainer_cls = builder.export_from_registry("deeplabv3plus")
    cfg.arch.input_size, cfg.arch.crop_size, cfg.train.batch_size = (3, 97, 129), (97, 129), 2
    torch.manual_seed(0)
    source = []
    for k, (h, w) in enumerate([(60, 80), (97, 129), (40, 30), (75, 140)]):
        labels = S.blocky_labels(h, w, seed=k, cell=16)
        source.append((torch.from_numpy(S.synth_picture(h, w, seed=k)), torch.from_numpy(S.colour_mask(labels, CMAP, [(1, 1)]))))

    def loader(seed):
        aug = seg_pipeline.DeviceSegAugmenter((97, 129), 129, colormap=CMAP, seed=seed, recipe=RECIPE, label_resize="nearest", unlisted="ignore")
        return seg_pipeline.DeviceSegLoader(source, 2, aug, length=3, device=dev)

    train_loader = loader(5)
    val_aug = seg_pipeline.DeviceSegAugmenter((97, 129), 129, colormap=CMAP, train=False, label_resize="nearest", unlisted="ignore")
    tr = trainer_cls(cfg, dev, dataloader=train_loader, val_dataloader=seg_pipeline.DeviceSegLoader(source, 2, val_aug, device=dev))
    assert tr.train_dataloader is train_loader
    tr.model.train()
    a, b, c = list(train_loader), list(loader(5)), list(loader(6))
    assert len(a) == 3 and all(tuple(x.shape) == (2, 3, 97, 129) and tuple(t.shape) == (2, 97, 129) for x, t in a)
    for (xa, ta), (xb, tb) in zip(a, b):
        assert torch.equal(xa, xb) and torch.equal(ta, tb)
    assert not all(torch.equal(xa, xc) for (xa, _), (xc, _) in zip(a, c))
    targets = torch.cat([t for _, t in a])
    assert bool((targets == -100).any()) and bool(((targets == -100) | ((targets >= 0) & (targets <= 20))).all())
    assert bool(torch.isfinite(torch.cat([x for x, _ in a])).all())
    loss = float(tr.train_loop(a[0], None)[0])
    assert np.isfinite(loss) and not tr.criterion.bad_targets()
