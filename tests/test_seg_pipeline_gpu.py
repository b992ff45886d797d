"""GPU: ``cvx_seg_pipeline`` through ``DeviceSegAugmenter`` / ``DeviceSegLoader`` against torch on the CPU (tests/seg_pipeline_restatement.py),
``cvx_seg_criterion_eval`` through ``SegmentationMetrics.add_rows`` against the unfused device path (exact) and against torch on the CPU, and the
DeepLabv3+ trainer with device loaders on both sides."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_pipeline_restatement as S
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import seg_pipeline
from computervision.pytorch_amd.deeplab import SegLoss
from core.algorithms.segmentation_2d import voc_colormap
from core.trainer.segmentation_trainer import SegmentationMetrics

pytestmark = pytest.mark.gpu

# (source size, base, crop): down- and upscaling on either axis, the identity (no draw), a 5 x 7 picture blown up, a non-square crop
SHAPES = [((37, 53), 33, (33, 33)), ((40, 29), 33, (33, 33)), ((33, 33), 33, (33, 33)), ((21, 64), 33, (33, 33)), ((5, 7), 33, (33, 33)),
          ((48, 120), 48, (32, 48))]
LABEL_SEED = 60                             # blocky_labels: at most 2 % of the resized labels within 1e-3 of a half-integer at every shape
CMAP = voc_colormap()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def jobs_of(size, base, crop):
    """hand-made training jobs -- both flips, the origin at 0, in the middle and at its maximum -- and the validation job"""
    (ih, iw), (H, W) = size, crop
    rh, rw = S.resized_size(ih, iw, base)
    mi, mj = rh - H, rw - W
    train = [dict(ih=ih, iw=iw, rh=rh, rw=rw, i=i, j=j, flip=f) for i, j, f in ((0, 0, 0), (mi, mj, 1), (mi // 2, mj // 2, 1), (mi, 0, 0))]
    return train, dict(ih=ih, iw=iw, rh=H, rw=W, i=0, j=0, flip=0)


@pytest.fixture(scope="module")
def cases():
    """per shape: the picture, its labels, the colour mask with a few pixels of an unlisted colour, and the labels the mask stands for"""
    out = []
    for size, base, crop in SHAPES:
        ih, iw = size
        labels = S.blocky_labels(ih, iw, seed=LABEL_SEED)
        unknown = [(0, 0), (ih - 1, iw - 1), (ih // 2, iw // 3)]
        mask = S.colour_mask(labels, CMAP, unknown)
        out.append(dict(size=size, base=base, crop=crop, picture=S.synth_picture(ih, iw, seed=ih), mask=mask, labels=S.label_indices(mask, CMAP),
                        raw_labels=labels, unknown=unknown))
    return out


def run(dev, case, jobs, train, colour=True, label_resize="bilinear"):
    aug = seg_pipeline.DeviceSegAugmenter(case["crop"], case["base"], colormap=CMAP if colour else None, train=train, label_resize=label_resize)
    pic = torch.from_numpy(case["picture"]).to(dev)
    mask = torch.from_numpy(case["mask"] if colour else case["labels"].astype(np.uint8)).to(dev)
    images, targets = aug.apply(jobs, [pic] * len(jobs), [mask] * len(jobs))
    assert images.dtype == torch.float32 and targets.dtype == torch.int64 and images.device == targets.device == dev
    assert tuple(images.shape) == (len(jobs), 3) + tuple(case["crop"]) and tuple(targets.shape) == (len(jobs),) + tuple(case["crop"])
    return images.cpu(), targets.cpu()


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_image_parity_with_torch(dev, cases, k):
    """Against torch-CPU F.interpolate -> crop -> flip -> normalise.  The bound is taken from the references alone: d = max |torch fp32 -
    fp64 restatement| of the same job, and the kernel must be within 4 d of torch: two fp32 evaluations with different operation order
    and contraction, each about d from the exact value, with room for the division by std.  The 33 x 33 -> 33 x 33 case is bit-exact."""
    case = cases[k]
    H, W = case["crop"]
    train, val = jobs_of(case["size"], case["base"], case["crop"])
    got = torch.cat([run(dev, case, train, True)[0], run(dev, case, [val], False)[0]])
    for job, g in zip(train + [val], got):
        want = S.image_torch(case["picture"], job, H, W)
        d = float(np.abs(S.image64(case["picture"], job, H, W) - want.double().numpy()).max())
        err = float((g - want).abs().max())
        print(f"{case['size']} -> {job['rh']} x {job['rw']} at ({job['i']}, {job['j']}) flip {job['flip']}: kernel - torch {err:.3e}, d {d:.3e}")
        assert err <= 4 * d, (job, err, d)
        if (job["ih"], job["iw"]) == (job["rh"], job["rw"]):
            assert torch.equal(g, want), job


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_label_parity_with_torch(dev, cases, k):
    """Exact against torch.round(F.interpolate(labels.float())) -> crop -> flip, except at pixels whose fp64 interpolated value lies within
    1e-3 of a half-integer (at most 2 % of the resized label picture, computed from the reference alone).  Unlisted colours are class
    0; an index mask gives the targets of the colour mask; label_resize="nearest" is exact against F.interpolate(mode="nearest").
    The validation job of the 48 x 120 picture (48 -> 32 rows, 120 -> 48 columns: the scales are 1.5 and 2.5, every lambda is 0.25 or
    0.75 and the labels are at most 20, so every product and sum is exact in fp32 whatever the order) is compared on ALL its pixels:
    several per cent of them are exact .5 ties, about half of those above an even integer, where half-to-even and half-away part."""
    case = cases[k]
    H, W = case["crop"]
    train, val = jobs_of(case["size"], case["base"], case["crop"])
    assert all(case["labels"][y, x] == 0 for y, x in case["unknown"]) and any(case["raw_labels"][y, x] != 0 for y, x in case["unknown"])
    got = torch.cat([run(dev, case, train, True)[1], run(dev, case, [val], False)[1]])
    by_index = torch.cat([run(dev, case, train, True, colour=False)[1], run(dev, case, [val], False, colour=False)[1]])
    assert torch.equal(got, by_index)
    nearest = torch.cat([run(dev, case, train, True, label_resize="nearest")[1], run(dev, case, [val], False, label_resize="nearest")[1]])
    for job, g, n in zip(train + [val], got, nearest):
        assert torch.equal(n, S.labels_torch(case["labels"], job, H, W, mode="nearest")), job
        if job is val and case["size"] == (48, 120):
            values = S.labels64(case["labels"], job, H, W)                   # exact in fp64 too
            ties = values - np.floor(values) == 0.5
            down = ties & (np.floor(values) % 2 == 0)                        # half-to-even rounds these down, half-away-from-zero up
            want = S.labels_torch(case["labels"], job, H, W)
            print(f"{case['size']} -> {job['rh']} x {job['rw']}: {int(ties.sum())} exact ties of {ties.size} pixels, {int(down.sum())} above an "
                  f"even integer, {int((g != want).sum())} pixels differ")
            assert int(ties.sum()) >= 0.03 * ties.size and int(down.sum()) >= 16 and int((ties & ~down).sum()) >= 16
            assert np.array_equal(want.numpy()[ties], np.rint(values)[ties])   # the pin itself rounds half to even
            assert torch.equal(g, want), job
            continue
        whole = dict(job, i=0, j=0, flip=0)
        share = float(S.near_half(S.labels64(case["labels"], whole, job["rh"], job["rw"])).mean())
        assert share <= 0.02, share
        safe = torch.from_numpy(~S.near_half(S.labels64(case["labels"], job, H, W)))
        want = S.labels_torch(case["labels"], job, H, W)
        print(f"{case['size']} -> {job['rh']} x {job['rw']}: {share:.2%} of the labels near a half-integer, {int((~safe).sum())} pixels left out, "
              f"{int((g != want)[safe].sum())} of the others differ")
        assert torch.equal(g[safe], want[safe]), job
        assert int(g.min()) >= 0 and int(g.max()) <= 20


def test_loader(dev, cases):
    """the training loader wraps around and honours its length; validation walks the source once with a short last batch (3, 3, 1 of 7);
    two loaders with one seed yield identical batches"""
    source = [(torch.from_numpy(cases[k % 5]["picture"]), torch.from_numpy(cases[k % 5]["mask"])) for k in range(7)]

    def loader(train, seed=3, **kw):
        aug = seg_pipeline.DeviceSegAugmenter((33, 33), 33, colormap=CMAP, train=train, seed=seed)
        return seg_pipeline.DeviceSegLoader(source, 3, aug, device=dev, **kw)

    a, b = list(loader(True, length=4)), list(loader(True, length=4))
    assert len(a) == 4 and all(tuple(x.shape) == (3, 3, 33, 33) and tuple(t.shape) == (3, 33, 33) for x, t in a)     # 12 items of 7: wraps around
    for (xa, ta), (xb, tb) in zip(a, b):
        assert xa.dtype == torch.float32 and ta.dtype == torch.int64 and xa.device == ta.device == dev
        assert torch.equal(xa, xb) and torch.equal(ta, tb)
    c = list(loader(True, seed=4, length=4))
    assert not all(torch.equal(xa, xc) for (xa, _), (xc, _) in zip(a, c))
    v = list(loader(False))
    assert [x.shape[0] for x, _ in v] == [3, 3, 1] and [t.shape[0] for _, t in v] == [3, 3, 1]
    assert [x.shape[0] for x, _ in loader(False, drop_last=True)] == [3, 3]
    job = dict(ih=40, iw=29, rh=33, rw=33, i=0, j=0, flip=0)                 # item 1 of the source is the 40 x 29 picture
    assert float((v[0][0][1].cpu() - S.image_torch(cases[1]["picture"], job, 33, 33)).abs().max()) < 1e-5


# ---- cvx_seg_criterion_eval -------------------------------------------------------------------------------------------------------------------------------
EVAL_SHAPES = [(2, 25, 33, 97, 129, 21, 0), (1, 9, 9, 33, 33, 21, 1), (3, 17, 12, 65, 45, 5, 0), (1, 5, 6, 40, 48, 21, 0)]


def eval_inputs(B, ih, iw, H, W, nc):
    g = torch.Generator().manual_seed(B * 1000 + H + nc)
    ld = (nc + 7) & ~7
    rows = torch.zeros(B, ih * iw, ld)
    rows[..., :nc] = torch.randn(B, ih * iw, nc, generator=g) * 2
    t = torch.randint(0, nc, (B, H, W), generator=g)
    t[torch.rand(B, H, W, generator=g) < 0.15] = -100
    return rows, t, ld


def add_rows(dev, rows, t, hw, nc, mode, metrics=None):
    metrics = metrics or SegmentationMetrics(nc, device=dev)
    slot = torch.zeros(3, device=dev)
    metrics.add_rows(rows.to(dev), t.to(dev), hw, SegLoss("focal" if mode == 0 else "ce"), slot[1:2])
    assert float(slot[0]) == 0.0 and float(slot[2]) == 0.0                  # the slot the caller chose, nothing beside it
    return metrics, float(slot[1])


def confusion_of(pred, t, nc):
    keep = (t >= 0) & (t < nc)
    return torch.bincount(nc * t[keep] + pred[keep], minlength=nc * nc).reshape(nc, nc)


@pytest.mark.parametrize("B,ih,iw,H,W,nc,mode", EVAL_SHAPES)
def test_seg_eval_equals_the_unfused_device_path(dev, B, ih, iw, H, W, nc, mode):
    """the confusion matrix against bincount over torch.argmax(cvx_resize_bilinear_rows_to_nchw(rows)) on the device: exact, because
    both interpolate with one device function; its sum is the number of non-ignored targets; a second call accumulates; rows whose
    stride is not a multiple of 8 floats (scalar loads) give the same matrix"""
    lib = L.load()
    rows, t, ld = eval_inputs(B, ih, iw, H, W, nc)
    logits = torch.empty(B, nc, H, W, device=dev)
    rd = rows.to(dev)
    L.check(lib.cvx_resize_bilinear_rows_to_nchw(L.ptr(rd), ld, B, nc, ih, iw, H, W, L.ptr(logits), L.stream_ptr(dev)), "rows_to_nchw")
    want = confusion_of(torch.argmax(logits, dim=1), t.to(dev), nc).cpu()
    m, loss = add_rows(dev, rows, t, (ih, iw), nc, mode)
    assert m.counts.dtype == torch.int64 and torch.equal(m.counts.cpu(), want)
    assert int(m.counts.sum()) == int((t != -100).sum())
    _, loss2 = add_rows(dev, rows, t, (ih, iw), nc, mode, m)
    assert torch.equal(m.counts.cpu(), 2 * want) and loss2 == loss
    assert float(m.confusion_matrix.sum()) == 0.0                            # the float64 matrix get_results reads takes them in at fold()
    assert m.fold().dtype == torch.float64 and torch.equal(m.confusion_matrix.cpu(), 2 * want.double()) and int(m.counts.sum()) == 0
    rows_odd = torch.zeros(B, ih * iw, nc + 1)
    rows_odd[..., :nc] = rows[..., :nc]
    m_odd, loss_odd = add_rows(dev, rows_odd, t, (ih, iw), nc, mode)
    assert torch.equal(m_odd.counts.cpu(), want) and abs(loss_odd - loss) <= 1e-6 * abs(loss)
    m.reset()
    assert int(m.counts.sum()) == 0 and float(m.confusion_matrix.sum()) == 0.0


def test_seg_eval_counts_in_global_memory_for_many_classes(dev):
    """nc = 96: 9216 cells do not fit the 8192 of the LDS histogram, so every pixel goes to the global matrix; ties go to the lowest class"""
    lib = L.load()
    B, ih, iw, H, W, nc = 2, 7, 9, 27, 35, 96
    rows, t, ld = eval_inputs(B, ih, iw, H, W, nc)
    rows[0, :, :nc] = 0.0                                                    # image 0: all logits equal, arg max 0
    logits = torch.empty(B, nc, H, W, device=dev)
    rd = rows.to(dev)
    L.check(lib.cvx_resize_bilinear_rows_to_nchw(L.ptr(rd), ld, B, nc, ih, iw, H, W, L.ptr(logits), L.stream_ptr(dev)), "rows_to_nchw")
    want = confusion_of(torch.argmax(logits, dim=1), t.to(dev), nc).cpu()
    m, _ = add_rows(dev, rows, t, (ih, iw), nc, 1)
    assert torch.equal(m.counts.cpu(), want)
    assert int(m.counts[:, 0].sum()) >= int((t[0] != -100).sum())


@pytest.mark.parametrize("B,ih,iw,H,W,nc,mode", EVAL_SHAPES)
def test_seg_eval_against_torch_on_the_cpu(dev, B, ih, iw, H, W, nc, mode):
    """the loss within 2e-5 relative of torch's fp32 value (the bound cvx_seg_criterion_loss is held to); the matrix within 2 x (the number of
    pixels whose fp64 top-two logit gap is below 1e-4) of the CPU matrix in L1 -- such a pixel may move from one cell to another -- and
    those pixels are at most 0.5 % of all (the seed is that of test_seg_loss_kernel_against_torch; the reference alone shows the share)"""
    rows, t, ld = eval_inputs(B, ih, iw, H, W, nc)
    rr = rows[..., :nc].reshape(B, ih, iw, nc).permute(0, 3, 1, 2).contiguous()
    logits = F.interpolate(rr, size=(H, W), mode="bilinear", align_corners=False)
    if mode == 0:
        ce = F.cross_entropy(logits, t, ignore_index=-100, reduction="none")
        ref = float((0.25 * (1 - torch.exp(-ce)) ** 2 * ce).mean())
    else:
        ref = float(F.cross_entropy(logits, t, reduction="mean"))
    top2 = F.interpolate(rr.double(), size=(H, W), mode="bilinear", align_corners=False).topk(2, dim=1).values
    close = int(((top2[:, 0] - top2[:, 1]) < 1e-4).sum())
    assert close <= 0.005 * B * H * W
    m, loss = add_rows(dev, rows, t, (ih, iw), nc, mode)
    l1 = int((m.counts.cpu() - confusion_of(torch.argmax(logits, dim=1), t, nc)).abs().sum())
    print(f"loss {loss:.7f} torch {ref:.7f} rel {abs(loss - ref) / abs(ref):.2e}; {close} close pixels, matrix L1 distance {l1}")
    assert abs(loss - ref) < 2e-5 * abs(ref), (loss, ref)
    assert l1 <= 2 * close, (l1, close)


# ---- the trainer -------------------------------------------------------------------------------------------------------------------------------
def test_trainer_with_device_loaders(dev, tmp_path):
    """DeeplabV3PlusTrainer at 97 x 129 (the size of the model's training fixture) with DeviceSegLoaders on both sides: one train step,
    the fused evaluate_loop against the unfused loop on the same batches -- the four accuracies identical (equal integer counts), the
    loss within 2e-5 relative -- and evaluate_on_voc's report"""
    import builder
    cfg, _, trainer_cls = builder.export_from_registry("deeplabv3plus")
    cfg.arch.input_size, cfg.arch.crop_size, cfg.train.batch_size = (3, 97, 129), (97, 129), 2
    torch.manual_seed(0)
    source = []
    for k, (h, w) in enumerate([(60, 80), (97, 129), (120, 90), (75, 140), (64, 64)]):
        labels = S.blocky_labels(h, w, seed=k, cell=16)
        source.append((torch.from_numpy(S.synth_picture(h, w, seed=k)), torch.from_numpy(S.colour_mask(labels, CMAP, [(1, 1)]))))
    base = max(cfg.arch.input_size[1:])
    train_loader = seg_pipeline.DeviceSegLoader(source, 2, seg_pipeline.DeviceSegAugmenter((97, 129), base, colormap=CMAP, seed=1), length=3, device=dev)
    val_loader = seg_pipeline.DeviceSegLoader(source, 2, seg_pipeline.DeviceSegAugmenter((97, 129), base, colormap=CMAP, train=False), device=dev)
    tr = trainer_cls(cfg, dev, dataloader=train_loader, val_dataloader=val_loader)
    assert tr.train_dataloader is train_loader and tr.val_dataloader is val_loader and len(val_loader) == 3
    tr.model.train()
    batch = next(iter(train_loader))
    assert tuple(batch[0].shape) == (2, 3, 97, 129) and tuple(batch[1].shape) == (2, 97, 129)
    loss = float(tr.train_loop(batch, None)[0])
    assert np.isfinite(loss) and not tr.criterion.bad_targets()
    fused = tr.evaluate_loop()
    assert set(fused) == {"Loss", "Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU"}
    assert int(tr.metrics.confusion_matrix.sum()) == 5 * 97 * 129 and int(tr.metrics.counts.sum()) == 0      # every pixel of the five, short last batch included
    path = tr.model_algorithm.evaluate_on_voc(tr.model, str(tmp_path), dataloader=val_loader)
    tr._injected_val_loader, tr.val_dataloader = None, list(val_loader)      # the same batches through the unfused loop
    unfused = tr.evaluate_loop()
    print(f"fused {fused}\nunfused {unfused}")
    for key in ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU"):
        assert fused[key] == unfused[key], key
    assert np.isfinite(fused["Loss"]) and abs(fused["Loss"] - unfused["Loss"]) <= 2e-5 * abs(unfused["Loss"])
    assert os.path.dirname(path) == os.path.join(str(tmp_path), "DeepLabV3Plus") and os.path.basename(path).startswith("DeepLabV3Plus_")
    lines = open(path, encoding="utf-8").read().split("\n")
    assert [ln.split(": ")[0] for ln in lines] == ["Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU"]
    assert [float(ln.split(": ")[1]) for ln in lines] == [fused[k] for k in ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU")]
    with pytest.raises(ValueError):
        tr.model_algorithm.evaluate_on_voc(tr.model, str(tmp_path), subset="test", dataloader=val_loader)
