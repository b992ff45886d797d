"""MI355X: multi-scale / flip test-time augmentation.  ``cvx_seg_tta_inputs`` and mode 0 of ``cvx_seg_fuse`` (csrc/seg_tta.hip) against the
numpy restatement (tests/seg_tta_restatement.py) bit for bit; mode 1 within a derived bound; the identities that tie the fusion to
``cvx_seg_criterion_eval``; and ``DeeplabV3PlusA.predict_labels`` / ``evaluate_on_voc`` end to end against the restatement's fusion of the rows the
network returned.

The bound on mode 1's probabilities, 1e-5 absolute, is derived and not measured: the z_k are bit-identical to the restatement's, and what
remains per view is one rounded subtraction (z - m is off by at most 6e-8 * |z - m|, so e by less than 1e-6 relative wherever e is not
negligible beside the largest term, which is exactly 1), expf at a few ulp (3e-7), an fp32 sum of at most 24 terms (1.4e-6 relative at
worst), one division (6e-8) and, over the views, a sum and one division by their number -- on a probability p <= 1 together about 2e-6 at
these sizes, and 1e-5 leaves a factor of five.  (The largest difference measured on an MI355X is in DESIGN.md section 7n.)  A label is
compared where the restatement's float64 top-2 margin exceeds 2e-5 -- twice the bound, since both probabilities may move -- and
tests/test_seg_tta_cpu.py shows for these very inputs that under 1 % of the pixels are left out."""
import numpy as np
import pytest
import torch

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import seg_tta as T
import seg_tta_restatement as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def device_views(dev, views):
    return [T.SegView(torch.from_numpy(rows).to(dev), (lh, lw), flip) for rows, lh, lw, flip in views]


# ---- 1. cvx_seg_tta_inputs against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("scale", [0.5, 0.75, 1.0, 1.5])
@pytest.mark.parametrize("hw", [(65, 97), (64, 50)])
@pytest.mark.parametrize("B", [1, 3])
def test_inputs_equal_the_restatement(dev, B, hw, scale, flip):
    h, w = hw
    oh, ow = int(np.floor(h * scale + 0.5)), int(np.floor(w * scale + 0.5))          # view_size's rule without its 33-pixel floor
    x = np.random.RandomState(10 * B + h).rand(B, 3, h, w).astype(np.float32)
    want = TR.tta_inputs(x, oh, ow, flip)
    d_x = torch.from_numpy(x).to(dev)
    got = T.tta_inputs(d_x, (oh, ow), flip)
    assert tuple(got.shape) == (B * (2 if flip else 1), 3, oh, ow) and got.dtype == torch.float32
    diff = np.abs(got.cpu().numpy() - want)
    print(f"{hw} -> {(oh, ow)}, flip {flip}: max |difference| {diff.max():.3g}")
    assert np.array_equal(got.cpu().numpy(), want)
    if scale == 1.0:
        assert torch.equal(got[:B], d_x) and (not flip or torch.equal(got[B:], torch.flip(d_x, dims=[3])))


# ---- 2. cvx_seg_fuse, mode 0, against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", TR.FUSE_BATCHES)
@pytest.mark.parametrize("n_views", TR.FUSE_TABLES)
@pytest.mark.parametrize("out_hw", TR.FUSE_OUTPUTS)
@pytest.mark.parametrize("nc,ld", TR.FUSE_SHAPES)
def test_fuse_logits_equals_the_restatement(dev, nc, ld, out_hw, n_views, batch):
    views, targets = TR.fuse_case(nc, ld, out_hw, n_views, batch)
    geometry = [(lh, lw) for _, lh, lw, _ in views]
    assert len(set(geometry)) == n_views and (n_views == 1 or (geometry[0] == (9, 13) and geometry[-1] == (29, 43)))
    assert n_views == 1 or 0 < sum(f for _, _, _, f in views) < n_views                         # mixed flip flags
    want = TR.labels_logits(views, nc, *out_hw)
    want_counts = TR.confusion(want, targets, nc)
    counts = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    d_views, d_targets = device_views(dev, views), torch.from_numpy(targets).to(dev)
    labels = T.fuse(d_views, nc, ld, out_hw, targets=d_targets, counts=counts, mode="logits")
    got = labels.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (batch,) + tuple(out_hw)
    wrong = int((got != want).sum())
    print(f"nc {nc} ld {ld} {out_hw} views {n_views} batch {batch}: {wrong} label mismatches of {got.size}, classes {np.unique(want).size}")
    assert wrong == 0
    assert np.unique(want).size == nc                                                            # the case bites: every class wins somewhere
    assert want_counts.sum() > 0 and np.array_equal(counts.cpu().numpy(), want_counts)
    assert T.fuse(d_views, nc, ld, out_hw, targets=d_targets, counts=counts, mode="logits", labels=False) is None
    assert np.array_equal(counts.cpu().numpy(), 2 * want_counts)                                 # the counts are added to, never cleared


def test_fuse_counts_128_classes_with_direct_atomics(dev):
    """nc * nc = 16384 cells do not fit the 32 KB LDS histogram: every pixel goes to the matrix directly, as in cvx_seg_criterion_eval"""
    nc = ld = 128
    rng = np.random.RandomState(9)
    views = [((3.0 * rng.standard_normal((2, lh * lw, ld))).astype(np.float32), lh, lw, flip) for lh, lw, flip in ((9, 13, False), (17, 25, True))]
    targets = rng.randint(0, 130, (2, 64, 50)).astype(np.int64)
    want = TR.labels_logits(views, nc, 64, 50)
    counts = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    labels = T.fuse(device_views(dev, views), nc, ld, (64, 50), targets=torch.from_numpy(targets).to(dev), counts=counts, mode="logits")
    assert np.array_equal(labels.cpu().numpy(), want) and np.unique(want).size > 64
    assert np.array_equal(counts.cpu().numpy(), TR.confusion(want, targets, nc))


# ---- 3. identities --------------------------------------------------------------------------------------------------------------------------
def test_one_plain_view_counts_what_seg_eval_counts(dev):
    from computervision.pytorch_amd.deeplab import SegLoss
    from core.trainer.segmentation_trainer import SegmentationMetrics
    nc, ld, out_hw = 21, 24, (65, 97)
    views, targets = TR.fuse_case(nc, ld, out_hw, 1, 3)
    (view,), d_targets = device_views(dev, views), torch.from_numpy(targets).to(dev)
    metrics = SegmentationMetrics(nc, device=dev)
    metrics.add_rows(view.rows, d_targets, view.level_hw, SegLoss("ce"), torch.zeros(1, device=dev))
    counts = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    T.fuse([view], nc, ld, out_hw, targets=d_targets, counts=counts, mode="logits", labels=False)
    assert int(counts.sum()) > 0 and torch.equal(counts, metrics.counts)


def test_a_view_listed_twice_and_a_view_with_its_mirror(dev):
    nc, ld, out_hw = 21, 24, (65, 97)
    views, _ = TR.fuse_case(nc, ld, out_hw, 1, 3)
    rows, lh, lw, _ = views[0]
    (view,) = device_views(dev, views)
    alone = T.fuse([view], nc, ld, out_hw, mode="logits")
    assert torch.equal(T.fuse([view, view], nc, ld, out_hw, mode="logits"), alone)               # z + z = 2 z, exactly
    mirrored = np.ascontiguousarray(rows.reshape(3, lh, lw, ld)[:, :, ::-1]).reshape(3, lh * lw, ld)
    both = T.fuse([view, T.SegView(torch.from_numpy(mirrored).to(dev), (lh, lw), True)], nc, ld, out_hw, mode="logits")
    assert torch.equal(both, alone)
    assert np.array_equal(alone.cpu().numpy(), TR.labels_logits(views, nc, *out_hw))


# ---- 4. mode 1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TR.PROB_CASES, ids=lambda c: f"nc{c[0]}-ld{c[1]}-{c[2][0]}x{c[2][1]}-k{c[3]}-b{c[4]}")
def test_fuse_prob_is_within_the_derived_bound(dev, case):
    nc, ld, out_hw, n_views, batch = case
    views, targets = TR.fuse_case(*case)
    want, want_p, margin = TR.labels_prob(views, nc, *out_hw)
    counts = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    labels, probs = T.fuse(device_views(dev, views), nc, ld, out_hw, targets=torch.from_numpy(targets).to(dev), counts=counts, probs=True, mode="prob")
    got, got_p = labels.cpu().numpy(), probs.cpu().numpy().astype(np.float64)
    assert got_p.shape == (batch, nc) + tuple(out_hw)
    err, total = float(np.abs(got_p - want_p).max()), float(np.abs(got_p.sum(1) - 1.0).max())
    sure = margin > TR.MARGIN
    wrong, excluded = int((got != want)[sure].sum()), float((~sure).mean())
    print(f"{case}: max |p - restatement| {err:.3g}, max |sum p - 1| {total:.3g}, {wrong} label mismatches, {excluded * 100:.3f} % of the pixels excluded")
    assert err <= 1e-5
    assert total <= 1e-5
    assert excluded < 0.01
    assert wrong == 0
    assert np.array_equal(counts.cpu().numpy(), TR.confusion(got, targets, nc))                  # the counts are of the labels written
    only = T.fuse(device_views(dev, views), nc, ld, out_hw, mode="prob")                         # labels alone: the same labels
    assert np.array_equal(only.cpu().numpy(), got)


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------------
HW, SCALES = (65, 97), (0.75, 1.0, 1.5)


@pytest.fixture(scope="module")
def deeplab(dev):
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    cfg = DeeplabV3PlusConfig()
    cfg.arch.input_size, cfg.arch.backbone_pretrained = (3,) + HW, False
    algo = DeeplabV3PlusA(cfg, dev)
    assert algo.num_classes == 21
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    return algo, model


def two_batches(dev, seed, nc=21):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        images = torch.rand(2, 3, *HW, generator=g)
        targets = torch.randint(0, nc + 1, (2,) + HW, generator=g)
        targets[targets == nc] = -100
        out.append((images.to(dev), targets.to(dev)))
    return out


def host_views(views):
    return [(v.rows.cpu().numpy(), v.level_hw[0], v.level_hw[1], v.flip) for v in views]


def test_predict_labels_equals_the_restatement_on_the_rows_of_the_views(dev, deeplab):
    algo, model = deeplab
    nc = algo.num_classes
    images = two_batches(dev, 50)[0][0]
    tta = T.SegTTA(SCALES, flip=True, mode="logits")
    views = tta.run(model, images)                                   # the rows forward_rows returned for the views, read from the device
    assert [(tuple(v.rows.shape[:1]), v.flip) for v in views] == [((2,), False), ((2,), True)] * 3
    assert len({v.level_hw for v in views}) == 3 and all(v.rows.shape[2] == model.layout.nc_pad == 24 for v in views)
    want = TR.labels_logits(host_views(views), nc, *HW)
    labels = algo.predict_labels(model, images, scales=SCALES, flip=True, fuse="logits")
    got = labels.cpu().numpy()
    print(f"predict_labels: {int((got != want).sum())} label mismatches of {got.size}, classes {np.unique(got).tolist()}")
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (2,) + HW and np.array_equal(got, want)
    assert np.unique(want).size > 1
    colours = algo.predict_tensor(model, images, scales=SCALES, flip=True, fuse="logits")
    from core.algorithms.segmentation_2d import voc_colormap
    assert torch.equal(colours, torch.tensor(voc_colormap(), device=dev)[labels.long()])
    l2, p = algo.predict_labels(model, images, scales=SCALES, flip=True, fuse="prob", probs=True)
    assert tuple(p.shape) == (2, nc) + HW and l2.dtype == torch.uint8
    finite = torch.isfinite(p).all(1)
    print(f"mean probabilities: {int((~finite).sum())} of {finite.numel()} pixels are not finite")
    assert int(finite.sum()) > 0 and float((p.sum(1)[finite] - 1).abs().max()) <= 1e-5


def report(path):
    return open(path, encoding="utf-8").read().splitlines()


def test_evaluate_on_voc_with_one_plain_view_writes_the_plain_numbers(dev, deeplab, tmp_path):
    """scale 1 without flip in "logits" mode is the plain evaluation: the input launch copies the batch bit for bit and 0 + z = z.  Where
    a logit of the random-weight network is not finite the two arg max rules differ by design (cvx_seg_criterion_eval starts from -inf, the fusion
    from class 0 as the stitch does), so those pixels' targets are set to ignored -- in both runs."""
    algo, model = deeplab
    loader = two_batches(dev, 51)
    with torch.no_grad():
        for images, targets in loader:
            bad = ~torch.isfinite(model(images)).all(1)
            print(f"{int(bad.sum())} of {bad.numel()} pixels have a non-finite logit")
            assert int(bad.sum()) < bad.numel()
            targets[bad] = -100
    plain = report(algo.evaluate_on_voc(model, str(tmp_path / "plain"), dataloader=loader))
    fused = report(algo.evaluate_on_voc(model, str(tmp_path / "tta"), dataloader=loader, scales=(1.0,), flip=False, fuse="logits"))
    print(plain, fused)
    assert len(plain) == 4 and [l.split(":")[0] for l in plain] == ["Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU"]
    assert fused == plain


def test_evaluate_on_voc_counts_the_restatements_matrix_without_a_host_wait(dev, deeplab, tmp_path, monkeypatch):
    from core.trainer import segmentation_trainer as ST
    algo, model = deeplab
    nc = algo.num_classes
    batches = two_batches(dev, 52)
    tta = T.SegTTA(SCALES, flip=True, mode="logits")
    want = np.zeros((nc, nc), np.int64)
    for images, targets in batches:                                   # also the first use of every engine and code object
        want += TR.confusion(TR.labels_logits(host_views(tta.run(model, images)), nc, *HW), targets.cpu().numpy(), nc)
    torch.cuda.synchronize()
    state = {"flagged": None}

    class Loader:
        """the two batches; a read-back between the first batch and the end of the iteration raises"""

        def __len__(self):
            return 2

        def __iter__(self):
            torch.cuda.set_sync_debug_mode("error")
            try:
                if state["flagged"] is None:
                    try:
                        torch.ones(1, device=dev).item()
                        state["flagged"] = False
                    except RuntimeError:
                        state["flagged"] = True
                yield from batches
            finally:
                torch.cuda.set_sync_debug_mode("default")

    seen = {}
    real = ST.SegmentationMetrics.get_results

    def keep_counts(self):
        seen["counts"] = self.counts.cpu().numpy().copy()
        return real(self)

    monkeypatch.setattr(ST.SegmentationMetrics, "get_results", keep_counts)
    try:
        path = algo.evaluate_on_voc(model, str(tmp_path), dataloader=Loader(), scales=SCALES, flip=True, fuse="logits")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not state["flagged"]:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a read-back on this build")
    assert want.sum() > 0 and np.array_equal(seen["counts"], want)
    expected = ST.SegmentationMetrics(nc)
    expected.confusion_matrix += torch.from_numpy(want).double()
    r = real(expected)
    assert report(path) == [f"{k}: {r[k]}" for k in ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU")]


def test_host_tensors_and_bad_arguments_are_refused(dev, deeplab):
    algo, model = deeplab
    images = torch.rand(2, 3, *HW)
    with pytest.raises(CvxError):
        algo.predict_labels(model, images)                           # host images
    with pytest.raises(ValueError):
        algo.predict_labels(model, images.to(dev), scales=(0.4,))    # 26 x 39: below the engine's minimum input
    with pytest.raises(ValueError):
        algo.predict_labels(model, images.to(dev), fuse="mean")
    with pytest.raises(ValueError):
        algo.predict_labels(model, images.to(dev), fuse="logits", probs=True)
    with pytest.raises(ValueError):
        algo.predict_labels(model, images.to(dev), scales=[1.0] * 9, flip=True)
    view = T.SegView(torch.zeros(2, 6, 4, device=dev), (2, 3), False)
    good = dict(nc=3, ld=4, out_hw=(7, 9))
    counts = torch.zeros(3, 3, dtype=torch.int64, device=dev)
    targets = torch.zeros(2, 7, 9, dtype=torch.long, device=dev)
    with pytest.raises(CvxError):
        T.fuse([view, T.SegView(torch.zeros(2, 6, 4), (2, 3), False)], **good)
    for bad in (dict(targets=targets), dict(targets=targets[:1], counts=counts), dict(targets=targets, counts=counts.int()),
                dict(targets=targets, counts=counts.cpu()), dict(probs=True, mode="logits")):
        with pytest.raises(ValueError):
            T.fuse([view], **{**good, **bad})
    for bad_view in (T.SegView(view.rows, (2, 4), False), T.SegView(view.rows.half(), (2, 3), False), T.SegView(view.rows[:1], (2, 3), False)):
        with pytest.raises(ValueError):
            T.fuse([view, bad_view], **good)
    labels = T.fuse([view], targets=targets, counts=counts, **good)
    assert not labels.any() and int(counts[0, 0]) == 2 * 7 * 9 and int(counts.sum()) == int(counts[0, 0])
