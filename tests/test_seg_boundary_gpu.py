"""MI355X: the boundary metrics.  ``cvx_seg_boundary`` (csrc/seg_boundary.hip) against the numpy restatement
(tests/seg_boundary_restatement.py): the six distance planes and the three tables as integers -- no tolerance exists in this feature.  The
shapes are the smallest that break each mechanism of three tiled passes with 64 x 32 tiles and a halo of the frame's widest band: every
size around one and two tiles, a band wider than the map, a band whose halo spans several tiles, widths that differ per frame, one and
eight widths, the class counts on either side of the LDS tables.  Then ``DeeplabV3PlusA.segment_tiled(boundary=)`` and
``evaluate_on_voc(boundary=)`` end to end."""
import functools

import numpy as np
import pytest
import torch

from computervision.pytorch_amd import seg_boundary as SB
import seg_boundary_restatement as BR

pytestmark = pytest.mark.gpu

T_H, T_W = 32, 64                        # the tile of csrc/seg_boundary.hip


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def padded(dev, host, extra, fill):
    """``host`` (h, w) on the device as a view whose rows are ``extra`` elements longer, the padding filled with ``fill``"""
    h, w = host.shape
    store = torch.full((h, w + extra), fill, dtype=torch.uint8, device=dev)
    view = store[:, :w]
    view.copy_(torch.from_numpy(host))
    assert view.stride(0) == w + extra
    return view, store


def reference(preds, targets, nc, widths):
    """per frame the restatement's dict, and the three tables summed over the frames"""
    frames = [BR.counts(p, g, nc, wd) for p, g, wd in zip(preds, targets, widths)]
    total = {k: sum(f[k] for f in frames) for k in ("trimap", "biou", "bf")}
    return frames, total


def assert_equal(got, frames, total, what=""):
    """the tables of the BoundaryCounts ``got`` against ``total`` and, where it has planes, each frame's against the restatement's"""
    for name in ("trimap", "biou", "bf"):
        have = getattr(got, name).cpu().numpy()
        print(f"{what} {name}: sum {int(have.sum())} (want {int(total[name].sum())}), {int((have != total[name]).sum())} cells differ")
        assert have.dtype == np.int64 and np.array_equal(have, total[name]), (what, name)
    if got.planes is not None:
        for f, want in enumerate(frames):
            if want is None:
                continue
            have = got.planes[f].cpu().numpy()
            wrong = [int((have[i] != want["planes"][i]).sum()) for i in range(6)]
            print(f"{what} frame {f} {have.shape[1:]}: plane mismatches {wrong}, widest distance {int(want['planes'][:4].max())}")
            assert wrong == [0] * 6, (what, f)


# ---- 1. every size around one and two tiles, widths that differ per frame -----------------------------------------------------------------------
SIZES = [(1, 1), (1, 200), (200, 1)] + [(h, w) for h in (T_H - 1, T_H, T_H + 1, 2 * T_H + 1) for w in (T_W - 1, T_W, T_W + 1, 2 * T_W + 1)]
RATIOS = (0.02, 0.08)


@functools.lru_cache(maxsize=None)
def sizes_case():
    targets = [BR.blobby(h, w, 100 + i, classes=3, cell=7) for i, (h, w) in enumerate(SIZES)]
    preds = [BR.jitter(g, 200 + i, 3, wild=True) for i, g in enumerate(targets)]
    widths = [[BR.ratio_width(r, h, w) for r in RATIOS] for h, w in SIZES]
    return targets, preds, widths, reference(preds, targets, 3, widths)


def test_sizes_around_the_tile_in_one_ragged_batch(dev):
    """19 frames in one call under a ratio spec: the widths run from (1, 1) at 1 x 1 to (4, 16) at 1 x 200, so the frames of the batch
    stage halos of different depths.  Blobby targets with void outlines, predictions moved by a pixel with values >= nc among them."""
    targets, preds, widths, (frames, total) = sizes_case()
    assert len({tuple(w) for w in widths}) >= 6 and widths[0] == [1, 1] and widths[1] == [4, 16] and max(max(w) for w in widths) == 16
    got = SB.boundary_counts([on(dev, p) for p in preds], [on(dev, g) for g in targets], 3, SB.SegBoundary(ratio=RATIOS), planes=True)
    assert got.widths == widths
    assert_equal(got, frames, total, "sizes")
    assert total["trimap"].min() > 0 and total["bf"][..., 0].min() > 0                      # every class and every cell takes part


# ---- 2. widths: 1 alone, 64 on a map smaller than 64 and on one whose halo spans several tiles, eight at once ----------------------------------
@functools.lru_cache(maxsize=None)
def wide_case():
    targets = [BR.blobby(40, 50, 31, classes=3, cell=17), BR.blobby(70, 150, 32, classes=3, cell=23)]
    targets[1][:, 80:] = 2                                                                  # a stretch wider than the widest band
    preds = [BR.jitter(g, 41 + i, 3, share=0.002) for i, g in enumerate(targets)]
    widths = [[1, 2, 3, 5, 8, 13, 21, 64]] * 2
    return targets, preds, widths, reference(preds, targets, 3, widths)


def test_eight_widths_up_to_64(dev):
    """K = 8.  At width 64 the 40 x 50 map lies inside every window, and the 70 x 150 map's windows reach across all of its 3 x 3 tiles;
    distances between 22 and 64 occur, and so does 65, "none within 64"."""
    targets, preds, widths, (frames, total) = wide_case()
    seen = np.unique(frames[1]["planes"][:4])
    assert seen.max() == 65 and ((seen > 21) & (seen < 65)).any()
    got = SB.boundary_counts([on(dev, p) for p in preds], [on(dev, g) for g in targets], 3, SB.SegBoundary(widths[0]), planes=True)
    assert_equal(got, frames, total, "wide")
    assert (np.diff(total["biou"][:, :, 1], axis=0) >= 0).all() and total["biou"][7, :, 1].sum() > total["biou"][6, :, 1].sum()


def test_one_width_of_one_on_the_patterns(dev):
    """K = 1, d = 1: a checkerboard (every pixel is band and contour), one class only, stripes one pixel wide (both ways), a void-only
    target, and a prediction equal to its target"""
    blob = BR.blobby(50, 90, 5, classes=3)
    targets = [BR.checkerboard(33, 65), np.full((40, 70), 1, np.uint8), BR.stripes(35, 66), BR.stripes(66, 35, vertical=False),
               np.full((20, 30), 255, np.uint8), blob]
    preds = [BR.checkerboard(33, 65, 1, 0), np.full((40, 70), 1, np.uint8), BR.stripes(35, 66), np.roll(targets[3], 1, 0),
             BR.checkerboard(20, 30), blob.copy()]
    widths = [[1]] * 6
    frames, total = reference(preds, targets, 3, widths)
    assert frames[0]["planes"][:4].max() == 1 and (frames[0]["planes"][4:] > 0).all()       # the checkerboard: all band, all contour
    assert not frames[1]["trimap"].any() and not frames[1]["bf"].any() and frames[1]["biou"][0, 1].tolist() == [216] * 3
    assert not any(frames[4][k].any() for k in ("trimap", "biou", "bf", "planes"))          # a void target: no count, planes 0
    got = SB.boundary_counts([on(dev, p) for p in preds], [on(dev, g) for g in targets], 3, SB.SegBoundary((1,)), planes=True)
    assert_equal(got, frames, total, "patterns")


def test_a_prediction_equal_to_the_target_folds_to_exactly_one(dev):
    g = BR.blobby(70, 150, 6, classes=4)
    m = SB.BoundaryMetrics(4, SB.SegBoundary((1, 4, 15)), dev)
    m.add_labels([on(dev, g)], [on(dev, g)])
    r = m.get_results()
    assert [r[name][d] for name in ("Trimap mIoU", "Boundary IoU", "BF") for d in (1, 4, 15)] == [1.0] * 9
    assert int(m.trimap.sum()) > 0 and int(m.bf.sum()) > 0
    m.reset()
    assert not m.trimap.any() and not m.biou.any() and not m.bf.any()


# ---- 3. class counts on either side of the LDS tables ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 21, 255])
def test_class_counts(dev, nc):
    """nc = 1: one class and void.  nc = 21 at K = 2: the trimap cells (882) sit in LDS.  nc = 255 at K = 2: 130 050 cells do not, the counts
    go to the global table directly -- and the map uses the top classes, 250 .. 254; 255 stays void."""
    h, w = 45, 100
    g = BR.blobby(h, w, 60 + nc, classes=5, cell=8)
    if nc == 1:
        g[(g != 0) & (g != 255)] = 255
        p = BR.jitter(g, 70, 2)
    else:
        lift = nc - 5
        p = BR.jitter(g, 70 + nc, 5, wild=False)
        g[g != 255] += lift
        p += lift
        p[3, 4:9] = 255                                                                      # a prediction may say 255 too: void
    frames, total = reference([p], [g], nc, [[2, 6]])
    assert total["trimap"].sum() > 0 and (nc == 1 or (total["trimap"][:, nc - 1, nc - 1] > 0).all())
    got = SB.boundary_counts([on(dev, p)], [on(dev, g)], nc, SB.SegBoundary((2, 6)), planes=True)
    assert_equal(got, frames, total, f"nc {nc}")


# ---- 4. padded views, a frame that is not there, accumulation, repeatability ---------------------------------------------------------------
def test_padded_views_a_null_frame_and_accumulation(dev):
    sizes = [(37, 70), (33, 129), (20, 20)]
    targets = [BR.blobby(h, w, 80 + i, classes=3) for i, (h, w) in enumerate(sizes)]
    preds = [BR.jitter(g, 90 + i, 3, wild=True) for i, g in enumerate(targets)]
    spec = SB.SegBoundary((1, 3, 9))
    frames, total = reference(preds[:2], targets[:2], 3, [[1, 3, 9]] * 2)
    d_pred = [padded(dev, preds[0], 5, 1)[0], on(dev, preds[1]), None]                      # garbage that is a class in the padding
    d_target = [on(dev, targets[0]), padded(dev, targets[1], 3, 2)[0], on(dev, targets[2])]
    got = SB.boundary_counts(d_pred, d_target, 3, spec, planes=True)
    assert_equal(got, frames + [None], total, "padded")
    assert not got.planes[2].any()                                                           # the frame without a prediction is skipped
    again = SB.boundary_counts(d_pred, d_target, 3, spec, out=(got.trimap, got.biou, got.bf))
    assert again.trimap is got.trimap
    assert_equal(again, [], {k: 2 * v for k, v in total.items()}, "second call")             # the tables are added to


def test_two_calls_from_zeroed_tables_give_the_same_bytes(dev):
    targets = [BR.blobby(97, 131, 21, classes=4), BR.checkerboard(64, 64)]
    preds = [BR.jitter(targets[0], 22, 4, wild=True), BR.stripes(64, 64, 2)]
    d_pred, d_target = [on(dev, p) for p in preds], [on(dev, g) for g in targets]
    spec = SB.SegBoundary((1, 2, 4, 8, 15))
    a = SB.boundary_counts(d_pred, d_target, 4, spec, planes=True)
    kept = [t.clone() for t in (a.trimap, a.biou, a.bf, *a.planes)]
    b = SB.boundary_counts(d_pred, d_target, 4, spec, planes=True)
    for x, y in zip(kept, (b.trimap, b.biou, b.bf, *b.planes)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    frames, total = reference(preds, targets, 4, [[1, 2, 4, 8, 15]] * 2)
    assert_equal(b, frames, total, "repeat")


def test_int64_targets_and_a_batch_tensor(dev):
    """``BoundaryMetrics.add_labels`` with a (B, H, W) uint8 prediction and int64 targets: values outside [0, nc) are void"""
    g = np.stack([BR.blobby(40, 66, 7, classes=3), BR.blobby(40, 66, 8, classes=3)])
    p = np.stack([BR.jitter(g[0], 9, 3), BR.jitter(g[1], 10, 3)])
    t64 = g.astype(np.int64)
    t64[g == 255] = -100
    t64[0, 5, 5:9] = 1000
    g[0, 5, 5:9] = 255
    m = SB.BoundaryMetrics(3, SB.SegBoundary(ratio=(0.05,)), dev)
    got = m.add_labels(on(dev, p), on(dev, t64))
    assert got.widths == [[4]] * 2
    frames, total = reference(list(p), list(g), 3, [[4]] * 2)
    assert_equal(got, frames, total, "int64")
    r = m.get_results()
    want = SB.fold_counts(total["trimap"], total["biou"], total["bf"], (0.05,))
    assert all(r[name] == want[name] for name in ("Trimap mIoU", "Boundary IoU", "BF")) and 0 < r["BF"][0.05] < 1 and set(r["Boundary IoU"]) == {0.05}


# ---- 5. end to end, random weights --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deeplab(dev):
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    cfg = DeeplabV3PlusConfig()
    cfg.arch.input_size, cfg.arch.backbone_pretrained = (3, 65, 97), False                  # the input of tests/test_seg_tta_gpu.py
    algo = DeeplabV3PlusA(cfg, dev)
    assert algo.num_classes == 21
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    return algo, model


def test_segment_tiled_with_boundary_equals_boundary_counts_on_its_maps(dev, deeplab):
    from core.trainer.segmentation_trainer import SegmentationMetrics
    algo, model = deeplab
    rng = np.random.RandomState(51)
    host = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((100, 150), (65, 97))]
    targets = [on(dev, BR.blobby(h, w, 52 + i, classes=21, cell=11)) for i, (h, w) in enumerate(((100, 150), (65, 97)))]
    spec = SB.SegBoundary((1, 4))
    bm = SB.BoundaryMetrics(21, spec, dev)
    labels = algo.segment_tiled(model, [on(dev, a) for a in host], overlap=0.2, batch_size=4, draw=False, targets=targets, boundary=bm)
    assert [tuple(l.shape) for l in labels] == [(100, 150), (65, 97)]
    want = SB.boundary_counts(labels, targets, 21, spec)
    for name in ("trimap", "biou", "bf"):
        assert torch.equal(getattr(bm, name), getattr(want, name)) and int(getattr(want, name).sum()) > 0, name
    frames, total = reference([l.cpu().numpy() for l in labels], [t.cpu().numpy() for t in targets], 21, [[1, 4]] * 2)
    assert_equal(want, frames, total, "segment_tiled")
    # with metrics as well: the confusion counts are the stitch's, the boundary tables double
    metrics = SegmentationMetrics(21, dev)
    again = algo.segment_tiled(model, [on(dev, a) for a in host], overlap=0.2, batch_size=4, draw=False, targets=targets, metrics=metrics,
                               boundary=bm)
    assert all(torch.equal(a, b) for a, b in zip(again, labels))
    assert int(metrics.counts.sum()) == sum(int((t < 21).sum()) for t in targets) and torch.equal(bm.trimap, 2 * want.trimap)


def two_batches(dev, seed, nc=21, hw=(65, 97)):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(2):
        images = torch.rand(2, 3, *hw, generator=g)
        coarse = torch.randint(0, nc, (2, 1, 5, 7), generator=g).float()
        targets = torch.nn.functional.interpolate(coarse, size=hw, mode="nearest")[:, 0].long()
        targets[torch.rand(2, *hw, generator=g) < 0.03] = -100
        out.append((images.to(dev), targets.to(dev)))
    return out


def report(path):
    return open(path, encoding="utf-8").read().splitlines()


def test_evaluate_on_voc_with_boundary_writes_four_and_six_lines(dev, deeplab, tmp_path, monkeypatch):
    from core.trainer.segmentation_trainer import SegmentationMetrics
    algo, model = deeplab
    nc = algo.num_classes
    loader = two_batches(dev, 61)
    spec = SB.SegBoundary((1, 4))
    preds, targets = [], []
    confusion = np.zeros((nc, nc), np.int64)
    for images, t in loader:
        labels = algo.predict_labels(model, images, scales=(1.0,), flip=False, fuse="prob").cpu().numpy()
        t = t.cpu().numpy()
        valid = (t >= 0) & (t < nc)
        np.add.at(confusion, (t[valid], labels[valid]), 1)
        preds += list(labels)
        targets += list(np.where(valid, t, 255).astype(np.uint8))
    _, total = reference(preds, targets, nc, [[1, 4]] * 4)
    assert total["trimap"].sum() > 0 and total["bf"].sum() > 0
    plain = SegmentationMetrics(nc)
    plain.confusion_matrix += torch.from_numpy(confusion).double()
    r = plain.get_results()
    want = [f"{k}: {r[k]}" for k in ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU")]
    want += SB.report_lines(SB.fold_counts(total["trimap"], total["biou"], total["bf"], (1, 4)), (1, 4))
    got = report(algo.evaluate_on_voc(model, str(tmp_path / "boundary"), dataloader=loader, boundary=spec))
    print(got)
    assert len(got) == 4 + 6 and [l.split(":")[0] for l in got[4:]] == ["Trimap mIoU@1", "Boundary IoU@1", "BF@1", "Trimap mIoU@4", "Boundary IoU@4", "BF@4"]
    assert got == want
    # without the keyword: the four old lines, and cvx_seg_boundary is never called
    calls = []
    real = SB.boundary_counts
    monkeypatch.setattr(SB, "boundary_counts", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    old = report(algo.evaluate_on_voc(model, str(tmp_path / "plain"), dataloader=loader))
    tta = report(algo.evaluate_on_voc(model, str(tmp_path / "tta"), dataloader=loader, scales=(1.0,), fuse="prob"))
    rng = np.random.RandomState(3)
    algo.segment_tiled(model, [on(dev, rng.randint(0, 256, (70, 100, 3), dtype=np.uint8))], draw=False)
    assert calls == []
    assert len(old) == 4 and [l.split(":")[0] for l in old] == ["Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU"]
    assert tta == got[:4]                                                                    # boundary= alone is the one-view fusion
    SB.BoundaryMetrics(nc, spec, dev).add_labels([on(dev, preds[0])], [on(dev, targets[0])])
    assert calls == [1]                                                                      # the wrapper does count


def test_boundary_counts_does_not_synchronise(dev):
    g = [on(dev, BR.blobby(70, 90, 11)), on(dev, BR.blobby(40, 200, 12))]
    p = [on(dev, BR.jitter(t.cpu().numpy(), 13 + i, 3)) for i, t in enumerate(g)]
    m = SB.BoundaryMetrics(3, SB.SegBoundary((1, 4)), dev)
    m.add_labels(p, g)                                                                       # first use: code objects, workspace, tables
    first = m.trimap.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=dev).item()
            flags = False
        except RuntimeError:
            flags = True
        print(f"set_sync_debug_mode('error') flags a read-back on this build: {flags}")
        m.add_labels(p, g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(m.trimap, 2 * first)
