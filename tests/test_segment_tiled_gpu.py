"""MI355X: sliding-window segmentation.  ``cvx_seg_stitch`` (csrc/seg_tiles.hip) against the numpy restatement
(tests/seg_tiled_restatement.py) byte for byte -- labels, overlay and the int64 confusion counts --, against ``cvx_seg_overlay`` where the two
must agree, and ``DeeplabV3PlusA.segment_tiled`` / ``segment_frames`` end to end against the same composition with the restatement's stitch
on the host.  Zero mismatches are allowed: every fp32 step of the kernel is one rounded operation and the restatement's fma is exact."""
import functools

import numpy as np
import pytest
import torch

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import render as R
import render_restatement as RS
import seg_tiled_restatement as SR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def pictures(shapes, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def on(dev, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def padded(dev, host, extra, fill=77):
    """``host`` (h, w[, 3]) uint8 on the device as a view with ``extra`` more bytes per row"""
    h, row = host.shape[0], int(np.prod(host.shape[1:]))
    store = torch.full((h, row + extra), fill, dtype=torch.uint8, device=dev)
    view = store[:, :row].view(host.shape)
    view.copy_(torch.from_numpy(host))
    assert view.stride(0) == row + extra and not view.is_contiguous()
    return view, store


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------------------------
# (70, 101): padded rows and an odd pitch (3 * 101 + 4 = 307), the byte store path; (64, 96) contiguous, the wide store path; (32, 48): one
# tile at the (32, 48) network size; (20, 30): smaller than the tile on both axes
KERNEL_FRAMES = [(70, 101), (64, 96), (32, 48), (20, 30)]


def kernel_frames(dev):
    host = pictures(KERNEL_FRAMES, 41)
    frames = on(dev, host)
    frames[0], store = padded(dev, host[0], 4)
    assert frames[0].stride(0) % 2 == 1 and frames[1].is_contiguous() and frames[1].stride(0) % 4 == 0
    return host, frames, store


@functools.lru_cache(maxsize=None)
def kernel_case(nc, ld, net_hw, level_hw, overlap):
    """the seeded inputs of one geometry, shared by its weight / bgr cases: logits drawn directly (no forward) with the padding columns
    past nc far above every class -- they must not be read as classes --, targets in [0, nc + 2) with some 255"""
    rng = np.random.RandomState(1000 * nc + 10 * net_hw[0] + int(overlap * 10))
    grids = [R.tile_grid(h, w, net_hw, overlap) for h, w in KERNEL_FRAMES]
    slots = sum(len(g) for g in grids)
    logits = rng.standard_normal((slots, level_hw[0] * level_hw[1], ld)).astype(np.float32)
    logits[..., nc:] = 100.0
    targets = [rng.randint(0, nc + 2, (h, w)).astype(np.uint8) for h, w in KERNEL_FRAMES]
    for t in targets:
        t[rng.rand(*t.shape) < 0.1] = 255
    return grids, logits, targets


@functools.lru_cache(maxsize=None)
def kernel_reference(weight, nc, ld, net_hw, level_hw, overlap):
    grids, logits, targets = kernel_case(nc, ld, net_hw, level_hw, overlap)
    labels, counts, s = [], np.zeros((nc, nc), np.int64), 0
    for f, (hw, grid) in enumerate(zip(KERNEL_FRAMES, grids)):
        labels.append(SR.stitch(hw, grid, logits[s:s + len(grid)], nc, level_hw[0], level_hw[1], net_hw[0], net_hw[1], weight))
        counts += SR.confusion(labels[-1], targets[f], nc)
        s += len(grid)
    return labels, counts


def cover_count(hw, grid):
    n = np.zeros(hw, np.int64)
    for y0, x0, th, tw in grid:
        n[y0:y0 + th, x0:x0 + tw] += 1
    return n


@pytest.mark.parametrize("overlap", [0.2, 0.6])
@pytest.mark.parametrize("net_hw,level_hw", [((32, 48), (8, 12)), ((31, 50), (8, 13))])
@pytest.mark.parametrize("nc,ld", [(3, 4), (5, 5), (21, 24)])          # the vector path, the scalar path, the production padding
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("weight", ["mean", "linear"])
def test_stitch_kernel_equals_the_restatement(dev, weight, bgr, nc, ld, net_hw, level_hw, overlap):
    grids, logits, targets = kernel_case(nc, ld, net_hw, level_hw, overlap)
    want_labels, want_counts = kernel_reference(weight, nc, ld, net_hw, level_hw, overlap)
    covers = [cover_count(hw, g) for hw, g in zip(KERNEL_FRAMES, grids)]
    assert all(c.min() >= 1 for c in covers) and covers[3].max() == 1 and len(grids[3]) == 1
    if overlap == 0.6:                                               # three tiles per axis over a pixel, and a last tile shifted back
        assert covers[0].max() == 9 and grids[0][-1][0] == 70 - net_hw[0] and grids[0][-1][1] == 101 - net_hw[1]
    if net_hw == (32, 48):
        assert len(grids[2]) == 1
    host, frames, store = kernel_frames(dev)
    d_targets = on(dev, targets)
    d_targets[0], target_store = padded(dev, targets[0], 3, fill=0)   # a target map read through its own row pitch
    tb = R.TileBatch(frames, net_hw, overlap, full_frame=False)
    assert tb.tiles == grids and tb.slots == logits.shape[0]
    counts = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    lut = R.palette(nc)
    labels = R.stitch_segmentation(frames, torch.from_numpy(logits).to(dev), nc, level_hw, net_hw, tb, weight=weight, labels=True, draw=True,
                                   bgr=bgr, targets=d_targets, counts=counts)
    torch.cuda.synchronize()
    assert len(labels) == 4
    for f, hw in enumerate(KERNEL_FRAMES):
        got = labels[f].cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == hw
        wrong = int((got != want_labels[f]).sum())
        print(f"frame {hw}: {wrong} label mismatches of {got.size}, classes present {np.unique(want_labels[f]).size}")
        assert wrong == 0, f
        assert np.array_equal(frames[f].cpu().numpy(), SR.overlay(host[f], want_labels[f], lut, bgr)), f
    assert (store[:, 3 * 101:] == 77).all() and (target_store[:, 101:] == 0).all()          # the row padding is not written
    assert want_counts.sum() > 0 and np.array_equal(counts.cpu().numpy(), want_counts)
    assert all(np.unique(w).size >= min(nc, 3) for w in want_labels[:2])                     # the case bites: several classes win


def test_stitch_outputs_are_optional(dev):
    nc, ld, net_hw, level_hw, overlap = 3, 4, (32, 48), (8, 12), 0.2
    grids, logits, targets = kernel_case(nc, ld, net_hw, level_hw, overlap)
    want_labels, want_counts = kernel_reference("linear", nc, ld, net_hw, level_hw, overlap)
    host, frames, _ = kernel_frames(dev)
    tb = R.TileBatch(frames, net_hw, overlap, full_frame=False)
    d_logits = torch.from_numpy(logits).to(dev)
    labels = R.stitch_segmentation(frames, d_logits, nc, level_hw, net_hw, tb)                # labels only: the frames stay as they were
    torch.cuda.synchronize()
    for f in range(4):
        assert np.array_equal(labels[f].cpu().numpy(), want_labels[f]) and np.array_equal(frames[f].cpu().numpy(), host[f])
    counts = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    assert R.stitch_segmentation(frames, d_logits, nc, level_hw, net_hw, tb, labels=False, targets=on(dev, targets), counts=counts) is None
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert R.stitch_segmentation(frames, d_logits, nc, level_hw, net_hw, tb, labels=False, draw=True) is None
    lut = R.palette(nc)
    for f in range(4):
        assert np.array_equal(frames[f].cpu().numpy(), SR.overlay(host[f], want_labels[f], lut)), f


# ---- 2. ties and degenerate input ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", ["mean", "linear"])
def test_ties_ignored_targets_and_accumulating_counts(dev, weight):
    nc, ld, net_hw, level_hw = 5, 8, (32, 48), (8, 12)
    host, frames, _ = kernel_frames(dev)
    tb = R.TileBatch(frames, net_hw, 0.6, full_frame=False)
    zeros = torch.zeros(tb.slots, 8 * 12, ld, dtype=torch.float32, device=dev)
    rng = np.random.RandomState(7)
    targets = [rng.randint(0, nc, hw).astype(np.uint8) for hw in KERNEL_FRAMES]
    targets[1][:] = 255                                                # a frame whose every target is ignored
    targets[0][::3] = 255
    counts = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    labels = R.stitch_segmentation(frames, zeros, nc, level_hw, net_hw, tb, weight=weight, targets=on(dev, targets), counts=counts)
    assert all(not l.any() for l in labels)                            # all logits equal: class 0 everywhere
    want = sum(SR.confusion(np.zeros(hw, np.uint8), t, nc) for hw, t in zip(KERNEL_FRAMES, targets))
    assert want[:, 1:].sum() == 0 and want.sum() == sum(int((t != 255).sum()) for t in targets)
    assert np.array_equal(counts.cpu().numpy(), want)
    R.stitch_segmentation(frames, zeros, nc, level_hw, net_hw, tb, weight=weight, labels=False, targets=on(dev, targets), counts=counts)
    assert np.array_equal(counts.cpu().numpy(), 2 * want)              # the counts are added to, never cleared


def test_counts_up_to_128_classes(dev):
    """the largest histogram the counting path keeps in LDS (64 KB)"""
    nc, ld, net_hw, level_hw = 128, 128, (32, 48), (8, 12)
    rng = np.random.RandomState(9)
    host = pictures([(40, 70)], 43)
    frames = on(dev, host)
    tb = R.TileBatch(frames, net_hw, 0.2, full_frame=False)
    logits = rng.standard_normal((tb.slots, 96, ld)).astype(np.float32)
    target = rng.randint(0, 130, (40, 70)).astype(np.uint8)
    want = SR.stitch((40, 70), tb.tiles[0], logits, nc, 8, 12, 32, 48, "linear")
    counts = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    labels = R.stitch_segmentation(frames, torch.from_numpy(logits).to(dev), nc, level_hw, net_hw, tb, targets=on(dev, [target]), counts=counts)
    assert np.array_equal(labels[0].cpu().numpy(), want) and np.unique(want).size > 20
    assert np.array_equal(counts.cpu().numpy(), SR.confusion(want, target, nc))


# ---- 3. against the existing overlay kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bgr", [False, True])
def test_one_tile_with_mean_weight_equals_seg_overlay(dev, bgr):
    """a frame of exactly the network size is one tile, the nearest-index map of cvx_seg_overlay is the identity, and fma(1, z, 0) = z"""
    nc, ld, net_hw, level_hw = 21, 24, (32, 48), (8, 12)
    host = pictures([net_hw], 44)
    rows = torch.from_numpy(np.random.RandomState(11).standard_normal((1, 96, ld)).astype(np.float32)).to(dev)
    a, b = on(dev, host), on(dev, host)
    tb = R.TileBatch(a, net_hw, 0.2, full_frame=False)
    assert tb.slots == 1
    R.stitch_segmentation(a, rows, nc, level_hw, net_hw, tb, weight="mean", labels=False, draw=True, bgr=bgr)
    R.seg_overlay(b, rows, nc, level_hw, net_hw, bgr=bgr)
    assert torch.equal(a[0], b[0]) and not torch.equal(a[0], torch.from_numpy(host[0]).to(dev))


# ---- 4. segment_tiled end to end ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deeplab(dev):
    from configs import DeeplabV3PlusConfig
    from core.algorithms.segmentation_2d import DeeplabV3PlusA
    cfg = DeeplabV3PlusConfig()
    cfg.arch.input_size, cfg.arch.backbone_pretrained = (3, 97, 129), False
    algo = DeeplabV3PlusA(cfg, dev)
    torch.manual_seed(0)
    model = algo.build_model()[0].to(dev).eval()
    return algo, model


MODEL_FRAMES = [(150, 300), (97, 129), (60, 200)]


def composition(model, frames, overlap, batch_size):
    """the expectation's device half: the same ``TileBatch`` input through ``forward_rows`` in the same chunks"""
    tb = R.TileBatch(frames, (97, 129), overlap, full_frame=False)
    x = tb.network_input()
    rows = []
    with torch.no_grad():
        for c0, c1 in R.slot_chunks(tb.slots, batch_size):
            chunk = x[c0:c1]
            rows.append(model.forward_rows(chunk if chunk.data_ptr() % 8 == 0 else chunk.clone()).clone())
    return tb, torch.cat(rows)


@pytest.mark.parametrize("weight", ["linear", "mean"])
def test_segment_tiled_equals_the_composition(dev, deeplab, weight):
    from core.trainer.segmentation_trainer import SegmentationMetrics
    algo, model = deeplab
    nc = algo.num_classes
    host = pictures(MODEL_FRAMES, 45)
    tb, rows = composition(model, on(dev, host), 0.2, 4)
    assert [len(g) for g in tb.tiles] == [6, 1, 2] and tb.slots == 9 and R.slot_chunks(9, 4) == [(0, 3), (3, 6), (6, 9)]
    lh, lw = model._last_engine.graph.level_hw[0]
    z = rows.cpu().numpy()
    rng = np.random.RandomState(46)
    targets = [rng.randint(0, nc + 1, hw).astype(np.uint8) for hw in MODEL_FRAMES]
    for t in targets:
        t[t == nc] = 255
    want_labels, want_counts, s = [], np.zeros((nc, nc), np.int64), 0
    for f, hw in enumerate(MODEL_FRAMES):
        n = len(tb.tiles[f])
        want_labels.append(SR.stitch(hw, tb.tiles[f], z[s:s + n], nc, lh, lw, 97, 129, weight))
        want_counts += SR.confusion(want_labels[-1], targets[f], nc)
        s += n
    frames = on(dev, host)
    metrics = SegmentationMetrics(nc, device=dev)
    labels = algo.segment_tiled(model, frames, overlap=0.2, weight=weight, batch_size=4, targets=on(dev, targets), metrics=metrics, sync=True)
    lut = R.palette(nc)
    for f in range(3):
        got = labels[f].cpu().numpy()
        print(f"frame {MODEL_FRAMES[f]}: {int((got != want_labels[f]).sum())} label mismatches, classes {np.unique(got).tolist()}")
        assert np.array_equal(got, want_labels[f]), f
        assert np.array_equal(frames[f].cpu().numpy(), SR.overlay(host[f], want_labels[f], lut)), f
    assert np.array_equal(metrics.counts.cpu().numpy(), want_counts)
    expected = SegmentationMetrics(nc)
    expected.confusion_matrix += torch.from_numpy(want_counts).double()
    got_r, want_r = metrics.get_results(), expected.get_results()
    assert got_r.keys() == want_r.keys()
    for k in ("Overall Acc", "Mean Acc", "FreqW Acc", "Mean IoU"):
        assert got_r[k] == want_r[k], k
    np.testing.assert_array_equal(np.array(list(got_r["Class IoU"].values())), np.array(list(want_r["Class IoU"].values())))
    if weight == "mean":
        # the (97, 129) frame alone is one slot with weight 1: fma(1, z, 0) = z, so the labels are the arg max of the resized logits
        single = [torch.from_numpy(host[1]).to(dev)]
        tb1, rows1 = composition(model, single, 0.2, 4)
        assert tb1.slots == 1
        alone = algo.segment_tiled(model, single, weight="mean", draw=False)
        resized = model.rows_to_nchw(rows1, 97, 129)[0]
        # The random-weight network overflows fp16 in places, so some logits are inf and their interpolation NaN.  torch.argmax takes a NaN
        # for the maximum; the kernel's rule is strict > from class 0 (a NaN never wins, as in cvx_seg_overlay).  Where every class is
        # finite the two are the same statement, and there torch.argmax is the expectation; everywhere, the stated rule applied to the
        # resized logits is.
        finite = torch.isfinite(resized).all(0)
        print(f"one-tile frame: {int((~finite).sum())} of {finite.numel()} pixels have a non-finite logit")
        assert int(finite.sum()) > finite.numel() // 2
        assert torch.equal(alone[0].long()[finite], torch.argmax(resized, 0)[finite])
        assert np.array_equal(alone[0].cpu().numpy(), RS.argmax_lowest(resized.cpu().numpy(), 0))
        assert torch.equal(single[0], torch.from_numpy(host[1]).to(dev))       # draw=False leaves the frame alone
        assert torch.equal(alone[0], labels[1])


def test_segment_tiled_with_an_odd_chunk(dev, deeplab):
    """3 * 97 * 129 floats per slot is odd, so a chunk from an odd slot on begins at an address the engine does not take as it is (8-byte
    alignment); 9 slots at batch_size 5 are chunks of 5 and 4"""
    algo, model = deeplab
    host = pictures(MODEL_FRAMES, 48)
    tb, rows = composition(model, on(dev, host), 0.2, 5)
    assert tb.slots == 9 and R.slot_chunks(9, 5) == [(0, 5), (5, 9)] and tb.network_input()[5:9].data_ptr() % 8 != 0
    lh, lw = model._last_engine.graph.level_hw[0]
    z, s = rows.cpu().numpy(), 0
    labels = algo.segment_tiled(model, on(dev, host), batch_size=5, draw=False)
    for f, hw in enumerate(MODEL_FRAMES):
        n = len(tb.tiles[f])
        assert np.array_equal(labels[f].cpu().numpy(), SR.stitch(hw, tb.tiles[f], z[s:s + n], algo.num_classes, lh, lw, 97, 129, "linear")), f
        s += n


def test_segment_tiled_and_segment_frames_do_not_synchronise(dev, deeplab):
    from scripts import detect
    algo, model = deeplab
    host = pictures(MODEL_FRAMES, 47)
    algo.segment_tiled(model, on(dev, host), batch_size=4, sync=False)          # first use: code objects, palette, engines
    for _ in detect.segment_frames(algo, model, iter(on(dev, host)), 2, overlap=0.2):
        pass
    once, video = on(dev, host), on(dev, host)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device=dev).item()
            caught = False
        except RuntimeError:
            caught = True
        if not caught:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a read-back on this build")
        labels = algo.segment_tiled(model, once, batch_size=4, sync=False)
        batches = list(detect.segment_frames(algo, model, iter(video), 2, overlap=0.2))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert [len(b) for b in batches] == [2, 1] and all(f is v for f, v in zip([f for b in batches for f in b], video))
    lut = R.palette(algo.num_classes)
    for f in range(3):
        want = SR.overlay(host[f], labels[f].cpu().numpy(), lut)
        assert np.array_equal(once[f].cpu().numpy(), want), f
        assert not np.array_equal(want, host[f])
    # a frame's tiles do not depend on its batch, but the forward's batch size may move a logit by an ulp: compare with the same grouping
    again = on(dev, host)
    l01 = algo.segment_tiled(model, again[:2], sync=False)
    l2 = algo.segment_tiled(model, again[2:], sync=True)
    for f, l in enumerate(l01 + l2):
        assert torch.equal(video[f], again[f]), f
        assert np.array_equal(video[f].cpu().numpy(), SR.overlay(host[f], l.cpu().numpy(), lut)), f


# ---- 5. argument validation on the device -------------------------------------------------------------------------------------------------
def test_stitch_segmentation_validates_its_arguments(dev):
    nc, ld, net_hw, level_hw = 3, 4, (32, 48), (8, 12)
    host, frames, _ = kernel_frames(dev)
    tb = R.TileBatch(frames, net_hw, 0.2, full_frame=False)
    rows = torch.zeros(tb.slots, 96, ld, device=dev)
    targets = [torch.zeros(hw, dtype=torch.uint8, device=dev) for hw in KERNEL_FRAMES]
    counts = torch.zeros(nc, nc, dtype=torch.int64, device=dev)
    good = dict(nc=nc, level_hw=level_hw, net_hw=net_hw, tile_batch=tb)
    for bad_rows in (rows[:-1], torch.cat([rows, rows[:1]]), rows.half(), rows.cpu()):      # slots count, dtype, device
        with pytest.raises(ValueError):
            R.stitch_segmentation(frames, bad_rows, **good)
    for bad in (dict(weight="gauss"), dict(nc=257), dict(net_hw=(31, 50)), dict(tile_batch=R.TileBatch(frames, net_hw, 0.2, full_frame=True)),
                dict(targets=targets), dict(targets=targets[:3], counts=counts), dict(targets=targets, counts=counts.int()),
                dict(targets=targets, counts=counts.cpu()), dict(targets=[t.long() for t in targets], counts=counts),
                dict(targets=targets[::-1], counts=counts), dict(draw=True, lut=torch.zeros(2, 3, dtype=torch.uint8, device=dev))):
        with pytest.raises(ValueError):
            R.stitch_segmentation(frames, rows, **{**good, **bad})
    with pytest.raises(ValueError):
        R.stitch_segmentation(frames[:3], rows, **good)                         # the tile batch was built for other frames
    with pytest.raises(CvxError):
        R.stitch_segmentation([f.cpu() for f in frames], rows, **good)
    labels = R.stitch_segmentation(frames, rows, targets=targets, counts=counts, **good)
    assert all(not l.any() for l in labels) and int(counts[0, 0]) == sum(h * w for h, w in KERNEL_FRAMES) and int(counts.sum()) == int(counts[0, 0])
