"""MI355X: seeded sweeps of the three hand-written kernel files every evaluator's numbers pass through -- ``cvx_nms_variant``,
``cvx_centernet_decode``, ``cvx_yolo7_decode`` -- on the cases of tests/eval_tail_cases.py against the project's oracles.
tests/test_eval_tail_cpu.py shows, from the oracles alone, what each case was built to catch.  No tolerance is new here: NMS is compared
bit for bit as in test_nms_bit_exact_against_the_oracle, the CenterNet decode as in test_centernet_decode_matches_the_reference_fixture
(indices, classes, survivors exact; scores within one ulp of torch.sigmoid; boxes rtol 1e-6 / atol 1e-5), the YOLOv7 decode as in
test_yolov7_forward_decode_nms_match_the_reference_fixture (rtol 2e-6 / atol 1e-7)."""
import numpy as np
import pytest
import torch

import eval_tail_cases as T
from computervision.pytorch_amd import engine as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("name", [c.name for c in T.nms_cases()])
def test_nms_sweep(dev, name):
    """All four batched_nms strategies on one case: counts, kept anchor indices and the 6-column rows bit for bit; counts = -1 (and nothing
    else) for an image with more candidates than the kernel sorts."""
    c = T.nms_case(name)
    y = torch.from_numpy(c.pred).to(dev)
    for variant in T.VARIANTS:
        rows, index, counts = (t.cpu().numpy() for t in E.nms(y, c.conf, c.iou, c.max_det, variant=variant, boxes_xyxy=c.xyxy))
        for b, ref in enumerate(T.nms_reference(c, variant)):
            if ref is None:
                assert counts[b] == -1, (variant, b, counts[b])
                continue
            k = int(counts[b])
            assert k == len(ref[1]), (variant, b, k, len(ref[1]))
            assert np.array_equal(index[b, :k].astype(np.int64), ref[1]), (variant, b)
            assert np.array_equal(bits(rows[b, :k]), bits(ref[0])), (variant, b)


@pytest.mark.parametrize("name", [c.name for c in T.centernet_cases()])
def test_centernet_decode_sweep(dev, name):
    """Top-K list (flat indices, classes), score mask and DIoU-NMS survivors exact, ties included; scores within one ulp of torch.sigmoid; boxes
    to fp32 round-off.  Where fewer than K peaks have a score the list is cut short (-1 / zeros); the reference's stable sort goes on into
    the zeros, so the prefix with a score is compared.  counts = -1 for the image whose ties overflow one slice's sort."""
    c = next(k for k in T.centernet_cases() if k.name == name)
    x = T.centernet_device_input(c)
    ld, reg_col, wh_col = c.cols
    assert x.shape[2] == ld
    out = {k: v.cpu() for k, v in E.centernet_decode(x.to(dev), c.H, c.W, c.nc, reg_col, wh_col, c.K, c.conf, c.nms_thr, c.use_nms).items()}
    for b, ref in enumerate(T.centernet_reference(c)):
        if ref is None:
            assert int(out["counts"][b]) == -1
            continue
        nz = int((ref["scores"] > 0).sum())
        assert torch.equal(out["topk_index"][b, :nz].long(), ref["index"][:nz]), b
        assert bool((out["topk_index"][b, nz:] == -1).all()) and bool((out["classes"][b, nz:] == 0).all())
        assert bool((out["scores"][b, nz:] == 0).all()) and bool((out["boxes"][b, nz:] == 0).all())
        assert torch.equal(out["classes"][b, :nz].long(), ref["classes"][:nz]), b
        ulp = np.abs(bits(out["scores"][b, :nz].numpy()).astype(np.int64) - bits(ref["scores"][:nz].numpy()).astype(np.int64))
        print(f"{name} image {b}: {nz} of {c.K} with a score, scores off by {int(ulp.max())} ulp at most, {float((ulp == 0).mean()):.2f} equal")
        assert ulp.max() <= 1, (b, int(ulp.max()))
        assert bool(torch.isfinite(out["boxes"][b]).all())
        np.testing.assert_allclose(out["boxes"][b, :nz].numpy(), ref["boxes"][:nz].numpy(), rtol=1e-6, atol=1e-5)
        n = int(out["counts"][b])
        assert n == len(ref["keep"]), (b, n, len(ref["keep"]))
        assert torch.equal(out["keep"][b, :n].long(), ref["keep"]), b


@pytest.mark.parametrize("slack", [0, 2])
@pytest.mark.parametrize("nc", T.Y7_NC)
def test_yolo7_decode_sweep(dev, nc, slack):
    """5 + nc attributes below, at and above one wave per anchor, ragged levels, three images (workgroups of 32 anchors straddle anchors,
    levels and images), optionally two NaN slack columns behind every row."""
    preds, rows, want = T.yolo7_case(nc, slack)
    dec, y = E.yolo7_decode(rows.to(dev), nc, T.Y7_LEVELS, T.Y7_ANCHORS, T.Y7_INPUT_HW)
    assert tuple(dec.shape) == tuple(want.shape) and bool(torch.isfinite(dec).all()) and bool(torch.isfinite(y).all())
    err = (dec.cpu() - want).abs()
    print(f"nc {nc} slack {slack}: max abs {float(err.max()):.3e}, max rel {float((err / want.abs().clamp_min(1e-30)).max()):.3e}")
    np.testing.assert_allclose(dec.cpu().numpy(), want.numpy(), rtol=2e-6, atol=1e-7)
    assert np.array_equal(bits(y[:, :4].cpu().numpy()), bits(dec[..., :4].transpose(1, 2).cpu().numpy()))
    prod = (dec[..., 4:5] * dec[..., 5:]).transpose(1, 2)            # one fp32 product of the kernel's own values
    assert np.array_equal(bits(y[:, 4:].cpu().numpy()), bits(prod.cpu().numpy()))
