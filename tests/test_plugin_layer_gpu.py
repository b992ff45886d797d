"""MI355X: the grow-and-retry NMS call of the YOLOv7 and SSD wrappers -- 1024 rows per block first, four times the room while a block
comes back full, ``CvxError`` on the kernel's count of -1 -- on planted candidates that do not overlap, so every one of them is kept."""
import numpy as np
import pytest
import torch

import builder
from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd import engine as E

pytestmark = pytest.mark.gpu
N_MANY, N_FEW = 1100, 3           # kept rows of the two images: past the first block of 1024, and far below it


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class Calls(list):
    fail = False          # True: the next call's last count comes back as -1, the kernel's "more candidates than the sort holds"


@pytest.fixture
def nms_calls(monkeypatch):
    """The ``max_det`` of every ``engine.nms`` call the test makes, in order"""
    real, calls = E.nms, Calls()

    def nms(*args, **kw):
        calls.append(kw["max_det"])
        rows, index, counts = real(*args, **kw)
        if calls.fail:
            counts[-1] = -1
        return rows, index, counts

    monkeypatch.setattr(E, "nms", nms)
    return calls


def test_yolov7_nms_device_grows_the_row_block(dev, nms_calls):
    cfg, algo_cls, _ = builder.export_from_registry("yolo7")
    algo = algo_cls(cfg, dev)
    nc, A = algo.num_classes, 1200
    g = torch.Generator().manual_seed(11)
    ii = torch.arange(A)
    dec = torch.zeros(2, A, 5 + nc)
    dec[:, :, 0] = (ii % 40).float() / 40 + 0.01         # a 40 x 30 grid of disjoint boxes (centre x, centre y, w, h), normalised
    dec[:, :, 1] = (ii // 40).float() / 30 + 0.01
    dec[:, :, 2:4] = 0.006
    many, few = torch.randperm(A, generator=g)[:N_MANY], torch.randperm(A, generator=g)[:N_FEW]
    dec[0, many, 4] = 0.5 + 0.5 * torch.rand(N_MANY, generator=g)       # objectness; 0 elsewhere
    dec[1, few, 4] = 0.5 + 0.5 * torch.rand(N_FEW, generator=g)
    dec[:, :, 5 + 3] = 0.9                                                # one class
    dec = dec.to(dev)
    y = torch.cat((dec[:, :, :4], dec[:, :, 4:5] * dec[:, :, 5:]), 2).permute(0, 2, 1).contiguous()
    (det0, idx0), (det1, idx1) = algo.nms_device(y, dec, 0.3)
    assert nms_calls == [1024, 4096]
    assert det0.shape == (N_MANY, 7) and sorted(idx0.tolist()) == sorted(many.tolist())
    assert det1.shape == (N_FEW, 7) and sorted(idx1.tolist()) == sorted(few.tolist())
    assert bool((det0[:-1, 4] >= det0[1:, 4]).all()) and bool((det0[:, 6] == 3).all())
    nms_calls.fail = True
    with pytest.raises(CvxError, match="cvx_nms: more than 16384 candidates above the confidence threshold in image 1"):
        algo.nms_device(y, dec, 0.3)


def test_ssd_decode_device_grows_the_row_block(dev, nms_calls):
    from oracle import ssd_ref as SS
    cfg, algo_cls, _ = builder.export_from_registry("ssd")
    algo = algo_cls(cfg, dev)
    nc, A, column, side = algo.num_classes, algo.num_anchors, 7, 0.012
    # the first prior of every interior cell of the 38 x 38 map (its priors are not clipped), regressed to a square of `side` about the
    # prior's centre: the cells are 1 / 38 apart, so the squares are disjoint
    assert algo.feature_shapes[0] == 38
    per_cell = len(algo.aspect_ratios[0]) + 1
    cells = np.array([r * 38 + c for r in range(2, 36) for c in range(2, 36)])
    rs = np.random.RandomState(12)
    priors = cells[rs.permutation(len(cells))] * per_cell
    many, few = priors[:N_MANY], priors[N_MANY:N_MANY + N_FEW]
    var = algo.variance[::2].tolist()
    loc = torch.zeros(2, A, 4)
    wh = torch.from_numpy(algo.anchors[:, 2:4] - algo.anchors[:, 0:2])
    loc[:, :, 2:4] = torch.log(side / wh) / var[1]
    boxes = SS.parse_loc(loc[0], algo.anchors, var).numpy()[np.concatenate((many, few))]
    centres, sizes = (boxes[:, :2] + boxes[:, 2:]) / 2, boxes[:, 2:] - boxes[:, :2]
    gap = np.abs(centres[:, None] - centres[None]).max(-1) + np.eye(len(centres))
    assert np.abs(sizes - side).max() < 1e-6 and gap.min() > side              # the planted squares are what the comment says
    conf = torch.zeros(2, A, nc + 1)
    conf[:, :, 0] = 8.0                                                       # background everywhere ...
    for b, planted in enumerate((many, few)):
        conf[b, planted, 0] = 0.0
        conf[b, planted, column] = torch.from_numpy(6.0 + 2.0 * rs.rand(len(planted))).float()   # ... but at the planted priors: p > 0.95
    (det0, pairs0), (det1, pairs1) = algo.decode_device((loc.to(dev), conf.to(dev)), 0.5)
    assert nms_calls == [1024, 4096]
    assert det0.shape == (N_MANY, 6) and sorted(pairs0[:, 0].tolist()) == sorted(many.tolist()) and bool((pairs0[:, 1] == column).all())
    assert det1.shape == (N_FEW, 6) and sorted(pairs1[:, 0].tolist()) == sorted(few.tolist()) and bool((det1[:, 4] == column - 1).all())
    assert bool((det0[:-1, 5] >= det0[1:, 5]).all())
    nms_calls.fail = True
    with pytest.raises(CvxError, match="cvx_nms: more than 16384 candidates of one class above the confidence threshold in one image"):
        algo.decode_device((loc.to(dev), conf.to(dev)), 0.5)
