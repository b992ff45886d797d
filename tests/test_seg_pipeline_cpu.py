"""CPU: the host side of the segmentation input pipeline -- ``draw_seg_params`` against a literal restatement of torchvision's
``RandomCrop.get_params`` and the flip draw, the resized-size rule, the restatement (tests/seg_pipeline_restatement.py) against torch on the
CPU, the new symbols, and the trainer / algorithm surface that needs no GPU."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import seg_pipeline_restatement as S
from computervision.pytorch_amd import LIB_PATH, CvxError, seg_pipeline
from computervision.pytorch_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((37, 53), 33, (33, 33)), ((40, 29), 33, (33, 33)), ((33, 33), 33, (33, 33)), ((21, 64), 33, (33, 33)), ((5, 7), 33, (33, 33)),
          ((48, 120), 48, (32, 48))]
LABEL_SEED = 60                             # blocky_labels: at most 2 % of the resized labels within 1e-3 of a half-integer at every shape


def test_draw_seg_params_reproduces_the_literal_draws():
    """200 items of mixed sizes, one pair of generators each side: the same (i, j, flip) item after item, so the draws are consumed in
    the reference's order; an item whose resized picture has the crop size consumes no torch draw; validation consumes nothing."""
    rs = np.random.RandomState(0)
    sizes = [SHAPES[k][0] for k in rs.randint(0, 5, 200)]
    assert (33, 33) in sizes
    gen_a, gen_b = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    py_a, py_b = random.Random(5), random.Random(5)
    flips = 0
    for size in sizes:
        got = seg_pipeline.draw_seg_params(gen_a, py_a, size, 33, (33, 33))
        want = S.draw(gen_b, py_b, size, 33, (33, 33))
        assert got == want, (size, got, want)
        assert 0 <= got["i"] <= got["rh"] - 33 and 0 <= got["j"] <= got["rw"] - 33
        flips += got["flip"]
    assert 60 < flips < 140
    assert torch.equal(gen_a.get_state(), gen_b.get_state()) and py_a.getstate() == py_b.getstate()
    before, py_before = gen_a.get_state().clone(), py_a.getstate()
    p = seg_pipeline.draw_seg_params(gen_a, py_a, (33, 33), 33, (33, 33))
    assert (p["i"], p["j"]) == (0, 0) and torch.equal(gen_a.get_state(), before) and py_a.getstate() != py_before   # the flip alone was drawn
    before, py_before = gen_a.get_state().clone(), py_a.getstate()
    p = seg_pipeline.draw_seg_params(gen_a, py_a, (37, 53), 33, (33, 33), train=False)
    assert p == dict(ih=37, iw=53, rh=33, rw=33, i=0, j=0, flip=0)
    assert torch.equal(gen_a.get_state(), before) and py_a.getstate() == py_before
    with pytest.raises(CvxError):                                            # Resize(33) of 40 x 29 is 45 x 33: no room for a 40-wide crop
        seg_pipeline.draw_seg_params(gen_a, py_a, (40, 29), 33, (33, 40))


@pytest.mark.parametrize("size,base,want", [((37, 53), 33, (33, 47)), ((40, 29), 33, (45, 33)), ((21, 64), 33, (33, 100)),
                                            ((375, 500), 513, (513, 684))])
def test_resized_size_rule(size, base, want):
    assert seg_pipeline.resized_size(*size, base) == want == S.resized_size(*size, base)


@pytest.mark.parametrize("size,base,crop", SHAPES)
def test_restatement_against_torch(size, base, crop):
    """the fp64 restatement of the image path against F.interpolate (fp32): their distance d is what the GPU test scales its bound from,
    so it has to be rounding noise and nothing else; the restated label path against torch.round(F.interpolate(labels.float())) exactly,
    outside the pixels within 1e-3 of a half-integer (at most 2 % of them)"""
    H, W = crop
    rh, rw = S.resized_size(*size, base)
    picture = S.synth_picture(size[0], size[1], seed=size[0])
    labels = S.blocky_labels(size[0], size[1], seed=LABEL_SEED)
    for job in (dict(ih=size[0], iw=size[1], rh=rh, rw=rw, i=rh - H, j=rw - W, flip=1), dict(ih=size[0], iw=size[1], rh=H, rw=W, i=0, j=0, flip=0)):
        want = S.image_torch(picture, job, H, W).double().numpy()
        d = np.abs(S.image64(picture, job, H, W) - want).max()
        print(f"{size} -> {job['rh']} x {job['rw']}: F.interpolate fp32 against the fp64 restatement, normalised: {d:.3e}")
        assert d < 4e-6, d                  # ten-odd fp32 roundings of values below 2.7 (ulp 2.4e-7); a wrong tap or weight is off by 1e-2 and more
        if (job["rh"], job["rw"]) == (32, 48) and size == (48, 120):
            # scales 1.5 and 2.5: every lambda is 0.25 or 0.75 and the labels are at most 20, so the job is exact in fp32 and in fp64; it
            # is compared on ALL pixels, and its exact .5 ties (several per cent) are where the half-to-even rule shows
            values = S.labels64(labels, job, H, W)
            ties = values - np.floor(values) == 0.5
            down = ties & (np.floor(values) % 2 == 0)                        # half-to-even rounds these down, half-away-from-zero up
            assert ties.sum() >= 0.03 * ties.size and down.sum() >= 16 and (ties & ~down).sum() >= 16
            assert np.array_equal(np.rint(values), S.labels_torch(labels, job, H, W).numpy())
            continue
        whole = dict(job, i=0, j=0, flip=0)                                  # the share is taken over the whole resized label picture
        share = S.near_half(S.labels64(labels, whole, job["rh"], job["rw"])).mean()
        assert share <= 0.02, share
        values = S.labels64(labels, job, H, W)
        safe = ~S.near_half(values)
        assert np.array_equal(np.rint(values)[safe], S.labels_torch(labels, job, H, W).numpy()[safe])
    same = dict(ih=size[0], iw=size[1], rh=size[0], rw=size[1], i=0, j=0, flip=0)
    assert np.array_equal(S.labels_torch(labels, same, *size).numpy(), labels)          # the identity resize keeps the labels


def test_colour_table_lookup_of_the_restatement():
    from core.algorithms.segmentation_2d import voc_colormap
    cm = voc_colormap()
    labels = S.blocky_labels(21, 30, seed=3)
    mask = S.colour_mask(labels, cm, unknown=[(0, 0), (20, 29)])
    want = labels.copy()
    want[0, 0] = want[20, 29] = 0
    assert np.array_equal(S.label_indices(mask, cm), want)


def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH)
    for name in ("cvx_seg_pipeline", "cvx_seg_criterion_eval", "cvx_seg_criterion_workspace_bytes"):
        assert name in declared and name in L.PROTOTYPES and hasattr(lib, name)
    assert len(L.PROTOTYPES["cvx_seg_pipeline"][1]) == 12 and len(L.PROTOTYPES["cvx_seg_criterion_eval"][1]) == 9
    assert len(L.PROTOTYPES["cvx_seg_criterion_workspace_bytes"][1]) == 3
    sizes = {k: int(v) for k, v in re.findall(r"#define CVX_SEG_(DIMS|CRITERION)_BYTES (\d+)", header)}      # the library's static_assert holds these
    assert ctypes.sizeof(L.SegDims) == sizes["DIMS"] == 28 and ctypes.sizeof(L.SegCriterion) == sizes["CRITERION"] == 128
    assert "cvx_seg_job" in header and seg_pipeline.SEG_JOB_DTYPE.itemsize == 64
    assert seg_pipeline.SEG_JOB_DTYPE.fields["ih"][1] == 16 and seg_pipeline.SEG_JOB_DTYPE.fields["reserved"][1] == 48


def test_augmenter_and_loader_arguments():
    aug = seg_pipeline.DeviceSegAugmenter((33, 33), 33, seed=0)
    with pytest.raises(CvxError):                                            # no CPU path
        aug([torch.zeros(40, 40, 3, dtype=torch.uint8)], [torch.zeros(40, 40, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        seg_pipeline.DeviceSegAugmenter((33, 33), 33, label_resize="cubic")
    source = [(torch.zeros(40, 40, 3, dtype=torch.uint8), torch.zeros(40, 40, dtype=torch.uint8))] * 7
    val_aug = seg_pipeline.DeviceSegAugmenter((33, 33), 33, train=False)
    assert len(seg_pipeline.DeviceSegLoader(source, 3, val_aug, device="cpu")) == 3                   # the reference's drop_last=False
    assert len(seg_pipeline.DeviceSegLoader(source, 3, val_aug, device="cpu", drop_last=True)) == 2
    assert len(seg_pipeline.DeviceSegLoader(source, 3, aug, length=5, device="cpu")) == 5
    with pytest.raises(ValueError):
        seg_pipeline.DeviceSegLoader(source, 3, aug, device="cpu")           # a training loader needs its length


def test_trainer_keyword_and_evaluate_on_voc_without_a_gpu(tmp_path):
    import builder
    cfg, algo_cls, trainer_cls = builder.export_from_registry("deeplabv3plus")
    source = [(torch.zeros(40, 40, 3, dtype=torch.uint8), torch.zeros(40, 40, dtype=torch.uint8))] * 2
    cpu_loader = seg_pipeline.DeviceSegLoader(source, 2, seg_pipeline.DeviceSegAugmenter((33, 33), 33, train=False), device="cpu")
    with pytest.raises(CvxError, match="val_dataloader"):
        trainer_cls(cfg, torch.device("cpu"), val_dataloader=cpu_loader)
    algo = algo_cls(cfg, torch.device("cpu"))
    with pytest.raises(ValueError):
        algo.evaluate_on_voc(None, str(tmp_path), subset="test")
    with pytest.raises(CvxError, match="dataloader"):
        algo.evaluate_on_voc(None, str(tmp_path))
    assert not os.listdir(tmp_path)
    from core.trainer.segmentation_trainer import SegmentationMetrics
    m = SegmentationMetrics(3)
    m.add_batch(torch.tensor([0, 1, 2, 2]), torch.tensor([0, 1, 1, -100]))                           # add_batch as before
    assert m.confusion_matrix.dtype == torch.float64 and m.confusion_matrix.tolist() == [[1, 0, 0], [0, 1, 1], [0, 0, 0]]
    assert m.get_results()["Overall Acc"] == pytest.approx(2 / 3)
    with pytest.raises(CvxError):
        m.add_rows(torch.zeros(1, 4, 8), torch.zeros(1, 4, 4, dtype=torch.long), (2, 2), None, torch.zeros(1))
    m.reset()
    assert float(m.confusion_matrix.sum()) == 0.0
