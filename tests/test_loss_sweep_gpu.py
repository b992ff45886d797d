"""MI355X: seeded sweeps of the training-side loss and target kernels -- ``cvx_yolo7_loss``, ``cvx_centernet_loss``,
``cvx_centernet_draw_targets``, ``cvx_ssd_encode_targets`` -- on the cases of tests/loss_sweep_cases.py against the project's oracles in
float64.  tests/test_loss_sweep_cpu.py shows, from the oracles alone, what each case was built to catch and that the discrete decisions
of the SimOTA assignment keep clear of float32 round-off.  No bound is new here: loss items 2e-5 (YOLOv7) / 1e-5 (CenterNet), fp16
gradients 1e-3 relative L2 -- but per level and per column group, not over the whole tensor --, lists, flags, classes and index sets exact,
heat-map values rtol 2e-7, encoded boxes rtol 3e-7."""
import ctypes

import numpy as np
import pytest
import torch

import loss_sweep_cases as T
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import engine as E

pytestmark = pytest.mark.gpu

GRAD_BOUND = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def group_error(have, want):
    """relative L2 of one column group; a group that is identically zero in the oracle must be exactly zero"""
    if float(want.abs().max()) == 0.0:
        assert float(have.abs().max()) == 0.0
        return 0.0
    return T.rel(have, want)


def y7_device_lists(crit, c, n_targets):
    """the candidate lists per level and the matched lists per level (images in order) the kernels left in the workspace"""
    lib = L.load()
    A = sum(h * w for h, w in c.levels)
    out = (ctypes.c_int64 * 6)()
    L.check(lib.cvx_debug_yolo7_loss_layout(c.B, A, c.ld, n_targets, out), "cvx_debug_yolo7_loss_layout")
    cand_off, matched_off, mcount_off, state_off, cap, cmax = (int(v) for v in out)
    ws = crit._ws.cpu().numpy()
    state = ws[state_off:state_off + 28].view(np.int32)
    cand = ws[cand_off:cand_off + 3 * cap * 20].view(np.int32).reshape(3, cap, 5)
    matched = ws[matched_off:matched_off + 3 * c.B * cmax * 16].view(np.int32).reshape(3, c.B, cmax, 4)
    mcount = ws[mcount_off:mcount_off + c.B * 12].view(np.int32).reshape(c.B, 3)
    cands = [[tuple(int(v) for v in row) for row in cand[lv, :state[lv]]] for lv in range(3)]
    lists = [[(b,) + tuple(int(v) for v in row) for b in range(c.B) for row in matched[lv, b, :mcount[b, lv]]] for lv in range(3)]
    assert [int(v) for v in state[3:6]] == [len(m) for m in lists]
    return cands, lists, int(state[6])


@pytest.mark.parametrize("name", [c.name for c in T.Y7_CASES])
def test_yolo7_loss_sweep(dev, name):
    """Candidate lists and matched lists exact, order included (read back from the workspace through cvx_debug_yolo7_loss_layout); the four
    loss items rtol 2e-5; the gradient 1e-3 relative L2 separately per level and per column group (box 0:4, objectness 4, classes 5: of
    every anchor), a group that is zero in the oracle exactly zero, padding exactly zero; the objectness target of every cell, recovered
    from the objectness gradient g = k (sigmoid(x) - t), within 1e-3 |sigmoid(x) - t| (the gradient's bound carried over to t) plus
    2e-6 (float32 CIoU) plus one fp16 subnormal step of the scaled gradient.
    Measured on the MI355X over the nine cases: items 7.4e-8; box 3.1e-4, objectness 2.3e-4, classes 2.4e-4 (fp16 rounding of the scaled
    gradient: 2^-11 / sqrt(3) = 2.8e-4 for uniformly spread mantissas); recovered objectness targets 4.3e-4 absolute; 0.5 s for the crowd,
    0.35 s for the 64-ground-truth image, under 0.1 s for the others."""
    from computervision.pytorch_amd.yolov7 import Yolo7Loss
    ref = T.y7_reference(name)
    c = ref["case"]
    rows = T.y7_rows(ref["outs"], c.ld)
    crit = Yolo7Loss(None, c.nc, c.input_hw, label_smoothing=c.smoothing)
    items, dpred = crit.op(rows.to(dev), list(c.levels), ref["targets"], c.img_size, T.Y7_SCALE)
    assert crit.overflowed() == 0
    cands, lists, bad = y7_device_lists(crit, c, ref["targets"].shape[0])
    assert bad == 0
    for lv in range(3):
        assert cands[lv] == ref["cands"][lv], (lv, len(cands[lv]), len(ref["cands"][lv]))
        assert lists[lv] == ref["matched"][lv], (lv, len(lists[lv]), len(ref["matched"][lv]))
    got_items = items.cpu().double().numpy()
    print(f"{name}: items {got_items.tolist()}, relative error {np.abs(got_items / ref['items'].numpy() - 1).tolist()}")
    np.testing.assert_allclose(got_items, ref["items"].numpy(), rtol=2e-5, atol=1e-7)
    got = dpred.float().cpu().double() / T.Y7_SCALE
    groups = T.y7_groups(c)
    assert float(got[..., groups["pad"]].abs().max()) == 0.0 if groups["pad"] else True
    for lv, sl in enumerate(T.y7_level_slices(c)):
        errs = {g: group_error(got[:, sl][..., groups[g]], ref["grad"][:, sl][..., groups[g]]) for g in ("box", "obj", "cls")}
        h, w = c.levels[lv]
        k = crit.obj_ratio * T.Y.BALANCE[lv] / (c.B * 3 * h * w)
        x = rows[:, sl][..., groups["obj"]].double()
        t_rec = torch.sigmoid(x) - got[:, sl][..., groups["obj"]] / k
        t_ref = ref["tobj"][lv].permute(0, 2, 3, 1).reshape(c.B, h * w, 3)
        excess = (t_rec - t_ref).abs() - (GRAD_BOUND * (torch.sigmoid(x) - t_ref).abs() + 2e-6 + 2.0 ** -24 / (k * T.Y7_SCALE))
        print(f"{name} level {lv}: gradient error box {errs['box']:.3e} obj {errs['obj']:.3e} cls {errs['cls']:.3e}; objectness target max error "
              f"{float((t_rec - t_ref).abs().max()):.3e}, {int((t_ref > 0).sum())} cells with a target")
        assert all(v < GRAD_BOUND for v in errs.values()), (lv, errs)
        assert float(excess.max()) <= 0.0, (lv, float(excess.max()))


@pytest.mark.parametrize("name", [c.name for c in T.CN_CASES])
def test_centernet_loss_sweep(dev, name):
    """The four loss items 1e-5; the gradient 1e-3 relative L2 separately for the heat columns, the two "reg" columns and the two "wh"
    columns; padding exactly zero.
    Measured on the MI355X over the five cases: items 5.2e-7; heat 2.2e-4, "reg" pair 2.5e-4, "wh" pair 2.5e-4; 0.05 s at most."""
    from computervision.pytorch_amd.dla import CenterNetLoss
    c = T.cn_case(name)
    pred, targets = T.cn_inputs(name)
    want_items, want = T.cn_reference(name)
    items, dpred = CenterNetLoss(c.nc).op(T.cn_rows(c, pred).to(dev), targets, (c.h, c.w), T.CN_SCALE)
    got_items = items.cpu().double()
    err = ((got_items - want_items).abs() / want_items.abs()).tolist()
    got = dpred.float().cpu().double() / T.CN_SCALE
    groups = T.cn_groups(c)
    errs = {g: group_error(got[..., groups[g]], want[..., groups[g]]) for g in ("heat", "a", "b")}
    print(f"{name}: item errors {err}; gradient error heat {errs['heat']:.3e} a {errs['a']:.3e} b {errs['b']:.3e}")
    assert all(e < 1e-5 for e in err), err
    assert all(v < GRAD_BOUND for v in errs.values()), errs
    assert float(got[..., groups["pad"]].abs().max()) == 0.0


@pytest.mark.parametrize("name", [c.name for c in T.DRAW_CASES])
def test_centernet_draw_sweep(dev, name):
    """reg / wh / mask / indices exact, the heat map's == 1 and == 0 sets exact, its values rtol 2e-7; the reversed table draws the same
    heat map bit for bit.  Measured on the MI355X: every heat-map value equal to the oracle's (relative error 0)."""
    c = T.draw_case(name)
    lab, counts = T.draw_inputs(name)
    heat, reg, wh, mask, ind = (t.cpu().numpy() for t in E.centernet_draw_targets(lab.to(dev), counts.to(dev), (c.H, c.W), c.nc))
    worst = 0.0
    for b, (rh, rreg, rwh, rmask, rind) in enumerate(T.draw_reference(name)):
        assert np.array_equal(reg[b], rreg) and np.array_equal(wh[b], rwh) and np.array_equal(mask[b], rmask) and np.array_equal(ind[b], rind), b
        assert np.array_equal(heat[b] == 1.0, rh == 1.0) and np.array_equal(heat[b] == 0.0, rh == 0.0), b
        nz = rh > 0
        worst = max(worst, float((np.abs(heat[b][nz] - rh[nz]) / rh[nz]).max()) if nz.any() else 0.0)
        np.testing.assert_allclose(heat[b], rh, rtol=2e-7, atol=0)
    print(f"{name}: heat map max relative error {worst:.3e}")
    assert np.array_equal(heat[0].view(np.int32), heat[4].view(np.int32))


@pytest.mark.parametrize("which", T.SSD_PRIOR_SETS)
def test_ssd_encode_sweep(dev, which):
    """classes, background column and positive flag exact; encoded boxes rtol 3e-7 (atol 1e-7, as in the fixture test).  Measured on the
    MI355X: every encoded box equal to the oracle's (relative error 0)."""
    pri = T.ssd_priors(which)
    lab, counts, _ = T.ssd_inputs(which)
    ref = T.ssd_reference(which)
    y = E.ssd_encode_targets(torch.from_numpy(lab).to(dev), torch.from_numpy(counts).to(dev), torch.from_numpy(pri).to(dev), T.SSD_NC, T.SSD_THR).cpu().numpy()
    assert y.shape == ref.shape == (len(counts), len(pri), 4 + T.SSD_NC + 2)
    assert np.array_equal(y[..., 4:], ref[..., 4:])
    nz = ref[..., :4] != 0
    print(f"{which}: encoded boxes max relative error {float((np.abs(y[..., :4][nz] - ref[..., :4][nz]) / np.abs(ref[..., :4][nz])).max()):.3e}")
    np.testing.assert_allclose(y[..., :4], ref[..., :4], rtol=3e-7, atol=1e-7)
