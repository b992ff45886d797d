"""Weight averaging without a GPU: the recurrence the kernels are specified by, the model clone, the checkpoint format.

``ema_ref.npz`` holds the REAL reference ``ModelEMA`` run for 40 updates (tools/make_ema_golden.py); the kernels' formula

    e_new = rn( rn(e * float(d)) + rn(float(1 - d) * p) ),   d = decay * (1 - exp(-updates / tau)) formed in double

must reproduce it with 0 differing bits -- both sides are three correctly rounded fp32 operations in the same order.
"""
import copy
import math

import numpy as np
import pytest
import torch

from computervision.pytorch_amd import CvxError
from computervision.pytorch_amd.ema import ModelEMA, clone_model
from core.utils.ckpt import CheckPoint

LEGS = ("cold", "warm")


def host_replay(e, sources, updates0, decay, tau):
    """The recurrence in numpy fp32, one row of `sources` per update; returns every intermediate state."""
    e = np.asarray(e, dtype=np.float32).copy()
    out, u = [], int(updates0)
    for p in sources:
        u += 1
        d = float(decay) * (1 - math.exp(-u / float(tau)))
        e = (e * np.float32(d)).astype(np.float32) + (np.float32(1 - d) * np.asarray(p, dtype=np.float32)).astype(np.float32)
        out.append(e.copy())
    return np.stack(out)


@pytest.mark.parametrize("leg", LEGS)
def test_recurrence_reproduces_the_reference_bit_for_bit(gold, leg):
    g = gold("ema_ref.npz")
    n = g[f"{leg}_init"].shape[0]
    assert n % 4 != 0 and g[f"{leg}_src"].shape == (40, n)
    got = host_replay(g[f"{leg}_init"], g[f"{leg}_src"], g[f"{leg}_updates0"], g["decay"], g["tau"])
    differing = int((got.view(np.uint32) != g[f"{leg}_ema"].view(np.uint32)).sum())
    assert differing == 0
    assert not np.array_equal(g[f"{leg}_ema"][-1], g[f"{leg}_init"])                     # the average did move
    assert int(g[f"{leg}_nbt_final"]) == int(g[f"{leg}_nbt_init"])                       # not floating-point: left where it was cloned
    d_last = float(g["decay"]) * (1 - math.exp(-(int(g[f"{leg}_updates0"]) + 40) / float(g["tau"])))
    assert (d_last < 0.05) if leg == "cold" else (abs(d_last - float(g["decay"])) < 1e-9)


def _families():
    from computervision.pytorch_amd.deeplab import DeepLabV3PlusR101
    from computervision.pytorch_amd.dla import CenterNetDLA34
    from computervision.pytorch_amd.model import Yolo8
    from computervision.pytorch_amd.ssd import SSD300VGG
    from computervision.pytorch_amd.yolov7 import Yolo7L
    return {"yolo8": lambda: Yolo8("n", 20), "deeplab": lambda: DeepLabV3PlusR101(21, dropout_p=0.25), "centernet": lambda: CenterNetDLA34(20),
            "ssd": lambda: SSD300VGG(20), "yolo7": lambda: Yolo7L(20)}


def _inside(t, arena):
    lo = arena.data_ptr()
    return t.untyped_storage().data_ptr() == arena.untyped_storage().data_ptr() and lo <= t.data_ptr() < lo + max(arena.numel(), 1) * arena.element_size()


@pytest.mark.parametrize("family", ["yolo8", "deeplab", "centernet", "ssd", "yolo7"])
@pytest.mark.parametrize("how", ["clone_model", "deepcopy"])
def test_clone_owns_its_arenas(family, how):
    torch.manual_seed(3)
    m = _families()[family]()
    with torch.no_grad():
        m.flat_stats.add_(0.25)
        m._flat["nbt"].add_(5)
    rng = torch.get_rng_state()
    c = clone_model(m) if how == "clone_model" else copy.deepcopy(m)
    assert torch.equal(torch.get_rng_state(), rng)                                       # cloning draws nothing from the caller's stream
    assert type(c) is type(m) and c is not m and c.training == m.training
    assert c._flat["grad"] is None and not c._engines
    for k in ("param", "stat", "nbt"):
        assert torch.equal(c._flat[k], m._flat[k]), k
        assert c._flat[k].data_ptr() != m._flat[k].data_ptr(), k
    arena_of = {torch.float32: ("param", "stat"), torch.int64: ("nbt",)}
    msd, csd = m.state_dict(), c.state_dict()
    assert list(msd) == list(csd)
    outside = 0
    for k, v in csd.items():
        assert torch.equal(v, msd[k]), k
        if any(_inside(msd[k], m._flat[a]) for a in arena_of[msd[k].dtype]):
            assert any(_inside(v, c._flat[a]) for a in arena_of[v.dtype]), f"{k} of the clone is not a view of the clone's arenas"
        else:
            outside += 1
            assert v.data_ptr() != msd[k].data_ptr()
    assert outside <= 1                                                                  # YOLOv8's constant DFL weight
    for (n1, p1), (n2, p2) in zip(m.named_parameters(), c.named_parameters()):
        assert n1 == n2 and p1.requires_grad == p2.requires_grad
    if family == "deeplab":
        assert c.dropout_p == 0.25
    with torch.no_grad():                                                                # a write through a parameter lands in the clone's arena only
        before = m.flat_params.clone()
        next(c.parameters()).add_(1.0)
        assert torch.equal(m.flat_params, before) and not torch.equal(c.flat_params, before)


def test_clone_refuses_foreign_modules():
    with pytest.raises(CvxError):
        clone_model(torch.nn.Linear(2, 2))


def test_model_ema_surface_and_cpu_refusal():
    from computervision.pytorch_amd.model import Yolo8
    torch.manual_seed(0)
    m = Yolo8("n", 20).train()
    ema = ModelEMA(m, decay=0.99, tau=100, updates=4)
    assert not ema.ema.training and m.training and ema.updates == 4
    assert all(not p.requires_grad for p in ema.ema.parameters())
    assert ema.decay(10) == 0.99 * (1 - math.exp(-10 / 100))
    d, omd = ema.factors()
    assert d == ema.decay(4) and omd == 1 - d
    with pytest.raises(CvxError):
        ema.update(m)                                                                    # no CPU fallback
    assert ema.updates == 4
    m.names = ["a", "b"]
    ema.update_attr(m, include=("names",))
    assert ema.ema.names == ["a", "b"] and not ema.ema.training
    ema.update_attr(m)
    assert not ema.ema.training


def test_flat_adam_attach_checks_the_arenas():
    from computervision.pytorch_amd.model import Yolo8
    from computervision.pytorch_amd.train import FlatAdam
    m, other = Yolo8("n", 20), Yolo8("n", 80)
    opt = FlatAdam(m)
    with pytest.raises(CvxError):
        opt.attach_ema(ModelEMA(other))
    with pytest.raises(CvxError):
        opt.attach_ema(ModelEMA(m))                                                      # CPU arenas
    opt.attach_ema(None)


def test_checkpoint_round_trip_with_and_without_the_average(tmp_path):
    from computervision.pytorch_amd.model import Yolo8
    from computervision.pytorch_amd.train import FlatAdam
    torch.manual_seed(1)
    m = Yolo8("n", 20)
    ema = ModelEMA(m, updates=17)
    with torch.no_grad():                                                                # the average differs from the model
        ema.ema.flat_params.mul_(0.5)
        ema.ema.flat_stats.add_(1.0)
    sd = ema.state_dict()
    assert set(sd) == {"model", "updates"} and sd["updates"] == 17 and list(sd["model"]) == list(m.state_dict())
    opt = FlatAdam(m)
    with_ema, without = str(tmp_path / "a.pth"), str(tmp_path / "b.pth")
    CheckPoint.save(m, with_ema, optimizer=opt, ema=ema)
    CheckPoint.save(m, without, optimizer=opt)
    raw = torch.load(with_ema, map_location="cpu", weights_only=False)
    assert set(raw) == {"model", "optimizer", "ema"} and raw["ema"]["updates"] == 17
    assert "ema" not in torch.load(without, map_location="cpu", weights_only=False)
    # with the entry: the average comes back exactly
    m2 = Yolo8("n", 20)
    ema2 = ModelEMA(m2)
    CheckPoint.load(with_ema, "cpu", m2, optimizer=FlatAdam(m2), ema=ema2)
    assert ema2.updates == 17
    for k in ("param", "stat", "nbt"):
        assert torch.equal(ema2.ema._flat[k], ema.ema._flat[k]) and torch.equal(m2._flat[k], m._flat[k])
    assert not torch.equal(ema2.ema.flat_params, m2.flat_params)
    # without it: loads as before, and the average restarts from the loaded weights
    m3 = Yolo8("n", 20)
    ema3 = ModelEMA(m3, updates=5)
    CheckPoint.load(without, "cpu", m3, optimizer=FlatAdam(m3), ema=ema3)
    assert ema3.updates == 5
    for k in ("param", "stat", "nbt"):
        assert torch.equal(ema3.ema._flat[k], m._flat[k])
    # a file with the entry still loads where nobody asks for it, and as a bare model
    m4 = Yolo8("n", 20)
    CheckPoint.load(with_ema, "cpu", m4)
    CheckPoint.load_pure(with_ema, "cpu", m4)
    assert torch.equal(m4.flat_params, m.flat_params)
    bare = str(tmp_path / "c.pth")
    CheckPoint.save(ema.ema, bare)
    m5 = Yolo8("n", 20)
    CheckPoint.load_pure(bare, "cpu", m5)
    assert torch.equal(m5.flat_params, ema.ema.flat_params) and torch.equal(m5.flat_stats, ema.ema.flat_stats)
