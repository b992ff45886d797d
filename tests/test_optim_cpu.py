"""CPU: what FlatSGD / FlatAdamW add, without a device -- the restatement (tests/optim_restatement.py) against torch.optim and
torch.nn.utils on the CPU, the group map on the real layouts of all five models, the checkpoint layout against the stock torch optimisers,
and ``get_optimizer``.  tests/test_optim_gpu.py compares the kernels with the same restatement bit for bit."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import optim_restatement as R
from computervision.pytorch_amd import LIB_PATH, CvxError
from computervision.pytorch_amd import _lib as L
from computervision.pytorch_amd import engine as E
from computervision.pytorch_amd import optim as O
from core.utils.ckpt import CheckPoint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- 1. the restatement against torch.optim on the CPU -----------------------------------------------------------------------------------
SGD_CASES = {"plain": dict(lr=0.01), "momentum": dict(lr=0.01, momentum=0.9), "nesterov": dict(lr=0.01, momentum=0.937, nesterov=True),
             "decay": dict(lr=0.02, momentum=0.9, nesterov=True, weight_decay=5e-4)}


@pytest.mark.parametrize("case", list(SGD_CASES))
def test_sgd_restatement_against_torch_sgd(case):
    """5 steps, gradients scaled 10^(i-2).  torch's CPU kernels may fuse a multiply into an add, so the comparison is a tolerance, and a
    measured one: E = max |torch fp32 - torch fp64| per step, and the restatement must stay within 4 E of the same fp64 recurrence (both
    fp32 sides commit a handful of roundings per element and step and differ only in which of them are fused)."""
    kw = SGD_CASES[case]
    gen = torch.Generator().manual_seed(7)
    n = 4096
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (10.0 ** (i - 2)) for i in range(5)]
    t32, t64 = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.double())
    o32, o64 = torch.optim.SGD([t32], **kw), torch.optim.SGD([t64], **kw)
    p, b = p0.numpy().copy(), np.zeros(n, F)
    for i, g in enumerate(grads):
        t32.grad, t64.grad = g.clone(), g.double()
        o32.step()
        o64.step()
        p, b = R.sgd_step(p, b, g.numpy(), kw["lr"], kw.get("weight_decay", 0.0), kw.get("momentum", 0.0), kw.get("nesterov", False))
        ref = t64.detach().numpy()
        e_torch = float(np.abs(t32.detach().numpy().astype(np.float64) - ref).max())
        e_mine = float(np.abs(p.astype(np.float64) - ref).max())
        print(f"sgd {case} step {i}: E = {e_torch:.3e}, restatement {e_mine:.3e}, ratio {e_mine / e_torch:.2f}")
        assert e_torch > 0 and e_mine <= 4 * e_torch
        if kw.get("momentum"):
            eb = float(np.abs(o32.state[t32]["momentum_buffer"].numpy().astype(np.float64) - o64.state[t64]["momentum_buffer"].numpy()).max())
            mb = float(np.abs(b.astype(np.float64) - o64.state[t64]["momentum_buffer"].numpy()).max())
            assert mb <= 4 * eb


@pytest.mark.parametrize("lr,wd", [(1e-3, 1e-2), (3e-4, 5e-2), (0.1, 0.3), (1e-3, 0.0)])
def test_adamw_decay_is_torchs_multiply_bit_for_bit(lr, wd):
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(4099, generator=gen) * 10.0 ** torch.randint(-3, 4, (4099,), generator=gen).float()
    want = p.clone().mul_(1 - lr * wd)                                      # torch.optim.AdamW: param.mul_(1 - lr * weight_decay)
    assert np.array_equal(R.adamw_decay(p.numpy(), lr, wd).view(np.uint32), want.numpy().view(np.uint32))
    assert F(O.decay_factor(lr, wd)) == R.decay_factor(lr, wd) and (wd != 0.0 or O.decay_factor(lr, wd) == 1.0)
    # one AdamW step of torch = the multiply, then Adam: with a zero gradient the Adam part leaves p alone
    t = torch.nn.Parameter(p.clone())
    t.grad = torch.zeros_like(t)
    torch.optim.AdamW([t], lr=lr, weight_decay=wd).step()
    assert torch.equal(t.detach(), want)


def test_clip_coef_against_torch_clip_grad_norm():
    """max_norm is chosen from the fp64 norm so that some steps clip and some do not.  Fed the fp32 norm torch itself measured, the
    restated coefficient scales the gradients to torch's bits; fed the fp64 norm it agrees to 1e-5, the bound the device norm has."""
    gen = torch.Generator().manual_seed(11)
    shapes = [(16, 3, 3, 3), (16,), (21,), (255,), (64, 16, 1, 1)]
    seen = set()
    for i in range(6):
        grads = [torch.randn(s, generator=gen) * (10.0 ** (i % 3 - 1)) for s in shapes]
        norm64 = float(np.sqrt(sum((g.double() ** 2).sum().item() for g in grads)))
        max_norm = norm64 * (0.5 if i % 2 == 0 else 2.0)
        params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(params, max_norm)
        coef = R.clip_coef(total.item(), max_norm)
        seen.add(bool(coef < 1))
        assert (coef < 1) == (i % 2 == 0)
        for p, g in zip(params, grads):
            assert np.array_equal(R.scaled_grad(g.numpy(), 1.0, coef).view(np.uint32), p.grad.numpy().view(np.uint32))
        assert abs(float(R.clip_coef(norm64, max_norm)) - float(coef)) <= 1e-5 * float(coef)
    assert seen == {True, False}


# ---- 2. the group map on the real layouts ------------------------------------------------------------------------------------------------
def _models():
    from computervision.pytorch_amd.deeplab import DeepLabV3PlusR101
    from computervision.pytorch_amd.dla import CenterNetDLA34
    from computervision.pytorch_amd.model import Yolo8
    from computervision.pytorch_amd.ssd import SSD300VGG
    from computervision.pytorch_amd.yolov7 import Yolo7L
    return {"yolov8": lambda: Yolo8("n", 20), "yolov7": lambda: Yolo7L(20), "ssd": lambda: SSD300VGG(20), "centernet": lambda: CenterNetDLA34(20),
            "deeplab": lambda: DeepLabV3PlusR101(21)}


def _spec(spec, name, default=None):
    return spec.get(name, default) if isinstance(spec, dict) else getattr(spec, name, default)


def _by_name(named):
    """the classification the issue states, from names and ndim alone"""
    out = {}
    for k, p in named:
        out[k] = 3 if not p.requires_grad else 0 if p.dim() > 1 else 2 if k.endswith(".bias") else 1
    return out


@pytest.mark.parametrize("family", ["yolov8", "yolov7", "ssd", "centernet", "deeplab"])
def test_group_map_on_the_real_layout(family):
    torch.manual_seed(0)
    m = _models()[family]()
    lay = m.layout
    named = list(m.named_parameters())
    first = named[0][0]
    prefix = first[:first.index(".", first.index(".") + 1) + 1] if first.count(".") > 1 else first.rsplit(".", 1)[0] + "."
    with pytest.raises(ValueError):
        O.GroupPlan(m, O.NO_DECAY_NORM_BIAS, freeze=("no.such.module.",))
    assert all(p.requires_grad == (not k.endswith("dfl.conv.weight")) for k, p in named)          # the refused call froze nothing
    before = {k: p.requires_grad for k, p in named}
    plan = O.GroupPlan(m, O.NO_DECAY_NORM_BIAS, freeze=(prefix,))
    moved = [k for k, p in named if before[k] and not p.requires_grad]
    assert moved and moved == [k for k, _ in named if k.startswith(prefix) and before[k]]
    want = _by_name(named)
    assert plan.names == ["weights", "norm", "bias", "frozen"] and plan.frozen == 3
    for g in range(4):
        assert plan.keys[g] == [k for k, _ in named if want[k] == g], g
    assert all(plan.keys[g] for g in range(4))
    # every trainable slot once, by the restated builder from offsets and logical lengths
    slots = lay.slots
    segments = [(slots[k].offset, p.numel(), want[k]) for k, p in named if k in slots]
    assert {k for k, sl in slots.items() if sl.arena == "param" and sl.trainable} == {k for k, _ in named if k in slots}
    ref = R.build_group_map(lay.n_params, segments)
    assert plan.gmap.dtype == np.uint8 and np.array_equal(plan.gmap, ref)
    for g in range(4):
        assert int((plan.gmap == g).sum()) == sum((p.numel() + 3) // 4 for k, p in named if k in slots and want[k] == g)
    # the rows that pad a convolution to the engine's channel count are nobody's
    padded = 0
    for spec in lay.convs.values():
        if _spec(spec, "k") is None:                                       # CenterNet's depthwise up-convolutions: no channel padding
            continue
        couts = _spec(spec, "couts")
        cout = sum(couts) if couts is not None else _spec(spec, "cout")
        ce, kkc = _spec(spec, "cout_eng"), _spec(spec, "k") ** 2 * _spec(spec, "cin")
        if ce > cout:
            w_off = _spec(spec, "w_off")
            lo, hi = (w_off + cout * kkc + 3) // 4, (w_off + ce * kkc) // 4
            assert hi > lo and (plan.gmap[lo:hi] == R.UNMAPPED).all()
            padded += hi - lo
    assert padded > 0 and int((plan.gmap == R.UNMAPPED).sum()) >= padded
    # without grouping: one live group (and the frozen one)
    plain = O.GroupPlan(m, None)
    assert plain.names == ["all", "frozen"] and np.array_equal(plain.gmap == 1, plan.gmap == 3) and np.array_equal(plain.gmap == 255, plan.gmap == 255)


def test_group_map_refuses_what_it_cannot_map():
    slot = lambda off, shape, strides=None: SimpleNamespace(arena="param", offset=off, shape=shape, strides=strides or (1,), trainable=True)
    lay = lambda slots, n=16: SimpleNamespace(slots=slots, n_params=n)
    ok = lay({"a.weight": slot(0, (5,)), "a.bias": slot(8, (3,))})
    assert O.build_group_map(ok, {"a.weight": 0, "a.bias": 1}, 2).tolist() == [0, 0, 1, 255]
    for bad_layout, groups, n_groups in (
            (lay({"a.weight": slot(0, (5,)), "a.bias": slot(6, (3,))}), {"a.weight": 0, "a.bias": 1}, 2),          # offset not a multiple of 4
            (lay({"a.weight": slot(0, (5,)), "a.bias": slot(4, (3,))}), {"a.weight": 0, "a.bias": 1}, 2),          # a chunk claimed twice
            (ok, {"a.weight": 0}, 2),                                                                                # a slot left out
            (ok, {"a.weight": 0, "a.bias": 2}, 2),                                                                   # id >= n_groups
            (ok, {"a.weight": 0, "a.bias": 1}, 17),                                                                  # more than 16 groups
            (ok, {"a.weight": 0, "a.bias": 1, "b": 0}, 2),                                                           # a key that owns no slot
            (lay({"a.weight": slot(0, (5,)), "a.bias": slot(8, (3,))}, n=14), {"a.weight": 0, "a.bias": 1}, 2),    # arena not a multiple of 4
            (lay({"a.weight": slot(0, (5,)), "a.bias": slot(12, (7,))}), {"a.weight": 0, "a.bias": 1}, 2),         # behind the arena
            (lay({"a.weight": slot(0, (2, 2), (4, 1))}), {"a.weight": 0}, 1)):                                      # not dense
        with pytest.raises(CvxError):
            O.build_group_map(bad_layout, groups, n_groups)


# ---- 3. checkpoints -------------------------------------------------------------------------------------------------------------------
def _stock(opt, cls, model):
    """the stock torch optimiser over tensors of the reference's shapes, built with `opt`'s grouping"""
    named = list(model.named_parameters())
    ref = {k: torch.nn.Parameter(p.detach().clone().contiguous(), requires_grad=p.requires_grad) for k, p in named}
    hyper = [{k: v for k, v in g.items() if k not in ("params", "name", "frozen", "initial_lr")} for g in opt.param_groups]
    return cls([dict(h, params=[ref[k] for k in keys]) for h, keys in zip(hyper, opt.plan.keys)]), ref


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_checkpoint_round_trip_with_the_stock_torch_optimiser(kind, tmp_path):
    from computervision.pytorch_amd.model import Yolo8

    def make(m):
        if kind == "sgd":
            return O.FlatSGD(m, lr=0.02, momentum=0.9, nesterov=True, weight_decay=5e-4, groups=O.NO_DECAY_NORM_BIAS, bias_lr_scale=2.0,
                             freeze=("model.0.",), clip_grad_norm=10.0), torch.optim.SGD
        return O.FlatAdamW(m, lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.05, groups=O.NO_DECAY_NORM_BIAS, freeze=("model.0.",)), torch.optim.AdamW

    torch.manual_seed(0)
    m = Yolo8("n", 80)
    opt, cls = make(m)
    opt._ensure_state()
    gen = torch.Generator().manual_seed(5)
    for b in opt._buffers():                                                 # buffers filled by hand, as tests/test_trainer_cpu.py does for Adam
        b.copy_(torch.randn(b.shape, generator=gen))
    opt._state[1] = 3.0
    assert opt.device_step() == 3
    assert [g["lr"] for g in opt.param_groups] == ([0.02, 0.02, 0.04, 0.02] if kind == "sgd" else [2e-3] * 4)
    assert [g["weight_decay"] for g in opt.param_groups] == [5e-4 if kind == "sgd" else 0.05, 0.0, 0.0, 0.0]
    sd = opt.state_dict()
    index = {k: i for i, (k, _) in enumerate(m.named_parameters())}
    assert [g["params"] for g in sd["param_groups"]] == [[index[k] for k in keys] for keys in opt.plan.keys]
    assert sorted(i for g in sd["param_groups"] for i in g["params"]) == list(range(len(index)))
    stock, ref = _stock(opt, cls, m)
    assert set(sd["param_groups"][0]) - {"name", "frozen", "initial_lr"} == set(stock.state_dict()["param_groups"][0])
    stock.load_state_dict(sd)
    live = [k for g, keys in zip(opt.param_groups, opt.plan.keys) if not g["frozen"] for k in keys]
    assert len(stock.state) == len(live) and all(k.startswith("model.0.") or k.endswith("dfl.conv.weight") for k in opt.plan.keys[3])
    for k in live:
        for name, view in zip(opt.state_keys, opt._views(k)):
            assert torch.equal(stock.state[ref[k]][name], view), (k, name)
        if kind == "adamw":
            assert float(stock.state[ref[k]]["step"]) == 3.0
    # ... and back, through a checkpoint file, from the STOCK optimiser's own state_dict (ids in group order, not model order)
    path = str(tmp_path / "stock.pth")
    torch.save({"model": {k: v.detach().clone() for k, v in m.state_dict().items()}, "optimizer": stock.state_dict()}, path)
    torch.manual_seed(1)
    m2 = Yolo8("n", 80)
    opt2 = (O.FlatSGD(m2, lr=1.0, momentum=0.5, groups=O.NO_DECAY_NORM_BIAS, freeze=("model.0.",)) if kind == "sgd" else
            O.FlatAdamW(m2, lr=1.0, groups=O.NO_DECAY_NORM_BIAS, freeze=("model.0.",)))
    CheckPoint.load(path, "cpu", m2, optimizer=opt2)
    for k in live:
        for a, b in zip(opt._views(k), opt2._views(k)):
            assert torch.equal(a, b), k
    for g, g2 in zip(opt.param_groups, opt2.param_groups):
        for key in ("lr", "weight_decay") + (("momentum", "nesterov") if kind == "sgd" else ("betas", "eps")):
            assert g[key] == g2[key] or tuple(g[key]) == tuple(g2[key]), key
    assert opt2.device_step() == (3 if kind == "adamw" else 0)               # torch.optim.SGD counts no steps
    assert torch.equal(opt2._gs[:, :6], opt._gs[:, :6])
    # FlatOptimizer's own file through CheckPoint
    mine = str(tmp_path / "mine.pth")
    CheckPoint.save(m, mine, optimizer=opt)
    m3 = Yolo8("n", 80)
    opt3, _ = make(m3)
    CheckPoint.load(mine, "cpu", m3, optimizer=opt3)
    assert opt3.device_step() == 3 and all(torch.equal(a, b) for k in live for a, b in zip(opt._views(k), opt3._views(k)))
    with pytest.raises(CvxError):
        O.FlatSGD(Yolo8("n", 80), momentum=0.9).load_state_dict(sd)        # another grouping


# ---- 4. get_optimizer and the trainer --------------------------------------------------------------------------------------------------
def test_get_optimizer():
    from computervision.pytorch_amd.model import Yolo8
    from computervision.pytorch_amd.train import FlatAdam
    from core.trainer.engine_trainer import get_optimizer
    cfg = lambda train=None, **opt: SimpleNamespace(optimizer=SimpleNamespace(name="x", **opt), train=SimpleNamespace(**(train or {})))
    m = Yolo8("n", 80)
    assert type(get_optimizer("Adam", m, 1e-3)) is FlatAdam and type(get_optimizer("adam", m, 1e-3, cfg())) is FlatAdam
    sgd = get_optimizer("sgd", m, 0.01, cfg())
    assert type(sgd) is O.FlatSGD and len(sgd.param_groups) == 2 and sgd.clip_grad_norm is None
    g = sgd.param_groups[0]
    assert (g["lr"], g["momentum"], g["nesterov"], g["weight_decay"]) == (0.01, 0.937, True, 0.0)
    sgd = get_optimizer("SGD", Yolo8("n", 80), 0.01, cfg(dict(freeze=("model.0.", "model.1.")), momentum=0.9, nesterov=False, weight_decay=5e-4,
                                                         groups="no_decay_norm_bias", bias_lr_scale=2.0, clip_grad_norm=10.0))
    assert [(g["name"], g["lr"], g["weight_decay"], g["momentum"], g["nesterov"]) for g in sgd.param_groups] == [
        ("weights", 0.01, 5e-4, 0.9, False), ("norm", 0.01, 0.0, 0.9, False), ("bias", 0.02, 0.0, 0.9, False), ("frozen", 0.01, 0.0, 0.9, False)]
    assert sgd.clip_grad_norm == 10.0 and len(sgd.plan.keys[3]) == 7       # two Conv+BN blocks and the DFL projection
    adamw = get_optimizer("AdamW", m, 1e-3, cfg(weight_decay=0.05))
    assert type(adamw) is O.FlatAdamW and adamw.param_groups[0]["weight_decay"] == 0.05 and adamw.param_groups[0]["betas"] == (0.9, 0.999)
    adam = get_optimizer("adam", m, 1e-3, cfg(clip_grad_norm=1.0))
    assert type(adam) is O.FlatAdamW and adam.param_groups[0]["weight_decay"] == 0.0 and adam.clip_grad_norm == 1.0
    assert type(get_optimizer("adam", Yolo8("n", 80), 1e-3, cfg(dict(freeze=("model.0.",))))) is O.FlatAdamW
    for bad in ("rmsprop", "lamb"):
        with pytest.raises(ValueError):
            get_optimizer(bad, m, 1e-3, cfg())
    for name in ("sgd", "adamw", "rmsprop"):                               # without a config: the reference's function, Adam only (the trainers' call)
        with pytest.raises(ValueError, match=f"{name} is not supported"):
            get_optimizer(name, m, 1e-3)
    with pytest.raises(ValueError):
        O.FlatSGD(m, nesterov=True)
    with pytest.raises(ValueError):
        O.FlatSGD(m, clip_grad_norm=0.0)
    with pytest.raises(ValueError):
        O.FlatSGD(m, groups="by_layer")


def test_the_trainers_schedulers_walk_every_group():
    """MultiStepLR + LinearWarmup as EngineTrainer.set_lr_scheduler builds them, over a FlatSGD from get_optimizer: every group follows
    lr_t = initial * gamma^(milestones passed) * min(1, (t + 1) / warmup) times its own scale, and the device table's rows follow."""
    from computervision.pytorch_amd.model import Yolo8
    from core.trainer.base import LinearWarmup
    from core.trainer.engine_trainer import get_optimizer
    cfg = SimpleNamespace(optimizer=SimpleNamespace(name="sgd", groups="no_decay_norm_bias", bias_lr_scale=2.0, weight_decay=5e-4), train=SimpleNamespace())
    lr0, milestones = 0.01, [2, 4]
    opt = get_optimizer("sgd", Yolo8("n", 80), lr0, cfg)
    assert type(opt) is O.FlatSGD and [g["name"] for g in opt.param_groups] == ["weights", "norm", "bias", "frozen"]
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=milestones, gamma=0.1, last_epoch=-1)
    warm = LinearWarmup(opt, warmup_period=4, last_step=-1)
    scale = [1.0, 1.0, 2.0, 1.0]
    for t in range(9):
        want = lr0 * 0.1 ** sum(t >= m for m in milestones) * min(1.0, (t + 1) / 4)
        assert all(abs(g["lr"] - want * s) < 1e-12 for g, s in zip(opt.param_groups, scale)), t
        rows = opt._rows()
        assert [r[0] for r in rows] == [g["lr"] for g in opt.param_groups] and [r[3] for r in rows] == [0.0, 0.0, 0.0, 1.0]
        with warm.dampening():
            sched.step()


def test_new_symbols_in_header_library_and_prototypes():
    header = open(os.path.join(ROOT, "include", "cvx_engine.h")).read()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    lib = ctypes.CDLL(LIB_PATH) if os.path.exists(LIB_PATH) else None
    for name in ("cvx_optim_step", "cvx_grad_norm", "cvx_grad_norm_workspace"):
        assert name in declared and name in L.PROTOTYPES and (lib is None or hasattr(lib, name))
    assert len(L.PROTOTYPES["cvx_optim_step"][1]) == 21 and len(L.PROTOTYPES["cvx_grad_norm"][1]) == 12
    for name, value in (("CVX_OPTIM_MAX_GROUPS", E.OPTIM_MAX_GROUPS), ("CVX_OPTIM_GROUP_FLOATS", E.OPTIM_GROUP_FLOATS), ("CVX_OPTIM_UNMAPPED", E.OPTIM_UNMAPPED)):
        assert f"#define {name} {value}" in header
    assert "CVX_OPTIM_SGD = 0, CVX_OPTIM_ADAM = 1" in header and (E.OPTIM_SGD, E.OPTIM_ADAM) == (0, 1) and R.UNMAPPED == E.OPTIM_UNMAPPED
    assert "optim.hip" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
