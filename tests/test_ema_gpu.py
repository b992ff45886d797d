"""GPU (MI355X): the weight average -- ``cvx_ema_update``, ``cvx_adam_ema_step_dev``, ``ModelEMA``, ``FlatAdam.attach_ema``, the trainer.

Every comparison here is bit-exact (``torch.equal``), and can be: the average is three correctly rounded fp32 operations in a fixed order
on both sides (tests/test_ema_cpu.py pins that formula against the real reference), and the fused kernel's Adam arithmetic is specified
as ``cvx_adam_step_dev``'s own.
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from computervision.pytorch_amd import _lib as L  # noqa: E402
from computervision.pytorch_amd import engine as E  # noqa: E402
from computervision.pytorch_amd.ema import ModelEMA  # noqa: E402
from oracle import synth  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def factors(updates, decay=0.9999, tau=2000.0):
    d = float(decay) * (1 - math.exp(-updates / float(tau)))
    return d, 1 - d


def host_step(e, p, d, omd):
    """one update of the recurrence on the host, numpy fp32: rn(rn(e * d) + rn(omd * p))"""
    return (e * np.float32(d)).astype(np.float32) + (np.float32(omd) * p).astype(np.float32)


def host_replay(e0, snapshots, updates0=0, decay=0.9999, tau=2000.0):
    e = e0.detach().cpu().numpy().astype(np.float32).copy()
    for i, p in enumerate(snapshots):
        d, omd = factors(updates0 + i + 1, decay, tau)
        e = host_step(e, p.detach().cpu().numpy(), d, omd)
    return torch.from_numpy(e)


# ---- 1. the kernel against the reference fixture -----------------------------------------------------------
@pytest.mark.parametrize("leg", ["cold", "warm"])
def test_ema_update_kernel_is_bit_identical_to_the_reference(dev, gold, leg):
    g = gold("ema_ref.npz")
    e = torch.from_numpy(g[f"{leg}_init"]).to(dev)
    src = torch.from_numpy(g[f"{leg}_src"]).to(dev)
    ref = torch.from_numpy(g[f"{leg}_ema"]).to(dev)
    u = int(g[f"{leg}_updates0"])
    assert e.numel() % 4 != 0
    for t in range(src.shape[0]):
        d, omd = factors(u + t + 1, g["decay"], g["tau"])
        row = src[t].clone()                                   # (a fresh allocation: 16-byte aligned, which a row of `src` need not be)
        E.ema_update(e, row, d, omd)
        assert torch.equal(row, src[t])                        # the source is only read
    torch.cuda.synchronize()
    assert torch.equal(e, ref[-1])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_ema_update_kernel_small_sizes_and_refusals(dev, n):
    torch.manual_seed(n)
    guard = 8
    buf = torch.randn(n + guard, device=dev)                   # the values behind the n-th must not be touched
    e, p = buf[:n], torch.randn(n, device=dev)
    before = buf.clone()
    d, omd = factors(1234)
    E.ema_update(e, p, d, omd)
    torch.cuda.synchronize()
    want = torch.from_numpy(host_step(before[:n].cpu().numpy(), p.cpu().numpy(), d, omd))
    assert torch.equal(buf[:n].cpu(), want) and torch.equal(buf[n:], before[n:])
    lib = L.load()
    st = L.stream_ptr(dev)
    big = torch.zeros(16, device=dev)
    other = torch.zeros(16, device=dev)
    assert lib.cvx_ema_update(L.ptr(big[1:]), L.ptr(other), 4, 0.5, 0.5, st) != 0          # misaligned average
    assert lib.cvx_ema_update(L.ptr(big), L.ptr(other[1:]), 4, 0.5, 0.5, st) != 0          # misaligned source
    assert lib.cvx_ema_update(L.ptr(big), L.ptr(big), 4, 0.5, 0.5, st) != 0                # the average of itself
    assert b"align" in lib.cvx_last_error() or b"average" in lib.cvx_last_error()
    with pytest.raises(L.CvxError):
        E.ema_update(big, other[:8], 0.5, 0.5)
    torch.cuda.synchronize()
    assert float(big.abs().sum()) == 0.0


# ---- 2. fused == unfused -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4099, 1 << 16, 3])
def test_fused_adam_ema_equals_adam_then_ema(dev, n):
    """cvx_adam_ema_step_dev against cvx_adam_step_dev followed by cvx_ema_update on the same seeded arenas: p, m, v, g and the average bit for
    bit over 5 steps -- one of them skipped by found_inf (p, m, v and the step count stand still, the average moves), grad_scale = 0.5,
    zero_grad both ways, n not a multiple of 4 (n = 3: the scalar tail alone)."""
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (10.0 ** (i - 2)) for i in range(5)]
    betas, eps = (0.9, 0.999), 1e-8
    plan = [dict(inf=0, zg=True), dict(inf=0, zg=False), dict(inf=1, zg=True), dict(inf=0, zg=False), dict(inf=0, zg=True)]
    runs = []
    for fused in (True, False):
        p, g = p0.clone().to(dev), torch.zeros(n, device=dev)
        m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
        e = (p0 * 0.5 + 0.25).to(dev)
        state = torch.tensor([1e-2, 0.0, 0.0, 0.0], device=dev)
        found = torch.zeros(1, dtype=torch.int32, device=dev)
        trace = []
        for i, st in enumerate(plan):
            g.copy_(grads[i].to(dev))
            found.fill_(st["inf"])
            d, omd = factors(300 * (i + 1))
            before = (p.clone(), m.clone(), v.clone(), e.clone(), float(state[1]))
            if fused:
                E.adam_ema_step_dev(p, g, m, v, betas, eps, state, e, d, omd, found, st["zg"], 0.5)
            else:
                E.adam_step_dev(p, g, m, v, betas, eps, state, found, st["zg"], 0.5)
                E.ema_update(e, p, d, omd)
            torch.cuda.synchronize()
            if st["inf"]:
                assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2]) and float(state[1]) == before[4]
                assert not torch.equal(e, before[3])
            else:
                assert not torch.equal(p, before[0]) and float(state[1]) == before[4] + 1
            assert bool((g == 0).all()) == st["zg"]
            trace.append([t.clone().cpu() for t in (p, m, v, g, e, state)])
        runs.append(trace)
    for i, (a, b) in enumerate(zip(*runs)):
        for name, x, y in zip(("p", "m", "v", "g", "ema", "state"), a, b):
            assert torch.equal(x, y), f"step {i}: {name} differs between the fused and the two-launch step"
    lib = L.load()
    bad = torch.zeros(16, device=dev)
    args = lambda ema: (L.ptr(bad), L.ptr(bad), L.ptr(bad), L.ptr(bad), 4, 0.9, 0.999, 1e-8, L.ptr(torch.zeros(4, device=dev)), None, 1, 1.0, ema, 0.5, 0.5,
                        L.stream_ptr(dev))
    assert lib.cvx_adam_ema_step_dev(*args(L.ptr(bad))) != 0                                 # ema == params
    assert lib.cvx_adam_ema_step_dev(*args(L.ptr(torch.zeros(16, device=dev)[1:]))) != 0      # misaligned


# ---- 3 + 4. YOLOv8: the average does not disturb training, and the clone's forward sees it -----------------
def _yolo8_runs(dev, steps=3):
    from computervision.pytorch_amd.model import Yolo8
    from computervision.pytorch_amd.train import FlatAdam, FusedTrainStep, V8DetectionLoss
    from configs import Yolo8DetConfig
    x, batch = synth.images(2, 128, 128, seed=1).to(dev), {k: v.to(dev) for k, v in synth.targets(2, seed=2).items()}
    out = {}
    for with_ema in (False, True):
        torch.manual_seed(0)
        m = Yolo8("n", 80).to(dev).train()
        opt = FlatAdam(m, lr=1e-3)
        step = FusedTrainStep(m, V8DetectionLoss(Yolo8DetConfig(), m), opt, n_buckets=4)
        ema = None
        if with_ema:
            ema = ModelEMA(m)
            out["init"] = {k: ema.ema._flat[k].clone().cpu() for k in ("param", "stat", "nbt")}
            with torch.no_grad():
                out["y_before"] = ema.ema(x)[0].clone()           # the clone's engine now holds fp16 images of the initial weights
            opt.attach_ema(ema)
        losses, snaps = [], []
        for _ in range(steps):
            losses.append(step(x, batch).clone())
            snaps.append((m.flat_params.clone().cpu(), m.flat_stats.clone().cpu()))
        torch.cuda.synchronize()
        out[with_ema] = dict(losses=torch.stack(losses).cpu(), params=m.flat_params.clone().cpu(), stats=m.flat_stats.clone().cpu(), snaps=snaps,
                             ema=ema, model=m)
    out["x"] = x
    return out


def test_average_does_not_disturb_training_and_follows_the_recurrence(dev):
    r = _yolo8_runs(dev)
    plain, avg = r[False], r[True]
    assert torch.equal(plain["losses"], avg["losses"]) and torch.equal(plain["params"], avg["params"]) and torch.equal(plain["stats"], avg["stats"])
    ema = avg["ema"]
    assert ema.updates == 3
    assert torch.equal(ema.ema.flat_params.cpu(), host_replay(r["init"]["param"], [s[0] for s in avg["snaps"]]))
    assert torch.equal(ema.ema.flat_stats.cpu(), host_replay(r["init"]["stat"], [s[1] for s in avg["snaps"]]))
    assert not torch.equal(ema.ema.flat_params.cpu(), r["init"]["param"]) and not torch.equal(ema.ema.flat_stats.cpu(), r["init"]["stat"])
    assert torch.equal(ema.ema._flat["nbt"].cpu(), r["init"]["nbt"])
    assert not torch.equal(avg["model"]._flat["nbt"].cpu(), r["init"]["nbt"])


def test_the_clones_forward_sees_the_update(dev):
    """The clone ran a forward BEFORE the steps, so its engine holds fp16 weight images; the raw-pointer writes of the average must end them."""
    from computervision.pytorch_amd.model import Yolo8
    r = _yolo8_runs(dev)
    ema, x = r[True]["ema"], r["x"]
    with torch.no_grad():
        y_ema = ema.ema(x)[0]
        fresh = Yolo8("n", 80).to(dev).eval()
        fresh.load_state_dict(ema.ema.state_dict())
        y_fresh = fresh(x)[0]
    torch.cuda.synchronize()
    assert torch.equal(y_ema, y_fresh)
    assert not torch.equal(y_ema, r["y_before"])
    # the same through ModelEMA.update alone (no optimiser): one more update, one more forward
    ema.update(r[True]["model"])
    with torch.no_grad():
        y2 = ema.ema(x)[0]
        fresh.load_state_dict(ema.ema.state_dict())
        y2_fresh = fresh(x)[0]
    assert ema.updates == 4 and torch.equal(y2, y2_fresh) and not torch.equal(y2, y_ema)


# ---- 5. the other four families --------------------------------------------------------------------------------
def _family_cases(dev, gold):
    from computervision.pytorch_amd.deeplab import DeepLabV3PlusR101, SegLoss, SegTrainStep
    from computervision.pytorch_amd.dla import CenterNetDLA34, CenterNetLoss, CenterNetTrainStep
    from computervision.pytorch_amd.ssd import MultiBoxLoss, SSD300VGG, SsdTrainStep
    from computervision.pytorch_amd.yolov7 import Yolo7L, Yolo7Loss, Yolo7TrainStep
    from core.trainer.centernet_train import SyntheticCenterNetLoader
    from core.trainer.ssd_train import SyntheticSsdLoader
    from core.trainer.yolo7_train import SyntheticYolo7Loader

    def loader_batch(loader):
        images, targets = next(iter(loader))
        return images.to(dev), ([t.to(dev) for t in targets] if isinstance(targets, list) else targets.to(dev))

    def deeplab_batch():
        g = gold("deeplab_train_97x129.npz")
        return torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["target"].astype(np.int64)).to(dev)

    return {
        "deeplab": (lambda: DeepLabV3PlusR101(21), lambda m: SegLoss("focal"), SegTrainStep, deeplab_batch),
        "centernet": (lambda: CenterNetDLA34(20), lambda m: CenterNetLoss(20), CenterNetTrainStep,
                      lambda: loader_batch(SyntheticCenterNetLoader(2, (128, 160), 20, length=1, seed=2))),
        "ssd": (lambda: SSD300VGG(20), lambda m: MultiBoxLoss(3, 20), SsdTrainStep, lambda: loader_batch(SyntheticSsdLoader(2, (300, 300), 20, length=1, seed=2))),
        "yolov7": (lambda: Yolo7L(20), lambda m: Yolo7Loss(None, 20, (160, 224)), Yolo7TrainStep,
                   lambda: loader_batch(SyntheticYolo7Loader(2, (160, 224), 20, length=1, seed=2))),
    }


@pytest.mark.parametrize("family", ["deeplab", "centernet", "ssd", "yolov7"])
def test_other_families_average_inside_their_fused_step(dev, gold, family):
    """One fused train step each at the smallest shape the family's train tests use; the clone's two arenas against the host replay."""
    from computervision.pytorch_amd.train import DynamicLossScale, FlatAdam
    make, crit, step_cls, get_batch = _family_cases(dev, gold)[family]
    images, targets = get_batch()
    torch.manual_seed(0)
    m = make().to(dev).train()
    opt = FlatAdam(m, lr=1e-3)
    # (DeepLab's static scale is GradScaler's 65536: its existing step test starts the dynamic scale at 4096, so does this one)
    step = step_cls(m, crit(m), opt, scaler=DynamicLossScale(dev, init_scale=4096.0) if family == "deeplab" else None)
    ema = ModelEMA(m, decay=0.999, tau=50, updates=20)
    init = {k: ema.ema._flat[k].clone().cpu() for k in ("param", "stat", "nbt")}
    opt.attach_ema(ema)
    p0 = m.flat_params.clone()
    loss = step(images, targets)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and not torch.equal(m.flat_params, p0) and ema.updates == 21
    assert torch.equal(ema.ema.flat_params.cpu(), host_replay(init["param"], [m.flat_params], 20, 0.999, 50))
    assert torch.equal(ema.ema.flat_stats.cpu(), host_replay(init["stat"], [m.flat_stats], 20, 0.999, 50))
    assert not torch.equal(ema.ema.flat_params.cpu(), init["param"]) and torch.equal(ema.ema._flat["nbt"].cpu(), init["nbt"])
    assert not ema.ema.training and ema.ema._flat["grad"] is None


# ---- 6. trainer and checkpoints ---------------------------------------------------------------------------------
def test_yolo8_trainer_keeps_saves_resumes_and_evaluates_the_average(dev, tmp_path):
    """cfg.train.ema = True, three iterations, save_interval = 1.  (``train(max_iters=...)`` returns before any checkpoint is written, with or
    without an average, so the three iterations are one epoch over a three-batch loader.)"""
    import builder
    from computervision.pytorch_amd.model import Yolo8
    from core.trainer.yolo8_train import SyntheticDetectionLoader
    from core.utils.ckpt import CheckPoint

    def config(resume=""):
        cfg, _, trainer_cls = builder.export_from_registry("yolo8_det")
        cfg.arch.input_size = (3, 128, 128)
        cfg.engine.init_loss_scale = 1024.0
        cfg.train.batch_size, cfg.train.epoch, cfg.train.save_interval, cfg.train.eval_interval = 2, 1, 1, 1
        cfg.train.save_path = str(tmp_path / ("resumed" if resume else "saves"))
        cfg.train.ema, cfg.train.ema_decay, cfg.train.ema_tau = True, 0.999, 100
        cfg.log.print_interval = 1
        if resume:
            cfg.train.resume_training, cfg.train.last_epoch = resume, 0
        return cfg, trainer_cls

    cfg, trainer_cls = config()
    torch.manual_seed(0)
    loader = SyntheticDetectionLoader(2, (128, 128), cfg.dataset.num_classes, length=3, seed=5)
    tr = trainer_cls(cfg, dev, dataloader=loader)
    assert tr.ema is not None and tr.eval_model is tr.ema.ema and tr.optimizer._ema is tr.ema
    calls = {"model": 0, "clone": 0}
    tr.model.register_forward_hook(lambda *a: calls.__setitem__("model", calls["model"] + 1))
    tr.ema.ema.register_forward_hook(lambda *a: calls.__setitem__("clone", calls["clone"] + 1))
    tr.train()
    torch.cuda.synchronize()
    assert tr.ema.updates == 3
    assert calls == {"model": 0, "clone": 3}                       # evaluate_loop ran on the clone (the fused step does not go through __call__)
    assert not tr.ema.ema.training
    tag = f"{tr.model_name}_{str(tr.dataset_name).lower()}"
    ckpt_path = os.path.join(cfg.train.save_path, f"{tag}_epoch-0.pth")
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=False)
    assert ckpt["ema"]["updates"] == 3 and list(ckpt["ema"]["model"]) == list(ckpt["model"])
    assert not torch.equal(tr.ema.ema.flat_params, tr.model.flat_params)
    # the bare files: the model's, unchanged in kind, and the average's
    final, final_ema = Yolo8("n", cfg.dataset.num_classes), Yolo8("n", cfg.dataset.num_classes)
    CheckPoint.load_pure(os.path.join(cfg.train.save_path, f"{tag}_final.pth"), "cpu", final)
    CheckPoint.load_pure(os.path.join(cfg.train.save_path, f"{tag}_final_ema.pth"), "cpu", final_ema)
    assert torch.equal(final.flat_params, tr.model.flat_params.cpu()) and torch.equal(final_ema.flat_params, tr.ema.ema.flat_params.cpu())
    assert torch.equal(final_ema.flat_stats, tr.ema.ema.flat_stats.cpu())
    # resume
    cfg2, trainer_cls = config(resume=ckpt_path)
    torch.manual_seed(1)
    tr2 = trainer_cls(cfg2, dev, dataloader=loader)
    assert tr2.ema.updates == 0 and not torch.equal(tr2.ema.ema.flat_params, tr.ema.ema.flat_params)
    tr2.train()                                                    # epoch 1 of 1: loads the checkpoint, trains nothing
    assert tr2.ema.updates == 3
    for k in ("param", "stat", "nbt"):
        assert torch.equal(tr2.ema.ema._flat[k], tr.ema.ema._flat[k]), k
        assert torch.equal(tr2.model._flat[k], tr.model._flat[k]), k
