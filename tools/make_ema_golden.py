"""Writes tests/golden/ema_ref.npz: the REAL reference ``ModelEMA`` (core/trainer/lr_scheduler.py:55-84) run for 40 updates over a small
seeded conv + BN + conv module whose parameters, running statistics and ``num_batches_tracked`` are perturbed between updates.

    python tools/make_ema_golden.py /path/to/ComputerVision.pytorch

The reference module is loaded by file path (importing it as a package pulls in the whole trainer stack).  Two legs: ``cold`` starts at
``updates = 0`` (d ramps up from ~5e-4), ``warm`` at ``updates = 50000`` (d ~ decay).  Per leg, flattened in ``state_dict`` order over the
floating-point entries only (n = 206 values, n % 4 = 2, so the kernels' scalar tail is exercised):

* ``<leg>_init``  (n,)      the average's state when it was cloned;
* ``<leg>_src``   (40, n)   the model's state at each update;
* ``<leg>_ema``   (40, n)   the average after each update (the last row is the final state);
* ``<leg>_updates0`` / ``decay`` / ``tau``, ``<leg>_nbt_init`` and ``<leg>_nbt_final`` (the clone's ``num_batches_tracked``).
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 40
DECAY, TAU = 0.9999, 2000


def load_reference(ref_root):
    spec = importlib.util.spec_from_file_location("ref_lr_scheduler", os.path.join(ref_root, "core", "trainer", "lr_scheduler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_module():
    return nn.Sequential(nn.Conv2d(3, 5, 3), nn.BatchNorm2d(5), nn.Conv2d(5, 1, 3, bias=True))      # 140 + 20 + 46 = 206 floats


def flat(sd):
    return torch.cat([v.detach().reshape(-1).float() for v in sd.values() if v.dtype.is_floating_point]).numpy().copy()


def run_leg(ref, updates0, seed):
    torch.manual_seed(seed)
    model = make_module()
    with torch.no_grad():
        model[1].running_mean.normal_()
        model[1].running_var.uniform_(0.5, 2.0)
        model[1].num_batches_tracked.fill_(7)
    ema = ref.ModelEMA(model, decay=DECAY, tau=TAU, updates=updates0)
    out = {"init": flat(ema.ema.state_dict()), "nbt_init": np.int64(ema.ema[1].num_batches_tracked.item())}
    src, avg = [], []
    g = torch.Generator().manual_seed(seed + 1)
    for _ in range(STEPS):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
            model[1].running_mean.add_(torch.randn(5, generator=g) * 0.1)
            model[1].running_var.mul_(1.0 + 0.1 * torch.rand(5, generator=g))
            model[1].num_batches_tracked.add_(1)
        ema.update(model)
        src.append(flat(model.state_dict()))
        avg.append(flat(ema.ema.state_dict()))
    out["src"], out["ema"] = np.stack(src), np.stack(avg)
    out["nbt_final"] = np.int64(ema.ema[1].num_batches_tracked.item())
    out["updates0"] = np.int64(updates0)
    assert ema.updates == updates0 + STEPS
    return out


def main():
    ref = load_reference(sys.argv[1])
    arrays = {"decay": np.float64(DECAY), "tau": np.float64(TAU)}
    for leg, updates0, seed in (("cold", 0, 11), ("warm", 50000, 12)):
        for k, v in run_leg(ref, updates0, seed).items():
            arrays[f"{leg}_{k}"] = v
    n = arrays["cold_init"].shape[0]
    assert n % 4 != 0, n
    path = os.path.join(ROOT, "tests", "golden", "ema_ref.npz")
    np.savez_compressed(path, **arrays)
    print(path, "n =", n, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
