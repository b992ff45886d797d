"""Writes tests/golden/adam_trace.npz: what the library's three ungrouped Adam entry points leave behind over the 5-step plan of
tests/test_optim_gpu.py, recorded on the device, so that a later build can be held to these bits.

    CVX_LIB=/path/to/the/recorded/build/libcvx_engine.so python tools/make_adam_golden.py <commit id of that build>

It needs the device and refuses to run without one.  ``commit`` in the file names the build that was recorded.  Per n in ``SIZES``
(3: scalar tail only; 4: one 16-byte chunk; 1027: 257 chunks = two workgroups and a 3-element tail; 1028: the same with a full last
chunk) the file holds the seeded inputs -- so the fixture does not depend on a torch RNG stream --

* ``n<n>_p0``, ``n<n>_e0``  (n,)     parameters and average at the start (both moments start at zero);
* ``n<n>_grads``            (5, n)   the gradient of each step, scales 1e-2 ... 1e2;

and per leg, after each step of ``PLAN`` (one step skipped by ``found_inf``, both ``zero_grad`` values), ``n<n>_<leg>_<array>`` (5, n)
for ``p``, ``m``, ``v``, ``g``, plus ``state`` (5, 4) and ``e`` where the leg has one:

* ``dev``   ``cvx_adam_step_dev``, grad_scale 0.5;
* ``ema``   ``cvx_adam_ema_step_dev``, grad_scale 0.5, d = 0.999;
* ``host``  ``cvx_adam_step`` with host factors, step = 1 ... 5 (no grad_scale, no device state; the skipped step is recorded too).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from computervision.pytorch_amd import _lib as L  # noqa: E402
from computervision.pytorch_amd import engine as E  # noqa: E402

SIZES = (3, 4, 1027, 1028)
PLAN = [dict(inf=0, zg=True), dict(inf=0, zg=False), dict(inf=1, zg=True), dict(inf=0, zg=False), dict(inf=0, zg=True)]
LR, BETAS, EPS, GRAD_SCALE, D = 1e-2, (0.9, 0.999), 1e-8, 0.5, 0.999
LEGS = {"dev": ("p", "m", "v", "g", "state"), "ema": ("p", "m", "v", "g", "e", "state"), "host": ("p", "m", "v", "g")}


def inputs(n):
    """tests/test_optim_gpu.py's Arenas(n, seed=n): p, g, a, b, e drawn in this order, then five gradients"""
    gen = torch.Generator().manual_seed(n)
    full = {k: torch.randn(n + 64, generator=gen) for k in ("p", "g", "a", "b", "e")}
    grads = torch.stack([torch.randn(n, generator=gen) * (10.0 ** (i - 2)) for i in range(5)])
    return full["p"][:n].numpy().copy(), full["e"][:n].numpy().copy(), grads.numpy().copy()


def run_leg(leg, p0, e0, grads, dev):
    n = p0.size
    t = {"p": torch.from_numpy(p0).to(dev), "e": torch.from_numpy(e0).to(dev), "g": torch.zeros(n, device=dev),
         "m": torch.zeros(n, device=dev), "v": torch.zeros(n, device=dev), "state": torch.tensor([LR, 0.0, 0.0, 0.0], device=dev)}
    found = torch.zeros(1, dtype=torch.int32, device=dev)
    out = {k: [] for k in LEGS[leg]}
    for i, st in enumerate(PLAN):
        t["g"].copy_(torch.from_numpy(grads[i]))
        found.fill_(st["inf"])
        if leg == "dev":
            E.adam_step_dev(t["p"], t["g"], t["m"], t["v"], BETAS, EPS, t["state"], found, st["zg"], GRAD_SCALE)
        elif leg == "ema":
            E.adam_ema_step_dev(t["p"], t["g"], t["m"], t["v"], BETAS, EPS, t["state"], t["e"], D, 1.0 - D, found, st["zg"], GRAD_SCALE)
        else:
            E.adam_step(t["p"], t["g"], t["m"], t["v"], LR, BETAS, EPS, i + 1, found, st["zg"])
        torch.cuda.synchronize()
        for k in out:
            out[k].append(t[k].cpu().numpy().copy())
    return {k: np.stack(v) for k, v in out.items()}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    if not torch.cuda.is_available():
        sys.exit("make_adam_golden.py records the device's own output: it needs the GPU")
    dev = torch.device("cuda:0")
    arrays = {"commit": np.array(sys.argv[1]), "lr": np.float64(LR), "betas": np.array(BETAS, np.float64), "eps": np.float64(EPS),
              "grad_scale": np.float64(GRAD_SCALE), "d": np.float64(D), "sizes": np.array(SIZES, np.int64)}
    for n in SIZES:
        p0, e0, grads = inputs(n)
        arrays[f"n{n}_p0"], arrays[f"n{n}_e0"], arrays[f"n{n}_grads"] = p0, e0, grads
        for leg in LEGS:
            for k, v in run_leg(leg, p0, e0, grads, dev).items():
                arrays[f"n{n}_{leg}_{k}"] = v
    path = os.path.join(ROOT, "tests", "golden", "adam_trace.npz")
    np.savez_compressed(path, **arrays)
    print(path, "library", L.LIB_PATH, "commit", sys.argv[1], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
