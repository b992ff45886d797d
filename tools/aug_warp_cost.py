"""Cost of stage 2 of the device augmentation (affine / perspective warp and MixUp) next to the pipeline it extends:
batch 32 at 640 x 640, sources around 500 x 375, mosaic batches, ``fmt="yolo7"``, everything in one process.

Arms, interleaved -- every arm runs in every block, a block times 50 back-to-back repeats of an arm between two device events after a
warm-up, and the figure is the median over the blocks of the time per repeat:

* ``two_launches``            today's group, ``cvx_aug_images`` + ``cvx_aug_boxes`` (``DeviceAugmenter._launch``);
* ``four_launches_affine``    stage 1 into scratch (``cvx_aug_images`` + ``cvx_aug_boxes_padded``) + ``cvx_aug_warp_mix`` +
                              ``cvx_aug_boxes_warp``, no partners: every canvas is read once;
* ``four_launches_mixup``     the same with a partner for every output: every canvas is read twice;
* ``stage_2_affine`` / ``stage_2_mixup``   the two stage-2 launches alone on the canvases and labels stage 1 left.

Next to each stage-2 figure stand the bytes it must move (the canvases read once or twice, the batch written once) and the time those bytes
take at ``STREAM_RATE``.

    python tools/aug_warp_cost.py [--out profiles/aug_warp_cost.json]

Needs the GPU; there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, H, W = 32, 640, 640
BLOCKS, REPEATS, WARMUP = 9, 50, 5
STREAM_RATE = 5.3e12             # bytes / s read + written by the streaming kernels of this project on the MI355X (profiles/optim_step_cost.json: 5.2-5.5 TB/s)
SIZES = [(375, 500), (500, 375), (333, 500), (375, 500), (500, 500), (480, 360), (360, 480), (375, 500)]
AFFINE = dict(degrees=10.0, translate=0.1, scale=0.5, shear=2.0, perspective=0.0005)


def block_us(fn):
    for _ in range(WARMUP):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPEATS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPEATS


def capture(aug, groups, bgroups, **kw):
    """one checked call of the augmenter; returns the arguments its launch groups were given"""
    seen = {}
    for name in ("_launch", "_launch_padded", "_launch_warp"):
        def spy(*args, _name=name, _fn=getattr(aug, name)):
            seen[_name] = args
            _fn(*args)
        setattr(aug, name, spy)
    images, targets = aug(groups, bgroups, fmt="yolo7", **kw)
    for name in ("_launch", "_launch_padded", "_launch_warp"):
        delattr(aug, name)
    return seen, images, targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aug_warp_cost.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "aug_warp_cost needs the MI355X"
    import aug_restatement as R
    from computervision.pytorch_amd import augment as A
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(5)
    pics = [torch.from_numpy(R.synth_picture(h, w, 70 + i)).to(dev) for i, (h, w) in enumerate(SIZES)]
    boxes = [R.synth_boxes(h, w, 8, 80 + i) for i, (h, w) in enumerate(SIZES)]
    groups, bgroups = [], []
    for _ in range(B):
        ids = [int(v) for v in rng.randint(0, len(pics), 4)]
        groups.append([pics[k] for k in ids])
        bgroups.append([boxes[k] for k in ids])

    plain = A.DeviceAugmenter((H, W), seed=9)
    seen0, _, t0 = capture(plain, groups, bgroups)
    affine = A.DeviceAugmenter((H, W), seed=9, affine=AFFINE)
    seen1, im1, t1 = capture(affine, groups, bgroups)
    mixup = A.DeviceAugmenter((H, W), seed=9, affine=AFFINE, mixup=1.0)
    seen2, im2, t2 = capture(mixup, groups, bgroups)
    assert "_launch_warp" not in seen0 and int((mixup.last_warp["partner"] >= 0).sum()) == B and int((affine.last_warp["partner"] >= 0).sum()) == 0
    assert bool(torch.isfinite(im1).all()) and bool(torch.isfinite(im2).all())

    arms = {
        "two_launches": lambda: plain._launch(*seen0["_launch"]),
        "four_launches_affine": lambda: (affine._launch_padded(*seen1["_launch_padded"]), affine._launch_warp(*seen1["_launch_warp"])),
        "four_launches_mixup": lambda: (mixup._launch_padded(*seen2["_launch_padded"]), mixup._launch_warp(*seen2["_launch_warp"])),
        "stage_2_affine": lambda: affine._launch_warp(*seen1["_launch_warp"]),
        "stage_2_mixup": lambda: mixup._launch_warp(*seen2["_launch_warp"]),
    }
    times = {k: [] for k in arms}
    for _ in range(BLOCKS):
        for k, fn in arms.items():
            times[k].append(block_us(fn))
    batch_bytes = B * 3 * H * W * 4
    needed = {"stage_2_affine": 2 * batch_bytes, "stage_2_mixup": 3 * batch_bytes}
    result = {
        "method": f"{BLOCKS} blocks, every arm in every block ({REPEATS} back-to-back repeats between two device events after {WARMUP} warm-up "
                  f"repeats per arm), median over blocks of the time per repeat; one {torch.cuda.get_device_name(0)}; batch {B}, {H} x {W}, mosaic "
                  f"batches, sources {sorted(set(SIZES))} uint8 HWC, fmt yolo7, affine {AFFINE}",
        "batch_bytes": batch_bytes,
        "stream_rate_TB_per_s": STREAM_RATE / 1e12,
        "boxes": {"source": sum(len(b) for bg in bgroups for b in bg), "two_launches": int(t0.shape[0]), "affine": int(t1.shape[0]), "mixup": int(t2.shape[0])},
        "arms": {},
    }
    for k, v in times.items():
        arm = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
        if k in needed:
            arm["needed_bytes"] = needed[k]
            arm["floor_us"] = round(needed[k] / STREAM_RATE * 1e6, 2)
            arm["needed_TB_per_s"] = round(needed[k] / statistics.median(v) / 1e6, 3)
        result["arms"][k] = arm
    text = json.dumps(result, indent=1)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
