"""Cost of the device input pipeline next to the train step it feeds, all in one process, sources around 500 x 375:

* YOLO formats: event time of the two launches (``cvx_aug_images`` + ``cvx_aug_boxes``) at batch 32, 640 x 640, plain and mosaic; the
  write-bound floor (output bytes / the achievable HBM store rate); the YOLOv8-n fused train step at the same batch;
* ``fmt="ssd"`` at 300 x 300, batch 32, and ``fmt="centernet"`` at 384 x 384, batch 16, training (plain, mosaic) and validation: event time
  of the two launch groups -- image launch + ``cvx_aug_boxes_padded``, and the target kernel (``cvx_ssd_encode_targets`` /
  ``cvx_centernet_draw_targets``) on the labels and counts the first group left on the device -- and the trainer's fused step on such a batch.

    python tools/aug_cost.py [--out profiles/aug_cost.txt]

Needs the GPU; there is no CPU path.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, H, W = 32, 640, 640
HBM_STORE_RATE = 6.0e12          # bytes / s: plain coalesced stores as measured on the MI355X (6.0-6.2 TB/s; float4 copy 6.29 TB/s)
SIZES = [(375, 500), (500, 375), (333, 500), (375, 500), (500, 500), (480, 360), (360, 480), (375, 500)]


def event_ms(fn, warmup=5, iters=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def aug_case(dev, mosaic):
    """packs one batch with DeviceAugmenter.apply (checked run), then times its two launches alone on the same tables"""
    import aug_restatement as R
    from computervision.pytorch_amd import augment as A
    rng = np.random.RandomState(5)
    pics = [torch.from_numpy(R.synth_picture(h, w, 70 + i)).to(dev) for i, (h, w) in enumerate(SIZES)]
    boxes = [R.synth_boxes(h, w, 8, 80 + i) for i, (h, w) in enumerate(SIZES)]
    aug = A.DeviceAugmenter((H, W), seed=9)
    groups, bgroups = [], []
    for i in range(B):
        ids = [int(v) for v in rng.randint(0, len(pics), 4 if mosaic else 1)]
        groups.append([pics[k] for k in ids])
        bgroups.append([boxes[k] for k in ids])
    captured = {}
    launch = aug._launch

    def spy(*args):
        captured["args"] = args
        launch(*args)

    aug._launch = spy
    images, targets = aug(groups, bgroups, fmt="yolo7")
    aug._launch = launch
    n_in, n_out = sum(len(b) for bg in bgroups for b in bg), targets.shape[0]
    ms = event_ms(lambda: launch(*captured["args"]))
    return ms, n_in, n_out, float(images.mean())


def train_step_ms(dev):
    from computervision.pytorch_amd.model import Yolo8
    from computervision.pytorch_amd.train import FlatAdam, FusedTrainStep, V8DetectionLoss
    from configs import Yolo8DetConfig
    from oracle import synth
    cfg = Yolo8DetConfig()
    torch.manual_seed(0)
    model = Yolo8("n", 80, loss_scale=cfg.engine.loss_scale).to(dev).train()
    step = FusedTrainStep(model, V8DetectionLoss(cfg, model), FlatAdam(model, lr=cfg.train.initial_lr))
    x, batch = synth.images(B, H, W, seed=1).to(dev), synth.targets(B, seed=2)
    return event_ms(lambda: step(x, batch), warmup=10, iters=30)


def target_case(dev, fmt, hw, batch, alg, train, mosaic):
    """one ``fmt="ssd"`` / ``"centernet"`` batch through DeviceAugmenter (checked run), then its two launch groups alone on the same tables"""
    import aug_restatement as R
    from computervision.pytorch_amd import augment as A
    rng = np.random.RandomState(5)
    pics = [torch.from_numpy(R.synth_picture(h, w, 70 + i)).to(dev) for i, (h, w) in enumerate(SIZES)]
    boxes = [R.synth_boxes(h, w, 8, 80 + i) for i, (h, w) in enumerate(SIZES)]
    aug = A.DeviceAugmenter(hw, seed=9, train=train, target=alg)
    groups, bgroups = [], []
    for i in range(batch):
        ids = [int(v) for v in rng.randint(0, len(pics), 4 if mosaic else 1)]
        groups.append([pics[k] for k in ids] if mosaic else pics[ids[0]])
        bgroups.append([boxes[k] for k in ids] if mosaic else boxes[ids[0]])
    captured = {}
    launch = aug._launch_padded

    def spy(*args):
        captured["args"] = args
        launch(*args)

    aug._launch_padded = spy
    images, targets = aug(groups, bgroups, fmt=fmt)
    aug._launch_padded = launch
    labels, counts = captured["args"][5], captured["args"][6]
    make = alg.encode_targets if fmt == "ssd" else alg.draw_targets
    ms_aug = event_ms(lambda: launch(*captured["args"]))
    ms_tgt = event_ms(lambda: make(labels, counts))
    n_in = sum(len(b) for bg in bgroups for b in (bg if mosaic else [bg]))
    return ms_aug, ms_tgt, n_in, int(counts.sum()), tuple(labels.shape), (images, targets)


def target_lines(dev, name, fmt, hw, batch):
    """the three cases of one target format and the trainer's fused step on the mosaic batch"""
    import tempfile

    import builder
    cfg, alg_cls, trainer_cls = builder.export_from_registry(name)
    cfg.arch.input_size = (3,) + hw
    cfg.train.batch_size, cfg.train.epoch, cfg.train.pretrained = batch, 1, False
    cfg.train.save_path = tempfile.mkdtemp()
    alg = alg_cls(cfg, dev)
    lines = [f'fmt="{fmt}", batch {batch}, {hw[0]} x {hw[1]}: image launch + cvx_aug_boxes_padded | target kernel (event time, 50 repeats each)']
    batch_data = None
    for label, train, mosaic in (("train plain ", True, False), ("train mosaic", True, True), ("validation  ", False, False)):
        ms_aug, ms_tgt, n_in, n_out, shape, data = target_case(dev, fmt, hw, batch, alg, train, mosaic)
        lines.append(f"  {label}: {ms_aug * 1e3:8.1f} us | {ms_tgt * 1e3:8.1f} us; boxes {n_in} -> {n_out}, labels {shape}")
        if mosaic:
            batch_data = data
    torch.manual_seed(0)
    tr = trainer_cls(cfg, dev, dataloader=[batch_data])
    tr.model.train()
    ts = event_ms(lambda: tr.train_loop(batch_data, None), warmup=10, iters=30)
    lines.append(f"  {trainer_cls.__name__} fused train step on the mosaic batch, same run: {ts:.3f} ms")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aug_cost.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "aug_cost needs the MI355X"
    dev = torch.device("cuda:0")
    out_bytes = B * 3 * H * W * 4
    floor_ms = out_bytes / HBM_STORE_RATE * 1e3
    lines = [f"device augmentation, batch {B}, {H} x {W}, sources {sorted(set(SIZES))} uint8 HWC ({torch.cuda.get_device_name(0)})",
             f"output {out_bytes / 1e6:.1f} MB fp32 NCHW; write-bound floor at {HBM_STORE_RATE / 1e12:.1f} TB/s: {floor_ms * 1e3:.1f} us"]
    for mosaic in (False, True):
        ms, n_in, n_out, mean = aug_case(dev, mosaic)
        lines.append(f"{'mosaic' if mosaic else 'plain '}: cvx_aug_images + cvx_aug_boxes {ms * 1e3:8.1f} us per batch (event time, 50 launches) = "
                     f"{ms / floor_ms:.1f} x the floor, {out_bytes / ms / 1e9:.2f} TB/s written; boxes {n_in} -> {n_out}; mean pixel {mean:.4f}")
    ts = train_step_ms(dev)
    lines.append(f"YOLOv8-n fused train step, same batch and size, same run: {ts:.3f} ms")
    lines += target_lines(dev, "ssd", "ssd", (300, 300), 32)
    lines += target_lines(dev, "centernet", "centernet", (384, 384), 16)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
