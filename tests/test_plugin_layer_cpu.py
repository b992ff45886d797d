"""CPU: what the plugin layer (core/trainer, core/algorithms) shares between the models, pinned per model -- the inverse letterbox of the
SSD / YOLOv7 wrappers, the argument checks of ``evaluate_on_voc`` / ``evaluate_on_coco``, and the schedule, warm-up and loaders every
trainer sets up.  No engine call is made here."""
import numpy as np
import pytest
import torch

import builder
from computervision.pytorch_amd import CvxError

DETECTORS = ("yolo8_det", "yolo7", "ssd", "centernet")
TRAINERS = DETECTORS + ("deeplabv3plus",)


def correct_boxes_restated(box_xy, box_wh, input_shape, image_shape, letterbox_image):
    """The wrappers' ``_correct_boxes`` (yolo_correct_boxes, reference core/utils/image_process.py:161-181) operation by operation"""
    xywh = np.concatenate([box_xy, box_wh], axis=-1)
    if letterbox_image:
        ih, iw = image_shape
        h, w = input_shape
        scale = max(ih / h, iw / w)
        top, left = (h - ih / scale) // 2, (w - iw / scale) // 2
        cx, cy, bw, bh = xywh[:, 0] * w - left, xywh[:, 1] * h - top, xywh[:, 2] * w, xywh[:, 3] * h
        return np.stack([(cx - bw / 2) * scale, (cy - bh / 2) * scale, (cx + bw / 2) * scale, (cy + bh / 2) * scale], -1)
    out = np.stack([xywh[:, 0] - xywh[:, 2] / 2, xywh[:, 1] - xywh[:, 3] / 2, xywh[:, 0] + xywh[:, 2] / 2, xywh[:, 1] + xywh[:, 3] / 2], -1)
    out[:, ::2] *= image_shape[1]
    out[:, 1::2] *= image_shape[0]
    return out


@pytest.mark.parametrize("name", ["ssd", "yolo7"])
@pytest.mark.parametrize("letterbox_image", [True, False])
def test_correct_boxes_is_the_same_arithmetic(name, letterbox_image):
    cfg, algo_cls, _ = builder.export_from_registry(name)
    algo = algo_cls(cfg, "cpu")
    algo.letterbox_image = letterbox_image
    rs = np.random.RandomState(7)
    xy, wh = rs.rand(64, 2).astype(np.float32), (rs.rand(64, 2) * 0.5).astype(np.float32)
    for image_shape in ([375, 500], [500, 375]):
        got = algo._correct_boxes(xy, wh, algo.input_image_size, image_shape)
        want = correct_boxes_restated(xy, wh, algo.input_image_size, image_shape, letterbox_image)
        assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("name", DETECTORS)
def test_evaluation_arguments_are_checked_before_the_model(name, tmp_path):
    cfg, algo_cls, _ = builder.export_from_registry(name)
    algo = algo_cls(cfg, "cpu")
    with pytest.raises(ValueError) as e:
        algo.evaluate_on_voc(None, str(tmp_path), subset="train")
    assert str(e.value) == "sub_set must be one of 'test' and 'val', but got train"
    with pytest.raises(CvxError) as e:
        algo.evaluate_on_voc(None, str(tmp_path), dataloader=None)
    assert str(e.value) == ("evaluate_on_voc reads no dataset from disk: pass dataloader= yielding (images, dict(image_hw, gt, gt_counts)) on the "
                            "device over the VOC-val pictures in sorted-id order")
    with pytest.raises(ValueError) as e:
        algo.evaluate_on_coco(None, str(tmp_path), subset="train")
    assert str(e.value) == "evaluate_on_coco evaluates subset 'val' only, got train"
    with pytest.raises(CvxError) as e:
        algo.evaluate_on_coco(None, str(tmp_path), dataloader=None)
    assert str(e.value) == ("evaluate_on_coco reads no dataset from disk: pass dataloader= yielding (images, dict(image_hw, gt_coco, gt_counts)) "
                            "on the device over the COCO-val pictures in sorted-image-id order")
    assert not list(tmp_path.iterdir())


def trainer(name, loader, **train):
    cfg, _, trainer_cls = builder.export_from_registry(name)
    cfg.train.pretrained = False
    for k, v in train.items():
        setattr(cfg.train, k, v)
    return trainer_cls(cfg, "cpu", dataloader=loader)


@pytest.mark.parametrize("name", TRAINERS)
def test_trainer_schedule_warmup_and_loaders(name):
    """lr_t = initial * gamma^(iteration milestones passed) * min(1, (t + 1) / warmup), the formula of tests/test_trainer_cpu.py, from the
    trainer's own ``set_lr_scheduler``: epoch milestones [0, 1] on a two-batch loader are iterations [2, 4], and stay [0, 1] for
    DeepLabv3+ (``use_iter_milestones=False``)."""
    loader = [None, None]
    tr = trainer(name, loader, warmup_iters=4, milestones=[0, 1], gamma=0.1)
    assert tr.train_dataloader is loader and tr.val_dataloader is tr.train_dataloader
    assert tr.milestones == ([0, 1] if name == "deeplabv3plus" else [2, 4]) and tr.last_iter == 0
    assert type(tr.optimizer).__name__ == "FlatAdam" and tr.criterion is not None and tr.ema is None
    lrs = [tr.optimizer.param_groups[0]["lr"]]
    for _ in range(8):
        with tr.warmup_scheduler.dampening():
            tr.lr_scheduler.step()
        lrs.append(tr.optimizer.param_groups[0]["lr"])
    want = [tr.initial_lr * 0.1 ** sum(t >= m for m in tr.milestones) * min(1.0, (t + 1) / 4) for t in range(9)]
    assert all(abs(a - b) < 1e-12 for a, b in zip(lrs, want)), (lrs, want)


@pytest.mark.parametrize("name", TRAINERS)
def test_trainer_without_warmup_and_with_its_own_synthetic_loader(name):
    tr = trainer(name, None, warmup_iters=0, milestones=[])
    assert tr.warmup_scheduler is None and tr.lr_scheduler.milestones == {int(1e8): 1, int(1e8) + 1: 1}
    assert type(tr.train_dataloader).__name__.startswith("Synthetic") and tr.val_dataloader is tr.train_dataloader
    assert tr.milestones == [] and tr.optimizer.param_groups[0]["lr"] == tr.initial_lr
    want = {"yolo8_det": ["loss"], "yolo7": ["loss", "box_loss", "obj_loss", "cls_loss"], "ssd": ["loss", "loc_loss", "conf_loss"],
            "centernet": ["loss"], "deeplabv3plus": ["loss"]}[name]
    assert tr.metric_names == want and tr.show_option == [True] * len(want)


def test_unsupported_optimizer_name():
    cfg, _, trainer_cls = builder.export_from_registry("centernet")
    cfg.optimizer.name = "sgd"
    with pytest.raises(ValueError, match="sgd is not supported"):
        trainer_cls(cfg, "cpu", dataloader=[None])
