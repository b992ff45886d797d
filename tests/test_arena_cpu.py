"""The plumbing the five model families share (computervision.pytorch_amd/arena.py), without a GPU: the initial ``state_dict`` against
each family's oracle, the arena sizes, the ``_apply`` contract, the CPU refusal and the train-step constructor."""
import importlib

import pytest
import torch

from computervision.pytorch_amd import CvxError

PKG = "computervision.pytorch_amd."
# family -> (module, class, constructor arguments, oracle module, oracle arguments, state_dict entries, param arena, stat arena, input size)
FAMILIES = {
    "yolov8": ("model", "Yolo8", ("n", 80), "yolov8_ref", ("n", 80), 355, 3157184, 10592, (64, 64)),
    "yolov7": ("yolov7", "Yolo7L", (20,), "yolov7_ref", (20,), 558, 37306000, 49728, (64, 64)),
    "ssd": ("ssd", "SSD300VGG", (20,), "ssd_ref", (20,), 136, 26363072, 8448, (300, 300)),
    "centernet": ("dla", "CenterNetDLA34", (80,), "centernet_ref", (80,), 326, 18477560, 19072, (64, 64)),
    "deeplab": ("deeplab", "DeepLabV3PlusR101", (21,), "deeplab_ref", (21,), 674, 58754744, 109024, (65, 65)),
}
STEPS = {"yolov8": ("train", "FusedTrainStep"), "yolov7": ("yolov7", "Yolo7TrainStep"), "ssd": ("ssd", "SsdTrainStep"),
         "centernet": ("dla", "CenterNetTrainStep"), "deeplab": ("deeplab", "SegTrainStep")}
_MODELS = {}


def _model(family):
    """A freshly seeded model per family, built once; the tests that change one build their own."""
    if family not in _MODELS:
        _MODELS[family] = _fresh(family)
    return _MODELS[family]


def _fresh(family):
    mod, cls, args = FAMILIES[family][:3]
    torch.manual_seed(0)
    return getattr(importlib.import_module(PKG + mod), cls)(*args)


def _inside(t, arena):
    lo = arena.data_ptr()
    return t.untyped_storage().data_ptr() == arena.untyped_storage().data_ptr() and lo <= t.data_ptr() < lo + max(arena.numel(), 1) * arena.element_size()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_initial_state_dict_is_the_oracles_bit_for_bit(family):
    oracle, oargs, n = FAMILIES[family][3:6]
    sd = _model(family).state_dict()
    ref = importlib.import_module("oracle." + oracle).init_state_dict(*oargs, seed=0)
    assert len(sd) == n and list(sd) == list(ref)
    for k, v in sd.items():
        assert v.shape == ref[k].shape and v.dtype == ref[k].dtype, k
        assert torch.equal(v, ref[k]), k


@pytest.mark.parametrize("family", list(FAMILIES))
def test_arena_sizes(family):
    m = _model(family)
    assert (m._flat["param"].numel(), m._flat["stat"].numel()) == FAMILIES[family][6:8]
    assert m.flat_params is m._flat["param"] and m.flat_stats is m._flat["stat"] and m._flat["grad"] is None


@pytest.mark.parametrize("family", list(FAMILIES))
def test_apply_contract(family):
    m = _fresh(family)
    for cast in (m.double, m.half):
        with pytest.raises(CvxError, match="fp32 master parameters"):
            cast()
    frozen = next(n for n, p in m.named_parameters() if p.requires_grad)
    dict(m.named_parameters())[frozen].requires_grad_(False)
    grads = m.flat_grads                                       # a gradient arena exists before the move
    m._engines["stale"] = object()
    assert m.to("cpu") is m
    arenas = {torch.float32: ("param", "stat"), torch.int64: ("nbt",)}
    outside = [k for k, v in m.state_dict().items() if not any(_inside(v, m._flat[a]) for a in arenas[v.dtype])]
    assert outside == (["model.22.dfl.conv.weight"] if family == "yolov8" else [])     # YOLOv8's constant DFL weight
    for n, p in m.named_parameters():
        assert p.requires_grad == (n != frozen and n not in outside), n
    assert not m._engines and not m._grads_attached
    if family == "yolov8":                                     # the recorded difference: Yolo8 keeps an existing gradient arena
        assert m._flat["grad"] is not None and m._flat["grad"].shape == grads.shape
    else:
        assert m._flat["grad"] is None


@pytest.mark.parametrize("family", list(FAMILIES))
def test_cpu_model_refuses_to_run(family):
    m = _model(family)
    with pytest.raises(CvxError, match=f"{type(m).__name__} runs on an MI355X only") as e:
        m.engine_for(*FAMILIES[family][8])
    assert "no CPU fallback" in str(e.value) and not m._engines


@pytest.mark.parametrize("family", list(FAMILIES))
def test_train_step_constructor(family):
    assert not (torch.distributed.is_available() and torch.distributed.is_initialized())
    mod, cls = STEPS[family]
    m, crit, opt, scaler = _model(family), object(), object(), object()
    step = getattr(importlib.import_module(PKG + mod), cls)(m, crit, opt, scaler=scaler)
    assert step.world == 1 and step.distributed is False
    assert step.model is m and step.criterion is crit and step.optimizer is opt and step.scaler is scaler
