"""``Yolo8``: the reference's model object contract on top of the MI355X engine.

What callers of the reference rely on and is kept here:
* ``nn.Module`` whose ``state_dict`` has the reference's 355 keys / shapes / order for scale "n"
  (``model.<i>...``; core/models/yolov8/yolo_v8.py:16-62), so reference ``.pth`` files load;
* ``model.model[-1]`` exposes ``stride``, ``nc``, ``no``, ``reg_max`` (read by the loss,
  core/algorithms/yolo_v8.py:32-45);
* ``model.train()`` forward returns three NCHW tensors ``(B, nc+64, H/8.., W/8..)``; ``model.eval()``
  forward returns ``(y (B, 4+nc, A), [those three])`` (core/models/yolov8/modules.py:428-446);
* random init equals the reference constructor's under the same global seed (weights drawn in module
  construction order, BN buffers after the constructor's stride probe, Detect.bias_init).

What differs underneath: the sub-modules hold no compute.  Every tensor is a strided view of the flat
arenas and ``forward`` runs the whole graph through ``cvx_engine_forward`` (arena.py describes the
plumbing all model families share); autograd sees one custom Function whose backward calls
``cvx_engine_backward``.  Where ``Yolo8`` overrides that plumbing, the override says "differs from ArenaModel" and how.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from .arena import ArenaModel, _Holder
from .engine import decode
from .graph import REG_MAX, STRIDES, ParamLayout, build_yolov8_graph

BN_EPS, BN_MOMENTUM = 1e-3, 0.03       # core/models/yolov8/torch_utils.py:17-19


# ---- parameter-only module tree (names = the reference's) ---------------------------------------
class Conv2dParams(_Holder):
    def __init__(self, c1, c2, k, bias):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = c1, c2, (k, k)
        self.weight = nn.Parameter(torch.empty(0))
        if bias:
            self.bias = nn.Parameter(torch.empty(0))
        else:
            self.register_parameter("bias", None)


class BatchNormParams(_Holder):
    def __init__(self, c):
        super().__init__()
        self.num_features, self.eps, self.momentum = c, BN_EPS, BN_MOMENTUM
        self.weight = nn.Parameter(torch.empty(0))
        self.bias = nn.Parameter(torch.empty(0))
        self.register_buffer("running_mean", torch.empty(0))
        self.register_buffer("running_var", torch.empty(0))
        self.register_buffer("num_batches_tracked", torch.empty(0, dtype=torch.long))


class Conv(_Holder):                      # modules.py:19-33
    def __init__(self, c1, c2, k=1, s=1):
        super().__init__()
        self.conv = Conv2dParams(c1, c2, k, bias=False)
        self.bn = BatchNormParams(c2)
        self.stride = s


class Bottleneck(_Holder):                # modules.py:124-135
    def __init__(self, c, shortcut):
        super().__init__()
        self.cv1 = Conv(c, c, 3)
        self.cv2 = Conv(c, c, 3)
        self.add = shortcut


class C2f(_Holder):                       # modules.py:189-202
    def __init__(self, c1, c2, n, shortcut):
        super().__init__()
        self.c = c2 // 2
        self.cv1 = Conv(c1, 2 * self.c, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck(self.c, shortcut) for _ in range(n))


class SPPF(_Holder):                      # modules.py:304-318
    def __init__(self, c1, c2):
        super().__init__()
        self.cv1 = Conv(c1, c1 // 2, 1)
        self.cv2 = Conv((c1 // 2) * 4, c2, 1)


class Upsample(_Holder):
    pass


class Concat(_Holder):
    pass


class DFL(_Holder):                       # modules.py:67-83
    def __init__(self, c1=REG_MAX):
        super().__init__()
        self.conv = Conv2dParams(c1, 1, 1, bias=False)
        self.conv.weight.requires_grad_(False)
        self.c1 = c1


class Detect(_Holder):                    # modules.py:407-455
    def __init__(self, nc, ch, c_box, c_cls):
        super().__init__()
        self.nc, self.nl, self.reg_max = nc, len(ch), REG_MAX
        self.no = nc + 4 * REG_MAX
        self.stride = torch.tensor([float(s) for s in STRIDES])
        self.cv2 = nn.ModuleList(nn.Sequential(Conv(x, c_box, 3), Conv(c_box, c_box, 3), Conv2dParams(c_box, 4 * REG_MAX, 1, True)) for x in ch)
        self.cv3 = nn.ModuleList(nn.Sequential(Conv(x, c_cls, 3), Conv(c_cls, c_cls, 3), Conv2dParams(c_cls, nc, 1, True)) for x in ch)
        self.dfl = DFL(REG_MAX)


class PredList(list):
    """The three NCHW level tensors, plus the fused (B, A, no) tensor they are views/copies of."""
    pred: Optional[torch.Tensor] = None
    level_hw = None


class _EngineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, anchor, model):
        ctx.model = model
        pred = model._run_forward(images, training=True)
        return pred

    @staticmethod
    def backward(ctx, gpred):
        model = ctx.model
        model._run_backward(gpred)
        return None, None, None


class Yolo8(ArenaModel):
    bn_eps_momentum = (BN_EPS, BN_MOMENTUM)
    _bind_grads_in_eval = True       # differs from ArenaModel: the gradient arena is allocated and bound in eval mode too

    def __init__(self, scale_name: str = "n", num_classes: int = 80, ch: int = 3, loss_scale: float = 1024.0):
        if ch != 3:
            raise ValueError("the MI355X engine is built for 3-channel images")
        super().__init__(ParamLayout(scale_name, num_classes), num_classes, loss_scale)
        self.scale_name = scale_name

    def ctor_args(self):
        return dict(super().ctor_args(), scale_name=self.scale_name)

    def _build_graph(self, h, w):
        return build_yolov8_graph(self.layout, h, w)

    # ---- arenas <-> module tree -------------------------------------------------------------------
    def _build_tree(self):
        """differs from ArenaModel: the reference's real module tree (``model.model[-1]`` is read by the loss), not bare holders"""
        lay = self.layout
        c64, c128, c256, c512, c1024 = lay.c64, lay.c128, lay.c256, lay.c512, lay.c1024
        layers = [
            Conv(3, c64, 3, 2), Conv(c64, c128, 3, 2), C2f(c128, c128, lay.n3, True), Conv(c128, c256, 3, 2),
            C2f(c256, c256, lay.n6, True), Conv(c256, c512, 3, 2), C2f(c512, c512, lay.n6, True), Conv(c512, c1024, 3, 2),
            C2f(c1024, c1024, lay.n3, True), SPPF(c1024, c1024),
            Upsample(), Concat(), C2f(c1024 + c512, c512, lay.n3, False),
            Upsample(), Concat(), C2f(c512 + c256, c256, lay.n3, False),
            Conv(c256, c256, 3, 2), Concat(), C2f(c256 + c512, c512, lay.n3, False),
            Conv(c512, c512, 3, 2), Concat(), C2f(c512 + c1024, c1024, lay.n3, False),
            Detect(self.num_classes, lay.head_in, lay.c_box, lay.c_cls),
        ]
        self.model = nn.Sequential(*layers)
        self.stride = self.model[-1].stride

    def _attach_views(self):
        """differs from ArenaModel: ``ParamLayout`` has no ``num_batches_tracked`` slots (they follow the ``BatchNormParams`` modules'
        order), and the constant DFL weight lives outside the arenas"""
        super()._attach_views()
        i_bn = 0
        for mod in self.modules():
            if isinstance(mod, BatchNormParams):
                mod._buffers["num_batches_tracked"] = self._flat["nbt"][i_bn]
                i_bn += 1
        dfl = self.model[-1].dfl.conv
        if dfl.weight.numel() == 0:
            dfl._parameters["weight"] = nn.Parameter(torch.arange(REG_MAX, dtype=torch.float32).view(1, REG_MAX, 1, 1), requires_grad=False)

    def _apply(self, fn, recurse=True):
        """differs from ArenaModel: an existing gradient arena moves with the model (there it is dropped); the constant DFL weight and
        ``stride`` are tensors outside the arenas and move here"""
        grad = self._flat["grad"]
        super()._apply(fn)
        if grad is not None:
            self._flat["grad"] = fn(grad).contiguous()
        dfl = self.model[-1].dfl.conv
        dfl._parameters["weight"] = nn.Parameter(fn(dfl.weight.data), requires_grad=False)
        self.model[-1].stride = fn(self.model[-1].stride)
        self.stride = self.model[-1].stride
        return self

    def _init_like_reference(self):
        """Same draws, same order, as ``get_yolo8_*`` under the caller's global seed
        (yolo_v8.py:26-62 + torch's Conv2d.reset_parameters), then the constructor's side effects."""
        det = self.model[-1]
        with torch.no_grad():
            for mod in self.modules():
                if isinstance(mod, Conv2dParams):
                    k = mod.kernel_size[0]
                    w = torch.empty(mod.out_channels, mod.in_channels, k, k)
                    nn.init.kaiming_uniform_(w, a=math.sqrt(5))
                    if mod.weight.requires_grad:
                        mod.weight.copy_(w)
                    if mod.bias is not None:
                        bound = 1.0 / math.sqrt(mod.in_channels * k * k)
                        b = torch.empty(mod.out_channels)
                        nn.init.uniform_(b, -bound, bound)
                        mod.bias.copy_(b)
                elif isinstance(mod, BatchNormParams):
                    mod.weight.fill_(1.0)
                    mod.bias.zero_()
                    mod.running_mean.zero_()
                    mod.running_var.fill_(0.9)       # stride-probe forward on zeros, momentum 0.1 (yolo_v8.py:53-58)
            self._flat["nbt"].fill_(1)
            for a, b, s in zip(det.cv2, det.cv3, STRIDES):           # Detect.bias_init, modules.py:448-455
                a[-1].bias.fill_(1.0)
                b[-1].bias[:det.nc] = math.log(5 / det.nc / (640 / s) ** 2)

    # ---- engine plumbing ------------------------------------------------------------------------------
    def _run_forward(self, images: torch.Tensor, training: bool, pred: Optional[torch.Tensor] = None) -> torch.Tensor:
        """differs from ArenaModel: returns the reference's (B, A, 64 + nc) as a view of the rows, whose class columns are padded to 8"""
        out = super()._run_forward(images, training, pred)
        no = self.layout.no
        return out if out.shape[2] == no else out[..., :no]

    def _run_backward(self, gpred: torch.Tensor):
        dpred = (gpred * self.loss_scale).to(torch.float16)
        if self.layout.no_pad != self.layout.no:             # the engine reads rows of no_pad values; the padding is zero
            padded = torch.zeros(*dpred.shape[:2], self.layout.no_pad, dtype=torch.float16, device=dpred.device)
            padded[..., :self.layout.no] = dpred
            dpred = padded
        self._engine_backward(dpred.contiguous(), self.loss_scale)

    def level_shapes(self, h: int, w: int):
        return [(h // s, w // s) for s in STRIDES]

    # ---- the reference's forward contract --------------------------------------------------------------
    def forward(self, x: torch.Tensor):
        B, _, H, W = x.shape
        det = self.model[-1]
        if self.training and torch.is_grad_enabled():
            pred = _EngineFn.apply(x, self._anchor, self)
        else:
            pred = self._run_forward(x, training=self.training)
        outs = PredList()
        off = 0
        for (h, w) in self.level_shapes(H, W):
            outs.append(pred[:, off:off + h * w, :].permute(0, 2, 1).reshape(B, det.no, h, w))
            off += h * w
        outs.pred = pred
        outs.level_hw = self.level_shapes(H, W)
        if self.training:
            return outs
        y = decode(pred.detach(), det.nc, outs.level_hw, STRIDES)
        return y, outs


def get_yolo8(model_type: str, nc: int = 80, **kw) -> Yolo8:
    return Yolo8(model_type, nc, **kw)
