"""DeepLabv3+ (ResNet-101, output stride 16) on the MI355X engine: inference AND training (SURVEY.md section 8 row a19 / (f)2,
BASELINE.json configs[5]).

Mirrors ``core/models/deeplabv3plus.py:10-149`` + ``core/models/resnet.py:82-277`` of the reference as an engine graph:

* every Conv + BatchNorm (+ ReLU) is one convolution launch with the running statistics folded into its epilogue; a
  Bottleneck's ``relu(bn3(conv3) + identity)`` is the same launch (residual added before the activation); the
  downsample branch is Conv + BN without activation;
* layer4 runs dilated (``replace_stride_with_dilation=[False, False, True]``, resnet.py:212-220): its first block keeps
  dilation 1 at stride 1, the other two use dilation 2;
* ASPP (deeplabv3plus.py:43-75): the five branches write into the channel slices of ONE 1280-channel buffer (no
  ``torch.cat``); the three atrous 3x3 convolutions (rates 6, 12, 18) are tap tables of the generic implicit-GEMM kernel; the
  pooling branch is a global average pool, a 1x1 convolution on a 1x1 map and a bilinear resize from 1x1 (= broadcast);
  ``Dropout(0.1)`` is the identity in eval mode;
* decoder (deeplabv3plus.py:78-123): the 48-channel low-level projection and the bilinearly resized ASPP output (33 -> 129
  at 513 input, ``align_corners=False``) land in the two slices of one 304-channel buffer; the classifier's 1x1 (+bias)
  writes fp32 logits rows, which one last kernel resizes to the input resolution as the reference's NCHW tensor.

Parameters and statistics are views of flat arenas (arena.py); ``state_dict`` has the reference's 674 keys and
shapes in its order and is bit-identical to ``DeeplabV3Plus(num_classes, 16, pretrained_backbone=False)`` under the same
global seed.

Training (``model.train()``): the same graph with batch-statistics BatchNorm (bn_act.hip: ReLU / linear passes, the Bottleneck
residual inside the activation), ``Dropout(0.1)`` as an engine op with a counter-based mask, the backward of every op
(data gradients incl. the dilated and the 1x1 stride-2 convolutions, weight gradients, 3x3 max pool, global average pool,
bilinear resizes) and ``SegLoss`` (csrc/loss_seg.hip: upsampling + focal / cross-entropy loss + gradient down to the logits rows
in three launches).  ``SegTrainStep`` is the reference's ``train_loop`` (segmentation_trainer.py:114-131) as C-ABI calls.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch
import torch.nn as nn

from . import _lib as L
from .arena import ArenaLayout, ArenaModel, EngineTrainStep
from .graph import Graph

LAYERS = (3, 4, 23, 3)                            # resnet101 (resnet.py:272-277)
PLANES = (64, 128, 256, 512)
ASPP_RATES = (6, 12, 18)                          # output stride 16 (deeplabv3plus.py:134-136)
ASPP_OUT = 256
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _blocks():
    """ResNet._make_layer (resnet.py:190-232) for resnet101 with replace_stride_with_dilation = [False, False, True] as data:
    [(prefix, inplanes, width, outplanes, stride, dilation, has_downsample)] in module order."""
    out, inplanes, dilation = [], 64, 1
    for li, (planes, n, stride, dilate) in enumerate(zip(PLANES, LAYERS, (1, 2, 2, 2), (False, False, False, True))):
        prev = dilation
        if dilate:
            dilation *= stride
            stride = 1
        for b in range(n):
            first = b == 0
            out.append(dict(prefix=f"backbone.layer{li + 1}.{b}", cin=inplanes, width=planes, cout=planes * 4, stride=stride if first else 1,
                            dil=prev if first else dilation, down=first and (stride != 1 or inplanes != planes * 4), layer=li + 1))
            inplanes = planes * 4
    return out


class DeepLabLayout(ArenaLayout):
    """Arena offsets for every tensor of the reference's DeeplabV3Plus ``state_dict`` (same keys, shapes, order)."""

    def __init__(self, nc: int = 21):
        super().__init__()
        self.nc = nc
        self.nc_pad = (nc + 7) & ~7
        self.blocks = _blocks()
        self._plan()
        self._finish()

    def _plan(self):
        """state_dict order = module registration order (a Bottleneck's downsample comes after its bn3, resnet.py:118-119)."""
        self.conv_bn("backbone.conv1", "backbone.bn1", 64, 3, 7)
        for b in self.blocks:
            p = b["prefix"]
            self.conv_bn(p + ".conv1", p + ".bn1", b["width"], b["cin"], 1)
            self.conv_bn(p + ".conv2", p + ".bn2", b["width"], b["width"], 3)
            self.conv_bn(p + ".conv3", p + ".bn3", b["cout"], b["width"], 1)
            if b["down"]:
                self.conv_bn(p + ".downsample.0", p + ".downsample.1", b["cout"], b["cin"], 1)
        c = "classifier."
        self.conv_bn(c + "project.0", c + "project.1", 48, 256, 1)
        self.conv_bn(c + "aspp.convs.0.0", c + "aspp.convs.0.1", ASPP_OUT, 2048, 1)
        for i in range(3):
            self.conv_bn(c + f"aspp.convs.{i + 1}.0", c + f"aspp.convs.{i + 1}.1", ASPP_OUT, 2048, 3)
        self.conv_bn(c + "aspp.convs.4.1", c + "aspp.convs.4.2", ASPP_OUT, 2048, 1)
        self.conv_bn(c + "aspp.project.0", c + "aspp.project.1", ASPP_OUT, 5 * ASPP_OUT, 1)
        self.conv_bn(c + "classifier.0", c + "classifier.1", 256, 304, 3)
        self.conv(c + "classifier.3", self.nc, 256, 1, bias=True)

    # the order in which the reference CONSTRUCTS its convolutions (each draws its default init from the global RNG):
    # _make_layer builds a layer's downsample before its first block (resnet.py:205-216)
    def construction_order(self, part):
        keys = []
        if part == "backbone":
            keys.append("backbone.conv1")
            for b in self.blocks:
                p = b["prefix"]
                if b["down"]:
                    keys.append(p + ".downsample.0")
                keys += [p + ".conv1", p + ".conv2", p + ".conv3"]
        else:
            c = "classifier."
            keys += [c + "project.0", c + "aspp.convs.0.0", c + "aspp.convs.1.0", c + "aspp.convs.2.0", c + "aspp.convs.3.0", c + "aspp.convs.4.1",
                     c + "aspp.project.0", c + "classifier.0", c + "classifier.3"]
        return keys

    def module_order(self, part):
        return [k for k in self.convs if k.startswith(part)]


def conv_out(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def build_deeplab_graph(lay: DeepLabLayout, H: int, W: int, dropout_p: float = 0.1) -> Graph:
    """Buffer plan + op list for an (H, W) input (any size from 33 up: the reference runs 513 x 513).  Every convolution but the
    first carries its data gradient, so the one graph serves eval and training forwards."""
    if H < 33 or W < 33:
        raise ValueError("input height/width must be at least 33")
    g = Graph()

    def buf(h, w, ch, kind=L.BUF_ACT_F16):
        g.bufs.append((h, w, ch, kind))
        return len(g.bufs) - 1

    def V(b, off, ch, pix=0):
        return (b, off, ch, pix)

    def conv(ckey, vin, vout, hin, win, stride=1, dil=1, act=L.ACT_BN_RELU, res=None):
        s = lay.convs[ckey]
        k = s["k"]
        pad = dil * (k // 2)
        ho, wo = conv_out(hin, k, stride, pad, dil), conv_out(win, k, stride, pad, dil)
        op = dict(type=L.OP_CONV, name=ckey, out=vout, ih=hin, iw=win, oh=ho, ow=wo, k=k, stride=stride, pad=pad, dil=dil, act=act,
                  needs_dgrad=0 if ckey == "backbone.conv1" else 1,
                  w_cin=s["cin"], w_off=s["w_off"], gamma_off=s.get("gamma_off", 0), beta_off=s.get("beta_off", 0), bias_off=s.get("bias_off", 0),
                  rmean_off=s.get("rmean_off", 0), rvar_off=s.get("rvar_off", 0), flags=L.OPF_RES_PRE_ACT if res is not None else 0)
        op["in"] = vin
        if res is not None:
            op["res"] = res
        g.ops.append(op)
        return ho, wo

    def simple(kind, name, vin, vout, ih, iw, oh, ow):
        op = dict(type=kind, name=name, out=vout, ih=ih, iw=iw, oh=oh, ow=ow)
        op["in"] = vin
        g.ops.append(op)

    img = buf(H, W, 8)
    g.image_buf = img
    h1, w1 = conv_out(H, 7, 2, 3, 1), conv_out(W, 7, 2, 3, 1)
    c1 = buf(h1, w1, 64)
    conv("backbone.conv1", V(img, 0, 8), V(c1, 0, 64), H, W, stride=2)
    h, w = (h1 - 1) // 2 + 1, (w1 - 1) // 2 + 1
    cur = V(buf(h, w, 64), 0, 64)
    simple(L.OP_MAXPOOL3S2, "backbone.maxpool", V(c1, 0, 64), cur, h1, w1, h, w)
    low = None
    for b in lay.blocks:                                         # Bottleneck.forward (resnet.py:121-143)
        p, s, d = b["prefix"], b["stride"], b["dil"]
        ho, wo = conv_out(h, 3, s, d, d), conv_out(w, 3, s, d, d)
        t1, t2 = V(buf(h, w, b["width"]), 0, b["width"]), V(buf(ho, wo, b["width"]), 0, b["width"])
        out = V(buf(ho, wo, b["cout"]), 0, b["cout"])
        conv(p + ".conv1", cur, t1, h, w)
        conv(p + ".conv2", t1, t2, h, w, stride=s, dil=d)
        if b["down"]:
            ident = V(buf(ho, wo, b["cout"]), 0, b["cout"])
            conv(p + ".downsample.0", cur, ident, h, w, stride=s, act=L.ACT_BN_LINEAR)
        else:
            ident = cur
        conv(p + ".conv3", t2, out, ho, wo, res=ident)
        cur, h, w = out, ho, wo
        if b["layer"] == 1:
            low, lh, lw = cur, h, w                              # "low_level": the output of layer1 (resnet.py:245-246)

    # ASPP (deeplabv3plus.py:43-75) -> five slices of one buffer
    c = "classifier."
    cat = buf(h, w, 5 * ASPP_OUT)
    conv(c + "aspp.convs.0.0", cur, V(cat, 0, ASPP_OUT), h, w)
    for i, r in enumerate(ASPP_RATES):
        conv(c + f"aspp.convs.{i + 1}.0", cur, V(cat, (i + 1) * ASPP_OUT, ASPP_OUT), h, w, dil=r)
    pooled, pconv = V(buf(1, 1, 2048), 0, 2048), V(buf(1, 1, ASPP_OUT), 0, ASPP_OUT)
    simple(L.OP_AVGPOOL, c + "aspp.convs.4.0", cur, pooled, h, w, 1, 1)
    conv(c + "aspp.convs.4.1", pooled, pconv, 1, 1)
    simple(L.OP_RESIZE, c + "aspp.convs.4.up", pconv, V(cat, 4 * ASPP_OUT, ASPP_OUT), 1, 1, h, w)
    proj = V(buf(h, w, ASPP_OUT), 0, ASPP_OUT)
    conv(c + "aspp.project.0", V(cat, 0, 5 * ASPP_OUT), proj, h, w)
    aspp = V(buf(h, w, ASPP_OUT), 0, ASPP_OUT)
    g.ops.append(dict(type=L.OP_DROPOUT, name=c + "aspp.project.3", out=aspp, ih=h, iw=w, oh=h, ow=w, k=int(round(dropout_p * 65536))))
    g.ops[-1]["in"] = proj                                        # nn.Dropout(0.1) (deeplabv3plus.py:67): identity in eval
    # decoder (deeplabv3plus.py:113-123): [low-level 48 | resized ASPP 256]
    dec = buf(lh, lw, 48 + ASPP_OUT)
    conv(c + "project.0", low, V(dec, 0, 48), lh, lw)
    simple(L.OP_RESIZE, c + "aspp.up", aspp, V(dec, 48, ASPP_OUT), h, w, lh, lw)
    hid = V(buf(lh, lw, 256), 0, 256)
    conv(c + "classifier.0", V(dec, 0, 48 + ASPP_OUT), hid, lh, lw)
    pred = buf(lh * lw, 1, lay.nc_pad, L.BUF_PRED_F32)
    g.pred_buf = pred
    conv(c + "classifier.3", hid, V(pred, 0, lay.nc_pad, 0), lh, lw, act=L.ACT_BIAS)
    g.level_hw = [(lh, lw)]
    g.anchors = lh * lw
    return g


class DeepLabV3PlusR101(ArenaModel):
    """``DeeplabV3Plus(num_classes, output_stride=16, pretrained_backbone=False)`` of the reference (deeplabv3plus.py:126-149)
    on the engine: ``model(x)`` returns the (B, num_classes, H, W) fp32 logits; in training mode (grad enabled) the tensor is
    connected to the engine's backward pass, and carries the low-resolution rows as ``.rows`` for the fused ``SegLoss``."""

    bn_eps_momentum = (BN_EPS, BN_MOMENTUM)

    def __init__(self, num_classes: int = 21, loss_scale: float = 65536.0, dropout_p: float = 0.1):
        # loss_scale: torch.cuda.amp.GradScaler's initial scale (the reference trains under AMP)
        super().__init__(DeepLabLayout(num_classes), num_classes, loss_scale)
        self.dropout_p = float(dropout_p)            # aspp.project.3 = nn.Dropout(0.1); 0 disables it (parity tests)
        self.seed = 0                                # seed of the dropout masks (cvx_engine_set_seed)
        self.last_rows = None

    def ctor_args(self):
        return dict(super().ctor_args(), dropout_p=self.dropout_p)

    def _build_graph(self, h, w):
        return build_deeplab_graph(self.layout, h, w, self.dropout_p)

    def _engine_key(self, h, w, dev):
        return (h, w, dev, self.dropout_p)

    def _after_bind(self, eng):
        eng.set_seed(self.seed)

    def _check_input(self, x, training):
        super()._check_input(x, training)
        if training and x.shape[0] < 2:
            raise ValueError("training-mode BatchNorm needs more than one value per channel (ASPPPooling's 1x1 map): batch >= 2")

    def _init_like_reference(self):
        """The reference's RNG consumption, draw for draw (resnet.py:150-178, deeplabv3plus.py:99-110): every nn.Conv2d draws its
        default init when it is constructed (weight, then bias) -- a layer's downsample before its first block --; then ResNet
        re-initialises its convolutions with kaiming_normal_(fan_out, relu) in module order; then the head is constructed and
        re-initialises its convolution WEIGHTS with kaiming_normal_ (fan_in) in module order: the classifier's bias keeps the
        value drawn at construction."""
        lay = self.layout
        sd = dict(self.named_parameters())
        sd.update(dict(self.named_buffers()))

        def default_init(key):
            sl = lay.slots[key + ".weight"]
            w = torch.empty(sl.shape)
            nn.init.kaiming_uniform_(w, a=math.sqrt(5))
            sd[key + ".weight"].copy_(w)
            if "bias_off" in lay.convs[key]:
                bound = 1.0 / math.sqrt(sl.shape[1] * sl.shape[2] * sl.shape[3])
                bb = torch.empty(lay.slots[key + ".bias"].shape)
                nn.init.uniform_(bb, -bound, bound)
                sd[key + ".bias"].copy_(bb)

        with torch.no_grad():
            for key in lay.construction_order("backbone"):
                default_init(key)
            for key in lay.module_order("backbone"):
                w = torch.empty(lay.slots[key + ".weight"].shape)
                nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")
                sd[key + ".weight"].copy_(w)
            for key in lay.construction_order("classifier"):
                default_init(key)
            for key in lay.module_order("classifier"):
                w = torch.empty(lay.slots[key + ".weight"].shape)
                nn.init.kaiming_normal_(w)
                sd[key + ".weight"].copy_(w)
            for key, sl in lay.slots.items():
                stem, leaf = key.rsplit(".", 1)
                if (stem + ".running_mean") in lay.slots:
                    if leaf in ("weight", "running_var"):
                        sd[key].fill_(1.0)
                    elif leaf in ("bias", "running_mean"):
                        sd[key].zero_()
            self._flat["nbt"].zero_()

    def forward_rows(self, x: torch.Tensor) -> torch.Tensor:
        """(B,3,H,W) -> the engine's fp32 logits rows (B, h*w, nc_pad) at the decoder's resolution (stride 4)."""
        return self._run_forward(x, self.training)

    def rows_to_nchw(self, rows: torch.Tensor, H: int, W: int) -> torch.Tensor:
        """F.interpolate(classifier(features), size=(H, W), mode="bilinear", align_corners=False) (deeplabv3plus.py:147)."""
        B = rows.shape[0]
        lh, lw = self._last_engine.graph.level_hw[0]
        out = torch.empty(B, self.num_classes, H, W, dtype=torch.float32, device=rows.device)
        lib = L.load()
        L.check(lib.cvx_resize_bilinear_rows_to_nchw(L.ptr(rows), self.layout.nc_pad, B, self.num_classes, lh, lw, H, W, L.ptr(out),
                                                      L.stream_ptr(rows.device)), "cvx_resize_bilinear_rows_to_nchw")
        return out

    def backward_rows(self, dpred_f16: torch.Tensor, loss_scale: float):
        """Engine backward from loss_scale * dLoss/drows (B, h*w, nc_pad) fp16: parameter gradients are accumulated into the arena."""
        self._engine_backward(dpred_f16, loss_scale)

    def _backward_from_nchw(self, g: torch.Tensor):
        """Gradient w.r.t. the full-resolution logits -> rows (adjoint of the final resize) -> engine backward."""
        B, nc, H, W = g.shape
        lh, lw = self._last_engine.graph.level_hw[0]
        dpred = torch.empty(B, lh * lw, self.layout.nc_pad, dtype=torch.float16, device=g.device)
        lib = L.load()
        L.check(lib.cvx_resize_bilinear_nchw_grad_to_rows(L.ptr(g.contiguous().float()), B, nc, lh, lw, H, W, self.loss_scale, L.ptr(dpred),
                                                           self.layout.nc_pad, L.stream_ptr(g.device)), "cvx_resize_bilinear_nchw_grad_to_rows")
        self.backward_rows(dpred, self.loss_scale)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, _, H, W = x.shape
        if self.training and torch.is_grad_enabled():
            out = _SegFn.apply(x, self._anchor, self)
        else:
            self.last_rows = self._run_forward(x, self.training)
            out = self.rows_to_nchw(self.last_rows, H, W)
        out.rows, out.model = self.last_rows, self     # the fused loss starts from the low-resolution rows
        return out


class _SegFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, anchor, model):
        ctx.model = model
        ctx.set_materialize_grads(False)      # the fused SegLoss hands no gradient to the logits: then there is nothing to do here
        rows = model._run_forward(images, training=True)
        model.last_rows = rows
        return model.rows_to_nchw(rows, int(images.shape[2]), int(images.shape[3]))

    @staticmethod
    def backward(ctx, g):
        if g is not None:
            ctx.model._backward_from_nchw(g)
        return None, None, None


class _SegLossFn(torch.autograd.Function):
    """loss = SegLoss(rows, target) with the gradient taken by the fused kernel; ``.backward()`` runs the engine's backward."""

    @staticmethod
    def forward(ctx, logits, owner, rows, model, target, hw):
        loss, dpred = owner.op(rows, target, hw, model.loss_scale)
        ctx.model, ctx.dpred = model, dpred
        model.last_dpred = dpred
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        model = ctx.model
        # d loss is a scalar factor on dpred: fold it into the loss scale the engine divides by (1.0 for loss.backward())
        model.backward_rows(ctx.dpred, model.loss_scale / float(gout))
        return None, None, None, None, None, None


class SegLoss:
    """``FocalLoss()`` / ``nn.CrossEntropyLoss(reduction="mean")`` of ``DeeplabV3PlusA.build_loss`` (segmentation_2d.py:59-64,
    core/loss/focal_loss.py:6-22) on the engine: ``loss = criterion(preds, targets)`` with ``preds = model(images)``.  Value and
    gradient come from ``cvx_seg_criterion_loss`` on the low-resolution rows behind ``preds`` (no autograd tape through the upsampling);
    ``loss.backward()`` then runs the engine's backward pass.

    Options of ``"ce"`` (not in the reference; the same entry, the same fused chain):
    ``class_weights`` (``num_classes`` non-negative floats) and ``label_smoothing`` in [0, 1) are those of
    ``F.cross_entropy(weight=, label_smoothing=, reduction="mean")``; ``ohem=dict(thresh=t, min_kept=m)`` trains on the hard pixels
    only: those whose target probability is below ``t``, and at least the ``m * batch`` pixels with the largest cross-entropy (all
    pixels tied at that rank).  ``last_stats`` is the device tensor (kept pixels, valid pixels, theta_min, sum of target weights) of
    the last call, ``ohem_keys()`` its per-pixel selection keys.  Without an option the criterion runs the option-free kernel.

    ``region=dict(kind="dice" | "tversky", ...)`` (see ``seg_region_defaults``; the same entry again) adds a
    region loss to either loss type, with or without the options: the value is ``base_weight * base + weight * region`` with ``base``
    what the criterion computes without ``region``.  Over the valid pixels of the batch (``per_image``: of each image, then the mean
    over the images), with p the softmax and y the one-hot target: ``T_c = (I_c + smooth) / (I_c + alpha FP_c + beta FN_c + smooth)``,
    ``I = sum p y``, ``FP = sum p (1 - y)``, ``FN = sum (1 - p) y``; the loss is the (``class_weights``-weighted) mean of
    ``(1 - T_c)^gamma`` over the classes, those without a target pixel left out under ``skip_absent``.  Dice is ``alpha = beta = 0.5``.
    ``base_weight = 0`` trains on the region loss alone (the base chain is skipped).  OHEM selects pixels for the base term only.
    ``region_stats`` is the float64 device tensor ``(G, nc, 4)`` = I, P = sum p, Y = sum y, T of the last call (G = batch under
    ``per_image``, else 1).  Data parallel: every rank takes the sums over its own shard, like OHEM and the weighted denominators.

    ``lovasz=dict(weight=1.0, base_weight=1.0, per_image=False, skip_absent=True, class_weights=None)`` (see ``seg_lovasz_defaults``;
    not together with ``region=``) adds the Lovasz-Softmax loss (Berman et al., CVPR 2018), the surrogate of the mean IoU, in the same
    way: the value is ``base_weight * base + weight * lovasz``, the keys mean what they mean under ``region=``, ``skip_absent=True`` is
    the paper's ``classes="present"`` and ``False`` its ``"all"``.  Per group and class the errors ``e = [t == c] ? 1 - p_c : p_c`` of
    the valid pixels are sorted on the device (descending, ties by ascending pixel index) and weighted by the Lovasz extension's
    increments of the Jaccard loss along that order; the rules are in ``include/cvx_engine.h``.  ``region_stats`` is then
    ``(G, nc, 4)`` = 0, 0, Y_c, L_c, and ``lovasz_sorted()`` shows the order.  The sort's two ping-pong buffers of key + payload take
    ``2 * 8`` bytes per pixel and class -- 1.4 GB of workspace at batch 16, 513 x 513 labels and 21 classes, next to the gradient
    plane's 0.35 GB.  Data parallel: every rank sorts its own shard."""

    def __init__(self, loss_type: str = "focal", alpha: float = 0.25, gamma: float = 2.0, ignore_index: int = -100, check_targets: bool = True,
                 class_weights=None, label_smoothing: float = 0.0, ohem=None, region=None, lovasz=None):
        if loss_type not in ("focal", "ce"):
            raise ValueError("loss_type must be 'focal' or 'ce' (segmentation_2d.py:59-64)")
        self.mode = 0 if loss_type == "focal" else 1
        self.alpha, self.gamma, self.ignore_index = float(alpha), float(gamma), int(ignore_index)
        self.check_targets = check_targets           # False: skip the host check of the bad-label flag (no sync in the step)
        self._ws = self._ws_eval = None
        self._dpred = None
        self._bad = None
        self.class_weights = self.ohem = None
        self.label_smoothing = float(label_smoothing)
        self.last_stats = None
        self._weights_dev = self._keys_shape = None
        if region is not None and lovasz is not None:
            raise ValueError("region= and lovasz= exclude each other: a criterion has one region term")
        self.region = seg_region_defaults(**region) if region is not None else None
        self.has_region = self.region is not None
        self.lovasz = seg_lovasz_defaults(**lovasz) if lovasz is not None else None
        self.has_lovasz = self.lovasz is not None
        self._lovasz_view = None
        self.region_stats = None
        self._region_weights_dev = None
        self.has_options = class_weights is not None or self.label_smoothing != 0.0 or ohem is not None
        if not self.has_options:
            return
        if self.mode == 0:
            raise ValueError("class_weights, label_smoothing and ohem are options of loss_type='ce', not of 'focal'")
        if class_weights is not None:
            w = torch.as_tensor(class_weights, dtype=torch.float32).detach().cpu().reshape(-1).clone()
            if w.numel() == 0 or not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or not bool((w > 0).any()):
                raise ValueError("class_weights must be finite, non-negative and not all zero")
            self.class_weights = w
        if not 0.0 <= self.label_smoothing < 1.0:          # nan fails too
            raise ValueError("label_smoothing must lie in [0, 1)")
        if ohem is not None:
            thresh, min_kept = float(ohem["thresh"]), ohem["min_kept"]
            if not 0.0 < thresh <= 1.0:
                raise ValueError("ohem: thresh must lie in (0, 1]")
            if int(min_kept) != min_kept or int(min_kept) < 1:
                raise ValueError("ohem: min_kept must be an integer >= 1")
            self.ohem = {"thresh": thresh, "min_kept": int(min_kept)}
            self.ohem_theta = abs(math.log(thresh))         # -ln thresh as a host double (abs: thresh = 1 gives +0.0); fp32 at the call

    def bad_targets(self) -> bool:
        """True when the last call saw a label that is neither ignore_index nor a class (synchronises)."""
        return self._bad is not None and int(self._bad.item()) != 0

    def weights_on(self, device, nc: int):
        """The class weights on ``device`` (copied once), or None; their length is checked against ``nc`` here, where it is known."""
        if self.class_weights is None:
            return None
        if self.class_weights.numel() != nc:
            raise ValueError(f"class_weights has {self.class_weights.numel()} entries for {nc} classes")
        if self._weights_dev is None or self._weights_dev.device != device:
            self._weights_dev = self.class_weights.to(device)
        return self._weights_dev

    def ohem_keys(self) -> torch.Tensor:
        """(B, H, W) fp32 view of the last call's selection keys, max(lse - z_t, 0), with -1 at pixels that are not valid.  A view of
        the workspace: the next call overwrites it.  Does not synchronise."""
        if self.ohem is None or self._keys_shape is None:
            raise L.CvxError("ohem_keys: the criterion has no ohem option, or has not been called yet")
        B, H, W = self._keys_shape
        o = L.SEG_OPTS_KEY_OFFSET                          # the same offset whatever else the criterion holds
        return self._ws[o:o + B * H * W * 4].view(torch.float32).view(B, H, W)

    def lovasz_sorted(self):
        """``(keys, payload, segments)`` of the last training call, views of the workspace that the next call overwrites: ``keys``
        uint32 (the fp32 bit patterns of the errors, sorted descending inside each segment), ``payload`` uint32 (the pixel's linear
        index inside its group in bits 0..30, the foreground flag ``t == c`` in bit 31) and ``segments`` ``(G, nc, 2)`` int64 = element
        offset into both arrays and length (the group's valid pixels; 0 for a class the sort skipped: one without a target pixel under
        ``skip_absent``).  A debugging and test surface, like ``ohem_keys()``.  Does not synchronise."""
        if not self.has_lovasz or self._lovasz_view is None:
            raise L.CvxError("lovasz_sorted: the criterion has no lovasz term, or has not been called yet")
        (groups, nc, ng), (okey, opay, oseg) = self._lovasz_view
        n = groups * nc * ng
        keys = self._ws[okey:okey + n * 4].view(torch.uint32)
        payload = self._ws[opay:opay + n * 4].view(torch.uint32)
        return keys, payload, self._ws[oseg:oseg + groups * nc * 16].view(torch.int64).view(groups, nc, 2)

    def _criterion_struct(self, dev, nc: int, batch: int) -> L.SegCriterion:
        """``cvx_seg_criterion`` of this criterion for ``nc`` classes and ``batch`` images, its weights on ``dev`` (copied once; their
        lengths are checked here, where ``nc`` is known).  ``base_weight = 0`` drops the base term and its options with it."""
        r = self.region if self.region is not None else self.lovasz
        with_base = r is None or r["base_weight"] > 0.0
        c = L.SegCriterion(base=(1 if self.mode == 0 else 2) if with_base else 0, focal_alpha=self.alpha, focal_gamma=self.gamma,
                           ignore_index=self.ignore_index, ohem_theta=-1.0, region=2 if self.has_lovasz else int(r is not None))
        if with_base and self.has_options:
            weights = self.weights_on(dev, nc)
            c.class_weight = weights.data_ptr() if weights is not None else None
            c.label_smoothing = self.label_smoothing
            if self.ohem is not None:
                c.ohem_theta, c.ohem_min_kept = self.ohem_theta, self.ohem["min_kept"] * batch
        if r is not None:
            rw = r["class_weights"]
            if rw is not None:
                if rw.numel() != nc:
                    raise ValueError(f"{'lovasz' if self.has_lovasz else 'region'} class_weights has {rw.numel()} entries for {nc} classes")
                if self._region_weights_dev is None or self._region_weights_dev.device != dev:
                    self._region_weights_dev = rw.to(dev)
                c.region_class_weight = self._region_weights_dev.data_ptr()
            c.base_weight, c.weight = r["base_weight"], r["weight"]
            if not self.has_lovasz:
                c.alpha, c.beta, c.gamma, c.smooth = (r[k] for k in ("alpha", "beta", "gamma", "smooth"))
            c.per_image, c.skip_absent = int(r["per_image"]), int(r["skip_absent"])
        return c

    def _ensure_buffers(self, lib, dev, dims: L.SegDims, crit: L.SegCriterion, for_eval: bool = False) -> torch.Tensor:
        """The workspace of this call (training and validation each keep their own), with the bad-label flag, ``last_stats`` (a
        criterion with options or a region / Lovasz term) and ``region_stats`` (one with such a term) next to it: allocated by the first call of a shape and kept."""
        need = int(lib.cvx_seg_criterion_workspace_bytes(C.byref(dims), C.byref(crit), int(for_eval)))
        if need <= 0:
            raise L.CvxError("cvx_seg_criterion_workspace_bytes: bad sizes, or a criterion the library refuses")
        name = "_ws_eval" if for_eval else "_ws"
        ws = getattr(self, name)
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            setattr(self, name, ws)
        if self._bad is None or self._bad.device != dev:
            self._bad = torch.zeros(1, dtype=torch.int32, device=dev)
        has_term = self.has_region or self.has_lovasz
        if (self.has_options or has_term) and (self.last_stats is None or self.last_stats.device != dev):   # zeros without an option
            self.last_stats = torch.zeros(4, dtype=torch.float64, device=dev)
        shape = (dims.batch if crit.per_image else 1, dims.nc, 4)
        if has_term and (self.region_stats is None or self.region_stats.device != dev or tuple(self.region_stats.shape) != shape):
            self.region_stats = torch.zeros(shape, dtype=torch.float64, device=dev)
        return ws

    def op(self, rows: torch.Tensor, target: torch.Tensor, hw, loss_scale: float, dpred: Optional[torch.Tensor] = None,
           check: Optional[bool] = None):
        """rows (B, lh*lw, ld) fp32, target (B, H, W) int64, hw = (lh, lw) -> (loss (1,), dpred (B, lh*lw, ld) fp16)."""
        if rows.device.type != "cuda":
            raise L.CvxError("SegLoss runs on an MI355X only (there is no CPU path)")
        lib, dev = L.load(), rows.device
        B, A, ld = rows.shape
        if target.dim() != 3 or target.shape[0] != B:
            raise ValueError("targets must have shape (B, H, W)")
        nc = getattr(self, "nc", None) or ld
        target = target.to(device=dev, dtype=torch.long).contiguous()
        dims = L.SegDims(ld, B, nc, int(hw[0]), int(hw[1]), int(target.shape[1]), int(target.shape[2]))
        crit = self._criterion_struct(dev, nc, B)
        ws = self._ensure_buffers(lib, dev, dims, crit)
        if dpred is None:
            dpred = torch.empty(B, A, ld, dtype=torch.float16, device=dev)
        loss = torch.empty(1, device=dev)                   # a block of the caching allocator, no device allocation
        with torch.cuda.device(dev):
            L.check(lib.cvx_seg_criterion_loss(L.ptr(rows), C.byref(dims), L.ptr(target), C.byref(crit), float(loss_scale), L.ptr(loss), L.ptr(dpred),
                                               L.ptr(self._bad), L.ptr(self.last_stats), L.ptr(self.region_stats), L.ptr(ws), L.stream_ptr(dev)),
                    "cvx_seg_criterion_loss")
        if crit.ohem_theta >= 0.0:
            self._keys_shape = (B, dims.oh, dims.ow)
        if self.has_lovasz:
            groups = B if crit.per_image else 1
            key = (groups, nc, (B // groups) * dims.oh * dims.ow)
            if self._lovasz_view is None or self._lovasz_view[0] != key:
                offs = (C.c_int64 * 3)()
                L.check(lib.cvx_seg_criterion_lovasz_view(C.byref(dims), C.byref(crit), offs), "cvx_seg_criterion_lovasz_view")
                self._lovasz_view = (key, tuple(int(o) for o in offs))
        if (self.check_targets if check is None else check) and self.bad_targets():
            raise L.CvxError("SegLoss: a target label is neither ignore_index nor in [0, num_classes)")
        return loss, dpred

    def __call__(self, preds: torch.Tensor, targets: torch.Tensor):
        rows, model = getattr(preds, "rows", None), getattr(preds, "model", None)
        if rows is None or model is None:
            raise L.CvxError("SegLoss needs the output of DeepLabV3PlusR101.forward (it carries the logits rows the loss starts from)")
        self.nc = model.num_classes
        hw = model._last_engine.graph.level_hw[0]
        if model.training and torch.is_grad_enabled():
            return _SegLossFn.apply(preds, self, rows, model, targets, hw)
        return self.op(rows, targets, hw, model.loss_scale)[0].reshape(())


_REGION_KEYS = ("kind", "weight", "base_weight", "alpha", "beta", "gamma", "smooth", "per_image", "skip_absent", "class_weights")


def seg_region_defaults(kind: str = "dice", **kw) -> dict:
    """The filled-in ``region=`` dict of ``SegLoss``: ``kind`` "dice" (alpha = beta = 0.5, fixed) or "tversky" (alpha 0.3, beta 0.7 by
    default), ``weight`` 1, ``base_weight`` 1, ``gamma`` 1 (another value: focal Tversky), ``smooth`` 1, ``per_image`` False,
    ``skip_absent`` True, ``class_weights`` None.  Raises ``ValueError`` for an unknown kind or key and for a value outside its range."""
    if kind not in ("dice", "tversky"):
        raise ValueError("region: kind must be 'dice' or 'tversky'")
    unknown = sorted(set(kw) - set(_REGION_KEYS))
    if unknown:
        raise ValueError(f"region: unknown keys {unknown}")
    if kind == "dice":
        if any(kw.get(k) is not None and float(kw[k]) != 0.5 for k in ("alpha", "beta")):
            raise ValueError("region: kind 'dice' is alpha = beta = 0.5; use kind 'tversky' for other values")
        a, b = 0.5, 0.5
    else:
        a = 0.3 if kw.get("alpha") is None else float(kw["alpha"])
        b = 0.7 if kw.get("beta") is None else float(kw["beta"])

    def num(key, default):
        return default if kw.get(key) is None else float(kw[key])

    r = {"kind": kind, "weight": num("weight", 1.0), "base_weight": num("base_weight", 1.0), "alpha": a, "beta": b, "gamma": num("gamma", 1.0),
         "smooth": num("smooth", 1.0), "per_image": bool(kw.get("per_image", False)),
         "skip_absent": True if kw.get("skip_absent") is None else bool(kw["skip_absent"]), "class_weights": None}
    if not all(math.isfinite(r[k]) for k in ("weight", "base_weight", "alpha", "beta", "gamma", "smooth")):
        raise ValueError("region: every value must be finite")
    if r["weight"] <= 0 or r["base_weight"] < 0 or r["alpha"] < 0 or r["beta"] < 0 or r["gamma"] <= 0 or r["smooth"] < 0:
        raise ValueError("region: weight > 0, base_weight >= 0, alpha >= 0, beta >= 0, gamma > 0 and smooth >= 0")
    if kw.get("class_weights") is not None:
        w = torch.as_tensor(kw["class_weights"], dtype=torch.float32).detach().cpu().reshape(-1).clone()
        if w.numel() == 0 or not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or not bool((w > 0).any()):
            raise ValueError("region: class_weights must be finite, non-negative and not all zero")
        r["class_weights"] = w
    return r


_LOVASZ_KEYS = ("weight", "base_weight", "per_image", "skip_absent", "class_weights")


def seg_lovasz_defaults(**kw) -> dict:
    """The filled-in ``lovasz=`` dict of ``SegLoss``: ``weight`` 1, ``base_weight`` 1 (0: the Lovasz term alone), ``per_image`` False,
    ``skip_absent`` True (the paper's ``classes="present"``), ``class_weights`` None.  Raises ``ValueError`` for an unknown key and for
    a value outside its range."""
    unknown = sorted(set(kw) - set(_LOVASZ_KEYS))
    if unknown:
        raise ValueError(f"lovasz: unknown keys {unknown}")
    r = {"weight": 1.0 if kw.get("weight") is None else float(kw["weight"]),
         "base_weight": 1.0 if kw.get("base_weight") is None else float(kw["base_weight"]), "per_image": bool(kw.get("per_image", False)),
         "skip_absent": True if kw.get("skip_absent") is None else bool(kw["skip_absent"]), "class_weights": None}
    if not (math.isfinite(r["weight"]) and math.isfinite(r["base_weight"])):
        raise ValueError("lovasz: every value must be finite")
    if r["weight"] <= 0 or r["base_weight"] < 0:
        raise ValueError("lovasz: weight > 0 and base_weight >= 0")
    if kw.get("class_weights") is not None:
        w = torch.as_tensor(kw["class_weights"], dtype=torch.float32).detach().cpu().reshape(-1).clone()
        if w.numel() == 0 or not bool(torch.isfinite(w).all()) or bool((w < 0).any()) or not bool((w > 0).any()):
            raise ValueError("lovasz: class_weights must be finite, non-negative and not all zero")
        r["class_weights"] = w
    return r


def seg_class_weights(counts, scheme: str = "median_freq") -> torch.Tensor:
    """Class weights for ``SegLoss(class_weights=)`` from per-class pixel counts (e.g. the row sums of the confusion matrix of one
    ``cvx_seg_criterion_eval`` pass over the training loader).  With f the class frequency among the counted pixels: ``"median_freq"`` gives
    median(f over the classes that occur) / f_c, ``"enet"`` 1 / ln(1.02 + f_c); a class with count 0 gets weight 0.  Host only."""
    counts = torch.as_tensor(counts, dtype=torch.float64).reshape(-1)
    if scheme not in ("median_freq", "enet"):
        raise ValueError("scheme must be 'median_freq' or 'enet'")
    if counts.numel() == 0 or bool((counts < 0).any()) or float(counts.sum()) <= 0:
        raise ValueError("counts must be non-negative with a positive sum")
    seen = counts > 0
    f = counts / counts.sum()
    w = torch.zeros_like(f)
    w[seen] = torch.quantile(f[seen], 0.5) / f[seen] if scheme == "median_freq" else 1.0 / torch.log(1.02 + f[seen])
    return w.float()


class SegTrainStep(EngineTrainStep):
    """One optimisation step of the reference's ``DeeplabV3PlusTrainer.train_loop`` (segmentation_trainer.py:114-131:
    zero_grad -> forward -> criterion -> backward -> Adam under AMP) as C-ABI calls: engine forward (training), ``cvx_seg_criterion_loss``,
    engine backward, [gradient all-reduce over RCCL], fused Adam with the inf/nan check of GradScaler.step.  Returns the loss (1,).
    Data parallel: the flat gradient arena is summed over the ranks in a few large slices on a side stream after the backward
    pass (the mean's 1/world is folded into Adam); BatchNorm statistics stay per rank, as in the reference."""

    _pred = _dpred = None

    def __call__(self, images: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        m, crit = self.model, self.criterion
        scale = self._begin()
        B, _, H, W = images.shape
        eng = m.engine_for(H, W)
        lh, lw = eng.graph.level_hw[0]
        if self._pred is None or self._pred.shape[0] != B or self._pred.shape[1] != lh * lw:
            dev = m.flat_params.device
            self._pred = torch.empty(B, lh * lw, m.layout.nc_pad, device=dev)
            self._dpred = torch.empty(B, lh * lw, m.layout.nc_pad, device=dev, dtype=torch.float16)
        rows = m._run_forward(images, True, self._pred)
        crit.nc = m.num_classes
        loss, dpred = crit.op(rows, targets, (lh, lw), scale, self._dpred, check=False)   # no host sync in the step: crit.bad_targets() polls
        self._backward(eng, dpred, scale)
        self._update()
        return loss
