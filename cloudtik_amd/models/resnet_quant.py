"""Inference-only bottleneck ResNet with static int8 convolutions (``ops.conv2d_i8_static``,
csrc/quant_conv.hip); the counterpart of ``bert_quant`` for the image classifier.

Built from a trained ``models.resnet.ResNet``.  Every BatchNorm of a quantized stage is folded
into the convolution in front of it (``ops.fold_bn``: fp32 on the host, from the running
statistics), the folded weight is quantized per output channel (``ops.quantize_weight``) and
the BatchNorm shift becomes the convolution's fp32 bias.  A ``QuantBottleneck`` is then at most
four launches -- conv1 + ReLU, conv2 + ReLU, the optional downsample conv, conv3 + residual +
ReLU -- and every one of them writes int8 against the calibrated range of the tensor it
produces, so between the blocks of a quantized stage no bf16 activation exists: the residual
is the block's int8 input (or the int8 downsample output) with its own scale.

``sites`` says which of ``("layer1", "layer2", "layer3", "layer4")`` run in int8.  The stem
(Ci = 3 does not fit the 16-byte channel gather, about 3 % of the FLOPs), the pooling head and
``fc`` stay on the model's own path.  A float tensor entering a quantized stage goes through
``quantize_static``; the last quantized block in front of a float stage or the head emits the
model dtype instead of int8.

Ranges (``act_amax``, from ``calibrate``) are a dict of Python floats keyed ``"stem"`` (the
pooled stem output) and ``"layerL.J.bn1"`` / ``".bn2"`` / ``".down_bn"`` / ``".out"``; a block's
input range is the previous site's (the same tensor, so the same scale).  They reach the kernels
by value and are not part of the state dict, which holds for a quantized block
``<conv>_weight_q`` (int8 [Co, R*S*Ci], tap-major rows), ``<conv>_weight_scale`` (fp32) and
``<conv>_bias`` (fp32) for conv1, conv2, conv3 and down.

Number format: symmetric int8 without a zero point (the project's one format), so a post-ReLU
tensor uses only 0..127 of the range -- one bit less than an asymmetric format would give it.

BasicBlock and grouped (ResNeXt) models are not covered: ``from_float`` raises
NotImplementedError.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from cloudtik_amd.models.resnet import Bottleneck, ResNet
from cloudtik_amd.ops import quant

STAGES = ("layer1", "layer2", "layer3", "layer4")
# the trial ladder of the quantize workflow: everything; without layer1 (the widest activations
# and, at Co = 64, the least int8 gain); the two deep stages that hold most of the FLOPs
TRIALS = (("layer1", "layer2", "layer3", "layer4"), ("layer2", "layer3", "layer4"), ("layer3", "layer4"))
_CONVS = ("conv1", "conv2", "conv3", "down")


def _check_sites(sites: Iterable[str]) -> List[str]:
    sites = list(sites)
    bad = [s for s in sites if s not in STAGES]
    if bad:
        raise ValueError(f"unknown int8 site(s) {bad}; choose from {list(STAGES)}")
    return [s for s in STAGES if s in sites]


def _range(act_amax: Dict[str, float], key: str) -> float:
    if key not in act_amax:
        raise ValueError(f"act_amax has no range for {key!r}")
    v = float(act_amax[key])
    quant.ref.static_scales(v)                             # finite, non-negative, fp32
    return v


def quantize_nhwc(x: torch.Tensor, amax: float) -> torch.Tensor:
    """``quantize_static`` of an image tensor that keeps its memory format (the cast is flat, so a
    channels_last tensor goes through its NHWC view)."""
    if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous():
        return quant.quantize_static(x.permute(0, 2, 3, 1), amax).permute(0, 3, 1, 2)
    return quant.quantize_static(x, amax)


class QuantBottleneck(nn.Module):
    """One bottleneck block on int8 tensors; every tensor is a buffer (nothing here trains).
    ``ranges``: {"in", "bn1", "bn2", "out"} and, with a downsample branch, "down_bn".
    ``float_out``: emit ``dtype`` instead of int8 (the consumer is not an int8 block)."""

    def __init__(self, cin: int, inner: int, cout: int, stride: int, downsample: bool, ranges: Dict[str, float],
                 float_out: bool = False, device=None, dtype=torch.bfloat16):
        super().__init__()
        self.stride, self.has_down, self.float_out, self.dtype = int(stride), bool(downsample), bool(float_out), dtype
        need = ("in", "bn1", "bn2", "out") + (("down_bn",) if downsample else ())
        self.ranges = {k: _range(ranges, k) for k in need}
        shapes = {"conv1": (inner, cin), "conv2": (inner, 9 * inner), "conv3": (cout, inner)}
        if downsample:
            shapes["down"] = (cout, cin)
        for name, (n, k) in shapes.items():
            self.register_buffer(f"{name}_weight_q", torch.zeros(n, k, device=device, dtype=torch.int8))
            self.register_buffer(f"{name}_weight_scale", torch.zeros(n, device=device, dtype=torch.float32))
            self.register_buffer(f"{name}_bias", torch.zeros(n, device=device, dtype=torch.float32))

    @classmethod
    def from_float(cls, block: nn.Module, ranges: Dict[str, float], float_out: bool = False) -> "QuantBottleneck":
        if not isinstance(block, Bottleneck):
            raise NotImplementedError(f"int8 ResNets are built from Bottleneck blocks, not {type(block).__name__}")
        if any(c.groups != 1 or tuple(c.dilation) != (1, 1) for c in (block.conv1, block.conv2, block.conv3)):
            raise NotImplementedError("grouped (ResNeXt) and dilated bottlenecks have no int8 convolution")
        w = block.conv1.weight
        q = cls(w.shape[1], w.shape[0], block.conv3.weight.shape[0], block.conv2.stride[0], block.down is not None,
                ranges, float_out, device=w.device, dtype=w.dtype)
        pairs = [("conv1", block.conv1, block.bn1), ("conv2", block.conv2, block.bn2), ("conv3", block.conv3, block.bn3)]
        if block.down is not None:
            pairs.append(("down", block.down, block.down_bn))
        for name, conv, bn in pairs:
            rows, bias = quant.fold_bn(conv.weight, bn)
            wq, ws = quant.quantize_weight(rows)
            getattr(q, f"{name}_weight_q").copy_(wq)
            getattr(q, f"{name}_weight_scale").copy_(ws)
            getattr(q, f"{name}_bias").copy_(bias)
        return q

    def _conv(self, name, x_q, a_amax, stride, padding, relu, out_amax, res_q=None, res_amax=None):
        return quant.conv2d_i8_static(x_q, a_amax, getattr(self, f"{name}_weight_q"),
                                      getattr(self, f"{name}_weight_scale"), getattr(self, f"{name}_bias"), stride,
                                      padding, relu, res_q, res_amax, out_amax, dtype=self.dtype)

    @torch.no_grad()
    def forward(self, x_q: torch.Tensor) -> torch.Tensor:
        r = self.ranges
        h = self._conv("conv1", x_q, r["in"], 1, 0, True, r["bn1"])
        h = self._conv("conv2", h, r["bn1"], self.stride, 1, True, r["bn2"])
        if self.has_down:
            idt, idt_amax = self._conv("down", x_q, r["in"], self.stride, 0, False, r["down_bn"]), r["down_bn"]
        else:
            idt, idt_amax = x_q, r["in"]
        return self._conv("conv3", h, r["bn2"], 1, 0, True, None if self.float_out else r["out"], idt, idt_amax)


def _stage_plan(model: ResNet, sites: List[str], act_amax: Dict[str, float]):
    """Per stage name: None (float) or a list of (ranges, float_out) per block."""
    plan, prev = {}, "stem"
    for i, name in enumerate(STAGES):
        blocks = getattr(model, name)
        nxt_int8 = i + 1 < len(STAGES) and STAGES[i + 1] in sites
        if name in sites:
            per = []
            for j, b in enumerate(blocks):
                key = f"{name}.{j}"
                rg = {"in": _range(act_amax, prev), "bn1": _range(act_amax, key + ".bn1"),
                      "bn2": _range(act_amax, key + ".bn2"), "out": _range(act_amax, key + ".out")}
                if getattr(b, "down", None) is not None:
                    rg["down_bn"] = _range(act_amax, key + ".down_bn")
                per.append((rg, j == len(blocks) - 1 and not nxt_int8))
                prev = key + ".out"
            plan[name] = per
        else:
            plan[name] = None
            prev = f"{name}.{len(blocks) - 1}.out"
    return plan


class QuantResNet(nn.Module):
    """``ResNet`` for inference with the stages in ``sites`` on int8 convolutions; same call."""

    stem = ResNet.stem

    def __init__(self, model: ResNet, sites: Iterable[str], act_amax: Dict[str, float]):
        """Takes over ``model``'s float modules (stem, float stages, fc) and replaces the stages
        in ``sites``; use ``from_float``."""
        super().__init__()
        for name in STAGES:
            for b in getattr(model, name):
                if not isinstance(b, Bottleneck):
                    raise NotImplementedError(
                        f"int8 ResNets are built from Bottleneck blocks, not {type(b).__name__}")
                if b.conv2.groups != 1:
                    raise NotImplementedError("grouped (ResNeXt) bottlenecks have no int8 convolution")
        self.sites = _check_sites(sites)
        self.act_amax = {k: float(v) for k, v in act_amax.items()}
        self.conv1, self.bn1, self.fc = model.conv1, model.bn1, model.fc
        plan = _stage_plan(model, self.sites, self.act_amax)
        self._entry = {}                                   # stage -> the range its float input is cast against
        prev_int8 = False
        for name in STAGES:
            blocks = getattr(model, name)
            if plan[name] is None:
                setattr(self, name, blocks)
                prev_int8 = False
            else:
                if not prev_int8:
                    self._entry[name] = plan[name][0][0]["in"]
                setattr(self, name, nn.Sequential(*[QuantBottleneck.from_float(b, rg, fo)
                                                    for b, (rg, fo) in zip(blocks, plan[name])]))
                prev_int8 = not plan[name][-1][1]
        self.requires_grad_(False)
        self.eval()

    @classmethod
    def from_float(cls, model: ResNet, sites: Iterable[str] = STAGES, act_amax: Optional[Dict[str, float]] = None
                   ) -> "QuantResNet":
        """Quantize a trained bottleneck ``ResNet`` (its float modules are shared, not copied).
        ``act_amax`` comes from ``calibrate``."""
        if act_amax is None:
            raise ValueError("static int8 convolutions need calibrated ranges (act_amax); see calibrate()")
        return cls(model, sites, act_amax)

    def train(self, mode: bool = True):
        return super().train(False)                        # inference only: BatchNorm on running statistics

    def trunk(self, x):
        """The four stages on the pooled stem output; returns the four stage outputs."""
        outs = []
        for name in STAGES:
            if name in self._entry:
                x = quantize_nhwc(x, self._entry[name])
            x = getattr(self, name)(x)
            outs.append(x)
        return outs

    @torch.no_grad()
    def forward(self, x):
        x = self.trunk(self.stem(x))[-1]
        x = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
        return self.fc(x)


@torch.no_grad()
def calibrate(float_model: ResNet, batches) -> Dict[str, float]:
    """Activation ranges for ``QuantResNet``: run the float model in eval mode over ``batches``
    (image tensors, or ``(images, labels)`` pairs) and return the largest ``abs()`` seen at the
    pooled stem output (``"stem"``) and, per bottleneck ``layerL.J``, at the outputs of ``bn1``,
    ``bn2``, ``down_bn`` (where present) and the block (``.out``) -- Python floats holding fp32
    values.  The running maxima stay on the device and are read back once, at the end."""
    p = float_model.fc.weight
    dev, dtype = p.device, p.dtype
    seen: Dict[str, torch.Tensor] = {}

    def note(key):
        def hook(_m, _inp, out):
            v = out.detach().abs().amax().float()
            seen[key] = v if key not in seen else torch.maximum(seen[key], v)
        return hook

    hooks = []
    for name in STAGES:
        for j, b in enumerate(getattr(float_model, name)):
            if not isinstance(b, Bottleneck):
                raise NotImplementedError(f"int8 ResNets are built from Bottleneck blocks, not {type(b).__name__}")
            key = f"{name}.{j}"
            hooks += [b.bn1.register_forward_hook(note(key + ".bn1")), b.bn2.register_forward_hook(note(key + ".bn2")),
                      b.register_forward_hook(note(key + ".out"))]
            if b.down is not None:
                hooks.append(b.down_bn.register_forward_hook(note(key + ".down_bn")))
    was_training = float_model.training
    float_model.eval()
    n = 0
    try:
        for b in batches:
            x = b[0] if isinstance(b, (tuple, list)) else b
            x = x.to(dev, dtype)
            if dev.type == "cuda":
                x = x.contiguous(memory_format=torch.channels_last)
            x = float_model.stem(x)
            note("stem")(None, None, x)
            for name in STAGES:
                x = getattr(float_model, name)(x)
            n += 1
    finally:
        for h in hooks:
            h.remove()
        float_model.train(was_training)
    if n == 0:
        raise ValueError("calibrate: no batches")
    keys = sorted(seen)
    vals = torch.stack([seen[k] for k in keys]).cpu().tolist()
    return dict(zip(keys, vals))
