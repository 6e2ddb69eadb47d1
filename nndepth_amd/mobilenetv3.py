"""timm-free parameter containers of the MobileNetV3-Large backbone of IGEVStereoMBNet.

The reference builds `timm.models.mobilenetv3.tf_mobilenetv3_large_100(features_only=True)` (timm 1.0.16, MobileNetV3Features)
inside `MobilenetV3LargeEncoder` (nndepth/encoders/mobilenetv3_encoder.py) and stores it as `fnet.backbone`.  The modules here
register the same parameters and buffers under the same names, with the same shapes and in the same order, so a reference checkpoint
loads with strict=True:

    conv_stem (16,3,3,3) | bn1 | blocks.<stage>.<block>.{conv_dw, bn1, conv_pw, bn2}           DepthwiseSeparable (stage 0)
                                 blocks.<stage>.<block>.{conv_pw, bn1, conv_dw, bn2,
                                                         [se.conv_reduce, se.conv_expand], conv_pwl, bn3}   InvertedResidual
                                 blocks.6.0.{conv, bn1}                                        ConvBnAct (stage 6)

The `tf_` variant: BatchNorm eps 1e-3 and TensorFlow "same" padding (`same_pad`).  The PyTorch forward here is the explicit
opt-in of IGEVStereoMBNet(hip_encoder=False) and the float64 oracle of the tests; the HIP path (csrc/mbv3.hip) folds the same
modules (ops.MobileNetV3Engine).  No weights are downloaded: parameters come only from a checkpoint.
"""
import math
import re
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

BN_EPS = 1e-3  # timm's BN_EPS_TF_DEFAULT

# timm's _gen_mobilenet_v3 arch_def for "large" ("nre": ReLU, else hard-swish)
ARCH_DEF = [
    ["ds_r1_k3_s1_e1_c16_nre"],
    ["ir_r1_k3_s2_e4_c24_nre", "ir_r1_k3_s1_e3_c24_nre"],
    ["ir_r3_k5_s2_e3_c40_se0.25_nre"],
    ["ir_r1_k3_s2_e6_c80", "ir_r1_k3_s1_e2.5_c80", "ir_r2_k3_s1_e2.3_c80"],
    ["ir_r2_k3_s1_e6_c112_se0.25"],
    ["ir_r3_k5_s2_e6_c160_se0.25"],
    ["cn_r1_k1_s1_c960"],
]
STEM_C = 16
HOOKS = (1, 2, 3, 4, 5)  # the stages whose outputs MobilenetV3LargeEncoder returns (IGEVStereoMBNet: feature_hooks=[1, 2, 3, 4, 5])


def make_divisible(v: float, divisor: int = 8, min_value=None, round_limit: float = 0.9) -> int:
    """timm.layers.make_divisible."""
    min_value = min_value or divisor
    new_v = max(min_value, int(v + divisor / 2) // divisor * divisor)
    if new_v < round_limit * v:
        new_v += divisor
    return new_v


def decode_block(s: str) -> dict:
    """One timm arch string -> {type, repeat, k, s, e, c, se, relu}."""
    ops = s.split("_")
    d = {"type": ops[0], "se": 0.0, "e": 1.0, "relu": False}
    for op in ops[1:]:
        if op == "nre":
            d["relu"] = True
            continue
        m = re.match(r"([a-z]+)([\d.]+)$", op)
        key, val = m.group(1), m.group(2)
        if key == "r":
            d["repeat"] = int(val)
        elif key == "k":
            d["k"] = int(val)
        elif key == "s":
            d["s"] = int(val)
        elif key == "e":
            d["e"] = float(val)
        elif key == "c":
            d["c"] = int(val)
        elif key == "se":
            d["se"] = float(val)
    return d


def block_table() -> List[List[dict]]:
    """Every block of every stage: {type, cin, mid, cout, k, stride, rd (SE reduce channels, 0: none), relu, skip}, the widths
    from the arch strings with timm's rules (mid = make_divisible(cin * e), SE from the expanded width: make_divisible(mid * se))."""
    stages, cin = [], STEM_C
    for stage in ARCH_DEF:
        blocks = []
        for s in stage:
            d = decode_block(s)
            for r in range(d["repeat"]):
                stride = d["s"] if r == 0 else 1
                mid = make_divisible(cin * d["e"]) if d["type"] == "ir" else cin
                rd = make_divisible(mid * d["se"]) if d["se"] > 0 else 0
                skip = d["type"] != "cn" and stride == 1 and cin == d["c"]
                blocks.append(dict(type=d["type"], cin=cin, mid=mid, cout=d["c"], k=d["k"], stride=stride, rd=rd, relu=d["relu"],
                                   skip=skip))
                cin = d["c"]
        stages.append(blocks)
    return stages


def same_pad(x: torch.Tensor, k: int, stride: int) -> torch.Tensor:
    """TensorFlow "same" padding: total max((ceil(n / s) - 1) * s + k - n, 0) per axis, the smaller half before (timm pad_same)."""
    h, w = x.shape[-2:]
    ph = max((math.ceil(h / stride) - 1) * stride + k - h, 0)
    pw = max((math.ceil(w / stride) - 1) * stride + k - w, 0)
    if ph == 0 and pw == 0:
        return x
    return F.pad(x, [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2])


class SameConv2d(nn.Conv2d):
    """nn.Conv2d (same parameters / keys) with TF "same" padding: static k // 2 at stride 1 (timm's nn.Conv2d), dynamic at stride 2
    (timm's Conv2dSame)."""

    def __init__(self, cin: int, cout: int, k: int, stride: int = 1, groups: int = 1, bias: bool = False):
        super().__init__(cin, cout, k, stride, 0, groups=groups, bias=bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        k, s = self.kernel_size[0], self.stride[0]
        return F.conv2d(same_pad(x, k, s), self.weight, self.bias, s, 0, 1, self.groups)


def _bn(c: int) -> nn.BatchNorm2d:
    return nn.BatchNorm2d(c, eps=BN_EPS)


def _act(x: torch.Tensor, relu: bool) -> torch.Tensor:
    return F.relu(x) if relu else F.hardswish(x)


class SqueezeExcite(nn.Module):
    """x * hardsigmoid(conv_expand(relu(conv_reduce(mean_hw(x)))))."""

    def __init__(self, c: int, rd: int):
        super().__init__()
        self.conv_reduce = nn.Conv2d(c, rd, 1, bias=True)
        self.conv_expand = nn.Conv2d(rd, c, 1, bias=True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        s = x.mean((2, 3), keepdim=True)
        return x * F.hardsigmoid(self.conv_expand(F.relu(self.conv_reduce(s))))


class DepthwiseSeparable(nn.Module):
    def __init__(self, b: dict):
        super().__init__()
        self.spec = dict(b)
        self.conv_dw = SameConv2d(b["cin"], b["cin"], b["k"], b["stride"], groups=b["cin"])
        self.bn1 = _bn(b["cin"])
        self.conv_pw = nn.Conv2d(b["cin"], b["cout"], 1, bias=False)
        self.bn2 = _bn(b["cout"])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = self.bn2(self.conv_pw(_act(self.bn1(self.conv_dw(x)), self.spec["relu"])))
        return x + y if self.spec["skip"] else y


class InvertedResidual(nn.Module):
    def __init__(self, b: dict):
        super().__init__()
        self.spec = dict(b)
        self.conv_pw = nn.Conv2d(b["cin"], b["mid"], 1, bias=False)
        self.bn1 = _bn(b["mid"])
        self.conv_dw = SameConv2d(b["mid"], b["mid"], b["k"], b["stride"], groups=b["mid"])
        self.bn2 = _bn(b["mid"])
        self.se = SqueezeExcite(b["mid"], b["rd"]) if b["rd"] else nn.Identity()
        self.conv_pwl = nn.Conv2d(b["mid"], b["cout"], 1, bias=False)
        self.bn3 = _bn(b["cout"])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        relu = self.spec["relu"]
        y = _act(self.bn1(self.conv_pw(x)), relu)
        y = self.se(_act(self.bn2(self.conv_dw(y)), relu))
        y = self.bn3(self.conv_pwl(y))
        return x + y if self.spec["skip"] else y


class ConvBnAct(nn.Module):
    def __init__(self, b: dict):
        super().__init__()
        self.spec = dict(b)
        self.conv = SameConv2d(b["cin"], b["cout"], b["k"], b["stride"])
        self.bn1 = _bn(b["cout"])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return _act(self.bn1(self.conv(x)), self.spec["relu"])


_BLOCK = {"ds": DepthwiseSeparable, "ir": InvertedResidual, "cn": ConvBnAct}


class MobileNetV3Features(nn.Module):
    """The parameter layout of timm's tf_mobilenetv3_large_100(features_only=True): conv_stem, bn1, act1 (hard-swish), 7 stages.
    It has no forward of its own: MobilenetV3LargeEncoder runs it, as the reference's wrapper runs timm's."""

    def __init__(self):
        super().__init__()
        self.conv_stem = SameConv2d(3, STEM_C, 3, 2)
        self.bn1 = _bn(STEM_C)
        self.act1 = nn.Hardswish()
        self.blocks = nn.Sequential(*[nn.Sequential(*[_BLOCK[b["type"]](b) for b in stage]) for stage in block_table()])


class MobilenetV3LargeEncoder(nn.Module):
    """The reference's wrapper (nndepth/encoders/mobilenetv3_encoder.py) with feature_hooks: conv_stem -> bn1 -> hard-swish ->
    blocks, the outputs of the hooked stages in order.  Stage 6 holds parameters (reference checkpoints carry them) but its output
    is never used, so it is not run here (the reference runs it and discards it)."""

    def __init__(self, feature_hooks=HOOKS):
        super().__init__()
        self.backbone = MobileNetV3Features()
        self.feature_hooks = list(feature_hooks)

    def forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        bb = self.backbone
        x = bb.act1(bb.bn1(bb.conv_stem(x)))
        feats = []
        last = max(self.feature_hooks)
        for i, blk in enumerate(bb.blocks):
            if i > last:
                break
            x = blk(x)
            if i in self.feature_hooks:
                feats.append(x)
        return feats
