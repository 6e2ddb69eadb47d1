"""MobileNetV3DepthModel: the reference's MiDaS-style monocular depth model on the HIP path.

Drop-in for `nndepth.models.midas.models.mobilenet_v3.MobileNetV3DepthModel` (inference entry point: nndepth/models/midas/scripts/
inference.py, model name "mbnet_v3"): the same constructor kwargs and the same state_dict keys, shapes and order

    encoder.backbone.*                                            tf_mobilenetv3_large_100(features_only=True), nndepth_amd.mobilenetv3
    decoder.skip_layers.N.0.{weight,bias}                         3x3 (24 / 40 / 112 / 160 -> C) + ReLU
    decoder.upsampler_layers.N.{conv1,conv2,out_conv,bn1,bn2}.*   UpsamplerBlock (nndepth/blocks/upsampler_block.py)
    last_conv.{0,2,4}.{weight,bias}                               3x3, x2 bilinear, 3x3, ReLU, 1x1 (C -> 1), ReLU

so a reference checkpoint loads with strict=True (`weights=`: .pth, or .safetensors where that package is installed).  Nothing is
downloaded: the reference's `pretrained=True` ImageNet initialisation of the backbone is not reproduced.

hip=True (default): the whole forward is ONE C-ABI call (csrc/midas.hip: nnd_midas_forward, exact fp32; ops.MidasEngine folds the
BatchNorms on the host in float64 and repacks only when a parameter changes).  Inference only: forward() raises in training mode.
H and W must be multiples of 32.  hip=False is the explicit PyTorch path of these modules (any device / dtype; the float64 oracle of
the tests); there is no silent fallback from one to the other.
"""
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._lib import NndError
from .mobilenetv3 import MobilenetV3LargeEncoder
from .raft_stereo import load_weights

HOOKS = (1, 2, 4, 5)  # the backbone stages the decoder reads (1/4 ... 1/32)
TAP_CHANNELS = (24, 40, 112, 160)


class UpsamplerBlock(nn.Module):
    """out = relu(out_conv(up2x(relu(bn2(conv2(feat [+ relu(bn1(conv1(skip_feat)))])))))), up2x bilinear with align_corners=False."""

    def __init__(self, in_channels: int, out_channels: int, use_bn: bool = True):
        super().__init__()
        self.in_channels, self.out_channels, self.use_bn = in_channels, out_channels, use_bn
        self.conv1 = nn.Conv2d(in_channels, in_channels, kernel_size=3, padding=1, stride=1)
        self.conv2 = nn.Conv2d(in_channels, in_channels, kernel_size=3, padding=1, stride=1)
        self.out_conv = nn.Conv2d(in_channels, out_channels, kernel_size=1, padding=0, stride=1)
        self.bn1 = nn.BatchNorm2d(in_channels) if use_bn else nn.Identity()
        self.bn2 = nn.BatchNorm2d(in_channels) if use_bn else nn.Identity()
        self.activation = nn.ReLU()

    def forward(self, feat: torch.Tensor, skip_feat: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = feat
        if skip_feat is not None:
            out = out + self.activation(self.bn1(self.conv1(skip_feat)))
        out = self.activation(self.bn2(self.conv2(out)))
        out = F.interpolate(out, scale_factor=2, mode="bilinear", align_corners=False)
        return self.activation(self.out_conv(out))


class BaseDecoder(nn.Module):
    """One 3x3 + ReLU per tap, then the UpsamplerBlocks from the coarsest tap up; the coarsest block runs without a skip input (its
    conv1 / bn1 are parameters that are never evaluated)."""

    def __init__(self, in_channels: List[int], out_channels):
        super().__init__()
        if isinstance(out_channels, int):
            out_channels = [out_channels] * len(in_channels)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.skip_layers = nn.ModuleList(
            nn.Sequential(nn.Conv2d(ci, co, kernel_size=3, padding=1, stride=1), nn.ReLU()) for ci, co in zip(in_channels, out_channels))
        self.upsampler_layers = nn.ModuleList(UpsamplerBlock(c, c, use_bn=True) for c in out_channels)

    def forward(self, feats: List[torch.Tensor]) -> torch.Tensor:
        skips = [layer(f) for layer, f in zip(self.skip_layers, feats)]
        out = self.upsampler_layers[-1](skips[-1])
        for i in range(len(skips) - 2, -1, -1):
            out = self.upsampler_layers[i](out, skips[i])
        return out


class MobileNetV3DepthModel(nn.Module):
    def __init__(self, feature_channels: int = 64, weights: Optional[str] = None, strict_load: bool = True, hip: bool = True):
        super().__init__()
        self.feature_channels, self.weights, self.strict_load, self.hip = feature_channels, weights, strict_load, hip
        c = feature_channels
        self.encoder = MobilenetV3LargeEncoder(feature_hooks=list(HOOKS))
        self.decoder = BaseDecoder(in_channels=list(TAP_CHANNELS), out_channels=[c] * 4)
        self.last_conv = nn.Sequential(
            nn.Conv2d(c, c, kernel_size=3, padding=1, stride=1),
            nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False),
            nn.Conv2d(c, c, kernel_size=3, padding=1, stride=1),
            nn.ReLU(),
            nn.Conv2d(c, 1, kernel_size=1, padding=0, stride=1),
            nn.ReLU(),
        )
        self._engine = ops.ParamCache()
        if weights is not None:
            if not (weights.endswith(".pth") or weights.endswith(".safetensors")):
                raise ValueError(f"Unsupported weight format: {weights}")
            load_weights(self, weights, strict_load)

    # ------------------------------------------------------------------ explicit PyTorch path (hip=False) and test oracle
    def forward_torch(self, x: torch.Tensor) -> dict:
        """The modules' own forward, every map the tests compare: {tap0..tap3, decoder, pre_relu, depth}."""
        taps = self.encoder(x)
        dec = self.decoder(taps)
        pre = self.last_conv[:5](dec)
        r = {f"tap{i}": t for i, t in enumerate(taps)}
        r.update(decoder=dec, pre_relu=pre, depth=self.last_conv[5](pre))
        return r

    # ------------------------------------------------------------------ HIP path
    def engine(self, device) -> "ops.MidasEngine":
        """The packed engine for the current parameters: refolded and repacked only when a parameter / buffer changed or a module
        was replaced (ops.ParamCache)."""
        if self.training:
            raise NndError(f"{type(self).__name__} is inference-only on the HIP path: call model.eval() first (BatchNorm is folded with "
                           "its running statistics; pass hip=False for the PyTorch modules)")
        return self._engine.get((self,), device, lambda: ops.MidasEngine.from_model(self, device), track_modules=True)

    def forward_maps(self, x: torch.Tensor):
        """HIP forward that also returns the intermediate maps (views of the engine's workspace, valid until the next call)."""
        if x.dim() == 4 and (x.shape[2] % 32 or x.shape[3] % 32):
            raise NndError(f"{type(self).__name__}: H {x.shape[2]} / W {x.shape[3]} must be multiples of 32 on the HIP path")
        eng = self.engine(x.device)
        return eng.forward(x, keep=True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.hip:
            return self.forward_torch(x)["depth"]
        if x.dim() == 4 and (x.shape[2] % 32 or x.shape[3] % 32):
            raise NndError(f"{type(self).__name__}: H {x.shape[2]} / W {x.shape[3]} must be multiples of 32 on the HIP path (pad or "
                           "resize the frame, e.g. prepost.preprocess_frame)")
        if self.training:
            self.engine(x.device)  # raises: inference-only
        if not x.is_cuda:
            raise NndError(f"nndepth_amd ops run on the HIP device only; got a tensor on {x.device} (no CPU fallback exists; hip=False "
                           "is the explicit PyTorch path)")
        return self.engine(x.device).forward(x)


# mirrors NAME_TO_MODEL_CONFIG of the reference's inference script
DEPTH_MODELS = {"mbnet_v3": MobileNetV3DepthModel}
