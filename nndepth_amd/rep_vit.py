"""Encoder side of Coarse2FineGroupRepViTRAFTStereo: the RepViT backbone (reference: nndepth/encoders/rep_vit.py:482-744), its
blocks (rep_vit.py:10-480), LinearSelfAttention (nndepth/blocks/attn_block.py:100-169) and MobileOneBlock / RepLargeKernelConv /
FeatureFusionBlock (nndepth/blocks/conv.py:130-567).

Parameter containers: module paths, parameter names, shapes and registration order are the reference's train-time layout (what its
constructor builds and its checkpoints hold), so a reference state_dict loads with strict=True.  At inference the model class runs
the whole encoder side as hand-written HIP (csrc/repvit.hip through ops.RepViTEngine, one C-ABI call: nnd_repvit_forward), with
every branch / BatchNorm / layer scale folded on the host; the `forward` methods here are the plain PyTorch formulation and are only
reached through the explicit opt-out `hip_encoder=False` of the model class (never silently).

Reference behaviours reproduced on purpose (each also commented where it happens):
  * RepLargeKernelConv applies its activation and discards the result: the patch-embed depthwise conv has NO activation
    (conv.py:454).
  * MobileOneBlock.rbr_skip exists only if in == out and `stride == 1` (conv.py:201-203): a stride given as the tuple (1, 1), as the
    reference's stem_strides are, does not compare equal to 1, so such a block has no skip branch.
  * LinearSelfAttention gets the 4-D (B, C, H, W) map from AttentionBlock: its softmax runs over W, per row and per sample, and the
    context vector is per (channel, row) (attn_block.py:151-160).
  * FeatureFusionBlock upsamples with bilinear interpolate, align_corners=False (conv.py:559-562).
There is no timm dependency: DropPath is an identity at inference (drop_path_rate is 0 in every reference config) and
trunc_normal_ is torch.nn.init's.
"""
from typing import List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F


def _conv_bn(cin: int, cout: int, k: int, stride, padding: int, groups: int) -> nn.Sequential:
    """conv (no bias) + BatchNorm, registered as `conv` / `bn` (conv.py:350-371, 525-546)."""
    m = nn.Sequential()
    m.add_module("conv", nn.Conv2d(cin, cout, k, stride=stride, padding=padding, groups=groups, bias=False))
    m.add_module("bn", nn.BatchNorm2d(cout))
    return m


class MobileOneBlock(nn.Module):
    """Train-time MobileOne block (conv.py:130-371): sum of the skip BatchNorm, the 1x1 scale branch and `num_conv_branches`
    conv+BN branches, then the activation (exact GELU unless use_act=False).  Squeeze-excitation (use_se) is not built."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 3, stride=1, padding: int = 1, groups: int = 1,
                 use_act: bool = True, use_scale_branch: bool = True, num_conv_branches: int = 1, inference_mode: bool = False,
                 use_se: bool = False, activation: Optional[nn.Module] = None):
        super().__init__()
        if inference_mode or use_se:
            raise ValueError("MobileOneBlock: only the train-time layout without squeeze-excitation is built "
                             "(reparameterised checkpoints are not supported)")
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding, self.groups, self.num_conv_branches = stride, padding, groups, num_conv_branches
        self.inference_mode = False
        self.se = nn.Identity()
        self.activation = (activation if activation is not None else nn.GELU()) if use_act else nn.Identity()
        # conv.py:201-203: `stride == 1` is False for the tuple (1, 1) -> no skip branch there
        self.rbr_skip = nn.BatchNorm2d(in_channels) if out_channels == in_channels and stride == 1 else None
        self.rbr_conv = (nn.ModuleList([_conv_bn(in_channels, out_channels, kernel_size, stride, padding, groups)
                                        for _ in range(num_conv_branches)]) if num_conv_branches > 0 else None)
        self.rbr_scale = _conv_bn(in_channels, out_channels, 1, stride, 0, groups) if kernel_size > 1 and use_scale_branch else None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        # the reference's summation order (conv.py:226-243): (scale + skip), then each conv branch added in place
        identity_out = self.rbr_skip(x) if self.rbr_skip is not None else 0
        scale_out = self.rbr_scale(x) if self.rbr_scale is not None else 0
        out = scale_out + identity_out
        if self.rbr_conv is not None:
            for branch in self.rbr_conv:
                out += branch(x)
        return self.activation(self.se(out))


class RepLargeKernelConv(nn.Module):
    """Large depthwise kernel + small kernel branch, each conv + BN (conv.py:374-442).  No activation is applied (conv.py:454)."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride, groups: int, small_kernel: int = 3,
                 activation: Optional[nn.Module] = None, inference_mode: bool = False):
        super().__init__()
        if inference_mode:
            raise ValueError("RepLargeKernelConv: reparameterised (lkb_reparam) checkpoints are not supported")
        self.in_channels, self.out_channels, self.kernel_size, self.small_kernel = in_channels, out_channels, kernel_size, small_kernel
        self.stride, self.groups, self.padding = stride, groups, kernel_size // 2
        self.activation = activation if activation is not None else nn.GELU()
        self.lkb_origin = _conv_bn(in_channels, out_channels, kernel_size, stride, self.padding, groups)
        if small_kernel is not None:
            assert small_kernel <= kernel_size
            self.small_conv = _conv_bn(in_channels, out_channels, small_kernel, stride, small_kernel // 2, groups)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        out = self.lkb_origin(x)
        if hasattr(self, "small_conv"):
            out += self.small_conv(x)
        # conv.py:454 calls self.activation(out) and throws the result away: the block's output is NOT activated
        return out


class FeatureFusionBlock(nn.Module):
    """relu(conv3(cat[conv1(up(feats[0])), conv2(feats[1])])), up = bilinear, align_corners=False (conv.py:549-567)."""

    def __init__(self, in_channels_1: int, in_channels_2: int, out_channels: int, kernel_size: int = 3, padding: int = 3):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels_1, in_channels_1, kernel_size=kernel_size, padding=padding)
        self.conv2 = nn.Conv2d(in_channels_2, in_channels_2, kernel_size=kernel_size, padding=padding)
        self.conv3 = nn.Conv2d(in_channels_1 + in_channels_2, out_channels, kernel_size=kernel_size, padding=padding)
        self.act = nn.ReLU()

    def forward(self, feats: List[torch.Tensor]) -> torch.Tensor:
        up = F.interpolate(feats[0], size=feats[1].shape[-2:], mode="bilinear", align_corners=False)
        return self.act(self.conv3(torch.cat([self.conv1(up), self.conv2(feats[1])], dim=1)))


class LinearSelfAttention(nn.Module):
    """MobileViTv2 linear attention (attn_block.py:100-169) on a 4-D map (B, C, H, W): query = channel 0 of qkv_proj,
    softmax over the LAST axis (W: per sample and row), context[c, row] = sum_w key[c, row, w] * score[row, w],
    out = out_proj(relu(value) * context)."""

    def __init__(self, dim: int, head_dim: int = 32, attn_dropout: float = 0.0, bias: bool = True):
        super().__init__()
        self.qkv_proj = nn.Conv2d(dim, 1 + 2 * dim, kernel_size=1, bias=bias)
        self.attn_dropout = nn.Dropout(p=attn_dropout)
        self.out_proj = nn.Conv2d(dim, dim, kernel_size=1, bias=bias)
        self.embed_dim = dim

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        q, k, v = torch.split(self.qkv_proj(x), [1, self.embed_dim, self.embed_dim], dim=1)
        scores = self.attn_dropout(F.softmax(q, dim=-1))  # over W, per (sample, row): the map is 4-D here
        context = torch.sum(k * scores, dim=-1, keepdim=True)
        return self.out_proj(F.relu(v) * context.expand_as(v))


class ChannelMixer(nn.Module):
    """fc1 (1x1) -> GELU -> fc2 (1x1); dropouts are identities at inference (rep_vit.py:69-114)."""

    def __init__(self, in_channels: int, hidden_channels: int, drop: float = 0.0):
        super().__init__()
        self.fc1 = nn.Conv2d(in_channels, hidden_channels, kernel_size=1)
        self.act = nn.GELU()
        self.fc2 = nn.Conv2d(hidden_channels, in_channels, kernel_size=1)
        self.drop = nn.Dropout(drop)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class RepTokenMixer(nn.Module):
    """x + layer_scale * (mixer(x) - norm(x)) (rep_vit.py:117-224); `norm` is a skip BatchNorm alone (no conv, no scale branch)."""

    def __init__(self, dim: int, kernel_size: int = 3, use_layer_scale: bool = True, layer_scale_init_value: float = 1e-5):
        super().__init__()
        self.dim, self.kernel_size, self.inference_mode = dim, kernel_size, False
        self.norm = MobileOneBlock(dim, dim, kernel_size, padding=kernel_size // 2, groups=dim, use_act=False,
                                   use_scale_branch=False, num_conv_branches=0)
        self.mixer = MobileOneBlock(dim, dim, kernel_size, padding=kernel_size // 2, groups=dim, use_act=False)
        self.use_layer_scale = use_layer_scale
        if use_layer_scale:
            self.layer_scale = nn.Parameter(layer_scale_init_value * torch.ones((dim, 1, 1)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.use_layer_scale:
            return x + self.layer_scale * (self.mixer(x) - self.norm(x))
        return x + self.mixer(x) - self.norm(x)


class RepFormerBlock(nn.Module):
    """token_mixer, then (use_ffn) x + layer_scale * convffn(x) (rep_vit.py:227-306)."""

    def __init__(self, dim: int, kernel_size: int = 3, use_ffn: bool = True, ffn_exp_ratio: float = 4.0, drop: float = 0.0,
                 use_layer_scale: bool = True, layer_scale_init_value: float = 1e-5):
        super().__init__()
        self.token_mixer = RepTokenMixer(dim, kernel_size, use_layer_scale, layer_scale_init_value)
        self.use_ffn = use_ffn
        if use_ffn:
            self.convffn = ChannelMixer(dim, int(dim * ffn_exp_ratio), drop)
            self.drop_path = nn.Identity()
            self.use_layer_scale = use_layer_scale
            if use_layer_scale:
                self.layer_scale = nn.Parameter(layer_scale_init_value * torch.ones((dim, 1, 1)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.token_mixer(x)
        if not self.use_ffn:
            return x
        if self.use_layer_scale:
            return x + self.drop_path(self.layer_scale * self.convffn(x))
        return x + self.drop_path(self.convffn(x))


class AttentionBlock(nn.Module):
    """x + ls1 * token_mixer(norm(x)), then x + ls2 * convffn(x); norm = BatchNorm2d (rep_vit.py:363-426)."""

    def __init__(self, dim: int, ffn_exp_ratio: float = 4.0, drop: float = 0.0, use_layer_scale: bool = True,
                 layer_scale_init_value: float = 1e-5):
        super().__init__()
        self.norm = nn.BatchNorm2d(dim)
        self.token_mixer = LinearSelfAttention(dim)
        self.convffn = ChannelMixer(dim, int(dim * ffn_exp_ratio), drop)
        self.drop_path = nn.Identity()
        self.use_layer_scale = use_layer_scale
        if use_layer_scale:
            self.layer_scale_1 = nn.Parameter(layer_scale_init_value * torch.ones((dim, 1, 1)))
            self.layer_scale_2 = nn.Parameter(layer_scale_init_value * torch.ones((dim, 1, 1)))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.use_layer_scale:
            x = x + self.drop_path(self.layer_scale_1 * self.token_mixer(self.norm(x)))
            return x + self.drop_path(self.layer_scale_2 * self.convffn(x))
        x = x + self.drop_path(self.token_mixer(self.norm(x)))
        return x + self.drop_path(self.convffn(x))


class ConvPatchEmbed(nn.Module):
    """proj = [RepLargeKernelConv (depthwise patch_size x patch_size, stride, small kernel 3), MobileOneBlock 1x1 -> embed_dim]
    (rep_vit.py:309-360)."""

    def __init__(self, patch_size: int, stride, in_channels: int, embed_dim: int):
        super().__init__()
        self.proj = nn.Sequential(
            RepLargeKernelConv(in_channels, in_channels, patch_size, stride, groups=in_channels, small_kernel=3),
            MobileOneBlock(in_channels, embed_dim, kernel_size=1, stride=1, padding=0, groups=1, num_conv_branches=1))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.proj(x)


def convolutional_stem(in_channels: int, out_channels: int, strides: Sequence) -> nn.Sequential:
    """3x3 dense, 3x3 depthwise, 1x1 MobileOne blocks with GELU (rep_vit.py:429-479)."""
    return nn.Sequential(
        MobileOneBlock(in_channels, out_channels, 3, stride=strides[0], padding=1, groups=1),
        MobileOneBlock(out_channels, out_channels, 3, stride=strides[1], padding=1, groups=out_channels),
        MobileOneBlock(out_channels, out_channels, 1, stride=strides[2], padding=0, groups=1))


class RepViT(nn.Module):
    """stem (16 ch) + four stages of [ConvPatchEmbed, blocks]; forward returns the five outputs [stem, stage_0 .. stage_3]."""
    BASE_NUM_CHANNELS = [32, 64, 128, 256]

    def __init__(self, in_channels: int = 3, patch_size: int = 7, stem_strides=((2, 2), (2, 2), (1, 1)),
                 num_blocks_per_stage=(4, 4, 6, 2), width_multipliers=(1, 1, 1, 1), use_ffn_per_stage=(False, True, True, True),
                 ffn_exp_ratios=(1.0, 3.0, 3.0, 4.0), downsample_ratios=((2, 2), (2, 2), (2, 2), (2, 2)),
                 token_mixer_types=("repmixer", "repmixer", "repmixer", "attention"), drop_rate: float = 0.0,
                 drop_path_rate: float = 0.0, use_layer_scale: bool = True, layer_scale_init_value: float = 1e-5,
                 inference_mode: bool = False, **kwargs):
        super().__init__()
        if inference_mode:
            raise ValueError("RepViT: inference_mode (reparameterised) checkpoints are not supported")
        if drop_path_rate != 0.0:
            raise ValueError("RepViT: drop_path_rate must be 0 (DropPath is not built; it is an identity at inference)")
        assert len(num_blocks_per_stage) == len(width_multipliers)
        self.num_blocks_per_stage, self.width_multipliers = list(num_blocks_per_stage), list(width_multipliers)
        self.patch_size, self.stem_strides, self.downsample_ratios = patch_size, stem_strides, downsample_ratios
        self.token_mixer_types, self.use_ffn_per_stage, self.ffn_exp_ratios = token_mixer_types, use_ffn_per_stage, ffn_exp_ratios
        self.stem = convolutional_stem(in_channels, 16, stem_strides)
        cin = 16
        for i in range(4):
            ch = int(self.BASE_NUM_CHANNELS[i] * width_multipliers[i])
            blocks = []
            for _ in range(num_blocks_per_stage[i]):
                if token_mixer_types[i] == "repmixer":
                    blocks.append(RepFormerBlock(ch, 3, use_ffn_per_stage[i], ffn_exp_ratios[i], drop_rate, use_layer_scale,
                                                 layer_scale_init_value))
                elif token_mixer_types[i] == "attention":
                    blocks.append(AttentionBlock(ch, ffn_exp_ratios[i], drop_rate, use_layer_scale, layer_scale_init_value))
                else:
                    raise ValueError(f"Token mixer type: {token_mixer_types[i]} not supported")
            setattr(self, f"stage_{i}", nn.Sequential(ConvPatchEmbed(patch_size, downsample_ratios[i], cin, ch), nn.Sequential(*blocks)))
            cin = ch
        self.num_channels = cin

    def forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        features = []
        for layer in (self.stem, self.stage_0, self.stage_1, self.stage_2, self.stage_3):
            x = layer(x)
            features.append(x)
        return features


def reparam_blocker(*modules: nn.Module) -> Optional[str]:
    """The first reparameterised submodule (`reparam_conv` / `lkb_reparam` present) of `modules`, named, or None."""
    for top in modules:
        for name, m in top.named_modules():
            for attr in ("reparam_conv", "lkb_reparam"):
                if hasattr(m, attr):
                    return f"{type(m).__name__} '{name}' is reparameterised ({attr})"
    return None
