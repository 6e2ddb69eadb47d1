"""Shared by tests/test_calib_cpu.py and tests/test_gpu_calib.py (not a test module): the update-block cases of the fp16x2
calibration tests and a plain float64 walk of one BasicUpdateBlock call that also returns, per convolution of
csrc/update_block.hip (kConvNames), the largest |x| of the tensor that convolution stages — what a calibration forward must
record (include/nndepth_amd.h "fp16x2 activation range", csrc/calib.hip).

Which tensor a layer stages is read off the launchers (update_block.hip: conv_io, run_update, enqueue_refine, calib_flow_branch):
  single call (nnd_update_block_forward -> run_update)      fused loops (enqueue_refine)
    encoder.convc1        corr                                the same four encoder layers,
    encoder.convc2        relu(convc1(corr))                  gru.convz1+convr1[h,motion]   cat(h, motion)
    encoder.convf2        relu(convf1(flow))                  gru.convq1[rh,motion]         cat(r*h, motion)
    encoder.conv          cat(cor, flo)                       gru.convz1+convr1[inp], gru.convq1[inp]   inp
    gru.convz1+convr1     cat(h, inp, motion)                 (pass 2 likewise, h = the result of pass 1)
    gru.convq1            cat(r*h, inp, motion)               flow_head.conv1+mask.0, mask.2 as on the left
    flow_head.conv1+mask.0  the new hidden state
    mask.2                relu(mask.0(h))
`motion` is the motion encoder's output WITH the flow channels behind it.  The two entry points run different packings of the GRU
convolutions, so each leaves the other's layers at their previous scale: LOOP_ONLY / SINGLE_ONLY below."""
import math
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from nndepth_amd import weightgen
from oracle import torch_ref as R

B, H, W = 2, 13, 22  # ragged: neither a multiple of the 8 x 32 pixel tile nor of the 4 x 8 one
DEFAULT_RANGE = 16376.0  # 65504 / 2^2: a freshly packed layer (split_arith.h: SPLIT_F16_XSHIFT)

# the four entries of CASES in test_gpu_parity.py and one conv_gru block;  last column: the seed of the inputs, chosen so that
# every recorded maximum is at least 1 % away from a power of two (asserted in test_calib_cpu.py)
CASES = {
    "raft_h128_c64": (dict(hidden_dim=128, context_dim=64, cor_planes=36, flow_channel=1, spatial_scale=8), "sep_conv", 2),
    "raft_h128_c128": (dict(hidden_dim=128, context_dim=128, cor_planes=36, flow_channel=1, spatial_scale=8), "sep_conv", 0),
    "cre_h128_c128_f2": (dict(hidden_dim=128, context_dim=128, cor_planes=36, flow_channel=2, spatial_scale=8), "sep_conv", 6),
    "igev_h64_c64_cp576": (dict(hidden_dim=64, context_dim=64, cor_planes=576, flow_channel=1, spatial_scale=4), "sep_conv", 0),
    "convgru_h128_c128": (dict(hidden_dim=128, context_dim=128, cor_planes=36, flow_channel=1, spatial_scale=8), "conv_gru", 0),
}
NAMES = tuple(CASES)


def is_loop_only(name: str) -> bool:
    """Layers that only the fused loops run (update_block.hip:915-919 C_*X, :840-841 C_*C)."""
    return name.endswith("]")


def is_single_only(name: str) -> bool:
    """Layers that only nnd_update_block_forward runs (update_block.hip:552-556: C_ZR1, C_Q1, C_ZR2, C_Q2)."""
    return name.startswith("gru.") and not name.endswith("]")


def is_fp16x2(name: str, kw: dict) -> bool:
    """Layers the plan gives the fp16x2 arithmetic (update_block.hip:73-76: convc1 only where its K is whole 16-channel chunks —
    36 correlation planes stay fp32 inside the fused lookup kernels; every other MFMA conv of the block)."""
    return name != "encoder.convc1" or kw["cor_planes"] % 16 == 0


def expected_range(M: float) -> float:
    """nnd_*_calibration_finish: xs = 11 - e with M = m * 2^e, m in [0.5, 1); the layer is valid for |x| < 65504 / 2^xs."""
    return 65504.0 * 2.0 ** (math.frexp(M)[1] - 11)


def power_of_two_margin(M: float) -> float:
    """Relative distance of M to the nearest power of two (0.01 = 1 %)."""
    m = math.frexp(M)[0]
    return min(m / 0.5 - 1.0, 1.0 / m - 1.0)


def make_case(name: str, seed: int = None):
    """-> (kw, gru, sd, prefix, (net, inp, corr, flow)): generated fp32 weights and seeded fp32 inputs at O(1) scale on the CPU."""
    kw, gru, seed0 = CASES[name]
    g = torch.Generator().manual_seed(1000 * NAMES.index(name) + (seed0 if seed is None else seed))
    prefix = "ub." + name
    sd = weightgen.fill_state_dict(R.update_block_spec(prefix, kw["hidden_dim"], kw["cor_planes"], kw["context_dim"],
                                                       kw["flow_channel"], kw["spatial_scale"], gru=gru))
    net = 0.9 * torch.tanh(torch.randn(B, kw["hidden_dim"], H, W, generator=g))
    inp = torch.relu(torch.randn(B, kw["context_dim"], H, W, generator=g))
    corr = torch.randn(B, kw["cor_planes"], H, W, generator=g)
    flow = 2.0 * torch.randn(B, kw["flow_channel"], H, W, generator=g)
    return kw, gru, sd, prefix, (net, inp, corr, flow)


def staged_maxima(sd, prefix: str, net, inp, corr, flow, gru: str = "sep_conv") -> Tuple[tuple, Dict[str, float]]:
    """One BasicUpdateBlock call in float64 -> ((net_out, mask, delta), {conv name: max |x| of what that conv stages})."""
    sd = {k: v.double() for k, v in sd.items()}
    net, inp, corr, flow = (x.double() for x in (net, inp, corr, flow))
    M: Dict[str, float] = {}

    def conv(name, x, padding=0):
        return F.conv2d(x, sd[f"{prefix}.{name}.weight"], sd[f"{prefix}.{name}.bias"], padding=padding)

    def rec(name, *tensors):
        M[name] = max(float(x.abs().max()) for x in tensors)

    rec("encoder.convc1", corr)
    cor = torch.relu(conv("encoder.convc1", corr))
    rec("encoder.convc2", cor)
    cor = torch.relu(conv("encoder.convc2", cor, 1))
    flo = torch.relu(conv("encoder.convf1", flow, 3))
    rec("encoder.convf2", flo)
    flo = torch.relu(conv("encoder.convf2", flo, 1))
    cf = torch.cat([cor, flo], 1)
    rec("encoder.conv", cf)
    motion = torch.cat([torch.relu(conv("encoder.conv", cf, 1)), flow], 1)
    h = net
    passes = (("1", (0, 2)), ("2", (2, 0))) if gru == "sep_conv" else (("1", 1),)
    for sfx, pad in passes:
        rec(f"gru.convz{sfx}+convr{sfx}", h, inp, motion)
        rec(f"gru.convz{sfx}+convr{sfx}[h,motion]", h, motion)
        rec(f"gru.convz{sfx}+convr{sfx}[inp]", inp)
        hx = torch.cat([h, inp, motion], 1)
        z = torch.sigmoid(conv("gru.convz" + sfx, hx, pad))
        r = torch.sigmoid(conv("gru.convr" + sfx, hx, pad))
        rec(f"gru.convq{sfx}", r * h, inp, motion)
        rec(f"gru.convq{sfx}[rh,motion]", r * h, motion)
        rec(f"gru.convq{sfx}[inp]", inp)
        q = torch.tanh(conv("gru.convq" + sfx, torch.cat([r * h, inp, motion], 1), pad))
        h = (1 - z) * h + z * q
    rec("flow_head.conv1+mask.0", h)
    delta = conv("flow_head.conv2", torch.relu(conv("flow_head.conv1", h, 1)), 1)
    m0 = torch.relu(conv("mask.0", h, 1))
    rec("mask.2", m0)
    mask = 0.25 * conv("mask.2", m0)
    return (h, mask, delta), M
