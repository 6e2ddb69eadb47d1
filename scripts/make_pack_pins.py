"""Pins of the host packers: for every case of CASES the sizes the library returns and the SHA-256 of the packed host blob.

    python scripts/make_pack_pins.py > pins.json

tests/test_pack_pins_cpu.py imports CASES / run_case from this file and compares against the output of this script as the commit
BEFORE a refactor of the packing code produced it (pasted into the test).  Weights come from nndepth_amd.weightgen and every blob
starts zero-filled, so a pin is a pure function of its case.  Host work only: no GPU is touched.
"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nndepth_amd import weightgen  # noqa: E402
from nndepth_amd._lib import Conv3dDesc, ConvDesc, EncoderDesc, UpdateBlockDesc, lib  # noqa: E402
from nndepth_amd.ops import LOFTR_KEYS  # noqa: E402

ARITH = {"fp32": 0, "bf16x3": 3, "fp16x2": 2}
BN = ("weight", "bias", "running_mean", "running_var")


def _t(key, shape):
    return weightgen.make_tensor("pins." + key, shape)


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _arr(tensors):
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _sha(blob):
    return hashlib.sha256(blob.numpy().tobytes()).hexdigest()


def _bn(key, c, on):
    return [_t(f"{key}.bn.{s}", (c,)) if on else None for s in BN]


# ------------------------------------------------------------------ update block
def _ub_tensors(hid, ctx, cp, fc, mc, gru):
    gin = 2 * hid + ctx
    k = (3, 3) if gru == "conv_gru" else (1, 5)
    convs = [("encoder.convc1", 256, cp, 1, 1), ("encoder.convc2", 192, 256, 3, 3), ("encoder.convf1", 128, fc, 7, 7),
             ("encoder.convf2", 64, 128, 3, 3), ("encoder.conv", hid - fc, 256, 3, 3)]
    convs += [(f"gru.conv{g}1", hid, gin, *k) for g in "zrq"]
    if gru == "sep_conv":
        convs += [(f"gru.conv{g}2", hid, gin, 5, 1) for g in "zrq"]
    convs += [("flow_head.conv1", hid, hid, 3, 3), ("flow_head.conv2", fc, hid, 3, 3), ("mask.0", 2 * hid, hid, 3, 3),
              ("mask.2", mc, 2 * hid, 1, 1)]
    out = []
    for name, co, ci, kh, kw in convs:
        out += [_t(f"ub.{name}.weight", (co, ci, kh, kw)), _t(f"ub.{name}.bias", (co,))]
    return out


def update_block(gru, hid, ctx, cp, fc, mc, arith, split_layers=0):
    d = UpdateBlockDesc(hid, ctx, cp, fc, mc, 0 if gru == "sep_conv" else 1, ARITH[arith], split_layers, 0)
    t = _ub_tensors(hid, ctx, cp, fc, mc, gru)
    assert lib.nnd_update_block_num_tensors(C.byref(d)) == len(t)
    n = lib.nnd_update_block_packed_floats(C.byref(d))
    blob = torch.zeros(n)
    assert lib.nnd_update_block_pack(C.byref(d), _arr(t), _ptr(blob)) == 0
    slots = (C.c_int64 * 64)()
    ns = lib.nnd_update_block_scale_slots(C.byref(d), slots, 64)
    return {"packed_floats": n, "workspace_floats": lib.nnd_update_block_workspace_floats(C.byref(d), 1, 68, 120),
            "scale_slots": list(slots[:ns]), "sha256": _sha(blob)}


# ------------------------------------------------------------------ single convs
def conv2d(cout, cin, kh, kw, arith):
    n = lib.nnd_conv2d_packed_floats_ex(cout, cin, kh, kw, ARITH[arith])
    if n < 0:  # the arithmetic does not accept the shape: pinned as a refusal
        return {"packed_floats": n}
    w, b, blob = _t("c2d.weight", (cout, cin, kh, kw)), _t("c2d.bias", (cout,)), torch.zeros(n)
    assert lib.nnd_conv2d_pack_ex(_ptr(w), _ptr(b), cout, cin, kh, kw, ARITH[arith], _ptr(blob)) == 0
    return {"packed_floats": n, "sha256": _sha(blob)}


def conv_norm(cout, cin, k, stride, bn, bias):
    d = ConvDesc(cout, cin, k, k, stride)
    n = lib.nnd_conv_packed_floats(C.byref(d))
    blob = torch.zeros(n)
    t = [_t("cn.weight", (cout, cin, k, k)), _t("cn.bias", (cout,)) if bias else None] + _bn("cn", cout, bn)
    assert lib.nnd_conv_pack(C.byref(d), *[_ptr(x) for x in t], 1e-5, _ptr(blob)) == 0
    return {"packed_floats": n, "sha256": _sha(blob)}


def conv3d(cout, cin0, cin1, stride, arith, bn=True, bias=False):
    d = Conv3dDesc(cout, cin0, cin1, stride, ARITH[arith], 0)
    n = lib.nnd_conv3d_packed_floats(C.byref(d))
    blob = torch.zeros(n)
    t = [_t("c3d.weight", (cout, cin0 + cin1, 3, 3, 3)), _t("c3d.bias", (cout,)) if bias else None] + _bn("c3d", cout, bn)
    assert lib.nnd_conv3d_pack(C.byref(d), *[_ptr(x) for x in t], 1e-5, _ptr(blob)) == 0
    return {"packed_floats": n, "sha256": _sha(blob)}


# ------------------------------------------------------------------ encoder, LoFTR
def encoder(norm, cnet_dim, arith, output_dim=256):
    d = EncoderDesc(output_dim, norm, cnet_dim, ARITH[arith], 0)
    units = [("conv1", (64, 3, 7, 7), True)]
    cin = 64
    for i, dim in enumerate((64, 64, 96, 96, 128, 128)):
        units += [(f"l{i}.conv1", (dim, cin, 3, 3), True), (f"l{i}.conv2", (dim, dim, 3, 3), True), (f"l{i}.down", (dim, cin, 1, 1), True)]
        cin = dim
    units.append(("conv2", (output_dim, 128, 1, 1), False))
    if cnet_dim > 0:
        units.append(("cnet", (cnet_dim, output_dim, 3, 3), False))
    t = []
    for name, shape, normed in units:
        t += [_t(f"enc.{name}.weight", shape), _t(f"enc.{name}.bias", shape[:1])] + _bn(f"enc.{name}", shape[0], normed and norm == 1)
    assert lib.nnd_encoder_num_tensors(C.byref(d)) == len(t)
    n = lib.nnd_encoder_packed_floats(C.byref(d))
    blob = torch.zeros(n)
    assert lib.nnd_encoder_pack(C.byref(d), _arr(t), 1e-5, _ptr(blob)) == 0
    return {"packed_floats": n, "workspace_floats": lib.nnd_encoder_workspace_floats(C.byref(d), 2, 544, 960), "sha256": _sha(blob)}


def loftr(d_model, nhead):
    c = d_model
    shapes = [(c, c)] * 4 + [(2 * c, 2 * c), (c, 2 * c)] + [(c,)] * 4
    t = [_t("loftr." + k, s) for k, s in zip(LOFTR_KEYS, shapes)]
    n = lib.nnd_loftr_packed_floats(d_model, nhead)
    blob = torch.zeros(n)
    assert lib.nnd_loftr_pack(d_model, nhead, _arr(t), _ptr(blob)) == 0
    return {"packed_floats": n, "workspace_floats": lib.nnd_loftr_workspace_floats(d_model, nhead, 1, 60, 80), "sha256": _sha(blob)}


# ------------------------------------------------------------------ the case list
# the (Cout, Cin0, Cin1, stride) of every Conv3d that igev_stereo.CostVolumeFilterNetwork(8, ...) constructs: J = 1, 2, 4 slices per
# launch element; thin only (fp32 / bf16x3), thin + slab (fp16x2), neither (Cout 32 / 64)
CONV3D_IGEV = [(16, 8, 0, 2), (16, 16, 0, 1), (32, 16, 0, 2), (32, 32, 0, 1), (64, 32, 0, 2), (64, 64, 0, 1), (32, 64, 0, 1),
               (32, 32, 32, 1), (16, 32, 0, 1), (16, 16, 16, 1), (8, 16, 0, 1), (8, 8, 0, 1)]
CONV2D_SHAPES = [(192, 256, 3, 3), (127, 256, 3, 3), (576, 256, 1, 1), (256, 36, 1, 1), (256, 320, 1, 5), (128, 320, 5, 1), (1, 128, 3, 3)]
UPDATE_BLOCKS = [("sep_conv", 128, 64, 36, 1, 576), ("conv_gru", 128, 128, 36, 2, 576), ("sep_conv", 128, 128, 576, 1, 144)]


def _cases():
    out = []
    for a in ARITH:
        out += [(update_block, ub + (a,)) for ub in UPDATE_BLOCKS]
        out += [(conv2d, s + (a,)) for s in CONV2D_SHAPES]
        out += [(encoder, (norm, cnet, a)) for norm in (0, 1, 2) for cnet in (0, 192)]
        out += [(conv3d, c + (a,)) for c in CONV3D_IGEV]
        out.append((conv3d, (8, 16, 0, 1, a, False, True)))  # no BatchNorm, with a bias
    out.append((update_block, UPDATE_BLOCKS[0] + ("fp16x2", 0x2 | 0x20 | 0x200)))  # split_layers: convc2, convq1[rh,motion], mask.2
    out += [(conv_norm, (96, 64, k, st, bn, bias)) for k in (3, 1) for st in (1, 2) for bn in (False, True) for bias in (True, False)]
    out.append((loftr, (256, 8)))
    return out


CASES = {f"{fn.__name__}-" + "-".join(str(int(a) if isinstance(a, bool) else a) for a in args): (fn, args) for fn, args in _cases()}


def run_case(case_id):
    fn, args = CASES[case_id]
    return fn(*args)


if __name__ == "__main__":
    print(json.dumps({k: run_case(k) for k in CASES}, indent=0, sort_keys=True))
