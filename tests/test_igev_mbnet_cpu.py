"""IGEVStereoMBNet drop-in class and its MobileNetV3 encoder side, without a GPU: state_dict layout derived from timm's arch strings
and against the reference class (tests/golden/igev_mbnet.npz, scripts/make_golden_igev_mbnet.py), TF "same" padding of the
containers' forward, the host fold (ops.MobileNetV3Engine.fold) in float64, and the refusals of the C-ABI / Python side."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nndepth_amd import weightgen

GOLD = os.path.join(os.path.dirname(__file__), "golden", "igev_mbnet.npz")
# timm 1.0.16 _gen_mobilenet_v3("large"), written out independently of nndepth_amd.mobilenetv3
ARCH = [["ds_r1_k3_s1_e1_c16_nre"], ["ir_r1_k3_s2_e4_c24_nre", "ir_r1_k3_s1_e3_c24_nre"], ["ir_r3_k5_s2_e3_c40_se0.25_nre"],
        ["ir_r1_k3_s2_e6_c80", "ir_r1_k3_s1_e2.5_c80", "ir_r2_k3_s1_e2.3_c80"], ["ir_r2_k3_s1_e6_c112_se0.25"],
        ["ir_r3_k5_s2_e6_c160_se0.25"], ["cn_r1_k1_s1_c960"]]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def divisible(v, d=8):
    n = max(d, int(v + d / 2) // d * d)
    return n + d if n < 0.9 * v else n


def expected_layout():
    """(key, shape) of MobilenetV3LargeEncoder.backbone, derived from the arch strings with make_divisible."""
    def bn(p, c):
        return [(f"{p}.{n}", (c,)) for n in ("weight", "bias", "running_mean", "running_var")] + [(f"{p}.num_batches_tracked", ())]

    out = [("conv_stem.weight", (16, 3, 3, 3))] + bn("bn1", 16)
    cin = 16
    for si, stage in enumerate(ARCH):
        bi = 0
        for s in stage:
            o = {op[0]: op[1:] for op in s.split("_")[1:] if op != "nre"}
            kind, r, k, c = s.split("_")[0], int(o["r"]), int(o["k"]), int(o["c"])
            e = float(o.get("e", 1))
            se = float(s.split("_se")[1].split("_")[0]) if "_se" in s else 0.0
            for _ in range(r):
                p = f"blocks.{si}.{bi}"
                if kind == "ds":
                    out += [(f"{p}.conv_dw.weight", (cin, 1, k, k))] + bn(f"{p}.bn1", cin)
                    out += [(f"{p}.conv_pw.weight", (c, cin, 1, 1))] + bn(f"{p}.bn2", c)
                elif kind == "ir":
                    mid = divisible(cin * e)
                    out += [(f"{p}.conv_pw.weight", (mid, cin, 1, 1))] + bn(f"{p}.bn1", mid)
                    out += [(f"{p}.conv_dw.weight", (mid, 1, k, k))] + bn(f"{p}.bn2", mid)
                    if se:
                        rd = divisible(mid * se)
                        out += [(f"{p}.se.conv_reduce.weight", (rd, mid, 1, 1)), (f"{p}.se.conv_reduce.bias", (rd,)),
                                (f"{p}.se.conv_expand.weight", (mid, rd, 1, 1)), (f"{p}.se.conv_expand.bias", (mid,))]
                    out += [(f"{p}.conv_pwl.weight", (c, mid, 1, 1))] + bn(f"{p}.bn3", c)
                else:
                    out += [(f"{p}.conv.weight", (c, cin, k, k))] + bn(f"{p}.bn1", c)
                cin = c
                bi += 1
    return out


def build(**kw):
    from nndepth_amd.igev_stereo import IGEVStereoMBNet
    m = IGEVStereoMBNet(iters=4, **kw)
    weightgen.fill_module_(m, "igevmb.")
    return m.eval()


def test_backbone_layout_derived_from_arch_strings():
    from nndepth_amd.mobilenetv3 import MobilenetV3LargeEncoder
    sd = MobilenetV3LargeEncoder().state_dict()
    want = expected_layout()
    assert [(k[len("backbone."):], tuple(v.shape)) for k, v in sd.items()] == want
    # the widths the issue table lists: mid 64, 72, 72, 120, 240, 200, 184, 480, 672, 960; SE 24, 32, 120, 168, 240
    mids = {s for k, s in want if k.endswith("conv_pw.weight") and ".0.0." not in k}
    assert {s[0] for s in mids} >= {64, 72, 120, 240, 200, 184, 480, 672, 960}
    assert {s[0] for k, s in want if k.endswith("conv_reduce.weight")} == {24, 32, 120, 168, 240}


def test_state_dict_matches_reference_key_for_key(gold):
    m = build()
    sd = m.state_dict()
    assert list(sd.keys()) == list(gold["keys"])
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == list(gold["shapes"])
    ref_sd = {k: weightgen.make_tensor("ckpt." + k, tuple(int(x) for x in s.split(",") if x), sd[k].dtype)
              for k, s in zip(gold["keys"], gold["shapes"])}
    m.load_state_dict(ref_sd, strict=True)
    assert torch.equal(m.fnet.backbone.blocks[6][0].conv.weight, ref_sd["fnet.backbone.blocks.6.0.conv.weight"])


def test_registered_and_constructor():
    from nndepth_amd.igev_stereo import STEREO_MODELS, IGEVStereoMBNet
    assert STEREO_MODELS == {"igev_stereo_mbnet": IGEVStereoMBNet}
    m = IGEVStereoMBNet(update_cls="basic_update_block", cv_groups=8, iters=12, hidden_dim=64, context_dim=96, corr_levels=4,
                        corr_radius=4, tracing=False, include_preprocessing=False, weights=None, strict_load=True)
    assert m.hip_encoder and m.fnet_proj[0].out_channels == 128 and m.cnet_proj[0].out_channels == 192
    assert m.fnet.backbone.bn1.eps == 1e-3


def test_weights_load_through_constructor(tmp_path):
    from nndepth_amd.igev_stereo import IGEVStereoMBNet
    src = build()
    path = str(tmp_path / "ckpt.pt")
    torch.save({k: v.detach().clone() for k, v in src.state_dict().items()}, path)
    m = IGEVStereoMBNet(iters=4, weights=path)
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k


def ref_same_forward(enc, x):
    """The backbone in float64 with every conv padded by an explicit F.pad (TF same), written out apart from the containers."""
    bb = enc.backbone

    def conv(x, c, stride, groups=1):
        k = c.weight.shape[-1]
        H, W = x.shape[-2:]
        ph = max((math.ceil(H / stride) - 1) * stride + k - H, 0)
        pw = max((math.ceil(W / stride) - 1) * stride + k - W, 0)
        x = F.pad(x, [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2])
        return F.conv2d(x, c.weight, c.bias, stride, 0, 1, groups)

    def bn(x, b):
        return F.batch_norm(x, b.running_mean, b.running_var, b.weight, b.bias, False, 0.0, b.eps)

    x = F.hardswish(bn(conv(x, bb.conv_stem, 2), bb.bn1))
    feats = []
    for si, stage in enumerate(list(bb.blocks)[:6]):
        for blk in stage:
            sp = blk.spec
            act = F.relu if sp["relu"] else F.hardswish
            if sp["type"] == "ds":
                y = bn(conv(act(bn(conv(x, blk.conv_dw, sp["stride"], sp["cin"]), blk.bn1)), blk.conv_pw, 1), blk.bn2)
            else:
                y = act(bn(conv(x, blk.conv_pw, 1), blk.bn1))
                y = act(bn(conv(y, blk.conv_dw, sp["stride"], sp["mid"]), blk.bn2))
                if sp["rd"]:
                    s = F.relu(F.conv2d(y.mean((2, 3), keepdim=True), blk.se.conv_reduce.weight, blk.se.conv_reduce.bias))
                    y = y * F.relu6(F.conv2d(s, blk.se.conv_expand.weight, blk.se.conv_expand.bias) + 3) / 6
                y = bn(conv(y, blk.conv_pwl, 1), blk.bn3)
            x = x + y if sp["skip"] else y
        if si >= 1:
            feats.append(x)
    return feats


@pytest.mark.parametrize("hw", [(100, 148), (97, 131)])
def test_container_same_padding_at_odd_and_even_sizes(hw):
    m = build().double()
    x = torch.from_numpy(weightgen.uniform01(f"pad{hw}", 2 * 3 * hw[0] * hw[1]).reshape(2, 3, *hw)).double() * 2 - 1
    with torch.no_grad():
        got = m.fnet(x)
        ref = ref_same_forward(m.fnet, x)
    h, w = hw
    sizes = []
    for _ in range(5):
        h, w = -(-h // 2), -(-w // 2)
        sizes.append((h, w))
    want_hw = [sizes[1], sizes[2], sizes[3], sizes[3], sizes[4]]
    for i, (g, r, s) in enumerate(zip(got, ref, want_hw)):
        assert tuple(g.shape[-2:]) == s, (i, g.shape, s)
        err = (g - r).abs().max().item()
        assert err <= 1e-12 * max(1.0, r.abs().max().item()), (i, err)


def test_host_fold_reproduces_module_forward_in_float64():
    from nndepth_amd._lib import lib
    from nndepth_amd.ops import MobileNetV3Engine
    m = build().double()
    desc = MobileNetV3Engine.descriptor(m.fnet, m.fnet_proj, m.cnet_proj)
    layers = MobileNetV3Engine.fold(m.fnet, m.fnet_proj, m.cnet_proj)
    assert 2 * len(layers) == lib.nnd_mbv3_num_tensors(C.byref(desc))
    f1, f2 = weightgen.synthetic_frames(7, 2, 100, 148)
    f1, f2 = f1.double(), f2.double()
    with torch.no_grad():
        fm1, fm2, cn1, guides, _ = MobileNetV3Engine.fold_forward(layers, f1, f2)
        m.hip_encoder = False
        r = m.forward_fnet(f1, f2)
    for name, a, b in zip(["fmap1", "fmap2", "cnet1", "guide0", "guide1", "guide2"], [fm1, fm2, cn1] + guides, list(r[:3]) + r[3]):
        assert a.shape == b.shape, name
        rel = (a - b).abs().max().item() / b.abs().max().item()
        print(f"fold vs module forward, float64: {name} {tuple(a.shape)} rel {rel:.2e}")
        assert rel <= 1e-12, (name, rel)


def test_hip_encoder_false_matches_reference_encoder(gold):
    m = build(hip_encoder=False)
    f1, f2 = weightgen.synthetic_frames(7, 1, 128, 192)
    with torch.no_grad():
        fm1, fm2, cn1, guides = m.forward_fnet(f1, f2)
    for name, t in zip(["fmap1", "fmap2", "cnet1", "guide0", "guide1", "guide2"], [fm1, fm2, cn1] + guides):
        a = t.reshape(-1).double().numpy()
        err = np.abs(a[weightgen.sample_index(name, a.size, 4096)] - gold[name]).max()
        bar = 4.0 * float(gold[name + "_err64"]) + 1e-7 * float(gold[name + "_maxabs"])  # CPU fp32 drift across machines
        assert err <= bar, (name, err, bar)


def test_cabi_refuses_bad_descriptors_before_any_launch():
    from nndepth_amd._lib import MobileNetV3Desc, lib
    d = MobileNetV3Desc(fnet_dim=256, cnet_dim=256, flags=0)
    assert lib.nnd_mbv3_num_tensors(C.byref(d)) > 0 and lib.nnd_mbv3_packed_floats(C.byref(d)) > 0
    assert lib.nnd_mbv3_workspace_floats(C.byref(d), 1, 64, 96) > 0
    bad = MobileNetV3Desc.from_buffer_copy(d)
    bad.struct_size = 8
    assert lib.nnd_mbv3_num_tensors(C.byref(bad)) < 0
    assert b"struct_size" in lib.nnd_last_error()
    bad = MobileNetV3Desc.from_buffer_copy(d)
    bad.flags = 1
    assert lib.nnd_mbv3_packed_floats(C.byref(bad)) < 0
    bad = MobileNetV3Desc.from_buffer_copy(d)
    bad.fnet_dim = 0
    assert lib.nnd_mbv3_forward(C.byref(bad), None, None, None, None, None, None, None, None, None, None, 1, 64, 96, None) < 0
    assert b"fnet_dim" in lib.nnd_last_error()
    assert lib.nnd_mbv3_forward(C.byref(d), None, None, None, None, None, None, None, None, None, None, 1, 64, 96, None) < 0
    assert b"null" in lib.nnd_last_error()
    assert lib.nnd_mbv3_depthwise(None, None, None, None, None, 1, 1, 8, 8, 7, 1, 0, None) < 0
    assert lib.nnd_mbv3_pointwise_packed_floats(8, 8, 5) < 0


def test_python_side_names_what_it_refuses():
    from nndepth_amd._lib import NndError
    from nndepth_amd.ops import MobileNetV3Engine
    m = build()
    assert MobileNetV3Engine.blocker(m, m.fnet, m.fnet_proj, m.cnet_proj) is None
    saved = m.fnet.backbone.blocks[3][1]
    m.fnet.backbone.blocks[3][1] = torch.nn.Identity()
    why = MobileNetV3Engine.blocker(m, m.fnet, m.fnet_proj, m.cnet_proj)
    assert "blocks.3.1" in why
    with pytest.raises(NndError, match="blocks.3.1"):
        m(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
    m.fnet.backbone.blocks[3][1] = saved
    m.fnet_proj[0] = torch.nn.Conv2d(24, 256, 5, 1, 2)
    assert "fnet_proj" in MobileNetV3Engine.blocker(m, m.fnet, m.fnet_proj, m.cnet_proj)
    m2 = build()
    m2.train()
    assert "training" in MobileNetV3Engine.blocker(m2, m2.fnet, m2.fnet_proj, m2.cnet_proj)
    with pytest.raises(NndError, match="inference-only"):
        m2(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
    m2.eval()
    with pytest.raises(NndError, match="3, H, W"):  # a non-3-channel input, refused before any launch
        m2.forward_fnet(torch.zeros(1, 1, 64, 64), torch.zeros(1, 1, 64, 64))
    with pytest.raises(NndError):  # the HIP path refuses a CPU run, never falls back
        m2(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
