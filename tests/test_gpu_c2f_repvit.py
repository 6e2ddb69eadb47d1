"""Coarse2FineGroupRepViTRAFTStereo on the MI355X: the HIP encoder side (csrc/repvit.hip, one nnd_repvit_forward call) against the
reference's maps (tests/golden/c2f_repvit.npz) and against the containers' forward in float64, and the drop-in model end to end."""
import os

import numpy as np
import pytest
import torch

from nndepth_amd import weightgen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "c2f_repvit.npz")
CONFIGS = {
    "default": dict(corr_levels=1),
    "alt": dict(corr_levels=1, context_dim=64, hidden_dim=64, num_blocks_per_stage=[1, 2, 1, 1],
                token_mixer_types=["repmixer", "attention", "repmixer", "attention"], use_ffn_per_stage=[True, True, False, True]),
}
SIDE = ["fnet4", "fused1", "fused2", "cnet0", "cnet1", "cnet2"]  # what the HIP call writes: feats[0..2], cnets[0..2]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def build(cfg="default", **kw):
    from nndepth_amd.raft_stereo import Coarse2FineGroupRepViTRAFTStereo
    m = Coarse2FineGroupRepViTRAFTStereo(iters=4, **CONFIGS[cfg], **kw)
    weightgen.fill_module_(m, "c2frv.")
    return m.eval().to(DEV)


def frames(B=1, H=128, W=192, seed=3):
    f1, f2 = weightgen.synthetic_frames(seed, B, H, W)
    return f1.to(DEV), f2.to(DEV)


def side_maps(feats, cnets):
    return dict(zip(SIDE, list(feats) + list(cnets)))


def north_star(err, mag):
    return 1e-4 * max(1.0, mag / 25.8)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_encoder_side_matches_reference(gold, cfg):
    m = build(cfg)
    f1, f2 = frames()
    with torch.no_grad():
        feats, cnets = m.forward_features(f1, f2)
    torch.cuda.synchronize()
    for name, t in side_maps(feats, cnets).items():
        key = f"{cfg}_{name}"
        a = t.reshape(-1).double().cpu().numpy()
        got = a[weightgen.sample_index(key, a.size, 4096)]
        err = np.abs(got - gold[key]).max()
        mx = float(gold[key + "_maxabs"])
        bar = min(2.0 * float(gold[key + "_err64"]), 1e-5 * mx)  # 2x the fp32 reference's own error vs float64, capped
        print(f"[{cfg}] {name}: HIP vs reference {err:.3e}, reference fp32-vs-float64 {float(gold[key + '_err64']):.3e}, "
              f"bar {bar:.3e} (max-abs {mx:.3f})")
        assert err <= bar, (cfg, name, err, bar)


def test_encoder_side_512x960_against_float64():
    from nndepth_amd.raft_stereo import Coarse2FineRAFTStereoBase
    m = build()
    f1, f2 = frames(1, 512, 960, seed=1)
    with torch.no_grad():
        feats, cnets = m.forward_features(f1, f2)
        m64 = build(hip_encoder=False).double()
        r_feats, r_cnets = Coarse2FineRAFTStereoBase.forward_features(m64, f1.double(), f2.double())
        m32 = build(hip_encoder=False)
        p_feats, p_cnets = Coarse2FineRAFTStereoBase.forward_features(m32, f1, f2)
    for name, t, r, p in zip(SIDE, feats + cnets, r_feats + r_cnets, p_feats + p_cnets):
        err = (t.double() - r).abs().max().item()
        perr = (p.double() - r).abs().max().item()
        mx = r.abs().max().item()
        bar = min(2.0 * perr, 1e-5 * mx)
        print(f"512x960 {name} {tuple(t.shape)}: HIP vs float64 {err:.3e}, PyTorch fp32 (same GPU) vs float64 {perr:.3e}, "
              f"bar {bar:.3e} (max-abs {mx:.3f})")
        assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("arith", ["fp32", "fp16x2"])
def test_end_to_end_against_reference(gold, arith):
    m = build(arithmetic=arith)
    f1, f2 = frames()
    out = m(f1, f2)
    assert len(out) == 12
    worst = 0.0
    for i, o in enumerate(out):
        key = f"up{i}"
        a = o["up_disp"].reshape(-1).double().cpu().numpy()
        got = a[weightgen.sample_index(key, a.size, 4096)]
        err = np.abs(got - gold[key]).max()
        bar = north_star(err, float(gold[key + "_maxabs"]))
        worst = max(worst, err / bar)
        assert err <= bar, (arith, i, err, bar)
    print(f"{arith}: worst up_disp error / bar = {worst:.3f} (margin {1 / max(worst, 1e-12):.1f}x)")


def test_hip_encoder_against_pytorch_encoder():
    m = build(arithmetic="fp32")
    f1, f2 = frames(seed=5)
    out = m(f1, f2)
    m.hip_encoder = False
    ref = m(f1, f2)
    for a, b in zip(out, ref):
        err = (a["up_disp"] - b["up_disp"]).abs().max().item()
        assert err <= north_star(err, b["up_disp"].abs().max().item()), err
    print(f"hip_encoder True vs False: final up_disp diff {err:.3e}")


def test_last_equals_all_and_graph_equals_eager():
    from nndepth_amd.graph import GraphedForward
    m = build(arithmetic="fp16x2")
    f1, f2 = frames()
    all_ = m(f1, f2)
    m.outputs = "last"
    last = m(f1, f2)
    assert len(last) == 1 and torch.equal(last[0]["up_disp"], all_[-1]["up_disp"])
    m.outputs = "all"
    eager = m(f1, f2)
    g = GraphedForward(m)
    for _ in range(3):
        rep = g(f1, f2)
    torch.cuda.synchronize()
    assert all(torch.equal(a["up_disp"], b["up_disp"]) for a, b in zip(eager, rep))


def test_batch_and_repeat_are_bit_identical():
    m = build(arithmetic="fp32")
    fa, fb = frames(1, 128, 192, seed=3), frames(1, 128, 192, seed=4)
    f1, f2 = torch.cat([fa[0], fb[0]]), torch.cat([fa[1], fb[1]])
    with torch.no_grad():
        bf, bc = m.forward_features(f1, f2)
        af, ac = m.forward_features(*fa)
        xf, xc = m.forward_features(*fb)
        again, _ = m.forward_features(f1, f2)
    for j in range(3):
        assert torch.equal(bf[j], again[j])
        assert torch.equal(bf[j][[0, 2]], af[j]) and torch.equal(bf[j][[1, 3]], xf[j])  # batch order [l0, l1, r0, r1]
        assert torch.equal(bc[j][:1], ac[j]) and torch.equal(bc[j][1:], xc[j])
    outs = m(f1, f2)
    single = m(*fa)
    err = (outs[-1]["up_disp"][:1] - single[-1]["up_disp"]).abs().max().item()
    assert err <= north_star(err, single[-1]["up_disp"].abs().max().item()), err


def test_patch_coarse2fine_hip_encoder_equals_drop_in():
    import copy
    from nndepth_amd.raft_stereo import patch_coarse2fine
    m = build(arithmetic="fp32")
    ref_shaped = copy.deepcopy(m)
    ref_shaped.hip_encoder = False
    patch_coarse2fine(ref_shaped, arithmetic="fp32", hip_encoder=True)
    f1, f2 = frames()
    a = m(f1, f2)
    b = ref_shaped(f1, f2)
    assert all(torch.equal(x["up_disp"], y["up_disp"]) for x, y in zip(a, b))



# ------------------------------------------------------------------------------------------ per kernel, against float64
# Each kernel through its own entry point (the launchers nnd_repvit_forward uses), on odd sizes and the channel counts of the model;
# bar: the HIP error at most 2x the error of PyTorch's own fp32 evaluation of the same op on the same GPU, both printed.
def _call(name, *args):
    from nndepth_amd._lib import check, lib
    from nndepth_amd.ops import _stream
    check(getattr(lib, name)(*args, _stream(torch.device(DEV))), name)
    torch.cuda.synchronize()


def _p(t):
    from nndepth_amd.ops import _p as p
    return p(t)


def _judge(what, hip, f32, f64):
    e_hip = (hip.double() - f64).abs().max().item()
    e_pt = (f32.double() - f64).abs().max().item()
    print(f"{what}: HIP vs float64 {e_hip:.3e}, PyTorch fp32 vs float64 {e_pt:.3e} (max-abs {f64.abs().max().item():.3f})")
    assert e_hip <= 2.0 * e_pt, (what, e_hip, e_pt)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C", [16, 32, 128, 256])
@pytest.mark.parametrize("gelu", [False, True])
def test_kernel_depthwise(k, stride, C, gelu):
    F = torch.nn.functional
    N, H, W = 2, 37, 53
    x = _rand(N, C, H, W, seed=1)
    w = _rand(C, 1, k, k, seed=2, scale=(1.0 / k))
    b = _rand(C, seed=3, scale=0.1)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty(N, C, Ho, Wo, device=DEV)
    _call("nnd_repvit_depthwise", _p(x), _p(w), _p(b), _p(y), N, C, H, W, k, stride, int(gelu))

    def ref(x, w, b):
        r = F.conv2d(x, w, b, stride=stride, padding=k // 2, groups=C)
        return F.gelu(r) if gelu else r
    f64 = ref(x.double(), w.double(), b.double())
    assert y.shape == f64.shape
    _judge(f"depthwise k{k} s{stride} C{C} {N}x{H}x{W}{' GELU' if gelu else ''}", y, ref(x, w, b), f64)


@pytest.mark.parametrize("stride", [1, 2])
def test_kernel_stem(stride):
    F = torch.nn.functional
    N, H, W = 2, 37, 53
    x, x1 = _rand(1, 3, H, W, seed=4), _rand(1, 3, H, W, seed=5)
    w, b = _rand(16, 3, 3, 3, seed=6, scale=0.3), _rand(16, seed=7, scale=0.1)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty(N, 16, Ho, Wo, device=DEV)
    _call("nnd_repvit_stem", _p(x), _p(x1), 1, _p(w), _p(b), _p(y), N, H, W, stride)
    xx = torch.cat([x, x1])

    def ref(x, w, b):
        return F.gelu(F.conv2d(x, w, b, stride=stride, padding=1))
    _judge(f"stem 3x3 3->16 s{stride} {N}x{H}x{W}", y, ref(xx, w, b), ref(xx.double(), w.double(), b.double()))


@pytest.mark.parametrize("cin,cout,stride,mode", [(64, 192, 1, "gelu"), (256, 1024, 1, "gelu"), (16, 16, 2, "gelu"),
                                                  (384, 128, 1, "resid"), (128, 257, 1, "none")])
def test_kernel_pointwise(cin, cout, stride, mode):
    F = torch.nn.functional
    from nndepth_amd._lib import check, lib
    N, H, W = 2, 37, 53
    x = _rand(N, cin, H, W, seed=8)
    w = _rand(cout, cin, 1, 1, seed=9, scale=cin ** -0.5)
    b = _rand(cout, seed=10, scale=0.1)
    ls = _rand(cout, seed=11) if mode == "resid" else None
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    res = _rand(N, cout, Ho, Wo, seed=12) if mode == "resid" else None
    bias_packed = (ls.double() * b.double()).float() if mode == "resid" else b
    n = int(lib.nnd_repvit_pointwise_packed_floats(cout, cin, stride))
    blob = torch.empty(n, dtype=torch.float32)
    wc, bc, lc = w.cpu().contiguous(), bias_packed.cpu().contiguous(), None if ls is None else ls.cpu().contiguous()
    check(lib.nnd_repvit_pointwise_pack(cout, cin, stride, _p(wc), _p(bc), _p(lc), _p(blob)), "pointwise_pack")
    blob = blob.to(DEV)
    y = torch.empty(N, cout, Ho, Wo, device=DEV)
    _call("nnd_repvit_pointwise", cout, cin, stride, _p(blob), _p(x), _p(res), _p(y), N, H, W, int(mode == "gelu"))

    def ref(x, w, b, ls, res):
        r = F.conv2d(x, w, b, stride=stride)
        if mode == "gelu":
            return F.gelu(r)
        if mode == "resid":
            return res + ls.reshape(1, -1, 1, 1) * r
        return r
    d = lambda t: None if t is None else t.double()  # noqa: E731
    _judge(f"pointwise {cin}->{cout} s{stride} {mode} {N}x{H}x{W}", y, ref(x, w, b, ls, res), ref(d(x), d(w), d(b), d(ls), d(res)))


@pytest.mark.parametrize("W", [1, 3, 15])
@pytest.mark.parametrize("C", [128, 256])
def test_kernel_linear_attention(W, C):
    F = torch.nn.functional
    N, H = 2, 5
    qkv = _rand(N, 1 + 2 * C, H, W, seed=13)
    out = torch.empty(N, C, H, W, device=DEV)
    _call("nnd_repvit_linear_attention", _p(qkv), _p(out), N, C, H, W)

    def ref(qkv):
        q, k, v = torch.split(qkv, [1, C, C], dim=1)
        return F.relu(v) * (k * F.softmax(q, dim=-1)).sum(-1, keepdim=True)
    _judge(f"linear attention C{C} {N}x{H}x{W}", out, ref(qkv), ref(qkv.double()))


@pytest.mark.parametrize("hw,HW", [((8, 15), (32, 60)), ((2, 3), (8, 12)), ((5, 7), (17, 23)), ((9, 14), (32, 48))])
def test_kernel_fusion_upsample(hw, HW):
    F = torch.nn.functional
    N, C = 2, 64
    a = _rand(N, C, *hw, seed=14)
    fine = _rand(N, C, *HW, seed=15)
    y = fine.clone()
    _call("nnd_repvit_upsample_add_relu", _p(a), _p(y), N, C, hw[0], hw[1], HW[0], HW[1])

    def ref(a, fine):
        return F.relu(fine + F.interpolate(a, size=HW, mode="bilinear", align_corners=False))
    _judge(f"fusion upsample {hw} -> {HW} (x{HW[0] / hw[0]:.3g}, x{HW[1] / hw[1]:.3g})", y, ref(a, fine), ref(a.double(), fine.double()))


def test_fusion_block_at_a_non_integer_ratio():
    """A whole FeatureFusionBlock pair through the encoder side at a frame size whose stage maps are not 4x apart (odd sizes)."""
    from nndepth_amd.raft_stereo import Coarse2FineRAFTStereoBase
    m = build()
    f1, f2 = frames(1, 100, 148, seed=2)  # stem 25x37, stage 1 7x10, stage 3 2x3: ratios 3.57 / 3.5 and 3.7 / 3.33
    with torch.no_grad():
        feats, cnets = m.forward_features(f1, f2)
        r_feats, r_cnets = Coarse2FineRAFTStereoBase.forward_features(build(hip_encoder=False).double(), f1.double(), f2.double())
        p_feats, p_cnets = Coarse2FineRAFTStereoBase.forward_features(build(hip_encoder=False), f1, f2)
    for name, t, r, p in zip(SIDE, feats + cnets, r_feats + r_cnets, p_feats + p_cnets):
        assert t.shape == r.shape, (name, t.shape, r.shape)
        err, perr, mx = (t.double() - r).abs().max().item(), (p.double() - r).abs().max().item(), r.abs().max().item()
        bar = min(2.0 * perr, 1e-5 * mx)
        print(f"100x148 {name} {tuple(t.shape)}: HIP vs float64 {err:.3e}, PyTorch fp32 vs float64 {perr:.3e}, bar {bar:.3e}")
        assert err <= bar, (name, err, bar)
