"""MobileNetV3DepthModel on the MI355X: the new kernels of csrc/midas.hip one at a time and the whole forward (one nnd_midas_forward
call) against float64, the drop-in model against the reference's fixture (tests/golden/midas_mbnet.npz), reproducibility, graph
replay, and the IGEVStereoMBNet encoder side that shares the backbone code.

Bars.  Against float64: err <= min(2 * e_torch, 1e-5 * maxabs), e_torch = the error of PyTorch fp32 on the same GPU against the same
float64 result (the rule of tests/test_gpu_igev_mbnet.py).  Against the fixture: err <= 2 * err64 + 1e-6 * maxabs per stored map,
err64 = the reference's own fp32-vs-float64 error.  The generated last_conv.4.bias (-0.045) clamps 76 % of the output to zero, so
the end-to-end comparisons run with last_conv.4.bias = +0.0107 and assert that at most 1 % of the reference's elements are zero;
one test keeps the generated bias for the clamp itself."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nndepth_amd import weightgen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "midas_mbnet.npz")
IGEV_GOLD = os.path.join(os.path.dirname(__file__), "golden", "igev_mbnet.npz")
SHIFT_BIAS = 0.0107
MAPS = ["tap0", "tap1", "tap2", "tap3", "decoder", "pre_relu", "depth"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def build(hip=True, shift=True, channels=64, prefix="midas."):
    from nndepth_amd.midas import MobileNetV3DepthModel
    m = MobileNetV3DepthModel(feature_channels=channels, hip=hip)
    weightgen.fill_module_(m, prefix)
    if shift:
        with torch.no_grad():
            m.last_conv[4].bias.fill_(SHIFT_BIAS)
    return m.eval().to(DEV)


def frame(B=1, H=128, W=192, seed=7):
    return weightgen.synthetic_frames(seed, B, H, W)[0].to(DEV)


def rand(tag, *shape, scale=1.0):
    n = int(np.prod(shape))
    return (torch.from_numpy(weightgen.uniform01(tag, n)).reshape(shape).float() * 2 - 1).mul(scale).to(DEV)


def up(t):
    return F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)


def judge(what, got, r64, p32):
    """err <= min(2 * e_torch, 1e-5 * maxabs) on the whole map and, separately, on its border rows / columns."""
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    for part, sl in (("all", (Ellipsis,)), ("row 0", (Ellipsis, 0, slice(None))), ("last row", (Ellipsis, -1, slice(None))),
                     ("col 0", (Ellipsis, 0)), ("last col", (Ellipsis, -1))):
        err = (got.double() - r64)[sl].abs().max().item()
        perr, mx = (p32.double() - r64).abs().max().item(), r64.abs().max().item()
        bar = min(2.0 * perr, 1e-5 * mx)
        print(f"{what} [{part}]: HIP vs float64 {err:.3e}, PyTorch fp32 (same GPU) vs float64 {perr:.3e}, bar {bar:.3e} (max-abs {mx:.4f})")
        assert err <= bar, (what, part, err, bar)


CASES = [(1, 16, 8, 16), (3, 64, 5, 48), (1, 128, 13, 80), (1, 64, 3, 5), (3, 16, 16, 16), (1, 96, 7, 48)]


# ------------------------------------------------------------------------------------------ the new kernels one at a time
@pytest.mark.parametrize("B,C,h,w", CASES)
def test_up2x_pw_kernel(B, C, h, w):
    from nndepth_amd import ops
    x = rand(f"upx{C}", B, C, h, w)
    wt, b = rand(f"upw{C}", C, C, 1, 1, scale=C ** -0.5), rand(f"upb{C}", C, scale=0.1)
    got = ops.midas_up2x_pw(x, wt, b)
    r64 = F.relu(F.conv2d(up(x.double()), wt.double(), b.double()))
    p32 = F.relu(F.conv2d(up(x), wt, b))
    assert (r64 == 0).double().mean().item() < 0.9
    judge(f"up2x_pw B{B} C{C} {h}x{w} -> {2 * h}x{2 * w}", got, r64, p32)


@pytest.mark.parametrize("B,C,h,w", CASES)
def test_head_kernel(B, C, h, w):
    from nndepth_amd import ops
    t = rand(f"hdx{C}", B, C, h, w)
    w2, b2 = rand(f"hdw2{C}", C, C, 3, 3, scale=(9 * C) ** -0.5), rand(f"hdb2{C}", C, scale=0.1)
    w4, b4 = rand(f"hdw4{C}", 1, C, 1, 1, scale=C ** -0.5), torch.full((1,), 0.02, device=DEV)
    packed = ops.midas_head_pack(w2, b2, w4, b4, DEV)
    depth, pre = ops.midas_head(t, packed, want_pre=True)

    def ref(t, cast):
        y = F.relu(F.conv2d(up(cast(t)), cast(w2), cast(b2), padding=1))
        return F.conv2d(y, cast(w4), cast(b4))

    r64, p32 = ref(t, lambda a: a.double()), ref(t, lambda a: a)
    judge(f"head pre-ReLU B{B} C{C} {h}x{w} -> {2 * h}x{2 * w}", pre, r64, p32)
    zeros = (r64 <= 0).double().mean().item()
    assert 0.02 < zeros < 0.98, zeros  # both sides of the final clamp are exercised
    assert torch.equal(depth, F.relu(pre))
    assert torch.equal(ops.midas_head(t, packed), depth)


@pytest.mark.parametrize("B,Cin,C,H,W", [(1, 24, 64, 32, 48), (3, 64, 64, 5, 7), (1, 160, 128, 4, 6), (1, 16, 16, 12, 20)])
def test_conv_add_kernel(B, Cin, C, H, W):
    from nndepth_amd import ops
    x, feat = rand(f"cax{Cin}", B, Cin, H, W), rand(f"caf{C}", B, C, H, W, scale=0.5)
    wt, b = rand(f"caw{Cin}{C}", C, Cin, 3, 3, scale=(9 * Cin) ** -0.5), rand(f"cab{C}", C, scale=0.1)
    got = ops.midas_conv_add(x, feat, wt, b)
    r64 = feat.double() + F.relu(F.conv2d(x.double(), wt.double(), b.double(), padding=1))
    p32 = feat + F.relu(F.conv2d(x, wt, b, padding=1))
    # the activation is BEFORE the addition: the other order gives something else on these inputs
    other = F.relu(feat.double() + F.conv2d(x.double(), wt.double(), b.double(), padding=1))
    assert (other - r64).abs().max().item() > 1e-2
    judge(f"conv_add B{B} {Cin}->{C} {H}x{W}", got, r64, p32)


# ------------------------------------------------------------------------------------------ whole forward against float64
@pytest.mark.parametrize("hw", [(384, 384), (96, 160)])
def test_forward_against_float64(hw):
    m = build()
    x = frame(1, *hw, seed=11)
    with torch.no_grad():
        depth, maps = m.forward_maps(x)
        maps = dict(maps, depth=depth)
        r64 = build(hip=False).double().forward_torch(x.double())
        p32 = build(hip=False).forward_torch(x)
    zeros = (r64["depth"] == 0).double().mean().item()
    assert zeros <= 0.01, zeros
    for name in MAPS:
        judge(f"{hw} {name}", maps[name], r64[name], p32[name])
    assert torch.equal(m(x), depth)


def test_forward_matches_reference_fixture(gold):
    m = build()
    with torch.no_grad():
        depth, maps = m.forward_maps(frame())
    maps = dict(maps, depth=depth)
    assert (gold["depth_shift"] == 0).mean() <= 0.01
    worst = 0.0
    for name in MAPS:
        key = name + "_shift" if name in ("pre_relu", "depth") else name
        a = maps[name].reshape(-1).double().cpu().numpy()
        err = np.abs(a[weightgen.sample_index(key, a.size, 4096)] - gold[key]).max()
        bar = 2.0 * float(gold[key + "_err64"]) + 1e-6 * float(gold[key + "_maxabs"])
        worst = max(worst, err / bar)
        print(f"{key}: HIP vs reference fixture {err:.3e}, reference fp32-vs-float64 {float(gold[key + '_err64']):.3e}, bar {bar:.3e}")
        assert err <= bar, (key, err, bar)
    print(f"worst error / bar = {worst:.3f}")


def test_final_clamp_with_generated_bias(gold):
    """The generator's own last_conv.4.bias: 76 % of the output is exactly zero.  The pre-ReLU map meets the fixture bar and the zero
    pattern agrees wherever |pre-ReLU| exceeds it."""
    m = build(shift=False)
    with torch.no_grad():
        depth, maps = m.forward_maps(frame())
    pre = maps["pre_relu"].reshape(-1).double().cpu().numpy()
    idx = weightgen.sample_index("pre_relu", pre.size, 4096)
    bar = 2.0 * float(gold["pre_relu_err64"]) + 1e-6 * float(gold["pre_relu_maxabs"])
    err = np.abs(pre[idx] - gold["pre_relu"]).max()
    print(f"pre_relu (generated bias): HIP vs reference fixture {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (err, bar)
    assert torch.equal(depth, F.relu(maps["pre_relu"]))
    got0 = (depth.reshape(-1) == 0).cpu().numpy()[idx]
    ref0 = gold["pre_relu"] <= 0
    assert 0.5 < ref0.mean() < 0.95, ref0.mean()  # the clamp is exercised on both sides
    sure = np.abs(gold["pre_relu"]) > bar
    print(f"zero pattern: {sure.sum()} of {sure.size} sampled elements decided beyond the bar, reference zeros {100 * ref0.mean():.1f} %")
    assert np.array_equal(got0[sure], ref0[sure])
    d = depth.reshape(-1).double().cpu().numpy()
    derr = np.abs(d[weightgen.sample_index("depth", d.size, 4096)] - gold["depth"]).max()
    assert derr <= 2.0 * float(gold["depth_err64"]) + 1e-6 * float(gold["depth_maxabs"]), derr


# ------------------------------------------------------------------------------------------ reproducibility, graph replay
def test_batch_and_repeat_are_bit_identical():
    m = build()
    x = frame(3, 96, 160, seed=3)
    with torch.no_grad():
        whole = m(x).clone()
        again = m(x).clone()
        singles = torch.cat([m(x[i:i + 1]).clone() for i in range(3)])
    assert torch.equal(whole, again)
    assert torch.equal(whole, singles)


def test_graphed_forward_is_bit_identical():
    from nndepth_amd.graph import GraphedForward
    m = build()
    x = frame(2, 96, 160, seed=5)
    with torch.no_grad():
        eager = m(x).clone()
        fwd = GraphedForward(m)
        assert torch.equal(fwd(x), eager)
        assert torch.equal(fwd(x), eager)


def test_other_feature_channels():
    x = frame(1, 64, 96, seed=2)
    for c in (16, 128):
        with torch.no_grad():
            got = build(channels=c)(x)
            r64 = build(hip=False, channels=c).double()(x.double())
            p32 = build(hip=False, channels=c)(x)
        judge(f"feature_channels {c}", got, r64, p32)


# ------------------------------------------------------------------------------------------ the shared backbone still serves IGEV
def test_igev_mbnet_encoder_side_still_matches_its_fixture():
    from nndepth_amd.igev_stereo import IGEVStereoMBNet
    g = dict(np.load(IGEV_GOLD))
    m = IGEVStereoMBNet(iters=4)
    weightgen.fill_module_(m, "igevmb.")
    m = m.eval().to(DEV)
    f1, f2 = weightgen.synthetic_frames(7, 1, 128, 192)
    with torch.no_grad():
        fm1, fm2, cn1, guides = m.forward_fnet(f1.to(DEV), f2.to(DEV))
    for name, t in zip(["fmap1", "fmap2", "cnet1", "guide0", "guide1", "guide2"], [fm1, fm2, cn1] + list(guides)):
        a = t.reshape(-1).double().cpu().numpy()
        err = np.abs(a[weightgen.sample_index(name, a.size, 4096)] - g[name]).max()
        bar = 2.0 * float(g[name + "_err64"]) + 1e-6 * float(g[name + "_maxabs"])
        print(f"{name}: HIP vs reference fixture {err:.3e}, bar {bar:.3e}")
        assert err <= bar, (name, err, bar)


def test_both_models_run_the_same_backbone_walk():
    """The two models share ONE backbone walk (mbv3.hip: mb_walk).  With the same MobilenetV3LargeEncoder weights in both, MiDaS'
    taps of stages 2 and 5 equal the stereo encoder side's guide0 and guide2 bit for bit on x = frame1.  B = 2: the stereo call
    runs stages 0..1 on 4 samples and stages 2..5 on 2, the MiDaS call runs 2 throughout (fixed split-K per layer, per-sample
    kernels: no output depends on the batch it runs in).  64x96 is the smallest size MiDaS accepts."""
    from nndepth_amd.igev_stereo import IGEVStereoMBNet
    from nndepth_amd.ops import MidasEngine, MobileNetV3Engine
    md = build()
    ig = IGEVStereoMBNet(iters=4)
    weightgen.fill_module_(ig, "igevmb.")
    ig.fnet.load_state_dict(md.encoder.state_dict(), strict=True)
    ig = ig.eval().to(DEV)
    assert list(md.encoder.feature_hooks) == [1, 2, 4, 5] and list(ig.fnet.feature_hooks) == [1, 2, 3, 4, 5]
    f1, f2 = (t.to(DEV) for t in weightgen.synthetic_frames(11, 2, 64, 96))
    with torch.no_grad():
        _, maps = MidasEngine.from_model(md, DEV).forward(f1, keep=True)
        _, _, _, guides = MobileNetV3Engine.from_modules(ig.fnet, ig.fnet_proj, ig.cnet_proj, DEV).forward(f1, f2)
    assert maps["tap1"].shape == guides[0].shape == (2, 40, 8, 12) and maps["tap3"].shape == guides[2].shape == (2, 160, 2, 3)
    assert maps["tap1"].abs().max().item() > 0 and maps["tap3"].abs().max().item() > 0
    assert torch.equal(maps["tap1"], guides[0])
    assert torch.equal(maps["tap3"], guides[2])
