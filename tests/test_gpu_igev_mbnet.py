"""IGEVStereoMBNet on the MI355X: the HIP MobileNetV3 encoder side (csrc/mbv3.hip, one nnd_mbv3_forward call) kernel by kernel and as
a whole against float64, and the drop-in model end to end against the reference's fixture (tests/golden/igev_mbnet.npz)."""
import os

import numpy as np
import pytest
import torch

from nndepth_amd import weightgen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "igev_mbnet.npz")
SIDE = ["fmap1", "fmap2", "cnet1", "guide0", "guide1", "guide2"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def build(**kw):
    from nndepth_amd.igev_stereo import IGEVStereoMBNet
    m = IGEVStereoMBNet(iters=4, **kw)
    weightgen.fill_module_(m, "igevmb.")
    return m.eval().to(DEV)


def frames(B=1, H=128, W=192, seed=7):
    f1, f2 = weightgen.synthetic_frames(seed, B, H, W)
    return f1.to(DEV), f2.to(DEV)


def flat(out):
    fm1, fm2, cn1, guides = out
    return [fm1, fm2, cn1] + list(guides)


def north_star(err, mag):
    return 1e-4 * max(1.0, mag / 25.8)


# ------------------------------------------------------------------------------------------ encoder side against float64
@pytest.mark.parametrize("hw", [(544, 960), (100, 148)])
def test_encoder_side_against_float64(hw):
    m = build()
    f1, f2 = frames(1, *hw, seed=1)
    with torch.no_grad():
        got = flat(m.forward_fnet(f1, f2))
        r = flat(build(hip_encoder=False).double().forward_fnet(f1.double(), f2.double()))
        p = flat(build(hip_encoder=False).forward_fnet(f1, f2))
    for name, t, r64, p32 in zip(SIDE, got, r, p):
        assert t.shape == r64.shape, (name, t.shape, r64.shape)
        err, perr, mx = (t.double() - r64).abs().max().item(), (p32.double() - r64).abs().max().item(), r64.abs().max().item()
        bar = min(2.0 * perr, 1e-5 * mx)
        print(f"{hw} {name} {tuple(t.shape)}: HIP vs float64 {err:.3e}, PyTorch fp32 (same GPU) vs float64 {perr:.3e}, "
              f"bar {bar:.3e} (max-abs {mx:.3f})")
        assert err <= bar, (hw, name, err, bar)


def test_encoder_side_matches_reference_fixture(gold):
    m = build()
    f1, f2 = frames()
    with torch.no_grad():
        got = flat(m.forward_fnet(f1, f2))
    for name, t in zip(SIDE, got):
        a = t.reshape(-1).double().cpu().numpy()
        err = np.abs(a[weightgen.sample_index(name, a.size, 4096)] - gold[name]).max()
        bar = 2.0 * float(gold[name + "_err64"]) + 1e-6 * float(gold[name + "_maxabs"])
        print(f"{name}: HIP vs reference fixture {err:.3e}, reference fp32-vs-float64 {float(gold[name + '_err64']):.3e}, bar {bar:.3e}")
        assert err <= bar, (name, err, bar)


# ------------------------------------------------------------------------------------------ the model end to end
@pytest.mark.parametrize("arith", ["fp32", "bf16x3", "fp16x2"])
def test_end_to_end_against_reference(gold, arith):
    m = build(arithmetic=arith)
    f1, f2 = frames()
    out = m(f1, f2)
    assert len(out) == 4
    worst = 0.0
    for i, o in enumerate(out):
        key = f"up{i}"
        a = o["up_disp"].reshape(-1).double().cpu().numpy()
        err = np.abs(a[weightgen.sample_index(key, a.size, 4096)] - gold[key]).max()
        bar = north_star(err, float(gold[key + "_maxabs"]))
        worst = max(worst, err / bar)
        assert err <= bar, (arith, i, err, bar)
    print(f"{arith}: worst up_disp error / bar = {worst:.3f} (margin {1 / max(worst, 1e-12):.1f}x)")


def test_hip_encoder_against_pytorch_encoder():
    m = build(arithmetic="fp32")
    f1, f2 = frames(1, 480, 640, seed=5)
    out = m(f1, f2)
    m.hip_encoder = False
    ref = m(f1, f2)
    for a, b in zip(out, ref):
        err = (a["up_disp"] - b["up_disp"]).abs().max().item()
        assert err <= north_star(err, b["up_disp"].abs().max().item()), err
    print(f"hip_encoder True vs False at 480x640: final up_disp diff {err:.3e}")


def test_batch_and_repeat_are_bit_identical():
    m = build(arithmetic="fp32")
    fs = [frames(1, 128, 192, seed=s) for s in (3, 4, 7)]
    f1, f2 = torch.cat([f[0] for f in fs]), torch.cat([f[1] for f in fs])
    with torch.no_grad():
        batch = flat(m.forward_fnet(f1, f2))
        again = flat(m.forward_fnet(f1, f2))
        alone = flat(m.forward_fnet(*fs[1]))
    for name, b, a, s in zip(SIDE, batch, again, alone):
        assert torch.equal(b, a), name
        assert torch.equal(b[1:2], s), name
    outs = m(f1, f2)
    single = m(*fs[1])
    err = (outs[-1]["up_disp"][1:2] - single[-1]["up_disp"]).abs().max().item()
    assert err <= north_star(err, single[-1]["up_disp"].abs().max().item()), err


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


def test_refusals_before_any_launch():
    from nndepth_amd._lib import NndError
    m = build()
    f1, f2 = frames()
    m.train()
    with pytest.raises(NndError, match="inference-only|eval"):
        m(f1, f2)
    m.eval()
    m.fnet.backbone.blocks[4][1] = torch.nn.Identity()
    with pytest.raises(NndError, match="blocks.4.1"):
        m(f1, f2)
    m = build()
    with pytest.raises(NndError, match="3, H, W"):
        m.forward_fnet(f1[:, :1], f2[:, :1])
    torch.cuda.synchronize()


def test_reference_smoke_mirror():
    """The reference's own smoke: IGEVStereoMBNet() with default kwargs on torch.rand 480x640 frames."""
    from nndepth_amd.igev_stereo import IGEVStereoMBNet
    m = IGEVStereoMBNet().eval().to(DEV)
    f1, f2 = torch.rand(1, 3, 480, 640, device=DEV), torch.rand(1, 3, 480, 640, device=DEV)
    out = m(f1, f2)
    assert isinstance(out, list) and len(out) == m.iters
    for o in out:
        assert tuple(o["up_disp"].shape) == (1, 1, 480, 640) and torch.isfinite(o["up_disp"]).all()


# ------------------------------------------------------------------------------------------ per kernel, against float64
# Each kernel through its own entry point (the launchers nnd_mbv3_forward uses), at even and odd sizes; bar: the HIP error at most
# 2x the error of PyTorch's own fp32 evaluation of the same op on the same GPU, both printed.
ACTS = {0: lambda t: t, 1: torch.relu, 2: torch.nn.functional.hardswish}


def _call(name, *args):
    from nndepth_amd._lib import check, lib
    from nndepth_amd.ops import _stream
    check(getattr(lib, name)(*args, _stream(torch.device(DEV))), name)
    torch.cuda.synchronize()


def _p(t):
    from nndepth_amd.ops import _p as p
    return p(t)


def _judge(what, hip, f32, f64):
    assert hip.shape == f64.shape, (what, hip.shape, f64.shape)
    e_hip = (hip.double() - f64).abs().max().item()
    e_pt = (f32.double() - f64).abs().max().item()
    print(f"{what}: HIP vs float64 {e_hip:.3e}, PyTorch fp32 vs float64 {e_pt:.3e} (max-abs {f64.abs().max().item():.3f})")
    assert e_hip <= 2.0 * e_pt, (what, e_hip, e_pt)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _same(x, k, s):
    from nndepth_amd.mobilenetv3 import same_pad
    return same_pad(x, k, s)


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", [(36, 52), (37, 53)])
@pytest.mark.parametrize("C,act", [(72, 1), (240, 2), (16, 0)])
def test_kernel_depthwise(k, stride, hw, C, act):
    F = torch.nn.functional
    N, (H, W) = 2, hw
    x = _rand(N, C, H, W, seed=1)
    w = _rand(C, 1, k, k, seed=2, scale=1.0 / k)
    b = _rand(C, seed=3, scale=0.1)
    Ho, Wo = -(-H // stride), -(-W // stride)
    y = torch.empty(N, C, Ho, Wo, device=DEV)
    _call("nnd_mbv3_depthwise", _p(x), _p(w), _p(b), _p(y), None, N, C, H, W, k, stride, act)

    def ref(x, w, b):
        return ACTS[act](F.conv2d(_same(x, k, stride), w, b, stride=stride, groups=C))
    _judge(f"depthwise k{k} s{stride} C{C} act{act} {N}x{H}x{W}", y, ref(x, w, b), ref(x.double(), w.double(), b.double()))


@pytest.mark.parametrize("hw", [(36, 52), (37, 53), (544, 960)])
def test_kernel_stem(hw):
    F = torch.nn.functional
    N, (H, W) = 2, hw
    x, x1 = _rand(1, 3, H, W, seed=4), _rand(1, 3, H, W, seed=5)
    w, b = _rand(16, 3, 3, 3, seed=6, scale=0.3), _rand(16, seed=7, scale=0.1)
    y = torch.empty(N, 16, -(-H // 2), -(-W // 2), device=DEV)
    _call("nnd_mbv3_stem", _p(x), _p(x1), 1, _p(w), _p(b), _p(y), N, H, W)
    xx = torch.cat([x, x1])

    def ref(x, w, b):
        return F.hardswish(F.conv2d(_same(x, 3, 2), w, b, stride=2))
    _judge(f"stem 3x3 s2 3->16 {N}x{H}x{W}", y, ref(xx, w, b), ref(xx.double(), w.double(), b.double()))


@pytest.mark.parametrize("C,rd,k,stride,hw,act", [(72, 24, 5, 2, (67, 119), 1), (120, 32, 5, 1, (34, 60), 1),
                                                  (672, 168, 3, 1, (17, 30), 2), (960, 240, 5, 1, (9, 15), 2)])
def test_kernel_squeeze_excite(C, rd, k, stride, hw, act):
    """depthwise with the SE partial sums, then the SE gate applied in place: act(dw(x)) * hardsigmoid(...)."""
    F = torch.nn.functional
    from nndepth_amd._lib import lib
    N, (H, W) = 2, hw
    x = _rand(N, C, H, W, seed=8)
    w, b = _rand(C, 1, k, k, seed=9, scale=1.0 / k), _rand(C, seed=10, scale=0.1)
    wr, br = _rand(rd, C, seed=11, scale=C ** -0.5), _rand(rd, seed=12, scale=0.1)
    we, be = _rand(C, rd, seed=13, scale=2 * rd ** -0.5), _rand(C, seed=14, scale=0.5)
    Ho, Wo = -(-H // stride), -(-W // stride)
    y = torch.empty(N, C, Ho, Wo, device=DEV)
    part = torch.empty(int(lib.nnd_mbv3_se_partials(N, C, Ho, Wo)), dtype=torch.float64, device=DEV)
    gate = torch.empty(N, C, device=DEV)
    _call("nnd_mbv3_depthwise", _p(x), _p(w), _p(b), _p(y), _p(part), N, C, H, W, k, stride, act)
    _call("nnd_mbv3_se", _p(y), _p(part), _p(wr), _p(br), _p(we), _p(be), _p(gate), N, C, rd, Ho, Wo)

    def ref(x, w, b, wr, br, we, be):
        t = ACTS[act](F.conv2d(_same(x, k, stride), w, b, stride=stride, groups=C))
        s = F.relu(F.conv2d(t.mean((2, 3), keepdim=True), wr[:, :, None, None], br))
        return t * F.hardsigmoid(F.conv2d(s, we[:, :, None, None], be))
    args = (x, w, b, wr, br, we, be)
    _judge(f"SE C{C} rd{rd} dw k{k} s{stride} {N}x{H}x{W}", y, ref(*args), ref(*[a.double() for a in args]))
    # bit-reproducible: the same call again
    y2 = torch.empty_like(y)
    _call("nnd_mbv3_depthwise", _p(x), _p(w), _p(b), _p(y2), _p(part), N, C, H, W, k, stride, act)
    _call("nnd_mbv3_se", _p(y2), _p(part), _p(wr), _p(br), _p(we), _p(be), _p(gate), N, C, rd, Ho, Wo)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("cin,cout,k,mode", [(16, 64, 1, "relu"), (80, 480, 1, "hswish"), (112, 672, 1, "hswish"),
                                             (960, 160, 1, "resid"), (72, 40, 1, "none"), (16, 16, 1, "resid"),
                                             (24, 256, 3, "relu"), (24, 96, 3, "relu")])
def test_kernel_pointwise(cin, cout, k, mode):
    F = torch.nn.functional
    from nndepth_amd._lib import check, lib
    N, H, W = 2, 37, 53
    x = _rand(N, cin, H, W, seed=15)
    w = _rand(cout, cin, k, k, seed=16, scale=(cin * k * k) ** -0.5)
    b = _rand(cout, seed=17, scale=0.1)
    res = _rand(N, cout, H, W, seed=18) if mode == "resid" else None
    act = {"none": 0, "resid": 0, "relu": 1, "hswish": 2}[mode]
    n = int(lib.nnd_mbv3_pointwise_packed_floats(cout, cin, k))
    blob = torch.empty(n, dtype=torch.float32)
    wc, bc = w.cpu().contiguous(), b.cpu().contiguous()
    check(lib.nnd_mbv3_pointwise_pack(cout, cin, k, _p(wc), _p(bc), _p(blob)), "pointwise_pack")
    blob = blob.to(DEV)
    y = torch.empty(N, cout, H, W, device=DEV)
    _call("nnd_mbv3_pointwise", cout, cin, k, _p(blob), _p(x), _p(res), _p(y), N, H, W, act)

    def ref(x, w, b, res):
        r = ACTS[act](F.conv2d(x, w, b, padding=k // 2))
        return res + r if res is not None else r
    d = lambda t: None if t is None else t.double()  # noqa: E731
    _judge(f"pointwise {k}x{k} {cin}->{cout} {mode} {N}x{H}x{W}", y, ref(x, w, b, res), ref(d(x), d(w), d(b), d(res)))


@pytest.mark.parametrize("cout,hw", [(256, (37, 53)), (96, (36, 52)), (256, (136, 240))])
def test_kernel_projection(cout, hw):
    """fnet_proj / cnet_proj: Conv2d(24 -> cout, 3, padding 1) + ReLU."""
    F = torch.nn.functional
    N, cin, (H, W) = 2, 24, hw
    x = _rand(N, cin, H, W, seed=19)
    w = _rand(cout, cin, 3, 3, seed=20, scale=(cin * 9) ** -0.5)
    b = _rand(cout, seed=21, scale=0.1)
    y = torch.empty(N, cout, H, W, device=DEV)
    _call("nnd_mbv3_proj", _p(x), _p(w), _p(b), _p(y), N, cin, cout, H, W)

    def ref(x, w, b):
        return F.relu(F.conv2d(x, w, b, padding=1))
    _judge(f"projection 3x3 {cin}->{cout} {N}x{H}x{W}", y, ref(x, w, b), ref(x.double(), w.double(), b.double()))
