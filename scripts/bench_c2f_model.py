"""Coarse2FineGroupRepViTRAFTStereo on one MI355X: the encoder side (HIP, one nnd_repvit_forward call, vs hip_encoder=False, the
containers' eager PyTorch forward on the same GPU) and the drop-in model end to end (pairs/s, 3 stages x `--iters` iterations).

    python scripts/bench_c2f_model.py [--height 512 --width 960 --iters 12 --steps 20]
    python scripts/bench_c2f_model.py --kernels     # each encoder-side kernel alone at its 512x960 shapes
Prints one JSON line per measurement.  The encoder side's fp32 floor is computed from the layer shapes: dense flops at the fp32 MFMA
rate, depthwise flops at the fp32 VALU rate, both 157.3 TFLOP/s on the MI355X (256 CUs x 256 flop / clk x 2.4 GHz)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def floor_us(m, H, W):
    """fp32 floor of the folded chain (what the kernels compute), from the layer shapes."""
    from nndepth_amd.ops import RepViTEngine
    d = RepViTEngine.descriptor(m.fnet, m.cnet_proj, m.fusion_blocks)
    layers = RepViTEngine.fold(m.fnet, m.cnet_proj, m.fusion_blocks)
    dense, dw = 0.0, 0.0
    f1 = torch.zeros(1, 3, H, W)
    shapes = []
    orig = torch.nn.functional.conv2d

    def spy(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        y = orig(x, w, b, stride, padding, dilation, groups)
        shapes.append((y.numel(), w.shape[1] * w.shape[2] * w.shape[3], groups > 1))
        return y
    torch.nn.functional.conv2d = spy
    try:
        RepViTEngine.fold_forward(layers, d, f1, f1)
    finally:
        torch.nn.functional.conv2d = orig
    for n, k, is_dw in shapes:
        if is_dw:
            dw += 2.0 * n * k
        else:
            dense += 2.0 * n * k
    mfma = valu = 157.3e12
    return dense, dw, (dense / mfma + dw / valu) * 1e6


def kernels(steps):
    """Each encoder-side kernel alone (its nnd_repvit_* entry point) at the 512x960 pair's shapes, with its bytes / flops; and the
    stem's 3x3 3 -> 16 stride-2 conv on stem_conv_kernel against the exact fp32 conv_mfma (nnd_conv_forward, same shape)."""
    from nndepth_amd._lib import check, lib
    from nndepth_amd.ops import ConvNorm, _p, _stream
    dev = torch.device("cuda:0")
    st = _stream(dev)
    r = lambda *s: torch.randn(*s, device=dev)  # noqa: E731

    def rep(what, fn, nbytes, flops):
        t = timed(fn, steps)
        print(json.dumps({"kernel": what, "us": round(t * 1e6, 1), "GB/s": round(nbytes / t / 1e9, 1),
                          "TFLOP/s": round(flops / t / 1e12, 2)}))
    N = 2
    # stem: frames 512x960 -> 16 x 256x480
    x, x1, w, b, y = r(1, 3, 512, 960), r(1, 3, 512, 960), r(16, 3, 3, 3), r(16), torch.empty(N, 16, 256, 480, device=dev)
    io = 4 * (2 * 3 * 512 * 960 + N * 16 * 256 * 480)
    rep("stem_conv_kernel 3->16 3x3 s2", lambda: check(lib.nnd_repvit_stem(_p(x), _p(x1), 1, _p(w), _p(b), _p(y), N, 512, 960, 2, st)),
        io, 2.0 * N * 16 * 27 * 256 * 480)
    cn, xx = ConvNorm(w, b, stride=2, device=dev), torch.cat([x, x1])
    rep("conv_mfma 3->16 3x3 s2 (same shape, for comparison)", lambda: cn(xx), io, 2.0 * N * 16 * 27 * 256 * 480)
    for C, H, W, k, s in ((16, 256, 480, 3, 2), (16, 128, 240, 7, 2), (32, 64, 120, 3, 1), (64, 32, 60, 3, 1), (128, 16, 30, 3, 1)):
        xi, wi, bi = r(N, C, H, W), r(C, 1, k, k), r(C)
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        yo = torch.empty(N, C, Ho, Wo, device=dev)
        rep(f"dwconv_kernel<{k}> C{C} {H}x{W} s{s}", lambda: check(lib.nnd_repvit_depthwise(_p(xi), _p(wi), _p(bi), _p(yo), N, C, H, W, k,
                                                                                               s, 1, st)),
            4 * (xi.numel() + yo.numel()), 2.0 * yo.numel() * k * k)
    for C, H, W in ((256, 8, 15),):
        q, o = r(N, 1 + 2 * C, H, W), torch.empty(N, C, H, W, device=dev)
        rep(f"linattn_kernel C{C} {H}x{W}", lambda: check(lib.nnd_repvit_linear_attention(_p(q), _p(o), N, C, H, W, st)),
            4 * (q.numel() + o.numel()), 4.0 * N * C * H * W)
    for C, h, w_, H, W in ((64, 8, 15, 32, 60), (64, 32, 60, 128, 240)):
        a, yy = r(N, C, h, w_), r(N, C, H, W)
        rep(f"upsample_add_relu_kernel C{C} {h}x{w_} -> {H}x{W}",
            lambda: check(lib.nnd_repvit_upsample_add_relu(_p(a), _p(yy), N, C, h, w_, H, W, st)), 4 * (a.numel() + 2 * yy.numel()),
            8.0 * yy.numel())
    for cin, cout, H, W in ((16, 16, 128, 240), (64, 192, 32, 60), (192, 64, 32, 60), (128, 384, 16, 30), (256, 1024, 8, 15)):
        n = int(lib.nnd_repvit_pointwise_packed_floats(cout, cin, 1))
        blob = torch.empty(n)
        wc, bc = torch.randn(cout, cin, 1, 1), torch.randn(cout)
        check(lib.nnd_repvit_pointwise_pack(cout, cin, 1, _p(wc), _p(bc), None, _p(blob)), "pack")
        blob, xi, yo = blob.to(dev), r(N, cin, H, W), torch.empty(N, cout, H, W, device=dev)
        rep(f"conv_mfma 1x1 EPI_GELU {cin}->{cout} {H}x{W}",
            lambda: check(lib.nnd_repvit_pointwise(cout, cin, 1, _p(blob), _p(xi), None, _p(yo), N, H, W, 1, st)),
            4 * (xi.numel() + yo.numel()), 2.0 * N * cin * cout * H * W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--encoder-only", action="store_true", help="time the HIP encoder side only (for a rocprofv3 run)")
    ap.add_argument("--kernels", action="store_true", help="time each encoder-side kernel alone")
    a = ap.parse_args()
    if a.kernels:
        return kernels(a.steps)
    from nndepth_amd import weightgen
    from nndepth_amd.raft_stereo import Coarse2FineGroupRepViTRAFTStereo, Coarse2FineRAFTStereoBase
    dev = "cuda:0"
    m = Coarse2FineGroupRepViTRAFTStereo(iters=a.iters, corr_levels=1)
    weightgen.fill_module_(m, "c2frv.")
    m = m.eval().to(dev)
    f1, f2 = (t.to(dev) for t in weightgen.synthetic_frames(1, 1, a.height, a.width))
    with torch.no_grad():
        hip = timed(lambda: m.forward_features(f1, f2), a.steps)
        if a.encoder_only:
            print(json.dumps({"what": "encoder side HIP", "HxW": [a.height, a.width], "us": round(hip * 1e6, 1)}))
            return
        eager = timed(lambda: Coarse2FineRAFTStereoBase.forward_features(m, f1, f2), a.steps)
    dense, dw, fl = floor_us(m.cpu(), a.height, a.width)
    m.to(dev)
    print(json.dumps({"what": "encoder side, one pair", "HxW": [a.height, a.width], "hip_us": round(hip * 1e6, 1),
                      "eager_pytorch_us": round(eager * 1e6, 1), "speedup": round(eager / hip, 2),
                      "folded_gflop_dense": round(dense / 1e9, 3), "folded_gflop_depthwise": round(dw / 1e9, 3),
                      "fp32_floor_us": round(fl, 1), "fraction_of_floor": round(fl / (hip * 1e6), 3)}))
    for arith in ("fp16x2", "fp32"):
        for outputs in ("all", "last"):
            mm = Coarse2FineGroupRepViTRAFTStereo(iters=a.iters, corr_levels=1, arithmetic=arith, outputs=outputs)
            mm.load_state_dict(m.state_dict())
            mm = mm.eval().to(dev)
            t = timed(lambda: mm(f1, f2), a.steps)
            print(json.dumps({"what": "end to end", "HxW": [a.height, a.width], "iters": f"3 x {a.iters}", "arithmetic": arith,
                              "outputs": outputs, "ms_per_pair": round(t * 1e3, 3), "pairs_per_s": round(1 / t, 1)}))


if __name__ == "__main__":
    main()
