"""MobileNetV3DepthModel on one MI355X: ms per image and images/s, eager and HIP-graph replay, the HIP path against hip=False (the
modules' eager PyTorch forward) on the same GPU in the same run; and an A/B of the fused head kernel (nnd_midas_head) against the
unfused composition (F.interpolate x2 + nnd_mbv3_pointwise 3x3 + ReLU + nnd_mbv3_pointwise 1x1 + ReLU, which writes and re-reads
the two full-resolution C-channel maps).
    python scripts/bench_midas.py [--configs 384x384x1,384x384x8,480x640x1 --steps 30]
    python scripts/bench_midas.py --forward-only --steps 20     # the HIP forward alone (for a kernel trace)
Prints one JSON line per measurement: median of `--steps` timed calls after 3 warm-up calls, synchronised per call, with the
spread (min, max) of three such medians so that a difference can be told from run-to-run noise."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

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


def timed3(fn, steps):
    """-> (median of three medians, min, max) in ms."""
    m = sorted(timed(fn, steps) * 1e3 for _ in range(3))
    return m[1], m[0], m[2]


def head_ab(model, B, H, W, steps, dev):
    """Fused head vs the unfused composition on the same input t = last_conv.0's output (B, C, H/2, W/2)."""
    from nndepth_amd import ops
    from nndepth_amd._lib import check, lib
    lc = model.last_conv
    Cc = lc[0].out_channels
    t = torch.rand(B, Cc, H // 2, W // 2, device=dev) - 0.5
    packed = ops.midas_head_pack(lc[2].weight, lc[2].bias, lc[4].weight, lc[4].bias, dev)

    def pw_pack(conv, k):
        w, b = conv.weight.detach().cpu().float().contiguous(), conv.bias.detach().cpu().float().contiguous()
        blob = torch.empty(int(lib.nnd_mbv3_pointwise_packed_floats(conv.out_channels, conv.in_channels, k)), dtype=torch.float32)
        check(lib.nnd_mbv3_pointwise_pack(conv.out_channels, conv.in_channels, k, C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()),
                                          C.c_void_p(blob.data_ptr())), "pack")
        return blob.to(dev)

    p3, p1 = pw_pack(lc[2], 3), pw_pack(lc[4], 1)
    y3 = torch.empty(B, Cc, H, W, device=dev)
    y1 = torch.empty(B, 1, H, W, device=dev)
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    ptr = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731

    def unfused():
        u = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
        check(lib.nnd_mbv3_pointwise(Cc, Cc, 3, ptr(p3), ptr(u), None, ptr(y3), B, H, W, 1, st()), "3x3")
        check(lib.nnd_mbv3_pointwise(1, Cc, 1, ptr(p1), ptr(y3), None, ptr(y1), B, H, W, 1, st()), "1x1")
        return y1

    fused = lambda: ops.midas_head(t, packed)  # noqa: E731
    diff = (fused() - unfused()).abs().max().item()
    f, u = timed3(fused, steps), timed3(unfused, steps)
    return {"what": "head_ab", "B": B, "H": H, "W": W, "C": Cc, "fused_ms": f[0], "fused_min_max": f[1:], "unfused_ms": u[0],
            "unfused_min_max": u[1:], "speedup": u[0] / f[0], "max_abs_diff": diff}


def main():
    from nndepth_amd import weightgen
    from nndepth_amd.graph import GraphedForward
    from nndepth_amd.midas import MobileNetV3DepthModel
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="384x384x1,384x384x8,480x640x1")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--forward-only", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"

    def model(**kw):
        m = MobileNetV3DepthModel(**kw)
        weightgen.fill_module_(m, "midas.")
        with torch.no_grad():
            m.last_conv[4].bias.fill_(0.0107)  # the generated bias clamps most of the output to zero
        return m.eval().to(dev)

    m, ref = model(), model(hip=False)
    for cfg in a.configs.split(","):
        H, W, B = (int(v) for v in cfg.split("x"))
        x = weightgen.synthetic_frames(1, B, H, W)[0].to(dev)
        with torch.no_grad():
            if a.forward_only:
                print(json.dumps({"what": "forward_hip", "B": B, "H": H, "W": W, "ms": timed(lambda: m(x), a.steps) * 1e3}), flush=True)
                continue
            err = (m(x) - ref(x)).abs().max().item()
            hip, pt = timed3(lambda: m(x), a.steps), timed3(lambda: ref(x), a.steps)
            gh, gp = GraphedForward(m), GraphedForward(ref)
            ghip, gpt = timed3(lambda: gh(x), a.steps), timed3(lambda: gp(x), a.steps)
        print(json.dumps({"what": "model", "B": B, "H": H, "W": W, "hip_ms_per_image": hip[0] / B, "hip_images_per_s": 1e3 * B / hip[0],
                          "hip_min_max_ms": hip[1:], "pytorch_ms_per_image": pt[0] / B, "pytorch_images_per_s": 1e3 * B / pt[0],
                          "pytorch_min_max_ms": pt[1:], "speedup": pt[0] / hip[0], "graphed_hip_ms_per_image": ghip[0] / B,
                          "graphed_hip_images_per_s": 1e3 * B / ghip[0], "graphed_pytorch_ms_per_image": gpt[0] / B,
                          "graphed_speedup": gpt[0] / ghip[0], "max_abs_diff": err}), flush=True)
        with torch.no_grad():
            print(json.dumps(head_ab(m, B, H, W, a.steps, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
