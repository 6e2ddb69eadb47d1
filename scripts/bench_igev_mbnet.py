"""IGEVStereoMBNet on one MI355X: the encoder side (HIP, one nnd_mbv3_forward call, vs hip_encoder=False, the containers' eager
PyTorch forward on the same GPU) and the drop-in model end to end (pairs/s, `--iters` iterations), for each arithmetic.

    python scripts/bench_igev_mbnet.py [--height 544 --width 960 --iters 32 --batches 1,8 --steps 20]
    python scripts/bench_igev_mbnet.py --encoder-only --steps 20     # the HIP encoder side alone (for a kernel trace)
Prints one JSON line per measurement (median of `--steps` timed calls after 3 warm-up calls, synchronised per call)."""
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


def main():
    from nndepth_amd import weightgen
    from nndepth_amd.igev_stereo import IGEVStereoMBNet
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=544)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--encoder-only", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    H, W = a.height, a.width

    def model(**kw):
        m = IGEVStereoMBNet(iters=a.iters, **kw)
        weightgen.fill_module_(m, "igevmb.")
        return m.eval().to(dev)

    for B in [int(b) for b in a.batches.split(",")]:
        f1, f2 = (t.to(dev) for t in weightgen.synthetic_frames(1, B, H, W))
        m = model(arithmetic="fp32")
        with torch.no_grad():
            hip = timed(lambda: m.forward_fnet(f1, f2), a.steps)
            if a.encoder_only:
                print(json.dumps({"what": "encoder_side_hip", "B": B, "H": H, "W": W, "ms": hip * 1e3}), flush=True)
                continue
            m.hip_encoder = False
            pt = timed(lambda: m.forward_fnet(f1, f2), a.steps)
        print(json.dumps({"what": "encoder_side", "B": B, "H": H, "W": W, "hip_ms": hip * 1e3, "pytorch_ms": pt * 1e3,
                          "speedup": pt / hip}), flush=True)
        del m
        for arith in ("fp32", "bf16x3", "fp16x2"):
            m = model(arithmetic=arith)
            m(f1, f2)  # first forward: pack + calibration (fp16x2)
            t = timed(lambda: m(f1, f2), max(5, a.steps // 2))
            m.hip_encoder = False
            tp = timed(lambda: m(f1, f2), max(5, a.steps // 2))
            print(json.dumps({"what": "model", "arithmetic": arith, "B": B, "H": H, "W": W, "iters": a.iters, "ms": t * 1e3,
                              "pairs_per_s": B / t, "ms_pytorch_encoder": tp * 1e3, "pairs_per_s_pytorch_encoder": B / tp}),
                  flush=True)
            del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
