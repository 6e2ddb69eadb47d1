"""Coarse2FineGroupRepViTRAFTStereo end to end on one MI355X with its frame-size stage outputs resized by nnd_resize_nearest_scaled
(default) against NND_C2F_TORCH_RESIZE=1 (F.interpolate(u, size=frame) * rate on PyTorch-ROCm, 24 outputs x 2 kernels).

    python scripts/bench_c2f_resize.py [--height 512 --width 960 --iters 12 --out profiles/c2f_resize_bench.jsonl]
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_c2f_resize.py --trace     # three default forwards, nothing timed

Device events, warm-up (the first forward calibrates fp16x2), the median of 5 rounds of 10 forwards with the two paths alternating
inside one process, and the spread (min .. max of the rounds)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUNDS, CALLS = 5, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "c2f_resize_bench.jsonl"))
    a = ap.parse_args()
    from nndepth_amd import weightgen
    from nndepth_amd.raft_stereo import Coarse2FineGroupRepViTRAFTStereo
    dev = "cuda:0"
    m = Coarse2FineGroupRepViTRAFTStereo(iters=a.iters, corr_levels=1, arithmetic="fp16x2")
    weightgen.fill_module_(m, "c2frv.")
    m = m.eval().to(dev)
    f1, f2 = (t.to(dev) for t in weightgen.synthetic_frames(1, 1, a.height, a.width))
    os.environ.pop("NND_C2F_TORCH_RESIZE", None)
    for _ in range(3):
        outs = m(f1, f2)
    torch.cuda.synchronize()
    if a.trace:
        return

    def forwards(torch_resize):
        if torch_resize:
            os.environ["NND_C2F_TORCH_RESIZE"] = "1"
        else:
            os.environ.pop("NND_C2F_TORCH_RESIZE", None)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(CALLS):
            m(f1, f2)
        e.record()
        e.synchronize()
        os.environ.pop("NND_C2F_TORCH_RESIZE", None)
        return s.elapsed_time(e) / CALLS

    forwards(True)  # warm-up of the PyTorch expression
    ms = {"hip": [], "torch": []}
    for _ in range(ROUNDS):
        ms["hip"].append(forwards(False))
        ms["torch"].append(forwards(True))
    med = {k: statistics.median(v) for k, v in ms.items()}
    rec = {"model": "Coarse2FineGroupRepViTRAFTStereo", "HxW": [a.height, a.width], "iters": f"3 x {a.iters}", "arithmetic": "fp16x2",
           "outputs": len(outs), "rounds": ROUNDS, "forwards_per_round": CALLS}
    for k, name in (("hip", "hip_resize"), ("torch", "torch_resize")):
        rec[name + "_ms_per_pair"] = round(med[k], 3)
        rec[name + "_ms_min_max"] = [round(min(ms[k]), 3), round(max(ms[k]), 3)]
        rec[name + "_pairs_per_s"] = round(1e3 / med[k], 1)
    rec["not_slower"] = bool(med["hip"] <= med["torch"])
    print(json.dumps(rec), flush=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
