"""outputs="all" against outputs="last" (the last-upsample-only loops, NND_FLAG_LAST_UPSAMPLE_ONLY) in one process, the two modes
alternating rep by rep on the same seeded pair, per configuration:
    raft      RAFT-Stereo 544x960, 32 iterations, batch 1 (the bench.py workload)
    kitti     RAFT-Stereo 8 x 384x1248 (KITTI padded), 32 iterations
    cre       CREStereo 1080x1920, 20 iterations (cascade 10 + 10 + 20)
For each: pairs/s of both modes (median of the reps), the peak allocated memory of one forward of each, and whether the finals are
torch.equal.
    python scripts/bench_outputs.py [raft,kitti,cre] [--arithmetic fp16x2] [--reps 9]          (on the GPU box)"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from nndepth_amd import weightgen  # noqa: E402

DEV = "cuda:0"


def build(which, arithmetic):
    from nndepth_amd.cre_stereo import CREStereoBase
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    if which == "raft":
        m, (B, H, W), seed, label = BaseRAFTStereo(iters=32, context_dim=64, arithmetic=arithmetic), (1, 544, 960), 100, \
            "RAFT-Stereo 544x960, 32 iters, batch 1"
    elif which == "kitti":
        m, (B, H, W), seed, label = BaseRAFTStereo(iters=32, context_dim=64, arithmetic=arithmetic), (8, 384, 1248), 2, \
            "RAFT-Stereo 8 x 384x1248, 32 iters"
    elif which == "cre":
        m, (B, H, W), seed, label = CREStereoBase(iters=20, arithmetic=arithmetic), (1, 1080, 1920), 3, \
            "CREStereo 1080x1920, 20 iters (10 + 10 + 20)"
    else:
        raise SystemExit(f"unknown configuration {which!r}")
    weightgen.fill_module_(m)
    f1, f2 = (x.to(DEV) for x in weightgen.synthetic_frames(seed, B, H, W))
    return m.to(DEV).eval(), f1, f2, B, label


def run(which, arithmetic, reps):
    m, f1, f2, B, label = build(which, arithmetic)
    final = {}
    peak = {}
    for mode in ("all", "last"):  # warm-up (and the fp16x2 calibration on the first forward), then one forward for the peak
        m.outputs = mode
        m(f1, f2)
        m(f1, f2)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = m(f1, f2)
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated() - base
        final[mode] = out[-1]["up_disp"].clone()
        del out
    times = {"all": [], "last": []}
    for _ in range(reps):
        for mode in ("all", "last"):
            m.outputs = mode
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m(f1, f2)
            torch.cuda.synchronize()
            times[mode].append(time.perf_counter() - t0)
            del out
    m.outputs = "all"
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    pps = {k: B / v for k, v in med.items()}
    equal = torch.equal(final["all"], final["last"])
    print(f"{label} [{arithmetic}], median of {reps} alternating reps:\n"
          f"  all : {pps['all']:8.2f} pairs/s  ({med['all'] * 1e3:8.2f} ms / batch)  peak allocated during the forward {peak['all'] / 2**20:8.1f} MiB\n"
          f"  last: {pps['last']:8.2f} pairs/s  ({med['last'] * 1e3:8.2f} ms / batch)  peak allocated during the forward {peak['last'] / 2**20:8.1f} MiB\n"
          f"  last / all: {pps['last'] / pps['all']:.3f}x throughput; finals torch.equal: {equal}", flush=True)
    return equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="?", default="raft,kitti,cre")
    ap.add_argument("--arithmetic", default="fp16x2", choices=["fp16x2", "bf16x3", "fp32"])
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    ok = all([run(which, args.arithmetic, args.reps) for which in args.configs.split(",")])
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
