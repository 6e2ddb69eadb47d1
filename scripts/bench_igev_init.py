"""IGEV's initial disparity beyond 8 groups / 512 candidates on one MI355X: the chunked kernel (nnd_igev_init_disparity_dev) against the
path such a shape ran before it existed — the squeezer as a PyTorch-ROCm Conv3d on the permuted view of the volume, then
nnd_softargmin_disparity — selected the way tests/test_gpu_igev_init_general.py selects it (ops.igev_init_disparity_supported patched
to False in front of the two branches of IGEVStereoBase._forward).

    python scripts/bench_igev_init.py [--out profiles/igev_init_bench.jsonl]

Device events, every shape warmed up, the median of 5 rounds of 10 calls with the two paths alternating inside one process, and the
spread (min .. max of the rounds).  Algorithmic bytes = the volume once plus the output; the share is of 8 TB/s.  The older
row-walking kernel at G = 8, 136x240x240 is timed in the same run for comparison."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nndepth_amd import ops  # noqa: E402

DEV = "cuda:0"
ROUNDS, CALLS = 5, 10


def init_disparity(geo, conv, host_params, B, G, H, W, D):
    """The two branches of IGEVStereoBase._forward."""
    if ops.igev_init_disparity_supported(G, D):
        params = host_params if ops.igev_init_disparity_host_params(G, D) else (conv.weight, conv.bias)
        return ops.igev_init_disparity(geo, *params, B, G, H, W, D)
    logits = conv(geo.reshape(B, G, H, W, D).permute(0, 1, 4, 2, 3)).squeeze(1)
    return ops.softargmin_disparity(logits.float())


def round_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / CALLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "igev_init_bench.jsonl"))
    a = ap.parse_args()
    supported = ops.igev_init_disparity_supported
    lines = []
    with torch.no_grad():
        for (B, G, H, W, D) in ((1, 16, 136, 240, 240), (1, 8, 136, 600, 600), (1, 8, 136, 240, 240)):
            torch.manual_seed(G + D)
            geo = torch.randn((B * G * H * W, D), device=DEV)
            conv = torch.nn.Conv3d(G, 1, 3, 1, 1).to(DEV)
            host = (ops._host(conv.weight), ops._host(conv.bias))
            paths = {"hip": lambda: init_disparity(geo, conv, host, B, G, H, W, D)}
            older = ops.igev_init_disparity_host_params(G, D)  # a shape the older kernels serve: timed for comparison, no fallback to beat
            if not older:
                def fallback():
                    ops.igev_init_disparity_supported = lambda g, d: False
                    try:
                        return init_disparity(geo, conv, host, B, G, H, W, D)
                    finally:
                        ops.igev_init_disparity_supported = supported
                paths["fallback"] = fallback
            outs = {k: fn() for k, fn in paths.items()}  # warm-up (and the LDS limit, MIOpen's choice of a Conv3d kernel)
            for fn in paths.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            us = {k: [] for k in paths}
            for _ in range(ROUNDS):
                for k, fn in paths.items():
                    us[k].append(round_us(fn))
            nbytes = 4 * (geo.numel() + B * H * W)
            med = {k: statistics.median(v) for k, v in us.items()}
            rec = {"shape": {"B": B, "G": G, "H": H, "W": W, "D": D}, "volume_MB": round(4 * geo.numel() / 1e6, 1),
                   "kernel": ops.igev_init_disparity_kernel(B, G, H, W, D), "hip_us": round(med["hip"], 1),
                   "hip_us_min_max": [round(min(us["hip"]), 1), round(max(us["hip"]), 1)],
                   "hip_share_of_8TBs": round(nbytes / (med["hip"] * 1e-6) / 8e12, 3), "rounds": ROUNDS, "calls_per_round": CALLS}
            if not older:
                rec.update({"fallback_us": round(med["fallback"], 1),
                            "fallback_us_min_max": [round(min(us["fallback"]), 1), round(max(us["fallback"]), 1)],
                            "speedup": round(med["fallback"] / med["hip"], 2),
                            "max_abs_hip_vs_fallback": float((outs["hip"] - outs["fallback"]).abs().max()),
                            "not_slower": bool(med["hip"] <= med["fallback"])})
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del geo, outs
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
