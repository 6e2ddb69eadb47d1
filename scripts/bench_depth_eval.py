"""The monocular evaluation criterion on one GPU: DepthEvalCriterion on the device against the same formulas in eager
PyTorch-ROCm ops on the same GPU in the same run (profiles/depth_eval_bench.jsonl).

One batch, 8 x 1 x 384 x 384 with a 70 % valid mask (depth log-uniform in (0.05, 100), prediction 0.7 gt + 2 + 10 % noise):
  call_ms            DepthEvalCriterion.__call__: the seven launches of nnd_depth_eval and the copy of ten doubles, wall time
  metrics_tensor_ms  DepthEvalCriterion.metrics_tensor: the launches alone (events; no host synchronisation inside)
  eager_ms           eager_criterion below: the reference's steps (evaluate.py:48-211, loss.py:6-59) as PyTorch ops on the device in
                     fp32, the fit in its closed form instead of torch.linalg.lstsq; wall time, it synchronises at every .item()
                     as the reference does
`launches` is counted from the source for the HIP route (seven kernels, whatever the shape) and by torch.profiler for the eager
one (null where the profiler is not available).  The reference itself does not travel with the repository, so it is not timed.

Method: 5 warm-up calls, then the median of 30 timed calls, min and max beside it.  No pass / fail threshold.

    timeout -k 10 300 python scripts/bench_depth_eval.py [--out profiles/depth_eval_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
HIP_LAUNCHES = 7  # csrc/depth_eval.hip: fit_mean, fit_moment, metrics, median, ssi_scale, ssi_error, final


def eager_criterion(pred, gt, mask, max_depth=80.0):
    aligned = pred.clone()
    for i in range(pred.shape[0]):
        m = mask[i]
        if torch.sum(m) > 100:
            p, g = pred[i][m], gt[i][m]
            pm, gm = p.mean(), g.mean()
            scale = ((p - pm) * (g - gm)).sum() / ((p - pm) ** 2).sum()
            aligned[i] = pred[i] * scale + (gm - scale * pm)
    valid = mask & (gt > 0.1) & (gt < max_depth)
    a, g = aligned[valid], gt[valid]
    if len(a) == 0:
        return None
    out = [torch.mean(torch.abs(a - g) / g).item(), torch.mean((a - g) ** 2 / g).item(), torch.sqrt(torch.mean((a - g) ** 2)).item(),
           torch.sqrt(torch.mean((torch.log(a) - torch.log(g)) ** 2)).item()]
    ratio = torch.maximum(a / g, g / a)
    out += [torch.mean((ratio < 1.25 ** k).float()).item() for k in (1, 2, 3)]
    gn = (gt - g.min()) / (g.max() - g.min() + 1e-6)
    an = (aligned - a.min()) / (a.max() - a.min() + 1e-6)
    ssi = []
    for x in (gn, an):
        shifts, scales = [], []
        for i in range(x.shape[0]):
            v = x[i][valid[i]]
            shift = torch.median(v)
            shifts.append(shift)
            scales.append(torch.mean(torch.abs(v - shift)))
        scale, shift = torch.stack(scales)[:, None, None, None], torch.stack(shifts)[:, None, None, None]
        scale[scale == 0] = 1
        ssi.append((x - shift) / scale)
    d = (ssi[1] - ssi[0])[valid]
    return out + [torch.mean(torch.abs(d)).item(), torch.sqrt(torch.mean(d ** 2)).item()]


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def device_ms(fn, warmup=5, reps=30):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def wall_ms(fn, warmup=5, reps=30):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def eager_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:  # the profiler is optional equipment
        print(f"torch.profiler not usable here ({type(e).__name__}: {e}); eager launches not counted", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_eval_bench.jsonl"))
    args = ap.parse_args()
    from nndepth_amd import weightgen
    from nndepth_amd.prepost import DEPTH_METRICS, DepthEvalCriterion
    assert torch.cuda.is_available(), "bench_depth_eval.py needs the MI355X"
    B, H, W = 8, 384, 384
    shape = (B, 1, H, W)
    u = lambda tag: weightgen.uniform01(f"bench_depth_eval/{tag}", B * H * W).reshape(shape)
    gt = np.exp(np.log(0.05) + u("gt").astype(np.float64) * (np.log(100.0) - np.log(0.05))).astype(np.float32)
    pred = np.maximum(0.7 * gt + 2.0 + 0.1 * gt * (2.0 * u("noise") - 1.0), 0.3).astype(np.float32)
    pred, gt, mask = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(u("mask") < 0.7).to(DEV)
    crit = DepthEvalCriterion(80.0)
    ours, eager = crit(pred, gt, mask), eager_criterion(pred, gt, mask)
    row = {"what": "depth_eval", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "H": H, "W": W,
           "mask_fraction": float(mask.float().mean().item()),
           "call_ms": med(wall_ms(lambda: crit(pred, gt, mask))),
           "metrics_tensor_ms": med(device_ms(lambda: crit.metrics_tensor(pred, gt, mask))),
           "eager_ms": med(wall_ms(lambda: eager_criterion(pred, gt, mask))),
           "launches": {"hip": HIP_LAUNCHES, "eager": eager_launches(lambda: eager_criterion(pred, gt, mask))},
           "max_rel_diff_eager_fp32_vs_hip_fp64": max(abs(e - ours[k]) / max(1.0, abs(ours[k])) for k, e in zip(DEPTH_METRICS, eager))}
    row["eager_over_call"] = row["eager_ms"]["median"] / row["call_ms"]["median"]
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
