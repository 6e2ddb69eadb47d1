"""The value of the monocular loss on one GPU: MiDasLoss on the device against the same formulas in eager PyTorch-ROCm ops on
the same GPU in the same run (profiles/midas_loss_bench.jsonl).

Two batches, 8 x 1 x 384 x 384 and 1 x 1 x 384 x 384 with a 70 % valid mask (target log-uniform in (0.05, 100), prediction
0.7 t + 2 + 10 % noise); one JSON line each:
  call_ms            MiDasLoss.__call__: the nine launches of nnd_midas_loss and the copy of six doubles, wall time per call
  eager_ms           eager_loss below: the reference's steps (loss.py:6-221) as PyTorch ops on the device in fp32; wall time per
                     call, it synchronises at every boolean-mask gather and .item() as the reference does
  values_tensor_ms   MiDasLoss.values_tensor enqueued 20 times between two events, per call (no host synchronisation inside)
  kernels_ms         the nine kernels alone: values_tensor captured into a HIP graph, the replay between two events
`launches` is counted from the source for the HIP route (nine kernels, whatever the shape) and by torch.profiler for the eager
one (null where the profiler is not available).  The reference itself does not travel with the repository, so it is not timed.

Method: one process; after 5 warm-up calls of each path, 5 rounds, each timing 20 calls of one path and then 20 of the other;
the median over the rounds, min and max beside it.  No pass / fail threshold.

    timeout -k 10 300 python scripts/bench_midas_loss.py [--out profiles/midas_loss_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
HIP_LAUNCHES = 9  # csrc/midas_loss.hip: stats, median, scale, level 0, levels 1-3, trim, final
ROUNDS, CALLS = 5, 20


def eager_loss(pred, target, mask, c_trim=1.0, c_grad=0.1):
    tv = target[mask]
    tn = (target - tv.min()) / (tv.max() - tv.min() + 1e-6)
    ssi = []
    for x in (tn, pred):
        shifts, scales = [], []
        for i in range(x.shape[0]):
            v = x[i][mask[i]]
            shift = torch.median(v)
            shifts.append(shift)
            scales.append(torch.mean(torch.abs(v - shift)))
        scale, shift = torch.stack(scales)[:, None, None, None], torch.stack(shifts)[:, None, None, None]
        scale[scale == 0] = 1
        ssi.append((x - shift) / scale)
    st, sp = ssi
    total, pixels = [], 0
    for i in range(pred.shape[0]):
        e = torch.abs(sp[i][mask[i]] - st[i][mask[i]])
        trim = int(e.shape[-1] * 0.1)
        e = torch.sort(e, stable=True)[0][:-trim]
        pixels += e.shape[-1]
        total.append(e.sum())
    trimmed = torch.stack(total).sum() / pixels
    T, P, M = tn.clone(), sp, mask
    T[~M] = 0
    g = 0
    for _ in range(4):
        R = P - T
        term = torch.abs(R[:, :, :-1, :-1] - R[:, :, :-1, 1:]) + torch.abs(R[:, :, :-1, :-1] - R[:, :, 1:, :-1])
        g = g + term[M[:, :, 1:, 1:]].sum()
        T, idx = F.max_pool2d(T, 2, stride=2, return_indices=True)
        M = M.flatten(2).gather(2, idx.flatten(2)).view_as(idx)
        P = F.avg_pool2d(P, 2, stride=2)
    grad = g / mask.sum()
    loss = trimmed * c_trim + grad * c_grad
    abs_dev = torch.abs(sp - st)[mask].mean()
    return [loss.item(), trimmed.item(), grad.item(), abs_dev.item()]


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def wall_per_call(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / CALLS


def events_per_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / CALLS


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


def bench(B, H, W):
    from nndepth_amd import weightgen
    from nndepth_amd.prepost import MIDAS_LOSS_METRICS, MiDasLoss
    shape = (B, 1, H, W)
    u = lambda tag: weightgen.uniform01(f"bench_midas_loss/{B}/{tag}", B * H * W).reshape(shape)
    t = np.exp(np.log(0.05) + u("t").astype(np.float64) * (np.log(100.0) - np.log(0.05))).astype(np.float32)
    pred = (0.7 * t + 2.0 + 0.1 * t * (2.0 * u("noise") - 1.0)).astype(np.float32)
    pred, t, mask = torch.from_numpy(pred).to(DEV), torch.from_numpy(t).to(DEV), torch.from_numpy(u("mask") < 0.7).to(DEV)
    crit = MiDasLoss()
    hip, eager = (lambda: crit(pred, t, mask)), (lambda: eager_loss(pred, t, mask))
    tensor = lambda: crit.values_tensor(pred, t, mask)
    for _ in range(5):
        ours, theirs = hip()[1], eager()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            captured = tensor()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert captured.cpu().tolist()[:4] == list(ours.values())
    call, eag, vt, kern = [], [], [], []
    for _ in range(ROUNDS):
        call.append(wall_per_call(hip))
        eag.append(wall_per_call(eager))
        vt.append(events_per_call(tensor))
        kern.append(events_per_call(graph.replay))
    row = {"what": "midas_loss", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "B": B, "H": H, "W": W,
           "mask_fraction": float(mask.float().mean().item()), "rounds": ROUNDS, "calls_per_round": CALLS,
           "call_ms": med(call), "eager_ms": med(eag), "values_tensor_ms": med(vt), "kernels_ms": med(kern),
           "launches": {"hip": HIP_LAUNCHES, "eager": eager_launches(eager)},
           "max_rel_diff_eager_fp32_vs_hip_fp64": max(abs(e - ours[k]) / max(1.0, abs(ours[k])) for k, e in zip(MIDAS_LOSS_METRICS, theirs))}
    row["eager_over_call"] = row["eager_ms"]["median"] / row["call_ms"]["median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "midas_loss_bench.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_midas_loss.py needs the MI355X"
    rows = [bench(8, 384, 384), bench(1, 384, 384)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
