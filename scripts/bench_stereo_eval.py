"""The stereo evaluation criterion over every output of a forward on one GPU: StereoEvalCriterion on the device against the
calls it replaces and against the same formulas in eager PyTorch-ROCm ops, on the same GPU in the same run
(profiles/stereo_eval_bench.jsonl, one line per workload, appended).

Workload 1 (a RAFT-Stereo forward): 32 outputs of 1 x 1 x 544 x 960, slices of one stacked tensor, a 70 % valid mask.
Workload 2 (a CREStereo-shaped forward): 40 two-channel outputs, 10 at 270 x 480, 10 at 540 x 960, 20 at 1080 x 1920, against a
1-channel 1080 x 1920 ground truth, no mask.
  metrics_tensor_ms  StereoEvalCriterion.metrics_tensor: the launches alone (events; no host synchronisation inside)
  call_ms            StereoEvalCriterion.__call__: the launches and the one copy of N*K + 1 doubles, wall time
  eval_criterion_ms  workload 1 only: one EvalCriterion call per output on the same maps (each is a single-output
                     StereoEvalCriterion call: fills a descriptor, launches twice, copies K + 1 doubles and synchronises), wall
                     time; it returns epe and the `above` fractions only
  eager_ms           the reference's lines (evaluate.py:63-82, loss.py:23-33, 47-50) as PyTorch ops on the device in fp32, one
                     copy at the end, wall time
`bytes` is the algorithmic traffic: every output read once, the ground truth and the mask once per size group;
`achieved_TB_s` = bytes / the median of metrics_tensor_ms.  `launches` is counted from the source (one per distinct size, one
final).  The reference itself does not travel with the repository, so it is not timed.

Method: 5 warm-up calls, then the median of 30 timed calls (10 for the eager route), min and max beside it.  The only
requirement: on workload 1, call_ms is below eval_criterion_ms (asserted).

    timeout -k 10 600 python scripts/bench_stereo_eval.py [--out profiles/stereo_eval_bench.jsonl] [--note TEXT]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
ABOVE = {"d1": 1.0, "d3": 3.0}
BELOW = {"0.5px": 0.5, "1px": 1.0, "3px": 3.0, "5px": 5.0}


def eager_criterion(gt, outs, mask, max_flow=1000.0, gamma=0.8):
    rows, loss, n = [], 0.0, len(outs)
    for i, p in enumerate(outs):
        if p.shape[-2:] != gt.shape[-2:]:
            scale = gt.shape[-1] // p.shape[-1]
            g = F.interpolate(-F.max_pool2d(-gt, kernel_size=scale) / scale, size=p.shape[-2:])
        else:
            g = gt
        epe = torch.sum((p - g) ** 2, dim=1).sqrt()
        valid = torch.sum(g ** 2, dim=1, keepdim=True).sqrt() < max_flow
        if mask is not None:
            valid = valid & mask
        l1 = (valid * (p - g).abs()).mean()
        e = epe.view(-1)[valid.view(-1)]
        rows.append(torch.stack([e.mean(), torch.tensor(float(e.numel()), device=e.device), l1]
                                + [(e > t).float().mean() for t in ABOVE.values()] + [(e < t).float().mean() for t in BELOW.values()]))
        loss = loss + gamma ** (n - 1 - i) * l1
    return torch.stack(rows).cpu(), float(loss)


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


def gt_at(gt, size):
    if tuple(gt.shape[-2:]) == tuple(size):
        return gt
    s = gt.shape[-1] // size[-1]
    return F.interpolate(-F.max_pool2d(-gt, kernel_size=s) / s, size=tuple(size))


def make(gen, gt_shape, out_shapes, stacked):
    gt = (torch.rand(gt_shape, device=DEV, generator=gen) * 2 - 1) * 60.0
    outs = []
    for i, (Cc, h, w) in enumerate(out_shapes):
        noise = (torch.rand((gt_shape[0], Cc, h, w), device=DEV, generator=gen) * 2 - 1) * (6.0 * (0.5 + 0.5 / (i + 1)))
        outs.append(gt_at(gt, (h, w)) + noise)
    if stacked:
        up = torch.stack(outs)
        outs = [up[i] for i in range(len(outs))]
    return gt, outs


def traffic_bytes(gt, outs, mask):
    groups = {tuple(o.shape[1:]) for o in outs}
    per_group = gt.numel() * 4 + (mask.numel() if mask is not None else 0)
    return sum(o.numel() * 4 for o in outs) + len(groups) * per_group


def measure(name, gt, outs, mask, with_eval_criterion):
    from nndepth_amd.prepost import EvalCriterion, StereoEvalCriterion
    crit = StereoEvalCriterion(ABOVE, BELOW)
    ours = torch.tensor([[r[k] for k in crit.columns] for r in crit(gt, outs, mask)], dtype=torch.float64)
    eager, _ = eager_criterion(gt, outs, mask)
    nbytes = traffic_bytes(gt, outs, mask)
    row = {"what": "stereo_eval", "workload": name, "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "gt": list(gt.shape), "outputs": [list(o.shape) for o in outs], "mask_fraction": None if mask is None else float(mask.float().mean()),
           "columns": list(crit.columns), "bytes": nbytes, "launches": len({tuple(o.shape[1:]) for o in outs}) + 1,
           "metrics_tensor_ms": med(device_ms(lambda: crit.metrics_tensor(gt, outs, mask))),
           "call_ms": med(wall_ms(lambda: crit(gt, outs, mask))),
           "eager_ms": med(wall_ms(lambda: eager_criterion(gt, outs, mask), warmup=2, reps=10)),
           "max_rel_diff_eager_fp32_vs_hip_fp64": float(((eager.double() - ours).abs() / ours.abs().clamp(min=1.0)).max())}
    row["achieved_TB_s"] = nbytes / (row["metrics_tensor_ms"]["median"] * 1e-3) / 1e12
    row["eager_over_call"] = row["eager_ms"]["median"] / row["call_ms"]["median"]
    if with_eval_criterion:
        old = EvalCriterion(dict(ABOVE))
        per_map = [old(gt, o, mask) for o in outs]
        assert all(abs(m["epe"] - float(ours[i, 0])) <= 1e-5 * max(1.0, float(ours[i, 0])) for i, m in enumerate(per_map))
        row["eval_criterion_ms"] = med(wall_ms(lambda: [old(gt, o, mask) for o in outs]))
        row["eval_criterion_over_call"] = row["eval_criterion_ms"]["median"] / row["call_ms"]["median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_eval_bench.jsonl"))
    ap.add_argument("--note", default=None, help="kept in every line, e.g. the commit measured")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stereo_eval.py needs the MI355X"
    gen = torch.Generator(device=DEV)
    gen.manual_seed(0)
    rows = []
    gt, outs = make(gen, (1, 1, 544, 960), [(1, 544, 960)] * 32, stacked=True)
    mask = torch.rand((1, 1, 544, 960), device=DEV, generator=gen) < 0.7
    rows.append(measure("raft_32x544x960", gt, outs, mask, True))
    del gt, outs, mask
    gt, outs = make(gen, (1, 1, 1080, 1920), [(2, 270, 480)] * 10 + [(2, 540, 960)] * 10 + [(2, 1080, 1920)] * 20, stacked=False)
    rows.append(measure("cre_40x3sizes_1080x1920", gt, outs, None, False))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for row in rows:
            if args.note:
                row["note"] = args.note
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
    r = rows[0]
    assert r["call_ms"]["median"] < r["eval_criterion_ms"]["median"], (r["call_ms"], r["eval_criterion_ms"])


if __name__ == "__main__":
    main()
