"""The one-piece fp16 arithmetic ("fp16") against the default "fp16x2", measured in ONE process on one MI355X, alternating.

Workloads (synthetic frames, generated weights, both models of a workload hold the same weights and are calibrated on the pair they
are timed on, outside the timed region):
  raft544       RAFT-Stereo base (ctx 64), 544x960, 32 iterations, batch 1, all 32 maps          (bench.py's flagship)
  raft544_last  the same with outputs="last"
  kitti8        RAFT-Stereo base, 8 x 375x1242 -> Padder(32) -> 384x1248, 32 iterations, one batch of 8
  cre1080       CREStereo, 1080x1920, 20 iterations, 2-stage cascade, batch 1
Each workload: `--warmup` untimed forwards per arithmetic, then `--rounds` rounds; a round times `--steps` forwards of one
arithmetic (host clock around work that ends in a device synchronise), then of the other, so drift of the box hits both.  Reported
per arithmetic: the median round and min / max.
Then the loop convs of raft544 per launch INSIDE the fused loop (nnd_profile_loop_conv: events around the launch in every
iteration), both arithmetics, alternating per conv.
One JSON line per workload and one for the per-launch table are appended to profiles/fp16_bench.jsonl (--out).

    python scripts/bench_fp16.py [--workloads raft544,raft544_last,kitti8,cre1080,convs] [--steps 10] [--rounds 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARITHS = ("fp16x2", "fp16")


def log(msg):
    print(f"[bench_fp16] {msg}", file=sys.stderr, flush=True)


def build(workload, dev):
    """-> ({arith: forward()}, pairs per forward, description, {arith: model}, (f1, f2))"""
    import torch
    from nndepth_amd import weightgen
    fwd, models = {}, {}
    if workload in ("raft544", "raft544_last", "kitti8"):
        from nndepth_amd.prepost import Padder
        from nndepth_amd.raft_stereo import BaseRAFTStereo
        n, hw = (8, (375, 1242)) if workload == "kitti8" else (1, (544, 960))
        f1, f2 = (torch.cat(x).to(dev) for x in zip(*[weightgen.synthetic_frames(100 + i, 1, *hw) for i in range(n)]))
        if workload == "kitti8":
            f1, f2 = Padder(hw, divis_by=32).pad(f1, f2)
        for a in ARITHS:
            m = BaseRAFTStereo(iters=32, context_dim=64, arithmetic=a, outputs="last" if workload == "raft544_last" else "all")
            weightgen.fill_module_(m)
            models[a] = m.to(dev).eval()
            fwd[a] = (lambda m_: lambda: m_(f1, f2)[-1]["up_disp"])(models[a])
        what = {"raft544": "RAFT-Stereo base (ctx 64), 544x960, 32 iters, batch 1, all outputs",
                "raft544_last": "RAFT-Stereo base (ctx 64), 544x960, 32 iters, batch 1, outputs=\"last\"",
                "kitti8": "RAFT-Stereo base (ctx 64), 8 x 375x1242 (Padder 32 -> 384x1248), 32 iters, one batch of 8"}[workload]
    elif workload == "cre1080":
        from nndepth_amd.cre_stereo import CREStereoBase, two_stage_forward
        n = 1
        f1, f2 = (x.to(dev) for x in weightgen.synthetic_frames(200, 1, 1080, 1920))
        for a in ARITHS:
            m = CREStereoBase(iters=20, arithmetic=a)
            weightgen.fill_module_(m)
            models[a] = m.to(dev).eval()
            fwd[a] = (lambda m_: lambda: two_stage_forward(m_, f1, f2)[-1]["up_disp"])(models[a])
        what = "CREStereo, 1080x1920, 20 iters, 2-stage cascade, batch 1"
    else:
        raise SystemExit(f"unknown workload {workload!r}")
    return fwd, n, what, models, (f1, f2)


def time_workload(workload, dev, args):
    import torch
    fwd, n, what, models, _ = build(workload, dev)
    finals = {}
    for a in ARITHS:  # the first forward packs and calibrates; then the warm-up
        for _ in range(1 + args.warmup):
            finals[a] = fwd[a]()
        torch.cuda.synchronize(dev)
        assert torch.isfinite(finals[a]).all(), (workload, a)
    diff = (finals["fp16"] - finals["fp16x2"]).abs()
    ms = {a: [] for a in ARITHS}
    for r in range(args.rounds):
        for a in (ARITHS if r % 2 == 0 else ARITHS[::-1]):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                fwd[a]()
            torch.cuda.synchronize(dev)
            ms[a].append(1e3 * (time.perf_counter() - t0) / args.steps)
    row = {"kind": "workload", "workload": workload, "config": what, "pairs_per_forward": n, "steps": args.steps, "rounds": args.rounds,
           "warmup": args.warmup, "final_map_mean_abs_diff_px": diff.mean().item(), "final_map_max_abs_diff_px": diff.max().item()}
    for a in ARITHS:
        med = statistics.median(ms[a])
        row[a] = {"ms_per_forward_median": med, "ms_min_max": [min(ms[a]), max(ms[a])], "pairs_per_s": 1e3 * n / med}
    row["speedup_fp16_over_fp16x2"] = row["fp16x2"]["ms_per_forward_median"] / row["fp16"]["ms_per_forward_median"]
    log(f"{workload}: fp16x2 {row['fp16x2']['pairs_per_s']:.2f} pairs/s, fp16 {row['fp16']['pairs_per_s']:.2f} pairs/s "
        f"(x{row['speedup_fp16_over_fp16x2']:.3f}); final maps differ by {row['final_map_mean_abs_diff_px']:.2e} px mean-abs")
    return row


def time_convs(dev, args):
    """The stand-alone conv launches of the raft544 loop, inside the loop, per arithmetic (us per launch)."""
    import torch
    from nndepth_amd.cost_volume import CorrBlock1D
    fwd, _, _, models, (f1, f2) = build("raft544", dev)
    ctx = {}
    for a in ARITHS:
        m = models[a]
        fwd[a]()  # packs, calibrates
        eng = m.update_block.sync_engine(dev)
        fmap1, fmap2, cnet = m.forward_fnet(f1, f2)
        net, inp = torch.split(cnet, [m.hidden_dim, m.context_dim], dim=1)
        ctx[a] = (eng, CorrBlock1D(fmap1, fmap2, 4, 4)._pyr, torch.tanh(net).contiguous(), torch.relu(inp).contiguous())
    names = ctx["fp16"][0].conv_names()
    rows = []
    for i, nm in enumerate(names):
        if nm in ("encoder.convc1", "mask.2"):
            continue  # fused into lookup + convc1 / into mask + upsample: no launch of their own in the loop
        us = {a: [] for a in ARITHS}
        for r in range(args.rounds):
            for a in (ARITHS if r % 2 == 0 else ARITHS[::-1]):
                eng, pyr, net, inp = ctx[a]
                us[a].append(1e3 * eng.profile_loop_conv(i, pyr, 4, 4, net, inp, 8, 32))
        row = {"conv": nm if nm != "encoder.convf2" else "encoder.convf1+convf2 (merged with lookup+convc1)"}
        for a in ARITHS:
            row[a + "_us"] = statistics.median(us[a])
        row["ratio"] = row["fp16x2_us"] / row["fp16_us"]
        rows.append(row)
        log(f"  {row['conv']:<50} fp16x2 {row['fp16x2_us']:7.2f} us   fp16 {row['fp16_us']:7.2f} us   x{row['ratio']:.3f}")
    return {"kind": "loop_convs", "config": "raft544 loop (68x120, batch 1, 32 iterations), events around each launch inside the loop",
            "rounds": args.rounds, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="raft544,raft544_last,kitti8,cre1080,convs")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp16_bench.jsonl"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_fp16.py needs a HIP device (no CPU fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for w in args.workloads.split(","):
        row = time_convs(dev, args) if w == "convs" else time_workload(w, dev, args)
        row["device"] = torch.cuda.get_device_name(dev)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
