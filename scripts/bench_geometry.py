"""Stereo geometry on one GPU (csrc/geometry.hip): each HIP op against the same formula written in eager PyTorch ops, measured in
ONE process, alternating (profiles/geometry_bench.jsonl).

Ops, each at 1x1x544x960 and 8x1x384x1248 with a 70 % valid mask:
  to_depth         Disparity.to_depth with a mask        eager: negate, double divide, float cast, three compares, where
  to_disparity     Depth.to_disparity                    eager: c / (z + eps)
  points_map       Depth.to_points_map                   eager: two double products and quotients over cached pixel grids, stack, where
  points_compact   Depth.points_tensor, with and without 3 feature channels
                                                         eager: the dense points, permuted, indexed by the boolean mask (that
                                                         indexing synchronises with the host to size its result) + counts' cumsum
  lr_consistency   geometry.lr_consistency on a mirrored right map
                                                         eager: flip, floor, two gathers, mul mul add, compares
  both_views       geometry.pair_both_views              eager: two cats of a frame and a flipped frame
and `occlusion`: geometry.occlusion (one forward at batch 2B) against two separate forwards plus torch flips and the eager
left-right check, RAFT-Stereo base (ctx 64), 32 iterations.

Method: per op `--warmup` untimed calls of each side, then `--rounds` rounds; a round times `--steps` back-to-back calls of one side
between two device events, then of the other, order alternating by round.  `us_per_call` is that window over the calls: for
kernels of a few MB it is the launch path (Python wrapper + enqueue) as much as the kernel, which is what a serving loop pays; it
is NOT a kernel time.  `gb_per_s` = the bytes the algorithm has to move (computed from the shape, below) over that time, `of_8tb`
its share of 8 TB/s.  The eager side is checked against the HIP side on the same inputs before timing (`equal`); no pass / fail
threshold on speed.

    timeout -k 10 600 python scripts/bench_geometry.py [--ops ...] [--steps 50] [--rounds 5] [--out profiles/geometry_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((1, 544, 960), (8, 384, 1248))
OPS = ("to_depth", "to_disparity", "points_map", "points_compact", "points_compact_feats", "lr_consistency", "both_views")
FX, BASELINE, HBM = 320.0, 0.25, 8e12


def log(msg):
    print(f"[bench_geometry] {msg}", file=sys.stderr, flush=True)


def eager_to_depth(d, mask, fx, baseline):
    import torch
    m = -d
    z = (fx * baseline / m.double()).float()
    ok = mask.bool() & torch.isfinite(m) & (m > 0)
    return torch.where(ok, z, torch.zeros_like(z)), ok.to(torch.uint8)


def eager_points_map(z, mask, grids, K):
    import torch
    u, v = grids
    Z = z.double()
    X = ((u - K[0, 2].double()) * Z / K[0, 0].double()).float()
    Y = ((v - K[1, 2].double()) * Z / K[1, 1].double()).float()
    return torch.where(mask.bool(), torch.cat([X, Y, z], 1), torch.zeros((), device=z.device))


def eager_compact(z, mask, grids, K, feats):
    import torch
    pm = eager_points_map(z, mask, grids, K)
    keep = mask.bool()[:, 0]
    pts = pm.permute(0, 2, 3, 1)[keep]
    fo = feats.permute(0, 2, 3, 1)[keep] if feats is not None else None
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device=z.device), keep.flatten(1).sum(1).cumsum(0)])
    return pts, fo, off


def eager_lr(dl, dr_flipped, thr):
    import torch
    W = dl.shape[-1]
    mL, mR = -dl, -dr_flipped.flip(-1)
    x = torch.arange(W, device=dl.device, dtype=torch.float32).expand_as(dl)
    go = torch.isfinite(mL) & ~(mL < 0)
    xr = torch.where(go, x - mL, torch.zeros_like(mL))
    go = go & ~(xr < 0) & ~(xr > W - 1)
    xr = torch.where(go, xr, torch.zeros_like(xr))
    fl = torch.floor(xr)
    i0 = fl.long()
    i1 = (i0 + 1).clamp(max=W - 1)
    f = xr - fl
    s = torch.gather(mR, 3, i0) * (1 - f) + torch.gather(mR, 3, i1) * f
    err = torch.where(go, (mL - s).abs(), torch.full_like(mL, float("inf")))
    return (~(err <= thr)).to(torch.uint8)


def alternate(sides, args):
    """{name: fn} -> {name: [us per call, one per round]}; events around `steps` back-to-back calls, order alternating."""
    import torch
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in sides}
    names = list(sides)
    for r in range(args.rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                sides[k]()
            b.record()
            b.synchronize()
            us[k].append(1e3 * a.elapsed_time(b) / args.steps)
    return us


def summary(us):
    return {"us_per_call_median": statistics.median(us), "us_min_max": [min(us), max(us)]}


def bench_op(op, B, H, W, dev, args):
    import torch
    from nndepth_amd import geometry
    from nndepth_amd.scene import Camera, Depth, Disparity
    g = torch.Generator().manual_seed(B * 1000 + H)
    px = B * H * W
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    disp = (-60 * (0.55 + 0.45 * torch.sin(3 * xx) * torch.cos(2 * yy)) - 0.3 * torch.rand(B, 1, H, W, generator=g)).to(dev)
    mask = (torch.rand(B, 1, H, W, generator=g) < 0.7).to(dev)
    nvalid = int(mask.sum())
    K = torch.tensor([[FX, 0, W / 2], [0, FX, H / 2], [0, 0, 1]], device=dev)
    cam = Camera(K)
    depth = Disparity(disp, baseline=BASELINE).to_depth(cam).data
    grids = (torch.arange(W, device=dev, dtype=torch.float64).expand(B, 1, H, W), torch.arange(H, device=dev, dtype=torch.float64).view(1, 1, H, 1).expand(B, 1, H, W))
    feats = torch.rand(B, 3, H, W, generator=g).to(dev)
    if op == "to_depth":
        obj = Disparity(disp, baseline=BASELINE)
        hip = lambda: obj.to_depth(cam, valid_mask=mask)
        eager = lambda: eager_to_depth(disp, mask, FX, BASELINE)
        same = lambda a, e: torch.equal(a.data, e[0]) and torch.equal(a.valid_mask, e[1])
        nbytes = px * (4 + 1 + 4 + 1)
    elif op == "to_disparity":
        obj = Depth(depth)
        c = torch.tensor(-BASELINE * FX, device=dev)
        hip = lambda: obj.to_disparity(cam, BASELINE)
        eager = lambda: c / (depth + 1e-8)
        same = lambda a, e: torch.equal(a.data, e)
        nbytes = px * 8
    elif op == "points_map":
        obj = Depth(depth, mask)
        hip = lambda: obj.to_points_map(cam)
        eager = lambda: eager_points_map(depth, mask, grids, K)
        same = lambda a, e: torch.equal(a, e)
        nbytes = px * (4 + 1 + 12)
    elif op in ("points_compact", "points_compact_feats"):
        obj = Depth(depth, mask)
        f = feats if op.endswith("feats") else None
        hip = lambda: obj.points_tensor(cam, f)
        eager = lambda: eager_compact(depth, mask, grids, K, f)
        same = lambda a, e: (torch.equal(a[2], e[2]) and torch.equal(a[0][:nvalid], e[0])
                             and (f is None or torch.equal(a[1][:nvalid], e[1])))
        nbytes = px * 2 + nvalid * (4 + 12 + (24 if f is not None else 0))  # the mask twice; depth, point (, features in and out) per valid pixel
    elif op == "lr_consistency":
        right = disp.flip(-1).contiguous()
        hip = lambda: geometry.lr_consistency(disp, right, 1.0, right_flipped=True)
        eager = lambda: eager_lr(disp, right, 1.0)
        same = lambda a, e: torch.equal(a, e)
        nbytes = px * (4 + 4 + 1)
    elif op == "both_views":
        left, right = torch.rand(B, 3, H, W, generator=g).to(dev), torch.rand(B, 3, H, W, generator=g).to(dev)
        hip = lambda: geometry.pair_both_views(left, right)
        eager = lambda: (torch.cat([left, right.flip(-1)]), torch.cat([right, left.flip(-1)]))
        same = lambda a, e: torch.equal(a[0], e[0]) and torch.equal(a[1], e[1])
        nbytes = px * 3 * 4 * (2 + 4)
    else:
        raise SystemExit(f"unknown op {op!r}")
    equal = bool(same(hip(), eager()))
    us = alternate({"hip": hip, "eager": eager}, args)
    row = {"kind": "op", "op": op, "B": B, "H": H, "W": W, "valid_fraction": nvalid / px, "equal": equal, "steps": args.steps,
           "rounds": args.rounds, "algorithmic_bytes": nbytes, "hip": summary(us["hip"]), "eager": summary(us["eager"])}
    t = row["hip"]["us_per_call_median"] * 1e-6
    row["hip"]["gb_per_s"] = nbytes / t / 1e9
    row["hip"]["of_8tb"] = nbytes / t / HBM
    row["eager_over_hip"] = row["eager"]["us_per_call_median"] / row["hip"]["us_per_call_median"]
    log(f"{op:22s} {B}x1x{H}x{W}: hip {row['hip']['us_per_call_median']:8.1f} us ({row['hip']['gb_per_s']:7.1f} GB/s, "
        f"{100 * row['hip']['of_8tb']:.1f} % of 8 TB/s), eager {row['eager']['us_per_call_median']:8.1f} us, x{row['eager_over_hip']:.2f}, equal={equal}")
    return row


def bench_occlusion(B, H, W, dev, args):
    import torch
    from nndepth_amd import geometry, weightgen
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    m = BaseRAFTStereo(iters=32, context_dim=64, outputs="last")
    weightgen.fill_module_(m)
    m = m.to(dev).eval()
    left, right = (torch.cat(x).to(dev) for x in zip(*[weightgen.synthetic_frames(300 + i, 1, H, W) for i in range(B)]))

    def two_forwards():
        dl = m(left, right)[-1]["up_disp"]
        dr = m(right.flip(-1), left.flip(-1))[-1]["up_disp"]
        return dl, eager_lr(dl, dr, 1.0)

    one = lambda: geometry.occlusion(m, left, right, 1.0)
    a, (dl, occ) = one(), two_forwards()
    torch.cuda.synchronize()
    # the 2B batch runs the same kernels per sample; where a kernel's tiling depends on the batch, last bits may differ
    row = {"kind": "occlusion", "config": f"RAFT-Stereo base (ctx 64), {B}x{H}x{W}, 32 iters, outputs=\"last\"", "B": B, "H": H, "W": W,
           "disp_left_max_abs_diff_px": (a.data - dl).abs().max().item(), "mask_pixels_differing": int((a.occlusion != occ).sum()),
           "occluded_fraction": a.occlusion.float().mean().item()}
    steps, args.steps = args.steps, max(2, args.steps // 10)
    us = alternate({"one_2B_forward": one, "two_forwards_torch_flips": two_forwards}, args)
    row["steps"], args.steps = args.steps, steps
    for k, v in us.items():
        row[k] = {"ms_per_call_median": statistics.median(v) / 1e3, "ms_min_max": [min(v) / 1e3, max(v) / 1e3]}
    row["two_over_one"] = row["two_forwards_torch_flips"]["ms_per_call_median"] / row["one_2B_forward"]["ms_per_call_median"]
    log(f"occlusion {B}x{H}x{W}: one 2B forward {row['one_2B_forward']['ms_per_call_median']:.2f} ms, two forwards + flips "
        f"{row['two_forwards_torch_flips']['ms_per_call_median']:.2f} ms (x{row['two_over_one']:.3f})")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", default=",".join(OPS) + ",occlusion")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_bench.jsonl"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_geometry.py needs a HIP device (no CPU fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rows = [{"kind": "context", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
             "note": "us_per_call = events around back-to-back calls: launch path + kernel, not a kernel time; gb_per_s = algorithmic bytes over it"}]
    for op in args.ops.split(","):
        for B, H, W in SHAPES:
            rows.append(bench_occlusion(B, H, W, dev, args) if op == "occlusion" else bench_op(op, B, H, W, dev, args))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
