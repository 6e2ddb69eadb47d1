"""The view warp and hole filling on one GPU (csrc/warp.hip) against the same results from eager PyTorch ops on the same GPU and
from `.cpu()` plus numpy (profiles/warp_fill_bench.jsonl; kernel times: profiles/warp_fill_kernels.txt).

Shapes 1x1x544x960 and 8x1x384x1248; input: tests/warp_cases.py `scene` (two planes, a foreground box, salt, blobs; 10 % masked
out).  Per shape:

  warp, warp_feats   geometry.warp_disparity (other view, valid, occluded, source; with three feature channels)
  fill               geometry.fill_holes ("min_abs", vertical) of the map masked by its own warp occlusion (about 20 % holes), with
                     a workspace kept across calls
    hip     `--rounds` rounds of `--steps` back-to-back calls between two device events, median of the rounds: the launch path
            (Python wrapper + enqueues) as well as the kernels, NOT a kernel time
    eager   the same outputs from PyTorch ops on the device: int64 keys and `scatter_reduce_("amax")` for the warp, `cummax` /
            `cummin` along the row and the column for the fill; timed the same way, alternating with hip
    host    `.cpu()` and the numpy oracle of tests/warp_cases.py, wall clock, `--host-reps` repeats, median
    equal   hip against eager and against host, before timing (bits of the maps, masks and sources as integers)
  occlusion          geometry.occlusion_from_warp (one forward at batch B) against geometry.occlusion (one at batch 2B), RAFT-Stereo
                     base, 32 iterations, last map only, at 1x544x960 on the TartanAir pair of tests/golden (synthetic weights:
                     nndepth_amd.weightgen); the share of pixels on which the two masks agree.  With synthetic weights the output
                     is no disparity of that scene (the row records the share of pixels with a usable sign), so the times count
                     and the agreement says nothing; hence:
  agreement          both masks of a left map whose right-view map is known in closed form: a slanted background plane (it
                     stretches in the right view: the cracks) and a fronto-parallel box in front of it, `lr_consistency` against
                     the exact right map, `warp_disparity` on the left map alone, both at threshold 1

Kernel times come from a separate run under the profiler, never from the windows above:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python scripts/bench_warp_fill.py --drive
    python scripts/bench_warp_fill.py --summarise DIR          # -> profiles/warp_fill_kernels.txt

    timeout -k 10 600 python scripts/bench_warp_fill.py [--ops warp,warp_feats,fill,occlusion] [--steps 20] [--rounds 5]
"""
import argparse
import collections
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((1, 544, 960), (8, 384, 1248))
OPS = ("warp", "warp_feats", "fill", "occlusion", "agreement")
THRESHOLD, HBM = 1.0, 8e12


def log(msg):
    print(f"[bench_warp_fill] {msg}", file=sys.stderr, flush=True)


def eager_warp(d, mask, feats, thr):
    """disp negative, to the right view: (disp_other, valid_other, occluded, source[, features_other])"""
    import torch
    B, _, H, W = d.shape
    m = -d + 0.0
    x = torch.arange(W, device=d.device, dtype=torch.float32).expand_as(d)
    t = torch.round(x - m)  # half to even
    lands = mask.bool() & torch.isfinite(m) & (m >= 0) & (t >= 0) & (t <= W - 1)
    ti = torch.where(lands, t, torch.zeros_like(t)).long()
    key = (m.view(torch.int32).long() << 32) | (W - x.long())
    key = torch.where(lands, key, torch.zeros_like(key))
    best = torch.zeros_like(key).scatter_reduce_(3, ti, key, "amax", include_self=True)
    won = best != 0
    m_win = (best >> 32).to(torch.int32).view(torch.float32)
    source = torch.where(won, W - (best & 0xffffffff), torch.full_like(best, -1)).to(torch.int32)
    other = torch.where(won, -m_win, torch.zeros_like(m_win))
    occluded = ~(lands & ((torch.gather(m_win, 3, ti) - m) <= thr))
    out = (other, won.to(torch.uint8), occluded.to(torch.uint8), source)
    if feats is not None:
        g = torch.gather(feats, 3, source.clamp(min=0).long().expand_as(feats))
        out += (torch.where(won.expand_as(feats), g, torch.zeros_like(g)),)
    return out


def _nearest(ok, dim):
    import torch
    n = ok.shape[dim]
    shape = [1] * ok.ndim
    shape[dim] = n
    idx = torch.arange(n, device=ok.device).view(shape).expand_as(ok)
    before = torch.cummax(torch.where(ok, idx, torch.full_like(idx, -1)), dim).values
    after = torch.cummin(torch.where(ok, idx, torch.full_like(idx, n)).flip(dim), dim).values.flip(dim)
    return idx, before, torch.where(after == n, torch.full_like(after, -1), after)


def eager_fill(d, mask):
    """min_abs, vertical, fill 0, a valid mask: (filled, was_filled, mask_out)"""
    import torch
    ok = mask.bool() & torch.isfinite(d)

    def one_pass(values, have, dim):
        _, a, b = _nearest(have, dim)
        va, vb = torch.gather(values, dim, a.clamp(min=0)), torch.gather(values, dim, b.clamp(min=0))
        first = torch.where(b < 0, torch.ones_like(have), torch.where(a < 0, torch.zeros_like(have), va.abs() <= vb.abs()))
        return torch.where(first, va, vb), (a >= 0) | (b >= 0)

    row, _ = one_pass(d, ok, 3)
    nonempty = ok.any(dim=3, keepdim=True).expand_as(ok)
    out = torch.where(nonempty, row, torch.zeros_like(row))
    col, reach = one_pass(out, nonempty, 2)
    reach = reach & ~nonempty
    out = torch.where(ok, d, torch.where(reach, col, out))
    has = nonempty | reach
    return out, (has & ~ok).to(torch.uint8), has.to(torch.uint8)


def same(a, b):
    import torch
    raw = lambda t: t if t.dtype == torch.uint8 else t.contiguous().view(torch.uint8)  # noqa: E731  bits, not values
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(raw(x), raw(y)) for x, y in zip(a, b))


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


def make_input(B, H, W, dev):
    import numpy as np
    import torch
    import warp_cases as Wc
    d, mask = Wc.scene((B, 1, H, W), 500 + B, "negative")
    feats = Wc.S.rng(B).random((B, 3, H, W)).astype(np.float32)
    occ = Wc.warp(d, "negative", "right", THRESHOLD, mask)[2]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return (d, mask, feats, occ == 0), (to(d), to(mask), to(feats), to(occ == 0))


def bench_op(op, B, H, W, dev, args):
    import torch
    import warp_cases as Wc
    from nndepth_amd import geometry
    (d, mask, feats, vis), (dd, mm, ff, vv) = make_input(B, H, W, dev)
    px = B * H * W
    if op == "fill":
        ws = torch.empty(geometry.fill_workspace_bytes(B, H, W) // 4, dtype=torch.int32, device=dev)
        hip = lambda: geometry.fill_holes(dd, vv, True, "min_abs", True, 0.0, ws)  # noqa: E731
        eager = lambda: eager_fill(dd, vv)  # noqa: E731
        host = lambda: Wc.fill_holes(dd.cpu().numpy(), vv.cpu().numpy(), True, "min_abs", True, 0.0)  # noqa: E731
        nbytes, extra = px * (4 + 1 + 4 + 1 + 1), {"holes": float(1.0 - vis.mean())}
    else:
        f_dev = ff if op == "warp_feats" else None
        hip = lambda: geometry.warp_disparity(dd, "negative", "right", THRESHOLD, mm, f_dev, 0.0, True)  # noqa: E731
        eager = lambda: eager_warp(dd, mm, f_dev, THRESHOLD)  # noqa: E731
        host = lambda: [a for a in Wc.warp(dd.cpu().numpy(), "negative", "right", THRESHOLD, mm.cpu().numpy(),  # noqa: E731
                                           None if f_dev is None else f_dev.cpu().numpy(), 0.0) if a is not None]
        nbytes, extra = px * (4 + 1 + 4 + 1 + 1 + 4 + (24 if f_dev is not None else 0)), Wc.collisions(d, "negative", "right", mask, THRESHOLD)
    got = hip()
    equal_eager = bool(same(got, eager()))
    equal_host = bool(same(got, [torch.from_numpy(a).to(dev) for a in host()]))
    us = alternate({"hip": hip, "eager": eager}, args)
    host_ms = []
    for _ in range(args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host()
        host_ms.append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in us.items()}
    row = {"kind": op, "B": B, "H": H, "W": W, "steps": args.steps, "rounds": args.rounds, "equal_eager": equal_eager, "equal_host": equal_host,
           "algorithmic_bytes": nbytes, **extra,
           "hip": {"us_per_call_median": med["hip"], "us_min_max": [min(us["hip"]), max(us["hip"])], "gb_per_s": nbytes / (med["hip"] * 1e-6) / 1e9},
           "eager": {"us_per_call_median": med["eager"], "us_min_max": [min(us["eager"]), max(us["eager"])]},
           "host": {"ms_per_call_median": statistics.median(host_ms), "ms_min_max": [min(host_ms), max(host_ms)], "reps": args.host_reps},
           "eager_over_hip": med["eager"] / med["hip"], "host_over_hip": statistics.median(host_ms) * 1e3 / med["hip"]}
    log(f"{op:10s} {B}x1x{H}x{W}: hip {med['hip']:8.1f} us ({row['hip']['gb_per_s']:.1f} GB/s of algorithmic bytes), eager {med['eager']:8.1f} us "
        f"(x{row['eager_over_hip']:.1f}), host {row['host']['ms_per_call_median']:.1f} ms (x{row['host_over_hip']:.0f}), "
        f"equal eager={equal_eager} host={equal_host}")
    return row


def tartanair_pair(dev):
    import numpy as np
    import torch
    from PIL import Image
    frames = []
    for side in ("left", "right"):
        img = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", f"tartanair_000000_{side}.png")).convert("RGB"))
        t = torch.from_numpy(img.copy()).permute(2, 0, 1)[None].float()
        t = torch.nn.functional.interpolate(t, (544, 960), mode="bilinear")
        frames.append(((t - 127.5) / 127.5).to(dev))
    return frames


def bench_occlusion(dev, args):
    import torch
    from nndepth_amd import geometry, weightgen
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    m = BaseRAFTStereo(iters=32, context_dim=64, outputs="last")
    weightgen.fill_module_(m)
    m = m.to(dev).eval()
    left, right = tartanair_pair(dev)
    from_warp = lambda: geometry.occlusion_from_warp(m, left, right, THRESHOLD)  # noqa: E731
    from_lr = lambda: geometry.occlusion(m, left, right, THRESHOLD)  # noqa: E731
    a, b = from_warp(), from_lr()
    torch.cuda.synchronize()
    ao, bo = a.occlusion != 0, b.occlusion != 0
    row = {"kind": "occlusion", "config": "RAFT-Stereo base (ctx 64), 1x544x960, 32 iters, outputs=\"last\", synthetic weights, TartanAir pair",
           "threshold": THRESHOLD, "masks_agree": (ao == bo).float().mean().item(), "occluded_from_warp": ao.float().mean().item(),
           "occluded_lr_consistency": bo.float().mean().item(), "both_occluded": (ao & bo).float().mean().item(),
           "disp_left_max_abs_diff_px": (a.data - b.data).abs().max().item(),
           "usable_sign_share": (torch.isfinite(a.data) & (a.data <= 0)).float().mean().item()}
    steps, args.steps = args.steps, max(2, args.steps // 10)
    us = alternate({"occlusion_from_warp": from_warp, "occlusion": from_lr}, args)
    row["steps"], args.steps = args.steps, steps
    for k, v in us.items():
        row[k] = {"ms_per_call_median": statistics.median(v) / 1e3, "ms_min_max": [min(v) / 1e3, max(v) / 1e3]}
    row["lr_over_warp"] = row["occlusion"]["ms_per_call_median"] / row["occlusion_from_warp"]["ms_per_call_median"]
    log(f"occlusion 1x544x960: from warp {row['occlusion_from_warp']['ms_per_call_median']:.2f} ms, lr_consistency at batch 2B "
        f"{row['occlusion']['ms_per_call_median']:.2f} ms (x{row['lr_over_warp']:.2f}); the masks agree on {100 * row['masks_agree']:.1f} % "
        f"({100 * row['occluded_from_warp']:.1f} % / {100 * row['occluded_lr_consistency']:.1f} % occluded)")
    return row


def bench_agreement(dev, H=544, W=960):
    """The exact pair of maps of a two-surface scene, magnitudes: background m = 4 + 0.02 x + 0.01 y, a box of m = 24 in front."""
    import torch
    from nndepth_amd import geometry
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    rows = (y >= H // 4) & (y < H // 4 + H // 2)
    left = torch.where(rows & (x >= W // 3) & (x < 2 * (W // 3)), torch.full_like(x, 24.0), 4.0 + 0.02 * x + 0.01 * y)
    # the right view: the box moved 24 columns to the left; the plane's point at x' = x - m(x) has x = (x' + 4 + 0.01 y) / 0.98
    xb = (x + 4.0 + 0.01 * y) / 0.98
    right = torch.where(rows & (x + 24.0 >= W // 3) & (x + 24.0 < 2 * (W // 3)), torch.full_like(x, 24.0), 4.0 + 0.02 * xb + 0.01 * y)
    dl, dr = (-left).float()[None, None].to(dev), (-right).float()[None, None].to(dev)
    lr = geometry.lr_consistency(dl, dr, THRESHOLD) != 0
    wp = geometry.warp_disparity(dl, "negative", "right", THRESHOLD)[2] != 0
    row = {"kind": "agreement", "scene": "plane 4 + 0.02 x + 0.01 y, box 24 over the middle third, exact right-view map", "H": H, "W": W,
           "threshold": THRESHOLD, "masks_agree": (lr == wp).float().mean().item(), "occluded_from_warp": wp.float().mean().item(),
           "occluded_lr_consistency": lr.float().mean().item(), "warp_only": (wp & ~lr).float().mean().item(),
           "lr_only": (lr & ~wp).float().mean().item()}
    log(f"agreement {H}x{W}: the masks agree on {100 * row['masks_agree']:.2f} % ({100 * row['occluded_from_warp']:.2f} % occluded by the warp, "
        f"{100 * row['occluded_lr_consistency']:.2f} % by lr_consistency; warp only {100 * row['warp_only']:.2f} %, lr only {100 * row['lr_only']:.2f} %)")
    return row


DRIVEN = ("warp", "warp_feats", "fill")


def drive(dev):
    import torch
    from nndepth_amd import geometry
    for B, H, W in SHAPES:
        _, (dd, mm, ff, vv) = make_input(B, H, W, dev)
        for op in DRIVEN:
            for _ in range(5):
                if op == "fill":
                    geometry.fill_holes(dd, vv, True, "min_abs", True)
                else:
                    geometry.warp_disparity(dd, "negative", "right", THRESHOLD, mm, ff if op == "warp_feats" else None, 0.0, True)
            torch.cuda.synchronize()
            log(f"drove {op} {B}x1x{H}x{W}")


def summarise(directory, out_path):
    """The trace holds, per shape and op in the order `drive` ran them, 5 launches of nnd::warp_row_kernel or 5 x 3 of nnd::fill_*."""
    path = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(path)) if "nnd::warp_row" in r["Kernel_Name"] or "nnd::fill_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    lines = ["# rocprofv3 --kernel-trace over `python scripts/bench_warp_fill.py --drive` on the MI355X: average of 5 launches per kernel;",
             "# `sum` = the kernels of one call; GB/s = the algorithmic bytes of the call over that sum (warp: map 4 + mask 1 read, map 4 +",
             "# two masks 1 + 1 + source 4 written, + 24 with three feature channels; fill: map 4 + mask 1 read, map 4 + two masks written;",
             "# the fill's workspace is not counted); share of 8 TB/s beside it"]
    pos = 0
    for B, H, W in SHAPES:
        for op in DRIVEN:
            n = 5 * (3 if op == "fill" else 1)
            chunk, pos = rows[pos:pos + n], pos + n
            assert len(chunk) == n and all(("fill_" in r["Kernel_Name"]) == (op == "fill") for r in chunk), f"the trace does not match --drive at {op}"
            by = collections.OrderedDict()
            for r in chunk:
                k = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("nnd::", "")
                by.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            total = sum(sum(v) / len(v) for v in by.values())
            nbytes = B * H * W * (11 if op == "fill" else 15 + (24 if op == "warp_feats" else 0))
            lines.append(f"{op} {B}x1x{H}x{W}: sum {total:9.1f} us, {nbytes / (total * 1e-6) / 1e9:8.1f} GB/s ({100 * nbytes / (total * 1e-6) / HBM:.2f} % of 8 TB/s)")
            for k, v in by.items():
                lines.append(f"    {k:18s} n {len(v)}  avg {sum(v) / len(v):9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}")
    assert pos == len(rows), f"{len(rows)} launches in the trace, {pos} expected"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", default=",".join(OPS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--drive", action="store_true", help="run every op 5 times for a profiler, time nothing")
    ap.add_argument("--summarise", metavar="DIR", help="write the kernel table of a rocprofv3 --kernel-trace csv directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_fill_bench.jsonl"))
    ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "warp_fill_kernels.txt"))
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.kernels_out)
    import torch
    assert torch.cuda.is_available(), "bench_warp_fill.py needs a HIP device (no CPU fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.drive:
        return drive(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rows = [{"kind": "context", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
             "note": "us_per_call = events around back-to-back calls: launch path + kernels, not a kernel time; eager = PyTorch ops on the same "
                     "device; host = .cpu() + numpy, wall clock"}]
    for op in [o for o in args.ops.split(",") if o]:
        for B, H, W in (SHAPES if op not in ("occlusion", "agreement") else SHAPES[:1]):
            rows.append(bench_occlusion(dev, args) if op == "occlusion" else bench_agreement(dev) if op == "agreement"
                        else bench_op(op, B, H, W, dev, args))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
