"""View synthesis + photometric error on one GPU (csrc/photometric.hip) against the same formula from eager PyTorch ops on the same
GPU (profiles/photometric_bench.jsonl; kernel times: profiles/photometric_kernels.txt).

Shapes 1x3x544x960 and 8x3x384x1248; input: tests/photometric_cases.py `scene` (a slanted plane, a nearer box, 0.2 px of noise,
rectangular holes in the mask) at ssim_weight 0.85.  Cases:

  error             geometry.photometric_error: the maps and the per-sample statistics (two launches)
  error_maps        the same without statistics (one launch)
  synthesize        geometry.synthesize_view alone
    hip     `--rounds` rounds of `--steps` back-to-back calls between two device events, median of the rounds: the launch path
            (Python wrapper + enqueue) as well as the kernels, NOT a kernel time
    eager   the same formula from PyTorch ops on the device: grid_sample along the row, F.pad(reflect) + avg_pool2d for the five
            means, the clamped quotient, the channel means, the `in` mask through a 3 x 3 min-pool and masked sums in float64;
            timed the same way, alternating with hip in one process
    compared before timing: the valid masks as integers (must be equal), the error on the valid pixels (eager rounds differently:
            the largest |difference| is reported, not asserted to be 0), the counts (equal) and the sums (relative difference)

Kernel times come from a separate run under the profiler, never from the windows above:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python scripts/bench_photometric.py --drive
    python scripts/bench_photometric.py --summarise DIR          # -> profiles/photometric_kernels.txt

    timeout -k 10 600 python scripts/bench_photometric.py [--cases error,error_maps,synthesize] [--steps 20] [--rounds 5]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((1, 3, 544, 960), (8, 3, 384, 1248))
CASES = ("error", "error_maps", "synthesize")
KERNELS = {"error": ("photometric_kernel", "photometric_stats_kernel"), "error_maps": ("photometric_kernel",), "synthesize": ("synthesize_kernel",)}
W_SSIM, HBM = 0.85, 8e12


def log(msg):
    print(f"[bench_photometric] {msg}", file=sys.stderr, flush=True)


def eager_sample(other, d, mask):
    """(rec, in) for a left-view map of negative sign and a valid mask."""
    import torch
    import torch.nn.functional as F
    B, C, H, W = other.shape
    m = -d[:, 0]
    xr = torch.arange(W, dtype=torch.float32, device=d.device).view(1, 1, W) - m
    inn = mask[:, 0].bool() & torch.isfinite(m) & (m >= 0) & (xr >= 0) & (xr <= W - 1)
    gx = 2.0 * torch.where(inn, xr, torch.zeros_like(xr)) / (W - 1) - 1.0
    gy = (2.0 * torch.arange(H, dtype=torch.float32, device=d.device) / (H - 1) - 1.0).view(1, H, 1).expand(B, H, W)
    rec = F.grid_sample(other, torch.stack([gx, gy], dim=-1), mode="bilinear", padding_mode="border", align_corners=True)
    return rec, inn


def eager_error(target, other, d, mask, stats=True):
    """(error, valid uint8, stats or None) as geometry.photometric_error defines them, from framework operations."""
    import torch
    import torch.nn.functional as F
    rec, inn = eager_sample(other, d, mask)
    pool = lambda v: F.avg_pool2d(F.pad(v, (1, 1, 1, 1), mode="reflect"), 3, 1)  # noqa: E731
    c1, c2 = 0.02 ** 2, 0.06 ** 2
    mx, my = pool(target), pool(rec)
    sx, sy, sxy = pool(target * target) - mx * mx, pool(rec * rec) - my * my, pool(target * rec) - mx * my
    ds = torch.clamp((1 - (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sx + sy + c2))) / 2, 0, 1).mean(1, keepdim=True)
    l1 = ((target - rec).abs() * 0.5).mean(1, keepdim=True)
    e = W_SSIM * ds + (1 - W_SSIM) * l1
    in9 = -F.max_pool2d(F.pad(-inn[:, None].float(), (1, 1, 1, 1), mode="reflect"), 3, 1) > 0.5
    valid = in9 & torch.isfinite(e)
    zero = torch.zeros_like(e)
    error = torch.where(valid, e, zero)
    st = None
    if stats:
        v64 = valid.double()
        st = torch.stack([v64.sum((1, 2, 3)), torch.where(valid, e, zero).double().sum((1, 2, 3)), torch.where(valid, l1, zero).double().sum((1, 2, 3)),
                          torch.where(valid, ds, zero).double().sum((1, 2, 3))], dim=1)
    return error, valid.to(torch.uint8), st


def alternate(sides, steps, args):
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
            for _ in range(steps):
                sides[k]()
            b.record()
            b.synchronize()
            us[k].append(1e3 * a.elapsed_time(b) / steps)
    return us


def make_input(shape, dev):
    import numpy as np
    import torch
    import photometric_cases as Pc
    t, o, d, mask = Pc.scene(shape, 500 + shape[0])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return to(t), to(o), to(d), to(mask)


def sides_of(name, tt, oo, dd, mm, ws):
    from nndepth_amd import geometry
    if name == "error":
        return (lambda: geometry.photometric_error(tt, oo, dd, valid_mask=mm, ssim_weight=W_SSIM, workspace=ws),
                lambda: eager_error(tt, oo, dd, mm))
    if name == "error_maps":
        return (lambda: geometry.photometric_error(tt, oo, dd, valid_mask=mm, ssim_weight=W_SSIM, stats=False),
                lambda: eager_error(tt, oo, dd, mm, stats=False))
    return lambda: geometry.synthesize_view(oo, dd, valid_mask=mm), lambda: eager_sample(oo, dd, mm)


def algorithmic_bytes(name, shape):
    B, C, H, W = shape
    return B * H * W * (((2 * C + 1) * 4 + 4) if name != "synthesize" else ((C + 1) * 4 + 1 + C * 4 + 1))


def bench_case(name, shape, dev, args):
    import torch
    from nndepth_amd import geometry
    B, C, H, W = shape
    tt, oo, dd, mm = make_input(shape, dev)
    ws = torch.empty(geometry.photometric_workspace_bytes(B, H, W) // 8, dtype=torch.float64, device=dev)
    hip, eager = sides_of(name, tt, oo, dd, mm, ws)
    got, ref = hip(), eager()
    cmp = {}
    if name == "synthesize":
        valid = got[1].bool()[:, 0]
        cmp["valid_equal"] = bool(torch.equal(valid, ref[1]))
        cmp["max_abs_diff_valid"] = float(((got[0] - ref[0]).abs() * valid[:, None]).max())
    else:
        valid = got[1].bool()
        cmp["valid_equal"] = bool(torch.equal(got[1], ref[1]))
        cmp["max_abs_diff_valid"] = float(((got[0] - ref[0]).abs() * valid).max())
        if got[2] is not None:
            cmp["count_equal"] = bool(torch.equal(got[2][:, 0], ref[2][:, 0]))
            cmp["sums_max_rel_diff"] = float(((got[2][:, 1:] - ref[2][:, 1:]).abs() / ref[2][:, 1:].abs().clamp(min=1e-30)).max())
    cmp["valid_share"] = float(valid.float().mean())
    us = alternate({"hip": hip, "eager": eager}, args.steps, args)
    med = {k: statistics.median(v) for k, v in us.items()}
    nbytes = algorithmic_bytes(name, shape)
    row = {"kind": name, "B": B, "C": C, "H": H, "W": W, "ssim_weight": W_SSIM, "steps": args.steps, "rounds": args.rounds, "compared": cmp,
           "algorithmic_bytes": nbytes,
           "hip": {"us_per_call_median": med["hip"], "us_min_max": [min(us["hip"]), max(us["hip"])], "gb_per_s": nbytes / (med["hip"] * 1e-6) / 1e9},
           "eager": {"us_per_call_median": med["eager"], "us_min_max": [min(us["eager"]), max(us["eager"])]},
           "eager_over_hip": med["eager"] / med["hip"]}
    log(f"{name:10s} {B}x{C}x{H}x{W}: hip {med['hip']:8.1f} us, eager {med['eager']:9.1f} us (x{row['eager_over_hip']:.1f}), {cmp}")
    return row


def drive(dev):
    import torch
    from nndepth_amd import geometry
    for shape in SHAPES:
        tt, oo, dd, mm = make_input(shape, dev)
        ws = torch.empty(geometry.photometric_workspace_bytes(shape[0], shape[2], shape[3]) // 8, dtype=torch.float64, device=dev)
        for name in CASES:
            hip = sides_of(name, tt, oo, dd, mm, ws)[0]
            for _ in range(5):
                hip()
            torch.cuda.synchronize()
            log(f"drove {name} {shape}")


def summarise(directory, out_path):
    """The trace holds, per shape and case in the order `drive` ran them, 5 launches of each of the case's kernels."""
    path = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(path)) if "photometric_" in r["Kernel_Name"] or "synthesize_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    lines = ["# rocprofv3 --kernel-trace over `python scripts/bench_photometric.py --drive` on the MI355X: 5 calls per case; per kernel the",
             "# average, smallest and largest time; GB/s = the algorithmic bytes of the call over the average of the main kernel ((2C+1) x 4",
             "# read + 4 written per pixel for the error; pictures, map and masks for synthesize) and its share of 8 TB/s"]
    pos = 0
    for shape in SHAPES:
        B, C, H, W = shape
        for name in CASES:
            n = 5 * len(KERNELS[name])
            chunk, pos = rows[pos:pos + n], pos + n
            assert len(chunk) == n, f"the trace does not match --drive at {name}"
            for kernel in KERNELS[name]:
                us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in chunk if kernel in r["Kernel_Name"]]
                assert len(us) == 5, f"{len(us)} launches of {kernel} at {name} {shape}"
                avg = sum(us) / 5
                line = f"{name} {B}x{C}x{H}x{W} {kernel}: avg {avg:8.1f} us  min {min(us):8.1f}  max {max(us):8.1f}"
                if "stats" not in kernel:
                    nbytes = algorithmic_bytes(name, shape)
                    line += f"  {nbytes / (avg * 1e-6) / 1e9:8.1f} GB/s ({100 * nbytes / (avg * 1e-6) / HBM:.2f} % of 8 TB/s)"
                lines.append(line)
    assert pos == len(rows), f"{len(rows)} launches in the trace, {pos} expected"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--drive", action="store_true", help="run every case 5 times for a profiler, time nothing")
    ap.add_argument("--summarise", metavar="DIR", help="write the kernel table of a rocprofv3 --kernel-trace csv directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photometric_bench.jsonl"))
    ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "photometric_kernels.txt"))
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.kernels_out)
    import torch
    assert torch.cuda.is_available(), "bench_photometric.py needs a HIP device (no CPU fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.drive:
        return drive(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rows = [{"kind": "context", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
             "note": "us_per_call = events around back-to-back calls: launch path + kernels, not a kernel time; eager = the same formula from "
                     "PyTorch ops on the same device, which rounds differently: the masks are compared as integers, the errors by their "
                     "largest difference on the valid pixels"}]
    for name in [c for c in args.cases.split(",") if c]:
        for shape in SHAPES:
            rows.append(bench_case(name, shape, dev, args))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
