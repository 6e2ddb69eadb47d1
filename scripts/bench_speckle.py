"""Connected regions / speckle filter on one GPU (csrc/speckle.hip) against what a user does today: `.cpu()` and a host labelling
pass (profiles/speckle_bench.jsonl; kernel times: profiles/speckle_kernels.txt).

Shapes 1x1x544x960 and 8x1x384x1248; inputs (tests/speckle_cases.py): `scene` (two planes, salt noise, blobs, 10 % holes),
`constant` (one region: every size add of launch 3 lands on one address per sample) and `serpentine` (one path through every
tile: the longest label chains).  Per input and shape:

  hip       geometry.speckle_filter (filtered map, mask, speckle mask, sizes; 4 neighbours, max_size 64) with a workspace kept
            across calls: `--rounds` rounds of `--steps` back-to-back calls between two device events, median of the rounds.  That
            window is the launch path (Python wrapper + four enqueues) as well as the kernels: it is NOT a kernel time.
  host      the map and the mask copied to the host, then scipy.sparse.csgraph.connected_components on the contract's edge list
            and the size test in numpy (speckle_cases.regions_scipy); wall clock, `--host-reps` repeats, median.  Without scipy the
            numpy oracle of speckle_cases takes its place and the row says so.
  equal     the device's sizes and speckle mask against that host result, before timing

`--inputs serpentine --once`: ONE timed call after a warm-up on a small map of another shape (the code objects are loaded, the
path itself is walked cold); run it in a process of its own under its own time limit.

Kernel times come from a separate run under the profiler, never from the windows above:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python scripts/bench_speckle.py --drive
    python scripts/bench_speckle.py --summarise DIR          # -> profiles/speckle_kernels.txt

`--drive` runs every input and shape 5 times and times nothing.  The summary sets each kernel's average duration against the
bytes the algorithm has to move, computed from the shape: the map (4 B / px) and the mask (1 B / px) read, sizes and the filtered
map (4 B / px each) and the two masks (1 B / px each) written; labels (4 B / px) in place of the filtered map for
connected_regions.  The workspace traffic (9 B / px written by launch 1 and read again) is the method's own and is not counted.

    timeout -k 10 600 python scripts/bench_speckle.py [--inputs scene,constant] [--steps 20] [--rounds 5]
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
INPUTS = ("scene", "constant", "serpentine")
MAX_SIZE, MAX_DIFF, CONN, HBM = 64, 0.5, 4, 8e12
ALGO_BYTES_PER_PX = 4 + 1 + 4 + 4 + 1 + 1  # map, mask in; sizes, filtered, mask, speckle mask out


def log(msg):
    print(f"[bench_speckle] {msg}", file=sys.stderr, flush=True)


def make_input(name, B, H, W):
    import numpy as np
    import speckle_cases as S
    if name == "scene":
        d, mask, _ = S.scene((B, 1, H, W), 500 + B)
    elif name == "constant":
        d, mask = S.constant((B, 1, H, W))[0], np.ones((B, 1, H, W), bool)
    elif name == "serpentine":
        d = np.repeat(S.serpentine(H, W, 0, W - 1)[0], B, axis=0)
        mask = np.ones((B, 1, H, W), bool)
    else:
        raise SystemExit(f"unknown input {name!r}")
    return d, mask


def host_labelling():
    import speckle_cases as S
    try:
        import scipy  # noqa: F401
        return S.regions_scipy, "scipy.sparse.csgraph.connected_components"
    except ImportError:
        return S.regions, "numpy hook-and-compress (scipy is not installed)"


def bench(name, B, H, W, dev, args):
    import numpy as np
    import torch
    from nndepth_amd import geometry
    d, mask = make_input(name, B, H, W)
    dd, mm = torch.from_numpy(d).to(dev), torch.from_numpy(mask).to(dev)
    ws = torch.empty(geometry.regions_workspace_bytes(B, H, W) // 8 + 1, dtype=torch.int64, device=dev)
    hip = lambda: geometry.speckle_filter(dd, MAX_SIZE, MAX_DIFF, mm, True, CONN, 0.0, True, ws)  # noqa: E731
    label, label_name = host_labelling()

    def host():
        dh, mh = dd.cpu().numpy(), mm.cpu().numpy()
        _, sizes = label(dh, MAX_DIFF, mh, True, CONN)
        return sizes, (mh & np.isfinite(dh) & (sizes <= MAX_SIZE)).astype(np.uint8)

    if args.once:
        small = torch.zeros((1, 1, 40, 70), device=dev)
        geometry.speckle_filter(small, MAX_SIZE, MAX_DIFF, None, True, CONN, 0.0, True)
        torch.cuda.synchronize()
        steps, rounds = 1, 1
    else:
        for _ in range(args.warmup):
            hip()
        steps, rounds = args.steps, args.rounds
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            out = hip()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b) / steps)
    host_ms = []
    for _ in range(args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want_sizes, want_speckle = host()
        host_ms.append(1e3 * (time.perf_counter() - t0))
    equal = bool(np.array_equal(out[3].cpu().numpy(), want_sizes) and np.array_equal(out[2].cpu().numpy(), want_speckle))
    px = B * H * W
    med = statistics.median(us)
    row = {"kind": "speckle_filter", "input": name, "B": B, "H": H, "W": W, "connectivity": CONN, "max_size": MAX_SIZE,
           "max_diff": MAX_DIFF, "once": bool(args.once), "steps": steps, "rounds": rounds, "equal": equal,
           "removed_fraction": float(want_speckle.mean()), "largest_region": int(want_sizes.max()),
           "algorithmic_bytes": px * ALGO_BYTES_PER_PX,
           "hip": {"us_per_call_median": med, "us_min_max": [min(us), max(us)], "gb_per_s": px * ALGO_BYTES_PER_PX / (med * 1e-6) / 1e9},
           "host": {"labelling": label_name, "ms_per_call_median": statistics.median(host_ms), "ms_min_max": [min(host_ms), max(host_ms)],
                    "reps": args.host_reps},
           "host_over_hip": statistics.median(host_ms) * 1e3 / med}
    log(f"{name:10s} {B}x1x{H}x{W}: hip {med:9.1f} us per call ({row['hip']['gb_per_s']:.1f} GB/s of algorithmic bytes), host "
        f"{row['host']['ms_per_call_median']:.1f} ms, x{row['host_over_hip']:.0f}, equal={equal}")
    return row


def drive(dev, inputs):
    import torch
    from nndepth_amd import geometry
    for name in inputs:
        for B, H, W in SHAPES:
            d, mask = make_input(name, B, H, W)
            dd, mm = torch.from_numpy(d).to(dev), torch.from_numpy(mask).to(dev)
            for _ in range(5):
                geometry.speckle_filter(dd, MAX_SIZE, MAX_DIFF, mm, True, CONN, 0.0, True)
            torch.cuda.synchronize()
            log(f"drove {name} {B}x1x{H}x{W}")


def summarise(directory, out_path, inputs):
    """The trace holds, per input and shape in the order `drive` ran them, 5 x 4 launches of nnd::cc_* kernels."""
    path = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(path)) if "nnd::cc_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_case = 5 * 4
    cases = [(n, s) for n in inputs for s in SHAPES]
    assert len(rows) == per_case * len(cases), f"{len(rows)} cc_ launches in the trace, {per_case * len(cases)} expected"
    lines = ["# rocprofv3 --kernel-trace over `python scripts/bench_speckle.py --drive` on the MI355X: average of 5 launches per kernel;",
             "# `sum` = the four kernels of one speckle_filter call; GB/s = the algorithmic bytes of the call (15 B / px: map 4 + mask 1 read,",
             "# sizes 4 + filtered 4 + two masks 1 + 1 written; the 9 B / px workspace is not counted) over that sum; share of 8 TB/s beside it"]
    for ci, (name, (B, H, W)) in enumerate(cases):
        chunk = rows[ci * per_case:(ci + 1) * per_case]
        by = collections.OrderedDict()
        for r in chunk:
            k = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("nnd::", "")
            by.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        total = sum(sum(v) / len(v) for v in by.values())
        nbytes = B * H * W * ALGO_BYTES_PER_PX
        lines.append(f"{name} {B}x1x{H}x{W}: sum {total:9.1f} us, {nbytes / (total * 1e-6) / 1e9:8.1f} GB/s ({100 * nbytes / (total * 1e-6) / HBM:.2f} % of 8 TB/s)")
        for k, v in by.items():
            lines.append(f"    {k:18s} n {len(v)}  avg {sum(v) / len(v):9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="scene,constant")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one timed call after a warm-up on another shape (the serpentine)")
    ap.add_argument("--drive", action="store_true", help="run every input 5 times for a profiler, time nothing")
    ap.add_argument("--summarise", metavar="DIR", help="write the kernel table of a rocprofv3 --kernel-trace csv directory")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speckle_bench.jsonl"))
    ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "speckle_kernels.txt"))
    args = ap.parse_args()
    inputs = [i for i in args.inputs.split(",") if i]
    if args.summarise:
        return summarise(args.summarise, args.kernels_out, inputs)
    import torch
    assert torch.cuda.is_available(), "bench_speckle.py needs a HIP device (no CPU fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.drive:
        return drive(dev, inputs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rows = [] if args.append else [{"kind": "context", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
                                    "note": "hip us_per_call = events around back-to-back calls: launch path + kernels, not a kernel time; host = "
                                            ".cpu() + host labelling, wall clock"}]
    for name in inputs:
        for B, H, W in SHAPES:
            rows.append(bench(name, B, H, W, dev, args))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    with open(args.out, "a" if args.append else "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
