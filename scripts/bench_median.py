"""The masked median and the guided weighted median on one GPU (csrc/median.hip) against the same bits from eager PyTorch ops on the
same GPU and from `.cpu()` plus numpy (profiles/median_bench.jsonl; kernel times: profiles/median_kernels.txt).

Shapes 1x1x544x960 and 8x1x384x1248; input: tests/median_cases.py `scene` (two planes, a foreground box, salt, blobs; about 20 %
holes) and a 3-channel guide (a step edge per plane plus noise).  Cases:

  r1, r2            geometry.median_filter, unweighted, radius 1 and 2, fill_invalid
  guided_r3         radius 3, the 3-channel guide, range_weights(0.2)
  guided_rmax       the largest radius, the same guide
    hip     `--rounds` rounds of `--steps` back-to-back calls between two device events, median of the rounds: the launch path
            (Python wrapper + enqueue) as well as the kernel, NOT a kernel time
    eager   the same bits from PyTorch ops on the device: the keys as float64 (exact to 2^53) through `F.unfold`, `sort`, `gather`
            of the weights, `cumsum`, `argmax`, `gather`; timed the same way, alternating with hip; windows above 49 taps with a
            tenth of the steps (a call materialises (2r+1)^2 copies of the map several times over)
    host    `.cpu()` and the numpy oracle of tests/median_cases.py, wall clock, on the first shape only (the oracle holds
            (2r+1)^2 int64 per pixel several times over: 7 GB per array at 8x1x384x1248 and radius 7)
    equal   hip against eager and against host, before timing (bits of the maps, masks as integers)
    rounds  the mean number of bisection rounds per pixel on this input (0 for the 3 x 3 and 5 x 5 networks): bit length of kmin ^ kmax

Kernel times come from a separate run under the profiler, never from the windows above:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python scripts/bench_median.py --drive
    python scripts/bench_median.py --summarise DIR          # -> profiles/median_kernels.txt

    timeout -k 10 600 python scripts/bench_median.py [--cases r1,r2,guided_r3,guided_rmax] [--steps 20] [--rounds 5]
"""
import argparse
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
CASES = ("r1", "r2", "guided_r3", "guided_rmax")
SIGMA, HBM = 0.2, 8e12
BAD = float(0xFFFFFFFF)


def log(msg):
    print(f"[bench_median] {msg}", file=sys.stderr, flush=True)


def case_of(name):
    """(radius, guided)"""
    from nndepth_amd import geometry
    return {"r1": (1, False), "r2": (2, False), "guided_r3": (3, True), "guided_rmax": (geometry.median_max_radius(), True)}[name]


def eager_keys(d, mask):
    import torch
    ok = mask.bool() & torch.isfinite(d)
    b = d.view(torch.int32).long() & 0xFFFFFFFF
    key = b ^ torch.where(b & 0x80000000 != 0, torch.full_like(b, 0xFFFFFFFF), torch.full_like(b, 0x80000000))
    return ok, torch.where(ok, key, torch.full_like(key, 0xFFFFFFFF)).double()


def eager_median(d, mask, r, guide, inv_step, table, min_count, fill_invalid, fill):
    """(filtered, mask_out) with a valid mask; table: the 256 weights as int64 on the device."""
    import torch
    import torch.nn.functional as F
    B, _, H, W = d.shape
    K = 2 * r + 1
    ok, key = eager_keys(d, mask)
    kt = F.unfold(F.pad(key, (r, r, r, r), value=BAD), K)  # (B, K*K, H*W)
    okt = kt != BAD
    if guide is None:
        w = okt.long()
    else:
        C = guide.shape[1]
        gt = F.unfold(F.pad(guide, (r, r, r, r)), K).view(B, C, K * K, H * W)
        dist = None
        for c in range(C):
            a = (guide[:, c].reshape(B, 1, H * W) - gt[:, c]).abs()
            dist = a if dist is None else dist + a
        s = dist * inv_step
        w = torch.where(okt, table[torch.where(s < 255.0, s, torch.full_like(s, 255.0)).long()], torch.zeros_like(okt, dtype=torch.long))
    ks, order = torch.sort(kt, dim=1, stable=True)
    ws = torch.gather(w, 1, order)
    T, n = w.sum(1, keepdim=True), okt.sum(1, keepdim=True)
    first = (2 * torch.cumsum(ws, 1) >= T).to(torch.uint8).argmax(1, keepdim=True)  # the first maximal value
    kstar = torch.gather(ks, 1, first).long().view(B, 1, H, W)
    vb = kstar ^ torch.where(kstar & 0x80000000 != 0, torch.full_like(kstar, 0x80000000), torch.full_like(kstar, 0xFFFFFFFF))
    vstar = ((vb + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32).view(torch.float32)
    produced = (ok | bool(fill_invalid)) & (n >= min_count).view(B, 1, H, W) & (T > 0).view(B, 1, H, W)
    out = torch.where(produced, vstar, torch.where(ok, d, torch.full_like(d, fill)))
    return out, (ok | produced).to(torch.uint8)


def mean_rounds(d, mask, r):
    """The mean over the pixels of the bisection rounds of their window: the bit length of kmin ^ kmax over the ok taps."""
    import torch
    import torch.nn.functional as F
    _, key = eager_keys(d, mask)
    K = 2 * r + 1
    total = 0.0
    for b in range(d.shape[0]):  # a sample at a time: (2r+1)^2 doubles per pixel
        kt = F.unfold(F.pad(key[b:b + 1], (r, r, r, r), value=BAD), K)
        kmin = kt.min(1).values
        kmax = torch.where(kt != BAD, kt, torch.zeros_like(kt)).max(1).values
        x = kmin.long() ^ kmax.long()
        bits = torch.where((x > 0) & (kmin != BAD), torch.floor(torch.log2(x.clamp(min=1).double())) + 1, torch.zeros_like(kmin))
        total += bits.sum().item()
    return total / d[:, 0].numel()


def same(a, b):
    import torch
    raw = lambda t: t if t.dtype == torch.uint8 else t.contiguous().view(torch.uint8)  # noqa: E731  bits, not values
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(raw(x), raw(y)) for x, y in zip(a, b))


def alternate(sides, steps, args):
    """{name: fn} -> {name: [us per call, one per round]}; events around `steps[name]` back-to-back calls, order alternating."""
    import torch
    for k, fn in sides.items():
        for _ in range(min(args.warmup, steps[k])):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in sides}
    names = list(sides)
    for r in range(args.rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps[k]):
                sides[k]()
            b.record()
            b.synchronize()
            us[k].append(1e3 * a.elapsed_time(b) / steps[k])
    return us


def make_input(B, H, W, dev):
    import numpy as np
    import torch
    import median_cases as Mc
    d, mask = Mc.scene((B, 1, H, W), 500 + B)
    g = Mc.S.rng(B)
    guide = (np.where(d > np.median(d), 0.7, 0.3)[:, [0, 0, 0]] + g.uniform(-0.05, 0.05, (B, 3, H, W))).astype(np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return (d, mask, guide), (to(d), to(mask), to(guide))


def bench_case(name, B, H, W, dev, args, with_host):
    import numpy as np
    import torch
    import median_cases as Mc
    from nndepth_amd import geometry
    r, guided = case_of(name)
    (d, mask, guide), (dd, mm, gg) = make_input(B, H, W, dev)
    table, inv_step = Mc.range_weights(SIGMA)
    table_dev = torch.from_numpy(table.astype(np.int64)).to(dev)
    g_dev, g_host = (gg, guide) if guided else (None, None)
    px, taps = B * H * W, (2 * r + 1) ** 2
    hip = lambda: geometry.median_filter(dd, r, mm, True, g_dev, SIGMA, fill_invalid=True)  # noqa: E731
    eager = lambda: eager_median(dd, mm, r, g_dev, float(inv_step), table_dev, 1, True, 0.0)  # noqa: E731
    host = lambda: Mc.median_filter(dd.cpu().numpy(), r, mm.cpu().numpy(), True, None if g_dev is None else g_dev.cpu().numpy(),  # noqa: E731
                                    inv_step, table, 1, True, 0.0)[:2]
    got = hip()
    equal_eager = bool(same(got, eager()))
    torch.cuda.empty_cache()
    steps = {"hip": args.steps, "eager": args.steps if taps <= 49 else max(1, args.steps // 10)}
    us = alternate({"hip": hip, "eager": eager}, steps, args)
    med = {k: statistics.median(v) for k, v in us.items()}
    nbytes = px * (10 + (12 if guided else 0))
    row = {"kind": name, "radius": r, "guide_channels": 3 if guided else 0, "B": B, "H": H, "W": W, "steps": steps, "rounds": args.rounds,
           "equal_eager": equal_eager, "algorithmic_bytes": nbytes, "holes": float(1.0 - (mask & np.isfinite(d)).mean()),
           "mean_bisection_rounds": 0.0 if not guided else mean_rounds(dd, mm, r),  # r1, r2: sorting networks
           "hip": {"us_per_call_median": med["hip"], "us_min_max": [min(us["hip"]), max(us["hip"])], "gb_per_s": nbytes / (med["hip"] * 1e-6) / 1e9},
           "eager": {"us_per_call_median": med["eager"], "us_min_max": [min(us["eager"]), max(us["eager"])]},
           "eager_over_hip": med["eager"] / med["hip"]}
    msg = (f"{name:12s} {B}x1x{H}x{W}: hip {med['hip']:9.1f} us ({row['hip']['gb_per_s']:.1f} GB/s of algorithmic bytes), eager "
           f"{med['eager']:11.1f} us (x{row['eager_over_hip']:.1f}), equal eager={equal_eager}")
    if with_host:
        host_ms, result = [], None
        for _ in range(args.host_reps if taps <= 49 else 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = host()
            host_ms.append(1e3 * (time.perf_counter() - t0))
        equal_host = bool(same(got, [torch.from_numpy(a).to(dev) for a in result]))
        row["equal_host"] = equal_host
        row["host"] = {"ms_per_call_median": statistics.median(host_ms), "ms_min_max": [min(host_ms), max(host_ms)], "reps": len(host_ms)}
        row["host_over_hip"] = statistics.median(host_ms) * 1e3 / med["hip"]
        msg += f", host {row['host']['ms_per_call_median']:.1f} ms (x{row['host_over_hip']:.0f}), equal host={equal_host}"
    log(msg)
    return row


def drive(dev):
    import torch
    from nndepth_amd import geometry
    for B, H, W in SHAPES:
        _, (dd, mm, gg) = make_input(B, H, W, dev)
        for name in CASES:
            r, guided = case_of(name)
            for _ in range(5):
                geometry.median_filter(dd, r, mm, True, gg if guided else None, SIGMA, fill_invalid=True)
            torch.cuda.synchronize()
            log(f"drove {name} {B}x1x{H}x{W}")


def summarise(directory, out_path, bench_path):
    """The trace holds, per shape and case in the order `drive` ran them, 5 launches of nnd::median_kernel."""
    path = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(path)) if "median_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    rounds = {}
    if os.path.exists(bench_path):
        for line in open(bench_path):
            j = json.loads(line)
            if "mean_bisection_rounds" in j:
                rounds[(j["kind"], j["B"], j["H"], j["W"])] = j["mean_bisection_rounds"]
    lines = ["# rocprofv3 --kernel-trace over `python scripts/bench_median.py --drive` on the MI355X: 5 launches of nnd::median_kernel per case;",
             "# GB/s = the algorithmic bytes of the call (map 4 + mask 1 read, map 4 + mask 1 written = 10 per pixel, + 12 with the 3-channel guide)",
             "# over the average, and its share of 8 TB/s; for the bisection paths ps per pixel, tap and round with the mean rounds per pixel of",
             "# this input (profiles/median_bench.jsonl): the whole kernel time, staging included, so an upper bound of the VALU time"]
    pos = 0
    for B, H, W in SHAPES:
        for name in CASES:
            chunk, pos = rows[pos:pos + 5], pos + 5
            assert len(chunk) == 5, f"the trace does not match --drive at {name}"
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in chunk]
            avg = sum(us) / 5
            radius = int(chunk[0]["Kernel_Name"].split("median_kernel<")[1].split(",")[0]) if "median_kernel<" in chunk[0]["Kernel_Name"] else -1
            guided = name.startswith("guided")
            nbytes = B * H * W * (10 + (12 if guided else 0))
            line = (f"{name} {B}x1x{H}x{W} (radius {radius}): avg {avg:9.1f} us  min {min(us):9.1f}  max {max(us):9.1f}  "
                    f"{nbytes / (avg * 1e-6) / 1e9:8.1f} GB/s ({100 * nbytes / (avg * 1e-6) / HBM:.2f} % of 8 TB/s)")
            mr = rounds.get((name, B, H, W))
            if mr and radius > 0:
                line += f"  {avg * 1e6 / (B * H * W * (2 * radius + 1) ** 2 * mr):.2f} ps per pixel-tap-round at {mr:.1f} rounds"
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
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--drive", action="store_true", help="run every case 5 times for a profiler, time nothing")
    ap.add_argument("--summarise", metavar="DIR", help="write the kernel table of a rocprofv3 --kernel-trace csv directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_bench.jsonl"))
    ap.add_argument("--kernels-out", default=os.path.join(ROOT, "profiles", "median_kernels.txt"))
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.kernels_out, args.out)
    import torch
    assert torch.cuda.is_available(), "bench_median.py needs a HIP device (no CPU fallback)"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.drive:
        return drive(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    rows = [{"kind": "context", "device": torch.cuda.get_device_name(dev), "torch": torch.__version__,
             "note": "us_per_call = events around back-to-back calls: launch path + kernel, not a kernel time; eager = PyTorch ops on the same "
                     "device; host = .cpu() + numpy, wall clock, first shape only"}]
    for name in [c for c in args.cases.split(",") if c]:
        for i, (B, H, W) in enumerate(SHAPES):
            rows.append(bench_case(name, B, H, W, dev, args, with_host=i == 0))
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
