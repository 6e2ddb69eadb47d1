"""Scene types on one GPU: the coloured view on the device against the host route (profiles/scene_bench.jsonl).

For a 544x960 and a 1080x1920 single map and a 384x1248 batch of 8:
  device route   Disparity(map).get_view_tensor(table) (nnd_view_range + nnd_colorize) and the copy of the uint8 picture to
                 the host; `device_ms` is the kernels alone (events), `device_route_ms` the wall time including the copy
  host route     map.cpu() and the numpy float64 closed form of the view on the host (the arithmetic matplotlib does in the
                 reference's get_view, without its masked-array overhead)
and Disparity.resize(maxpool) with an occlusion mask, 2x1x480x640 -> 240x320.

Context, measured on a CPU-only container and NOT by this script (the reference does not travel with the repository): the
reference's own get_view, one call on the CPU, takes 29-59 ms on a 544x960 map depending on the colormap, 13 ms on a 384x384
depth map with a valid mask; its Disparity.resize(maxpool) with an occlusion mask takes 6-14 ms for 2x1x480x640.

Method: 5 warm-up calls, then the median of 30 (device) / 5 (host) timed calls, min and max beside it; events around the device
part; bytes moved per call beside the time.  These kernels move a few MB per launch: at 544x960 they sit near the launch-latency
floor, far from the HBM line, so `gb_per_s` says how far, not how good.  No pass / fail threshold.  Needs no matplotlib.

    timeout -k 10 300 python scripts/bench_scene.py [--out profiles/scene_bench.jsonl]
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


def host_view(data: np.ndarray, table: np.ndarray) -> np.ndarray:
    """The closed form of Disparity.get_view for (B,C,H,W) on the host, float64 (tests/test_scene_cpu.py pins it)."""
    N = table.shape[0]
    pics = []
    for b in range(data.shape[0]):
        v = np.abs(data[b])
        lo, hi = float(v.min()), float(v.max())
        x = np.clip(v[0].astype(np.float64), lo, hi)
        n = np.zeros_like(x) if lo == hi else (x - lo) / (hi - lo)
        t = n * N
        idx = np.where(t == N, N - 1, t.astype(np.int64))
        pics.append(table[np.clip(idx, 0, N - 1)])
    return np.stack(pics)


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


def wall_ms(fn, warmup, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bench.jsonl"))
    args = ap.parse_args()
    from nndepth_amd.scene import Disparity
    assert torch.cuda.is_available(), "bench_scene.py needs the MI355X"
    table_host = np.load(os.path.join(ROOT, "tests", "golden", "scene.npz"))["table_RdYlGn"]
    table = torch.from_numpy(table_host).to(DEV)
    rows = [{"what": "context", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
             "note": "kernels of a few MB: near the launch-latency floor at 544x960, not the HBM line; box-to-box +-5 %"}]
    g = torch.Generator().manual_seed(0)
    for B, H, W in ((1, 544, 960), (1, 1080, 1920), (8, 384, 1248)):
        yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        disp = (-60 * (0.55 + 0.45 * torch.sin(3 * xx) * torch.cos(2 * yy)) + 0.3 * torch.randn(B, 1, H, W, generator=g)).to(DEV)
        obj = Disparity(disp, "negative")
        same = np.array_equal(obj.get_view_tensor(cmap=table).cpu().numpy(), host_view(disp.cpu().numpy(), table_host))
        dev = device_ms(lambda: obj.get_view_tensor(cmap=table))
        route = wall_ms(lambda: obj.get_view_tensor(cmap=table).cpu(), 5, 30)
        host = wall_ms(lambda: host_view(disp.cpu().numpy(), table_host), 1, 5)
        d2h_f32 = wall_ms(lambda: disp.cpu(), 3, 10)
        nbytes = 2 * 4 * B * H * W + 3 * B * H * W  # the map read twice (range, colour), the picture written once
        row = {"what": "view", "B": B, "H": H, "W": W, "table": "RdYlGn", "byte_identical_to_host_closed_form": bool(same),
               "device_ms": med(dev), "device_bytes": nbytes, "gb_per_s": nbytes / (statistics.median(dev) * 1e-3) / 1e9,
               "device_route_ms": med(route), "host_route_ms": med(host), "d2h_float_map_ms": med(d2h_f32),
               "speedup_route": statistics.median(host) / statistics.median(route)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    B, H, W = 2, 480, 640
    disp = (-torch.rand(B, 1, H, W, generator=g) * 80).to(DEV)
    occ = (torch.rand(B, 1, H, W, generator=g) < 0.2).to(DEV)
    dev = device_ms(lambda: Disparity(disp, "negative", occ).resize((240, 320), "maxpool"))
    nbytes = 4 * B * H * W + (4 + 1 + 1) * B * 240 * 320  # map read; values, gathered and source occlusion bytes
    row = {"what": "resize_maxpool_occlusion", "B": B, "H": H, "W": W, "size": [240, 320], "device_ms": med(dev),
           "device_bytes": nbytes, "gb_per_s": nbytes / (statistics.median(dev) * 1e-3) / 1e9}
    rows.append(row)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
