"""Times the LoFTR layer with full (softmax) attention in HIP against the same layer on the package's eager PyTorch token path on
the same GPU, with the HIP linear layer for context; appends JSON lines to profiles/loftr_full_bench.jsonl (or --out).

    python scripts/bench_loftr_full.py [--out PATH] [--rounds 5] [--e2e] [--profile-pass]

Method: per shape the three candidates alternate inside one process; a round of a candidate is `calls` back-to-back calls between
two device events (calls sized so that a round lasts >= ~20 ms), after a warm-up of every candidate at that shape; the figure is
the median of the rounds, with their min and max as the spread.  The comparison is against eager PyTorch (einsum + softmax, which
materialises the (N, L, S, H) scores), not against a fused library kernel.
--e2e adds CREStereoBase at 1080x1920 (padded to 1088), 20 iterations, linear against full, in pairs/s.
--profile-pass runs each HIP full layer shape a few times and nothing else: the workload of a separate
`rocprofv3 --kernel-trace --stats` run, whose full_attention_kernel time gives the attention's share of the fp32 matrix peak
(scripts/bench_loftr_full.py --share KERNEL_STATS_CSV turns it into the derived lines)."""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

DEV = "cuda:0"
SHAPES = ((1, 17, 30), (8, 17, 30), (1, 33, 60), (2, 33, 60), (1, 68, 120))  # N, H, W
D_MODEL, NHEAD = 256, 8
PEAK_FP32_MATRIX = 157.3e12  # FLOP/s, MI355X fp32 matrix peak
PROFILE_CALLS = 20


def attention_flops(n, h, w):
    return 4 * n * NHEAD * (h * w) ** 2 * 32


def layers():
    from nndepth_amd import ops, weightgen
    from nndepth_amd.cre_stereo import LoFTREncoderLayer
    tok = weightgen.fill_module_(LoFTREncoderLayer(D_MODEL, NHEAD, "full"), "bench.loftr.").eval().to(DEV)
    sd = {k: v.cpu() for k, v in tok.state_dict().items()}
    return (ops.LoftrEngine(D_MODEL, NHEAD, "full").load(sd, device=DEV), ops.LoftrEngine(D_MODEL, NHEAD, "linear").load(sd, device=DEV), tok)


def inputs(n, h, w):
    g = torch.Generator().manual_seed(1000 * h + w + n)
    return (torch.randn(n, D_MODEL, h, w, generator=g).to(DEV), torch.randn(n, D_MODEL, h, w, generator=g).to(DEV))


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls  # us per call


def bench_layers(rounds, emit):
    full, linear, tok = layers()
    for n, h, w in SHAPES:
        x, s = inputs(n, h, w)
        xt, st = (t.permute(0, 2, 3, 1).reshape(n, h * w, D_MODEL).contiguous() for t in (x, s))
        cands = {"hip_full": lambda: full.forward(x, s), "eager_full": lambda: tok(xt, st), "hip_linear": lambda: linear.forward(x, s)}
        calls = {}
        with torch.no_grad():
            got, want = cands["hip_full"](), cands["eager_full"]().reshape(n, h, w, D_MODEL).permute(0, 3, 1, 2)
            err = float((got - want).abs().max())
            for k, fn in cands.items():  # warm-up, and the number of calls that fills ~20 ms
                timed(fn, 3)
                calls[k] = max(3, min(2000, int(20e3 / max(timed(fn, 3), 1.0))))
            t = {k: [] for k in cands}
            for _ in range(rounds):
                for k, fn in cands.items():
                    t[k].append(timed(fn, calls[k]))
        rec = {"what": "loftr_layer", "N": n, "H": h, "W": w, "tokens": h * w, "rounds": rounds, "attention_flops": attention_flops(n, h, w),
               "hip_full_vs_eager_max_abs": err}
        for k in cands:
            rec[k + "_us"] = {"median": round(statistics.median(t[k]), 2), "min": round(min(t[k]), 2), "max": round(max(t[k]), 2),
                              "calls_per_round": calls[k]}
        rec["eager_over_hip_full"] = round(rec["eager_full_us"]["median"] / rec["hip_full_us"]["median"], 3)
        emit(rec)


def bench_e2e(rounds, emit):
    from nndepth_amd import weightgen
    from nndepth_amd.cre_stereo import CREStereoBase
    f1, f2 = (t.to(DEV) for t in weightgen.synthetic_frames(7, 1, 1088, 1920))  # 1080 rows padded to a multiple of 32
    models = {a: weightgen.fill_module_(CREStereoBase(iters=20, attention=a, outputs="last"), "bench.cre.").eval().to(DEV)
              for a in ("linear", "full")}
    t = {a: [] for a in models}
    for a, m in models.items():
        for _ in range(2):
            m(f1, f2)
    for _ in range(rounds):
        for a, m in models.items():
            t[a].append(timed(lambda: m(f1, f2), 3))
    rec = {"what": "cre_stereo_1080x1920_it20", "rounds": rounds, "arithmetic": models["linear"].arithmetic}
    for a in models:
        rec[a + "_pairs_per_s"] = {"median": round(1e6 / statistics.median(t[a]), 3), "min": round(1e6 / max(t[a]), 3),
                                   "max": round(1e6 / min(t[a]), 3)}
    emit(rec)


def profile_pass():
    full, _, _ = layers()
    with torch.no_grad():
        for n, h, w in SHAPES:
            x, s = inputs(n, h, w)
            for _ in range(PROFILE_CALLS):
                full.forward(x, s)
    torch.cuda.synchronize()


def share(trace_csv, emit):
    """Per shape: the mean time of full_attention_kernel from a kernel-trace CSV of --profile-pass (the launches come in the order
    of SHAPES, PROFILE_CALLS each; the first of each shape is dropped as warm-up)."""
    rows = [r for r in csv.DictReader(open(trace_csv)) if "full_attention_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == PROFILE_CALLS * len(SHAPES), f"{len(rows)} launches of full_attention_kernel in the trace"
    for i, (n, h, w) in enumerate(SHAPES):
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows[i * PROFILE_CALLS + 1:(i + 1) * PROFILE_CALLS]]
        us = statistics.median(ns) / 1e3
        fl = attention_flops(n, h, w)
        emit({"what": "full_attention_kernel", "N": n, "H": h, "W": w, "attention_flops": fl, "kernel_us_median": round(us, 2),
              "kernel_us_min": round(min(ns) / 1e3, 2), "kernel_us_max": round(max(ns) / 1e3, 2),
              "tflops": round(fl / us / 1e6, 2), "share_of_fp32_matrix_peak": round(fl / (us * 1e-6) / PEAK_FP32_MATRIX, 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loftr_full_bench.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--share", metavar="KERNEL_TRACE_CSV")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")

    if a.share:
        return share(a.share, emit)
    if not torch.cuda.is_available():
        raise SystemExit("bench_loftr_full: no HIP device; a timing on the CPU says nothing")
    if a.profile_pass:
        return profile_pass()
    emit({"what": "run", "device": torch.cuda.get_device_name(0), "torch": torch.__version__})
    bench_layers(a.rounds, emit)
    if a.e2e:
        bench_e2e(a.rounds, emit)


if __name__ == "__main__":
    main()
