"""Fixture of the stereo evaluation criterion (tests/golden/stereo_eval.npz, REPORT_stereo_eval.txt).

Runs only where the reference checkout is importable (like scripts/make_golden_depth_eval.py; it installs the stand-ins of
oracle/make_golden.py and changes nothing under oracle/), on the CPU.  The inputs of every case are a pure function of the
case's name (tests/stereo_eval_cases.py: make_case, through nndepth_amd.weightgen), so no input array is stored, only:

  names        JSON list of the case names
  columns      JSON list of the column names (epe, count, l1, the `above` keys, the `below` keys)
  <name>/r     (N, K) float64: the reference's own fp32 results, held exactly: epe and the `above` fractions from EvalCriterion
               (nndepth/models/raft_stereo/scripts/evaluate.py) called once per output; for the cases without a mask, the `below`
               fractions of the LAST output from RAFTLoss's metrics (nndepth/models/raft_stereo/loss.py).  NaN where the
               reference has no counterpart (<name>/has_r says which entries are results)
  <name>/has_r (N, K) bool
  <name>/f     (N, K) float64: the contract of nnd_stereo_eval (include/nndepth_amd.h) evaluated in float64 with numpy here
  <name>/counts (N, 1 + n_above + n_below) int64: valid pixels and the numerator of every fraction
  <name>/loss  (3,) float64: f's sequence loss, RAFTLoss's disp_loss (NaN for a case with a mask: RAFTLoss takes none), has_r

A case in which a finite r is further than 1e-5 * max(1, |f|) from f is refused: an ill-conditioned case would only loosen the
bar the GPU test derives from |r - f|.

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_stereo_eval.py [path of the reference checkout; default: oracle's]
"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
CAP = 1e-5


def gt_at(gt: np.ndarray, h: int, w: int) -> np.ndarray:
    """-max_pool2d(-gt, s) / s through the nearest source pixel, in numpy (s = W // w; floor pooling)."""
    B, C, H, W = gt.shape
    if (H, W) == (h, w):
        return gt
    s = W // w
    Hp, Wp = H // s, W // s
    pooled = gt[:, :, :Hp * s, :Wp * s].reshape(B, C, Hp, s, Wp, s).min(axis=(3, 5)) / np.float32(s)

    def src(n_out, n_in):
        ratio = np.float32(n_in) / np.float32(n_out)
        return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * ratio).astype(np.int64), n_in - 1)

    return pooled[:, :, src(h, Hp)][:, :, :, src(w, Wp)]


def contract64(gt, outputs, mask, max_flow, above, below, gamma):
    """The contract in numpy: fp32 per-pixel values, float64 sums.  ((N,K) metrics, loss, (N,1+na+nb) counts)."""
    rows, counts, loss = [], [], 0.0
    N = len(outputs)
    for i, p in enumerate(outputs):
        g = gt_at(gt, p.shape[2], p.shape[3]).astype(np.float32)
        d = (p - g).astype(np.float32)  # broadcasts a 1-channel ground truth
        se = np.zeros(d[:, 0].shape, np.float32)
        for c in range(d.shape[1]):
            se = se + d[:, c] * d[:, c]
        sg = np.zeros(g[:, 0].shape, np.float32)
        for c in range(g.shape[1]):
            sg = sg + g[:, c] * g[:, c]
        epe = np.sqrt(se)
        valid = np.sqrt(sg) < np.float32(max_flow)
        if mask is not None:
            valid = valid & mask[:, 0]
        e = epe[valid]
        n = int(e.size)
        l1 = float(np.sum(np.abs(d).astype(np.float64) * valid[:, None])) / p.size
        cnt = [n] + [int(np.count_nonzero(e > np.float32(t))) for t in above] + [int(np.count_nonzero(e < np.float32(t))) for t in below]
        rows.append([np.sum(e.astype(np.float64)) / n if n else math.nan, float(n), l1] + [c / n if n else math.nan for c in cnt[1:]])
        counts.append(cnt)
        loss += gamma ** (N - 1 - i) * l1
    return np.array(rows, np.float64), loss, np.array(counts, np.int64)


def main(ref_path):
    import oracle.make_golden as mg
    if ref_path:
        mg.REF = ref_path
    mg._install_standins()
    from nndepth.models.raft_stereo.loss import RAFTLoss
    from nndepth.models.raft_stereo.scripts.evaluate import EvalCriterion
    import stereo_eval_cases as sc

    assert tuple(sc.BELOW) == ("0.5px", "1px", "3px", "5px")  # RAFTLoss's metrics
    rep = ["StereoEvalCriterion: the reference's EvalCriterion (raft_stereo/scripts/evaluate.py) and RAFTLoss (raft_stereo/loss.py) on the "
           "CPU in fp32 (r) against the float64 statement of the contract (f); scripts/make_golden_stereo_eval.py, "
           f"torch {torch.__version__.split('+')[0]}, numpy {np.__version__}",
           f"refused above |r - f| = {CAP:g} * max(1, |f|); per case, output and column: f, then |r - f| (-: the reference has no counterpart)"]
    store = dict(names=np.array(json.dumps(list(sc.NAMES))), columns=np.array(json.dumps(list(sc.COLUMNS))))
    worst = 0.0

    def held(name, what, rv, fv):
        nonlocal worst
        if math.isfinite(fv) and math.isfinite(rv):
            e = abs(rv - fv)
            worst = max(worst, e / max(1.0, abs(fv)))
            if e > CAP * max(1.0, abs(fv)):
                raise SystemExit(f"case {name} {what}: r = {rv!r}, f = {fv!r}: |r - f| = {e:.3e} is above the cap; the case is ill-conditioned")
            return f"|r - f| = {e:.3e}"
        if not ((math.isnan(rv) and math.isnan(fv)) or rv == fv):
            raise SystemExit(f"case {name} {what}: r = {rv!r} but f = {fv!r}")
        return f"r = {float(rv)!r}"

    for name, gshape, outs in sc.CASES:
        case = sc.make_case(name)
        N = len(case.outputs)
        f, loss_f, counts = contract64(case.gt.numpy(), [o.numpy() for o in case.outputs], None if case.mask is None else case.mask.numpy(),
                                       case.max_flow, list(sc.ABOVE.values()), list(sc.BELOW.values()), sc.GAMMA)
        r = np.full((N, sc.K), np.nan)
        has = np.zeros((N, sc.K), bool)
        crit = EvalCriterion(dict(sc.ABOVE), max_flow=case.max_flow)
        for i, p in enumerate(case.outputs):
            res = crit(case.gt.clone(), p.clone(), None if case.mask is None else case.mask.clone())
            r[i, 0], has[i, 0] = res["epe"], True
            for k, key in enumerate(sc.ABOVE):
                r[i, 3 + k], has[i, 3 + k] = res[key], True
        loss_r, loss_has = math.nan, False
        if case.mask is None:
            dl, met = RAFTLoss(gamma=sc.GAMMA, max_flow=case.max_flow)(case.gt.clone(), [{"up_disp": p.clone()} for p in case.outputs])
            loss_r, loss_has = float(dl), True
            assert float(np.float32(met["epe"])) == r[N - 1, 0] or (math.isnan(met["epe"]) and math.isnan(r[N - 1, 0]))
            for k, key in enumerate(sc.BELOW):
                r[N - 1, 3 + len(sc.ABOVE) + k], has[N - 1, 3 + len(sc.ABOVE) + k] = met[key], True
        rep.append(f"case {name:2s} gt {gshape!s:18s} outputs {[tuple(o) for o in outs]!s}  mask "
                   f"{'None' if case.mask is None else int(case.mask.sum())}  max_flow {case.max_flow:g}")
        for i in range(N):
            rep.append(f"  output {i}: valid pixels {counts[i, 0]}")
            for k, col in enumerate(sc.COLUMNS):
                tail = held(name, f"output {i} {col}", r[i, k], f[i, k]) if has[i, k] else "-"
                rep.append(f"    {col:6s} f = {float(f[i, k])!r:<24s} {tail}")
        rep.append(f"  loss   f = {loss_f!r:<24s} " + (held(name, "loss", loss_r, loss_f) if loss_has else "-"))
        store.update({f"{name}/r": r, f"{name}/has_r": has, f"{name}/f": f, f"{name}/counts": counts,
                      f"{name}/loss": np.array([loss_f, loss_r, float(loss_has)])})
    rep.append(f"worst |r - f| / max(1, |f|) = {worst:.3e}")
    path = os.path.join(GOLD, "stereo_eval.npz")
    np.savez_compressed(path, **store)
    rep.append(f"stereo_eval.npz: {os.path.getsize(path)} bytes")
    with open(os.path.join(GOLD, "REPORT_stereo_eval.txt"), "w") as fh:
        fh.write("\n".join(rep) + "\n")
    print("\n".join(rep))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
