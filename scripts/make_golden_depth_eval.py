"""Fixture of the monocular evaluation criterion (tests/golden/depth_eval.npz, REPORT_depth_eval.txt).

Runs only where the reference checkout is importable (like scripts/make_golden_scene.py; it installs the stand-ins of
oracle/make_golden.py and changes nothing under oracle/), on the CPU.  The inputs of every case are a pure function of the
case's name (tests/depth_eval_cases.py: make_case, through nndepth_amd.weightgen), so no input array is stored, only:

  names      JSON list of the case names
  shapes     (ncases, 3) int64: B, H, W
  r          (ncases, 9) float64: what the reference's DepthEvalCriterion(max_depth=80) returns (fp32 results, held exactly)
  f          (ncases, 9) float64: the contract of nnd_depth_eval (include/nndepth_amd.h) evaluated in float64 with numpy here
  count      (ncases,) int64: the number of pixels in the metric mask

A case in which a finite r is further than 1e-5 * max(1, |f|) from f is refused: an ill-conditioned case would only loosen the
bar the GPU test derives from |r - f|.

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_depth_eval.py [path of the reference checkout; default: oracle's]
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


def contract64(pred: np.ndarray, gt: np.ndarray, mask, max_depth: float):
    """The contract in numpy float64: (nine metrics, pixels in the metric mask)."""
    B = pred.shape[0]
    valid = np.ones(gt.shape, bool) if mask is None else mask.astype(bool)
    p, g = pred.astype(np.float64), gt.astype(np.float64)
    a = p.copy()
    for b in range(B):
        m = valid[b]
        if m.sum() > 100:
            pv, gv = p[b][m], g[b][m]
            pm, gm = pv.mean(), gv.mean()
            spp, spg = np.sum((pv - pm) ** 2), np.sum((pv - pm) * (gv - gm))
            if spp == 0.0:  # constant prediction: the minimum-norm solution
                scale, shift = pm * gm / (pm * pm + 1.0), gm / (pm * pm + 1.0)
            else:
                scale = spg / spp
                shift = gm - scale * pm
            a[b] = p[b] * scale + shift
    mm = valid & (gt > np.float32(0.1)) & (gt < np.float32(max_depth))
    n = int(mm.sum())
    if n == 0:
        return np.array([math.inf] * 4 + [0.0] * 3 + [math.inf] * 2), 0
    av, gv = a[mm], g[mm]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = [np.mean(np.abs(av - gv) / gv), np.mean((av - gv) ** 2 / gv), np.sqrt(np.mean((av - gv) ** 2)),
               np.sqrt(np.mean((np.log(av) - np.log(gv)) ** 2))]
        ratio = np.maximum(av / gv, gv / av)
    out += [np.count_nonzero(ratio < 1.25 ** k) / n for k in (1, 2, 3)]
    gn = (g - gv.min()) / (gv.max() - gv.min() + 1e-6)
    an = (a - av.min()) / (av.max() - av.min() + 1e-6)
    diffs = []
    for b in range(B):
        m = mm[b]
        k = int(m.sum())
        if k == 0:
            continue
        ssi = []
        for x in (an[b][m], gn[b][m]):
            shift = np.partition(x, (k - 1) // 2)[(k - 1) // 2]  # the lower median
            scale = np.mean(np.abs(x - shift))
            ssi.append((x - shift) / (scale if scale != 0.0 else 1.0))
        diffs.append(ssi[0] - ssi[1])
    diffs = np.concatenate(diffs)
    out += [np.sum(np.abs(diffs)) / n, np.sqrt(np.sum(diffs ** 2) / n)]
    return np.array(out, np.float64), n


def main(ref_path):
    import oracle.make_golden as mg
    if ref_path:
        mg.REF = ref_path
    mg._install_standins()
    from nndepth.models.midas.scripts.evaluate import DepthEvalCriterion
    import depth_eval_cases as dc

    crit = DepthEvalCriterion(max_depth=dc.MAX_DEPTH)
    rep = ["DepthEvalCriterion: the reference's nndepth/models/midas/scripts/evaluate.py on the CPU in fp32 (r) against the float64 "
           f"statement of the contract (f); scripts/make_golden_depth_eval.py, torch {torch.__version__.split('+')[0]}, numpy {np.__version__}",
           f"refused above |r - f| = {CAP:g} * max(1, |f|); per case and metric: f, then |r - f|"]
    R, F, counts, shapes = [], [], [], []
    worst = 0.0
    for name, shape, _ in dc.CASES:
        pred, gt, mask = dc.make_case(name)
        res = crit(pred.clone(), gt.clone(), None if mask is None else mask.clone())
        assert tuple(res.keys()) == dc.METRICS
        r = np.array([res[k] for k in dc.METRICS], np.float64)
        f, n = contract64(pred.numpy(), gt.numpy(), None if mask is None else mask.numpy(), dc.MAX_DEPTH)
        rep.append(f"case {name:2s} {tuple(pred.shape)!s:18s} mask {'None' if mask is None else int(mask.sum())!s:>7s}  metric pixels {n}")
        for k, rv, fv in zip(dc.METRICS, r, f):
            if math.isfinite(fv) and math.isfinite(rv):
                e = abs(rv - fv)
                worst = max(worst, e / max(1.0, abs(fv)))
                if e > CAP * max(1.0, abs(fv)):
                    raise SystemExit(f"case {name} {k}: r = {rv!r}, f = {fv!r}: |r - f| = {e:.3e} is above the cap; the case is ill-conditioned")
                rep.append(f"    {k:9s} f = {fv:<22.15g} |r - f| = {e:.3e}")
            else:
                same = (math.isnan(rv) and math.isnan(fv)) or rv == fv
                if not same:
                    raise SystemExit(f"case {name} {k}: r = {rv!r} but f = {fv!r}")
                rep.append(f"    {k:9s} f = {float(fv)!r:<22s} r = {float(rv)!r}")
        R.append(r), F.append(f), counts.append(n), shapes.append(shape)
    rep.append(f"worst |r - f| / max(1, |f|) = {worst:.3e}")
    path = os.path.join(GOLD, "depth_eval.npz")
    np.savez_compressed(path, names=np.array(json.dumps(list(dc.NAMES))), shapes=np.array(shapes, np.int64), r=np.array(R), f=np.array(F),
                        count=np.array(counts, np.int64))
    rep.append(f"depth_eval.npz: {os.path.getsize(path)} bytes")
    with open(os.path.join(GOLD, "REPORT_depth_eval.txt"), "w") as fh:
        fh.write("\n".join(rep) + "\n")
    print("\n".join(rep))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
