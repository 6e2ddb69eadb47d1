"""Fixture of the monocular loss value (tests/golden/midas_loss.npz, REPORT_midas_loss.txt).

Runs only where the reference checkout is importable (like scripts/make_golden_depth_eval.py; it installs the stand-ins of
oracle/make_golden.py and changes nothing under oracle/), on the CPU.  The inputs of every case are a pure function of the
case's name (tests/midas_loss_cases.py: make_case, through nndepth_amd.weightgen), so no input array is stored, only:

  names      JSON list of the case names
  shapes     (ncases, 3) int64: B, H, W
  r          (ncases, 4) float64: loss, trimmed_mae, gradient_reg, abs_dev as the reference's MiDasLoss() returns them in its
             metrics dict (fp32 results, held exactly); NaN x 4 where the reference raises (a batch without a valid pixel)
  f          (ncases, 4) float64: the contract of nnd_midas_loss (include/nndepth_amd.h) evaluated in float64 with numpy here
  n          (ncases,) int64: the valid pixels of the batch
  kept       (ncases,) int64: sum_b k_b, the pixels the trimmed error is taken over

A case in which a finite r is further than 1e-5 * max(1, |f|) from f is refused: an ill-conditioned case would only loosen the
bar the GPU test derives from |r - f|.

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_midas_loss.py [path of the reference checkout; default: oracle's]
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


def _windows(x: np.ndarray) -> np.ndarray:
    """(B,1,h,w) -> (B,1,h//2,w//2,4): the 2x2 stride-2 windows in row-major window order (floor sizes)."""
    h, w = x.shape[2] // 2 * 2, x.shape[3] // 2 * 2
    x = x[:, :, :h, :w]
    return np.stack([x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]], axis=-1)


def contract64(pred: np.ndarray, target: np.ndarray, mask: np.ndarray, coefs):
    """The contract in numpy float64: (four values, valid pixels, kept pixels)."""
    nan = float("nan")
    p, t, m = pred.astype(np.float64), target.astype(np.float64), mask.astype(bool)
    B = p.shape[0]
    n = int(m.sum())
    if n == 0:
        return np.full(4, nan), 0, 0
    tmin, tmax = t[m].min(), t[m].max()
    tn = (t - tmin) / (tmax - tmin + 1e-6)
    st, sp = np.full(t.shape, nan), np.full(t.shape, nan)
    for x, out in ((tn, st), (p, sp)):
        for b in range(B):
            nb = int(m[b].sum())
            if nb == 0:
                continue
            v = x[b][m[b]]
            shift = np.partition(v, (nb - 1) // 2)[(nb - 1) // 2]  # the lower median
            scale = np.mean(np.abs(v - shift))
            out[b] = (x[b] - shift) / (scale if scale != 0.0 else 1.0)
    e = np.abs(sp - st)
    abs_dev = e[m].sum() / n
    total, kept = 0.0, 0
    for b in range(B):
        nb = int(m[b].sum())
        trim = int(nb * 0.1)
        if trim == 0:
            continue
        k = nb - trim
        total += np.sort(e[b][m[b]])[:k].sum()
        kept += k
    trimmed = total / kept if kept else nan
    T, P, M = np.where(m, tn, 0.0), sp, m
    g = 0.0
    for _ in range(4):
        R = P - T
        term = np.abs(R[:, :, :-1, :-1] - R[:, :, :-1, 1:]) + np.abs(R[:, :, :-1, :-1] - R[:, :, 1:, :-1])
        g += term[M[:, :, 1:, 1:]].sum()
        wt, wm, wp = _windows(T), _windows(M), _windows(P)
        at = np.argmax(wt, axis=-1)[..., None]  # the first maximum; a NaN counts as the maximum
        T = np.take_along_axis(wt, at, -1)[..., 0]
        M = np.take_along_axis(wm, at, -1)[..., 0]
        P = (((wp[..., 0] + wp[..., 1]) + wp[..., 2]) + wp[..., 3]) / 4.0
    grad = g / n
    return np.array([trimmed * coefs[0] + grad * coefs[1], trimmed, grad, abs_dev], np.float64), n, kept


def main(ref_path):
    import oracle.make_golden as mg
    if ref_path:
        mg.REF = ref_path
    mg._install_standins()
    from nndepth.models.midas.loss import MiDasLoss
    import midas_loss_cases as mc

    crit = MiDasLoss(*mc.COEFS)
    rep = ["MiDasLoss: the reference's nndepth/models/midas/loss.py on the CPU in fp32 (r) against the float64 statement of the contract "
           f"(f); scripts/make_golden_midas_loss.py, torch {torch.__version__.split('+')[0]}, numpy {np.__version__}",
           f"refused above |r - f| = {CAP:g} * max(1, |f|); per case and value: f, then |r - f|"]
    R, Fv, N, K, shapes = [], [], [], [], []
    worst = 0.0
    for name, shape, _ in mc.CASES:
        pred, target, mask = mc.make_case(name)
        f, n, kept = contract64(pred.numpy(), target.numpy(), mask.numpy(), mc.COEFS)
        if n == 0:  # the reference raises on min() of an empty tensor; the contract answers NaN
            try:
                crit(pred.clone(), target.clone(), mask.clone())
                raise SystemExit(f"case {name}: the reference did not raise on a batch without a valid pixel")
            except (RuntimeError, IndexError, ValueError) as exc:
                raised = type(exc).__name__
            r = np.full(4, math.nan)
        else:
            raised = None
            loss, res = crit(pred.clone(), target.clone(), mask.clone())
            assert tuple(res.keys()) == mc.VALUES
            r = np.array([res[k] for k in mc.VALUES], np.float64)
            assert mc.same_or_both_nan(float(loss), r[0])
        rep.append(f"case {name:3s} {tuple(pred.shape)!s:18s} valid {n:7d}  kept {kept:7d}  per sample {mask.flatten(1).sum(1).tolist()}"
                   + (f"  (the reference raises {raised})" if raised else ""))
        for k, rv, fv in zip(mc.VALUES, r, f):
            if math.isfinite(fv) and math.isfinite(rv):
                e = abs(rv - fv)
                worst = max(worst, e / max(1.0, abs(fv)))
                if e > CAP * max(1.0, abs(fv)):
                    raise SystemExit(f"case {name} {k}: r = {rv!r}, f = {fv!r}: |r - f| = {e:.3e} is above the cap; the case is ill-conditioned")
                rep.append(f"    {k:12s} f = {fv:<22.15g} |r - f| = {e:.3e}")
            else:
                if not mc.same_or_both_nan(float(rv), float(fv)):
                    raise SystemExit(f"case {name} {k}: r = {rv!r} but f = {fv!r}")
                rep.append(f"    {k:12s} f = {float(fv)!r:<22s} r = {float(rv)!r}")
        R.append(r), Fv.append(f), N.append(n), K.append(kept), shapes.append(shape)
    rep.append(f"worst |r - f| / max(1, |f|) = {worst:.3e}")
    path = os.path.join(GOLD, "midas_loss.npz")
    np.savez_compressed(path, names=np.array(json.dumps(list(mc.NAMES))), shapes=np.array(shapes, np.int64), r=np.array(R), f=np.array(Fv),
                        n=np.array(N, np.int64), kept=np.array(K, np.int64))
    rep.append(f"midas_loss.npz: {os.path.getsize(path)} bytes")
    with open(os.path.join(GOLD, "REPORT_midas_loss.txt"), "w") as fh:
        fh.write("\n".join(rep) + "\n")
    print("\n".join(rep))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
