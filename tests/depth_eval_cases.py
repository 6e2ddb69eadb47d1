"""Shared by tests/test_depth_eval_cpu.py, tests/test_gpu_depth_eval.py and scripts/make_golden_depth_eval.py (not a test
module): the inputs of the DepthEvalCriterion cases, each a pure function of its name through nndepth_amd.weightgen (so
tests/golden/depth_eval.npz stores no input array), and the tests' float64 statement of the criterion's contract
(include/nndepth_amd.h: nnd_depth_eval) in torch.float64.  The fixture script has its own statement in numpy; the CPU test holds
the two against each other."""
import math
from typing import Optional, Tuple

import numpy as np
import torch

from nndepth_amd import weightgen

METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "delta1", "delta2", "delta3", "ssi_mae", "ssi_rmse")
MAX_DEPTH = 80.0
#        name  (B, H, W)      gt range
CASES = (("A", (2, 48, 64), (0.5, 60.0)),
         ("B", (3, 33, 47), (0.05, 100.0)),
         ("C", (2, 8, 12), (0.5, 60.0)),
         ("C2", (2, 11, 11), (0.5, 60.0)),
         ("D", (2, 32, 40), (0.5, 60.0)),
         ("G", (2, 32, 40), (0.5, 60.0)),
         ("F", (2, 16, 20), (0.5, 60.0)),
         ("H", (1, 384, 384), (0.05, 100.0)),
         ("E", (2, 16, 16), (0.5, 60.0)),
         ("R", (1, 16, 16), (0.5, 60.0)))
NAMES = tuple(c[0] for c in CASES)


def _u(tag: str, shape) -> np.ndarray:
    return weightgen.uniform01(tag, int(np.prod(shape))).reshape(shape)


def make_case(name: str) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """(depth_pred, depth_gt, valid_mask or None): (B,1,H,W) fp32, fp32, bool on the CPU."""
    (B, H, W), (lo, hi) = next((s, r) for n, s, r in CASES if n == name)
    shape = (B, 1, H, W)
    tag = f"depth_eval/{name}"
    gt = np.exp(np.log(lo) + _u(tag + "/gt", shape).astype(np.float64) * (np.log(hi) - np.log(lo))).astype(np.float32)
    noise = 2.0 * _u(tag + "/noise", shape) - 1.0
    pred = np.maximum(np.float32(0.7) * gt + np.float32(2.0) + np.float32(0.1) * gt * noise, np.float32(0.3)).astype(np.float32)
    mask = None
    if name == "B":
        mask = _u(tag + "/mask", shape) < 0.7
        mask[2] = False
    elif name == "C":
        mask = np.ones(shape, bool)
    elif name == "C2":  # exactly 100 and 101 valid pixels: the first stays unaligned, the second is aligned
        mask = np.zeros((B, H * W), bool)
        for b, n in enumerate((100, 101)):
            mask[b, weightgen.sample_index(f"{tag}/mask{b}", H * W, n)] = True
        mask = mask.reshape(shape)
    elif name == "D":  # the fit leaves negative aligned values: rmse_log is NaN, the other eight metrics are finite
        pred = (gt + np.float32(8.0) * noise).astype(np.float32)
    elif name == "G":  # inverse depth against depth: the fitted scale is negative
        pred = (np.float32(1.0) / gt + np.float32(0.01) * noise).astype(np.float32)
        mask = _u(tag + "/mask", shape) < 0.8
    elif name == "F":  # many ties, even counts; sample 1: 64 pixels (no alignment) of a constant prediction and a constant gt
        gt, pred = np.round(gt * 2) / 2, np.round(pred * 2) / 2
        gt[1], pred[1] = 5.0, 4.0
        mask = np.ones((B, H * W), bool)
        mask[1] = False
        mask[1, weightgen.sample_index(f"{tag}/mask1", H * W, 64)] = True
        mask = mask.reshape(shape)
        gt, pred = gt.astype(np.float32), pred.astype(np.float32)
    elif name == "H":
        mask = _u(tag + "/mask", shape) < 0.7
    elif name == "E":
        mask = np.zeros(shape, bool)
    elif name == "R":  # a constant prediction: the minimum-norm branch of the fit
        pred = np.full(shape, 3.0, np.float32)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    return t(pred), t(gt), (None if mask is None else t(mask))


def empty_metrics() -> np.ndarray:
    return np.array([math.inf] * 4 + [0.0] * 3 + [math.inf] * 2)


def contract64(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor], max_depth: float = MAX_DEPTH) -> Tuple[np.ndarray, int]:
    """The nine metrics of the contract in torch.float64 on the CPU, and the number of pixels in the metric mask."""
    B = pred.shape[0]
    valid = torch.ones_like(gt, dtype=torch.bool) if mask is None else mask.bool()
    p, g = pred.double(), gt.double()
    a = p.clone()
    for b in range(B):
        m = valid[b]
        n = int(m.sum())
        if n > 100:
            pv, gv = p[b][m], g[b][m]
            pm, gm = pv.sum() / n, gv.sum() / n
            spp, spg = ((pv - pm) ** 2).sum(), ((pv - pm) * (gv - gm)).sum()
            if float(spp) == 0.0:
                scale, shift = pm * gm / (pm * pm + 1.0), gm / (pm * pm + 1.0)
            else:
                scale = spg / spp
                shift = gm - scale * pm
            a[b] = p[b] * scale + shift
    lo, hi = torch.tensor(0.1, dtype=torch.float32), torch.tensor(max_depth, dtype=torch.float32)  # compared as fp32
    mm = valid & (gt > lo) & (gt < hi)
    n = int(mm.sum())
    if n == 0:
        return empty_metrics(), 0
    av, gv = a[mm], g[mm]
    d = av - gv
    out = [(d.abs() / gv).sum() / n, (d * d / gv).sum() / n, torch.sqrt((d * d).sum() / n),
           torch.sqrt(((torch.log(av) - torch.log(gv)) ** 2).sum() / n)]
    ratio = torch.maximum(av / gv, gv / av)
    out += [(ratio < 1.25 ** k).sum().double() / n for k in (1, 2, 3)]
    gn = (g - gv.min()) / (gv.max() - gv.min() + 1e-6)
    an = (a - av.min()) / (av.max() - av.min() + 1e-6)
    e1, e2 = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    for b in range(B):
        m = mm[b]
        k = int(m.sum())
        if k == 0:
            continue
        ssi = []
        for x in (an[b][m], gn[b][m]):
            shift = torch.sort(x).values[(k - 1) // 2]
            scale = (x - shift).abs().sum() / k
            ssi.append((x - shift) / (scale if float(scale) != 0.0 else 1.0))
        e1 += (ssi[0] - ssi[1]).abs().sum()
        e2 += ((ssi[0] - ssi[1]) ** 2).sum()
    out += [e1 / n, torch.sqrt(e2 / n)]
    return np.array([float(v) for v in out]), n
