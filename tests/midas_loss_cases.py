"""Shared by tests/test_midas_loss_cpu.py, tests/test_gpu_midas_loss.py and scripts/make_golden_midas_loss.py (not a test module):
the inputs of the MiDasLoss cases, each a pure function of its name through nndepth_amd.weightgen (so tests/golden/midas_loss.npz
stores no input array), and the tests' float64 statement of the loss's contract (include/nndepth_amd.h: nnd_midas_loss) in
torch.float64.  The fixture script has its own statement in numpy; the CPU test holds the two against each other."""
import math
from typing import Tuple

import numpy as np
import torch
import torch.nn.functional as F

from nndepth_amd import weightgen

VALUES = ("loss", "trimmed_mae", "gradient_reg", "abs_dev")
COEFS = (1.0, 0.1)  # the reference's defaults: trimmed_loss_coef, gradient_reg_coef
#        name  (B, H, W)       target range
CASES = (("A", (2, 16, 16), (0.5, 60.0)),    # the minimum size: levels 16 / 8 / 4 / 2
         ("B", (2, 17, 19), (0.5, 60.0)),    # floor pooling drops a row and a column; sample 1: exactly 6 valid pixels (trim == 0)
         ("C", (3, 33, 47), (0.5, 60.0)),    # odd at every level (47 -> 23 -> 11 -> 5); sample 2 fully invalid; inverse depth
         ("D", (2, 40, 72), (0.5, 60.0)),    # several blocks per sample and level
         ("T", (2, 16, 20), (0.5, 60.0)),    # values rounded to halves: ties in both medians; sample 1: every e twice, k_b odd
         ("K", (1, 16, 16), (0.5, 60.0)),    # constant prediction: scale 0 -> 1
         ("Z", (2, 16, 16), (0.5, 60.0)),    # the batch's minimum target beside invalid pixels: the first-maximum rule
         ("N9", (1, 16, 16), (0.5, 60.0)),   # 9 valid pixels: int(9 * 0.1) == 0, nothing is kept
         ("N10", (1, 16, 16), (0.5, 60.0)),  # 10 valid pixels: one is trimmed
         ("E", (2, 16, 16), (0.5, 60.0)),    # no valid pixel at all
         ("H", (1, 384, 384), (0.05, 100.0)))  # the model's own size
NAMES = tuple(c[0] for c in CASES)
Z_MIN = ((0, 4, 6), (1, 9, 11))  # case Z: (sample, y, x) of the two pixels that hold the batch's minimum target


def _u(tag: str, shape) -> np.ndarray:
    return weightgen.uniform01(tag, int(np.prod(shape))).reshape(shape)


def make_case(name: str) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pred, target, valid_mask): (B,1,H,W) fp32, fp32, bool on the CPU."""
    (B, H, W), (lo, hi) = next((s, r) for n, s, r in CASES if n == name)
    shape = (B, 1, H, W)
    tag = f"midas_loss/{name}"
    t = np.exp(np.log(lo) + _u(tag + "/t", shape).astype(np.float64) * (np.log(hi) - np.log(lo))).astype(np.float32)
    noise = 2.0 * _u(tag + "/noise", shape) - 1.0
    pred = (np.float32(0.7) * t + np.float32(2.0) + np.float32(0.1) * t * noise).astype(np.float32)
    mask = np.ones(shape, bool)
    if name == "B":
        mask = _u(tag + "/mask", shape) < 0.5
        m1 = np.zeros(H * W, bool)
        m1[weightgen.sample_index(tag + "/mask1", H * W, 6)] = True
        mask[1, 0] = m1.reshape(H, W)
    elif name == "C":
        pred = (np.float32(1.0) / t + np.float32(0.01) * noise).astype(np.float32)
        mask = _u(tag + "/mask", shape) < 0.7
        mask[2] = False
    elif name in ("D", "H"):
        mask = _u(tag + "/mask", shape) < 0.7
    elif name == "T":
        t, pred = (np.round(t * 2) / 2).astype(np.float32), (np.round(pred * 2) / 2).astype(np.float32)
        # sample 1: the second half of the map repeats the first, and 5 pixels of each half are invalid: 310 valid pixels (even), every
        # e at least twice, k_b = 310 - 31 = 279 is odd, so the trim threshold falls between two equal values
        half = H * W // 2
        for x in (t, pred):
            flat = x[1, 0].reshape(-1)
            flat[half:] = flat[:half]
        m1 = np.ones(H * W, bool)
        m1[half - 5:half] = False
        m1[2 * half - 5:] = False
        mask[1, 0] = m1.reshape(H, W)
    elif name == "K":
        pred = np.full(shape, 3.0, np.float32)
    elif name == "Z":
        # sample 0: the minimum is FIRST in its 2x2 window (rows 4-5, columns 6-7) and the other three are invalid (T = 0 as well):
        # the pooled mask bit is the minimum's own, set.  sample 1: it is LAST in its window (rows 8-9, columns 10-11) behind three
        # invalid pixels: the pooled mask bit is the first invalid pixel's, cleared
        for b, y, x in Z_MIN:
            t[b, 0, y, x] = np.float32(0.25)
        mask[0, 0, 4, 7] = mask[0, 0, 5, 6] = mask[0, 0, 5, 7] = False
        mask[1, 0, 8, 10] = mask[1, 0, 8, 11] = mask[1, 0, 9, 10] = False
    elif name in ("N9", "N10"):
        m = np.zeros(H * W, bool)
        m[weightgen.sample_index(tag + "/mask", H * W, int(name[1:]))] = True
        mask = m.reshape(shape)
    elif name == "E":
        mask = np.zeros(shape, bool)
    c = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    return c(pred), c(t), c(mask)


def contract64(pred: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, coefs=COEFS) -> Tuple[np.ndarray, int, int]:
    """(the four values of the contract in torch.float64 on the CPU, the valid pixels n, the kept pixels sum_b k_b)."""
    nan = float("nan")
    p, t, m = pred.double(), target.double(), mask.bool()
    B = p.shape[0]
    n = int(m.sum())
    if n == 0:
        return np.full(4, nan), 0, 0
    tv = t[m]
    tn = (t - tv.min()) / (tv.max() - tv.min() + 1e-6)
    ssi = []
    for x in (tn, p):
        out = torch.empty_like(x)
        for b in range(B):
            nb = int(m[b].sum())
            if nb == 0:  # the median and the mean of nothing
                out[b] = nan
                continue
            v = x[b][m[b]]
            shift = torch.sort(v).values[(nb - 1) // 2]
            scale = (v - shift).abs().sum() / nb
            out[b] = (x[b] - shift) / (scale if float(scale) != 0.0 else 1.0)
        ssi.append(out)
    st, sp = ssi
    e = (sp - st).abs()
    abs_dev = e[m].sum() / n
    total, kept = torch.zeros((), dtype=torch.float64), 0
    for b in range(B):
        nb = int(m[b].sum())
        trim = int(nb * 0.1)
        if trim == 0:  # loss[:-0] is empty
            continue
        k = nb - trim
        total += torch.sort(e[b][m[b]]).values[:k].sum()
        kept += k
    trimmed = float(total) / kept if kept else nan
    T, P, M = torch.where(m, tn, torch.zeros_like(tn)), sp, m
    g = torch.zeros((), dtype=torch.float64)
    for _ in range(4):
        R = P - T
        term = (R[:, :, :-1, :-1] - R[:, :, :-1, 1:]).abs() + (R[:, :, :-1, :-1] - R[:, :, 1:, :-1]).abs()
        g += term[M[:, :, 1:, 1:]].sum()
        T, idx = F.max_pool2d(T, 2, stride=2, return_indices=True)
        M = M.flatten(2).gather(2, idx.flatten(2)).view_as(idx)
        P = F.avg_pool2d(P, 2, stride=2)
    grad = float(g) / n
    loss = trimmed * coefs[0] + grad * coefs[1]
    return np.array([loss, trimmed, grad, float(abs_dev)], np.float64), n, kept


def same_or_both_nan(a: float, b: float) -> bool:
    return (math.isnan(a) and math.isnan(b)) or a == b
