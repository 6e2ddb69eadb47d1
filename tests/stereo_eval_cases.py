"""Shared by tests/test_stereo_eval_cpu.py, tests/test_gpu_stereo_eval.py and scripts/make_golden_stereo_eval.py (not a test
module): the inputs of the StereoEvalCriterion cases, each a pure function of its name through nndepth_amd.weightgen (so
tests/golden/stereo_eval.npz stores no input array), and the tests' float64 statement of the criterion's contract
(include/nndepth_amd.h: nnd_stereo_eval) in torch: the reference's fp32 steps on the CPU, then double sums.  The fixture script
has its own statement in numpy; the CPU test holds the two against each other."""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from nndepth_amd import weightgen

ABOVE = {"d1": 1.0, "d3": 3.0}
BELOW = {"0.5px": 0.5, "1px": 1.0, "3px": 3.0, "5px": 5.0}
COLUMNS = ("epe", "count", "l1") + tuple(ABOVE) + tuple(BELOW)
K = len(COLUMNS)
NCOUNTS = 1 + len(ABOVE) + len(BELOW)  # valid pixels, then the numerator of every fraction
GAMMA = 0.8
MAX_FLOW = 1000.0
GT_RANGE = 60.0  # |gt| up to about this many px
NOISE = 6.0      # |pred - g| per channel up to this: every threshold splits the pixels

#        name  ground truth        outputs (C, h, w)
CASES = (("A", (2, 1, 37, 53), ((1, 37, 53),)),
         ("B", (3, 1, 33, 47), ((1, 33, 47),)),
         ("T", (1, 1, 16, 20), ((1, 16, 20),)),
         ("C", (2, 2, 37, 53), ((2, 37, 53),)),
         ("D", (2, 1, 37, 53), ((2, 37, 53),)),
         ("M", (2, 1, 24, 40), ((1, 24, 40),)),
         ("E", (2, 1, 16, 16), ((1, 16, 16),)),
         ("G2", (2, 1, 75, 124), ((1, 37, 62),)),
         ("G3", (2, 1, 75, 125), ((1, 24, 41),)),
         ("G4", (1, 1, 76, 130), ((1, 25, 42),)),
         ("S", (2, 1, 72, 124), ((2, 18, 31), (2, 18, 31), (2, 36, 62), (2, 72, 124), (2, 72, 124))),
         ("R", (1, 1, 40, 56), ((1, 40, 56),) * 8),
         ("V", (2, 1, 37, 53), ((1, 37, 53),)))
NAMES = tuple(c[0] for c in CASES)
T_DELTAS = (0.5, 1.0, 3.0, 0.25, 6.0)  # case T: pred - gt of pixel i is T_DELTAS[i % 5], exactly


class Case(NamedTuple):
    gt: torch.Tensor                    # (B,Cg,H,W) fp32
    outputs: List[torch.Tensor]         # (B,C,h,w) fp32 each; views where the case says so
    mask: Optional[torch.Tensor]        # (B,1,h,w) bool or None
    max_flow: float


def _u(tag: str, shape) -> np.ndarray:
    return weightgen.uniform01(tag, int(np.prod(shape))).reshape(shape)


def gt_at(gt: torch.Tensor, size) -> torch.Tensor:
    """The ground truth at an output's size: the reference's three lines (evaluate.py:63-66, loss.py:23-26)."""
    if tuple(gt.shape[-2:]) == tuple(size):
        return gt
    scale = gt.shape[-1] // size[-1]
    g = -F.max_pool2d(-gt, kernel_size=scale) / scale
    return F.interpolate(g, size=tuple(size))


def pooled_size(gt_shape, size) -> Tuple[int, int]:
    s = gt_shape[-1] // size[-1]
    return gt_shape[-2] // s, gt_shape[-1] // s


def make_case(name: str) -> Case:
    gshape, outs = next((g, o) for n, g, o in CASES if n == name)
    tag = f"stereo_eval/{name}"
    B = gshape[0]
    gt = ((2.0 * _u(tag + "/gt", gshape) - 1.0) * np.float32(GT_RANGE)).astype(np.float32)
    if name == "T":
        gt = (np.round(gt * 4) / 4).astype(np.float32)  # multiples of 0.25: gt + delta and (gt + delta) - gt are exact
    gt = torch.from_numpy(np.ascontiguousarray(gt))
    outputs = []
    for i, (Cc, h, w) in enumerate(outs):
        g = gt_at(gt, (h, w)).expand(B, Cc, h, w) if gshape[1] == 1 else gt_at(gt, (h, w))
        noise = torch.from_numpy((2.0 * _u(f"{tag}/noise{i}", (B, Cc, h, w)) - 1.0) * np.float32(NOISE * (0.5 + 0.5 / (i + 1))))
        outputs.append((g + noise).float().contiguous())
    mask, max_flow = None, MAX_FLOW
    mshape = (B, 1) + tuple(outs[0][1:])
    if name == "B":
        mask = _u(tag + "/mask", mshape) < 0.7
        mask[2] = False
    elif name == "T":
        d = np.array(T_DELTAS, np.float32)[np.arange(16 * 20) % 5].reshape(gshape)
        outputs = [gt + torch.from_numpy(d)]
    elif name == "M":
        max_flow = 40.0
    elif name == "E":
        mask = np.zeros(mshape, bool)
    elif name == "R":  # up[i] views of one stacked tensor, as a loop that writes its maps into one buffer returns them
        mask = _u(tag + "/mask", mshape) < 0.7
        up = torch.stack(outputs)
        outputs = [up[i] for i in range(len(outs))]
    elif name == "V":  # a cropped view of a larger map: what Padder.unpad would have copied out
        big = torch.from_numpy(_u(tag + "/big", (2, 1, 44, 60)) * np.float32(100.0)).float()
        big[..., 3:40, 2:55] = outputs[0]
        outputs = [big[..., 3:40, 2:55]]
    return Case(gt, outputs, None if mask is None else torch.from_numpy(mask), max_flow)


def _sqrtf(x: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp32 square root (sqrtf): torch's own CPU sqrt may be an ulp off it (vector math library), and the
    square root in double, rounded once more, is exact for fp32 arguments."""
    return x.double().sqrt().float()


def contract64(case: Case, above: Dict[str, float] = ABOVE, below: Dict[str, float] = BELOW,
               gamma: float = GAMMA) -> Tuple[np.ndarray, float, np.ndarray]:
    """((N,K) float64 metrics, the sequence loss, (N,NCOUNTS) int64: valid pixels and the numerator of every fraction)."""
    rows, counts, loss = [], [], 0.0
    N = len(case.outputs)
    for i, p in enumerate(case.outputs):
        g = gt_at(case.gt, p.shape[-2:])
        epe = _sqrtf(torch.sum((p - g) ** 2, dim=1))
        valid = _sqrtf(torch.sum(g ** 2, dim=1, keepdim=True)) < case.max_flow
        if case.mask is not None:
            valid = valid & case.mask
        e = epe.reshape(-1)[valid.reshape(-1)]
        n = int(e.numel())
        l1 = float((valid * (p - g).abs()).double().sum()) / p.numel()
        cnt = [n] + [int((e > torch.tensor(t, dtype=torch.float32)).sum()) for t in above.values()] \
            + [int((e < torch.tensor(t, dtype=torch.float32)).sum()) for t in below.values()]
        nan = float("nan")
        rows.append([float(e.double().sum()) / n if n else nan, float(n), l1] + [c / n if n else nan for c in cnt[1:]])
        counts.append(cnt)
        loss += gamma ** (N - 1 - i) * l1
    return np.array(rows, np.float64), loss, np.array(counts, np.int64)
