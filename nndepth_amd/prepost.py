"""Device-side pre- and post-processing: drop-ins for `preprocess_frame`
(nndepth/models/raft_stereo/scripts/inference.py:55-60), `Padder` (nndepth/data/dataloaders/utils.py:5-21) and
`EvalCriterion` (nndepth/models/raft_stereo/scripts/evaluate.py:29-83) that keep the frames and the disparity on the GPU, and
for `DepthEvalCriterion` with its dataset mean (nndepth/models/midas/scripts/evaluate.py:38-211, 300-312) on the monocular side."""
import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from ._lib import NndError, check, lib
from .ops import _dev, _mask_bytes, _p, _stream


def preprocess_frame(frame: torch.Tensor, HW: Tuple[int, int]) -> torch.Tensor:
    """frame: float (3,h,w) / (B,3,h,w), or the decoded uint8 image (h,w,3) / (B,h,w,3), on the GPU
    -> (B,3,H,W) float: bilinear resize to HW, then (x - 127.5) / 127.5."""
    if frame.device.type != "cuda":
        raise NndError("preprocess_frame: the frame must be on the HIP device (upload the decoded image, then call)")
    u8 = frame.dtype == torch.uint8
    if frame.dim() == 3:
        frame = frame.unsqueeze(0)
    frame = frame.contiguous()
    if u8:
        B, h, w, Cc = frame.shape
    else:
        _dev(frame)
        B, Cc, h, w = frame.shape
    H, W = int(HW[0]), int(HW[1])
    out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=frame.device)
    with torch.cuda.device(frame.device):
        check(lib.nnd_resize_normalize(_p(frame), int(u8), _p(out), B, Cc, h, w, H, W, 127.5, 127.5, _stream(frame.device)),
              "resize_normalize")
    return out


def replicate_pad(x: torch.Tensor, pad) -> torch.Tensor:
    """F.pad(x, (left, right, top, bottom), mode="replicate") for (B,C,H,W) fp32 on the GPU; negative entries crop."""
    d = _dev(x)
    x = x.contiguous()
    B, Cc, H, W = x.shape
    left, right, top, bottom = (int(v) for v in pad)
    out = torch.empty((B, Cc, H + top + bottom, W + left + right), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_replicate_pad(_p(x), _p(out), B, Cc, H, W, left, right, top, bottom, _stream(d)), "replicate_pad")
    return out


class Padder:
    """Pads images such that dimensions are divisible by `divis_by` (same arithmetic as the reference's Padder)."""

    def __init__(self, HW: Tuple[int, int], divis_by: int = 8):
        self.ht, self.wd = HW
        pad_ht = (((self.ht // divis_by) + 1) * divis_by - self.ht) % divis_by
        pad_wd = (((self.wd // divis_by) + 1) * divis_by - self.wd) % divis_by
        self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, 0, pad_ht]

    def pad(self, *inputs):
        assert all((x.ndim == 4) for x in inputs)
        return [replicate_pad(x, self._pad) for x in inputs]

    def unpad(self, x: torch.Tensor) -> torch.Tensor:
        assert x.ndim == 4
        return replicate_pad(x, [-self._pad[0], -self._pad[1], -self._pad[2], -self._pad[3]])


class EvalCriterion:
    """EPE and dX metrics computed on the device; returns the same dict of floats as the reference (one D2H of a few
    floats instead of the disparity maps).  Inputs of different sizes are first brought to the prediction's size the way
    the reference does it (max-pool of the negated GT, nearest resize) with PyTorch ops on the device."""

    def __init__(self, d_threshold: Optional[Dict[str, float]] = None, max_flow: int = 1000):
        self.d_threshold = d_threshold
        self.max_flow = max_flow

    def __call__(self, disp_gt: torch.Tensor, disp_pred: torch.Tensor, valid_mask: Optional[torch.Tensor] = None):
        d = _dev(disp_gt, disp_pred)
        if disp_pred.shape[-2:] != disp_gt.shape[-2:]:
            scale = disp_gt.shape[-1] // disp_pred.shape[-1]
            gt = -torch.nn.functional.max_pool2d(-disp_gt, kernel_size=scale) / scale
            gt = torch.nn.functional.interpolate(gt, size=disp_pred.shape[-2:])
        else:
            gt = disp_gt
        gt, pred = gt.contiguous(), disp_pred.contiguous()
        B, Cc, H, W = pred.shape
        keys = list(self.d_threshold.keys()) if self.d_threshold else []
        if len(keys) > 4:
            raise NndError("EvalCriterion: at most 4 thresholds per call")
        thr = (C.c_float * max(1, len(keys)))(*[float(self.d_threshold[k]) for k in keys])
        mask = None
        if valid_mask is not None:
            mask = valid_mask.to(device=d, dtype=torch.uint8).contiguous()
            if mask.numel() != B * H * W:
                raise NndError(f"EvalCriterion: valid_mask has {mask.numel()} elements, expected {B * H * W}")
        ws = torch.empty(int(lib.nnd_epe_metrics_workspace_bytes()), dtype=torch.uint8, device=d)
        out = torch.empty(2 + len(keys), dtype=torch.float32, device=d)
        with torch.cuda.device(d):
            check(lib.nnd_epe_metrics(_p(gt), _p(pred), _p(mask), B, Cc, H, W, float(self.max_flow), thr, len(keys), _p(ws), _p(out),
                                      _stream(d)), "epe_metrics")
        vals = out.cpu().tolist()
        metrics = {"epe": vals[0]}
        for i, k in enumerate(keys):
            metrics[k] = vals[2 + i]
        return metrics


DEPTH_METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "delta1", "delta2", "delta3", "ssi_mae", "ssi_rmse")
_DEPTH_EVAL_WS: Dict[str, torch.Tensor] = {}  # per device, grown to the largest batch seen


def _depth_eval_workspace(device: torch.device, B: int) -> torch.Tensor:
    n = int(lib.nnd_depth_eval_workspace_bytes(B))
    if n <= 0:
        check(n, "depth_eval_workspace_bytes")
    ws = _DEPTH_EVAL_WS.get(str(device))
    if ws is None or ws.numel() * 8 < n:
        ws = _DEPTH_EVAL_WS[str(device)] = torch.empty((n + 7) // 8, dtype=torch.float64, device=device)
    return ws


class DepthEvalCriterion:
    """The monocular evaluation criterion computed on the device: scale / shift alignment per sample, abs_rel, sq_rel, rmse,
    rmse_log, delta1..3 and the two scale-and-shift-invariant errors, in float64 (nnd_depth_eval states every step).  Returns
    the reference's dict of floats, same keys in the same order; the maps stay on the GPU and ten doubles come back."""

    def __init__(self, max_depth: float = 80.0):
        self.max_depth = max_depth

    def metrics_tensor(self, depth_pred: torch.Tensor, depth_gt: torch.Tensor, valid_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(10,) float64 on the device: the nine metrics in the dict's order, then the number of pixels they were taken over.
        No host synchronisation, allocations through PyTorch only: it can be captured into a HIP graph (call once before the
        capture, so that the device's workspace exists)."""
        what = "DepthEvalCriterion"
        if not (torch.is_tensor(depth_pred) and torch.is_tensor(depth_gt)):
            raise NndError(f"{what}: depth_pred and depth_gt are tensors on the HIP device")
        if valid_mask is not None and valid_mask.dtype not in (torch.bool, torch.uint8):
            raise NndError(f"{what}: valid_mask is torch.bool or torch.uint8; got {valid_mask.dtype}")
        if depth_pred.dim() != 4 or depth_pred.shape[1] != 1:
            raise NndError(f"{what}: depth maps are (B,1,H,W); got depth_pred {tuple(depth_pred.shape)}")
        if depth_gt.shape != depth_pred.shape or (valid_mask is not None and valid_mask.shape != depth_pred.shape):
            raise NndError(f"{what}: depth_pred {tuple(depth_pred.shape)}, depth_gt {tuple(depth_gt.shape)}"
                           + (f", valid_mask {tuple(valid_mask.shape)}" if valid_mask is not None else "") + " must have one shape")
        d = _dev(depth_pred, depth_gt)
        pred, gt = depth_pred.contiguous(), depth_gt.contiguous()
        mask = _mask_bytes(valid_mask, pred, what)
        B, _, H, W = pred.shape
        ws = _depth_eval_workspace(d, B)
        out = torch.empty(10, dtype=torch.float64, device=d)
        with torch.cuda.device(d):
            check(lib.nnd_depth_eval(_p(pred), _p(gt), _p(mask), B, H, W, float(self.max_depth), _p(ws), ws.numel() * 8, _p(out),
                                     _stream(d)), "depth_eval")
        return out

    def __call__(self, depth_pred: torch.Tensor, depth_gt: torch.Tensor, valid_mask: Optional[torch.Tensor] = None) -> Dict[str, float]:
        vals = self.metrics_tensor(depth_pred, depth_gt, valid_mask).cpu().tolist()
        return dict(zip(DEPTH_METRICS, vals[:9]))


class DepthEvalMean:
    """The evaluation loop's mean over batches (evaluate.py:300-312) kept on the device: `update` only enqueues the batch's
    criterion and adds its finite metrics to running sums; `result` copies the sums once.  A metric that was never finite comes
    back as the reference's inf (0.0 for the deltas)."""

    def __init__(self, max_depth: float = 80.0):
        self.criterion = DepthEvalCriterion(max_depth)
        self._acc: Optional[torch.Tensor] = None  # (2, 9) float64: sums, counts

    def update(self, depth_pred: torch.Tensor, depth_gt: torch.Tensor, valid_mask: Optional[torch.Tensor] = None) -> None:
        m = self.criterion.metrics_tensor(depth_pred, depth_gt, valid_mask)
        if self._acc is None:
            self._acc = torch.zeros((2, 9), dtype=torch.float64, device=m.device)
        elif self._acc.device != m.device:
            raise NndError(f"DepthEvalMean: batches on {self._acc.device} and on {m.device}")
        with torch.cuda.device(m.device):
            check(lib.nnd_depth_eval_accumulate(_p(m), _p(self._acc[0]), _p(self._acc[1]), _stream(m.device)), "depth_eval_accumulate")

    def result(self) -> Dict[str, float]:
        sums, counts = self._acc.cpu().tolist() if self._acc is not None else ([0.0] * 9, [0.0] * 9)
        return {k: (s / c if c > 0 else (0.0 if k.startswith("delta") else float("inf")))
                for k, s, c in zip(DEPTH_METRICS, sums, counts)}
