"""Device-side pre- and post-processing: drop-ins for `preprocess_frame`
(nndepth/models/raft_stereo/scripts/inference.py:55-60), `Padder` (nndepth/data/dataloaders/utils.py:5-21) and
`EvalCriterion` (nndepth/models/raft_stereo/scripts/evaluate.py:29-83) that keep the frames and the disparity on the GPU, for
the stereo scripts' criterion, sequence loss and dataset mean over every output of a forward (`StereoEvalCriterion`,
`StereoEvalMean`: evaluate.py:48-83, 141-169, loss.py:15-52), and for `DepthEvalCriterion` with its dataset mean
(nndepth/models/midas/scripts/evaluate.py:38-211, 300-312) and the value of `MiDasLoss` with the validation loop's mean
(nndepth/models/midas/loss.py:62-221, trainer.py:321-352) on the monocular side."""
import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from ._lib import NND_STEREO_EVAL_MAX_OUTPUTS, NND_STEREO_EVAL_MAX_THRESHOLDS, NndError, StereoEvalDesc, check, lib
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


def downsample_gt(disp_gt: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """The ground truth at a coarse output's size, as the reference's criterion and losses make it (evaluate.py:63-66):
    scale = W // size[1]; F.interpolate(-F.max_pool2d(-disp_gt, scale) / scale, size=size), bit for bit, in one kernel."""
    d = _dev(disp_gt)
    if disp_gt.dim() != 4:
        raise NndError(f"downsample_gt: the ground truth is (B,C,H,W); got {tuple(disp_gt.shape)}")
    gt = disp_gt.contiguous()
    B, Cc, H, W = gt.shape
    h, w = int(size[0]), int(size[1])
    out = torch.empty((B, Cc, h, w), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_min_pool_nearest(_p(gt), _p(out), B, Cc, H, W, h, w, _stream(d)), "min_pool_nearest")
    return out


class EvalCriterion:
    """EPE and dX metrics computed on the device; returns the same dict of floats as the reference (one D2H of a few doubles
    instead of the disparity maps).  The single-output front of `StereoEvalCriterion`: a coarse prediction is scored against the
    ground truth brought to its size the reference's way, a 1-channel ground truth serves both channels of a 2-channel map."""

    def __init__(self, d_threshold: Optional[Dict[str, float]] = None, max_flow: int = 1000):
        self.d_threshold = d_threshold
        self.max_flow = max_flow

    def __call__(self, disp_gt: torch.Tensor, disp_pred: torch.Tensor, valid_mask: Optional[torch.Tensor] = None):
        keys = list(self.d_threshold) if self.d_threshold else []
        # the caller's keys stay here (any name, "count" too); the columns get positional names
        crit = StereoEvalCriterion({f"above{i}": self.d_threshold[k] for i, k in enumerate(keys)}, None, self.max_flow)
        d = _dev(disp_gt, disp_pred)
        mask = None
        if valid_mask is not None:  # any dtype, shape and device with B*h*w elements
            B, _, h, w = disp_pred.shape
            mask = valid_mask.to(device=d, dtype=torch.uint8).contiguous()
            if mask.numel() != B * h * w:
                raise NndError(f"EvalCriterion: valid_mask has {mask.numel()} elements, expected {B * h * w}")
            mask = mask.view(B, h, w)
        out, _ = crit._run(disp_gt, disp_pred, mask)
        vals = out.cpu().numpy().astype(np.float32).tolist()  # the reference's results are fp32
        metrics = {"epe": vals[0]}
        for i, k in enumerate(keys):
            metrics[k] = vals[3 + i]
        return metrics


_STEREO_EVAL_WS: Dict[str, torch.Tensor] = {}  # per device, grown to the largest number of outputs seen


def _cached_workspace(cache: Dict[str, torch.Tensor], device: torch.device, nbytes: int) -> torch.Tensor:
    """`cache`'s float64 buffer of `device`, grown to the `nbytes` a *_workspace_bytes of the library answered (negative: its refusal,
    which nnd_last_error names)."""
    nbytes = int(nbytes)
    if nbytes <= 0:
        check(nbytes, "workspace_bytes")
    ws = cache.get(str(device))
    if ws is None or ws.numel() * 8 < nbytes:
        ws = cache[str(device)] = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
    return ws


def _threshold_dict(d: Optional[Dict[str, float]], what: str) -> Dict[str, float]:
    d = dict(d) if d else {}
    if len(d) > NND_STEREO_EVAL_MAX_THRESHOLDS:
        raise NndError(f"StereoEvalCriterion: at most {NND_STEREO_EVAL_MAX_THRESHOLDS} {what} thresholds; got {len(d)}")
    return {str(k): float(v) for k, v in d.items()}


StereoOutputs = Union[torch.Tensor, Sequence[torch.Tensor], Sequence[Dict[str, torch.Tensor]]]


class StereoEvalCriterion:
    """The stereo scripts' criterion for every output of a forward in one call on the device (nnd_stereo_eval states every step):
    per output the EPE, the number of valid pixels, the sequence loss's L1 term, the fraction of valid pixels with epe > each
    `d_threshold` (evaluate.py:82) and with epe < each `below` (loss.py:47-50), in float64; and the value of the sequence loss,
    sum_i gamma^(N-1-i) l1_i.  A coarse output is scored against the ground truth brought to its size the reference's way; a
    1-channel ground truth serves every channel of an output (the reference's broadcasting in cre_stereo/scripts/evaluate.py)."""

    def __init__(self, d_threshold: Optional[Dict[str, float]] = None, below: Optional[Dict[str, float]] = None, max_flow: float = 1000,
                 gamma: float = 0.8):
        self.d_threshold = _threshold_dict(d_threshold, "d_threshold")
        self.below = _threshold_dict(below, "below")
        self.max_flow = max_flow
        self.gamma = gamma
        self.columns: Tuple[str, ...] = ("epe", "count", "l1") + tuple(self.d_threshold) + tuple(self.below)
        if len(set(self.columns)) != len(self.columns):
            raise NndError(f"StereoEvalCriterion: the column names {self.columns} are not distinct")

    @staticmethod
    def _maps(outputs: StereoOutputs) -> List[torch.Tensor]:
        what = "StereoEvalCriterion"
        if torch.is_tensor(outputs):
            outputs = [outputs]
        maps = [o["up_disp"] if isinstance(o, dict) else o for o in outputs]
        if not 0 < len(maps) <= NND_STEREO_EVAL_MAX_OUTPUTS:
            raise NndError(f"{what}: 1 .. {NND_STEREO_EVAL_MAX_OUTPUTS} outputs per call; got {len(maps)}")
        for i, t in enumerate(maps):
            if not torch.is_tensor(t) or t.dim() != 4:
                raise NndError(f"{what}: output {i} is not a (B,C,h,w) tensor")
        return maps

    def describe(self, disp_gt: torch.Tensor, outputs: StereoOutputs, valid_mask: Optional[torch.Tensor] = None):
        """(the call's nnd_stereo_eval_desc, its device, the tensors the descriptor points into: keep them until the call is
        enqueued).  Every refusal of the Python seam happens here."""
        what = "StereoEvalCriterion"
        maps = self._maps(outputs)
        if not torch.is_tensor(disp_gt) or disp_gt.dim() != 4:
            raise NndError(f"{what}: disp_gt is a (B,C,H,W) tensor on the HIP device")
        B, Cg, H, W = disp_gt.shape
        for t in [disp_gt] + maps:
            if t.dtype != torch.float32:
                raise NndError(f"{what}: the maps are fp32; got {t.dtype}")
        for i, t in enumerate(maps):
            if t.shape[0] != B:
                raise NndError(f"{what}: output {i} has batch size {t.shape[0]}, the ground truth {B}")
            if Cg != 1 and Cg != t.shape[1]:
                raise NndError(f"{what}: output {i} has {t.shape[1]} channels, the ground truth {Cg} (equal, or 1 to broadcast)")
        mask = None
        if valid_mask is not None:
            if valid_mask.dtype not in (torch.bool, torch.uint8):
                raise NndError(f"{what}: valid_mask is torch.bool or torch.uint8; got {valid_mask.dtype}")
            ms = tuple(valid_mask.shape)
            if not ((len(ms) == 4 and ms[1] == 1) or len(ms) == 3) or ms[0] != B:
                raise NndError(f"{what}: valid_mask is (B,1,h,w) or (B,h,w) with B = {B}; got {ms}")
            for i, t in enumerate(maps):
                if tuple(t.shape[-2:]) != ms[-2:]:
                    raise NndError(f"{what}: valid_mask is {ms[-2]}x{ms[-1]} but output {i} is {t.shape[-2]}x{t.shape[-1]}: a mask needs "
                                   "every output of the call at its size")
        d = _dev(disp_gt, *maps)  # the shapes are judged first: those refusals read the same wherever the tensors live
        if valid_mask is not None:
            if valid_mask.device != d:
                raise NndError(f"{what}: valid_mask is on {valid_mask.device}, the maps on {d} (no CPU fallback exists)")
            mask = valid_mask.contiguous()
            mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        gt = disp_gt.contiguous()
        maps = [t if (t.stride(3) == 1 or t.shape[3] == 1) else t.contiguous() for t in maps]  # kept alive across the call
        desc = StereoEvalDesc()
        desc.gt, desc.B, desc.Cg, desc.H, desc.W = gt.data_ptr(), B, Cg, H, W
        if mask is not None:
            desc.mask, desc.mask_h, desc.mask_w = mask.data_ptr(), mask.shape[-2], mask.shape[-1]
        desc.gamma, desc.max_flow = float(self.gamma), float(self.max_flow)
        desc.n_above, desc.n_below = len(self.d_threshold), len(self.below)
        for k, v in enumerate(self.d_threshold.values()):
            desc.above[k] = v
        for k, v in enumerate(self.below.values()):
            desc.below[k] = v
        desc.num_outputs = len(maps)
        for i, t in enumerate(maps):
            o = desc.outputs[i]
            o.data, o.C, o.h, o.w = t.data_ptr(), t.shape[1], t.shape[2], t.shape[3]
            o.stride_b, o.stride_c, o.stride_row = t.stride(0), t.stride(1), t.stride(2)
        return desc, d, (gt, maps, mask)

    def _run(self, disp_gt: torch.Tensor, outputs: StereoOutputs, valid_mask: Optional[torch.Tensor]) -> Tuple[torch.Tensor, int]:
        """The N*K + 1 doubles of nnd_stereo_eval on the device, and N."""
        desc, d, keep = self.describe(disp_gt, outputs, valid_mask)
        n = desc.num_outputs
        ws = _cached_workspace(_STEREO_EVAL_WS, d, lib.nnd_stereo_eval_workspace_bytes(n))
        out = torch.empty(n * len(self.columns) + 1, dtype=torch.float64, device=d)
        with torch.cuda.device(d):
            check(lib.nnd_stereo_eval(C.byref(desc), _p(ws), ws.numel() * 8, _p(out), _stream(d)), "stereo_eval")
        del keep
        return out, n

    def metrics_tensor(self, disp_gt: torch.Tensor, outputs: StereoOutputs,
                       valid_mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """((N,K) float64 in the order of `columns`, () float64: the sequence loss), both on the device.  `outputs`: one tensor, a
        list of tensors, or the list of {"up_disp": t} dicts a model's forward() returns; slices of a stacked tensor and cropped
        views are read where they lie.  No host synchronisation: 1 + (number of distinct output sizes) launches."""
        out, n = self._run(disp_gt, outputs, valid_mask)
        return out[:-1].view(n, len(self.columns)), out[-1]

    def __call__(self, disp_gt: torch.Tensor, outputs: StereoOutputs, valid_mask: Optional[torch.Tensor] = None) -> List[Dict[str, float]]:
        """One dict of floats per output, keys = `columns`; one device-to-host copy."""
        out, n = self._run(disp_gt, outputs, valid_mask)
        vals = out.cpu().tolist()
        K = len(self.columns)
        return [dict(zip(self.columns, vals[i * K:(i + 1) * K])) for i in range(n)]


class StereoEvalMean:
    """The stereo evaluation loop's mean over the dataset (evaluate.py:141-169) kept on the device: `update` enqueues the pair's
    criterion and adds its doubles to running sums; `result` / `curve` copy the sums once and divide by the number of updates,
    which is np.mean of the per-pair values: a NaN (a pair without a valid pixel) propagates, as it does in the reference."""

    def __init__(self, d_threshold: Optional[Dict[str, float]] = None, below: Optional[Dict[str, float]] = None, max_flow: float = 1000,
                 gamma: float = 0.8):
        self.criterion = StereoEvalCriterion(d_threshold, below, max_flow, gamma)
        self._sums: Optional[torch.Tensor] = None  # (N*K + 1,) float64
        self._sizes: Optional[List[Tuple[int, ...]]] = None
        self._updates = 0

    def update(self, disp_gt: torch.Tensor, outputs: StereoOutputs, valid_mask: Optional[torch.Tensor] = None) -> None:
        sizes = [tuple(t.shape[1:]) for t in self.criterion._maps(outputs)]
        if self._sizes is not None and sizes != self._sizes:
            raise NndError(f"StereoEvalMean: this update has {len(sizes)} outputs of sizes {sizes}, the first had {len(self._sizes)} of "
                           f"sizes {self._sizes}")
        m, _ = self.criterion._run(disp_gt, outputs, valid_mask)
        if self._sums is None:
            self._sums, self._sizes = torch.zeros(m.numel(), dtype=torch.float64, device=m.device), sizes
        elif self._sums.device != m.device:
            raise NndError(f"StereoEvalMean: pairs on {self._sums.device} and on {m.device}")
        with torch.cuda.device(m.device):
            check(lib.nnd_stereo_eval_accumulate(_p(m), m.numel(), _p(self._sums), _stream(m.device)), "stereo_eval_accumulate")
        self._updates += 1

    def curve(self) -> List[Dict[str, float]]:
        """The dataset mean of every column, per output index."""
        if self._sums is None:
            return []
        vals = (self._sums.cpu().numpy() / self._updates).tolist()
        cols = self.criterion.columns
        return [dict(zip(cols, vals[i * len(cols):(i + 1) * len(cols)])) for i in range(len(self._sizes))]

    def result(self) -> Dict[str, float]:
        """The reference script's table for the last output: epe and the threshold metrics, each the mean of the per-pair values."""
        keys = ("epe",) + self.criterion.columns[3:]
        if self._sums is None:
            return {k: float("nan") for k in keys}  # np.mean of an empty list
        last = self.curve()[-1]
        return {k: last[k] for k in keys}


DEPTH_METRICS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "delta1", "delta2", "delta3", "ssi_mae", "ssi_rmse")
_DEPTH_EVAL_WS: Dict[str, torch.Tensor] = {}  # per device, grown to the largest batch seen


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
        ws = _cached_workspace(_DEPTH_EVAL_WS, d, lib.nnd_depth_eval_workspace_bytes(B))
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


MIDAS_LOSS_METRICS = ("loss", "trimmed_mae", "gradient_reg", "abs_dev")
_MIDAS_LOSS_WS: Dict[str, torch.Tensor] = {}  # per device, grown to the largest batch of maps seen


class MiDasLoss:
    """The value of the reference's MiDasLoss (nndepth/models/midas/loss.py:168-221) computed on the device: the trimmed
    scale-and-shift-invariant error, the four-level gradient term and the absolute deviation, in float64 (nnd_midas_loss states
    every step and the three places where it departs from the reference).  A value only: there is no backward, so a prediction
    that asks for a gradient is refused.  The maps stay on the GPU and are never modified; six doubles come back."""

    def __init__(self, trimmed_loss_coef: float = 1.0, gradient_reg_coef: float = 0.1):
        self.trimmed_loss_coef = trimmed_loss_coef
        self.gradient_reg_coef = gradient_reg_coef

    def values_tensor(self, pred: torch.Tensor, target: torch.Tensor, valid_mask: torch.Tensor) -> torch.Tensor:
        """(6,) float64 on the device: loss, trimmed_mae, gradient_reg, abs_dev, the number of valid pixels, the number of pixels
        the trimmed error was taken over.  No host synchronisation, allocations through PyTorch only: it can be captured into a HIP
        graph (call once before the capture, so that the device's workspace exists)."""
        what = "MiDasLoss"
        if not (torch.is_tensor(pred) and torch.is_tensor(target)):
            raise NndError(f"{what}: pred and target are tensors on the HIP device")
        if valid_mask is None:
            raise NndError(f"{what}: valid_mask is required (torch.bool or torch.uint8, the shape of pred)")
        if not torch.is_tensor(valid_mask) or valid_mask.dtype not in (torch.bool, torch.uint8):
            raise NndError(f"{what}: valid_mask is torch.bool or torch.uint8; got {getattr(valid_mask, 'dtype', type(valid_mask))}")
        if pred.dtype != torch.float32 or target.dtype != torch.float32:
            raise NndError(f"{what}: pred and target are fp32; got {pred.dtype} and {target.dtype}")
        if pred.dim() != 4 or pred.shape[1] != 1:
            raise NndError(f"{what}: maps are (B,1,H,W); got pred {tuple(pred.shape)}")
        if target.shape != pred.shape or valid_mask.shape != pred.shape:
            raise NndError(f"{what}: pred {tuple(pred.shape)}, target {tuple(target.shape)}, valid_mask {tuple(valid_mask.shape)} "
                           "must have one shape")
        B, _, H, W = pred.shape
        if H < 16 or W < 16:
            raise NndError(f"{what}: maps of {H}x{W}: H and W must be at least 16 (four levels of 2x2 pooling; the reference raises "
                           "below that too)")
        d = _dev(pred, target)
        if pred.requires_grad and torch.is_grad_enabled():
            raise NndError(f"{what}: pred requires grad, but this is the loss's value and has no backward (call it under "
                           "torch.no_grad(), as the validation loop does, or detach the prediction)")
        p = pred.detach()
        if p.stride(3) != 1:
            p = p.contiguous()  # kept alive across the call
        tgt = target.detach().contiguous()
        mask = _mask_bytes(valid_mask, tgt, what)
        ws = _cached_workspace(_MIDAS_LOSS_WS, d, lib.nnd_midas_loss_workspace_bytes(B, H, W))
        out = torch.empty(6, dtype=torch.float64, device=d)
        with torch.cuda.device(d):
            check(lib.nnd_midas_loss(_p(p), _p(tgt), _p(mask), B, H, W, p.stride(0), p.stride(2), float(self.trimmed_loss_coef),
                                     float(self.gradient_reg_coef), _p(ws), ws.numel() * 8, _p(out), _stream(d)), "midas_loss")
        return out

    def __call__(self, pred: torch.Tensor, target: torch.Tensor, valid_mask: torch.Tensor) -> Tuple[torch.Tensor, Dict[str, float]]:
        """(loss, metrics) as the reference returns them: the loss a 0-dim float64 device tensor, the metrics Python floats from one
        copy of the six doubles."""
        values = self.values_tensor(pred, target, valid_mask)
        return values[0], dict(zip(MIDAS_LOSS_METRICS, values.cpu().tolist()[:4]))


class MiDasLossMean:
    """The validation loop's mean over batches (midas/trainer.py:341-350) kept on the device: `update` only enqueues the batch's
    loss and adds its doubles to running sums; `result` copies the sums once and divides by the number of updates, which is np.mean
    of the per-batch values: a NaN propagates, as it does in the reference."""

    def __init__(self, trimmed_loss_coef: float = 1.0, gradient_reg_coef: float = 0.1):
        self.criterion = MiDasLoss(trimmed_loss_coef, gradient_reg_coef)
        self._acc: Optional[torch.Tensor] = None  # (7,) float64: the six sums, the number of updates

    def update(self, pred: torch.Tensor, target: torch.Tensor, valid_mask: torch.Tensor) -> None:
        v = self.criterion.values_tensor(pred, target, valid_mask)
        if self._acc is None:
            self._acc = torch.zeros(7, dtype=torch.float64, device=v.device)
        elif self._acc.device != v.device:
            raise NndError(f"MiDasLossMean: batches on {self._acc.device} and on {v.device}")
        with torch.cuda.device(v.device):
            check(lib.nnd_midas_loss_accumulate(_p(v), _p(self._acc), _p(self._acc[6:]), _stream(v.device)), "midas_loss_accumulate")

    def result(self) -> Dict[str, float]:
        keys = [f"val/{k}" for k in MIDAS_LOSS_METRICS]
        if self._acc is None:
            return {k: float("nan") for k in keys}  # np.mean of an empty list
        acc = self._acc.cpu().tolist()
        return {k: s / acc[6] for k, s in zip(keys, acc[:4])}
