"""Stereo geometry on the device (csrc/geometry.hip): what a caller does with a disparity map next, without a `.cpu()`.

The reference stores `Disparity.baseline` (nndepth/scene/disparity.py:79-108) and `Camera.intrinsic` (camera.py:5-8) and never
consumes them; its `Disparity.occlusion` is only ever filled from ground truth (kitti_stereo_2015.py:188-194, 1 = no valid
disparity); its one conversion is TartanAir's `disparity = -BASELINE * FX / (depth + 1e-8)` (tartanair_dataset.py:30,239-241).
Here:

    disparity_to_depth / depth_to_disparity    (Disparity.to_depth, Depth.to_disparity of scene.py)
    depth_to_points / points_compact           (Depth.to_points_map, Depth.points_tensor, Depth.to_points)
    lr_consistency, both_views, occlusion      a left-right check of a PREDICTED map -> an occlusion mask, 1 = occluded
    connected_regions, speckle_mask, speckle_filter    (csrc/speckle.hip; Disparity.remove_speckles, Depth.remove_speckles)
    warp_disparity, occlusion_from_warp, fill_holes    (csrc/warp.hip; Disparity.to_other_view / warp_occlusion / fill_holes,
                                                        Depth.fill_holes): the other view and an occlusion mask from ONE map
    median_filter, range_weights                       (csrc/median.hip; Disparity.median_filter, Depth.median_filter): a masked
                                                        k x k median, or a weighted median guided by a picture
    synthesize_view, photometric_error, photometric_score    (csrc/photometric.hip; Disparity.synthesize,
                                                        Disparity.photometric_error): the other PICTURE seen from this view, and the
                                                        L1 + SSIM error of that reconstruction with its per-sample sums

Maps are (B,1,H,W) fp32 on the HIP device; a batch stride is read where it lies (a channel slice of CREStereo's 2-channel
output, half of a stacked batch).  Masks are torch.bool or torch.uint8, (B,1,H,W) or (B,H,W).  Camera values come from
`Camera.intrinsic`, (3,3) or (B,3,3): fx [0,0], fy [1,1], cx [0,2], cy [1,2]; the kernels read them from a small device array
(a host tensor is copied once per Camera and device, and no call synchronises on it).  Nothing falls back to PyTorch: a CPU map
is refused.  No function here synchronises with the host except `Depth.to_points`, which says so."""
from typing import Callable, Optional, Tuple

import torch

from ._lib import NndError, check, lib
from .ops import _p, _stream

_SIGNS = ("negative", "positive")


def _is_map(t: torch.Tensor) -> bool:
    return t.ndim == 4 and t.shape[1] == 1 and t.numel() > 0


def _map4(t, what: str, mask=None, shape_first: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The (B,1,H,W) fp32 device map `t` with dense rows (its batch stride is kept; anything else is made contiguous) and its
    bool / uint8 mask, (B,1,H,W) or (B,H,W), as contiguous bytes (None stays None).  The refusals come in this order; with
    `shape_first` (the warp, fill and median families) a wrong shape is named as such whatever the mask and the device."""
    if not torch.is_tensor(t):
        raise NndError(f"{what}: the map must be a tensor on the HIP device; got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise NndError(f"{what}: maps are torch.float32; got {t.dtype}")
    if shape_first and not _is_map(t):
        raise NndError(f"{what}: a map is (B,1,H,W); got {tuple(t.shape)}")
    if mask is not None and (not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8)):
        raise NndError(f"{what}: masks are torch.bool or torch.uint8; got {getattr(mask, 'dtype', type(mask).__name__)}")
    if t.device.type != "cuda":
        raise NndError(f"{what}: the map must be on the HIP device (got {t.device}); there is no CPU fallback")
    if not _is_map(t):
        raise NndError(f"{what}: a map is (B,1,H,W); got {tuple(t.shape)}")
    B, _, H, W = t.shape
    if not (t.stride(3) == 1 and t.stride(2) == W and (B == 1 or t.stride(0) >= H * W)):
        t = t.contiguous()
    if mask is not None:
        if mask.device != t.device:
            raise NndError(f"{what}: the mask is on {mask.device}, the map on {t.device} (no CPU fallback exists)")
        if tuple(mask.shape) not in ((B, 1, H, W), (B, H, W)):
            raise NndError(f"{what}: the mask is {tuple(mask.shape)}, the map {tuple(t.shape)}")
        mask = mask.contiguous()
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    return t, mask


def _nbytes(sizer: str, B: int, H: int, W: int, what: str) -> int:
    """What the library's `sizer` asks for a (B,1,H,W) map; a shape it refuses is refused here under the name `what`."""
    nbytes = int(getattr(lib, sizer)(int(B), int(H), int(W)))
    if nbytes < 0:
        check(nbytes, what)
    return nbytes


def _bstride(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[2] * t.shape[3]


def _features(features, B: int, H: int, W: int, device: torch.device, what: str) -> Tuple[Optional[torch.Tensor], int]:
    """(the (B,C,H,W) fp32 features beside a (B,1,H,W) map on `device`, contiguous; C), or (None, 0)"""
    if features is None:
        return None, 0
    if not torch.is_tensor(features) or features.dtype != torch.float32:
        raise NndError(f"{what}: features are torch.float32; got {getattr(features, 'dtype', type(features).__name__)}")
    if features.device != device:
        raise NndError(f"{what}: the features are on {features.device}, the map on {device} (no CPU fallback exists)")
    if features.ndim != 4 or features.shape[0] != B or tuple(features.shape[2:]) != (H, W) or features.shape[1] < 1:
        raise NndError(f"{what}: features are (B,C,H,W) = ({B},C,{H},{W}); got {tuple(features.shape)}")
    return features.contiguous(), features.shape[1]


def _workspace(nbytes: int, workspace, dtype: torch.dtype, device: torch.device, what: str, sizer_name: str) -> torch.Tensor:
    """The caller's workspace if it holds `nbytes` device bytes, a fresh one of `dtype` words if there is none."""
    if workspace is None:
        return torch.empty(-(-nbytes // dtype.itemsize), dtype=dtype, device=device)
    if not torch.is_tensor(workspace) or workspace.device != device or not workspace.is_contiguous():
        raise NndError(f"{what}: the workspace must be a contiguous tensor on {device}")
    if workspace.numel() * workspace.element_size() < nbytes:
        raise NndError(f"{what}: a workspace of {workspace.numel() * workspace.element_size()} bytes, {nbytes} needed ({sizer_name})")
    return workspace


def _sign(sign: str, what: str) -> int:
    if sign not in _SIGNS:
        raise NndError(f"{what}: disp_sign must be either 'positive' or 'negative'; got {sign!r}")
    return int(sign == "negative")


def camera_params(camera_or_fx, B: int, device: torch.device, what: str = "camera_params",
                  fx_only: bool = True) -> Tuple[torch.Tensor, int]:
    """(device floats {fx, fy, cx, cy} per camera, stride between batch elements: 0 = one camera for all B) of a `scene.Camera`,
    a (3,3) / (B,3,3) intrinsic tensor, or a number (fx alone: what the disparity conversions read).  The device copy of a
    Camera's intrinsic is kept on the Camera (until the tensor is replaced or edited in place)."""
    K = getattr(camera_or_fx, "intrinsic", camera_or_fx)
    if K is None:
        raise NndError(f"{what}: the camera has no intrinsic")
    if isinstance(K, (int, float)):
        if not fx_only:
            raise NndError(f"{what}: fx alone does not back-project; pass a scene.Camera or an intrinsic tensor")
        return torch.empty((1, 4), dtype=torch.float32, device=device).fill_(float(K)), 0  # a fill on the device: no copy
    if not torch.is_tensor(K):
        raise NndError(f"{what}: a scene.Camera, an intrinsic tensor or fx as a number; got {type(K).__name__}")
    if K.ndim not in (2, 3) or tuple(K.shape[-2:]) != (3, 3) or (K.ndim == 3 and K.shape[0] not in (1, B)):
        raise NndError(f"{what}: the intrinsic is (3,3) or (B,3,3) with B = {B}; got {tuple(K.shape)}")
    key = (K.data_ptr(), K._version, str(device))
    cached = getattr(camera_or_fx, "_device_params", None) if camera_or_fx is not K else None
    if cached is not None and cached[0] == key:
        par = cached[1]
    else:
        K3 = K.reshape(-1, 3, 3)
        par = torch.stack([K3[:, 0, 0], K3[:, 1, 1], K3[:, 0, 2], K3[:, 1, 2]], dim=1).to(torch.float32).contiguous()
        par = par.to(device, non_blocking=True)
        if camera_or_fx is not K:
            camera_or_fx._device_params = (key, par)
    return par, (4 if par.shape[0] > 1 else 0)


def disparity_to_depth(disp: torch.Tensor, camera_or_fx, baseline: float, disp_sign: str = "negative", min_disp: float = 0.0,
                       max_depth: Optional[float] = None, valid_mask: Optional[torch.Tensor] = None):
    """(depth (B,1,H,W) fp32, valid (B,1,H,W) uint8).  m = -d for "negative"; z = fp32(double(fx_b) * double(baseline) /
    double(m)); valid = valid_mask && isfinite(m) && m > min_disp && (max_depth is None || z <= max_depth); depth = valid ? z : 0."""
    what = "disparity_to_depth"
    neg = _sign(disp_sign, what)
    if baseline is None:
        raise NndError(f"{what}: no baseline (pass one, or construct the Disparity with its baseline)")
    d, m = _map4(disp, what, valid_mask)
    B, _, H, W = d.shape
    cam, cs = camera_params(camera_or_fx, B, d.device, what)
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=d.device)
    valid = torch.empty((B, 1, H, W), dtype=torch.uint8, device=d.device)
    with torch.cuda.device(d.device):
        check(lib.nnd_disparity_to_depth(_p(d), _bstride(d), _p(m), _p(cam), cs, float(baseline), neg, float(min_disp),
                                         int(max_depth is not None), float(max_depth or 0.0), _p(depth), _p(valid), B, H, W,
                                         _stream(d.device)), what)
    return depth, valid


def depth_to_disparity(depth: torch.Tensor, camera_or_fx, baseline: float, disp_sign: str = "negative", eps: float = 1e-8) -> torch.Tensor:
    """The reference's TartanAir line in its fp32 order: fp32(-baseline * fx) / (depth + fp32(eps)); negated for "positive"."""
    what = "depth_to_disparity"
    neg = _sign(disp_sign, what)
    if baseline is None:
        raise NndError(f"{what}: no baseline")
    z, _ = _map4(depth, what)
    B, _, H, W = z.shape
    cam, cs = camera_params(camera_or_fx, B, z.device, what)
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        check(lib.nnd_depth_to_disparity(_p(z), _bstride(z), _p(cam), cs, float(baseline), neg, float(eps), _p(out), B, H, W,
                                         _stream(z.device)), what)
    return out


def depth_to_points(depth: torch.Tensor, camera, valid_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B,3,H,W): X = fp32((u - cx) * Z / fx), Y = fp32((v - cy) * Z / fy) in double, Z copied; 0 where valid_mask is 0."""
    what = "depth_to_points"
    z, m = _map4(depth, what, valid_mask)
    B, _, H, W = z.shape
    cam, cs = camera_params(camera, B, z.device, what, fx_only=False)
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        check(lib.nnd_depth_to_points(_p(z), _bstride(z), _p(m), _p(cam), cs, _p(out), B, H, W, _stream(z.device)), what)
    return out


def points_compact(depth: torch.Tensor, camera, valid_mask: Optional[torch.Tensor] = None, features: Optional[torch.Tensor] = None):
    """(points (B*H*W,3) fp32, feats (B*H*W,C) or None, offsets (B+1,) int64), all on the device, no host synchronisation.
    The valid points of sample b are rows offsets[b]:offsets[b+1] in row-major pixel order; rows past offsets[B] are
    unspecified.  `features` (B,C,H,W) fp32 is gathered into the same rows.  The same bytes on every run."""
    what = "points_compact"
    z, m = _map4(depth, what, valid_mask)
    B, _, H, W = z.shape
    features, Cf = _features(features, B, H, W, z.device, what)
    feats = torch.empty((B * H * W, Cf), dtype=torch.float32, device=z.device) if Cf else None
    cam, cs = camera_params(camera, B, z.device, what, fx_only=False)
    nbytes = _nbytes("nnd_points_compact_workspace_bytes", B, H, W, what)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=z.device)
    points = torch.empty((B * H * W, 3), dtype=torch.float32, device=z.device)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=z.device)
    with torch.cuda.device(z.device):
        check(lib.nnd_points_compact(_p(z), _bstride(z), _p(m), _p(cam), cs, _p(features), Cf, _p(points), _p(feats), _p(offsets),
                                     _p(ws), ws.numel() * 8, B, H, W, _stream(z.device)), what)
    return points, feats, offsets


def lr_consistency(disp_left: torch.Tensor, disp_right: torch.Tensor, threshold: float = 1.0, left_sign: str = "negative",
                   right_sign: str = "negative", right_flipped: bool = False, return_error: bool = False):
    """The occlusion mask of a left disparity map from the right view's: uint8 of disp_left's shape, 1 = occluded / inconsistent
    (the polarity of the reference's KITTI mask).  `disp_right` is the disparity of the RIGHT view; right_flipped: it is stored
    mirrored in W (the second output of `both_views`) and read in place.  Per pixel (y,x), each step one rounded fp32 operation:

        mL = sL * dL[y,x]                      !isfinite(mL) or mL < 0 -> occluded
        xr = float(x) - mL                     xr < 0 or xr > W-1      -> occluded
        i0 = floor(xr); i1 = min(i0+1, W-1); f = xr - i0
        s = mR(i0) * (1-f) + mR(i1) * f ;  err = |mL - s| ;  occluded = !(err <= threshold)      (a NaN gives occluded)

    return_error: also the (B,1,H,W) fp32 err, +inf where an earlier test decided."""
    what = "lr_consistency"
    nl, nr = _sign(left_sign, what), _sign(right_sign, what)
    dl, dr = _map4(disp_left, what)[0], _map4(disp_right, what)[0]
    if dl.shape != dr.shape or dl.device != dr.device:
        raise NndError(f"{what}: disp_left is {tuple(dl.shape)} on {dl.device}, disp_right {tuple(dr.shape)} on {dr.device}")
    B, _, H, W = dl.shape
    occ = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dl.device)
    err = torch.empty((B, 1, H, W), dtype=torch.float32, device=dl.device) if return_error else None
    with torch.cuda.device(dl.device):
        check(lib.nnd_lr_consistency(_p(dl), _bstride(dl), _p(dr), _bstride(dr), nl, nr, int(bool(right_flipped)), float(threshold),
                                     _p(occ), _p(err), B, H, W, _stream(dl.device)), what)
    return (occ, err) if return_error else occ


def regions_workspace_bytes(B: int, H: int, W: int) -> int:
    """Device bytes `connected_regions` / `speckle_filter` need for a (B,1,H,W) map (9 per pixel); 8-byte aligned."""
    return _nbytes("nnd_connected_regions_workspace_bytes", B, H, W, "regions_workspace_bytes")


def regions_tile() -> Tuple[int, int]:
    """(height, width) of the tile one workgroup labels on chip; regions that cross its borders are merged in a second launch."""
    return int(lib.nnd_connected_regions_tile(0)), int(lib.nnd_connected_regions_tile(1))


def _connectivity(connectivity, what: str) -> int:
    if connectivity not in (4, 8):
        raise NndError(f"{what}: connectivity must be 4 or 8; got {connectivity!r}")
    return int(connectivity)


def _at_least_0(value, name: str, what: str) -> float:
    value = float(value)
    if not value >= 0.0:
        raise NndError(f"{what}: {name} must be >= 0 (+inf is allowed); got {value}")
    return value


def connected_regions(map: torch.Tensor, max_diff: float, valid_mask: Optional[torch.Tensor] = None, connectivity: int = 4,
                      workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(labels, sizes), both (B,1,H,W) int32 on the device.  Per sample: valid = valid_mask (1 = valid; None: set) &&
    isfinite(d); two neighbours (4- or 8-neighbourhood) are joined iff both are valid and fabsf(d[p] - d[q]) <= max_diff, one
    rounded fp32 subtraction; a region is a connected component of that graph.  labels[p] = the smallest row-major index y*W + x
    of p's region, -1 where invalid; sizes[p] = the region's pixel count, 0 where invalid.  Four launches whatever the data, no
    host synchronisation, the same bytes on every run.  `workspace`: a device tensor of `regions_workspace_bytes(B,H,W)` bytes
    to reuse across calls (what a graph capture wants); allocated per call if None."""
    what = "connected_regions"
    conn, md = _connectivity(connectivity, what), _at_least_0(max_diff, "max_diff", what)
    d, m = _map4(map, what, valid_mask)
    B, _, H, W = d.shape
    nbytes = _nbytes("nnd_connected_regions_workspace_bytes", B, H, W, what)
    ws = _workspace(nbytes, workspace, torch.int64, d.device, what, "regions_workspace_bytes")
    labels = torch.empty((B, 1, H, W), dtype=torch.int32, device=d.device)
    sizes = torch.empty((B, 1, H, W), dtype=torch.int32, device=d.device)
    with torch.cuda.device(d.device):
        check(lib.nnd_connected_regions(_p(d), _bstride(d), _p(m), 1, md, conn, _p(labels), _p(sizes), _p(ws),
                                        ws.numel() * ws.element_size(), B, H, W, _stream(d.device)), what)
    return labels, sizes


def speckle_filter(map: torch.Tensor, max_size: int, max_diff: float = 1.0, mask: Optional[torch.Tensor] = None,
                   mask_is_valid: bool = True, connectivity: int = 4, fill: float = 0.0, return_sizes: bool = False,
                   workspace: Optional[torch.Tensor] = None):
    """(filtered (B,1,H,W) fp32, mask_out (B,1,H,W) uint8, speckle (B,1,H,W) uint8[, sizes int32]) in one enqueue.  `mask` is a
    valid mask (mask_is_valid, 1 = valid) or an occlusion mask (1 = invalid); speckle = valid && region size <= max_size (regions
    as in `connected_regions`); filtered = speckle ? fill : map, every other pixel bit for bit; mask_out, in the polarity of
    `mask`, flags as invalid what was invalid (masked out or not finite) or is a speckle."""
    what = "speckle_filter"
    conn, md = _connectivity(connectivity, what), _at_least_0(max_diff, "max_diff", what)
    if isinstance(max_size, bool) or not isinstance(max_size, int) or max_size < 0:
        raise NndError(f"{what}: max_size must be an integer >= 0; got {max_size!r}")
    d, m = _map4(map, what, mask)
    B, _, H, W = d.shape
    nbytes = _nbytes("nnd_connected_regions_workspace_bytes", B, H, W, what)
    ws = _workspace(nbytes, workspace, torch.int64, d.device, what, "regions_workspace_bytes")
    filtered = torch.empty((B, 1, H, W), dtype=torch.float32, device=d.device)
    mask_out = torch.empty((B, 1, H, W), dtype=torch.uint8, device=d.device)
    speckle = torch.empty((B, 1, H, W), dtype=torch.uint8, device=d.device)
    sizes = torch.empty((B, 1, H, W), dtype=torch.int32, device=d.device) if return_sizes else None
    with torch.cuda.device(d.device):
        check(lib.nnd_speckle_filter(_p(d), _bstride(d), _p(m), int(bool(mask_is_valid)), md, conn, max_size, float(fill),
                                     _p(filtered), _p(mask_out), _p(speckle), _p(sizes), _p(ws), ws.numel() * ws.element_size(),
                                     B, H, W, _stream(d.device)), what)
    return (filtered, mask_out, speckle, sizes) if return_sizes else (filtered, mask_out, speckle)


def speckle_mask(map: torch.Tensor, max_size: int, max_diff: float = 1.0, valid_mask: Optional[torch.Tensor] = None,
                 connectivity: int = 4, return_sizes: bool = False):
    """The (B,1,H,W) uint8 mask of the speckles, 1 = a valid pixel whose region (see `connected_regions`) has at most `max_size`
    pixels; with return_sizes also the (B,1,H,W) int32 region sizes."""
    out = speckle_filter(map, max_size, max_diff, valid_mask, True, connectivity, 0.0, return_sizes)
    return (out[2], out[3]) if return_sizes else out[2]


# ---------------------------------------------------------------------------------- view warp and hole filling (csrc/warp.hip)
_RULES = ("min_abs", "max_abs", "nearest")
_VIEWS = ("left", "right")


def warp_max_width() -> int:
    """The widest map `warp_disparity` accepts: a row's 64-bit keys live in LDS."""
    return int(lib.nnd_warp_disparity_limit(0))


def warp_chunk() -> int:
    """The columns of a row a `warp_disparity` workgroup handles per pass."""
    return int(lib.nnd_warp_disparity_limit(1))


def fill_chunk() -> int:
    """The columns of a row a `fill_holes` wave scans per step."""
    return int(lib.nnd_fill_holes_chunk())


def fill_workspace_bytes(B: int, H: int, W: int) -> int:
    """Device bytes `fill_holes` needs for a (B,1,H,W) map (a word per row and chunk, two per row); 4-byte aligned."""
    return _nbytes("nnd_fill_holes_workspace_bytes", B, H, W, "fill_workspace_bytes")


def _warp(what: str, disp, disp_sign, to_view, threshold, mask, mask_is_valid, features, fill, want_source):
    """(disp_other, valid_other in the polarity of the mask, occluded, source or None, features_other or None)"""
    neg = _sign(disp_sign, what)
    if to_view not in _VIEWS:
        raise NndError(f"{what}: to_view must be 'right' or 'left'; got {to_view!r}")
    threshold = _at_least_0(threshold, "threshold", what)
    d, m = _map4(disp, what, mask, shape_first=True)
    B, _, H, W = d.shape
    if W > warp_max_width():
        raise NndError(f"{what}: a width of {W} is above the maximum width {warp_max_width()} (warp_max_width)")
    features, Cf = _features(features, B, H, W, d.device, what)
    feats = torch.empty((B, Cf, H, W), dtype=torch.float32, device=d.device) if Cf else None
    other = torch.empty((B, 1, H, W), dtype=torch.float32, device=d.device)
    valid = torch.empty((B, 1, H, W), dtype=torch.uint8, device=d.device)
    occ = torch.empty((B, 1, H, W), dtype=torch.uint8, device=d.device)
    src = torch.empty((B, 1, H, W), dtype=torch.int32, device=d.device) if want_source else None
    with torch.cuda.device(d.device):
        check(lib.nnd_warp_disparity(_p(d), _bstride(d), _p(m), int(bool(mask_is_valid)), neg, int(to_view == "right"), threshold,
                                     float(fill), _p(features), Cf, _p(other), _p(valid), _p(occ), _p(src), _p(feats), B, H, W,
                                     _stream(d.device)), what)
    return other, valid, occ, src, feats


def warp_disparity(disp: torch.Tensor, disp_sign: str = "negative", to_view: str = "right", threshold: float = 1.0,
                   valid_mask: Optional[torch.Tensor] = None, features: Optional[torch.Tensor] = None, fill: float = 0.0,
                   return_source: bool = False):
    """(disp_other (B,1,H,W) fp32, valid_other uint8, occluded uint8[, source int32][, features_other (B,C,H,W) fp32]): the map
    seen from the other view by a z-buffered forward warp to the nearest column, in one launch.  Per row, each step one rounded
    fp32 operation:

        m      = (negative ? -d[y,x] : d[y,x]) + 0.0f
        src_ok = valid_mask[y,x] (None: 1) && isfinite(m) && m >= 0
        xr     = to_view == "right" ? float(x) - m : float(x) + m ;  t = rintf(xr)  (ties to even)
        lands  = src_ok && 0 <= t <= W-1

    Of the sources that land on (y,t) the largest m wins, among equal m the smallest x: disp_other[y,t] = the winner's value in
    the same sign, valid_other = 1, source = x_win, features_other[:,y,t] = features[:,y,x_win] bit for bit.  A target without a
    source is a hole: `fill`, 0, -1, features 0.  occluded[y,x] = !(lands && m_win(y,t) - m <= threshold): 1 = occluded, out of
    frame or invalid, the polarity of `lr_consistency`.  to_view="left" takes a right-view map.  It is NOT `lr_consistency`: a
    surface that stretches in the other view has one-pixel cracks, and a hidden pixel behind a crack counts as visible."""
    out = _warp("warp_disparity", disp, disp_sign, to_view, threshold, valid_mask, True, features, fill, return_source)
    return tuple(t for t in out if t is not None)


def fill_holes(map: torch.Tensor, mask: Optional[torch.Tensor] = None, mask_is_valid: bool = True, rule: str = "min_abs",
               vertical: bool = True, fill: float = 0.0, workspace: Optional[torch.Tensor] = None):
    """(filled (B,1,H,W) fp32, was_filled uint8, mask_out uint8 in the polarity of `mask`).  ok = mask-valid && isfinite(map).  In a
    row with an ok pixel, a pixel that is not ok takes the value of L or R, its nearest ok columns: the one that exists, else by
    `rule`: "min_abs" L if |v_L| <= |v_R| (the background of a disparity map: the KITTI devkit's rule), "max_abs" L if |v_L| >=
    |v_R|, "nearest" L if x-L <= R-x.  With `vertical`, a row without an ok pixel takes, column by column, the row-pass result of
    the nearest non-empty row above or below by the same rule (above on a tie).  What is left (a sample without an ok pixel; empty
    rows when not vertical) is `fill`.  Values are copied bit for bit, ok pixels too; was_filled = 1 where a value was copied in;
    mask_out flags what is still invalid.  Three launches whatever the data; `workspace`: `fill_workspace_bytes(B,H,W)` device
    bytes to reuse across calls, allocated per call if None."""
    what = "fill_holes"
    if rule not in _RULES:
        raise NndError(f"{what}: rule must be one of {_RULES}; got {rule!r}")
    d, m = _map4(map, what, mask, shape_first=True)
    B, _, H, W = d.shape
    workspace = _workspace(fill_workspace_bytes(B, H, W), workspace, torch.int32, d.device, what, "fill_workspace_bytes")
    filled = torch.empty((B, 1, H, W), dtype=torch.float32, device=d.device)
    was = torch.empty((B, 1, H, W), dtype=torch.uint8, device=d.device)
    mask_out = torch.empty((B, 1, H, W), dtype=torch.uint8, device=d.device)
    with torch.cuda.device(d.device):
        check(lib.nnd_fill_holes(_p(d), _bstride(d), _p(m), int(bool(mask_is_valid)), _RULES.index(rule), int(bool(vertical)),
                                 float(fill), _p(filled), _p(was), _p(mask_out), _p(workspace),
                                 workspace.numel() * workspace.element_size(), B, H, W, _stream(d.device)), what)
    return filled, was, mask_out


# ------------------------------------------------------------------ masked median and guided weighted median (csrc/median.hip)
_KINDS = ("exp", "gauss", "box")


def median_max_radius() -> int:
    """The largest radius `median_filter` accepts."""
    return int(lib.nnd_median_filter_limit(0))


def median_tile() -> Tuple[int, int]:
    """(height, width) of the output tile of one `median_filter` workgroup."""
    return int(lib.nnd_median_filter_limit(1)), int(lib.nnd_median_filter_limit(2))


def _step(sigma, step, what: str) -> float:
    step = float(sigma) / 32 if step is None else float(step)
    if not (step > 0.0 and step < float("inf")):
        raise NndError(f"{what}: step must be finite and > 0; got {step}")
    return step


def range_weights(sigma: float, step: Optional[float] = None, kind: str = "exp"):
    """(numpy uint16[256], inv_step) for `median_filter`: w[b] = floor(65535 * f(b * step) + 0.5) in float64 with f(d) =
    exp(-d / sigma) ("exp"), exp(-d^2 / (2 sigma^2)) ("gauss") or d <= sigma ("box"); `step`, the guide distance one entry of the
    table stands for, defaults to sigma / 32; inv_step = float32(1 / step)."""
    import numpy as np
    what = "range_weights"
    if kind not in _KINDS:
        raise NndError(f"{what}: kind must be one of {_KINDS}; got {kind!r}")
    sigma = float(sigma)
    if not (sigma > 0.0 and sigma < float("inf")):
        raise NndError(f"{what}: sigma must be finite and > 0; got {sigma}")
    step = _step(sigma, step, what)
    d = np.arange(256, dtype=np.float64) * step
    f = np.exp(-d / sigma) if kind == "exp" else np.exp(-d * d / (2.0 * sigma * sigma)) if kind == "gauss" else (d <= sigma).astype(np.float64)
    return np.floor(65535.0 * f + 0.5).astype(np.uint16), float(np.float32(1.0 / step))


def median_filter(map: torch.Tensor, radius: int = 1, valid_mask: Optional[torch.Tensor] = None, mask_is_valid: bool = True,
                  guide: Optional[torch.Tensor] = None, sigma: float = 0.2, step: Optional[float] = None, kind: str = "exp",
                  weights=None, min_count: int = 1, fill_invalid: bool = False, fill: float = 0.0, return_changed: bool = False):
    """(filtered (B,1,H,W) fp32, mask_out uint8 in the polarity of the mask[, changed uint8]): a masked (2r+1) x (2r+1) median, or
    with `guide` ((B,C,H,W) fp32, 1 <= C <= 4, e.g. the left picture) a weighted median that keeps the map's edges on the guide's,
    in one launch (csrc/median.hip).  A selection: every output is a copy of input bits.

      1  ok[q] = mask-valid[q] && isfinite(map[q]).
      2  The window of p = (y,x): the in-frame q with |qy-y| <= r and |qx-x| <= r.  Clipped at the border, no padding.
      3  Order on values: key(v) = bits(v) ^ (sign ? 0xFFFFFFFF : 0x80000000), compared as unsigned: -0.0 < +0.0, and denormals are
         ordinary values.
      4  Tap weight w(p,q): without a guide 1.  With a guide, every step one rounded fp32 operation: dist = |g0[p]-g0[q]|, then
         + |g1[p]-g1[q]|, and so on in channel order; s = dist * inv_step; b = (s < 255.0f) ? (int)s : 255 (a NaN from a non-finite
         guide value gives 255); w = weights[b].
      5  Over the ok taps of the window: n their count, T = sum of w, S(v) = sum of w over the ok taps with key <= key(v).  The
         weighted lower median v* is the tap value of smallest key with 2 S(v*) >= T; all of it integer arithmetic.  With unit
         weights v* is the element of rank (n-1)/2.
      6  produced[p] = (ok[p] || fill_invalid) && n >= min_count && T > 0.
      7  filtered[p] = v* bit for bit if produced[p]; else map[p] bit for bit if ok[p]; else `fill`.
      8  mask_out[p]: valid = ok[p] || produced[p].
      9  changed[p] = 1 where the output bits differ from the input bits, or where a pixel that was not ok got a value.

    The weights are `range_weights(sigma, step, kind)`, or `weights` (256 uint16 values, weights[0] > 0) with `step` (default
    sigma / 32); they travel in the launch's arguments: no device table, no host synchronisation, and the call can be captured
    into a graph.  radius 1 .. `median_max_radius()`, min_count 1 .. (2r+1)^2.  No CPU fallback."""
    import numpy as np
    what = "median_filter"
    if guide is not None and torch.is_tensor(map) and map.dtype == torch.float32 and _is_map(map):  # named whatever the device
        if not torch.is_tensor(guide) or guide.dtype != torch.float32:
            raise NndError(f"{what}: the guide is torch.float32; got {guide.dtype if torch.is_tensor(guide) else type(guide).__name__}")
        B, _, H, W = map.shape
        if guide.ndim != 4 or guide.shape[0] != B or tuple(guide.shape[2:]) != (H, W) or not 1 <= guide.shape[1] <= 4:
            raise NndError(f"{what}: the guide is (B,C,H,W) = ({B},1..4,{H},{W}); got {tuple(guide.shape)}")
    d, m = _map4(map, what, valid_mask, shape_first=True)
    B, _, H, W = d.shape
    radius, min_count = int(radius), int(min_count)
    if not 1 <= radius <= median_max_radius():
        raise NndError(f"{what}: radius {radius} is outside 1 .. {median_max_radius()} (median_max_radius)")
    if not 1 <= min_count <= (2 * radius + 1) ** 2:
        raise NndError(f"{what}: min_count {min_count} is outside 1 .. {(2 * radius + 1) ** 2} = (2 radius + 1)^2")
    C, inv_step, table = 0, 1.0, None
    if guide is not None:
        if guide.device != d.device:
            raise NndError(f"{what}: the guide is on {guide.device}, the map on {d.device} (no CPU fallback exists)")
        guide = guide.contiguous()
        C = guide.shape[1]
        if weights is None:
            table, inv_step = range_weights(sigma, step, kind)
        else:
            table = np.ascontiguousarray(weights)
            if table.dtype != np.uint16 or table.shape != (256,):
                raise NndError(f"{what}: weights are 256 uint16 values; got {table.dtype} {table.shape}")
            if table[0] == 0:
                raise NndError(f"{what}: weights[0] is 0: the centre tap must count")
            inv_step = float(np.float32(1.0 / _step(sigma, step, what)))
    elif weights is not None:
        raise NndError(f"{what}: weights without a guide")
    filtered = torch.empty((B, 1, H, W), dtype=torch.float32, device=d.device)
    mask_out = torch.empty((B, 1, H, W), dtype=torch.uint8, device=d.device)
    changed = torch.empty((B, 1, H, W), dtype=torch.uint8, device=d.device) if return_changed else None
    with torch.cuda.device(d.device):
        check(lib.nnd_median_filter(_p(d), _bstride(d), _p(m), int(bool(mask_is_valid)), radius, min_count, int(bool(fill_invalid)),
                                    float(fill), _p(guide), C, inv_step, None if table is None else table.ctypes.data, _p(filtered),
                                    _p(mask_out), _p(changed), B, H, W, _stream(d.device)), what)
    return (filtered, mask_out, changed) if return_changed else (filtered, mask_out)


# ------------------------------------------------------------------ view synthesis and photometric error (csrc/photometric.hip)
def photometric_max_channels() -> int:
    """The largest channel count of a picture that `synthesize_view` and `photometric_error` accept."""
    return int(lib.nnd_photometric_limit(0))


def photometric_tile() -> Tuple[int, int]:
    """(height, width) of the output tile of one `photometric_error` workgroup."""
    return int(lib.nnd_photometric_limit(1)), int(lib.nnd_photometric_limit(2))


def photometric_workspace_bytes(B: int, H: int, W: int) -> int:
    """Device bytes `photometric_error` needs for its statistics at (B,C,H,W): four doubles per workgroup."""
    return _nbytes("nnd_photometric_workspace_bytes", B, H, W, "photometric_workspace_bytes")


def _pictures(what: str, disp, valid_mask, pictures):
    """The (B,1,H,W) map and its mask through `_map4`, and each (name, picture) as a contiguous (B,C,H,W) fp32 tensor beside it;
    what does not fit is refused by name, whatever the device."""
    if torch.is_tensor(disp) and disp.dtype == torch.float32 and _is_map(disp):
        B, _, H, W = disp.shape
        cmax = photometric_max_channels()
        for name, p in pictures:
            if not torch.is_tensor(p) or p.dtype != torch.float32:
                raise NndError(f"{what}: {name} is torch.float32; got {p.dtype if torch.is_tensor(p) else type(p).__name__}")
            if p.ndim != 4 or p.shape[0] != B or tuple(p.shape[2:]) != (H, W) or not 1 <= p.shape[1] <= cmax:
                raise NndError(f"{what}: {name} is (B,C,H,W) = ({B},1..{cmax},{H},{W}); got {tuple(p.shape)}")
        if len({p.shape[1] for _, p in pictures}) > 1:
            raise NndError(f"{what}: the pictures have {' and '.join(str(p.shape[1]) for _, p in pictures)} channels")
    d, m = _map4(disp, what, valid_mask, shape_first=True)
    out = []
    for name, p in pictures:
        if p.device != d.device:
            raise NndError(f"{what}: {name} is on {p.device}, the map on {d.device} (no CPU fallback exists)")
        out.append(p.contiguous())
    if d.shape[2] < 2 or d.shape[3] < 2:
        raise NndError(f"{what}: a map of {tuple(d.shape)}: H and W must be at least 2 (the reflected border)")
    return d, m, out


def _view(view: str, what: str) -> int:
    if view not in _VIEWS:
        raise NndError(f"{what}: target_view must be one of {_VIEWS}; got {view!r}")
    return int(view == "left")


def synthesize_view(other: torch.Tensor, disp: torch.Tensor, disp_sign: str = "negative", target_view: str = "left",
                    valid_mask: Optional[torch.Tensor] = None, mask_is_valid: bool = True, fill: float = 0.0):
    """(recon (B,C,H,W) fp32, valid (B,1,H,W) uint8 in the polarity of the mask): the OTHER picture seen from the view `disp`
    belongs to, a backward warp along the row in one launch (csrc/photometric.hip).  Per pixel, each step one rounded fp32
    operation:

        m = (+-d) + 0.0f ;  src_ok = mask-valid && isfinite(m) && m >= 0
        xr = float(x) - m for target_view "left" (other = the right picture), float(x) + m for "right"
        in = src_ok && 0 <= xr <= W-1 ;  i0 = floor(xr), i1 = min(i0+1, W-1), f = xr - i0
        recon_c = in ? other_c[y,i0] * (1-f) + other_c[y,i1] * f : fill          (mul, mul, add)

    valid = in; with mask_is_valid False the returned mask is 1 where NOT in, like the occlusion mask that was read.  No CPU
    fallback."""
    what = "synthesize_view"
    neg, left = _sign(disp_sign, what), _view(target_view, what)
    d, m, (o,) = _pictures(what, disp, valid_mask, (("the other picture", other),))
    B, C, H, W = o.shape
    recon = torch.empty((B, C, H, W), dtype=torch.float32, device=d.device)
    valid = torch.empty((B, 1, H, W), dtype=torch.uint8, device=d.device)
    with torch.cuda.device(d.device):
        check(lib.nnd_synthesize_view(_p(o), _p(d), _bstride(d), _p(m), int(bool(mask_is_valid)), neg, left, float(fill), _p(recon),
                                      _p(valid), B, C, H, W, _stream(d.device)), what)
    return recon, valid


def photometric_error(target: torch.Tensor, other: torch.Tensor, disp: torch.Tensor, disp_sign: str = "negative",
                      target_view: str = "left", valid_mask: Optional[torch.Tensor] = None, mask_is_valid: bool = True,
                      ssim_weight: float = 0.85, data_range: float = 2.0, fill: float = 0.0, return_parts: bool = False,
                      stats: bool = True, workspace: Optional[torch.Tensor] = None):
    """(error (B,1,H,W) fp32, valid (B,1,H,W) uint8 in the polarity of the mask, stats[, l1, dssim]): how well `disp` explains
    `target` from `other`, the Monodepth photometric error ssim_weight * (1 - SSIM) / 2 + (1 - ssim_weight) * |target - recon| /
    data_range with a 3 x 3 reflected window, fused with the backward warp of `synthesize_view` in one launch
    (csrc/photometric.hip; the numbered contract is in include/nndepth_amd.h).  c1 = (0.01 data_range)^2, c2 = (0.03
    data_range)^2 and 1 / data_range are formed as float32 here, once; the default 2.0 fits the models' [-1, 1] frames.

    valid: every one of the nine reflected taps was reconstructed (ssim_weight 0: the pixel itself) and the error is finite; the
    other pixels hold `fill` in every map.  stats: a (B,4) float64 DEVICE tensor {count of valid pixels, sum error, sum l1, sum
    dssim} per sample (None with stats=False), added in double in a fixed order by a second small launch: stats[:, 1] / stats[:, 0]
    is the mean error, and nothing here synchronises with the host.  `workspace`: `photometric_workspace_bytes(B,H,W)` device
    bytes of the caller's (a fresh tensor otherwise).  With ssim_weight 0 the error is l1, dssim is `fill` and its sum 0.
    Not here: the edge-aware smoothness term, Monodepth2's identity auto-mask (pass a zero disparity for the unwarped error), other
    windows, gradients, 16-bit pictures.  No CPU fallback."""
    import numpy as np
    what = "photometric_error"
    neg, left = _sign(disp_sign, what), _view(target_view, what)
    w, r = float(ssim_weight), float(data_range)
    if not 0.0 <= w <= 1.0:
        raise NndError(f"{what}: ssim_weight must be in [0, 1]; got {ssim_weight}")
    if not (r > 0.0 and r < float("inf")):
        raise NndError(f"{what}: data_range must be finite and > 0; got {data_range}")
    c1, c2, inv_range = (float(np.float32(v)) for v in ((0.01 * r) ** 2, (0.03 * r) ** 2, 1.0 / r))
    d, m, (t, o) = _pictures(what, disp, valid_mask, (("the target picture", target), ("the other picture", other)))
    B, C, H, W = t.shape
    dev = d.device
    error = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    valid = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev)
    l1 = torch.empty_like(error) if return_parts else None
    dssim = torch.empty_like(error) if return_parts else None
    st, ws, ws_bytes = None, None, 0
    if stats:
        st = torch.empty((B, 4), dtype=torch.float64, device=dev)
        ws = _workspace(photometric_workspace_bytes(B, H, W), workspace, torch.float64, dev, what, "photometric_workspace_bytes")
        ws_bytes = ws.numel() * ws.element_size()
    with torch.cuda.device(dev):
        check(lib.nnd_photometric_error(_p(t), _p(o), _p(d), _bstride(d), _p(m), int(bool(mask_is_valid)), neg, left, w, c1, c2, inv_range,
                                        float(fill), _p(error), _p(l1), _p(dssim), _p(valid), _p(st), _p(ws), ws_bytes, B, C, H, W,
                                        _stream(dev)), what)
    return (error, valid, st, l1, dssim) if return_parts else (error, valid, st)


def photometric_score(forward: Callable, left: torch.Tensor, right: torch.Tensor, threshold: float = 1.0, **kw):
    """(scene.Disparity, error, stats): `occlusion_from_warp(forward, left, right, threshold)`, then `photometric_error(left,
    right, disp.data, valid_mask=disp.occlusion, mask_is_valid=False, **kw)`: one forward, and whether its map explains the right
    picture from the left where the warp does not call it occluded."""
    disp = occlusion_from_warp(forward, left, right, threshold)
    out = photometric_error(left, right, disp.data, valid_mask=disp.occlusion, mask_is_valid=False, **kw)
    return disp, out[0], out[2]


def occlusion_from_warp(forward: Callable, left: torch.Tensor, right: torch.Tensor, threshold: float = 1.0):
    """scene.Disparity(data=disp_left, disp_sign="negative", occlusion=mask) from ONE call of `forward` at batch B: the `occluded`
    mask of `warp_disparity` on outputs[-1]["up_disp"][:, :1].  The single-forward counterpart of `occlusion`; not the same
    definition (see `warp_disparity`)."""
    from .scene import Disparity
    up = forward(left, right)[-1]["up_disp"]
    if not torch.is_tensor(up) or up.ndim != 4 or up.shape[0] != left.shape[0]:
        raise NndError(f"occlusion_from_warp: the forward returned up_disp {tuple(getattr(up, 'shape', ()))} for a batch of "
                       f"{left.shape[0]}")
    dl = up[:, :1]
    mask = _warp("occlusion_from_warp", dl, "negative", "right", threshold, None, True, None, 0.0, False)[2]
    return Disparity(data=dl, disp_sign="negative", occlusion=mask)


def pair_both_views(left: torch.Tensor, right: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """frames1 = [left ; flipW(right)], frames2 = [right ; flipW(left)], batch 2B, in one launch."""
    what = "both_views"
    for t in (left, right):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise NndError(f"{what}: frames are torch.float32; got {getattr(t, 'dtype', type(t).__name__)}")
        if t.device.type != "cuda":
            raise NndError(f"{what}: the frames must be on the HIP device (got {t.device}); there is no CPU fallback")
    if left.ndim != 4 or left.shape != right.shape or left.device != right.device or left.numel() == 0:
        raise NndError(f"{what}: two (B,C,H,W) frames of one shape on one device; got {tuple(left.shape)} and {tuple(right.shape)}")
    left, right = left.contiguous(), right.contiguous()
    B, Cc, H, W = left.shape
    f1 = torch.empty((2 * B, Cc, H, W), dtype=torch.float32, device=left.device)
    f2 = torch.empty_like(f1)
    with torch.cuda.device(left.device):
        check(lib.nnd_pair_both_views(_p(left), _p(right), _p(f1), _p(f2), B, Cc, H, W, _stream(left.device)), what)
    return f1, f2


def both_views(forward: Callable, left: torch.Tensor, right: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(disp_left, disp_right_flipped) from ONE call of `forward` (a model or a `GraphedForward`) at batch 2B.  The flipped,
    swapped pair [flipW(right), flipW(left)] is a rectified pair whose "left" disparity is the right view's, mirrored in W:
    feed it to `lr_consistency(..., right_flipped=True)` as it is.  Only outputs[-1]["up_disp"] is used; the two halves come
    back as views of it (channel 0 of a 2-channel map)."""
    f1, f2 = pair_both_views(left, right)
    up = forward(f1, f2)[-1]["up_disp"]
    B = left.shape[0]
    if up.ndim != 4 or up.shape[0] != 2 * B:
        raise NndError(f"both_views: the forward returned up_disp {tuple(up.shape)} for a batch of {2 * B}")
    return up[:B, :1], up[B:, :1]


def occlusion(forward: Callable, left: torch.Tensor, right: torch.Tensor, threshold: float = 1.0):
    """scene.Disparity(data=disp_left, disp_sign="negative", occlusion=mask): `both_views`, then `lr_consistency`."""
    from .scene import Disparity
    dl, dr = both_views(forward, left, right)
    mask = lr_consistency(dl, dr, threshold, "negative", "negative", right_flipped=True)
    return Disparity(data=dl, disp_sign="negative", occlusion=mask)
