"""Device-side scene types: drop-ins for the reference's `nndepth.scene` (`Disparity`, `Depth`, `Frame`, `Camera`;
nndepth/scene/disparity.py, depth.py, frame.py, camera.py) that keep the maps on the GPU.

The tail of every inference script of the reference,

    Disparity(out[-1]["up_disp"][0].cpu(), "negative").get_view(cmap="RdYlGn")      # raft_stereo/scripts/inference.py:118-119
    Depth(depth[0].cpu(), valid_mask).get_view(cmap="magma")                        # midas/scripts/inference.py:106-110

is written here without the `.cpu()`: the map stays where the model left it, the HIP kernels of csrc/scene.hip colour it, and
the only device-to-host copy is the finished uint8 picture.  `get_view_tensor` returns that picture as a device tensor with no
host synchronisation (what a serving loop chains after `GraphedForward`).  The resizes of the dataloaders (`interpolate`,
`maxpool`, `minpool`) run on the device as well.  Nothing falls back to PyTorch: a CPU tensor is refused.  Beyond the reference:
`Disparity.to_depth`, `Depth.to_disparity`, `Depth.to_points_map`, `Depth.points_tensor` and `Depth.to_points` consume the
`baseline` and `Camera.intrinsic` the reference only stores (geometry.py, csrc/geometry.hip); `Disparity.remove_speckles` and
`Depth.remove_speckles` drop small connected patches (csrc/speckle.hip); `Disparity.to_other_view`, `Disparity.warp_occlusion` and the
two `fill_holes` warp a map into the other view, find the occlusion that warp reveals and fill holes (csrc/warp.hip); the two
`median_filter` end that chain with a masked median or a weighted median guided by the picture (csrc/median.hip).

Constructor arguments, attributes, method names, defaults and the ranks of what comes back are the reference's, its quirks
included (Q9, the pooled occlusion of every batch element is gathered from plane 0; `resize` leaves `self.data`
4-dimensional).  `cmap` may be a colormap name or a matplotlib `Colormap` (turned into a table on the host once, matplotlib
imported lazily), `"red2green"`, or an `(N,3)` / `(N,4)` table (uint8, or float in [0,1]; 2 <= N <= 4096) as a tensor or array."""
from typing import Dict, List, Literal, Optional, Tuple, Union

import numpy as np
import torch

from . import ops
from ._lib import NndError

_METHODS = ("interpolate", "maxpool", "minpool")
MAX_TABLE = 4096


class SceneValueError(NndError, ValueError):
    """A bad value refused on the host (the reference raises ValueError there)."""


_TABLES_HOST: Dict[str, np.ndarray] = {}
_TABLES_DEV: Dict[Tuple[str, str], torch.Tensor] = {}


def _table_of_colormap(c) -> np.ndarray:
    return (c(np.arange(c.N))[:, :3] * 255).astype(np.uint8)


def _named_table(name: str) -> np.ndarray:
    tab = _TABLES_HOST.get(name)
    if tab is None:
        try:
            import matplotlib
            import matplotlib.colors
        except ImportError as e:
            raise NndError(f"cmap={name!r}: matplotlib is not installed, so a colormap name cannot be turned into a table; "
                           "pass an (N,3) uint8 table instead") from e
        if name == "red2green":
            c = matplotlib.colors.LinearSegmentedColormap.from_list("rg", ["r", "w", "g"], N=256)
        else:
            try:
                c = matplotlib.colormaps[name]
            except KeyError as e:
                raise SceneValueError(f"cmap={name!r} is not a colormap matplotlib knows") from e
        tab = _TABLES_HOST[name] = _table_of_colormap(c)
    return tab


def colormap_table(cmap, device=None) -> torch.Tensor:
    """The (N,3) uint8 table `get_view` indexes, for a name, a matplotlib `Colormap` or an (N,3) / (N,4) table; on `device` if
    given (tables of names are uploaded once per device).  The table of a colormap c is
    (c(np.arange(c.N))[:, :3] * 255).astype(np.uint8)."""
    key = None
    if isinstance(cmap, str):
        key = (cmap, str(device))
        if device is not None and key in _TABLES_DEV:
            return _TABLES_DEV[key]
        tab = torch.from_numpy(_named_table(cmap))
    elif torch.is_tensor(cmap) or isinstance(cmap, (np.ndarray, list, tuple)):
        uploaded = torch.is_tensor(cmap) and cmap.dtype == torch.uint8  # a uint8 tensor stays where it is
        tab = cmap if uploaded else np.asarray(cmap.cpu() if torch.is_tensor(cmap) else cmap)
        if tab.ndim != 2 or tab.shape[1] not in (3, 4):
            raise NndError(f"cmap: a table is (N,3) or (N,4); got {tuple(tab.shape)}")
        tab = tab[:, :3]
        if not uploaded and tab.dtype != np.uint8:
            if tab.dtype.kind != "f":
                raise NndError(f"cmap: a table is uint8, or float in [0,1]; got {tab.dtype}")
            if tab.size and (tab.min() < 0.0 or tab.max() > 1.0):
                raise NndError("cmap: a float table holds values in [0,1]")
            tab = (tab * 255).astype(np.uint8)
        if not uploaded:
            tab = torch.from_numpy(np.ascontiguousarray(tab))
    elif callable(cmap) and hasattr(cmap, "N"):
        tab = torch.from_numpy(_table_of_colormap(cmap))
    else:
        raise NndError(f"cmap: a name, a matplotlib Colormap or an (N,3) / (N,4) table; got {type(cmap).__name__}")
    if not 2 <= tab.shape[0] <= MAX_TABLE:
        raise NndError(f"cmap: a table of N = {tab.shape[0]} colours (2 <= N <= {MAX_TABLE})")
    tab = tab.contiguous()
    if device is not None:
        tab = tab.to(device)
        if key is not None:
            _TABLES_DEV[key] = tab
    return tab


def _check_dtypes(t: torch.Tensor, mask: Optional[torch.Tensor], what: str) -> None:
    if not torch.is_tensor(t):
        raise NndError(f"{what}: the map must be a tensor on the HIP device; got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise NndError(f"{what}: maps are torch.float32; got {t.dtype}")
    if mask is not None and mask.dtype not in (torch.bool, torch.uint8):
        raise NndError(f"{what}: masks are torch.bool or torch.uint8; got {mask.dtype}")


def _check_device(t: torch.Tensor, what: str) -> None:
    if t.device.type != "cuda":
        raise NndError(f"{what}: the map must be on the HIP device (got {t.device}); there is no CPU fallback")


def _align(kwargs: dict, what: str) -> bool:
    extra = set(kwargs) - {"align_corners"}
    if extra:
        raise NndError(f"{what}: of F.interpolate's keywords only align_corners is built; got {sorted(extra)}")
    return bool(kwargs.get("align_corners", False))


def _mask_like(new: torch.Tensor, old: Optional[torch.Tensor]) -> torch.Tensor:
    """The new uint8 mask in the old mask's dtype, uint8 if there was none."""
    return new.view(torch.bool) if old is not None and old.dtype == torch.bool else new


def _pool_kernel(HW, size, what: str) -> Tuple[int, int]:
    kh, kw = HW[0] // int(size[0]), HW[1] // int(size[1])
    if kh < 1 or kw < 1:
        raise NndError(f"{what}: maxpool / minpool only shrink; {tuple(HW)} -> {tuple(size)}")
    return kh, kw


def _view_tensor(data: torch.Tensor, mask: Optional[torch.Tensor], kind: int, min, max, cmap, reverse, what: str) -> torch.Tensor:
    _check_dtypes(data, mask, what)
    if data.ndim not in (3, 4):
        raise NndError(f"{what}: a map of 3 or 4 dimensions; got {data.ndim}")
    if min is not None and max is not None and float(min) > float(max):
        raise SceneValueError(f"{what}: minvalue must be less than or equal to maxvalue (min={min}, max={max})")
    table = colormap_table(cmap)  # refuses a bad table before anything else happens
    _check_device(data, what)
    data4 = data if data.ndim == 4 else data[None]
    table = colormap_table(cmap, data.device)
    return ops.colorize(data4, mask, kind, table, None if min is None else float(min), None if max is None else float(max), reverse)


def _to_host(view: torch.Tensor, ndim: int) -> Union[np.ndarray, List[np.ndarray]]:
    pics = view.cpu().numpy()
    return pics[0] if ndim == 3 else [pics[i] for i in range(pics.shape[0])]


_VIEW_DOC = """
        `get_view_tensor` returns the (B,H,W,3) uint8 picture on the device (B = 1 for a 3-dimensional map): no host
        synchronisation, allocations through PyTorch only, so it can be captured into a HIP graph (pass the table as a device
        tensor, or call once before the capture so that the name's table is already uploaded).  `get_view` copies that picture
        to the host and returns what the reference returns: an (H,W,3) uint8 array for a 3-dimensional map, a list of them
        for a 4-dimensional one.  Only channel 0 is coloured; the range is taken over all channels of a batch element, per
        batch element; `self.data` is not modified.  A bound that is not given comes from the map on the device, so `min` >
        the map's own maximum cannot be refused on the host as the reference does (both bounds given with min > max is).
        Non-finite values in the map (outside a Depth's invalid pixels, which are filled) are outside the contract: they get
        some colour of the table."""


class Disparity:
    def __init__(self, data: torch.Tensor, disp_sign: Literal["negative", "positive"] = "negative",
                 occlusion: Optional[torch.Tensor] = None, baseline: Optional[float] = None):
        self.data = data
        self.disp_sign = disp_sign
        self.occlusion = occlusion
        self.baseline = baseline

    def resize(self, size: Tuple[int, int], method: str = "interpolate", **resize_kwargs):
        """Disparity.resize of the reference on the device; `data * W_new / W_old` in that order in fp32.

        `interpolate`: bilinear (align_corners from resize_kwargs, default False); the occlusion is interpolated as float and
        cast back to its dtype.  `maxpool` / `minpool`: the extreme of |data| over non-overlapping windows of
        (H // size[0], W // size[1]) with the sign of disp_sign, then a bilinear resize if the pooled size is not `size`.  The
        pooled occlusion is gathered as the reference gathers it, occlusion.flatten()[indices.flatten()] with plane-local
        indices: EVERY batch element and channel reads the occlusion of plane 0 (kept).  Pool + bilinear with an
        occlusion raises in the reference and is refused here."""
        assert method in _METHODS, "method must be in [`interpolate`, `maxpool`, `minpool`]"
        _check_dtypes(self.data, self.occlusion, "Disparity.resize")
        assert self.data.ndim <= 4, "Only support resize disparity with 3 or 4 dimensions"
        align = _align(resize_kwargs, "Disparity.resize")
        size = (int(size[0]), int(size[1]))
        missing_dim = 4 - self.data.ndim
        for _ in range(missing_dim):
            self.data = self.data[None]
        if self.occlusion is not None:
            assert self.occlusion.ndim <= 4, "Only support resize occlusion with 3 or 4 dimensions"
            missing_dim = 4 - self.occlusion.ndim
            for _ in range(missing_dim):
                self.occlusion = self.occlusion[None]
        W_old = self.data.shape[-1]
        rescale = (float(size[1]), float(W_old))
        occlusion = None
        if method == "interpolate":
            _check_device(self.data, "Disparity.resize")
            data, _ = ops.resize_bilinear(self.data, size, align, rescale=rescale)
            if self.occlusion is not None:
                occ = ops.resize_bilinear(self.occlusion, size, align, u8_mode=1 if self.occlusion.dtype == torch.bool else 2)
                occlusion = _mask_like(occ, self.occlusion)
        else:
            assert self.disp_sign in ("positive", "negative"), "disp_sign must be either 'positive' or 'negative'"
            H, W = self.data.shape[-2:]
            kh, kw = _pool_kernel((H, W), size, "Disparity.resize")
            exact = (H // kh, W // kw) == size
            if self.occlusion is not None and not exact:
                raise NndError(f"Disparity.resize: {method} of {(H, W)} to {size} needs a bilinear step after the pool, and the "
                               "reference cannot carry an occlusion through that (its gather no longer fits); drop the occlusion "
                               "or choose a size that divides")
            _check_device(self.data, "Disparity.resize")
            data, _, occ, _ = ops.pool_abs(self.data, (kh, kw), method == "minpool", self.disp_sign == "negative",
                                           rescale if exact else None, self.occlusion)
            if not exact:
                data, _ = ops.resize_bilinear(data, size, align, rescale=rescale)
            if occ is not None:
                occlusion = _mask_like(occ, self.occlusion)
        for _ in range(missing_dim):
            data = data[0]
            if occlusion is not None:
                occlusion = occlusion[0]
        return Disparity(data=data, disp_sign=self.disp_sign, occlusion=occlusion)

    def get_view_tensor(self, min=None, max=None, cmap="nipy_spectral", reverse=False) -> torch.Tensor:
        return _view_tensor(self.data, self.occlusion, 0, min, max, cmap, reverse, "Disparity.get_view")

    def get_view(self, min=None, max=None, cmap="nipy_spectral", reverse=False) -> Union[np.ndarray, List[np.ndarray]]:
        return _to_host(self.get_view_tensor(min, max, cmap, reverse), self.data.ndim)

    get_view.__doc__ = get_view_tensor.__doc__ = """The coloured |disparity| (occluded pixels, occlusion == 1, at 0).
""" + _VIEW_DOC

    def to_depth(self, camera_or_fx, baseline: Optional[float] = None, min_disp: float = 0.0, max_depth: Optional[float] = None,
                 valid_mask: Optional[torch.Tensor] = None) -> "Depth":
        """Metric depth on the device (geometry.disparity_to_depth): z = fp32(double(fx) * double(baseline) / double(m)) with
        m = -data for disp_sign "negative".  `camera_or_fx`: a Camera, an intrinsic tensor ((3,3) or (B,3,3)) or fx as a number;
        `baseline` defaults to self.baseline.  The returned Depth carries valid_mask (uint8, 1 = valid): `valid_mask` given here
        && isfinite(m) && m > min_disp && (max_depth is None || z <= max_depth); invalid pixels have depth 0.  (B,1,H,W) maps; not a
        method of the reference."""
        from . import geometry
        baseline = self.baseline if baseline is None else baseline
        if baseline is None:
            raise NndError("Disparity.to_depth: no baseline: pass one, or construct the Disparity with its baseline")
        depth, valid = geometry.disparity_to_depth(self.data, camera_or_fx, baseline, self.disp_sign, min_disp, max_depth, valid_mask)
        return Depth(data=depth, valid_mask=valid)

    def remove_speckles(self, max_size: int, max_diff: float = 1.0, connectivity: int = 4, fill: float = 0.0) -> "Disparity":
        """A new Disparity without its speckles, on the device (geometry.speckle_filter, csrc/speckle.hip): a speckle is a pixel
        whose connected region has at most `max_size` pixels, where two neighbours (4- or 8-neighbourhood) hang together iff
        neither is occluded, both are finite and |d[p] - d[q]| <= max_diff.  Speckles take the value `fill`; every other pixel is
        copied bit for bit.  The returned occlusion (1 = invalid, in the dtype of self.occlusion, uint8 if there was none) is the
        old one, the non-finite pixels and the removed ones.  (B,1,H,W) maps; not a method of the reference."""
        from . import geometry
        data, occ, _ = geometry.speckle_filter(self.data, max_size, max_diff, self.occlusion, False, connectivity, fill)
        return Disparity(data=data, disp_sign=self.disp_sign, occlusion=_mask_like(occ, self.occlusion), baseline=self.baseline)

    _FILL_RULES = {"background": "min_abs", "foreground": "max_abs", "nearest": "nearest"}

    def to_other_view(self, to: str = "right", threshold: float = 1.0, features: Optional[torch.Tensor] = None):
        """This map seen from the other view (geometry.warp_disparity, csrc/warp.hip): a z-buffered forward warp to the nearest
        column; `to="left"` for a right-view map.  Occluded pixels (self.occlusion == 1) are no sources.  The returned Disparity
        has the same disp_sign and baseline; its occlusion is 1 in the holes (targets no source lands on, value 0), in the dtype of
        self.occlusion, uint8 if there was none.  With `features` ((B,C,H,W) fp32, e.g. the left picture) returns (Disparity,
        features seen from the other view, 0 in the holes).  (B,1,H,W) maps; not a method of the reference."""
        from . import geometry
        data, hole, _, _, feats = geometry._warp("Disparity.to_other_view", self.data, self.disp_sign, to, threshold, self.occlusion,
                                                 False, features, 0.0, False)
        out = Disparity(data=data, disp_sign=self.disp_sign, occlusion=_mask_like(hole, self.occlusion), baseline=self.baseline)
        return out if features is None else (out, feats)

    def warp_occlusion(self, threshold: float = 1.0) -> "Disparity":
        """The same map with the occlusion that its own warp into the other view reveals (geometry.warp_disparity): a pixel is
        occluded if it was (self.occlusion == 1), is not finite or of the wrong sign, leaves the frame, or loses its target column
        to a surface more than `threshold` nearer.  One map, no second forward; not the definition of `lr_consistency` (a hidden
        pixel behind a one-pixel crack of a stretching surface counts as visible).  The mask keeps its dtype, uint8 if there was
        none."""
        from . import geometry
        occ = geometry._warp("Disparity.warp_occlusion", self.data, self.disp_sign, "right", threshold, self.occlusion, False, None,
                             0.0, False)[2]
        return Disparity(data=self.data, disp_sign=self.disp_sign, occlusion=_mask_like(occ, self.occlusion), baseline=self.baseline)

    def fill_holes(self, rule: str = "background", vertical: bool = True) -> "Disparity":
        """A dense map (geometry.fill_holes): occluded or non-finite pixels take the value of the nearest valid pixel of their row
        to the left or right, "background": the one of smaller |disparity| (the KITTI devkit's rule), "foreground": the larger,
        "nearest": the nearer; rows without a valid pixel are filled from the rows above and below when `vertical`.  Values are
        copied, never interpolated.  The returned occlusion (dtype kept, uint8 if there was none) is what remains invalid."""
        from . import geometry
        if rule not in self._FILL_RULES:
            raise NndError(f"Disparity.fill_holes: rule must be one of {tuple(self._FILL_RULES)}; got {rule!r}")
        data, _, occ = geometry.fill_holes(self.data, self.occlusion, False, self._FILL_RULES[rule], vertical)
        return Disparity(data=data, disp_sign=self.disp_sign, occlusion=_mask_like(occ, self.occlusion), baseline=self.baseline)

    def median_filter(self, radius: int = 1, guide=None, sigma: float = 0.2, fill_invalid: bool = False, min_count: int = 1,
                      **weights_kw) -> "Disparity":
        """A new Disparity filtered by a (2 radius + 1)^2 median over the pixels that are neither occluded nor non-finite
        (geometry.median_filter, csrc/median.hip); with `guide` (a Frame or a (B,C,H,W) fp32 tensor, C <= 4: the picture of this
        view) a weighted median, weight exp(-|colour difference| / sigma) (`weights_kw`: step, kind, weights of
        geometry.median_filter), which keeps disparity edges on colour edges.  Every value is a copy of one of the map's;
        `fill_invalid` also gives the occluded pixels the median of their valid neighbours (at least `min_count` of them).  The
        returned occlusion (dtype kept, uint8 if there was none) is what remains invalid."""
        from . import geometry
        data, occ = geometry.median_filter(self.data, radius, self.occlusion, False, _guide_tensor(guide), sigma,
                                           min_count=min_count, fill_invalid=fill_invalid, **weights_kw)
        return Disparity(data=data, disp_sign=self.disp_sign, occlusion=_mask_like(occ, self.occlusion), baseline=self.baseline)

    def synthesize(self, other, view: str = "left"):
        """(recon, invalid): the OTHER picture (a Frame or a (B,C,H,W) fp32 tensor, C <= 4) seen from this map's view
        (geometry.synthesize_view, csrc/photometric.hip): `view` says which view this map belongs to, "left" samples the right
        picture at x - |d|.  Occluded pixels (self.occlusion == 1) are not reconstructed and hold 0.  `invalid` is in the polarity
        of the occlusion, 1 = not reconstructed (occluded, not finite, of the wrong sign or sampled from outside the frame), in the
        dtype of self.occlusion, uint8 if there was none.  (B,1,H,W) maps; not a method of the reference."""
        from . import geometry
        recon, inv = geometry.synthesize_view(_guide_tensor(other), self.data, self.disp_sign, view, self.occlusion, False)
        return recon, _mask_like(inv, self.occlusion)

    def photometric_error(self, frame, other, view: str = "left", **kw):
        """(error, invalid, stats[, l1, dssim]): how well this map explains `frame` (the picture of its own view) from `other`
        (the other view's), the Monodepth L1 + SSIM error per pixel and its per-sample sums on the device
        (geometry.photometric_error; `kw`: ssim_weight, data_range, fill, return_parts, stats, workspace).  Both pictures are
        Frames or (B,C,H,W) fp32 tensors.  Occluded pixels (self.occlusion == 1) are not sampled; `invalid` is in the polarity of the
        occlusion, 1 = no trusted error at this pixel, in the dtype of self.occlusion, uint8 if there was none."""
        from . import geometry
        out = geometry.photometric_error(_guide_tensor(frame), _guide_tensor(other), self.data, self.disp_sign, view, self.occlusion,
                                         False, **kw)
        return (out[0], _mask_like(out[1], self.occlusion)) + tuple(out[2:])


def _guide_tensor(guide):
    """A Frame's picture, (C,H,W) or (B,C,H,W), or a tensor, as the (B,C,H,W) guide of geometry.median_filter."""
    if isinstance(guide, Frame):
        guide = guide.data
        if torch.is_tensor(guide) and guide.ndim == 3:
            guide = guide[None]
    return guide


class Depth:
    def __init__(self, data: torch.Tensor, valid_mask: Optional[torch.Tensor] = None, is_inverse: bool = False):
        self.data = data
        self.valid_mask = valid_mask
        self.is_inverse = is_inverse

    def resize(self, size: Tuple[int, int], method: str = "interpolate", **resize_kwargs):
        """Depth.resize of the reference on the device (no rescale).  With a valid mask the new mask is isfinite of the RESIZED
        data, in the mask's dtype (the old mask's values are not read, as in the reference)."""
        assert method in _METHODS, "method must be in [`interpolate`, `maxpool`, `minpool`]"
        _check_dtypes(self.data, self.valid_mask, "Depth.resize")
        assert self.data.ndim <= 4, "Only support resize depth with 3 or 4 dimensions"
        align = _align(resize_kwargs, "Depth.resize")
        size = (int(size[0]), int(size[1]))
        missing_dim = 4 - self.data.ndim
        for _ in range(missing_dim):
            self.data = self.data[None]
        if self.valid_mask is not None:
            assert self.valid_mask.ndim <= 4, "Only support resize valid_mask with 3 or 4 dimensions"
            missing_dim = 4 - self.valid_mask.ndim
            for _ in range(missing_dim):
                self.valid_mask = self.valid_mask[None]
        want = self.valid_mask is not None
        _check_device(self.data, "Depth.resize")
        if method == "interpolate":
            data, fin = ops.resize_bilinear(self.data, size, align, finite=want)
        else:
            H, W = self.data.shape[-2:]
            kh, kw = _pool_kernel((H, W), size, "Depth.resize")
            exact = (H // kh, W // kw) == size
            data, _, _, fin = ops.pool_abs(self.data, (kh, kw), method == "minpool", False, finite=want and exact)
            if not exact:
                data, fin = ops.resize_bilinear(data, size, align, finite=want)
        valid_mask = _mask_like(fin, self.valid_mask) if want else None
        for _ in range(missing_dim):
            data = data[0]
            if valid_mask is not None:
                valid_mask = valid_mask[0]
        return Depth(data=data, valid_mask=valid_mask)

    def inverse(self, clip_max: float = None, clip_min: float = None, eps: float = 1e-6) -> "Depth":
        """1 / (data + eps), clamped to clip_max and then to clip_min where given."""
        _check_dtypes(self.data, None, "Depth.inverse")
        _check_device(self.data, "Depth.inverse")
        data = ops.depth_inverse(self.data, clip_max, clip_min, eps)
        return Depth(data=data, valid_mask=self.valid_mask.clone() if self.valid_mask is not None else None,
                     is_inverse=not self.is_inverse)

    def get_view_tensor(self, min=None, max=None, cmap="nipy_spectral", reverse=False) -> torch.Tensor:
        return _view_tensor(self.data, self.valid_mask, 1, min, max, cmap, reverse, "Depth.get_view")

    def get_view(self, min=None, max=None, cmap="nipy_spectral", reverse=False) -> Union[np.ndarray, List[np.ndarray]]:
        return _to_host(self.get_view_tensor(min, max, cmap, reverse), self.data.ndim)

    get_view.__doc__ = get_view_tensor.__doc__ = """The coloured depth; pixels with valid_mask != 1 take the smallest valid depth
        of their batch element (a batch element without a valid pixel raises in the reference and is outside the contract).
""" + _VIEW_DOC

    # ---- geometry on the device (geometry.py, csrc/geometry.hip); not methods of the reference
    def to_disparity(self, camera_or_fx, baseline: float, disp_sign: Literal["negative", "positive"] = "negative",
                     eps: float = 1e-8) -> Disparity:
        """The reference's TartanAir line (tartanair_dataset.py:239-241) in its own fp32 order:
        fp32(-baseline * fx) / (data + fp32(eps)), negated for "positive"; `baseline` is stored on the result."""
        from . import geometry
        disp = geometry.depth_to_disparity(self.data, camera_or_fx, baseline, disp_sign, eps)
        return Disparity(data=disp, disp_sign=disp_sign, baseline=baseline)

    def remove_speckles(self, max_size: int, max_diff: float = 1.0, connectivity: int = 4, fill: float = 0.0) -> "Depth":
        """`Disparity.remove_speckles` on a depth map: pixels with valid_mask == 0 (or a non-finite depth) belong to no region,
        speckles take `fill`, and the returned valid_mask (1 = valid, in the dtype of self.valid_mask, uint8 if there was none)
        no longer holds them."""
        from . import geometry
        data, valid, _ = geometry.speckle_filter(self.data, max_size, max_diff, self.valid_mask, True, connectivity, fill)
        return Depth(data=data, valid_mask=_mask_like(valid, self.valid_mask), is_inverse=self.is_inverse)

    def fill_holes(self, rule: str = "background", vertical: bool = True) -> "Depth":
        """`Disparity.fill_holes` on a depth map: "background" is the LARGER depth (the smaller value when is_inverse),
        "foreground" the other one, "nearest" the nearer pixel.  The returned valid_mask (dtype kept, uint8 if there was none)
        is 1 wherever the map now has a value."""
        from . import geometry
        far, near = ("min_abs", "max_abs") if self.is_inverse else ("max_abs", "min_abs")
        rules = {"background": far, "foreground": near, "nearest": "nearest"}
        if rule not in rules:
            raise NndError(f"Depth.fill_holes: rule must be one of {tuple(rules)}; got {rule!r}")
        data, _, valid = geometry.fill_holes(self.data, self.valid_mask, True, rules[rule], vertical)
        return Depth(data=data, valid_mask=_mask_like(valid, self.valid_mask), is_inverse=self.is_inverse)

    def median_filter(self, radius: int = 1, guide=None, sigma: float = 0.2, fill_invalid: bool = False, min_count: int = 1,
                      **weights_kw) -> "Depth":
        """`Disparity.median_filter` on a depth map: the median over the pixels with valid_mask == 1 and a finite depth.  The
        returned valid_mask (dtype kept, uint8 if there was none) is 1 wherever the map now has a value."""
        from . import geometry
        data, valid = geometry.median_filter(self.data, radius, self.valid_mask, True, _guide_tensor(guide), sigma,
                                             min_count=min_count, fill_invalid=fill_invalid, **weights_kw)
        return Depth(data=data, valid_mask=_mask_like(valid, self.valid_mask), is_inverse=self.is_inverse)

    def to_points_map(self, camera) -> torch.Tensor:
        """(B,3,H,W): X = fp32((u - cx) * Z / fx), Y = fp32((v - cy) * Z / fy), arithmetic in double, Z copied;
        pixels with valid_mask == 0 become 0."""
        from . import geometry
        return geometry.depth_to_points(self.data, camera, self.valid_mask)

    def points_tensor(self, camera, features: Optional[torch.Tensor] = None):
        """(points (B*H*W,3) fp32, feats (B*H*W,C) or None, offsets (B+1,) int64) on the device, no host synchronisation: the
        valid points of sample b are rows offsets[b]:offsets[b+1] in row-major pixel order, `features` ((B,C,H,W) fp32, e.g.
        the frame's colours) gathered into the same rows; rows past offsets[B] are unspecified.  Deterministic."""
        from . import geometry
        return geometry.points_compact(self.data, camera, self.valid_mask, features)

    def to_points(self, camera, features: Optional[torch.Tensor] = None):
        """`points_tensor`, then ONE host synchronisation to read `offsets`: a list of per-sample (n_b,3) views, or of
        ((n_b,3), (n_b,C)) pairs when features are given."""
        points, feats, offsets = self.points_tensor(camera, features)
        off = offsets.tolist()
        if feats is None:
            return [points[off[b]:off[b + 1]] for b in range(len(off) - 1)]
        return [(points[off[b]:off[b + 1]], feats[off[b]:off[b + 1]]) for b in range(len(off) - 1)]


class Camera:
    """Host-side intrinsics / extrinsics (a 3x3 matrix: plain PyTorch, not a hot path)."""

    def __init__(self, intrinsic: Optional[torch.Tensor] = None, extrinsic: Optional[torch.Tensor] = None):
        self.intrinsic = intrinsic
        self.extrinsic = extrinsic

    def resize(self, size: Union[int, Tuple[int, int]], method: str = "bilinear", **kwargs) -> "Camera":
        """fx, x0 *= size[1]; fy, y0 *= size[0] (the reference multiplies by the size itself, kept)."""
        if self.intrinsic is None:
            return self
        K = self.intrinsic.clone()
        for row, ratio in ((0, size[1]), (1, size[0])):
            K[..., row, row] *= ratio
            K[..., row, 2] *= ratio
        return Camera(K, self.extrinsic)


class Frame:
    def __init__(self, data: torch.Tensor, disparity: Optional[Disparity] = None, depth: Optional[Depth] = None,
                 camera: Optional[Camera] = None, camera_id: Optional[str] = None, pose: Optional[torch.Tensor] = None):
        self.data = data
        self.disparity = disparity
        self.depth = depth
        self.camera = camera
        self.camera_id = camera_id
        self.pose = pose

    def resize(self, size: Tuple[int, int], align_corners=True, disparity_resize_method: str = "interpolate",
               depth_resize_method: str = "interpolate", disparity_resize_kwargs: dict = {}, depth_resize_kwargs: dict = {}):
        """The image by bilinear interpolation (align_corners True by default, unlike Disparity / Depth), the disparity, the
        depth and the camera by their own resize; camera_id is not carried over, as in the reference."""
        assert depth_resize_method in _METHODS, "depth_resize_method must be in [`interpolate`, `maxpool`, `minpool`]"
        assert disparity_resize_method in _METHODS, "disparity_resize_method must be in [`interpolate`, `maxpool`, `minpool`]"
        _check_dtypes(self.data, None, "Frame.resize")
        _check_device(self.data, "Frame.resize")
        assert self.data.ndim <= 4, "Only support resize tensor with 3 or 4 dimensions"
        missing_dim = 4 - self.data.ndim
        for _ in range(missing_dim):
            self.data = self.data[None]
        resized_img, _ = ops.resize_bilinear(self.data, (int(size[0]), int(size[1])), bool(align_corners))
        for _ in range(missing_dim):
            resized_img = resized_img[0]
        disparity = None if self.disparity is None else self.disparity.resize(size, disparity_resize_method, **disparity_resize_kwargs)
        depth = None if self.depth is None else self.depth.resize(size, depth_resize_method, **depth_resize_kwargs)
        camera = None if self.camera is None else self.camera.resize(size)
        return Frame(data=resized_img, disparity=disparity, depth=depth, camera=camera, pose=self.pose)
