"""RAFT-Stereo with the MI355X-native hot path.

`BaseRAFTStereo` keeps the reference's constructor kwargs (= `BaseRAFTStereoModelConfig.to_dict()`,
nndepth/models/raft_stereo/configs.py:11-23), `state_dict()` keys and `forward(frame1, frame2)
-> List[{"up_disp": Tensor}]` (nndepth/models/raft_stereo/model.py:17-163), so the reference's
inference / evaluate scripts can use it unchanged.  Inside `forward()`:

    encoder + cnet_proj      HIP, ONE C-ABI call (csrc/encoder.hip: nnd_encoder_forward; eval-mode BatchNorm folded).
                             `hip_encoder=False` is the explicit opt-in to PyTorch-ROCm modules for the encoder; there is
                             no silent fallback: an encoder the HIP path does not build (group norm, dropout) raises
                                                                                                    model.py:107-109
    corr pyramid build       HIP  (csrc/corr1d.hip)                     model.py:124
    for iters: lookup -> update block -> coords += delta -> convex upsample
                             HIP, ONE C-ABI call for the whole loop     model.py:130-137
                             (csrc/update_block.hip: nnd_raft_stereo_refine)

The classes are inference-only (eval-mode BatchNorm is folded into the convolutions and no autograd graph is recorded):
`forward()` raises in training mode.

`patch(model)` installs the same kernels behind the three duck-typed seams of an *unmodified*
reference model instance: `corr_fn`, `update_block`, `convex_upsample`.
"""
import contextlib
import functools
import json
import os
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import ops
from ._lib import NndError
from .blocks import BasicUpdateBlock
from .cost_volume import CorrBlock1D, GroupCorrBlock1D
from .encoder import BasicEncoder
from .upsample import convex_upsample


def load_weights(model: nn.Module, weights: str, strict_load: bool = True) -> nn.Module:
    """.pth / .safetensors, like nndepth/utils/common.py:8-16."""
    if weights.endswith(".safetensors"):
        from safetensors.torch import load_file
        state = load_file(weights, device="cpu")
    else:
        state = torch.load(weights, map_location="cpu")
    model.load_state_dict(state, strict=strict_load)
    return model


def require_eval(model: nn.Module) -> None:
    """The HIP hot path is inference-only: BatchNorm is folded with its running statistics and nothing records an autograd
    graph, so a model left in training mode would silently compute something else than the reference's training forward."""
    if model.training:
        raise NndError(f"{type(model).__name__} is inference-only on the HIP path: call model.eval() first "
                       "(training-mode BatchNorm / autograd are not built)")


OUTPUTS = ("all", "last")


def check_outputs(outputs: str) -> str:
    """The `outputs` switch of the model classes: "all" = every iteration's up_disp (the reference's list), "last" = the final one
    alone, as a list of one dict (`outs[-1]["up_disp"]` of the reference's inference / evaluate scripts is unchanged); the fused loops
    then compute no mask head and no upsample on the other iterations (NND_FLAG_LAST_UPSAMPLE_ONLY)."""
    if outputs not in OUTPUTS:
        raise NndError(f"outputs={outputs!r}: must be 'all' (every iteration's up_disp) or 'last' (the final one only)")
    return outputs


def last_only(model: nn.Module) -> bool:
    return check_outputs(getattr(model, "outputs", "all")) == "last"


def calibration_passes(run, max_passes: int, error: str) -> None:
    """`run()` inside `ops.calibration()` until no layer saw inf / NaN at the scale it had (status bit 0: that layer's scale was
    lowered by 2^12 since, so go again); NndError(error) if one still does after `max_passes` passes."""
    for _ in range(max_passes):
        with ops.calibration() as c, torch.no_grad():
            run()
        if not (c.status & 1):
            return
    raise NndError(error)


# ------------------------------------------------------------------------------------------------ calibration state
# The activation ranges of a model as data: {"version": 1, "arithmetic": name, "layers": {key: xs}} with xs the exponent of a layer's
# activation scale 2^xs (its valid range is |x| < 65504 / 2^xs) and key = "<module path>/<layer name>" — "fnet/layer1.0.conv1",
# "update_block/encoder.convc2" — or the module path alone where the module is one layer ("cv_regularizer.conv1.0").  Keys come
# from the model's structure, never from the order in which its engines were built or used.  The state is independent of the weights'
# own scales (those are fixed at pack time from the weights), plain Python, and never part of state_dict().  The functions take a
# model class of this package or a reference model patched with patch() / patch_coarse2fine().
CALIBRATION_STATE_VERSION = 1


def calibration_sites(model: nn.Module) -> Dict[str, "ops.ScaleSite"]:
    """{module path: ops.ScaleSite} of every engine that takes part in a calibration of `model`, in a fixed order."""
    fn = getattr(model, "_calibration_sites", None)
    if fn is not None:
        return fn()
    return {"update_block": model.update_block.calibration_site()}  # a patched reference model: the update block is the HIP engine


def _model_arithmetic(model: nn.Module) -> str:
    return getattr(model, "arithmetic", None) or model.update_block.engine.arithmetic


def _site_engine(site: "ops.ScaleSite"):
    """The site's engine if it is packed on a HIP device, else None (not built yet, or packed on the host)."""
    eng = site.engine()
    return eng if eng is not None and eng.on_device() else None


def _layer_key(path: str, name: str) -> str:
    return f"{path}/{name}" if name else path


def calibration_state(model: nn.Module) -> dict:
    """The model's activation ranges (see above).  A loaded state is returned as loaded, without a GPU; otherwise the exponents are
    read from the packed engines (one small launch each, ONE synchronisation), which must exist: after a forward or calibrate()."""
    pinned = getattr(model, "_calib_pinned", None)
    if pinned is not None:
        return {"version": CALIBRATION_STATE_VERSION, "arithmetic": pinned["arithmetic"], "layers": dict(pinned["layers"])}
    keys, parts = [], []
    for path, site in calibration_sites(model).items():
        if not site.names:
            continue
        eng = _site_engine(site)
        if eng is None:
            raise NndError(f"calibration_state: '{path}' is not packed yet: run a forward or calibrate() first, or load a state")
        keys += [_layer_key(path, n) for n in site.names]
        parts.append(eng.read_scales())
    xs = torch.cat([p.to(parts[0].device) for p in parts]).cpu().tolist() if parts else []
    return {"version": CALIBRATION_STATE_VERSION, "arithmetic": _model_arithmetic(model), "layers": dict(zip(keys, xs))}


def _apply_pinned(model: nn.Module, _built=None, force: bool = False) -> None:
    """Writes the loaded state into every packed engine that does not carry it yet (ParamCache.on_build: after every repack)."""
    pinned = getattr(model, "_calib_pinned", None)
    if pinned is None:
        return
    for path, site in calibration_sites(model).items():
        eng = _site_engine(site)
        if eng is not None and site.names and (force or not eng.calibrated):
            eng.write_scales([pinned["layers"][_layer_key(path, n)] for n in site.names])


def load_calibration_state(model: nn.Module, state: dict) -> nn.Module:
    """Pins `state` on the model: written into the engines that are packed (in place: a captured GraphedForward runs with it on its
    next replay), kept pending for the others and written when they are packed, and again after every repack; the model classes do
    not calibrate on their first forward any more.  NndError naming the difference if the state is of another arithmetic or its keys
    are not this model's.  clear_calibration_state() or an explicit calibrate() unpins it."""
    if not isinstance(state, dict) or state.get("version") != CALIBRATION_STATE_VERSION or not isinstance(state.get("layers"), dict):
        raise NndError(f"load_calibration_state: not a version {CALIBRATION_STATE_VERSION} calibration state "
                       "({'version', 'arithmetic', 'layers'})")
    arith = _model_arithmetic(model)
    if state.get("arithmetic") != arith:
        raise NndError(f"load_calibration_state: the state is of arithmetic {state.get('arithmetic')!r}, the model runs {arith!r}")
    sites = calibration_sites(model)
    want = {_layer_key(p, n) for p, s in sites.items() for n in s.names}
    missing, extra = sorted(want - set(state["layers"])), sorted(set(state["layers"]) - want)
    if missing or extra:
        raise NndError("load_calibration_state: the state's layers are not this model's: "
                       + "; ".join(f"{what}: {', '.join(k)}" for what, k in (("missing", missing), ("unexpected", extra)) if k))
    layers = {}
    for k, v in state["layers"].items():
        if isinstance(v, bool) or not isinstance(v, int) or abs(v) > 60:
            raise NndError(f"load_calibration_state: layer {k!r}: exponent {v!r} is not an integer in -60 .. 60")
        layers[k] = v
    model._calib_pinned = {"arithmetic": arith, "layers": layers}
    for site in sites.values():
        site.cache.on_build = functools.partial(_apply_pinned, model)
    _apply_pinned(model, force=True)
    return model


def clear_calibration_state(model: nn.Module) -> nn.Module:
    """Unpins a loaded state: the engines keep the scales they have, a repack returns to the defaults (and the model classes to
    calibrating on their next forward)."""
    model._calib_pinned = None
    for site in calibration_sites(model).values():
        site.cache.on_build = None
    return model


def save_calibration(model: nn.Module, path: str) -> None:
    with open(path, "w") as f:
        json.dump(calibration_state(model), f, indent=1, sort_keys=True)


def load_calibration(model: nn.Module, path: str) -> nn.Module:
    with open(path) as f:
        return load_calibration_state(model, json.load(f))


class AutoCalibrate:
    """fp16x2 activation range (include/nndepth_amd.h "fp16x2 activation range", csrc/calib.hip), shared by the model classes.

    The fp16x2 arithmetic carries an activation x as two fp16 pieces of x * 2^xs with xs per layer.  A freshly packed layer has
    xs = 2 (all 22 bits for 0.06 <= |x| < 16376); `calibrate(frame1, frame2)` runs the forward once with every layer recording the
    largest |activation| M it stages and then sets xs so that M * 2^xs lies in [2^10, 2^11): all 22 bits from M down to M * 2^-13,
    absolute error <= M * 2^-36 below, finite results up to 32 * M, inf / NaN in the output beyond (never a silently wrong value).
    With `auto_calibrate` (default) the first `forward()` after the parameters were (re)packed calibrates on its own input — one
    extra forward, once; call `calibrate()` yourself with representative frames to choose the data, or set
    `auto_calibrate = False` to keep the default scales.  `activation_ranges()` reports the valid |x| per update-block layer.

    The "fp16" arithmetic (opt-in) keeps the first of the two pieces only: 11 significand bits per operand — three more than the bf16
    autocast the reference's trainers validate under, not fp32 parity — with the same scales, calibration and range behaviour.

    The ranges are data (see "calibration state" above): `calibration_state()` / `load_calibration_state()` (`save_calibration` /
    `load_calibration`: a JSON file) carry them to another process or rank (parallel.sync_calibration: the same ranges on every rank);
    a loaded state is pinned — re-applied after every repack, no calibration on the first forward.  `calibrate(..., widen=True)` extends
    the ranges held before instead of replacing them: per layer the smaller exponent, so a range only grows — each step doubles the
    largest |x| and moves the 13 octaves of full precision up with it, away from the small values.  `watch_range = True` adds one small
    launch per forward that looks for inf / NaN in the final output (an exceeded range always reaches it), `range_status()` reads the
    answer; `range_report(frame1, frame2)` says which layer an input exceeds."""

    auto_calibrate = True
    watch_range = False  # True: every forward() ORs "the final output holds inf / NaN" into a device word (range_status)
    _calib_pinned = None  # a loaded calibration state: {"arithmetic", "layers"}
    _range_word = None
    _range_forwards = 0

    @contextlib.contextmanager
    def _all_outputs(self):
        """Inside, the model returns every iteration's map: the mask head records its range over all of them, whatever `outputs` is."""
        outputs = getattr(self, "outputs", "all")
        self.outputs = "all"
        try:
            yield
        finally:
            self.outputs = outputs

    def calibrate(self, *args, max_passes: int = 4, widen: bool = False, **kwargs):
        """widen=False (default): the ranges of these frames replace the ones held.  widen=True: every engine that was calibrated
        (or loaded) before keeps, per layer, the smaller of its old and its new exponent — the ranges only grow."""
        require_eval(self)
        clear_calibration_state(self)  # an explicit calibration unpins a loaded state
        before = []
        if widen and self.arithmetic in ops.RANGE_SCALED:
            for site in calibration_sites(self).values():
                eng = _site_engine(site)
                if eng is not None and site.names and eng.calibrated:
                    before.append((eng, eng.packed, eng.read_scales()))  # device tensors: no synchronisation
        with self._all_outputs():
            calibration_passes(lambda: self._forward(*args, **kwargs), max_passes,
                               f"{type(self).__name__}.calibrate: activations still overflow fp16 after {max_passes} passes "
                               "(non-finite inputs or weights?)")
        for eng, blob, xs in before:
            if eng.packed is blob:  # (not repacked in between)
                eng.widen_scales(xs)
        return self

    def _forward_calibrated(self, *args, **kwargs):
        """`_forward`, calibrating first if an fp16x2 engine on its path still has the default activation scales."""
        check_outputs(getattr(self, "outputs", "all"))  # (an attribute: it may have been set after construction)
        if self.arithmetic not in ops.RANGE_SCALED or not self.auto_calibrate or self._calib_pinned is not None:
            return self._watched(self._forward(*args, **kwargs))  # (a pinned state is written when an engine is packed)
        try:
            with ops.require_calibrated():
                return self._watched(self._forward(*args, **kwargs))
        except ops.NeedsCalibration:
            self.calibrate(*args, **kwargs)
            return self._watched(self._forward(*args, **kwargs))

    # ---- the ranges as data
    def _calibration_sites(self) -> Dict[str, "ops.ScaleSite"]:
        """{module path: site} of the engines a forward of this model calibrates; the model classes add theirs in front."""
        return {"update_block": self.update_block.calibration_site()}

    def _encoder_site(self, cache: "ops.ParamCache", output_dim: int, cnet_dim: int) -> "ops.ScaleSite":
        names = ops.EncoderEngine(output_dim, self.fnet.norm_fn, cnet_dim, self.arithmetic).scale_names()  # descriptor only: host work
        return ops.ScaleSite(names, lambda: cache.value, cache)

    def calibration_state(self) -> dict:
        return calibration_state(self)

    def load_calibration_state(self, state: dict):
        return load_calibration_state(self, state)

    def clear_calibration_state(self):
        return clear_calibration_state(self)

    def save_calibration(self, path: str) -> None:
        save_calibration(self, path)

    def load_calibration(self, path: str):
        return load_calibration(self, path)

    # ---- overflow
    def _watched(self, outs):
        if self.watch_range:
            final = outs if torch.is_tensor(outs) else outs[-1]["up_disp"]
            if self._range_word is None or self._range_word.device != final.device:
                self._range_word = torch.zeros(1, dtype=torch.int32, device=final.device)
            ops.nonfinite_flag(final, self._range_word)
            self._range_forwards += 1
        return outs

    def range_status(self) -> dict:
        """{"overflow": an inf / NaN reached the final output of a watched forward since the last reset, "forwards": how many were
        watched (calls of forward(): the replays of a captured graph are not counted)}.  One synchronisation."""
        word = 0 if self._range_word is None else int(self._range_word.item())
        return {"overflow": bool(word & 1), "forwards": self._range_forwards}

    def reset_range_status(self) -> None:
        if self._range_word is not None:
            self._range_word.zero_()
        self._range_forwards = 0

    def range_report(self, *args, **kwargs) -> Dict[str, Dict[str, float]]:
        """{layer: {"seen": the largest |x| the layer stages on these frames, "limit": 65504 / 2^xs, what it can represent}} — one forward
        that records (NND_FLAG_CALIBRATE) and whose records are read and cleared instead of being turned into scales: no scale
        changes.  seen > limit: that layer is exceeded (behind it the values are inf / NaN).  Layers off this forward's path: seen 0."""
        require_eval(self)
        if self.arithmetic not in ops.RANGE_SCALED:
            return {}
        try:
            with self._all_outputs(), ops.calibration(finish=False), torch.no_grad():
                self._forward(*args, **kwargs)
        finally:  # the records never stay behind: they would join the next calibration's
            sites = [(p, s, _site_engine(s)) for p, s in calibration_sites(self).items() if s.names]
            sites = [(p, s, e) for p, s, e in sites if e is not None]
            got = [(p, s, e.read_scales(), e.read_records(clear=True)) for p, s, e in sites]
        report = {}
        for path, site, xs, seen in got:
            for n, e, m in zip(site.names, xs.cpu().tolist(), seen.cpu().tolist()):
                report[_layer_key(path, n)] = {"seen": float(m), "limit": 65504.0 / 2.0 ** e}
        return report

    def activation_ranges(self):
        eng = self.update_block.engine
        return eng.activation_ranges() if eng.packed is not None else {}


def hip_encoder_blocker(fnet: nn.Module, norms) -> Optional[str]:
    """Why csrc/encoder.hip cannot run this BasicEncoder, or None."""
    if fnet.norm_fn not in norms:
        return f"norm_fn={fnet.norm_fn!r} is not built in HIP (built: {', '.join(norms)})"
    if fnet.dropout is not None:
        return "dropout > 0"
    return None


class BaseRAFTStereo(AutoCalibrate, nn.Module):
    def __init__(self, iters: int = 12, fnet_dim: int = 256, hidden_dim: int = 128, context_dim: int = 128,
                 corr_levels: int = 4, corr_radius: int = 4, tracing: bool = False,
                 include_preprocessing: bool = False, weights: Optional[str] = None, strict_load: bool = True,
                 fused_loop: bool = True, hip_encoder: bool = True, arithmetic: str = "fp16x2", outputs: str = "all", **kwargs):
        super().__init__()
        self.arithmetic = arithmetic  # update-block / encoder convolutions: "fp16x2" (default; 2 fp16 pieces, parity-gated), "bf16x3" (3 bf16 pieces), "fp32" (exact fp32 MFMA) or "fp16" (opt-in: ONE range-scaled fp16 piece, 11 significand bits, finite up to 32 x the calibrated maximum)
        self.outputs = check_outputs(outputs)  # "all": every iteration's up_disp; "last": [{"up_disp": final}] (check_outputs)
        self.iters, self.fnet_dim, self.hidden_dim, self.context_dim = iters, fnet_dim, hidden_dim, context_dim
        self.corr_levels, self.corr_radius = corr_levels, corr_radius
        self.tracing, self.include_preprocessing = tracing, include_preprocessing
        self.fused_loop = fused_loop
        self.hip_encoder = hip_encoder
        self._enc_cache = ops.ParamCache()
        self.fnet = BasicEncoder(output_dim=fnet_dim)
        self.cnet_proj = nn.Sequential(nn.Conv2d(fnet_dim, context_dim + hidden_dim, 3, padding=1), nn.ReLU(False))
        self.update_block = BasicUpdateBlock(hidden_dim=hidden_dim, cor_planes=corr_levels * (2 * corr_radius + 1),
                                             flow_channel=1, context_dim=context_dim, spatial_scale=8, arithmetic=arithmetic)
        self.corr_fn = CorrBlock1D
        self.weights, self.strict_load = weights, strict_load
        if weights is not None:
            load_weights(self, weights, strict_load)

    # seams kept as methods so callers that monkey-patch them keep working
    def convex_upsample(self, flow, mask, rate=8):
        return convex_upsample(flow, mask, rate)

    def initialize_coords(self, fmap1):
        B, _, H, W = fmap1.shape
        return torch.arange(W, device=fmap1.device).float()[None, None, None, :].repeat(B, 1, H, 1)

    def _encoder_engine(self, device) -> "ops.EncoderEngine":
        """(Re)pack fnet + cnet_proj for the HIP encoder if their parameters / buffers changed."""
        def build():
            eng = ops.EncoderEngine(self.fnet_dim, self.fnet.norm_fn, self.context_dim + self.hidden_dim, self.arithmetic)
            return eng.load(self.fnet.state_dict(), self.cnet_proj.state_dict(), eps=1e-5, device=device)
        return self._enc_cache.get((self.fnet, self.cnet_proj), device, build)

    def _calibration_sites(self):
        sites = {}
        if self.hip_encoder and hip_encoder_blocker(self.fnet, ("batch", "none")) is None:  # fnet + cnet_proj: one engine, one blob
            sites["fnet"] = self._encoder_site(self._enc_cache, self.fnet_dim, self.context_dim + self.hidden_dim)
        sites.update(super()._calibration_sites())
        return sites

    def forward_fnet(self, frame1, frame2):
        if self.hip_encoder:
            why = hip_encoder_blocker(self.fnet, ("batch", "none"))
            if why:
                raise NndError(f"BaseRAFTStereo: the HIP encoder cannot run this fnet ({why}); pass hip_encoder=False to run "
                               "the encoder's PyTorch-ROCm modules explicitly")
            # BasicEncoder + cnet_proj in ONE C-ABI call (csrc/encoder.hip); eval-mode BatchNorm folded into the convs
            B = frame1.shape[0]
            # (the two frame tensors are read where they lie: no torch.cat copy, basic_encoder.py:74-76)
            fmaps, cnet = self._encoder_engine(frame1.device).forward(frame1.float(), n_cnet=B, frames_b=frame2.float())
            return fmaps[:B], fmaps[B:], cnet
        fmap1, fmap2 = self.fnet([frame1, frame2])  # explicit opt-in (hip_encoder=False): PyTorch-ROCm modules
        return fmap1, fmap2, self.cnet_proj(fmap1)

    def forward(self, frame1: torch.Tensor, frame2: torch.Tensor, **kwargs) -> List[Dict[str, torch.Tensor]]:
        require_eval(self)
        with torch.no_grad():
            return self._forward_calibrated(frame1, frame2)

    def _forward(self, frame1: torch.Tensor, frame2: torch.Tensor) -> List[Dict[str, torch.Tensor]]:
        fmap1, fmap2, cnet = self.forward_fnet(frame1, frame2)
        rate = frame1.shape[-1] // fmap1.shape[-1]
        fmap1, fmap2 = fmap1.float(), fmap2.float()
        net, inp = ops.split_tanh_relu(cnet.float(), self.hidden_dim)  # split + tanh + relu in one kernel (model.py:119-122)
        corr = self.corr_fn(fmap1, fmap2, self.corr_levels, self.corr_radius)
        last = last_only(self)
        if self.fused_loop and isinstance(corr, CorrBlock1D):
            eng = self.update_block.sync_engine(frame1.device)
            up, _, _ = eng.refine(corr._pyr, self.corr_levels, self.corr_radius, net.float(), inp.float(),
                                  rate, self.iters, keep_all=not last, last_only=last)
            return [{"up_disp": up[i]} for i in range(up.shape[0])]
        # seam-by-seam loop (same shape as the reference's), every step still a HIP kernel
        coords1 = self.initialize_coords(fmap1)
        org = self.initialize_coords(fmap1)
        outs = []
        for i in range(self.iters):
            sampled = corr(coords1)
            net, mask, delta = self.update_block(net, inp, sampled, coords1 - org)
            coords1 = coords1 + delta
            if not last or i == self.iters - 1:
                outs.append({"up_disp": self.convex_upsample(coords1 - org, mask, rate=rate)})
        return outs


def frame_size_outputs(ups, frame_hw, stacked=None):
    """A stage's upsampled maps at frame size, scaled by the width ratio (model.py:309-314: F.interpolate(u, size=frame) * rate).
    An integer ratio in both axes — every frame the cascade accepts — is ONE HIP launch for `stacked`, the fused loop's
    (n, B, 1, h, w) tensor whose slices `ups` are (ops.resize_nearest_scaled, bit-identical to the PyTorch expression), or one
    launch per map without it.  NND_C2F_TORCH_RESIZE=1 (diagnostic, read per call) selects the PyTorch expression."""
    h, w = ups[0].shape[-2:]
    rate = frame_hw[1] / w
    if rate == 1:
        return list(ups)
    if frame_hw[0] % h or frame_hw[1] % w or os.environ.get("NND_C2F_TORCH_RESIZE", "0") not in ("", "0"):
        return [nn.functional.interpolate(u, size=frame_hw) * rate for u in ups]
    if stacked is None:  # the seam-by-seam loop: one launch per map
        return [ops.resize_nearest_scaled(u, frame_hw, rate) for u in ups]
    big = ops.resize_nearest_scaled(stacked, frame_hw, rate)
    return [big[i] for i in range(big.shape[0])]


class Coarse2FineRAFTStereoBase(AutoCalibrate, nn.Module):
    """The hot path of `Coarse2FineGroupRepViTRAFTStereo` (nndepth/models/raft_stereo/model.py:166-320) on HIP: per cascade stage the
    group correlation pyramid (GroupCorrBlock1D, quirks Q4 / Q6 kept), the ConvGRU update block (`gru="conv_gru"`, spatial scale
    (4, 4)), the convex upsample and the loop around them, stage after stage (1/64 -> 1/16 -> 1/4 with the reference's encoder), every
    iteration's disparity brought to frame size like the reference (`interpolate` x rate, nearest).

    The encoder side is NOT part of the path (the RepViT backbone, the MobileOne `cnet_proj` and the FeatureFusionBlocks
    are PyTorch modules in the reference and stay PyTorch-ROCm modules here): a subclass supplies them through `_init_fnet`,
    `_init_cnet_proj`, `_init_fusion_blocks` with the reference's interfaces — `fnet(x)` returns the feature pyramid of which
    `[::2][::-1]` are the stages, `cnet_proj[idx](fmap1)` -> (B, 2 * context_dim, H, W), split in halves into net / inp,
    `fusion_blocks[idx-1]([previous_feat, feat])` —, or `patch_coarse2fine(model)` adopts them from a reference instance."""

    def __init__(self, iters: int = 12, hidden_dim: int = 128, context_dim: int = 128, corr_levels: int = 1, corr_radius: int = 4,
                 num_groups: int = 4, weights: Optional[str] = None, strict_load: bool = True, fused_loop: bool = True,
                 arithmetic: str = "fp16x2", outputs: str = "all", **kwargs):
        super().__init__()
        assert corr_levels == 1, "Corr level must be 1 in Coarse2FineGroupRepViTRaftStereo"  # model.py:214
        self.arithmetic = arithmetic
        self.outputs = check_outputs(outputs)  # "last": every stage last-only, the final stage's map alone returned
        self.iters, self.hidden_dim, self.context_dim = iters, hidden_dim, context_dim
        self.corr_levels, self.corr_radius, self.num_groups = corr_levels, corr_radius, num_groups
        self.fused_loop = fused_loop
        self.fnet = self._init_fnet()
        self.cnet_proj = self._init_cnet_proj()
        self.fusion_blocks = self._init_fusion_blocks()
        self.update_block = BasicUpdateBlock(hidden_dim=hidden_dim, cor_planes=num_groups * corr_levels * (2 * corr_radius + 1),
                                             flow_channel=1, context_dim=context_dim, gru="conv_gru", spatial_scale=(4, 4),
                                             arithmetic=arithmetic)
        self.corr_fn = GroupCorrBlock1D
        self.weights, self.strict_load = weights, strict_load
        if weights is not None:
            load_weights(self, weights, strict_load)

    def _init_fnet(self) -> nn.Module:
        raise NotImplementedError("Coarse2FineRAFTStereoBase: supply the encoder (reference: nndepth.encoders.rep_vit.RepViT)")

    def _init_cnet_proj(self) -> nn.ModuleList:
        raise NotImplementedError("Coarse2FineRAFTStereoBase: supply cnet_proj (reference: three 1x1 MobileOneBlocks, model.py:216-222)")

    def _init_fusion_blocks(self) -> nn.ModuleList:
        raise NotImplementedError("Coarse2FineRAFTStereoBase: supply fusion_blocks (reference: two FeatureFusionBlocks, model.py:223-228)")

    def convex_upsample(self, flow, mask, rate=(4, 4)):
        rate = rate if isinstance(rate, int) else rate[0]
        return convex_upsample(flow, mask, rate)

    def initialize_coords(self, fmap1):
        B, _, H, W = fmap1.shape
        return torch.arange(W, device=fmap1.device).float()[None, None, None, :].repeat(B, 1, H, 1)

    def forward_features(self, frame1: torch.Tensor, frame2: torch.Tensor):
        """Encoder side (PyTorch-ROCm): per stage the fused feature map of both frames (2B, C, H, W) and cnet (model.py:275-288)."""
        B = frame1.shape[0]
        features = self.fnet(torch.cat([frame1, frame2], dim=0))[::2][::-1]
        feats, cnets, previous = [], [], None
        for idx, feat in enumerate(features):
            if previous is not None:
                feat = self.fusion_blocks[idx - 1]([previous, feat])
            feats.append(feat)
            cnets.append(self.cnet_proj[idx](feat[:B].clone()))
            previous = feat
        return feats, cnets

    def forward(self, frame1: torch.Tensor, frame2: torch.Tensor, **kwargs) -> List[Dict[str, torch.Tensor]]:
        require_eval(self)
        with torch.no_grad():
            return self._forward_calibrated(frame1, frame2)

    def _forward(self, frame1: torch.Tensor, frame2: torch.Tensor) -> List[Dict[str, torch.Tensor]]:
        feats, cnets = self.forward_features(frame1, frame2)
        return self.refine_stages(feats, cnets, tuple(frame1.shape[-2:]))

    def refine_stages(self, feats, cnets, frame_hw) -> List[Dict[str, torch.Tensor]]:
        """The cascade behind the encoder side (model.py:280-320): HIP kernels only.  outputs="last": every stage computes its last
        upsampled map alone (it seeds the next stage) and only the final stage's is returned."""
        B = feats[0].shape[0] // 2
        last = last_only(self)
        outs: List[Dict[str, torch.Tensor]] = []
        up_last = None
        for idx, feat in enumerate(feats):
            fmap1, fmap2 = feat[:B].float().contiguous(), feat[B:].float().contiguous()
            cnet = cnets[idx].float()
            net, inp = ops.split_tanh_relu(cnet, cnet.shape[1] // 2)
            corr = self.corr_fn(fmap1, fmap2, self.corr_levels, self.corr_radius, self.num_groups)
            if up_last is not None and tuple(up_last.shape[-2:]) != tuple(fmap1.shape[-2:]):
                raise NndError(f"Coarse2FineRAFTStereoBase: stage {idx} is {tuple(fmap1.shape[-2:])} but the previous stage's "
                               f"upsampled disparity is {tuple(up_last.shape[-2:])} (frame size not divisible by the pyramid's strides)")
            if self.fused_loop and isinstance(corr, GroupCorrBlock1D):
                eng = self.update_block.sync_engine(fmap1.device)
                up, _, _ = eng.refine_group(corr._pyr, self.num_groups, self.corr_levels, self.corr_radius, net, inp, 4, self.iters,
                                            disp_init=up_last, keep_all=not last, last_only=last)
                ups, stacked = [up[i] for i in range(up.shape[0])], up
            else:  # seam-by-seam loop (same shape as the reference's), every step still a HIP kernel
                org = self.initialize_coords(fmap1)
                coords1 = org if up_last is None else org + up_last
                ups, stacked = [], None
                for i in range(self.iters):
                    sampled = corr(coords1)
                    net, mask, delta = self.update_block(net, inp, sampled, coords1 - org)
                    coords1 = coords1 + delta
                    if not last or i == self.iters - 1:
                        ups.append(self.convex_upsample(coords1 - org, mask, rate=(4, 4)))
            if not last or idx == len(feats) - 1:
                outs.extend({"up_disp": u} for u in frame_size_outputs(ups, tuple(frame_hw), stacked))
            up_last = ups[-1]
        return outs


class FoldedEncoderSide:
    """A whole encoder side on HIP, ONE C-ABI call per forward, exact fp32 whatever the model's `arithmetic`: `engine_cls` is
    ops.RepViTEngine (Coarse2FineGroupRepViTRAFTStereo: RepViT `fnet`, the three MobileOne `cnet_proj` blocks, the two
    FeatureFusionBlocks; csrc/repvit.hip) or ops.MobileNetV3Engine (IGEVStereoMBNet: MobileNetV3 `fnet`, `fnet_proj`, `cnet_proj`;
    csrc/mbv3.hip).  The engine is packed from the modules' train-time parameters (branches, BatchNorms and layer scales folded on
    the host in float64) and repacked when ops.ParamCache's key changes; `track_modules`: a replaced submodule is such a change."""

    def __init__(self, engine_cls, track_modules: bool = False):
        self.engine_cls, self.track_modules, self.cache = engine_cls, track_modules, ops.ParamCache()

    def run(self, owner: nn.Module, modules, frame1: torch.Tensor, frame2: torch.Tensor):
        """modules = the engine's module tuple, fnet first -> what the model's own encoder-side method returns
        (Coarse2FineRAFTStereoBase.forward_features, IGEVStereoMBNet.forward_fnet)."""
        if owner.training or modules[0].training:
            raise NndError(f"{type(owner).__name__}: the HIP encoder side is inference-only (BatchNorm is folded with its running "
                           "statistics): call model.eval() first")

        def build():  # the module walk, the descriptor and the fold: only on a key change; otherwise the key is the whole check
            why = self.engine_cls.blocker(owner, *modules)
            if why:
                raise NndError(f"{type(owner).__name__}: the HIP encoder side cannot run this model ({why}); pass hip_encoder=False "
                               "to run the encoder side's PyTorch-ROCm modules explicitly")
            return self.engine_cls.from_modules(*modules, frame1.device)
        engine = self.cache.get(modules, frame1.device, build, track_modules=self.track_modules)
        # the two frame tensors are read where they lie: no torch.cat copy
        return engine.forward(frame1.float(), frame2.float())


class Coarse2FineGroupRepViTRAFTStereo(Coarse2FineRAFTStereoBase):
    """Drop-in for the reference's `Coarse2FineGroupRepViTRAFTStereo` (nndepth/models/raft_stereo/model.py:166-320): its
    constructor kwargs (= `RepViTRAFTStereoModelConfig`, with corr_levels=1 as the reference asserts), its state_dict keys in its
    order (fnet, cnet_proj, update_block, fusion_blocks) and `forward(frame1, frame2) -> List[{"up_disp"}]`.

    hip_encoder=True (default): the whole encoder side is ONE HIP call (FoldedEncoderSide), followed by the HIP cascade of
    Coarse2FineRAFTStereoBase.refine_stages.  A configuration the HIP encoder side does not build raises NndError naming it;
    hip_encoder=False is the explicit opt-in to the containers' PyTorch-ROCm forward (nndepth_amd.rep_vit)."""

    def __init__(self, num_groups: int = 4, downsample_ratios=((2, 2), (2, 2), (2, 2), (2, 2)), ffn_exp_ratios=(1.0, 3.0, 3.0, 4.0),
                 num_blocks_per_stage=(4, 4, 6, 2), patch_size: int = 7, stem_strides=((2, 2), (2, 2), (1, 1)),
                 token_mixer_types=("repmixer", "repmixer", "repmixer", "attention"), use_ffn_per_stage=(False, True, True, True),
                 width_multipliers=(1, 1, 1, 1), weights: Optional[str] = None, strict_load: bool = True, iters: int = 12,
                 fnet_dim: int = 256, hidden_dim: int = 128, context_dim: int = 128, corr_levels: int = 1, corr_radius: int = 4,
                 tracing: bool = False, include_preprocessing: bool = False, hip_encoder: bool = True, arithmetic: str = "fp16x2",
                 outputs: str = "all", fused_loop: bool = True, **kwargs):
        self.downsample_ratios, self.ffn_exp_ratios = downsample_ratios, ffn_exp_ratios
        self.num_blocks_per_stage, self.patch_size, self.stem_strides = num_blocks_per_stage, patch_size, stem_strides
        self.token_mixer_types, self.use_ffn_per_stage, self.width_multipliers = token_mixer_types, use_ffn_per_stage, width_multipliers
        self.fnet_dim, self.tracing, self.include_preprocessing = fnet_dim, tracing, include_preprocessing
        super().__init__(iters=iters, hidden_dim=hidden_dim, context_dim=context_dim, corr_levels=corr_levels, corr_radius=corr_radius,
                         num_groups=num_groups, weights=None, fused_loop=fused_loop, arithmetic=arithmetic, outputs=outputs)
        # the reference registers fusion_blocks after update_block (model.py:216-228 run after RAFTStereo.__init__): same order here
        self._modules["fusion_blocks"] = self._modules.pop("fusion_blocks")
        self.hip_encoder = hip_encoder
        self._encoder_side = FoldedEncoderSide(ops.RepViTEngine)
        self.weights, self.strict_load = weights, strict_load
        if weights is not None:
            load_weights(self, weights, strict_load)

    def _init_fnet(self) -> nn.Module:
        from .rep_vit import RepViT
        return RepViT(downsample_ratios=self.downsample_ratios, ffn_exp_ratios=self.ffn_exp_ratios,
                      num_blocks_per_stage=self.num_blocks_per_stage, patch_size=self.patch_size, stem_strides=self.stem_strides,
                      token_mixer_types=self.token_mixer_types, use_ffn_per_stage=self.use_ffn_per_stage,
                      width_multipliers=self.width_multipliers)

    def _init_cnet_proj(self) -> nn.ModuleList:
        from .rep_vit import MobileOneBlock
        return nn.ModuleList([MobileOneBlock(c, self.context_dim * 2, kernel_size=1, stride=1, padding=0) for c in (256, 64, 64)])

    def _init_fusion_blocks(self) -> nn.ModuleList:
        from .rep_vit import FeatureFusionBlock
        return nn.ModuleList([FeatureFusionBlock(256, 64, 64, 1, 0), FeatureFusionBlock(64, 16, 64, 1, 0)])

    def forward_features(self, frame1: torch.Tensor, frame2: torch.Tensor):
        if self.hip_encoder:
            return self._encoder_side.run(self, (self.fnet, self.cnet_proj, self.fusion_blocks), frame1, frame2)
        return super().forward_features(frame1, frame2)  # explicit opt-in (hip_encoder=False): PyTorch-ROCm modules


def patch_coarse2fine(model: nn.Module, arithmetic: str = "fp16x2", fused_loop: bool = True, outputs: str = "all",
                      hip_encoder: bool = False) -> nn.Module:
    """Swap the HIP hot path into a reference `Coarse2FineGroupRepViTRAFTStereo` instance in place: `patch()` for `update_block` and
    `convex_upsample`, `corr_fn` = GroupCorrBlock1D, and `forward` = the reference's encoder side (its own fnet / fusion_blocks /
    cnet_proj modules) followed by Coarse2FineRAFTStereoBase.refine_stages.  `outputs`: as on Coarse2FineRAFTStereoBase.
    hip_encoder=True: the instance's own fnet / cnet_proj / fusion_blocks are packed and run as the ONE HIP call of the drop-in
    class (FoldedEncoderSide) instead of their PyTorch modules."""
    model.outputs = check_outputs(outputs)
    patch(model, arithmetic)
    model.corr_fn = GroupCorrBlock1D
    model.convex_upsample = lambda flow, mask, rate=(4, 4): convex_upsample(flow, mask, rate if isinstance(rate, int) else rate[0])
    model.arithmetic, model.fused_loop = arithmetic, fused_loop
    cls = Coarse2FineRAFTStereoBase
    side = FoldedEncoderSide(ops.RepViTEngine) if hip_encoder else None

    def forward(frame1, frame2, **kwargs):
        require_eval(model)
        with torch.no_grad():
            if side is not None:
                feats, cnets = side.run(model, (model.fnet, model.cnet_proj, model.fusion_blocks), frame1, frame2)
            else:
                feats, cnets = cls.forward_features(model, frame1, frame2)
            return cls.refine_stages(model, feats, cnets, tuple(frame1.shape[-2:]))

    model.forward = forward
    return model


STEREO_MODELS = {"base-raft-stereo": BaseRAFTStereo, "coarse2fine": Coarse2FineGroupRepViTRAFTStereo}


def patch(model: nn.Module, arithmetic: str = "fp16x2") -> nn.Module:
    """Swap the HIP hot path into a reference-style RAFT-Stereo instance in place:
    `corr_fn`, `update_block` (state_dict carried over) and `convex_upsample`.  `arithmetic`: as on the model classes."""
    old = model.update_block
    sd = old.state_dict()
    hid = sd["flow_head.conv1.weight"].shape[0]
    gin = sd["gru.convz1.weight"].shape[1]
    new = BasicUpdateBlock(hidden_dim=hid, cor_planes=sd["encoder.convc1.weight"].shape[1],
                           context_dim=gin - 2 * hid,
                           gru="sep_conv" if "gru.convz2.weight" in sd else "conv_gru",
                           flow_channel=sd["flow_head.conv2.weight"].shape[0],
                           spatial_scale=int(round((sd["mask.2.weight"].shape[0] // 9) ** 0.5)), arithmetic=arithmetic)
    new.load_state_dict(sd, strict=True)
    new.to(next(old.parameters()).device)
    model.update_block = new
    model.corr_fn = CorrBlock1D
    model.convex_upsample = lambda flow, mask, rate=8: convex_upsample(flow, mask, rate)
    return model


def calibrate_patched(model: nn.Module, frame1: torch.Tensor, frame2: torch.Tensor, max_passes: int = 4) -> nn.Module:
    """fp16x2 activation-range calibration of a `patch()`ed reference model on one pair (see AutoCalibrate): the reference's own
    forward runs inside `ops.calibration()`, so the seams record what they stage."""
    calibration_passes(lambda: model(frame1, frame2), max_passes, "calibrate_patched: activations still overflow fp16")
    return model
