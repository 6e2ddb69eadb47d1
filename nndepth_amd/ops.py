"""Tensor-level wrappers over the C-ABI (include/nndepth_amd.h).

PyTorch is plumbing only: it owns device memory and the HIP stream; every computation is a
call into libnndepth_amd.so.  All ops require fp32 tensors on a HIP ("cuda") device and
raise otherwise — there is no CPU or eager fallback.
"""
import contextlib
import ctypes as C
import itertools
import os
import threading
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from ._lib import (NND_FLAG_CALIBRATE, NND_FLAG_LAST_UPSAMPLE_ONLY, NND_MIDAS_KEEP_PRE, Conv3dDesc, ConvDesc, EncoderDesc, MidasDesc,
                   MobileNetV3Desc, NndError, RepViTDesc,
                   UpdateBlockDesc,
                   check, lib)


def _dev(*tensors: torch.Tensor) -> torch.device:
    d = tensors[0].device
    for t in tensors:
        if t.device.type != "cuda":
            raise NndError("nndepth_amd ops run on the HIP device only; got a tensor on "
                           f"{t.device} (no CPU fallback exists)")
        if t.dtype != torch.float32:
            raise NndError(f"nndepth_amd ops are fp32; got {t.dtype}")
        if t.device != d:
            raise NndError("all tensors must live on the same device")
    return d


def _stream(device: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _p(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _host(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.detach().to("cpu", torch.float32).contiguous()


class ParamCache:
    """"Repack when the parameters changed", once: `get` returns what `build()` made for the current key and calls it again
    only when the key changed.  The key: (data_ptr, _version) of every parameter and buffer of `modules` (an in-place edit bumps
    _version, a replaced tensor has another data_ptr), the id of every submodule with `track_modules` (a replaced block), the
    device the packed object is for, and `extra`.  A `build()` that raises leaves the cache as it was."""

    def __init__(self):
        self.key, self.value = None, None
        self.on_build: Optional[Callable[[object], None]] = None  # called with every freshly built value (a pinned calibration state)

    def get(self, modules: Sequence[torch.nn.Module], device, build: Callable[[], object], extra: tuple = (),
            track_modules: bool = False):
        mods = [s for m in modules for s in m.modules()]  # one walk: nn.Module.parameters() + buffers() would make two slower ones
        key = (tuple((t.data_ptr(), t._version) for s in mods for t in itertools.chain(s._parameters.values(), s._buffers.values())
                     if t is not None),
               tuple(map(id, mods)) if track_modules else (), str(device), extra)
        if key != self.key:
            old, self.value = self.value, build()
            if self.on_build is not None:
                try:
                    self.on_build(self.value)
                except Exception:
                    self.value = old
                    raise
            self.key = key
        return self.value


# ------------------------------------------------------------- fp16x2 activation-range calibration
# include/nndepth_amd.h "fp16x2 activation range", csrc/calib.hip.  Inside `with calibration() as c:` every engine call made by
# this thread carries NND_FLAG_CALIBRATE (the layers record the largest |activation| they stage); leaving the block fixes the
# per-layer activation scales of every engine that ran (`nnd_*_calibration_finish`, on the stream, no synchronisation) —
# reading `c.status` afterwards synchronises: bit 0 = a layer saw inf / NaN at its old scale (run the block again), bit 1 = some
# fp16x2 layer of an engine was not on the path.
_calib_tls = threading.local()
# the arithmetics whose operands are range-scaled fp16 pieces: they have a per-layer activation range to calibrate
# ("fp16x2": two pieces, fp32 to rounding level; "fp16": one piece, 11 significand bits — csrc/split_arith.h)
RANGE_SCALED = ("fp16x2", "fp16")


def arithmetic_id(name: str) -> int:
    """The descriptor value of an arithmetic name (UpdateBlockEngine.ARITHMETIC); NndError for an unknown one."""
    if name not in UpdateBlockEngine.ARITHMETIC:
        raise NndError(f"unknown arithmetic {name!r} (fp32 = exact fp32 MFMA, bf16x3 = 3-piece split on the bf16 MFMA, "
                       "fp16x2 = 2-piece range-scaled split on the fp16 MFMA, fp16 = ONE range-scaled fp16 piece: 11 significand bits, "
                       "not fp32 parity)")
    return UpdateBlockEngine.ARITHMETIC[name]


class _Calibration:
    def __init__(self):
        self.engines: List[object] = []
        self._status: Optional[torch.Tensor] = None

    def flags(self, engine) -> int:
        """Called by an engine for each C-ABI call it makes: registers the engine, returns the flag word of the descriptor."""
        if all(e is not engine for e in self.engines):
            self.engines.append(engine)
        return NND_FLAG_CALIBRATE

    @property
    def status(self) -> int:
        return 0 if self._status is None else int(self._status.item())


class NeedsCalibration(NndError):
    """Raised inside `with require_calibrated()` by an fp16x2 engine whose activation scales are still the defaults."""


def _calib_flags(engine) -> int:
    c = getattr(_calib_tls, "active", None)
    if c is not None:
        return c.flags(engine)
    if getattr(_calib_tls, "require", False) and not engine.calibrated:
        raise NeedsCalibration(f"{type(engine).__name__}: fp16x2 activation scales not calibrated")
    return 0


def _call_desc(engine, extra_flags: int = 0):
    """The descriptor of ONE C-ABI call: a copy of `engine.desc` that carries this call's flags (NND_FLAG_CALIBRATE inside
    `with calibration()` for an fp16x2 engine, plus `extra_flags`).  The engine's own descriptor is never written after
    __init__, so calls on one engine from several threads do not race on it and no flag reaches a later call."""
    d = type(engine.desc).from_buffer_copy(engine.desc)
    d.flags = (_calib_flags(engine) if engine.arithmetic in RANGE_SCALED else 0) | extra_flags
    return d


@contextlib.contextmanager
def require_calibrated():
    """Inside the block an fp16x2 engine that has not been calibrated since its parameters were packed raises NeedsCalibration
    instead of running with the default activation scales (the model classes use it to calibrate on their first forward)."""
    old = getattr(_calib_tls, "require", False)
    _calib_tls.require = True
    try:
        yield
    finally:
        _calib_tls.require = old


@contextlib.contextmanager
def calibration(finish: bool = True):
    """finish=False: the engines record under NND_FLAG_CALIBRATE but no scale is set when the block is left — the records stay
    pending in the blobs for the caller to read AND clear (`read_records`, as the model classes' `range_report` does; a single
    ops.Conv2d has no such mode, it calibrates on the spot)."""
    if getattr(_calib_tls, "active", None) is not None:
        raise NndError("calibration(): already active on this thread")
    c = _Calibration()
    _calib_tls.active = c
    try:
        yield c
    finally:
        _calib_tls.active = None
    if not finish:
        return
    for e in c.engines:
        d = e.packed.device
        if c._status is None:
            c._status = torch.zeros(1, dtype=torch.int32, device=d)
        with torch.cuda.device(d):
            e._calibration_finish(c._status)
        e.calibrated = True


# ---- activation scales as data (include/nndepth_amd.h: nnd_*_scale_slots, nnd_scales_read / nnd_scales_write)
def _enumerate_slots(call: Callable, what: str) -> List[int]:
    """The offsets of one nnd_*_scale_slots function, `call(offsets, n)`: sized with offsets = NULL, then filled.  Host work."""
    n = int(call(None, 0))
    if n < 0:
        check(n, what)
    offs = (C.c_int64 * n)()
    rc = int(call(offs, n))
    if rc < 0:
        check(rc, what)
    return list(offs)


def scales_read(packed: torch.Tensor, offsets: Sequence[int], records: bool = False, clear: bool = False):
    """(xs int32, records float32 or None) on packed's device for the slots at `offsets`: one launch, no synchronisation."""
    d = packed.device
    xs = torch.empty(len(offsets), dtype=torch.int32, device=d)
    rec = torch.empty(len(offsets), dtype=torch.float32, device=d) if records else None
    if offsets:
        with torch.cuda.device(d):
            check(lib.nnd_scales_read(_p(packed), (C.c_int64 * len(offsets))(*offsets), len(offsets), _p(xs), _p(rec), int(clear), _stream(d)),
                  "scales_read")
    return xs, rec


def scales_write(packed: torch.Tensor, offsets: Sequence[int], xs, widen: bool = False) -> None:
    """xs (ints, or an integer tensor anywhere) into the slots at `offsets`, in place; widen: the smaller of the current and the given."""
    d = packed.device
    xs = torch.as_tensor(xs).to(device=d, dtype=torch.int32).reshape(-1).contiguous()
    if xs.numel() != len(offsets):
        raise NndError(f"scales_write: {xs.numel()} exponents for {len(offsets)} layers")
    if offsets:
        with torch.cuda.device(d):
            check(lib.nnd_scales_write(_p(packed), (C.c_int64 * len(offsets))(*offsets), len(offsets), _p(xs), int(bool(widen)), _stream(d)),
                  "scales_write")


def nonfinite_flag(x: torch.Tensor, word: torch.Tensor) -> None:
    """word (1 device int32) |= 1 if x holds an inf or a NaN: one launch, no synchronisation."""
    d = _dev(x)
    if word.device != d or word.dtype != torch.int32 or word.numel() < 1:
        raise NndError(f"nonfinite_flag: the word must be a torch.int32 tensor on {d}")
    x = x.contiguous()
    if x.numel():
        with torch.cuda.device(d):
            check(lib.nnd_nonfinite_flag(_p(x), x.numel(), _p(word), _stream(d)), "nonfinite_flag")


class ScaleSlots:
    """What the four range-scaled engines share: their layers' activation scales as data.  `_scale_slots()` (host work, from the
    descriptor alone) lists (layer name, slot offset) of the layers that have a scale — none under "fp32" / "bf16x3"."""

    def _scale_slots(self) -> List[Tuple[str, int]]:
        raise NotImplementedError

    def _slots(self) -> List[Tuple[str, int]]:
        if self.__dict__.get("_slot_list") is None:
            self._slot_list = self._scale_slots()
        return self._slot_list

    def on_device(self) -> bool:
        """Packed, and on a HIP device (a blob packed on the host has its default scales and nothing to launch on)."""
        return self.packed is not None and self.packed.device.type == "cuda"

    def _blob(self) -> torch.Tensor:
        if not self.on_device():
            raise NndError(f"{type(self).__name__}: parameters not packed on a HIP device, there are no scales to read or write")
        return self.packed

    def scale_names(self) -> List[str]:
        """The layers that carry an activation scale, by name, in the order of read_scales / write_scales (no GPU needed)."""
        return [n for n, _ in self._slots()]

    def read_scales(self) -> torch.Tensor:
        """int32 device tensor, one exponent xs per scale_names() entry (the layer stages x * 2^xs).  No synchronisation."""
        return scales_read(self._blob(), [o for _, o in self._slots()])[0]

    def read_records(self, clear: bool = True) -> torch.Tensor:
        """float32 device tensor: the largest |activation| each layer staged under NND_FLAG_CALIBRATE since the last finish (0: none)."""
        return scales_read(self._blob(), [o for _, o in self._slots()], records=True, clear=clear)[1]

    def write_scales(self, xs, widen: bool = False) -> None:
        """Sets the exponents, in scale_names() order, in place (a captured graph picks them up on its next replay); widen=True
        keeps the smaller of the current and the given one per layer.  Must not overlap a forward of this engine on another stream."""
        scales_write(self._blob(), [o for _, o in self._slots()], xs, widen)
        self.calibrated = True

    def widen_scales(self, before: torch.Tensor) -> None:
        """After a new calibration: per layer the smaller of the new exponent and `before` (read_scales() taken ahead of it)."""
        self.write_scales(before, widen=True)


class ScaleSite(NamedTuple):
    """One engine of a model, as the model classes' calibration state sees it: its layer names (host work: known before anything is
    packed), the packed engine (None until then) and the ParamCache that repacks it."""
    names: List[str]
    engine: Callable[[], Optional[ScaleSlots]]
    cache: ParamCache


# ---------------------------------------------------------------------------- correlation
def pyramid_layout(B: int, H: int, W: int, num_levels: int) -> Tuple[List[int], List[int], int]:
    offs = (C.c_int64 * (num_levels + 1))()
    wid = (C.c_int32 * (num_levels + 1))()
    tot = C.c_int64()
    check(lib.nnd_corr1d_pyramid_layout(B, H, W, num_levels, offs, wid, C.byref(tot)), "corr1d_pyramid_layout")
    return list(offs), list(wid), tot.value


def corr1d_build(fmap1: torch.Tensor, fmap2: torch.Tensor, num_levels: int) -> torch.Tensor:
    """-> flat fp32 pyramid buffer (see pyramid_layout)."""
    d = _dev(fmap1, fmap2)
    if fmap1.shape != fmap2.shape or fmap1.dim() != 4:
        raise NndError(f"corr1d_build: fmap shapes {tuple(fmap1.shape)} vs {tuple(fmap2.shape)}")
    fmap1, fmap2 = fmap1.contiguous(), fmap2.contiguous()
    B, Cc, H, W = fmap1.shape
    _, _, total = pyramid_layout(B, H, W, num_levels)
    pyr = torch.empty(total, dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_corr1d_build(_p(fmap1), _p(fmap2), _p(pyr), B, Cc, H, W, num_levels, _stream(d)), "corr1d_build")
    return pyr


def corr1d_lookup(pyr: torch.Tensor, coords: torch.Tensor, num_levels: int, radius: int) -> torch.Tensor:
    d = _dev(pyr, coords)
    coords = coords.contiguous()
    B, one, H, W = coords.shape
    if one != 1:
        raise NndError("corr1d_lookup: coords must be (B,1,H,W)")
    out = torch.empty((B, num_levels * (2 * radius + 1), H, W), dtype=torch.float32, device=d)
    if out.numel() == 0:
        return out
    with torch.cuda.device(d):
        check(lib.nnd_corr1d_lookup(_p(pyr), _p(coords), _p(out), B, H, W, num_levels, radius, _stream(d)), "corr1d_lookup")
    return out


def convex_upsample(flow: torch.Tensor, mask: torch.Tensor, rate: int) -> torch.Tensor:
    d = _dev(flow, mask)
    flow, mask = flow.contiguous(), mask.contiguous()
    B, Cf, H, W = flow.shape
    if tuple(mask.shape) != (B, 9 * rate * rate, H, W):
        raise NndError(f"convex_upsample: mask shape {tuple(mask.shape)} != {(B, 9 * rate * rate, H, W)}")
    out = torch.empty((B, Cf, rate * H, rate * W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_convex_upsample(_p(flow), _p(mask), _p(out), B, Cf, H, W, rate, _stream(d)), "convex_upsample")
    return out


# ------------------------------------------------------------------------ generic conv2d
class Conv2d(ScaleSlots):
    """One packed stride-1 "same" convolution (1x1, 3x3, 1x5, 5x1): arithmetic "fp32" = the exact fp32-MFMA kernel,
    "bf16x3" = fp32 operands as 3 bf16 pieces on the bf16 MFMA (csrc/conv_split.hip, Cin % 16 == 0), "fp16x2" = as 2 range-scaled
    fp16 pieces, "fp16" = as ONE range-scaled fp16 piece: 11 significand bits per operand (not fp32 parity), finite up to 32 x the
    calibrated maximum |x| and inf / NaN beyond.  Its one activation scale is the layer "" of scale_names()."""

    def _scale_slots(self) -> List[Tuple[str, int]]:
        offs = _enumerate_slots(lambda o, n: lib.nnd_conv2d_scale_slots_ex(self.Cout, self.Cin, self.KH, self.KW, self.arith, o, n),
                                "conv2d_scale_slots")
        return [("", o) for o in offs if o >= 0]


    def __init__(self, weight: torch.Tensor, bias: torch.Tensor, device="cuda", arithmetic: str = "fp32"):
        self.Cout, self.Cin, self.KH, self.KW = (int(s) for s in weight.shape)
        self.arith = arithmetic_id(arithmetic)
        n = int(lib.nnd_conv2d_packed_floats_ex(self.Cout, self.Cin, self.KH, self.KW, self.arith))
        if n <= 0:
            check(n, "conv2d_packed_floats")
        w, b = _host(weight), _host(bias)
        blob = torch.empty(n, dtype=torch.float32)
        check(lib.nnd_conv2d_pack_ex(_p(w), _p(b), self.Cout, self.Cin, self.KH, self.KW, self.arith, _p(blob)), "conv2d_pack")
        self.packed_host = blob
        self.packed = blob.to(device) if device is not None else None
        self.calibrated = False

    def calibrate(self, x: torch.Tensor) -> "Conv2d":
        """fp16x2 / fp16: set the layer's activation scale from the largest |x| of this input (include/nndepth_amd.h
        "fp16x2 activation range"); the other arithmetics have no range to calibrate."""
        d = _dev(x, self.packed)
        x = x.contiguous()
        B, Cin, H, W = x.shape
        if Cin != self.Cin:
            raise NndError(f"conv2d: input has {Cin} channels, weights expect {self.Cin}")
        with torch.cuda.device(d):
            check(lib.nnd_conv2d_calibrate_ex(_p(self.packed), _p(x), B, Cin, H, W, self.Cout, self.KH, self.KW, self.arith, None,
                                              _stream(d)), "conv2d_calibrate")
        self.calibrated = True
        return self

    def activation_range(self) -> float:
        """Largest |x| the layer represents (fp16x2 / fp16: 65504 / its activation scale; inf otherwise)."""
        if self.arith not in (1, 2):
            return float("inf")
        ncb = (self.Cout + 31) // 32
        n = self.packed.numel()
        return 65504.0 / float(self.packed[n - 4 + 1].item()) if ncb else float("inf")

    def __call__(self, x: torch.Tensor, relu: bool = False) -> torch.Tensor:
        d = _dev(x, self.packed)
        x = x.contiguous()
        B, Cin, H, W = x.shape
        if Cin != self.Cin:
            raise NndError(f"conv2d: input has {Cin} channels, weights expect {self.Cin}")
        if self.arith in (1, 2):
            if getattr(_calib_tls, "active", None) is not None:  # inside `with calibration()`: a single layer calibrates on the spot
                self.calibrate(x)
            else:
                _calib_flags(self)  # raises inside `with require_calibrated()` if the scale is still the default
        y = torch.empty((B, self.Cout, H, W), dtype=torch.float32, device=d)
        with torch.cuda.device(d):
            check(lib.nnd_conv2d_forward_ex(_p(self.packed), _p(x), _p(y), B, Cin, H, W, self.Cout, self.KH, self.KW,
                                            int(relu), self.arith, _stream(d)), "conv2d_forward")
        return y


def conv2d_offset(conv: "Conv2d", x: torch.Tensor, rng: float) -> torch.Tensor:
    """rng * (sigmoid(conv(x)) - 0.5) * 2 in the conv's epilogue (CREStereo search offsets, cre_stereo/model.py:158-159)."""
    d = _dev(x, conv.packed)
    if conv.arith != 0:
        raise NndError("conv2d_offset: exact fp32 packing expected")
    x = x.contiguous()
    B, Cin, H, W = x.shape
    if Cin != conv.Cin:
        raise NndError(f"conv2d_offset: input has {Cin} channels, weights expect {conv.Cin}")
    y = torch.empty((B, conv.Cout, H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_conv2d_offset_forward(_p(conv.packed), _p(x), _p(y), B, Cin, H, W, conv.Cout, conv.KH, conv.KW, float(rng),
                                            _stream(d)), "conv2d_offset_forward")
    return y


def split_tanh_relu(x: torch.Tensor, c_net: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """net = tanh(x[:, :c_net]), inp = relu(x[:, c_net:]) in one kernel (raft_stereo/model.py:119-122)."""
    d = _dev(x)
    x = x.contiguous()
    B, Cc, H, W = x.shape
    if not 0 < c_net < Cc:
        raise NndError(f"split_tanh_relu: cannot split {Cc} channels at {c_net}")
    net = torch.empty((B, c_net, H, W), dtype=torch.float32, device=d)
    inp = torch.empty((B, Cc - c_net, H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_split_tanh_relu(_p(x), _p(net), _p(inp), B, c_net, Cc - c_net, H, W, _stream(d)), "split_tanh_relu")
    return net, inp


def pos_enc_sine_add(x0: torch.Tensor, x1: Optional[torch.Tensor] = None, temp_bug_fix: bool = False):
    """x + PositionEncodingSine table (nndepth/blocks/pos_enc.py:22-42, incl. its `/ d_model // 2` precedence quirk unless
    temp_bug_fix), generated on the fly by the kernel; a second map of the same shape gets the same table in the same launch."""
    d = _dev(x0) if x1 is None else _dev(x0, x1)
    x0 = x0.contiguous()
    N, Cc, H, W = x0.shape
    y0 = torch.empty_like(x0)
    y1 = None
    if x1 is not None:
        x1 = x1.contiguous()
        if tuple(x1.shape) != tuple(x0.shape):
            raise NndError(f"pos_enc_sine_add: second map {tuple(x1.shape)} != {tuple(x0.shape)}")
        y1 = torch.empty_like(x1)
    with torch.cuda.device(d):
        check(lib.nnd_pos_enc_sine_add(_p(x0), _p(x1), _p(y0), _p(y1), N, Cc, H, W, int(temp_bug_fix), _stream(d)), "pos_enc_sine_add")
    return y0 if x1 is None else (y0, y1)


def avg_pool_2x_4x(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(F.avg_pool2d(x, 2, stride=2), F.avg_pool2d(x, 4, stride=4)) in one pass (cre_stereo/model.py:154-177)."""
    d = _dev(x)
    x = x.contiguous()
    N, Cc, H, W = x.shape
    o2 = torch.empty((N, Cc, H // 2, W // 2), dtype=torch.float32, device=d)
    o4 = torch.empty((N, Cc, H // 4, W // 4), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_avg_pool_2x_4x(_p(x), _p(o2), _p(o4), N, Cc, H, W, _stream(d)), "avg_pool_2x_4x")
    return o2, o4


def resize_bilinear_ac(x: torch.Tensor, size: Tuple[int, int], mul: float = 1.0) -> torch.Tensor:
    """mul * F.interpolate(x, size, mode="bilinear", align_corners=True) (cre_stereo/model.py:235-241)."""
    d = _dev(x)
    x = x.contiguous()
    N, Cc, h, w = x.shape
    H, W = int(size[0]), int(size[1])
    y = torch.empty((N, Cc, H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_resize_bilinear_ac(_p(x), _p(y), N, Cc, h, w, H, W, float(mul), _stream(d)), "resize_bilinear_ac")
    return y


def resize_nearest_scaled(x: torch.Tensor, size: Tuple[int, int], mul: float = 1.0) -> torch.Tensor:
    """mul * F.interpolate(x, size) (nearest) of a stack of single-channel maps (..., 1, h, w) -> (..., 1, H, W), integer ratios in
    both axes (raft_stereo/model.py:309-314: the Coarse2Fine stage outputs at frame size); bit-identical to the PyTorch expression."""
    d = _dev(x)
    x = x.contiguous()
    if x.dim() < 3 or x.shape[-3] != 1:
        raise NndError(f"resize_nearest_scaled: single-channel maps (..., 1, h, w) expected, got {tuple(x.shape)}")
    h, w = x.shape[-2:]
    H, W = int(size[0]), int(size[1])
    y = torch.empty(tuple(x.shape[:-2]) + (H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_resize_nearest_scaled(_p(x), _p(y), x.numel() // (h * w), h, w, H, W, float(mul), _stream(d)),
              "resize_nearest_scaled")
    return y


def mask_upsample(conv: "Conv2d", x: torch.Tensor, flow: torch.Tensor, rate: int) -> torch.Tensor:
    """convex_upsample(flow, 0.25 * conv1x1(x)) in one kernel; `conv` = Conv2d packed from mask.2's (9r^2,Cin,1,1)."""
    d = _dev(x, flow, conv.packed)
    x, flow = x.contiguous(), flow.contiguous()
    B, Cin, H, W = x.shape
    out = torch.empty((B, 1, rate * H, rate * W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_mask_upsample_forward(_p(conv.packed), _p(x), _p(flow), _p(out), B, Cin, H, W, rate, _stream(d)),
              "mask_upsample_forward")
    return out


# --------------------------------------------------------------------------- update block
# order of the reference module's state_dict (nndepth/blocks/update_block.py:39-55,68-101)
def update_block_keys(gru: str = "sep_conv") -> List[str]:
    names = ["encoder.convc1", "encoder.convc2", "encoder.convf1", "encoder.convf2", "encoder.conv",
             "gru.convz1", "gru.convr1", "gru.convq1"]
    if gru == "sep_conv":
        names += ["gru.convz2", "gru.convr2", "gru.convq2"]
    names += ["flow_head.conv1", "flow_head.conv2", "mask.0", "mask.2"]
    return [f"{n}.{s}" for n in names for s in ("weight", "bias")]


class _RefineCall(NamedTuple):
    """UpdateBlockEngine._refine_call: what a refine loop's C-ABI call line needs."""
    desc: UpdateBlockDesc
    d: torch.device
    net: torch.Tensor
    inp: torch.Tensor
    init: Optional[torch.Tensor]
    up: torch.Tensor
    stride: int
    low: torch.Tensor
    net_out: torch.Tensor
    ws: torch.Tensor
    B: int
    H: int
    W: int


class UpdateBlockEngine(ScaleSlots):
    """Packed parameters + workspace for one BasicUpdateBlock configuration."""

    def _scale_slots(self) -> List[Tuple[str, int]]:
        offs = _enumerate_slots(lambda o, n: lib.nnd_update_block_scale_slots(C.byref(self.desc), o, n), "update_block_scale_slots")
        out, seen = [], set()
        for i, o in enumerate(offs):
            if o >= 0 and o not in seen:  # conv_gru has one pass: the slots of pass 2 are those of pass 1 again
                seen.add(o)
                out.append((lib.nnd_conv_name(C.byref(self.desc), i).decode() or f"conv{i}", o))
        return out

    # "fp16": ONE range-scaled fp16 piece per operand (11 significand bits: above the bf16 autocast the reference validates under,
    # below fp32 parity; finite up to 32 x the calibrated maximum, inf / NaN beyond) — opt-in, never a default
    ARITHMETIC = {"fp32": 0, "bf16x3": 3, "fp16x2": 2, "fp16": 1}

    def __init__(self, hidden_dim: int, context_dim: int, cor_planes: int, flow_channels: int,
                 mask_channels: int, gru: str = "sep_conv", arithmetic: str = "fp32"):
        if gru not in ("sep_conv", "conv_gru"):
            raise NndError(f"unknown gru kind {gru!r}")
        arithmetic_id(arithmetic)  # refuses an unknown name
        self.gru = gru
        self.arithmetic = arithmetic
        # split_layers: diagnostic subset of the convolutions that take the split arithmetic (bit = index in conv_names();
        # part of the blob layout, so it lives in the descriptor) — NND_SPLIT_MASK is read here, once, by the bisecting scripts
        self.desc = UpdateBlockDesc(hidden_dim, context_dim, cor_planes, flow_channels, mask_channels,
                                    0 if gru == "sep_conv" else 1, self.ARITHMETIC[arithmetic],
                                    int(os.environ.get("NND_SPLIT_MASK", "0"), 0) & 0x7fffffff, 0)
        self.calibrated = False
        n = lib.nnd_update_block_packed_floats(C.byref(self.desc))
        if n <= 0:
            check(int(n), "update_block_packed_floats")
        self.packed_floats = int(n)
        self.packed: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None

    # ---- parameters
    def pack_host(self, state: dict, prefix: str = "") -> torch.Tensor:
        """state: {key: tensor}; returns the packed CPU blob (pure host work, no GPU)."""
        keys = update_block_keys(self.gru)
        assert len(keys) == lib.nnd_update_block_num_tensors(C.byref(self.desc))
        hold = [state[prefix + k].detach().to("cpu", torch.float32).contiguous() for k in keys]
        ptrs = (C.c_void_p * len(hold))(*[t.data_ptr() for t in hold])
        out = torch.empty(self.packed_floats, dtype=torch.float32)
        check(lib.nnd_update_block_pack(C.byref(self.desc), ptrs, _p(out)), "update_block_pack")
        return out

    def load(self, state: dict, prefix: str = "", device="cuda") -> "UpdateBlockEngine":
        self.packed = self.pack_host(state, prefix).to(device)
        self.calibrated = False  # a fresh blob carries the default activation scales
        return self

    # ---- fp16x2 activation range (include/nndepth_amd.h "fp16x2 activation range")
    @staticmethod
    def _keep_all(keep_all: Optional[bool], last_only: bool) -> bool:
        """keep_all=None (default): every iteration's map unless last_only."""
        if last_only and keep_all:
            raise NndError("refine: last_only=True computes one upsampled map; it cannot be combined with keep_all=True")
        return (not last_only) if keep_all is None else bool(keep_all)

    def _calibration_finish(self, status: Optional[torch.Tensor]) -> None:
        check(lib.nnd_update_block_calibration_finish(C.byref(self.desc), _p(self.packed), _p(status), _stream(self.packed.device)),
              "update_block_calibration_finish")

    def activation_ranges(self) -> Dict[str, float]:
        """{convolution: largest |activation| its fp16x2 operands represent} (65504 / the layer's activation scale)."""
        n = int(lib.nnd_update_block_scale_slots(C.byref(self.desc), None, 0))
        offs = (C.c_int64 * n)()
        check(min(0, int(lib.nnd_update_block_scale_slots(C.byref(self.desc), offs, n))), "update_block_scale_slots")
        blob = self.packed.cpu() if self.packed is not None else None
        out = {}
        for i in range(n):
            if offs[i] >= 0 and blob is not None:
                name = lib.nnd_conv_name(C.byref(self.desc), i).decode()
                if self.gru != "sep_conv" and ("convz2+convr2" in name or "convq2" in name):
                    continue  # conv_gru has one pass: these slots alias the layers of pass 1
                out[name or f"conv{i}"] = 65504.0 / float(blob[offs[i] + 1])
        return out

    # ---- workspace
    def workspace(self, B: int, H: int, W: int, device) -> torch.Tensor:
        n = int(lib.nnd_update_block_workspace_floats(C.byref(self.desc), B, H, W))
        if n <= 0:
            check(n, "update_block_workspace_floats")
        if self._ws is None or self._ws.numel() < n or self._ws.device != torch.device(device):
            self._ws = torch.empty(n, dtype=torch.float32, device=device)
        return self._ws

    def _check_state(self, what: str, net, inp, init, init_channels: int):
        """Shapes the C-ABI cannot see (it receives raw pointers): a wrong one would be an out-of-bounds device access."""
        ds = self.desc
        B, _, H, W = net.shape
        if tuple(net.shape) != (B, ds.hidden_dim, H, W):
            raise NndError(f"{what}: net shape {tuple(net.shape)} != {(B, ds.hidden_dim, H, W)}")
        if tuple(inp.shape) != (B, ds.context_dim, H, W):
            raise NndError(f"{what}: inp shape {tuple(inp.shape)} != {(B, ds.context_dim, H, W)}")
        if init is not None and tuple(init.shape) != (B, init_channels, H, W):
            raise NndError(f"{what}: initial disparity / flow shape {tuple(init.shape)} != {(B, init_channels, H, W)}")

    # ---- ops
    def forward(self, net, inp, corr, flow, want_mask: bool = True):
        if self.packed is None:
            raise NndError("UpdateBlockEngine: parameters not loaded")
        d = _dev(net, inp, corr, flow, self.packed)
        net, inp, corr, flow = (t.contiguous() for t in (net, inp, corr, flow))
        B, _, H, W = net.shape
        ds = self.desc
        exp = {"net": (B, ds.hidden_dim, H, W), "inp": (B, ds.context_dim, H, W),
               "corr": (B, ds.cor_planes, H, W), "flow": (B, ds.flow_channels, H, W)}
        for name, t in (("net", net), ("inp", inp), ("corr", corr), ("flow", flow)):
            if tuple(t.shape) != exp[name]:
                raise NndError(f"update_block: {name} shape {tuple(t.shape)} != {exp[name]}")
        net_out = torch.empty_like(net)
        mask = torch.empty((B, ds.mask_channels, H, W), dtype=torch.float32, device=d) if want_mask else None
        delta = torch.empty_like(flow)
        ws = self.workspace(B, H, W, d)
        with torch.cuda.device(d):
            check(lib.nnd_update_block_forward(C.byref(_call_desc(self)), _p(self.packed), _p(net), _p(inp), _p(corr), _p(flow),
                                               _p(net_out), _p(mask), _p(delta), _p(ws), B, H, W, _stream(d)),
                  "update_block_forward")
        return net_out, mask, delta

    def _refine_call(self, what: str, tensors, net, inp, init, channels: int, rate: int, iters: int,
                     keep_all: Optional[bool], last_only: bool) -> "_RefineCall":
        """What the four refine loops share in front of their C-ABI call: the argument checks that precede any launch, this call's
        descriptor, and the outputs (`channels` = 1 disparity, 2 CREStereo flow).  `tensors`: the loop's own device inputs."""
        if self.packed is None:
            raise NndError("UpdateBlockEngine: parameters not loaded")
        keep_all = self._keep_all(keep_all, last_only)
        desc = _call_desc(self, NND_FLAG_LAST_UPSAMPLE_ONLY if last_only else 0)  # (update_block_forward refuses that flag)
        d = _dev(*tensors, net, inp, self.packed)
        net, inp = net.contiguous(), inp.contiguous()
        B, _, H, W = net.shape
        self._check_state(what, net, inp, init, channels)
        if init is not None:
            _dev(init)
            init = init.contiguous()
        up = torch.empty((iters if keep_all else 1, B, channels, rate * H, rate * W), dtype=torch.float32, device=d)
        low = torch.empty((B, channels, H, W), dtype=torch.float32, device=d)
        return _RefineCall(desc, d, net, inp, init, up, up[0].numel() if keep_all else 0, low, torch.empty_like(net),
                           self.workspace(B, H, W, d), B, H, W)

    def refine(self, pyr, num_levels: int, radius: int, net, inp, rate: int, iters: int,
               disp_init=None, keep_all: Optional[bool] = None, last_only: bool = False):
        """Fused loop -> (up (iters or 1, B,1,rate*H,rate*W), low (B,1,H,W), net (B,hid,H,W)).
        keep_all (default unless last_only): every iteration's upsampled map; False: the last one, all of them computed.
        last_only: the last iteration's map alone is computed (NND_FLAG_LAST_UPSAMPLE_ONLY), the same bits as keep_all's up[-1]."""
        c = self._refine_call("refine", (pyr,), net, inp, disp_init, 1, rate, iters, keep_all, last_only)
        B, H, W = c.B, c.H, c.W
        if pyr.numel() != pyramid_layout(B, H, W, num_levels)[2]:
            raise NndError(f"refine: pyramid holds {pyr.numel()} floats, a {B}x{H}x{W} pyramid of {num_levels} levels has "
                           f"{pyramid_layout(B, H, W, num_levels)[2]}")
        with torch.cuda.device(c.d):
            check(lib.nnd_raft_stereo_refine(C.byref(c.desc), _p(self.packed), _p(pyr), num_levels, radius,
                                             _p(c.net), _p(c.inp), _p(c.init), _p(c.up), c.stride, _p(c.low), _p(c.net_out),
                                             _p(c.ws), B, H, W, rate, iters, _stream(c.d)), "raft_stereo_refine")
        return c.up, c.low, c.net_out

    def refine_group(self, group_pyr, num_groups: int, num_levels: int, radius: int, net, inp, rate: int, iters: int,
                     disp_init=None, keep_all: Optional[bool] = None, last_only: bool = False):
        """One cascade stage of Coarse2FineGroupRepViTRAFTStereo (raft_stereo/model.py:297-311): refine() with GroupCorrBlock1D's
        lookup over the pyramid of raft_group_corr_build -> (up, low, net)."""
        c = self._refine_call("refine_group", (group_pyr,), net, inp, disp_init, 1, rate, iters, keep_all, last_only)
        B, H, W = c.B, c.H, c.W
        need = pyramid_layout(B * num_groups, H, W, num_levels)[2]
        if group_pyr.numel() != need:
            raise NndError(f"refine_group: pyramid holds {group_pyr.numel()} floats, expected {need} for B*G={B * num_groups}, "
                           f"{H}x{W}, {num_levels} levels")
        with torch.cuda.device(c.d):
            check(lib.nnd_raft_stereo_group_refine(C.byref(c.desc), _p(self.packed), _p(group_pyr), num_groups, num_levels, radius,
                                                   _p(c.net), _p(c.inp), _p(c.init), _p(c.up), c.stride, _p(c.low), _p(c.net_out),
                                                   _p(c.ws), B, H, W, rate, iters, _stream(c.d)), "raft_stereo_group_refine")
        return c.up, c.low, c.net_out

    def refine_igev(self, feat_pyr, geo_pyr, num_groups: int, num_levels: int, radius: int, net, inp, rate: int,
                    iters: int, disp_init=None, keep_all: Optional[bool] = None, interleaved=None, last_only: bool = False):
        """IGEV loop (absolute coordinates, combined lookup) -> (up, low, net) like refine().
        interleaved: optional igev_interleave_pyramids(feat_pyr, geo_pyr, ...) — the loop then gathers from it."""
        c = self._refine_call("refine_igev", (feat_pyr, geo_pyr), net, inp, disp_init, 1, rate, iters, keep_all, last_only)
        B, H, W = c.B, c.H, c.W
        need = pyramid_layout(B * num_groups, H, W, num_levels)[2]
        if feat_pyr.numel() != need or geo_pyr.numel() != need:
            raise NndError(f"refine_igev: pyramids hold {feat_pyr.numel()} / {geo_pyr.numel()} floats, expected {need} "
                           f"for B*G={B * num_groups}, {H}x{W}, {num_levels} levels")
        if interleaved is not None:
            _dev(interleaved)
            need_il = int(lib.nnd_igev_interleaved_floats(B, num_groups, H, W, num_levels))
            if interleaved.numel() != need_il:
                raise NndError(f"refine_igev: interleaved copy holds {interleaved.numel()} floats, expected {need_il}")
        with torch.cuda.device(c.d):
            check(lib.nnd_igev_stereo_refine(C.byref(c.desc), _p(self.packed), _p(feat_pyr), _p(geo_pyr), _p(interleaved), num_groups,
                                             num_levels, radius, _p(c.net), _p(c.inp), _p(c.init), _p(c.up), c.stride, _p(c.low),
                                             _p(c.net_out), _p(c.ws), B, H, W, rate, iters, _stream(c.d)), "igev_stereo_refine")
        return c.up, c.low, c.net_out

    def refine_cre(self, fmap1, fmap2, net, inp, rate: int, iters: int, flow_init=None, extra_offset=None,
                   scratch=None, keep_all: Optional[bool] = None, last_only: bool = False):
        """One CREStereo cascade stage (AGCL -> update block -> flow += delta -> 2-channel upsample, `iters` times)
        -> (up (iters or 1, B,2,rate*H,rate*W), flow (B,2,H,W), net).  extra_offset=None: iter mode.
        scratch: optional caller-owned buffer, handed to the library as it is when it holds at least B*C*H*W floats (offset mode:
        below 2*B*C*H*W floats the library then takes the planar kernel); None: allocated here, 2*B*C*H*W floats in offset mode."""
        c = self._refine_call("refine_cre", (fmap1, fmap2), net, inp, flow_init, 2, rate, iters, keep_all, last_only)
        B, H, W = c.B, c.H, c.W
        fmap1, fmap2 = fmap1.contiguous(), fmap2.contiguous()
        Cf = fmap1.shape[1]
        if fmap2.shape != fmap1.shape or tuple(fmap1.shape) != (B, Cf, H, W):
            raise NndError(f"refine_cre: shapes fmap {tuple(fmap1.shape)} / {tuple(fmap2.shape)}, net {tuple(net.shape)}")
        if extra_offset is not None and extra_offset.numel() != B * 18 * H * W:
            raise NndError(f"refine_cre: extra_offset shape {tuple(extra_offset.shape)} != {(B, 18, H, W)}")
        if extra_offset is not None:
            extra_offset = extra_offset.contiguous()
            _dev(extra_offset)
        if scratch is None or scratch.numel() < fmap2.numel():
            need = fmap2.numel() if extra_offset is None else 2 * fmap2.numel()  # warped map / the two channels-last copies
            scratch = torch.empty(need, dtype=torch.float32, device=c.d)
        else:
            _dev(fmap2, scratch)
            if not scratch.is_contiguous():
                raise NndError("refine_cre: `scratch` must be contiguous")
        with torch.cuda.device(c.d):
            check(lib.nnd_cre_stereo_refine(C.byref(c.desc), _p(self.packed), _p(fmap1), _p(fmap2), Cf, _p(extra_offset),
                                            _p(scratch), scratch.numel(), _p(c.net), _p(c.inp), _p(c.init), _p(c.up), c.stride,
                                            _p(c.low), _p(c.net_out), _p(c.ws), B, H, W, rate, iters, _stream(c.d)), "cre_stereo_refine")
        return c.up, c.low, c.net_out

    # ---- profiling (bench.py roofline)
    def conv_names(self) -> List[str]:
        n = lib.nnd_num_convs(C.byref(self.desc))
        names = [lib.nnd_conv_name(C.byref(self.desc), i).decode() for i in range(n)]
        if self.gru != "sep_conv":
            names = [x for x in names if not x.endswith("2+convr2") and not x.endswith("convq2")]
        return names

    def profile_conv(self, which: int, B: int, H: int, W: int, reps: int, device) -> Tuple[float, float]:
        """-> (avg ms per launch measured with hipEvents on the launch stream, algorithmic FLOPs)."""
        ws = self.workspace(B, H, W, device)
        ms, fl = C.c_float(), C.c_double()
        d = torch.device(device)
        with torch.cuda.device(d):
            check(lib.nnd_profile_conv(C.byref(self.desc), _p(self.packed), _p(ws), B, H, W, which, reps, _stream(d),
                                       C.byref(ms), C.byref(fl)), "profile_conv")
        return ms.value, fl.value


    def profile_loop_conv(self, which: int, pyr, num_levels: int, radius: int, net, inp, rate: int, iters: int,
                          event_pair_only: bool = False) -> float:
        """-> avg ms of conv `which` INSIDE the fused RAFT-Stereo loop (hipEvents on the launch stream in every iteration).
        event_pair_only: the calibration run — both events in front of the conv, nothing between them."""
        d = _dev(pyr, net, inp, self.packed)
        net, inp = net.contiguous(), inp.contiguous()
        B, _, H, W = net.shape
        self._check_state("profile_loop_conv", net, inp, None, 1)
        up = torch.empty((B, 1, rate * H, rate * W), dtype=torch.float32, device=d)
        ws = self.workspace(B, H, W, d)
        ms = C.c_float()
        with torch.cuda.device(d):
            fn = lib.nnd_profile_loop_event_pair if event_pair_only else lib.nnd_profile_loop_conv
            check(fn(C.byref(self.desc), _p(self.packed), _p(pyr), num_levels, radius, _p(net), _p(inp),
                     _p(up), _p(ws), B, H, W, rate, iters, which, _stream(d), C.byref(ms)), "profile_loop_conv")
        return ms.value


# ------------------------------------------------------------------ IGEV geometry-encoding volume
def group_corr_build(fmap1: torch.Tensor, fmap2: torch.Tensor, num_groups: int, group_channels: int,
                     num_levels: int, pooled: bool = True) -> torch.Tensor:
    """Group-wise 1-D correlation pyramid; layout = pyramid_layout(B*num_groups, H, W, num_levels).
    pooled=False: the buffer has that layout but only level 0 is written (pyramid_pool_levels_ fills the rest on demand)."""
    d = _dev(fmap1, fmap2)
    fmap1, fmap2 = fmap1.contiguous(), fmap2.contiguous()
    B, Ctot, H, W = fmap1.shape
    _, _, total = pyramid_layout(B * num_groups, H, W, num_levels)
    pyr = torch.empty(total, dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_group_corr_build(_p(fmap1), _p(fmap2), _p(pyr), B, Ctot, H, W, num_groups, group_channels,
                                       num_levels if pooled else 0, _stream(d)), "group_corr_build")
    return pyr


def raft_group_corr_build(fmap1: torch.Tensor, fmap2: torch.Tensor, num_groups: int, num_levels: int) -> torch.Tensor:
    """GroupCorrBlock1D.corr + pyramid (raft_stereo/cost_volume.py:84-92,115-128): the first num_groups chunks of num_groups channels,
    divided by sqrt(C_total) (Q4); rows ordered (b,g,h,w1); layout = pyramid_layout(B*num_groups, H, W, num_levels)."""
    d = _dev(fmap1, fmap2)
    fmap1, fmap2 = fmap1.contiguous(), fmap2.contiguous()
    B, Ctot, H, W = fmap1.shape
    if num_groups * num_groups > Ctot:
        raise NndError(f"raft_group_corr_build: {num_groups} chunks of {num_groups} channels exceed the {Ctot} channels of the maps")
    _, _, total = pyramid_layout(B * num_groups, H, W, num_levels)
    pyr = torch.empty(total, dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_group_corr_build_scaled(_p(fmap1), _p(fmap2), _p(pyr), B, Ctot, H, W, num_groups, num_groups, num_levels,
                                              float(Ctot) ** 0.5, _stream(d)), "group_corr_build_scaled")
    return pyr


def group_corr1d_lookup(pyr: torch.Tensor, coords: torch.Tensor, num_groups: int, num_levels: int, radius: int) -> torch.Tensor:
    """GroupCorrBlock1D.__call__ (raft_stereo/cost_volume.py:94-113, view without the group permute included) ->
    (B, num_levels*num_groups*(2r+1), H, W)."""
    d = _dev(pyr, coords)
    coords = coords.contiguous()
    B, one, H, W = coords.shape
    if one != 1:
        raise NndError("group_corr1d_lookup: coords must be (B,1,H,W)")
    if pyr.numel() != pyramid_layout(B * num_groups, H, W, num_levels)[2]:
        raise NndError(f"group_corr1d_lookup: pyramid holds {pyr.numel()} floats, expected "
                       f"{pyramid_layout(B * num_groups, H, W, num_levels)[2]} for B*G={B * num_groups}, {H}x{W}, {num_levels} levels")
    out = torch.empty((B, num_levels * num_groups * (2 * radius + 1), H, W), dtype=torch.float32, device=d)
    if out.numel() == 0:
        return out
    with torch.cuda.device(d):
        check(lib.nnd_group_corr1d_lookup(_p(pyr), _p(coords), _p(out), B, num_groups, H, W, num_levels, radius, _stream(d)),
              "group_corr1d_lookup")
    return out


def pyramid_from_level0(level0: torch.Tensor, B: int, H: int, W: int, num_levels: int) -> torch.Tensor:
    """level0: (B*H*W, W) rows -> full avg-pool pyramid buffer (levels 1..num_levels built on the device)."""
    d = _dev(level0)
    offs, widths, total = pyramid_layout(B, H, W, num_levels)
    pyr = torch.empty(total, dtype=torch.float32, device=d)
    pyr[:B * H * W * W].copy_(level0.reshape(-1))
    with torch.cuda.device(d):
        check(lib.nnd_pyramid_from_level0(_p(pyr), B, H, W, num_levels, _stream(d)), "pyramid_from_level0")
    return pyr


def pyramid_pool_levels_(pyr: torch.Tensor, B: int, H: int, W: int, num_levels: int) -> torch.Tensor:
    """Levels 1..num_levels of a pyramid buffer whose level 0 is already in place (in-place variant of pyramid_from_level0)."""
    d = _dev(pyr)
    with torch.cuda.device(d):
        check(lib.nnd_pyramid_from_level0(_p(pyr), B, H, W, num_levels, _stream(d)), "pyramid_from_level0")
    return pyr


def igev_lookup(feat_pyr: torch.Tensor, geo_pyr: torch.Tensor, coords: torch.Tensor, num_groups: int,
                num_levels: int, radius: int) -> torch.Tensor:
    d = _dev(feat_pyr, geo_pyr, coords)
    coords = coords.contiguous()
    B, one, H, W = coords.shape
    out = torch.empty((B, num_levels * 2 * num_groups * (2 * radius + 1), H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_igev_lookup(_p(feat_pyr), _p(geo_pyr), _p(coords), _p(out), B, num_groups, H, W, num_levels,
                                  radius, _stream(d)), "igev_lookup")
    return out


def igev_interleave_pyramids(feat_pyr: torch.Tensor, geo_pyr: torch.Tensor, B: int, num_groups: int, H: int, W: int,
                             num_levels: int) -> torch.Tensor:
    """Group-interleaved copy of both pyramids (levels 0..num_levels-1) for the refinement loop's gathers."""
    d = _dev(feat_pyr, geo_pyr)
    out = torch.empty(lib.nnd_igev_interleaved_floats(B, num_groups, H, W, num_levels), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_igev_interleave_pyramids(_p(feat_pyr), _p(geo_pyr), _p(out), B, num_groups, H, W, num_levels,
                                               _stream(d)), "igev_interleave_pyramids")
    return out


def igev_refine_reads_interleaved(num_groups: int, num_levels: int, radius: int) -> bool:
    """True when nnd_igev_stereo_refine, given an interleaved copy, never reads the plain pyramids (their pooled levels
    need not exist)."""
    return bool(lib.nnd_igev_refine_reads_interleaved(num_groups, num_levels, radius))


def igev_interleave_level0_supported(num_groups: int, W: int, num_levels: int) -> bool:
    return bool(lib.nnd_igev_interleave_level0_supported(num_groups, W, num_levels))


def igev_interleave_level0(feat_level0: torch.Tensor, geo_level0: torch.Tensor, B: int, num_groups: int, H: int, W: int,
                           num_levels: int) -> torch.Tensor:
    """The interleaved levels 0..num_levels-1 from the two level-0 volumes (pooling in LDS; same values as pooling both
    pyramids and igev_interleave_pyramids).  The tensors may be whole pyramid buffers: only their level 0 is read."""
    d = _dev(feat_level0, geo_level0)
    n0 = B * num_groups * H * W * W
    assert feat_level0.numel() >= n0 and geo_level0.numel() >= n0 and feat_level0.is_contiguous() and geo_level0.is_contiguous()
    out = torch.empty(lib.nnd_igev_interleaved_floats(B, num_groups, H, W, num_levels), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_igev_interleave_level0(_p(feat_level0), _p(geo_level0), _p(out), B, num_groups, H, W, num_levels,
                                             _stream(d)), "igev_interleave_level0")
    return out


# ------------------------------------------------------------------ CREStereo AGCL (include/nndepth_amd.h)
def bilinear_sample(img: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
    """img (N,C,H,W), coords (N,Hg,Wg,2) pixel (x,y) -> (N,C,Hg,Wg); zero outside (cre_stereo/utils.py:5-20)."""
    d = _dev(img, coords)
    img, coords = img.contiguous(), coords.contiguous()
    N, C, H, W = img.shape
    if coords.dim() != 4 or coords.shape[0] != N or coords.shape[3] != 2:
        raise NndError(f"bilinear_sample: coords {tuple(coords.shape)} must be (N={N}, Hg, Wg, 2)")
    Hg, Wg = coords.shape[1], coords.shape[2]
    out = torch.empty((N, C, Hg, Wg), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_bilinear_sample(_p(img), _p(coords), _p(out), N, C, H, W, Hg, Wg, _stream(d)), "bilinear_sample")
    return out


def agcl_corr_iter(fmap1: torch.Tensor, fmap2: torch.Tensor, flow: torch.Tensor, small_patch: bool,
                   scratch: torch.Tensor = None) -> torch.Tensor:
    """cre_stereo/cost_volume.py:51-79.  scratch: optional (N,C,H,W) buffer for the warped right features."""
    d = _dev(fmap1, fmap2, flow)
    fmap1, fmap2, flow = fmap1.contiguous(), fmap2.contiguous(), flow.contiguous()
    N, C, H, W = fmap1.shape
    if fmap2.shape != fmap1.shape or tuple(flow.shape) != (N, 2, H, W):
        raise NndError(f"agcl_corr_iter: shapes {tuple(fmap1.shape)}, {tuple(fmap2.shape)}, flow {tuple(flow.shape)}")
    if scratch is None or scratch.numel() < fmap2.numel():
        scratch = torch.empty_like(fmap2)
    out = torch.empty((N, 36, H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_agcl_corr_iter(_p(fmap1), _p(fmap2), _p(flow), _p(scratch), _p(out), N, C, H, W,
                                     int(bool(small_patch)), _stream(d)), "agcl_corr_iter")
    return out


def nchw_to_nhwc(x: torch.Tensor) -> torch.Tensor:
    """(N,C,H,W) -> contiguous (N,H,W,C) copy (the channels-last maps of agcl_corr_offset)."""
    d = _dev(x)
    x = x.contiguous()
    N, C, H, W = x.shape
    out = torch.empty((N, H, W, C), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_nchw_to_nhwc(_p(x), _p(out), N, C, H, W, _stream(d)), "nchw_to_nhwc")
    return out


def agcl_corr_offset(fmap1: torch.Tensor, fmap2: torch.Tensor, flow: torch.Tensor, extra_offset: torch.Tensor,
                     small_patch: bool, channels_last: bool = False) -> torch.Tensor:
    """cre_stereo/cost_volume.py:81-154 after the optional attention.  channels_last: fmap1 / fmap2 are (N,H,W,C) copies
    made by nchw_to_nhwc (C = 256): the line-per-tap kernel."""
    d = _dev(fmap1, fmap2, flow, extra_offset)
    fmap1, fmap2, flow, extra_offset = (t.contiguous() for t in (fmap1, fmap2, flow, extra_offset))
    if channels_last:
        N, H, W, C = fmap1.shape
    else:
        N, C, H, W = fmap1.shape
    if fmap2.shape != fmap1.shape or tuple(flow.shape) != (N, 2, H, W) or extra_offset.numel() != N * 18 * H * W:
        raise NndError(f"agcl_corr_offset: shapes {tuple(fmap1.shape)}, {tuple(fmap2.shape)}, flow {tuple(flow.shape)}, "
                       f"extra_offset {tuple(extra_offset.shape)}")
    out = torch.empty((N, 36, H, W), dtype=torch.float32, device=d)
    fn = lib.nnd_agcl_corr_offset_nhwc if channels_last else lib.nnd_agcl_corr_offset
    with torch.cuda.device(d):
        check(fn(_p(fmap1), _p(fmap2), _p(flow), _p(extra_offset), _p(out), N, C, H, W, int(bool(small_patch)), _stream(d)),
              "agcl_corr_offset")
    return out


# ------------------------------------------------------------------ conv + folded norm, encoder (include/nndepth_amd.h)
def _pack_conv_norm(abi: str, desc, weight, bias, bn, eps: float, device) -> torch.Tensor:
    """One conv [+ eval-mode BatchNorm folded by the library] packed through nnd_<abi>_packed_floats / nnd_<abi>_pack -> the blob on
    `device`.  `bn` = (weight, bias, running_mean, running_var) or None."""
    n = int(getattr(lib, f"nnd_{abi}_packed_floats")(C.byref(desc)))
    if n <= 0:
        check(n, f"{abi}_packed_floats")
    host = [_host(t) for t in (weight, bias) + (tuple(bn) if bn is not None else (None,) * 4)]  # kept alive across the call
    blob = torch.empty(n, dtype=torch.float32)
    check(getattr(lib, f"nnd_{abi}_pack")(C.byref(desc), *[_p(t) for t in host], float(eps), _p(blob)), f"{abi}_pack")
    return blob.to(device)


class ConvNorm:
    """nn.Conv2d [+ BatchNorm2d(eval)] [+ ReLU] [+ residual add + ReLU] as one MFMA convolution (stride 1 or 2,
    1x1 / 3x3; 1x5 / 5x1 at stride 1).  `bn` = (weight, bias, running_mean, running_var) or None."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 1, bn=None, eps: float = 1e-5,
                 device="cuda"):
        Cout, Cin, KH, KW = (int(v) for v in weight.shape)
        self.desc = ConvDesc(Cout, Cin, KH, KW, int(stride))
        self.packed = _pack_conv_norm("conv", self.desc, weight, bias, bn, eps, device)

    def __call__(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None, relu: bool = False,
                 relu_after_residual: bool = False) -> torch.Tensor:
        d = _dev(x, self.packed)
        x = x.contiguous()
        B, Cin, H, W = x.shape
        if Cin != self.desc.Cin:
            raise NndError(f"conv: input has {Cin} channels, weights expect {self.desc.Cin}")
        st = self.desc.stride
        Ho, Wo = (H + st - 1) // st, (W + st - 1) // st
        y = torch.empty((B, self.desc.Cout, Ho, Wo), dtype=torch.float32, device=d)
        if residual is not None:
            residual = residual.contiguous()
            _dev(residual)
            if residual.shape != y.shape:
                raise NndError(f"conv: residual {tuple(residual.shape)} != output {tuple(y.shape)}")
        with torch.cuda.device(d):
            check(lib.nnd_conv_forward(C.byref(self.desc), _p(self.packed), _p(x), _p(residual), _p(y), B, H, W,
                                       int(relu), int(relu_after_residual), _stream(d)), "conv_forward")
        return y


ENCODER_BLOCKS = ("layer1.0", "layer1.1", "layer2.0", "layer2.1", "layer3.0", "layer3.1")


class EncoderEngine(ScaleSlots):
    """BasicEncoder (+ optional cnet_proj) on the HIP encoder (csrc/encoder.hip).  Parameters come from state-dict
    style mappings: `enc_sd` with the reference's BasicEncoder keys (conv1.weight, norm1.running_mean,
    layer1.0.conv1.weight, layer1.0.downsample.0.weight, layer1.0.norm3.weight, ..., conv2.bias) and, optionally,
    `cnet_sd` with `0.weight` / `0.bias` of the cnet_proj Sequential."""

    def _scale_slots(self) -> List[Tuple[str, int]]:
        offs = _enumerate_slots(lambda o, n: lib.nnd_encoder_scale_slots(C.byref(self.desc), o, n), "encoder_scale_slots")
        return [(lib.nnd_encoder_scale_name(C.byref(self.desc), i).decode(), o) for i, o in enumerate(offs) if o >= 0]

    def __init__(self, output_dim: int, norm: str = "batch", cnet_dim: int = 0, arithmetic: str = "fp32"):
        if norm not in ("batch", "none", "instance"):
            raise NndError(f"EncoderEngine: norm_fn '{norm}' is not built in HIP (batch in eval mode, instance, none)")
        self.norm = norm
        self.arithmetic = arithmetic
        self.desc = EncoderDesc(int(output_dim), {"none": 0, "batch": 1, "instance": 2}[norm], int(cnet_dim),
                                arithmetic_id(arithmetic), 0)
        self.calibrated = False
        n = int(lib.nnd_encoder_packed_floats(C.byref(self.desc)))
        if n <= 0:
            check(n, "encoder_packed_floats")
        self.packed_floats = n
        self.packed = None
        self._ws = None

    def _units(self, enc_sd, cnet_sd):
        def unit(conv: str, norm: Optional[str]):
            t = [enc_sd[conv + ".weight"], enc_sd[conv + ".bias"]]
            if norm is not None and self.norm == "batch":
                t += [enc_sd[norm + ".weight"], enc_sd[norm + ".bias"], enc_sd[norm + ".running_mean"], enc_sd[norm + ".running_var"]]
            else:
                t += [None] * 4
            return t
        units = [unit("conv1", "norm1")]
        for b in ENCODER_BLOCKS:
            units += [unit(f"{b}.conv1", f"{b}.norm1"), unit(f"{b}.conv2", f"{b}.norm2"), unit(f"{b}.downsample.0", f"{b}.norm3")]
        units.append(unit("conv2", None))
        if self.desc.cnet_dim > 0:
            units.append([cnet_sd["0.weight"], cnet_sd["0.bias"], None, None, None, None])
        return units

    def load(self, enc_sd, cnet_sd=None, eps: float = 1e-5, device="cuda") -> "EncoderEngine":
        if self.desc.cnet_dim > 0 and cnet_sd is None:
            raise NndError("EncoderEngine: cnet_dim > 0 needs the cnet_proj parameters")
        host = [_host(t) for u in self._units(enc_sd, cnet_sd) for t in u]
        n = int(lib.nnd_encoder_num_tensors(C.byref(self.desc)))
        if n != len(host):
            raise NndError(f"EncoderEngine: {len(host)} tensors, the library expects {n}")
        arr = (C.c_void_p * n)(*[0 if t is None else t.data_ptr() for t in host])
        blob = torch.empty(self.packed_floats, dtype=torch.float32)
        check(lib.nnd_encoder_pack(C.byref(self.desc), arr, float(eps), _p(blob)), "encoder_pack")
        self.packed = blob.to(device)
        self.calibrated = False
        return self

    def _calibration_finish(self, status: Optional[torch.Tensor]) -> None:
        check(lib.nnd_encoder_calibration_finish(C.byref(self.desc), _p(self.packed), _p(status), _stream(self.packed.device)),
              "encoder_calibration_finish")

    def forward(self, frames: torch.Tensor, n_cnet: int = 0, frames_b: Optional[torch.Tensor] = None):
        """frames (N,3,H,W) -> (fmap (N,output_dim,H/8,W/8), cnet (n_cnet,cnet_dim,H/8,W/8) or None).  With `frames_b` (same shape)
        the batch is [frames | frames_b] read where the two tensors lie (no torch.cat copy): fmap has 2N samples."""
        if self.packed is None:
            raise NndError("EncoderEngine: parameters not loaded")
        d = _dev(frames, self.packed)
        frames = frames.contiguous()
        N, c, H, W = frames.shape
        if c != 3:
            raise NndError(f"encoder: frames have {c} channels, expected 3")
        nsplit = N
        if frames_b is not None:
            _dev(frames_b, self.packed)
            frames_b = frames_b.contiguous()
            if tuple(frames_b.shape) != tuple(frames.shape):
                raise NndError(f"encoder: second frame tensor {tuple(frames_b.shape)} != {tuple(frames.shape)}")
            N = 2 * N
        h8, w8 = H, W
        for _ in range(3):
            h8, w8 = (h8 + 1) // 2, (w8 + 1) // 2
        fmap = torch.empty((N, self.desc.output_dim, h8, w8), dtype=torch.float32, device=d)
        cnet = torch.empty((n_cnet, self.desc.cnet_dim, h8, w8), dtype=torch.float32, device=d) if n_cnet > 0 else None
        need = int(lib.nnd_encoder_workspace_floats(C.byref(self.desc), N, H, W))
        if self._ws is None or self._ws.numel() < need or self._ws.device != d:
            self._ws = torch.empty(need, dtype=torch.float32, device=d)
        with torch.cuda.device(d):
            check(lib.nnd_encoder_forward2(C.byref(_call_desc(self)), _p(self.packed), _p(frames), _p(frames_b), nsplit, _p(fmap), _p(cnet), n_cnet,
                                           _p(self._ws), N, H, W, _stream(d)), "encoder_forward")
        return fmap, cnet


# ------------------------------------------------------------------------------------------ RepViT encoder side (Coarse2Fine)
def _d(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", torch.float64)


def _bn_affine(bn) -> Tuple[torch.Tensor, torch.Tensor]:
    """eval-mode BatchNorm as y = s * x + t (float64)."""
    s = _d(bn.weight) / torch.sqrt(_d(bn.running_var) + bn.eps)
    return s, _d(bn.bias) - _d(bn.running_mean) * s


def _fold_conv_bn(branch, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """conv (no bias) + BN -> (weight padded to k x k, bias) (conv.py:298-323, 503-522)."""
    s, t = _bn_affine(branch.bn)
    w = _d(branch.conv.weight) * s.reshape(-1, 1, 1, 1)
    p = (k - w.shape[-1]) // 2
    return torch.nn.functional.pad(w, [p, p, p, p]), t


def _identity_kernel(cin: int, groups: int, k: int) -> torch.Tensor:
    w = torch.zeros(cin, cin // groups, k, k, dtype=torch.float64)
    for i in range(cin):
        w[i, i % (cin // groups), k // 2, k // 2] = 1.0
    return w


def _fold_mobileone(m) -> Tuple[torch.Tensor, torch.Tensor]:
    """MobileOneBlock's branches (skip BN, 1x1 scale branch, conv branches) -> one conv + bias (conv.py:245-296)."""
    k, cout = m.kernel_size, m.out_channels
    w = torch.zeros(cout, m.in_channels // m.groups, k, k, dtype=torch.float64)
    b = torch.zeros(cout, dtype=torch.float64)
    if m.rbr_scale is not None:
        ws, bs = _fold_conv_bn(m.rbr_scale, k)
        w, b = w + ws, b + bs
    if m.rbr_skip is not None:
        s, t = _bn_affine(m.rbr_skip)
        w, b = w + _identity_kernel(m.in_channels, m.groups, k) * s.reshape(-1, 1, 1, 1), b + t
    if m.rbr_conv is not None:
        for br in m.rbr_conv:
            wc, bc = _fold_conv_bn(br, k)
            w, b = w + wc, b + bc
    return w, b


def _conv_wb(conv) -> Tuple[torch.Tensor, torch.Tensor]:
    b = _d(conv.bias) if conv.bias is not None else torch.zeros(conv.out_channels, dtype=torch.float64)
    return _d(conv.weight), b


def _stride1(s, what: str) -> int:
    """The reference's stride as given — an int or an (sy, sx) pair — as the one stride the HIP path builds (1 or 2), or NndError."""
    pair = tuple(s) if isinstance(s, (tuple, list)) else (s, s)
    if len(pair) != 2 or pair[0] != pair[1] or pair[0] not in (1, 2):
        raise NndError(f"RepViTEngine: {what} stride {s!r} is not built (only (1, 1) and (2, 2))")
    return int(pair[0])


def _layer(kind: str, w: torch.Tensor, b: torch.Tensor, stride: int = 1, act: str = "none", skip: bool = False, s=None) -> dict:
    """One folded layer of an encoder side: weight, bias, optional per-channel scale; k is the weight's kernel size."""
    return {"kind": kind, "w": w, "b": b, "s": s, "k": w.shape[-1], "stride": stride, "act": act, "skip": skip}


class _FoldedEngine:
    """What the three folded encoder sides share: the layers packed into one blob by the library (nnd_<abi>_num_tensors /
    _packed_floats / _pack, `_tensors` host tensors per layer: weight, bias [, scale or None]) and the cached workspace."""

    _abi: str  # "repvit" | "mbv3" | "midas"
    _tensors = 2

    def __init__(self, desc, layers: List[dict], device):
        self.desc, self.layers = desc, layers
        name, abi, tpl = type(self).__name__, self._abi, self._tensors
        n = int(getattr(lib, f"nnd_{abi}_num_tensors")(C.byref(desc)))
        if n < 0:
            check(n, f"{abi}_num_tensors")
        if n != tpl * len(layers):
            raise NndError(f"{name}: {len(layers)} layers folded, the library expects {n // tpl}")
        host = []  # kept alive across the call
        for l in layers:
            host += [None if t is None else t.float().contiguous() for t in (l["w"], l["b"], l["s"])[:tpl]]
        arr = (C.c_void_p * n)(*[0 if t is None else t.data_ptr() for t in host])
        total = int(getattr(lib, f"nnd_{abi}_packed_floats")(C.byref(desc)))
        if total <= 0:
            check(total, f"{abi}_packed_floats")
        blob = torch.empty(total, dtype=torch.float32)
        check(getattr(lib, f"nnd_{abi}_pack")(C.byref(desc), arr, _p(blob)), f"{abi}_pack")
        self.packed = blob.to(device)
        self._ws = None

    def _workspace(self, need: int, device: torch.device) -> torch.Tensor:
        """The cached workspace, grown to `need` floats (a negative `need` is the library's status: raised)."""
        if need < 0:
            check(need, f"{self._abi}_workspace_floats")
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(need, dtype=torch.float32, device=device)
        return self._ws


class RepViTEngine(_FoldedEngine):
    """The encoder side of Coarse2FineGroupRepViTRAFTStereo on the HIP path (csrc/repvit.hip, ONE call: nnd_repvit_forward), packed
    from the train-time modules of nndepth_amd.rep_vit (or of a reference instance: the same layout).  `fold(...)` turns every block
    into the plain layer chain the kernels run, in float64 on the host:
      MobileOneBlock        branches + BatchNorms -> one conv + bias (the skip BN as an identity kernel, the 1x1 scale branch padded)
      RepLargeKernelConv    the small 3x3 (conv + BN) padded into the large kernel (conv.py:456-469)
      RepTokenMixer         x + ls * (mixer(x) - norm(x)) -> ONE depthwise 3x3: id + ls * (W_mixer - W_norm), ls * (b_mixer - b_norm)
                            (rep_vit.py:187-224)
      AttentionBlock.norm   BatchNorm before the 1x1 qkv_proj: W diag(s), W t + b (exact: no padding between them)
      layer_scale*          the layer's `scale` (residual + ls * (conv + bias) in the conv epilogue; bias pre-multiplied here)
      FeatureFusionBlock    the 1x1 conv3 split in its two input halves and composed with conv1 / conv2
    then casts once to fp32.  Each layer is a dict {kind: stem|dw|pw, w, b, s (scale or None), stride, act: none|gelu|resid}."""

    _abi, _tensors = "repvit", 3

    # ---------------------------------------------------------------- checks
    @staticmethod
    def blocker(owner, fnet, cnet_proj, fusion_blocks) -> Optional[str]:
        """Why the HIP encoder side cannot run these modules, or None."""
        from .rep_vit import reparam_blocker
        if owner.training or fnet.training:
            return "training mode (call model.eval(): BatchNorm is folded with its running statistics)"
        why = reparam_blocker(fnet, cnet_proj, fusion_blocks)
        if why:
            return why + "; reparameterised (inference_mode) checkpoints are not supported"
        try:
            RepViTEngine.descriptor(fnet, cnet_proj, fusion_blocks)
        except NndError as e:
            return str(e)
        return None

    @staticmethod
    def descriptor(fnet, cnet_proj, fusion_blocks) -> RepViTDesc:
        d = RepViTDesc()
        for i, m in enumerate(fnet.stem):
            d.stem_strides[i] = _stride1(m.stride, f"stem.{i}")
            if getattr(m, "se", None) is not None and not isinstance(m.se, torch.nn.Identity):
                raise NndError(f"RepViTEngine: stem.{i} has squeeze-excitation (not built)")
        if fnet.stem[0].in_channels != 3 or fnet.stem[0].out_channels != 16:
            raise NndError("RepViTEngine: the stem must be 3 -> 16 channels")
        for i in range(4):
            stage = getattr(fnet, f"stage_{i}")
            lk = stage[0].proj[0]
            if lk.kernel_size % 2 == 0 or lk.kernel_size not in (3, 5, 7):
                raise NndError(f"RepViTEngine: patch_size {lk.kernel_size} is not built (odd 3, 5 or 7)")
            if getattr(lk, "small_kernel", None) is not None and (lk.small_kernel % 2 == 0 or lk.small_kernel > lk.kernel_size):
                raise NndError(f"RepViTEngine: small kernel {lk.small_kernel} is not built")
            d.patch_size = lk.kernel_size
            d.down_strides[i] = _stride1(lk.stride, f"stage_{i} patch embed")
            d.channels[i] = stage[0].proj[1].out_channels
            blocks = list(stage[1])
            d.num_blocks[i] = len(blocks)
            kinds = {type(b).__name__ for b in blocks}
            if len(kinds) > 1:
                raise NndError(f"RepViTEngine: stage_{i} mixes block types {sorted(kinds)}")
            if blocks:
                b0 = blocks[0]
                d.mixer[i] = 1 if type(b0).__name__ == "AttentionBlock" else 0
                ffn = b0.convffn if (d.mixer[i] == 1 or b0.use_ffn) else None
                d.ffn_hidden[i] = ffn.fc1.out_channels if ffn is not None else 0
                for b in blocks:
                    if d.mixer[i] == 0 and (b.use_ffn != bool(d.ffn_hidden[i]) or b.token_mixer.kernel_size != 3):
                        raise NndError(f"RepViTEngine: stage_{i}'s blocks differ in their FFN / kernel")
        d.cnet_dim = cnet_proj[0].out_channels
        d.fusion_dim[0], d.fusion_dim[1] = fusion_blocks[0].conv3.out_channels, fusion_blocks[1].conv3.out_channels
        want = [(d.channels[3], d.channels[1]), (d.fusion_dim[0], 16)]
        for j, fb in enumerate(fusion_blocks):
            if fb.conv3.kernel_size != (1, 1) or fb.conv1.kernel_size != (1, 1) or fb.conv2.kernel_size != (1, 1):
                raise NndError(f"RepViTEngine: fusion_blocks[{j}] has {fb.conv3.kernel_size} convs (built: kernel_size=1, padding=0)")
            if (fb.conv1.in_channels, fb.conv2.in_channels) != want[j]:
                raise NndError(f"RepViTEngine: fusion_blocks[{j}] takes {(fb.conv1.in_channels, fb.conv2.in_channels)} channels, "
                               f"the backbone gives {want[j]}")
        for j, (m, cin) in enumerate(zip(cnet_proj, (d.channels[3], d.fusion_dim[0], d.fusion_dim[1]))):
            if m.kernel_size != 1 or m.in_channels != cin or m.out_channels != d.cnet_dim or not isinstance(m.activation, torch.nn.GELU):
                raise NndError(f"RepViTEngine: cnet_proj[{j}] is not a 1x1 GELU MobileOneBlock {cin} -> {d.cnet_dim}")
        if d.fusion_dim[1] != d.fusion_dim[0]:
            raise NndError("RepViTEngine: cnet_proj[1] and [2] read maps of different widths")
        n = int(lib.nnd_repvit_num_tensors(C.byref(d)))
        if n < 0:
            check(n, "repvit descriptor")
        return d

    # ---------------------------------------------------------------- host fold
    @staticmethod
    def fold(fnet, cnet_proj, fusion_blocks) -> List[dict]:
        def ls_of(t):
            return _d(t).reshape(-1) if t is not None else None

        def resid(conv, ls):
            w, b = _conv_wb(conv)
            if ls is None:
                ls = torch.ones(w.shape[0], dtype=torch.float64)
            return _layer("pw", w, ls * b, act="resid", s=ls)

        L = []
        for i, m in enumerate(fnet.stem):
            w, b = _fold_mobileone(m)
            L.append(_layer("stem" if i == 0 else ("dw" if m.groups > 1 else "pw"), w, b, _stride1(m.stride, "stem"), "gelu"))
        for i in range(4):
            stage = getattr(fnet, f"stage_{i}")
            lk, pw = stage[0].proj
            w, b = _fold_conv_bn(lk.lkb_origin, lk.kernel_size)
            if hasattr(lk, "small_conv"):
                ws, bs = _fold_conv_bn(lk.small_conv, lk.kernel_size)
                w, b = w + ws, b + bs
            L.append(_layer("dw", w, b, _stride1(lk.stride, "patch embed"), "none"))  # no activation: conv.py:454
            w, b = _fold_mobileone(pw)
            L.append(_layer("pw", w, b, 1, "gelu"))
            for blk in stage[1]:
                if type(blk).__name__ == "AttentionBlock":
                    s, t = _bn_affine(blk.norm)
                    wq, bq = _conv_wb(blk.token_mixer.qkv_proj)
                    L.append(_layer("pw", wq * s.reshape(1, -1, 1, 1), bq + wq[:, :, 0, 0] @ t, 1, "none"))
                    L.append(resid(blk.token_mixer.out_proj, ls_of(getattr(blk, "layer_scale_1", None))))
                    ffn, ls = blk.convffn, ls_of(getattr(blk, "layer_scale_2", None))
                else:
                    tm = blk.token_mixer
                    wm, bm = _fold_mobileone(tm.mixer)
                    wn, bn = _fold_mobileone(tm.norm)
                    lsm = _d(tm.layer_scale).reshape(-1, 1, 1, 1) if tm.use_layer_scale else torch.ones(tm.dim, 1, 1, 1, dtype=torch.float64)
                    L.append(_layer("dw", _identity_kernel(tm.dim, tm.dim, tm.kernel_size) + lsm * (wm - wn), lsm.reshape(-1) * (bm - bn), 1,
                                 "none"))
                    ffn = blk.convffn if blk.use_ffn else None
                    ls = ls_of(getattr(blk, "layer_scale", None)) if ffn is not None and blk.use_layer_scale else None
                if ffn is not None:
                    w, b = _conv_wb(ffn.fc1)
                    L.append(_layer("pw", w, b, 1, "gelu"))
                    L.append(resid(ffn.fc2, ls))
        for m in cnet_proj:
            w, b = _fold_mobileone(m)
            L.append(_layer("pw", w, b, 1, "gelu"))
        for fb in fusion_blocks:
            w1, b1 = _conv_wb(fb.conv1)
            w2, b2 = _conv_wb(fb.conv2)
            w3, b3 = _conv_wb(fb.conv3)
            c1 = w1.shape[0]
            w3a, w3b = w3[:, :c1, 0, 0], w3[:, c1:, 0, 0]
            L.append(_layer("pw", (w3a @ w1[:, :, 0, 0])[:, :, None, None], w3a @ b1, 1, "none"))        # coarse half (before the upsample)
            L.append(_layer("pw", (w3b @ w2[:, :, 0, 0])[:, :, None, None], w3b @ b2 + b3, 1, "none"))   # fine half
        return [dict(l, w=l["w"].float(), b=l["b"].float(), s=None if l["s"] is None else l["s"].float()) for l in L]

    @staticmethod
    def fold_forward(layers: List[dict], desc: RepViTDesc, frame1: torch.Tensor, frame2: torch.Tensor):
        """The folded chain as plain fp32 F.conv2d calls, in the kernels' layer order: the host fold checked without a GPU."""
        F = torch.nn.functional
        it = iter(layers)

        def conv(x, l, res=None):
            w = l["w"].to(x.device)
            groups = x.shape[1] if l["kind"] == "dw" else 1
            y = F.conv2d(x, w, l["b"].to(x.device), stride=l["stride"], padding=w.shape[-1] // 2, groups=groups)
            if l["act"] == "gelu":
                return F.gelu(y)
            if l["act"] == "resid":  # residual + ls * (conv + bias): bias was pre-multiplied by ls
                y = F.conv2d(x, w, None) * l["s"].to(x.device).reshape(1, -1, 1, 1) + l["b"].to(x.device).reshape(1, -1, 1, 1)
                return res + y
            return y

        B = frame1.shape[0]
        x = torch.cat([frame1, frame2], 0)
        for _ in range(3):
            x = conv(x, next(it))
        feats = [x]
        for i in range(4):
            x = conv(conv(x, next(it)), next(it))
            for _ in range(desc.num_blocks[i]):
                if desc.mixer[i] == 0:
                    x = conv(x, next(it))
                else:
                    qkv = conv(x, next(it))
                    q, k, v = torch.split(qkv, [1, desc.channels[i], desc.channels[i]], dim=1)
                    ctx = (k * F.softmax(q, dim=-1)).sum(-1, keepdim=True)
                    x = conv(F.relu(v) * ctx, next(it), res=x)
                if desc.ffn_hidden[i] > 0:
                    x = conv(conv(x, next(it)), next(it), res=x)
            feats.append(x)
        cp = [next(it) for _ in range(3)]
        out = [feats[4]]
        for coarse_l, fine_l, fine in ((next(it), next(it), feats[2]), (next(it), next(it), feats[0])):
            a = conv(out[-1], coarse_l)
            up = F.interpolate(a, size=fine.shape[-2:], mode="bilinear", align_corners=False)
            out.append(F.relu(conv(fine, fine_l) + up))
        cnets = [conv(f[:B], l) for f, l in zip(out, cp)]
        return out, cnets, feats

    @classmethod
    def from_modules(cls, fnet, cnet_proj, fusion_blocks, device) -> "RepViTEngine":
        desc = cls.descriptor(fnet, cnet_proj, fusion_blocks)
        return cls(desc, cls.fold(fnet, cnet_proj, fusion_blocks), device)

    # ---------------------------------------------------------------- forward
    def forward(self, frame1: torch.Tensor, frame2: torch.Tensor):
        """(B,3,H,W) x 2 -> (feats, cnets) as Coarse2FineRAFTStereoBase.forward_features: feats[j] (2B, C, h, w) of both frames
        (left first), cnets[j] (B, cnet_dim, h, w) of the left frames; stage order coarse -> fine."""
        d = _dev(frame1, frame2, self.packed)
        frame1, frame2 = frame1.contiguous(), frame2.contiguous()
        if tuple(frame1.shape) != tuple(frame2.shape) or frame1.dim() != 4 or frame1.shape[1] != 3:
            raise NndError(f"repvit: frames {tuple(frame1.shape)} / {tuple(frame2.shape)}: expected two (B, 3, H, W) tensors")
        B, _, H, W = frame1.shape
        N, ds = 2 * B, self.desc

        def down(n, s):
            return (n - 1) // s + 1

        h, w = H, W
        sizes = []
        for s in list(ds.stem_strides) + list(ds.down_strides):
            h, w = down(h, s), down(w, s)
            sizes.append((h, w))
        stem_hw, s1_hw, s3_hw = sizes[2], sizes[4], sizes[6]
        f = lambda n, c, hw: torch.empty((n, c) + tuple(hw), dtype=torch.float32, device=d)  # noqa: E731
        feats = [f(N, ds.channels[3], s3_hw), f(N, ds.fusion_dim[0], s1_hw), f(N, ds.fusion_dim[1], stem_hw)]
        cnets = [f(B, ds.cnet_dim, s3_hw), f(B, ds.cnet_dim, s1_hw), f(B, ds.cnet_dim, stem_hw)]
        ws = self._workspace(int(lib.nnd_repvit_workspace_floats(C.byref(ds), N, H, W)), d)
        with torch.cuda.device(d):
            check(lib.nnd_repvit_forward(C.byref(ds), _p(self.packed), _p(frame1), _p(frame2), B, *[_p(t) for t in feats + cnets],
                                         _p(ws), N, H, W, _stream(d)), "repvit_forward")
        return feats, cnets


# ------------------------------------------------------------------------------------------ MobileNetV3 encoder side (IGEVStereoMBNet)
_MBV3_LAYOUT = None


def _mbv3_layout() -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of MobilenetV3LargeEncoder's state_dict, built once on the meta device."""
    global _MBV3_LAYOUT
    if _MBV3_LAYOUT is None:
        from .mobilenetv3 import MobilenetV3LargeEncoder
        with torch.device("meta"):
            ref = MobilenetV3LargeEncoder()
        _MBV3_LAYOUT = [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    return _MBV3_LAYOUT


def _check_mbv3_backbone(enc, hooks, who: str, what: str, any_order: bool = False) -> None:
    """NndError unless `enc` (named `what` in `who`'s messages) is nndepth_amd.mobilenetv3.MobilenetV3LargeEncoder with
    tf_mobilenetv3_large_100's parameter layout and the feature hooks `hooks` (any_order: in any order)."""
    from . import mobilenetv3 as mb
    if not isinstance(enc, mb.MobilenetV3LargeEncoder) or not isinstance(getattr(enc, "backbone", None), mb.MobileNetV3Features):
        raise NndError(f"{who}: {what} is a {type(enc).__name__}, not nndepth_amd.mobilenetv3.MobilenetV3LargeEncoder")
    got = [(k, tuple(v.shape)) for k, v in enc.state_dict().items()]
    want = _mbv3_layout()
    if got != want:
        bad = next((w for g, w in zip(got, want) if g != w), want[len(got)] if len(got) < len(want) else got[len(want)])
        raise NndError(f"{who}: {what}'s parameters differ from tf_mobilenetv3_large_100's layout (first difference at "
                       f"{bad[0]}); a replaced or reshaped block is not built")
    if (sorted(enc.feature_hooks) if any_order else list(enc.feature_hooks)) != list(hooks):
        raise NndError(f"{who}: feature_hooks {enc.feature_hooks} (built: {list(hooks)})")


def _mbv3_conv(x: torch.Tensor, l: dict, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One folded MobileNetV3 / MiDaS layer as F.conv2d in x's dtype: TF "same" padding for the stem and the depthwise convs,
    padding k // 2 for the others (0 for a 1x1); then the layer's activation, then the residual."""
    from .mobilenetv3 import same_pad
    F = torch.nn.functional
    w, b = l["w"].to(x), l["b"].to(x)
    if l["kind"] in ("stem", "dw"):
        y = F.conv2d(same_pad(x, l["k"], l["stride"]), w, b, stride=l["stride"], groups=x.shape[1] if l["kind"] == "dw" else 1)
    else:
        y = F.conv2d(x, w, b, padding=l["k"] // 2)
    if l["act"] == "relu":
        y = F.relu(y)
    elif l["act"] == "hswish":
        y = F.hardswish(y)
    elif l["act"] == "hsigmoid":
        y = F.hardsigmoid(y)
    return res + y if res is not None else y


def _mbv3_backbone_forward(it, x: torch.Tensor, n_left: Optional[int] = None) -> List[torch.Tensor]:
    """The stem and stages 0..5 over the folded layers `it` yields, in the kernels' layer order -> the six stage outputs.  n_left:
    stages 2..5 run on the first n_left samples only (the left frames; eval BatchNorm is per sample)."""
    from .mobilenetv3 import block_table
    x = _mbv3_conv(x, next(it))
    stages = []
    for si, specs in enumerate(block_table()[:6]):
        if si == 2 and n_left is not None:
            x = x[:n_left]
        for sp in specs:
            inp = x
            if sp["type"] == "ir":
                x = _mbv3_conv(x, next(it))
            x = _mbv3_conv(x, next(it))
            if sp["rd"]:
                x = x * _mbv3_conv(_mbv3_conv(x.mean((2, 3), keepdim=True), next(it)), next(it))
            x = _mbv3_conv(x, next(it), res=inp if sp["skip"] else None)
        stages.append(x)
    return stages


class MobileNetV3Engine(_FoldedEngine):
    """The encoder side of IGEVStereoMBNet on the HIP path (csrc/mbv3.hip, ONE call: nnd_mbv3_forward), packed from the modules of
    nndepth_amd.mobilenetv3 plus fnet_proj / cnet_proj.  `fold(...)` folds every eval-mode BatchNorm into its conv in float64 on the
    host (W * s, t with s = gamma / sqrt(var + eps), t = beta - mean * s); the SE convs and the projections keep their own biases.
    The layers are cast once to fp32 when packed.  Each layer is a dict {kind: stem|dw|pw|se_r|se_e|proj, w, b (float64), k,
    stride, act: none|relu|hswish, skip}."""

    _abi = "mbv3"

    # ---------------------------------------------------------------- checks
    @staticmethod
    def blocker(owner, fnet, fnet_proj, cnet_proj) -> Optional[str]:
        """Why the HIP encoder side cannot run these modules, or None."""
        if owner.training or fnet.training:
            return "training mode (call model.eval(): BatchNorm is folded with its running statistics)"
        try:
            MobileNetV3Engine.descriptor(fnet, fnet_proj, cnet_proj)
        except NndError as e:
            return str(e)
        return None

    @staticmethod
    def descriptor(fnet, fnet_proj, cnet_proj) -> MobileNetV3Desc:
        from . import mobilenetv3 as mb
        _check_mbv3_backbone(fnet, mb.HOOKS, "MobileNetV3Engine", "fnet", any_order=True)
        cls = {"ds": mb.DepthwiseSeparable, "ir": mb.InvertedResidual, "cn": mb.ConvBnAct}
        for i, (stage, specs) in enumerate(zip(fnet.backbone.blocks, mb.block_table())):
            for j, (blk, spec) in enumerate(zip(stage, specs)):
                if type(blk) is not cls[spec["type"]] or blk.spec != spec:
                    raise NndError(f"MobileNetV3Engine: blocks.{i}.{j} is a {type(blk).__name__} {getattr(blk, 'spec', '')}, "
                                   f"not the {cls[spec['type']].__name__} {spec} of the backbone")
                for conv in (m for m in blk.modules() if isinstance(m, torch.nn.Conv2d)):
                    k = conv.kernel_size[0]
                    if conv.dilation != (1, 1) or (type(conv) is torch.nn.Conv2d and conv.padding != (0, 0)) or \
                            (conv.groups != 1 and conv.groups != conv.in_channels):
                        raise NndError(f"MobileNetV3Engine: blocks.{i}.{j} has a {k}x{k} conv with dilation {conv.dilation}, "
                                       f"padding {conv.padding}, groups {conv.groups} (not built)")
        dims = []
        for name, seq in (("fnet_proj", fnet_proj), ("cnet_proj", cnet_proj)):
            conv = seq[0] if len(seq) == 2 else None
            if not (isinstance(conv, torch.nn.Conv2d) and isinstance(seq[1], torch.nn.ReLU) and conv.in_channels == mb.block_table()[1][-1]["cout"]
                    and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1)
                    and conv.groups == 1 and conv.bias is not None):
                raise NndError(f"MobileNetV3Engine: {name} is not Conv2d(24, C, 3, 1, 1) + ReLU")
            dims.append(conv.out_channels)
        d = MobileNetV3Desc(fnet_dim=dims[0], cnet_dim=dims[1], flags=0)
        n = int(lib.nnd_mbv3_num_tensors(C.byref(d)))
        if n < 0:
            check(n, "mbv3 descriptor")
        return d

    # ---------------------------------------------------------------- host fold
    @staticmethod
    def fold_backbone(fnet) -> List[dict]:
        """The backbone's layers alone (stem and stages 0..5), shared with MidasEngine."""
        def cbn(conv, bn):
            s, t = _bn_affine(bn)
            return _d(conv.weight) * s.reshape(-1, 1, 1, 1), t

        bb = fnet.backbone
        L = [_layer("stem", *cbn(bb.conv_stem, bb.bn1), 2, "hswish")]
        for stage in list(bb.blocks)[:6]:  # stage 6's output is never used
            for blk in stage:
                sp = blk.spec
                act = "relu" if sp["relu"] else "hswish"
                if sp["type"] == "ds":
                    L.append(_layer("dw", *cbn(blk.conv_dw, blk.bn1), sp["stride"], act))
                    L.append(_layer("pw", *cbn(blk.conv_pw, blk.bn2), skip=sp["skip"]))
                    continue
                L.append(_layer("pw", *cbn(blk.conv_pw, blk.bn1), act=act))
                L.append(_layer("dw", *cbn(blk.conv_dw, blk.bn2), sp["stride"], act))
                if sp["rd"]:
                    L.append(_layer("se_r", *_conv_wb(blk.se.conv_reduce), act="relu"))
                    L.append(_layer("se_e", *_conv_wb(blk.se.conv_expand), act="hsigmoid"))
                L.append(_layer("pw", *cbn(blk.conv_pwl, blk.bn3), skip=sp["skip"]))
        return L

    @staticmethod
    def fold(fnet, fnet_proj, cnet_proj) -> List[dict]:
        L = MobileNetV3Engine.fold_backbone(fnet)
        for seq in (fnet_proj, cnet_proj):
            L.append(_layer("proj", *_conv_wb(seq[0]), act="relu"))
        return L

    @staticmethod
    def fold_forward(layers: List[dict], frame1: torch.Tensor, frame2: torch.Tensor):
        """The folded chain as plain F.conv2d calls in the kernels' layer order and in the frames' dtype (float64: the fold checked
        without a GPU).  -> (fmap1, fmap2, cnet1, [guide0, guide1, guide2], stage outputs of the left frames)."""
        B = frame1.shape[0]
        stages = _mbv3_backbone_forward(iter(layers), torch.cat([frame1, frame2], 0), n_left=B)
        fmaps = _mbv3_conv(stages[1], layers[-2])
        cnet1 = _mbv3_conv(stages[1][:B], layers[-1])
        return fmaps[:B], fmaps[B:], cnet1, [stages[2], stages[3], stages[5]], [s[:B] for s in stages]

    @classmethod
    def from_modules(cls, fnet, fnet_proj, cnet_proj, device) -> "MobileNetV3Engine":
        desc = cls.descriptor(fnet, fnet_proj, cnet_proj)
        return cls(desc, cls.fold(fnet, fnet_proj, cnet_proj), device)

    # ---------------------------------------------------------------- forward
    def forward(self, frame1: torch.Tensor, frame2: torch.Tensor):
        """(B,3,H,W) x 2 -> (fmap1, fmap2, cnet1, [guide0, guide1, guide2]) as IGEVStereoMBNet.forward_fnet returns them."""
        if tuple(frame1.shape) != tuple(frame2.shape) or frame1.dim() != 4 or frame1.shape[1] != 3:
            raise NndError(f"mbv3: frames {tuple(frame1.shape)} / {tuple(frame2.shape)}: expected two (B, 3, H, W) tensors")
        d = _dev(frame1, frame2, self.packed)
        frame1, frame2 = frame1.contiguous(), frame2.contiguous()
        B, _, H, W = frame1.shape
        ds = self.desc
        hw = [(H, W)]
        for _ in range(5):
            hw.append(((hw[-1][0] + 1) // 2, (hw[-1][1] + 1) // 2))
        f = lambda c, s: torch.empty((B, c) + s, dtype=torch.float32, device=d)  # noqa: E731
        fmap1, fmap2, cnet1 = f(ds.fnet_dim, hw[2]), f(ds.fnet_dim, hw[2]), f(ds.cnet_dim, hw[2])
        guides = [f(40, hw[3]), f(80, hw[4]), f(160, hw[5])]
        ws = self._workspace(int(lib.nnd_mbv3_workspace_floats(C.byref(ds), B, H, W)), d)
        with torch.cuda.device(d):
            check(lib.nnd_mbv3_forward(C.byref(ds), _p(self.packed), _p(frame1), _p(frame2), _p(fmap1), _p(fmap2), _p(cnet1),
                                       *[_p(g) for g in guides], _p(ws), B, H, W, _stream(d)), "mbv3_forward")
        return fmap1, fmap2, cnet1, guides


class MidasEngine(_FoldedEngine):
    """MobileNetV3DepthModel on the HIP path (csrc/midas.hip, ONE call per forward: nnd_midas_forward), packed from the modules of
    nndepth_amd.midas.  `fold(model)` folds every eval-mode BatchNorm into its conv in float64 on the host, as
    MobileNetV3Engine.fold; the layers are cast once to fp32 when packed.  Layer order: the backbone (MobileNetV3Engine.
    fold_backbone) | skip_layers.0..3 | per UpsamplerBlock 0..3: [conv1 + bn1 (blocks 0..2: block 3 runs without a skip input)],
    conv2 + bn2, out_conv | last_conv.0, .2, .4."""

    MAPS = ("tap0", "tap1", "tap2", "tap3", "decoder", "pre_relu")

    _abi = "midas"

    @staticmethod
    def descriptor(model) -> MidasDesc:
        """The descriptor of a nndepth_amd.midas.MobileNetV3DepthModel, or NndError naming what the HIP path does not build."""
        from . import midas as md
        _check_mbv3_backbone(getattr(model, "encoder", None), md.HOOKS, "MidasEngine", "encoder")
        dec = getattr(model, "decoder", None)
        if not isinstance(dec, md.BaseDecoder) or list(dec.in_channels) != list(md.TAP_CHANNELS) or len(set(dec.out_channels)) != 1:
            raise NndError("MidasEngine: decoder is not BaseDecoder([24, 40, 112, 160], [C] * 4)")
        Cc = int(dec.out_channels[0])
        for blk in dec.upsampler_layers:
            if not isinstance(blk, md.UpsamplerBlock) or not blk.use_bn or blk.in_channels != Cc or blk.out_channels != Cc:
                raise NndError(f"MidasEngine: an UpsamplerBlock that is not UpsamplerBlock({Cc}, {Cc}, use_bn=True) is not built")
        lc = model.last_conv
        kinds = [torch.nn.Conv2d, torch.nn.Upsample, torch.nn.Conv2d, torch.nn.ReLU, torch.nn.Conv2d, torch.nn.ReLU]
        if len(lc) != 6 or any(type(m) is not k for m, k in zip(lc, kinds)) or lc[4].out_channels != 1 or lc[0].in_channels != Cc:
            raise NndError("MidasEngine: last_conv is not Conv3x3, Upsample(x2, bilinear), Conv3x3, ReLU, Conv1x1(C, 1), ReLU")
        d = MidasDesc(feature_channels=Cc, flags=0)
        n = int(lib.nnd_midas_num_tensors(C.byref(d)))
        if n < 0:
            check(n, "midas descriptor")
        return d

    @staticmethod
    def fold(model) -> List[dict]:
        def cbn(conv, bn):
            s, t = _bn_affine(bn)
            w, b = _conv_wb(conv)
            return w * s.reshape(-1, 1, 1, 1), b * s + t

        L = MobileNetV3Engine.fold_backbone(model.encoder)
        dec = model.decoder
        for seq in dec.skip_layers:
            L.append(_layer("skip", *_conv_wb(seq[0]), act="relu"))
        for i, blk in enumerate(dec.upsampler_layers):
            if i < len(dec.upsampler_layers) - 1:  # the last block runs with skip_feat=None: conv1 / bn1 are never evaluated
                L.append(_layer("up_conv1", *cbn(blk.conv1, blk.bn1), act="relu"))
            L.append(_layer("up_conv2", *cbn(blk.conv2, blk.bn2), act="relu"))
            L.append(_layer("up_out", *_conv_wb(blk.out_conv), act="relu"))
        lc = model.last_conv
        L.append(_layer("last0", *_conv_wb(lc[0])))
        L.append(_layer("last2", *_conv_wb(lc[2]), act="relu"))
        L.append(_layer("last4", *_conv_wb(lc[4]), act="relu"))
        return L

    @staticmethod
    def fold_forward(layers: List[dict], x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The folded chain as plain F.conv2d / F.interpolate calls in the kernels' layer order and in x's dtype (float64: the
        fold checked without a GPU).  -> {tap0..tap3, decoder, pre_relu, depth}."""
        F = torch.nn.functional
        it = iter(layers)
        conv = _mbv3_conv
        up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)  # noqa: E731
        stages = _mbv3_backbone_forward(it, x)
        taps = [stages[i] for i in (1, 2, 4, 5)]
        skips = [conv(t, next(it)) for t in taps]
        rest = list(it)
        ups = [rest[0:3], rest[3:6], rest[6:9], rest[9:11]]
        out = None
        for i in (3, 2, 1, 0):
            ls = ups[i]
            feat = skips[3] if i == 3 else conv(skips[i], ls[0], res=out)  # feat + relu(bn1(conv1(skip)))
            out = conv(up(conv(feat, ls[-2])), ls[-1])
        t = conv(out, rest[11])
        pre = conv(up(t), rest[12])
        l4 = rest[13]
        pre = F.conv2d(pre, l4["w"].to(x), l4["b"].to(x))
        r = {f"tap{i}": taps[i] for i in range(4)}
        r.update(decoder=out, pre_relu=pre, depth=F.relu(pre))
        return r

    @classmethod
    def from_model(cls, model, device) -> "MidasEngine":
        return cls(cls.descriptor(model), cls.fold(model), device)

    def forward(self, x: torch.Tensor, keep: bool = False):
        """x (B,3,H,W) -> depth (B,1,H,W).  keep=True: -> (depth, {tap0..tap3, decoder, pre_relu}), the intermediate maps as views
        of the workspace (valid until the next call)."""
        if x.dim() != 4 or x.shape[1] != 3:
            raise NndError(f"midas: input {tuple(x.shape)}: expected (B, 3, H, W)")
        d = _dev(x, self.packed)
        x = x.contiguous()
        B, _, H, W = x.shape
        ds = MidasDesc(feature_channels=self.desc.feature_channels, flags=NND_MIDAS_KEEP_PRE if keep else 0)
        ws = self._workspace(int(lib.nnd_midas_workspace_floats(C.byref(ds), B, H, W)), d)
        depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=d)
        with torch.cuda.device(d):
            check(lib.nnd_midas_forward(C.byref(ds), _p(self.packed), _p(x), _p(depth), _p(ws), B, H, W, _stream(d)), "midas_forward")
        if not keep:
            return depth
        Cc = ds.feature_channels
        shapes = [(B, c, H >> (i + 2), W >> (i + 2)) for i, c in enumerate((24, 40, 112, 160))] + [(B, Cc, H // 2, W // 2), (B, 1, H, W)]
        maps = {}
        for which, (name, shp) in enumerate(zip(self.MAPS, shapes)):
            off = int(lib.nnd_midas_workspace_offset(C.byref(ds), which, B, H, W))
            if off < 0:
                check(off, "midas_workspace_offset")
            n = shp[0] * shp[1] * shp[2] * shp[3]
            maps[name] = ws[off:off + n].view(shp)
        return depth, maps


# ---- MidasEngine's new kernels one at a time (per-kernel tests and profiles): parameters packed on every call
def _pack_host(n: int, what: str) -> torch.Tensor:
    if n <= 0:
        check(n, what)
    return torch.empty(n, dtype=torch.float32)


def midas_up2x_pw(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """relu(conv1x1(up2x(x)) + bias), up2x = bilinear x2 with align_corners=False, in one kernel: (N,Cin,h,w) -> (N,Cout,2h,2w)."""
    d = _dev(x)
    x = x.contiguous()
    N, Cin, h, w = x.shape
    Cout = weight.shape[0]
    blob = _pack_host(int(lib.nnd_midas_up2x_pw_packed_floats(Cout, Cin)), "midas_up2x_pw_packed_floats")
    wh, bh = _host(weight), _host(bias)  # kept alive across the call
    check(lib.nnd_midas_up2x_pw_pack(Cout, Cin, _p(wh), _p(bh), _p(blob)), "midas_up2x_pw_pack")
    blob = blob.to(d)
    y = torch.empty((N, Cout, 2 * h, 2 * w), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_midas_up2x_pw(Cout, Cin, _p(blob), _p(x), _p(y), N, h, w, _stream(d)), "midas_up2x_pw")
    return y


def midas_head_pack(w2: torch.Tensor, b2: torch.Tensor, w4: torch.Tensor, b4: torch.Tensor, device) -> torch.Tensor:
    Cc = w2.shape[0]
    blob = _pack_host(int(lib.nnd_midas_head_packed_floats(Cc)), "midas_head_packed_floats")
    host = [_host(t) for t in (w2, b2, w4, b4)]  # kept alive across the call
    check(lib.nnd_midas_head_pack(Cc, *[_p(t) for t in host], _p(blob)), "midas_head_pack")
    return blob.to(device)


def midas_head(t: torch.Tensor, packed: torch.Tensor, want_pre: bool = False):
    """relu(conv1x1_{C->1}(relu(conv3x3(up2x(t)) + b2)) + b4) in one kernel: (N,C,h,w) -> (N,1,2h,2w) [, the map before the last
    ReLU]; packed = midas_head_pack(...)."""
    d = _dev(t, packed)
    t = t.contiguous()
    N, Cc, h, w = t.shape
    depth = torch.empty((N, 1, 2 * h, 2 * w), dtype=torch.float32, device=d)
    pre = torch.empty_like(depth) if want_pre else None
    with torch.cuda.device(d):
        check(lib.nnd_midas_head(Cc, _p(packed), _p(t), _p(depth), _p(pre), N, h, w, _stream(d)), "midas_head")
    return (depth, pre) if want_pre else depth


def midas_conv_add(x: torch.Tensor, feat: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """feat + relu(conv k x k (1 or 3, padding k / 2)(x) + bias): the activation before the addition."""
    d = _dev(x, feat)
    x, feat = x.contiguous(), feat.contiguous()
    N, Cin, H, W = x.shape
    Cout, k = weight.shape[0], weight.shape[-1]
    if tuple(feat.shape) != (N, Cout, H, W):
        raise NndError(f"midas_conv_add: feat {tuple(feat.shape)} must be {(N, Cout, H, W)}")
    blob = _pack_host(int(lib.nnd_mbv3_pointwise_packed_floats(Cout, Cin, k)), "mbv3_pointwise_packed_floats")
    wh, bh = _host(weight), _host(bias)  # kept alive across the call
    check(lib.nnd_mbv3_pointwise_pack(Cout, Cin, k, _p(wh), _p(bh), _p(blob)), "mbv3_pointwise_pack")
    blob = blob.to(d)
    y = torch.empty_like(feat)
    with torch.cuda.device(d):
        check(lib.nnd_midas_conv_add(Cout, Cin, k, _p(blob), _p(x), _p(feat), _p(y), N, H, W, _stream(d)), "midas_conv_add")
    return y


def softargmin_disparity(logits: torch.Tensor) -> torch.Tensor:
    """IGEV initial disparity: logits (B,D,H,W) -> -sum_d d * softmax_d (B,1,H,W) (igev_stereo/model.py:92-95,145-146)."""
    d = _dev(logits)
    logits = logits.contiguous()
    B, D, H, W = logits.shape
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_softargmin_disparity(_p(logits), _p(out), B, D, H, W, _stream(d)), "softargmin_disparity")
    return out


def igev_init_disparity_supported(num_groups: int, D: int) -> bool:
    """Whether igev_init_disparity serves `num_groups` groups and D candidates: the library's own answer
    (nnd_igev_init_disparity_supported: up to 64 groups, up to 4096 candidates)."""
    return bool(lib.nnd_igev_init_disparity_supported(int(num_groups), int(D)))


def igev_init_disparity_kernel(B: int, G: int, H: int, W: int, D: int) -> Optional[str]:
    """Name of the kernel igev_init_disparity runs for the shape (under the current NND_IGEV_SQUEEZE_* switches); None: unsupported."""
    name = lib.nnd_igev_init_disparity_kernel(B, G, H, W, D)
    return None if name is None else name.decode()


def igev_init_disparity_host_params(G: int, D: int) -> bool:
    """Whether igev_init_disparity wants the squeezer's parameters as HOST tensors for this shape (the kernels that take them as
    kernel arguments) rather than where they lie on the device (the chunked kernel): the library's dispatch, asked by name."""
    return igev_init_disparity_kernel(1, G, 1, 1, D) not in (None, "igev_squeeze_general_kernel")


def _on_device(t: Optional[torch.Tensor], d: torch.device) -> Optional[torch.Tensor]:
    """fp32 contiguous on device `d`: the tensor itself when it already is (a model's parameter: no copy, no synchronisation)."""
    return None if t is None else t.detach().to(d, torch.float32).contiguous()


def igev_init_disparity_general(geo_level0: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], B: int, G: int, H: int,
                                W: int, D: int) -> torch.Tensor:
    """igev_init_disparity through nnd_igev_init_disparity_dev, the chunked kernel, at ANY supported shape: weight / bias are read
    where they lie on the device (no host copy, no synchronisation: the call captures into a HIP graph)."""
    d = _dev(geo_level0)
    assert geo_level0.numel() == B * G * H * W * D and tuple(weight.shape) == (1, G, 3, 3, 3)
    wd, bd = _on_device(weight, d), _on_device(bias, d)
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_igev_init_disparity_dev(_p(geo_level0.contiguous()), _p(wd), _p(bd), _p(out), B, G, H, W, D, _stream(d)),
              "igev_init_disparity_dev")
    return out


def igev_init_disparity(geo_level0: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], B: int, G: int, H: int,
                        W: int, D: int) -> torch.Tensor:
    """cv_squeezer Conv3d(G,1,3,1,1) + soft-argmin in one kernel (igev_stereo/model.py:144-146): geo_level0 = rows
    (b,g,h,w1) of D candidates on the device, weight (1,G,3,3,3) / bias (1) = the squeezer's parameters -> (B,1,H,W).
    G <= 8 and D <= 512: the kernels that take the weights as kernel arguments (host tensors wanted); any other shape up to 64
    groups / 4096 candidates: igev_init_disparity_general (device tensors wanted)."""
    if not igev_init_disparity_host_params(G, D):
        return igev_init_disparity_general(geo_level0, weight, bias, B, G, H, W, D)
    d = _dev(geo_level0)
    assert geo_level0.numel() == B * G * H * W * D and tuple(weight.shape) == (1, G, 3, 3, 3)
    # 27*G floats passed by value to the kernel: hand in host tensors (a device tensor costs a synchronising copy here)
    wh, bh = _host(weight), _host(bias)
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_igev_init_disparity(_p(geo_level0.contiguous()), _p(wh), _p(bh), _p(out), B, G, H, W, D, _stream(d)),
              "igev_init_disparity")
    return out


LOFTR_KEYS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight", "mlp.2.weight",
              "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


def full_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, nhead: int) -> torch.Tensor:
    """Softmax attention with 32 channels per head on channel-major maps (csrc/attention.hip; reference FullAttention,
    nndepth/blocks/attn_block.py:59-97, no masks): q (N, nhead*32, L), k and v (N, nhead*32, S) -> (N, nhead*32, L)."""
    d = _dev(q, k, v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    if q.dim() != 3 or k.dim() != 3 or k.shape != v.shape or k.shape[:2] != q.shape[:2] or q.shape[1] != 32 * int(nhead):
        raise NndError(f"full_attention: q {tuple(q.shape)} / k {tuple(k.shape)} / v {tuple(v.shape)} must be (N, {32 * int(nhead)}, L) "
                       f"and twice (N, {32 * int(nhead)}, S)")
    N, Cc, L = q.shape
    S = k.shape[2]
    out = torch.empty_like(q)
    with torch.cuda.device(d):
        check(lib.nnd_full_attention(_p(q), _p(k), _p(v), _p(out), N, int(nhead), L, S, Cc * L, Cc * S, Cc * L, _stream(d)),
              "full_attention")
    return out


class LoftrEngine:
    """One LoFTR encoder layer on (N, d_model, H, W) maps (csrc/loftr.hip): attention = "linear" (the elu feature map) or
    "full" (softmax, csrc/attention.hip).  Both kinds pack the same blob: the attention has no parameters."""

    def __init__(self, d_model: int, nhead: int, attention: str = "linear"):
        if attention not in ("linear", "full"):
            raise NndError(f"LoftrEngine: attention {attention!r} is neither 'linear' nor 'full'")
        self.d_model, self.nhead, self.attention = int(d_model), int(nhead), attention
        n = int(lib.nnd_loftr_packed_floats(self.d_model, self.nhead))
        if n <= 0:
            check(n, "loftr_packed_floats")
        self.packed_floats = n
        self.packed = None
        self._ws = None

    def load(self, sd, prefix: str = "", device="cuda") -> "LoftrEngine":
        host = [_host(sd[prefix + k]) for k in LOFTR_KEYS]
        arr = (C.c_void_p * len(host))(*[t.data_ptr() for t in host])
        blob = torch.empty(self.packed_floats, dtype=torch.float32)
        check(lib.nnd_loftr_pack(self.d_model, self.nhead, arr, _p(blob)), "loftr_pack")
        self.packed = blob.to(device)
        return self

    def forward(self, x: torch.Tensor, source: torch.Tensor) -> torch.Tensor:
        if self.packed is None:
            raise NndError("LoftrEngine: parameters not loaded")
        d = _dev(x, source, self.packed)
        x, source = x.contiguous(), source.contiguous()
        N, Cc, H, W = x.shape
        if Cc != self.d_model or source.shape != x.shape:
            raise NndError(f"loftr: x {tuple(x.shape)} / source {tuple(source.shape)} must both be (N, {self.d_model}, H, W)")
        full = self.attention == "full"
        ws_floats, run = ((lib.nnd_loftr_full_workspace_floats, lib.nnd_loftr_full_layer_forward) if full else
                          (lib.nnd_loftr_workspace_floats, lib.nnd_loftr_layer_forward))
        need = int(ws_floats(self.d_model, self.nhead, N, H, W))
        if self._ws is None or self._ws.numel() < need or self._ws.device != d:
            self._ws = torch.empty(need, dtype=torch.float32, device=d)
        out = torch.empty_like(x)
        with torch.cuda.device(d):
            check(run(self.d_model, self.nhead, _p(self.packed), _p(x), _p(source), _p(out), _p(self._ws), N, H, W, _stream(d)),
                  "loftr_full_layer_forward" if full else "loftr_layer_forward")
        return out


# ------------------------------------------------------------------ Conv3d on depth-major volumes (IGEV regulariser, a15)
def volume_to_depth_major(x: torch.Tensor) -> torch.Tensor:
    """(N,C,D,H,W) -> (N,D+2,C,H,W) with zero end slices."""
    d = _dev(x)
    x = x.contiguous()
    N, Cc, D, H, W = x.shape
    y = torch.empty((N, D + 2, Cc, H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_volume_to_depth_major(_p(x), _p(y), N, Cc, D, H, W, _stream(d)), "volume_to_depth_major")
    return y


def depth_major_to_volume(x: torch.Tensor) -> torch.Tensor:
    """(N,D+2,C,H,W) -> (N,C,D,H,W)."""
    d = _dev(x)
    x = x.contiguous()
    N, Dp, Cc, H, W = x.shape
    y = torch.empty((N, Cc, Dp - 2, H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_depth_major_to_volume(_p(x), _p(y), N, Cc, Dp - 2, H, W, _stream(d)), "depth_major_to_volume")
    return y


def volume_rows_to_depth_major(x: torch.Tensor) -> torch.Tensor:
    """(N,C,H,W,D) (candidate axis contiguous: the pyramid rows) -> (N,D+2,C,H,W) with zero end slices."""
    d = _dev(x)
    if not x.is_contiguous():
        raise NndError("volume_rows_to_depth_major: contiguous (N,C,H,W,D) expected")
    N, Cc, H, W, D = x.shape
    y = torch.empty((N, D + 2, Cc, H, W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_volume_rows_to_depth_major(_p(x), _p(y), N, Cc, D, H, W, _stream(d)), "volume_rows_to_depth_major")
    return y


def depth_major_to_volume_rows(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(N,D+2,C,H,W) -> (N,C,H,W,D), optionally into `out` (e.g. level 0 of a pyramid buffer)."""
    d = _dev(x)
    x = x.contiguous()
    N, Dp, Cc, H, W = x.shape
    if out is None:
        out = torch.empty((N, Cc, H, W, Dp - 2), dtype=torch.float32, device=d)
    if not out.is_contiguous() or out.numel() != N * Cc * H * W * (Dp - 2) or out.dtype != torch.float32 or out.device != d:
        raise NndError("depth_major_to_volume_rows: `out` must be a contiguous fp32 (N,C,H,W,D) tensor on the same device")
    with torch.cuda.device(d):
        check(lib.nnd_depth_major_to_volume_rows(_p(x), _p(out), N, Cc, Dp - 2, H, W, _stream(d)), "depth_major_to_volume_rows")
    return out


class Conv3dNorm(ScaleSlots):
    """nn.Conv3d(k=3, padding=1, stride 1|2) [+ BatchNorm3d(eval)] [+ LeakyReLU] on depth-major volumes; the input may be the
    channel concat of two volumes.  `bn` = (weight, bias, running_mean, running_var) or None."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 1, bn=None, eps: float = 1e-5,
                 leaky_slope: float = 1.0, split: int = 0, device="cuda", arithmetic: str = "fp32"):
        Cout, Cin = int(weight.shape[0]), int(weight.shape[1])
        if tuple(weight.shape[2:]) != (3, 3, 3):
            raise NndError("Conv3dNorm: only 3x3x3 kernels")
        cin0 = split if split > 0 else Cin
        self.arithmetic = arithmetic
        self.desc = Conv3dDesc(Cout, cin0, Cin - cin0, int(stride), arithmetic_id(arithmetic), 0)
        self.calibrated = False
        self.leaky = float(leaky_slope)
        self.packed = _pack_conv_norm("conv3d", self.desc, weight, bias, bn, eps, device)
        self._ran: Optional[torch.Tensor] = None  # device bools: which formulations recorded during the last calibration

    def _calibration_finish(self, status: Optional[torch.Tensor]) -> None:
        offs = [o for _, o in self.formulations()]
        if offs:  # which formulation(s) the calibration forwards took: the ones that hold a record (no synchronisation)
            self._ran = scales_read(self.packed, offs, records=True)[1] != 0
        check(lib.nnd_conv3d_calibration_finish(C.byref(self.desc), _p(self.packed), _p(status), _stream(self.packed.device)),
              "conv3d_calibration_finish")

    # ---- the layer's ONE activation range (scale_names() == [""]), held once per packed formulation
    @staticmethod
    def formulations_of(desc: Conv3dDesc) -> List[Tuple[str, int]]:
        """(name, slot offset) of the fp16x2 formulations the blob of `desc` packs: "plain", "grouped", "slab" (host work)."""
        offs = _enumerate_slots(lambda o, n: lib.nnd_conv3d_scale_slots(C.byref(desc), o, n), "conv3d_scale_slots")
        return [(lib.nnd_conv3d_scale_name(i).decode(), o) for i, o in enumerate(offs) if o >= 0]

    def formulations(self) -> List[Tuple[str, int]]:
        if self.__dict__.get("_formulations") is None:
            self._formulations = self.formulations_of(self.desc)
        return self._formulations

    def _scale_slots(self) -> List[Tuple[str, int]]:
        f = self.formulations()
        return [("", f[0][1])] if f else []

    def read_scales(self, per_formulation: bool = False) -> torch.Tensor:
        """The layer's exponent (1 element): that of the formulation(s) the last calibration ran, the smallest if several ran or none
        is known to have (a loaded state sets them all alike).  per_formulation=True: one per formulations() entry, as stored."""
        xs = scales_read(self._blob(), [o for _, o in self.formulations()])[0]
        if per_formulation or xs.numel() == 0:
            return xs
        if self._ran is None:
            return xs.min().reshape(1)
        ran = self._ran | ~self._ran.any()
        return torch.where(ran, xs, xs.max()).min().reshape(1)  # (the largest one stands in for those that did not run)

    def read_records(self, clear: bool = True) -> torch.Tensor:
        rec = scales_read(self._blob(), [o for _, o in self.formulations()], records=True, clear=clear)[1]
        return rec.max().reshape(1) if rec.numel() else rec  # (a NaN record wins, as it does in the slot)

    def write_scales(self, xs, widen: bool = False) -> None:
        """Every packed formulation takes the exponent: the one the forward picks for another depth runs in the same range."""
        offs = [o for _, o in self.formulations()]
        xs = torch.as_tensor(xs).reshape(-1)
        if xs.numel() != (1 if offs else 0):
            raise NndError(f"Conv3dNorm.write_scales: {xs.numel()} exponents for {1 if offs else 0} layer")
        scales_write(self._blob(), offs, xs.expand(len(offs)), widen)
        self._ran = None
        self.calibrated = True

    def widen_scales(self, before: torch.Tensor) -> None:
        self.write_scales(torch.minimum(self.read_scales(), before.to(self.packed.device)))

    def __call__(self, x0: torch.Tensor, x1: Optional[torch.Tensor] = None) -> torch.Tensor:
        d = _dev(x0, self.packed)
        x0 = x0.contiguous()
        N, Dp, c0, H, W = x0.shape
        if c0 != self.desc.Cin0 or (self.desc.Cin1 > 0) != (x1 is not None):
            raise NndError(f"conv3d: inputs do not match the layer ({c0} vs {self.desc.Cin0} channels, second input {x1 is not None})")
        if x1 is not None:
            x1 = x1.contiguous()
            _dev(x1)
            if tuple(x1.shape) != (N, Dp, self.desc.Cin1, H, W):
                raise NndError(f"conv3d: second input {tuple(x1.shape)} != {(N, Dp, self.desc.Cin1, H, W)}")
        st, D = self.desc.stride, Dp - 2
        Do, Ho, Wo = (D + st - 1) // st, (H + st - 1) // st, (W + st - 1) // st
        y = torch.empty((N, Do + 2, self.desc.Cout, Ho, Wo), dtype=torch.float32, device=d)
        with torch.cuda.device(d):
            check(lib.nnd_conv3d_forward(C.byref(_call_desc(self)), _p(self.packed), _p(x0), _p(x1), _p(y), N, D, H, W, self.leaky,
                                         _stream(d)), "conv3d_forward")
        return y


def volume_upsample2x(x: torch.Tensor) -> torch.Tensor:
    """Trilinear x2 (align_corners=True) of a depth-major volume (N,D+2,C,H,W) -> (N,2D+2,C,2H,2W)."""
    d = _dev(x)
    x = x.contiguous()
    N, Dp, Cc, H, W = x.shape
    y = torch.empty((N, 2 * (Dp - 2) + 2, Cc, 2 * H, 2 * W), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_volume_upsample2x(_p(x), _p(y), N, Cc, Dp - 2, H, W, _stream(d)), "volume_upsample2x")
    return y


def volume_gate_(vol: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """vol (N,D+2,C,H,W) *= sigmoid(logits (N,C,H,W)) in place (FeatureGuidedBlock)."""
    d = _dev(vol, logits)
    logits = logits.contiguous()
    N, Dp, Cc, H, W = vol.shape
    if not vol.is_contiguous() or tuple(logits.shape) != (N, Cc, H, W):
        raise NndError(f"volume_gate: vol {tuple(vol.shape)} / logits {tuple(logits.shape)}")
    with torch.cuda.device(d):
        check(lib.nnd_volume_gate(_p(vol), _p(logits), N, Cc, Dp - 2, H, W, _stream(d)), "volume_gate")
    return vol


# ------------------------------------------------------------- scene types (csrc/scene.hip; the drop-in classes are in scene.py)
def _mask_bytes(mask: Optional[torch.Tensor], like: torch.Tensor, what: str) -> Optional[torch.Tensor]:
    """A bool / uint8 mask of `like`'s shape on `like`'s device, as contiguous bytes (None stays None)."""
    if mask is None:
        return None
    if mask.device != like.device:
        raise NndError(f"{what}: the mask is on {mask.device}, the map on {like.device} (no CPU fallback exists)")
    if mask.dtype not in (torch.bool, torch.uint8):
        raise NndError(f"{what}: masks are torch.bool or torch.uint8; got {mask.dtype}")
    if mask.numel() != like.numel():
        raise NndError(f"{what}: the mask has {mask.numel()} elements, the map {like.numel()}")
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def view_range(data: torch.Tensor, mask: Optional[torch.Tensor], kind: int) -> torch.Tensor:
    """(B,2) device floats: min and max per batch element of the map `get_view` colours (kind 0: |disparity| with occluded
    pixels at 0; kind 1: depth over its valid pixels)."""
    d = _dev(data)
    data = data.contiguous()
    B, Cc, H, W = data.shape
    m = _mask_bytes(mask, data, "view_range")
    ws = torch.empty(max(1, int(lib.nnd_view_range_workspace_bytes(B))), dtype=torch.uint8, device=d)
    rng = torch.empty((B, 2), dtype=torch.float32, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_view_range(_p(data), _p(m), kind, B, Cc, H, W, _p(ws), _p(rng), _stream(d)), "view_range")
    return rng


def colorize(data: torch.Tensor, mask: Optional[torch.Tensor], kind: int, table: torch.Tensor, lo: Optional[float] = None,
             hi: Optional[float] = None, reverse: bool = False) -> torch.Tensor:
    """(B,H,W,3) uint8 on the device: channel 0 of `data` (B,C,H,W) through the (N,3) uint8 device `table`; a bound that is None
    is the batch element's own (view_range).  No host synchronisation."""
    d = _dev(data)
    data = data.contiguous()
    B, Cc, H, W = data.shape
    m = _mask_bytes(mask, data, "colorize")
    if table.device != d or table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] != 3:
        raise NndError(f"colorize: the table must be (N,3) torch.uint8 on {d}; got {tuple(table.shape)} {table.dtype} on {table.device}")
    table = table.contiguous()
    rng = view_range(data, m, kind) if (lo is None or hi is None or (kind == 1 and m is not None)) else None
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=d)
    with torch.cuda.device(d):
        check(lib.nnd_colorize(_p(data), _p(m), kind, B, Cc, H, W, _p(rng), int(lo is not None), float(lo or 0.0), int(hi is not None),
                               float(hi or 0.0), int(bool(reverse)), _p(table), table.shape[0], _p(out), _stream(d)), "colorize")
    return out


def pool_abs(x: torch.Tensor, kernel: Tuple[int, int], is_min: bool, negate: bool, rescale: Optional[Tuple[float, float]] = None,
             mask: Optional[torch.Tensor] = None, indices: bool = False, finite: bool = False):
    """max / min of |x| over non-overlapping windows -> (values, int64 indices or None, gathered mask bytes or None,
    isfinite bytes or None); see nnd_pool_abs."""
    d = _dev(x)
    x = x.contiguous()
    B, Cc, H, W = x.shape
    kh, kw = int(kernel[0]), int(kernel[1])
    if kh < 1 or kw < 1:
        raise NndError(f"pool_abs: a {H}x{W} map cannot be pooled to a larger size (window {kh}x{kw})")
    m = _mask_bytes(mask, x, "pool_abs")
    shape = (B, Cc, H // kh, W // kw)
    y = torch.empty(shape, dtype=torch.float32, device=d)
    idx = torch.empty(shape, dtype=torch.int64, device=d) if indices else None
    mo = torch.empty(shape, dtype=torch.uint8, device=d) if m is not None else None
    fo = torch.empty(shape, dtype=torch.uint8, device=d) if finite else None
    mul, div = (float(rescale[0]), float(rescale[1])) if rescale else (1.0, 1.0)
    with torch.cuda.device(d):
        check(lib.nnd_pool_abs(_p(x), _p(y), _p(idx), _p(m), _p(mo), _p(fo), B, Cc, H, W, kh, kw, int(is_min), int(negate),
                               int(rescale is not None), mul, div, _stream(d)), "pool_abs")
    return y, idx, mo, fo


def resize_bilinear(x: torch.Tensor, size: Tuple[int, int], align_corners: bool = False,
                    rescale: Optional[Tuple[float, float]] = None, finite: bool = False, u8_mode: int = 0):
    """F.interpolate(x, size, mode="bilinear", align_corners=...) of a (B,C,h,w) map.  fp32 x -> (values, isfinite bytes or
    None), values = (v * rescale[0]) / rescale[1] if given.  A bool / uint8 x (an occlusion mask) -> its bytes after the
    reference's float round trip: u8_mode 1 = non-zero (bool), 2 = truncated (uint8)."""
    if x.device.type != "cuda":
        raise NndError(f"resize_bilinear: the map must be on the HIP device; got {x.device} (no CPU fallback exists)")
    H, W = int(size[0]), int(size[1])
    with torch.cuda.device(x.device):
        if x.dtype in (torch.bool, torch.uint8):
            src = _mask_bytes(x, x, "resize_bilinear")
            B, Cc, h, w = src.shape
            out = torch.empty((B, Cc, H, W), dtype=torch.uint8, device=x.device)
            check(lib.nnd_resize_bilinear(_p(src), 1, None, _p(out), int(u8_mode), None, B * Cc, h, w, H, W, int(bool(align_corners)), 0,
                                          1.0, 1.0, _stream(x.device)), "resize_bilinear")
            return out
        d = _dev(x)
        x = x.contiguous()
        B, Cc, h, w = x.shape
        y = torch.empty((B, Cc, H, W), dtype=torch.float32, device=d)
        fo = torch.empty((B, Cc, H, W), dtype=torch.uint8, device=d) if finite else None
        mul, div = (float(rescale[0]), float(rescale[1])) if rescale else (1.0, 1.0)
        check(lib.nnd_resize_bilinear(_p(x), 0, _p(y), None, 0, _p(fo), B * Cc, h, w, H, W, int(bool(align_corners)),
                                      int(rescale is not None), mul, div, _stream(d)), "resize_bilinear")
    return y, fo


def depth_inverse(x: torch.Tensor, clip_max: Optional[float], clip_min: Optional[float], eps: float) -> torch.Tensor:
    """clamp(1 / (x + eps)): max first, then min (Depth.inverse)."""
    d = _dev(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    with torch.cuda.device(d):
        check(lib.nnd_depth_inverse(_p(x), _p(y), x.numel(), float(eps), int(clip_max is not None), float(clip_max or 0.0),
                                    int(clip_min is not None), float(clip_min or 0.0), _stream(d)), "depth_inverse")
    return y
