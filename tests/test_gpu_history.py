"""GPU: no result depends on what workspaces, scratch and output buffers held before the call (include/nndepth_amd.h, conventions).

Every engine reuses its cached workspace, dirty, for every later call, and every output is a torch.empty; a C caller may pass fresh
hipMalloc memory.  So one call with fixed inputs and fixed packed parameters must return the same bits — and, where it calibrates,
leave the same fp16x2 activation scales — whatever those buffers held on entry.  No tolerance and no reference: the code is compared
with itself under the prior contents of tests/history_util.py (zero, finite garbage, NaN).  Each case first runs twice on zero-filled
buffers, so that a kernel that does not repeat its own bits is reported as that and not as a history dependence.

Two ways in.  Engine level: the engine's `_ws` is replaced by a buffer of exactly the floats the library's *_workspace_floats asks for,
on a 256-byte boundary, holding the pattern (afterwards the engine must still hold that very buffer: it did not reallocate), and the
outputs the wrappers allocate come out of the poisoned allocators.  Model level: two forwards with torch.empty, torch.empty_like and
torch.zeros poisoned, the second starting from the first one's leftovers.  Shape history: a call at a larger ragged shape, then the
compared call at the small one on the same object, against a fresh object.

Shapes are the smallest with padding on both axes of the 4x8 workspace tiles and more than one tile."""
import copy
import ctypes as C
import functools

import pytest
import torch

import history_util as hu
from nndepth_amd import weightgen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARITH = ("fp32", "bf16x3", "fp16x2")
UNFUSE = ("NND_NO_FUSED_UPSAMPLE", "NND_NO_FUSED_LOOKUP", "NND_NO_FOLDED_FLOW_HEAD", "NND_NO_MERGED_FB_LOOKUP")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nndepth_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def rnd(tag, *shape, scale=1.0):
    """Seeded values in [-scale, scale) on the device, a pure function of (tag, shape); made once, never modified."""
    n = int(torch.Size(shape).numel())
    u = torch.from_numpy(weightgen.uniform01(f"history/{tag}/{shape}", n)).reshape(shape)
    return ((u * 2 - 1) * scale).to(DEV)


# ------------------------------------------------------------------------------------------------ the two checks
def _measure(ops, eng, call, calibrate, kind="zero"):
    """What one case compares: the call's tensors; for a calibrating engine the tensors of the calibrating call, those of a second
    call at the scales it fixed, the calibration's status (bit 0: a layer saw inf / NaN), the packed blob (it holds the scales) and the
    engine's activation_ranges()."""
    if not calibrate:
        return hu.snapshot(call(kind))
    with ops.calibration() as c:
        res = hu.snapshot(call(kind))
    res += hu.snapshot(call(kind)) + hu.flatten(c.status) + [eng.packed.clone()]
    if hasattr(eng, "activation_ranges"):
        res += hu.flatten(eng.activation_ranges())
    return res


def check_prior_contents(ops, monkeypatch, call, eng=None, pristine=None, ws_floats=0, calibrate=False, raw_bytes=False):
    """`call(kind)` under each pattern against itself on zero-filled buffers.  With `eng`: its parameters are restored from
    `pristine` and its workspace replaced by `ws_floats` floats of the pattern before every run."""
    def run(kind, seed):
        if eng is not None:
            eng.packed.copy_(pristine)
            eng.calibrated = False
            ws = eng._ws = hu.aligned_buffer(ws_floats, kind, DEV, seed)
        with hu.poisoned_allocators(monkeypatch, kind, seed, raw_bytes=raw_bytes) as filled:
            res = _measure(ops, eng, call, calibrate, kind)
        torch.cuda.synchronize()
        assert filled, "the call allocated nothing through the poisoned allocators"
        if eng is not None:  # the engine ran on this very buffer (it reallocates on a size or device mismatch)
            assert eng._ws.data_ptr() == ws.data_ptr() and eng._ws.numel() == ws_floats
        return res

    assert ws_floats > 0 or eng is None
    base = run("zero", 0)
    assert all(bool(torch.isfinite(t).all()) for t in base if t.is_floating_point()), "the baseline is not finite: NaN would equal NaN"
    repeat = hu.differences(base, run("zero", 0))
    assert not repeat, f"not deterministic on zero-filled buffers (no history involved): {repeat}"
    bad = {kind: d for kind in ("garbage", "nan") for d in [hu.differences(base, run(kind, 1))] if d}
    assert not bad, f"the result depends on what the buffers held on entry: {bad}"


def _twin(eng, pristine):
    """Another engine object on the same packed parameters: its own blob, no workspace yet."""
    e = copy.copy(eng)
    e.packed, e._ws, e.calibrated = pristine.clone(), None, False
    return e


def check_shape_history(ops, eng, pristine, call_at, big, small, calibrate=False):
    """One engine object called at `big`, then at `small`, against a fresh object called at `small` alone."""
    used, fresh = _twin(eng, pristine), _twin(eng, pristine)
    call_at(used, big)
    ws_after_big = used._ws
    got = _measure(ops, used, lambda kind: call_at(used, small), calibrate)
    assert used._ws is ws_after_big  # the small call ran in the large call's leftovers
    want = _measure(ops, fresh, lambda kind: call_at(fresh, small), calibrate)
    torch.cuda.synchronize()
    bad = hu.differences(want, got)
    assert not bad, f"{small} after {big} differs from {small} on a fresh engine: {bad}"


# ------------------------------------------------------------------------------------------------ update block
def _ub_configs():
    from test_gpu_parity import CASES
    cfg = {k: (v["hidden_dim"], v["context_dim"], v["cor_planes"], v["flow_channel"], v["spatial_scale"], "sep_conv")
           for k, v in CASES.items() if k in ("raft_h128_c64", "cre_h128_c128_f2", "igev_h64_c64_cp576")}
    cfg["conv_gru_h128_c128"] = (128, 128, 36, 1, 8, "conv_gru")
    cfg["group_h128_c128_cp144"] = (128, 128, 4 * 9 * 4, 1, 4, "conv_gru")  # Coarse2Fine's block over 4 groups x 4 levels
    return cfg


@functools.lru_cache(maxsize=None)
def ub_engine(name, arithmetic):
    from nndepth_amd import ops
    from oracle import torch_ref as R
    hid, ctx, cor, fc, scale, gru = _ub_configs()[name]
    sd = weightgen.fill_state_dict(R.update_block_spec("ub." + name, hid, cor, ctx, fc, scale, gru=gru))
    eng = ops.UpdateBlockEngine(hid, ctx, cor, fc, 9 * scale * scale, gru, arithmetic).load(sd, f"ub.{name}.", device=DEV)
    return eng, eng.packed.clone()


def ub_ws_floats(eng, B, H, W):
    from nndepth_amd._lib import lib
    return int(lib.nnd_update_block_workspace_floats(C.byref(eng.desc), B, H, W))


@functools.lru_cache(maxsize=None)
def ub_state(name, B, H, W):
    hid, ctx, cor, fc, _, _ = _ub_configs()[name]
    return (torch.tanh(rnd("net", B, hid, H, W, scale=2.0)), torch.relu(rnd("inp", B, ctx, H, W, scale=2.0)),
            rnd("corr", B, cor, H, W, scale=2.0), rnd("flow", B, fc, H, W, scale=4.0))


@pytest.mark.parametrize("arithmetic", ARITH)
@pytest.mark.parametrize("want_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("name", ["raft_h128_c64", "cre_h128_c128_f2", "igev_h64_c64_cp576", "conv_gru_h128_c128"])
def test_update_block_forward(ops, monkeypatch, name, want_mask, arithmetic):
    B, H, W = 2, 7, 13
    eng, pristine = ub_engine(name, arithmetic)
    args = ub_state(name, B, H, W)
    check_prior_contents(ops, monkeypatch, lambda kind: eng.forward(*args, want_mask=want_mask), eng, pristine,
                         ub_ws_floats(eng, B, H, W), calibrate=arithmetic == "fp16x2")


# ---- the refinement loops
LOOPS = {"refine": "raft_h128_c64", "refine_group": "group_h128_c128_cp144", "refine_igev": "igev_h64_c64_cp576",
         "refine_igev_interleaved": "igev_h64_c64_cp576", "refine_cre_iter": "cre_h128_c128_f2"}
LEVELS, RADIUS, ITERS, GROUPS = 4, 4, 3, 8


@functools.lru_cache(maxsize=None)
def loop_inputs(loop, B, H, W):
    """The loop's own device inputs (pyramids, feature maps), built once and never modified."""
    from nndepth_amd import ops
    if loop == "refine_cre_iter":
        return rnd("cre/f1", B, 256, H, W), rnd("cre/f2", B, 256, H, W)
    f = [rnd(f"{loop}/f{i}", B, 64, H, W) for i in range(4 if loop.startswith("refine_igev") else 2)]
    if loop == "refine":
        return (ops.corr1d_build(f[0], f[1], LEVELS),)
    if loop == "refine_group":
        return (ops.raft_group_corr_build(f[0], f[1], 4, LEVELS),)
    feat, geo = ops.group_corr_build(f[0], f[1], GROUPS, 8, LEVELS), ops.group_corr_build(f[2], f[3], GROUPS, 8, LEVELS)
    il = ops.igev_interleave_pyramids(feat, geo, B, GROUPS, H, W, LEVELS) if loop.endswith("interleaved") else None
    return feat, geo, il


def call_loop(eng, loop, shape, init=False, kind="zero", **mode):
    B, H, W = shape
    name = LOOPS[loop]
    net, inp, _, flow = ub_state(name, B, H, W)
    x = loop_inputs(loop, B, H, W)
    init = flow if init else None
    if loop == "refine":
        return eng.refine(x[0], LEVELS, RADIUS, net, inp, 8, ITERS, disp_init=init, **mode)
    if loop == "refine_group":
        return eng.refine_group(x[0], 4, LEVELS, RADIUS, net, inp, 4, ITERS, disp_init=init, **mode)
    if loop.startswith("refine_igev"):
        return eng.refine_igev(x[0], x[1], GROUPS, LEVELS, RADIUS, net, inp, 4, ITERS, disp_init=None if init is None else -init.abs(),
                               interleaved=x[2], **mode)
    scratch = hu.aligned_buffer(x[1].numel(), kind, DEV, seed=5)
    return eng.refine_cre(x[0], x[1], net, inp, 8, ITERS, flow_init=init, scratch=scratch, **mode)


@pytest.mark.parametrize("arithmetic", ARITH)
@pytest.mark.parametrize("switches", ["default", "unfused"])
@pytest.mark.parametrize("init", [False, True], ids=["noinit", "init"])
@pytest.mark.parametrize("mode", ["keep_all", "last_only"])
@pytest.mark.parametrize("loop", ["refine", "refine_group", "refine_igev", "refine_igev_interleaved"])
def test_refine_loops(ops, monkeypatch, loop, mode, init, switches, arithmetic):
    shape = (2, 7, 21)
    if switches == "unfused":
        for name in UNFUSE:
            monkeypatch.setenv(name, "1")
    eng, pristine = ub_engine(LOOPS[loop], arithmetic)
    loop_inputs(loop, *shape)  # built before any allocator is replaced
    check_prior_contents(ops, monkeypatch, lambda kind: call_loop(eng, loop, shape, init, kind, **{mode: True}), eng, pristine,
                         ub_ws_floats(eng, *shape), calibrate=arithmetic == "fp16x2")


@pytest.mark.parametrize("arithmetic", ARITH)
@pytest.mark.parametrize("init", [False, True], ids=["noinit", "init"])
@pytest.mark.parametrize("scratch", ["iter", "offset_x1", "offset_x2"])
def test_refine_cre(ops, monkeypatch, scratch, init, arithmetic):
    """9x14, 256 channels, 3 iterations: the 1x9 and the 3x3 window both run.  The library chooses the offset kernel by the size of
    the scratch it is handed (include/nndepth_amd.h, nnd_cre_stereo_refine): exactly B*C*H*W floats -> the planar kernel, exactly
    twice that -> the channels-last one.  So every C-ABI call is checked to have received the injected buffer and its size."""
    from nndepth_amd._lib import lib
    B, H, W = 2, 9, 14
    eng, pristine = ub_engine("cre_h128_c128_f2", arithmetic)
    net, inp, _, flow = ub_state("cre_h128_c128_f2", B, H, W)
    f1, f2 = loop_inputs("refine_cre_iter", B, H, W)
    extra = None if scratch == "iter" else rnd("cre/extra", B, 18, H, W)
    floats = f2.numel() * (2 if scratch == "offset_x2" else 1)

    real, seen = lib.nnd_cre_stereo_refine, []

    def spy(*args):  # (desc, packed, fmap1, fmap2, C, extra_offset, scratch, scratch_floats, ...)
        seen.append((args[6].value, int(args[7]), bool(args[5].value)))
        return real(*args)
    monkeypatch.setattr(lib, "nnd_cre_stereo_refine", spy)

    def call(kind):
        buf = hu.aligned_buffer(floats, kind, DEV, seed=5)
        del seen[:]
        out = eng.refine_cre(f1, f2, net, inp, 8, ITERS, flow_init=flow if init else None, extra_offset=extra, scratch=buf)
        assert seen == [(buf.data_ptr(), floats, extra is not None)], (seen, buf.data_ptr(), floats)
        return out
    check_prior_contents(ops, monkeypatch, call, eng, pristine, ub_ws_floats(eng, B, H, W), calibrate=arithmetic == "fp16x2")


@pytest.mark.parametrize("arithmetic", ARITH)
@pytest.mark.parametrize("loop", ["forward"] + list(LOOPS))
def test_update_block_shape_history(ops, loop, arithmetic):
    """13x29, then 7x21 (the CREStereo stage: 14x22, then 9x14) on one engine: the small shape sees the large one's leftovers at other
    offsets.  fp16x2: the large call runs at the default scales (out of range: inf stays in the workspace), then both engines
    calibrate on the small input before the compared call."""
    name = "raft_h128_c64" if loop == "forward" else LOOPS[loop]
    eng, pristine = ub_engine(name, arithmetic)
    big, small = ((2, 14, 22), (2, 9, 14)) if loop == "refine_cre_iter" else ((2, 13, 29), (2, 7, 21))

    def call_at(e, shape):
        if loop == "forward":
            return e.forward(*ub_state(name, *shape))
        return call_loop(e, loop, shape, init=True)
    check_shape_history(ops, eng, pristine, call_at, big, small, calibrate=arithmetic == "fp16x2")


# ------------------------------------------------------------------------------------------------ BasicEncoder
@functools.lru_cache(maxsize=None)
def encoder_engine(norm, arithmetic):
    from nndepth_amd import ops
    from oracle import cre_ref, torch_ref
    if norm == "batch":
        sd = weightgen.fill_state_dict(torch_ref.raft_stereo_spec())
        cnet = {k[len("cnet_proj."):]: v for k, v in sd.items() if k.startswith("cnet_proj.")}
        eng = ops.EncoderEngine(256, "batch", 192, arithmetic)
    else:
        sd, cnet = weightgen.fill_state_dict(cre_ref.cre_stereo_spec()), None
        eng = ops.EncoderEngine(256, "instance", 0, arithmetic)
    eng.load({k[len("fnet."):]: v for k, v in sd.items() if k.startswith("fnet.")}, cnet, device=DEV)
    return eng, eng.packed.clone()


def call_encoder(eng, H, W):
    f1, f2 = rnd("enc/f1", 1, 3, H, W), rnd("enc/f2", 1, 3, H, W)
    return eng.forward(f1, n_cnet=1 if eng.desc.cnet_dim > 0 else 0, frames_b=f2)


def encoder_ws_floats(eng, H, W):
    from nndepth_amd._lib import lib
    return int(lib.nnd_encoder_workspace_floats(C.byref(eng.desc), 2, H, W))


@pytest.mark.parametrize("arithmetic,layout", [(a, "c4") for a in ARITH] + [("bf16x3", "planar")])
@pytest.mark.parametrize("norm", ["batch", "instance"])
def test_encoder(ops, monkeypatch, norm, arithmetic, layout):
    """Two frame tensors of 1x3x51x77: the pyramid is 26x39, 13x20, 7x10."""
    H, W = 51, 77
    if layout == "planar":
        monkeypatch.setenv("NND_ENC_NO_C4", "1")
    eng, pristine = encoder_engine(norm, arithmetic)
    check_prior_contents(ops, monkeypatch, lambda kind: call_encoder(eng, H, W), eng, pristine, encoder_ws_floats(eng, H, W),
                         calibrate=arithmetic == "fp16x2")


@pytest.mark.parametrize("arithmetic", ARITH)
@pytest.mark.parametrize("norm", ["batch", "instance"])
def test_encoder_shape_history(ops, norm, arithmetic):
    eng, pristine = encoder_engine(norm, arithmetic)
    check_shape_history(ops, eng, pristine, lambda e, hw: call_encoder(e, *hw), (77, 117), (51, 77), calibrate=arithmetic == "fp16x2")


# ------------------------------------------------------------------------------------------------ folded encoder sides, MiDaS, LoFTR
@functools.lru_cache(maxsize=None)
def folded_engine(which):
    from nndepth_amd import ops
    if which == "repvit":
        from nndepth_amd.raft_stereo import Coarse2FineGroupRepViTRAFTStereo
        m = weightgen.fill_module_(Coarse2FineGroupRepViTRAFTStereo(iters=2, corr_levels=1), "c2frv.").eval()
        eng = ops.RepViTEngine.from_modules(m.fnet, m.cnet_proj, m.fusion_blocks, DEV)
    elif which == "mbv3":
        from nndepth_amd.igev_stereo import IGEVStereoMBNet
        m = weightgen.fill_module_(IGEVStereoMBNet(iters=2), "igevmb.").eval()
        eng = ops.MobileNetV3Engine.from_modules(m.fnet, m.fnet_proj, m.cnet_proj, DEV)
    else:
        from nndepth_amd.midas import MobileNetV3DepthModel
        eng = ops.MidasEngine.from_model(weightgen.fill_module_(MobileNetV3DepthModel(feature_channels=64), "midas.").eval(), DEV)
    return eng, eng.packed.clone()


def call_folded(eng, which, hw, keep=False):
    B = 2
    if which == "midas":
        return eng.forward(rnd("midas/x", B, 3, *hw), keep=keep)
    return eng.forward(rnd(which + "/f1", B, 3, *hw), rnd(which + "/f2", B, 3, *hw))


def folded_ws_floats(eng, which, hw, keep=False):
    from nndepth_amd._lib import NND_MIDAS_KEEP_PRE, MidasDesc, lib
    if which == "repvit":
        return int(lib.nnd_repvit_workspace_floats(C.byref(eng.desc), 4, *hw))
    if which == "mbv3":
        return int(lib.nnd_mbv3_workspace_floats(C.byref(eng.desc), 2, *hw))
    ds = MidasDesc(feature_channels=eng.desc.feature_channels, flags=NND_MIDAS_KEEP_PRE if keep else 0)
    return int(lib.nnd_midas_workspace_floats(C.byref(ds), 2, *hw))


# frame sizes: the smallest ragged ones the engines' own tests use (MiDaS refuses sizes that are no multiple of 32: 3x5 at 1/32)
FOLDED = {"repvit": ((100, 148), (148, 220)), "mbv3": ((100, 148), (148, 220)), "midas": ((96, 160), (160, 224))}


@pytest.mark.parametrize("which,keep", [("repvit", False), ("mbv3", False), ("midas", False), ("midas", True)])
def test_folded_engines(ops, monkeypatch, which, keep):
    """Batch 2, exact fp32 (the arithmetic these engines have); MiDaS with `keep` returns views of its workspace as well."""
    eng, pristine = folded_engine(which)
    hw = FOLDED[which][0]
    check_prior_contents(ops, monkeypatch, lambda kind: call_folded(eng, which, hw, keep), eng, pristine,
                         folded_ws_floats(eng, which, hw, keep))


@pytest.mark.parametrize("which", list(FOLDED))
def test_folded_engines_shape_history(ops, which):
    eng, pristine = folded_engine(which)
    small, big = FOLDED[which]
    check_shape_history(ops, eng, pristine, lambda e, hw: call_folded(e, which, hw, keep=which == "midas"), big, small)


@functools.lru_cache(maxsize=None)
def loftr_engine():
    from nndepth_amd import ops
    from oracle import cre_ref
    eng = ops.LoftrEngine(256, 8).load(weightgen.fill_state_dict(cre_ref.cre_stereo_spec()), "self_att_fn.layers.0.", device=DEV)
    return eng, eng.packed.clone()


def call_loftr(eng, style, shape):
    x = rnd("loftr/x", *shape)
    return eng.forward(x, x if style == "self" else rnd("loftr/source", *shape))


@pytest.mark.parametrize("style", ["self", "cross"])
def test_loftr(ops, monkeypatch, style):
    from nndepth_amd._lib import lib
    shape = (2, 256, 5, 9)
    eng, pristine = loftr_engine()
    check_prior_contents(ops, monkeypatch, lambda kind: call_loftr(eng, style, shape), eng, pristine,
                         int(lib.nnd_loftr_workspace_floats(256, 8, 2, 5, 9)))


def test_loftr_shape_history(ops):
    eng, pristine = loftr_engine()
    check_shape_history(ops, eng, pristine, lambda e, shape: call_loftr(e, "cross", shape), (2, 256, 8, 13), (2, 256, 5, 9))


# ------------------------------------------------------------------------------------------------ the small workspaces
def test_eval_criterion(ops, monkeypatch):
    """A mask and two thresholds at 2x2x37x53, the cached per-device workspace replaced by exactly the bytes the library asks for
    one output."""
    from nndepth_amd import prepost
    from nndepth_amd._lib import lib
    gt, pred = rnd("epe/gt", 2, 2, 37, 53, scale=40.0), rnd("epe/pred", 2, 2, 37, 53, scale=40.0)
    mask = rnd("epe/mask", 2, 1, 37, 53) > -0.4
    crit = prepost.EvalCriterion({"d1": 1.0, "d3": 3.0})
    nbytes = int(lib.nnd_stereo_eval_workspace_bytes(1))
    assert nbytes > 0 and nbytes % 8 == 0

    def call(kind):
        ws = prepost._STEREO_EVAL_WS[DEV] = hu.aligned_buffer(nbytes // 8, kind, DEV, seed=7, dtype=torch.float64)
        out = crit(gt, pred, mask)
        assert prepost._STEREO_EVAL_WS[DEV].data_ptr() == ws.data_ptr()
        return out
    try:
        check_prior_contents(ops, monkeypatch, call)
    finally:
        prepost._STEREO_EVAL_WS.pop(DEV, None)


def test_depth_eval_criterion(ops, monkeypatch):
    """metrics_tensor at 3x1x37x53 with a mask, the cached per-device workspace replaced by exactly the bytes the library asks for."""
    from nndepth_amd import prepost
    from nndepth_amd._lib import lib
    gt = rnd("depth/gt", 3, 1, 37, 53, scale=30.0).abs() + 0.5
    pred = 0.7 * gt + 2.0 + 0.1 * gt * rnd("depth/noise", 3, 1, 37, 53)
    mask = rnd("depth/mask", 3, 1, 37, 53) > -0.4
    crit = prepost.DepthEvalCriterion(max_depth=80.0)
    doubles = (int(lib.nnd_depth_eval_workspace_bytes(3)) + 7) // 8

    def call(kind):
        ws = prepost._DEPTH_EVAL_WS[DEV] = hu.aligned_buffer(doubles, kind, DEV, seed=7, dtype=torch.float64)
        out = crit.metrics_tensor(pred, gt, mask)
        assert prepost._DEPTH_EVAL_WS[DEV].data_ptr() == ws.data_ptr()
        return out
    try:
        check_prior_contents(ops, monkeypatch, call)
    finally:
        prepost._DEPTH_EVAL_WS.pop(DEV, None)


@pytest.mark.parametrize("kind_of_view", [0, 1], ids=["disparity", "depth"])
def test_view_range(ops, monkeypatch, kind_of_view):
    data = rnd("view/data", 3, 1, 37, 53, scale=50.0) if kind_of_view == 0 else rnd("view/data", 3, 1, 37, 53, scale=30.0).abs() + 0.1
    mask = rnd("view/mask", 3, 1, 37, 53) > -0.4
    check_prior_contents(ops, monkeypatch, lambda kind: ops.view_range(data, mask, kind_of_view), raw_bytes=True)


def test_depth_major_to_volume_rows_into_a_given_buffer(ops, monkeypatch):
    """The `out` argument (level 0 of a pyramid buffer in the IGEV cost volume) may hold anything."""
    N, D, Cc, H, W = 2, 13, 8, 5, 7
    x = rnd("rows/x", N, D + 2, Cc, H, W)

    def call(kind):
        out = hu.aligned_buffer(N * Cc * H * W * D, kind, DEV, seed=9).view(N, Cc, H, W, D)
        got = ops.depth_major_to_volume_rows(x, out)
        assert got.data_ptr() == out.data_ptr()
        return got, ops.depth_major_to_volume_rows(x)
    check_prior_contents(ops, monkeypatch, call)


# ------------------------------------------------------------------------------------------------ model level
def _raft(**kw):
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    return BaseRAFTStereo(iters=3, context_dim=64, **kw), "raft."


def _c2f(**kw):
    from nndepth_amd.raft_stereo import Coarse2FineGroupRepViTRAFTStereo
    return Coarse2FineGroupRepViTRAFTStereo(iters=2, corr_levels=1, **kw), "c2frv."


def _cre(**kw):
    from nndepth_amd.cre_stereo import CREStereoBase
    return CREStereoBase(iters=4, **kw), "cre."


def _igev(**kw):
    from igev_double import make_igev
    from nndepth_amd.igev_stereo import CostVolumeFilterNetwork, IGEVStereoBase
    return make_igev(IGEVStereoBase, CostVolumeFilterNetwork, iters=3, hidden_dim=64, context_dim=64, **kw), "igev."


def _igev_mbnet(**kw):
    from nndepth_amd.igev_stereo import IGEVStereoMBNet
    return IGEVStereoMBNet(iters=3, **kw), "igevmb."


def _midas(**kw):
    from nndepth_amd.midas import MobileNetV3DepthModel
    return MobileNetV3DepthModel(feature_channels=64), "midas."


# model -> (constructor, default arithmetic or None, the smallest frame size its golden test uses, a larger ragged one)
MODELS = {
    "BaseRAFTStereo": (_raft, "fp16x2", (96, 160), (136, 232)),
    "Coarse2FineGroupRepViTRAFTStereo": (_c2f, "fp16x2", (128, 192), (192, 320)),  # (multiples of 64: the cascade's strides)
    "CREStereoBase": (_cre, "fp16x2", (128, 192), (192, 288)),
    "IGEVStereoBase": (_igev, "fp16x2", (128, 192), (192, 288)),  # HIP regulariser on depth-major volumes behind the test double's encoder
    "IGEVStereoMBNet": (_igev_mbnet, "fp16x2", (128, 192), (192, 288)),
    "MobileNetV3DepthModel": (_midas, None, (128, 192), (192, 288)),
}
MODEL_CASES = [(n, a) for n, (_, default, _, _) in MODELS.items() for a in (("fp32", default) if default else (None,))]
HISTORY_CASES = [(n, a) for n, (_, default, _, _) in MODELS.items() for a in (("fp32", "bf16x3") if default else (None,))]
_frozen = {}  # IGEVStereoBase: the test double's PyTorch-ROCm encoder, evaluated once per frame size
_baseline = {}


@functools.lru_cache(maxsize=None)
def _template(name, arithmetic):
    m, prefix = MODELS[name][0](**({} if arithmetic is None else {"arithmetic": arithmetic}))
    return weightgen.fill_module_(m, prefix).eval()


def fresh_model(name, arithmetic):
    m = copy.deepcopy(_template(name, arithmetic)).to(DEV).eval()
    if name == "IGEVStereoBase":
        # the double's encoder side is PyTorch-ROCm, whose convolutions need not repeat their bits: every model object refines the
        # same features (what is compared is the HIP path behind them)
        def forward_fnet(f1, f2, own=m.forward_fnet):
            key = tuple(f1.shape)
            if key not in _frozen:
                with torch.no_grad():
                    _frozen[key] = own(f1, f2)
            return _frozen[key]
        m.forward_fnet = forward_fnet
    return m


def frames(name, hw):
    f = [x.to(DEV) for x in weightgen.synthetic_frames(5, 1, *hw)]
    return f[:1] if name == "MobileNetV3DepthModel" else f


def forward_all(m, fr):
    """Every tensor a forward returns (IGEV: and the loop's low-resolution state; fp16x2: and the scales the first forward fixed)."""
    out = m(*fr)
    maps = [out] if torch.is_tensor(out) else [o["up_disp"] for o in out]
    if hasattr(m, "last_low_coords"):
        maps.append(m.last_low_coords)
    res = hu.snapshot(maps)
    if getattr(m, "arithmetic", None) == "fp16x2" and hasattr(m, "activation_ranges"):
        res += hu.flatten(m.activation_ranges())
    return res


def two_forwards(monkeypatch, name, arithmetic, kind, seed):
    """Two forwards of a fresh model (the second in the first one's leftovers) with the three allocators poisoned."""
    fr = frames(name, MODELS[name][2])
    m = fresh_model(name, arithmetic)
    if name == "IGEVStereoBase":
        m.forward_fnet(*fr)
    with hu.poisoned_allocators(monkeypatch, kind, seed) as filled:
        res = forward_all(m, fr) + forward_all(m, fr)
    torch.cuda.synchronize()
    assert filled
    return res


def baseline(monkeypatch, name, arithmetic):
    if (name, arithmetic) not in _baseline:
        base = two_forwards(monkeypatch, name, arithmetic, "zero", 0)
        assert all(bool(torch.isfinite(t).all()) for t in base)
        _baseline[name, arithmetic] = (base, hu.differences(base, two_forwards(monkeypatch, name, arithmetic, "zero", 0)))
    return _baseline[name, arithmetic]


@pytest.mark.parametrize("kind", hu.PATTERNS)
@pytest.mark.parametrize("name,arithmetic", MODEL_CASES)
def test_model_forwards(monkeypatch, name, arithmetic, kind):
    """fp32 and the model's default arithmetic (fp16x2: the first forward calibrates, under the same poison).  `zero` is the
    determinism check of the baseline itself: two fresh models on zero-filled buffers."""
    base, repeat = baseline(monkeypatch, name, arithmetic)
    assert not repeat, f"not deterministic on zero-filled buffers (no history involved): {repeat}"
    if kind != "zero":
        bad = hu.differences(base, two_forwards(monkeypatch, name, arithmetic, kind, 1))
        assert not bad, f"the forwards depend on what torch.empty / empty_like / zeros returned ({kind}): {bad}"


@pytest.mark.parametrize("name,arithmetic", HISTORY_CASES)
def test_model_shape_history(name, arithmetic):
    """A forward at the larger size, then at the small one, against a fresh model at the small one.  fp16x2 is left out: a model
    calibrates on its first input, so the two models' scales legitimately differ."""
    _, _, small, big = MODELS[name]
    used, fresh = fresh_model(name, arithmetic), fresh_model(name, arithmetic)
    used(*frames(name, big))
    got, want = forward_all(used, frames(name, small)), forward_all(fresh, frames(name, small))
    bad = hu.differences(want, got)
    assert not bad, f"{small} after {big} differs from {small} on a fresh model: {bad}"
