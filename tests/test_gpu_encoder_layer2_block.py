"""GPU: the one-launch residual block of the encoder's second stage (csrc/enc_block.hip) against the three launches it replaces.

layer2.0 (64 -> 96, stride 2, 1x1 stride-2 shortcut in the split arithmetic) and layer2.1 (96 -> 96, stride 1, exact 1x1 shortcut)
of BasicEncoder run as one launch each in fp16x2 and fp16 wherever the convolution picker gives the block's split-arithmetic
launches a plan without split K (about 512 workgroup columns and more at quarter resolution); everywhere else, and in a
calibrating call, the three launches stay.  Each convolution keeps its packed blob, its K
order and its epilogue arithmetic, so the launch must return the BITS of the unfused schedule (NND_NO_FUSED_ENC_BLOCK): every
comparison here is torch.equal on the encoder's outputs, no tolerance.  The engines are calibrated on one input and evaluated on
others.  The verbose tag of the new block is "[nnd] enc_stage2_block" (layer1's "[nnd] enc_block" is counted by
test_gpu_encoder_fused_block.py) and appears twice per forward.

Frame shapes (the blocks write the quarter-resolution map in 8 x 16 tiles; layer2.0 reads the half-resolution one; workgroup columns of the
three-launch plan = samples x ceil(4x8 sub-tiles / 2), both frames of a pair are samples):
  397x666        100x167 map, 2 x 263 columns: ragged on both axes, odd half-resolution size (199x333: the stride-2 block's
                 last row and column read padding)
  12x16400       3x4100 map, 2 x 257 columns: lower than one tile, the whole vertical halo lies outside the image
  240x572 x 2+2  60x143 maps, 4 x 135 columns: four samples, the batch stride
  40x56          10x14 map: the picker splits K there, the three launches stay
The unfused run of every fused shape is checked to print ks=1 for the five split-arithmetic launches of the two blocks.
"""
import ctypes as C
import functools
import re

import pytest
import torch

import history_util as hu
from nndepth_amd import weightgen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARITH = ("fp16x2", "fp16")
SHAPES = {"397x666": (1, 397, 666), "12x16400": (1, 12, 16400), "240x572_b2": (2, 240, 572)}
SWITCH = "NND_NO_FUSED_ENC_BLOCK"
TAG = "[nnd] enc_stage2_block"
FUSED_BLOCKS = 2  # layer2.0, layer2.1


@functools.lru_cache(maxsize=None)
def frames(tag, B, H, W):
    """Seeded frames in [-1, 1) on the device, a pure function of (tag, shape); made once, never modified."""
    u = torch.from_numpy(weightgen.uniform01(f"enc_layer2_block/{tag}/{(B, H, W)}", B * 3 * H * W)).reshape(B, 3, H, W)
    return (u * 2 - 1).to(DEV)


@functools.lru_cache(maxsize=None)
def engine(arithmetic, norm):
    """BaseRAFTStereo's feature encoder with cnet_proj, calibrated on its own input (not one of the evaluated ones)."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nndepth_amd import ops
    from oracle import torch_ref
    sd = weightgen.fill_state_dict(torch_ref.raft_stereo_spec())
    cnet = {k[len("cnet_proj."):]: v for k, v in sd.items() if k.startswith("cnet_proj.")}
    eng = ops.EncoderEngine(256, norm, 192, arithmetic)
    eng.load({k[len("fnet."):]: v for k, v in sd.items() if k.startswith("fnet.")}, cnet, device=DEV)
    with ops.calibration():
        eng.forward(frames("calib/a", 1, 40, 56) * 2, n_cnet=1, frames_b=frames("calib/b", 1, 40, 56) * 2)
    torch.cuda.synchronize()
    return eng


def forward(eng, fa, fb):
    fmap, cnet = eng.forward(fa, n_cnet=fa.shape[0], frames_b=fb)
    return [fmap.clone(), cnet.clone()]


def both_schedules(monkeypatch, capfd, eng, fa, fb, fused_blocks=FUSED_BLOCKS):
    """(default, switch-forced) outputs; checks through NND_CONV_VERBOSE which schedule each run took and, where the default one is
    expected to fuse, that the three launches it replaces would have run without split K."""
    monkeypatch.setenv("NND_CONV_VERBOSE", "1")
    capfd.readouterr()
    fused = forward(eng, fa, fb)
    torch.cuda.synchronize()
    assert capfd.readouterr().err.count(TAG) == fused_blocks
    monkeypatch.setenv(SWITCH, "1")
    unfused = forward(eng, fa, fb)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert err.count(TAG) == 0, f"{SWITCH} did not force the three launches"
    plans = re.findall(r"conv_split \dx\d Cin=(?:64|96) Cout=96 [^\n]*", err)
    assert len(plans) == 5, plans  # layer2.0: conv1, shortcut, conv2; layer2.1: conv1, conv2
    if fused_blocks:
        assert all(" ks=1," in p for p in plans), plans
    monkeypatch.delenv(SWITCH)
    monkeypatch.delenv("NND_CONV_VERBOSE")
    return fused, unfused


def assert_same_bits(fused, unfused):
    for name, x, y in zip(("fmap", "cnet"), fused, unfused):
        assert torch.isfinite(y).all() and y.abs().max() > 0, name
        assert torch.equal(x, y), (name, float((x - y).abs().max()), int((x != y).sum()), x.numel())


def with_large_border(f):
    f = f.clone()
    f[:, :, 0, :] *= 8.0
    f[:, :, -1, :] *= 8.0
    f[:, :, :, 0] *= 8.0
    f[:, :, :, -1] *= 8.0
    f[:, :, -1, -1] = 8.0
    return f


@pytest.mark.parametrize("arithmetic", ARITH)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_block_returns_the_bits_of_the_three_launches(monkeypatch, capfd, shape, arithmetic):
    B, H, W = SHAPES[shape]
    eng = engine(arithmetic, "batch")
    assert_same_bits(*both_schedules(monkeypatch, capfd, eng, frames("a", B, H, W), frames("b", B, H, W)))


@pytest.mark.parametrize("arithmetic", ARITH)
def test_small_map_keeps_the_three_launches(monkeypatch, capfd, arithmetic):
    """40x56 frames: too few workgroup columns, the picker splits K, so the default schedule is the three launches (tag count 0; layer2.0's own
    64-input convs never split K, its 96 -> 96 conv2 does)."""
    eng = engine(arithmetic, "batch")
    assert_same_bits(*both_schedules(monkeypatch, capfd, eng, frames("a", 1, 40, 56), frames("b", 1, 40, 56), fused_blocks=0))


@pytest.mark.parametrize("arithmetic", ARITH)
def test_fused_block_without_norm(monkeypatch, capfd, arithmetic):
    """norm_fn = "none": the scale slots hold 1, the shifts the conv biases."""
    B, H, W = SHAPES["397x666"]
    eng = engine(arithmetic, "none")
    assert_same_bits(*both_schedules(monkeypatch, capfd, eng, frames("a", B, H, W), frames("b", B, H, W)))


@pytest.mark.parametrize("arithmetic", ARITH)
def test_large_border_values(monkeypatch, capfd, arithmetic):
    """Frame pixels on the border (and a corner) 8 x the range of the others (4 x the calibration input's, well inside the x 32
    headroom of the scales).  conv2 pads the map between the convs with zeros; a block that evaluated conv1 on the halo positions
    outside the image instead would add those large neighbours' products to every border pixel; at stride 2 an off-by-one of the
    padded first row / column moves them."""
    B, H, W = SHAPES["397x666"]
    fa, fb = with_large_border(frames("a", B, H, W)), with_large_border(frames("b", B, H, W))
    assert_same_bits(*both_schedules(monkeypatch, capfd, engine(arithmetic, "batch"), fa, fb))


@pytest.mark.parametrize("arithmetic", ARITH)
def test_calibrating_call_keeps_the_three_launches(monkeypatch, capfd, arithmetic):
    """conv2's range is recorded from the y it stages: under ops.calibration() the block is three launches (on an engine of its own:
    the call moves the scales)."""
    from nndepth_amd import ops
    B, H, W = SHAPES["397x666"]
    eng = engine.__wrapped__(arithmetic, "batch")
    monkeypatch.setenv("NND_CONV_VERBOSE", "1")
    capfd.readouterr()
    with ops.calibration():
        eng.forward(frames("a", B, H, W), n_cnet=B, frames_b=frames("b", B, H, W))
    torch.cuda.synchronize()
    assert capfd.readouterr().err.count(TAG) == 0
    forward(eng, frames("a", B, H, W), frames("b", B, H, W))
    torch.cuda.synchronize()
    assert capfd.readouterr().err.count(TAG) == FUSED_BLOCKS


@pytest.mark.parametrize("arithmetic", ARITH)
def test_result_does_not_depend_on_prior_buffer_contents(monkeypatch, arithmetic):
    """The output buffers and the workspace (its unused y / shortcut regions and the block's own destination included) hold zeros,
    finite garbage or NaN on entry: the same bits."""
    from nndepth_amd._lib import lib
    B, H, W = SHAPES["397x666"]
    eng = engine(arithmetic, "batch")
    fa, fb = frames("a", B, H, W), frames("b", B, H, W)
    ws_floats = int(lib.nnd_encoder_workspace_floats(C.byref(eng.desc), 2 * B, H, W))
    kept = eng._ws

    def run(kind, seed):
        ws = eng._ws = hu.aligned_buffer(ws_floats, kind, DEV, seed)
        with hu.poisoned_allocators(monkeypatch, kind, seed) as filled:
            res = hu.snapshot(eng.forward(fa, n_cnet=B, frames_b=fb))
        torch.cuda.synchronize()
        assert filled and eng._ws.data_ptr() == ws.data_ptr()
        return res

    try:
        base = run("zero", 0)
        assert all(bool(torch.isfinite(t).all()) for t in base)
        for kind in ("zero", "garbage", "nan"):
            bad = hu.differences(base, run(kind, 1))
            assert not bad, (kind, bad)
    finally:
        eng._ws = kept
