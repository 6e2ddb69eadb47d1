"""GPU: the one-launch residual block of the encoder's first stage (csrc/enc_block.hip) against the three launches it replaces.

layer1.0 and layer1.1 of BasicEncoder (64 -> 64, stride 1, 1x1 projection shortcut) run as one launch each in fp16x2 and fp16:
conv1 -> ReLU -> conv2 with the map between them kept in LDS, the shortcut from the same input tile, one store.  Each convolution
keeps its packed blob, its K order and its epilogue arithmetic, and the map between the two 3x3 convs is an fp32 value before it is
split with conv2's activation scale, so the launch must return the BITS of the unfused schedule (NND_NO_FUSED_ENC_BLOCK): every
comparison here is torch.equal on the encoder's outputs, no tolerance.  The engines are calibrated on one input (a calibrating call
runs the unfused schedule in both modes) and evaluated on others.

Frame shapes (the block runs on the half-resolution map, in 8 x 16 tiles with a 2-pixel input halo):
  40x56, 36x44   maps of 20x28 and 18x22: ragged tiles on both axes
  8x24           a 4x12 map, smaller than one tile: the whole halo lies outside the image
  72x136 x 2+2   36x68 maps, four samples: several tiles with interior halos, the batch stride
"""
import ctypes as C
import functools

import pytest
import torch

import history_util as hu
from nndepth_amd import weightgen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARITH = ("fp16x2", "fp16")
SHAPES = {"40x56": (1, 40, 56), "36x44": (1, 36, 44), "8x24": (1, 8, 24), "72x136_b2": (2, 72, 136)}
SWITCH = "NND_NO_FUSED_ENC_BLOCK"


@functools.lru_cache(maxsize=None)
def frames(tag, B, H, W):
    """Seeded frames in [-1, 1) on the device, a pure function of (tag, shape); made once, never modified."""
    u = torch.from_numpy(weightgen.uniform01(f"enc_block/{tag}/{(B, H, W)}", B * 3 * H * W)).reshape(B, 3, H, W)
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


def both_schedules(monkeypatch, capfd, eng, fa, fb):
    """(fused, unfused) outputs; checks through NND_CONV_VERBOSE that the two runs took the schedules they are named after."""
    monkeypatch.setenv("NND_CONV_VERBOSE", "1")
    capfd.readouterr()
    fused = forward(eng, fa, fb)
    torch.cuda.synchronize()
    assert capfd.readouterr().err.count("[nnd] enc_block") == 2, "layer1.0 and layer1.1 did not take the one-launch block"
    monkeypatch.setenv(SWITCH, "1")
    unfused = forward(eng, fa, fb)
    torch.cuda.synchronize()
    assert capfd.readouterr().err.count("[nnd] enc_block") == 0, f"{SWITCH} did not force the three launches"
    monkeypatch.delenv(SWITCH)
    monkeypatch.delenv("NND_CONV_VERBOSE")
    return fused, unfused


def assert_same_bits(fused, unfused):
    for name, x, y in zip(("fmap", "cnet"), fused, unfused):
        assert torch.isfinite(y).all() and y.abs().max() > 0, name
        assert torch.equal(x, y), (name, float((x - y).abs().max()), int((x != y).sum()), x.numel())


@pytest.mark.parametrize("arithmetic", ARITH)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_block_returns_the_bits_of_the_three_launches(monkeypatch, capfd, shape, arithmetic):
    B, H, W = SHAPES[shape]
    eng = engine(arithmetic, "batch")
    assert_same_bits(*both_schedules(monkeypatch, capfd, eng, frames("a", B, H, W), frames("b", B, H, W)))


@pytest.mark.parametrize("arithmetic", ARITH)
def test_fused_block_without_norm(monkeypatch, capfd, arithmetic):
    """norm_fn = "none": the scale slots hold 1, the shifts the conv biases."""
    eng = engine(arithmetic, "none")
    assert_same_bits(*both_schedules(monkeypatch, capfd, eng, frames("a", 1, 36, 44), frames("b", 1, 36, 44)))


@pytest.mark.parametrize("arithmetic", ARITH)
@pytest.mark.parametrize("shape", ["40x56", "8x24"])
def test_large_border_values(monkeypatch, capfd, shape, arithmetic):
    """Frame pixels on the border (and a corner) 8 x the range of the others (4 x the calibration input's, well inside the x 32
    headroom of the scales): the stem's outputs there are the block's largest inputs.
    conv2 pads the map between the convs with zeros; a block that evaluated conv1 on the halo positions outside the image instead
    would add those large neighbours' products to every border pixel."""
    B, H, W = SHAPES[shape]
    fa, fb = frames("a", B, H, W).clone(), frames("b", B, H, W).clone()
    for f in (fa, fb):
        f[:, :, 0, :] *= 8.0
        f[:, :, -1, :] *= 8.0
        f[:, :, :, 0] *= 8.0
        f[:, :, :, -1] *= 8.0
        f[:, :, -1, -1] = 8.0
    assert_same_bits(*both_schedules(monkeypatch, capfd, engine(arithmetic, "batch"), fa, fb))


@pytest.mark.parametrize("arithmetic", ARITH)
def test_result_does_not_depend_on_prior_buffer_contents(monkeypatch, arithmetic):
    """The output buffers and the workspace (its unused y / shortcut regions and the block's own destination included) hold zeros,
    finite garbage or NaN on entry: the same bits."""
    from nndepth_amd._lib import lib
    B, H, W = SHAPES["36x44"]
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
