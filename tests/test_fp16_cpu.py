"""CPU: the one-piece fp16 arithmetic ("fp16", descriptor value 1 = the number of pieces; csrc/split_arith.h) where no GPU is needed —
who accepts it, who refuses what, and the packed blob: one range-scaled fp16 piece per weight in the fragment order of the split
kernels, the SPLIT_TAIL_* slot of fp16x2 behind the bias, and the blobs of the other arithmetics unchanged (the pins of
scripts/make_pack_pins.py as tests/test_pack_pins_cpu.py holds them: the parent's output, not a second run of the code under test)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _keep_global_rng():
    """The module constructors draw their initial parameters from torch's global generator: leave it as it was found."""
    cpu = torch.get_rng_state()
    yield
    torch.set_rng_state(cpu)


def _p(t):
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ acceptance
def test_engines_and_sizing_calls_accept_fp16():
    from nndepth_amd import ops
    from nndepth_amd._lib import EncoderDesc, UpdateBlockDesc, lib
    assert ops.UpdateBlockEngine.ARITHMETIC["fp16"] == 1
    assert ops.UpdateBlockEngine.ARITHMETIC == {"fp32": 0, "bf16x3": 3, "fp16x2": 2, "fp16": 1}
    for gru, hid, ctx, cp, fc, mc in [("sep_conv", 128, 64, 36, 1, 576), ("conv_gru", 128, 128, 36, 2, 576), ("sep_conv", 64, 64, 576, 1, 144)]:
        e1 = ops.UpdateBlockEngine(hid, ctx, cp, fc, mc, gru, "fp16")
        e2 = ops.UpdateBlockEngine(hid, ctx, cp, fc, mc, gru, "fp16x2")
        assert e1.desc.arithmetic == 1 and 0 < e1.packed_floats < e2.packed_floats
        for eng in (e1, e2):  # the same layers carry a scale slot under both range-scaled arithmetics
            n = int(lib.nnd_update_block_scale_slots(C.byref(eng.desc), None, 0))
            offs = (C.c_int64 * n)()
            assert lib.nnd_update_block_scale_slots(C.byref(eng.desc), offs, n) == n
            eng.slots = [o >= 0 for o in offs]
        assert e1.slots == e2.slots and any(e1.slots)
        d = UpdateBlockDesc(hid, ctx, cp, fc, mc, 0 if gru == "sep_conv" else 1, 1, 0, 0)
        assert lib.nnd_update_block_workspace_floats(C.byref(d), 1, 13, 22) > 0
    for norm in ("batch", "instance", "none"):
        for cnet in (0, 192):
            n1 = ops.EncoderEngine(256, norm, cnet, "fp16")
            n2 = ops.EncoderEngine(256, norm, cnet, "fp16x2")
            assert n1.desc.arithmetic == 1
            p1, p2 = (int(lib.nnd_encoder_packed_floats(C.byref(e.desc))) for e in (n1, n2))
            assert 0 < p1 < p2
    assert lib.nnd_encoder_workspace_floats(C.byref(EncoderDesc(256, 1, 192, 1, 0)), 2, 64, 128) > 0
    for cout, cin, kh, kw in [(64, 128, 3, 3), (576, 256, 1, 1), (256, 320, 1, 5), (128, 320, 5, 1)]:
        n1, n2 = (int(lib.nnd_conv2d_packed_floats_ex(cout, cin, kh, kw, a)) for a in (1, 2))
        assert 0 < n1 < n2
    assert lib.nnd_conv2d_packed_floats_ex(256, 36, 1, 1, 1) < 0  # Cin % 16 != 0: refused like the other 16-bit arithmetics


def test_model_constructors_accept_fp16():
    import torch.nn as nn
    from c2f_double import make_c2f
    from igev_double import make_igev
    from nndepth_amd import ops, weightgen
    from nndepth_amd.blocks import BasicUpdateBlock
    from nndepth_amd.cre_stereo import CREStereoBase
    from nndepth_amd.igev_stereo import CostVolumeFilterNetwork, IGEVStereoBase
    from nndepth_amd.raft_stereo import BaseRAFTStereo, Coarse2FineRAFTStereoBase, patch, patch_coarse2fine
    ub = BasicUpdateBlock(hidden_dim=128, cor_planes=36, context_dim=64, flow_channel=1, spatial_scale=8, arithmetic="fp16")
    assert ub.engine.arithmetic == "fp16" and ub.engine.desc.arithmetic == 1
    weightgen.fill_module_(ub, "u.")
    eng = ub.sync_engine("cpu")
    assert eng.packed.numel() == eng.packed_floats
    assert set(eng.activation_ranges().values()) == {65504.0 / 4}  # uncalibrated: xs = 2 in every slot
    for model in (BaseRAFTStereo(arithmetic="fp16"), CREStereoBase(arithmetic="fp16"),
                  make_c2f(Coarse2FineRAFTStereoBase, corr_levels=1, arithmetic="fp16")):
        assert model.arithmetic == "fp16" and model.update_block.engine.desc.arithmetic == 1
        assert model.auto_calibrate
    igev = make_igev(IGEVStereoBase, CostVolumeFilterNetwork, arithmetic="fp16")
    assert igev.arithmetic == "fp16" and igev.update_block.engine.desc.arithmetic == 1
    assert igev.cv_regularizer.arithmetic == "fp16x2"  # Conv3d is not built in one piece: the regulariser runs fp16x2
    assert make_igev(IGEVStereoBase, CostVolumeFilterNetwork, arithmetic="bf16x3").cv_regularizer.arithmetic == "bf16x3"

    class Ref(nn.Module):  # what patch() needs of a reference model
        def __init__(self, **kw):
            super().__init__()
            self.update_block = BasicUpdateBlock(arithmetic="fp32", **kw)
    m = patch(Ref(hidden_dim=128, cor_planes=36, context_dim=128, flow_channel=1, spatial_scale=8), "fp16")
    assert m.update_block.engine.arithmetic == "fp16"
    m = patch_coarse2fine(Ref(hidden_dim=128, cor_planes=36, context_dim=128, flow_channel=1, spatial_scale=(4, 4), gru="conv_gru"), "fp16")
    assert m.update_block.engine.arithmetic == "fp16" and m.arithmetic == "fp16"
    conv = ops.Conv2d(torch.zeros(64, 128, 3, 3), torch.zeros(64), device=None, arithmetic="fp16")
    assert conv.arith == 1
    assert ops.RANGE_SCALED == ("fp16x2", "fp16")


def test_range_scaled_engines_are_asked_to_calibrate(monkeypatch):
    """ops._call_desc / require_calibrated treat "fp16" like "fp16x2"."""
    import contextlib
    from nndepth_amd import _lib, ops
    monkeypatch.setattr(ops.torch.cuda, "device", lambda d: contextlib.nullcontext())
    for arith, want in (("fp16", 1), ("fp16x2", 1), ("bf16x3", 0), ("fp32", 0)):
        eng = ops.UpdateBlockEngine(128, 64, 36, 1, 576, "sep_conv", arith)
        eng._calibration_finish = lambda status: None
        eng.packed = torch.zeros(1)  # (leaving the block looks at the blob's device only)
        with ops.calibration():
            assert ops._call_desc(eng).flags & _lib.NND_FLAG_CALIBRATE == want, arith
        with ops.require_calibrated():
            eng.calibrated = False
            if want:
                with pytest.raises(ops.NeedsCalibration):
                    ops._call_desc(eng)
            else:
                assert ops._call_desc(eng).flags == 0


def test_unknown_arithmetics_are_refused():
    from nndepth_amd import ops
    from nndepth_amd._lib import EncoderDesc, NndError, UpdateBlockDesc, lib
    for bad in (4, -1, 5):
        assert lib.nnd_update_block_packed_floats(C.byref(UpdateBlockDesc(128, 64, 36, 1, 576, 0, bad, 0, 0))) < 0
        assert lib.nnd_encoder_packed_floats(C.byref(EncoderDesc(256, 1, 0, bad, 0))) < 0
        assert lib.nnd_conv2d_packed_floats_ex(64, 128, 3, 3, bad) < 0
    for make in (lambda: ops.UpdateBlockEngine(128, 64, 36, 1, 576, "sep_conv", "fp16x1"),
                 lambda: ops.EncoderEngine(256, "batch", 0, "half"),
                 lambda: ops.Conv2d(torch.zeros(64, 128, 3, 3), torch.zeros(64), device=None, arithmetic="fp8")):
        with pytest.raises(NndError) as e:
            make()
        assert "unknown arithmetic" in str(e.value) and "fp16 =" in str(e.value)


def test_conv3d_refuses_one_piece_with_its_message():
    from nndepth_amd._lib import Conv3dDesc, lib
    for cout, c0, c1, st in [(16, 16, 0, 1), (32, 16, 0, 2), (16, 16, 16, 1), (8, 8, 0, 1)]:
        assert lib.nnd_conv3d_packed_floats(C.byref(Conv3dDesc(cout, c0, c1, st, 1, 0))) < 0
        msg = lib.nnd_last_error().decode()
        assert "conv3d: arithmetic 1 (fp16) is not built for Conv3d" in msg and "fp16x2" in msg, msg
        assert lib.nnd_conv3d_packed_floats(C.byref(Conv3dDesc(cout, c0, c1, st, 2, 0))) > 0


# ------------------------------------------------------------------------------------------------ the packed blob
@pytest.mark.parametrize("cout,cin,kh,kw", [(64, 128, 3, 3), (576, 256, 1, 1)])
def test_pack_one_piece(cout, cin, kh, kw):
    from nndepth_amd._lib import lib
    g = torch.Generator().manual_seed(cout + cin)
    w = torch.randn(cout, cin, kh, kw, generator=g) * 10.0 ** torch.empty(cout, cin, kh, kw).uniform_(-6, 0, generator=g)
    b = torch.randn(cout, generator=g)
    n1, n2 = (int(lib.nnd_conv2d_packed_floats_ex(cout, cin, kh, kw, a)) for a in (1, 2))
    ncb, nch, nt = cout // 32, cin // 16, kh * kw
    assert n1 == ncb * nch * nt * 256 + ncb * 32 + 4  # one 1-KiB fragment per (block, chunk, tap) | bias | tail
    assert n2 == ncb * nch * nt * 512 + ncb * 32 + 4 and n1 < n2
    blob = torch.full((n1 + 8,), 7.0)  # 8 guard floats behind the blob: the packer writes n1 floats
    assert lib.nnd_conv2d_pack_ex(_p(w), _p(b), cout, cin, kh, kw, 1, _p(blob)) == 0
    assert torch.equal(blob[n1:], torch.full((8,), 7.0))
    blob = blob[:n1]
    nw = ncb * nch * nt * 256
    # fragments: [cb][chunk][tap][lane = h * 32 + (co % 32)][8 x fp16] holding channels chunk * 16 + 8 h + j
    frag = blob[:nw].numpy().view(np.float16).reshape(ncb, nch, nt, 2, 32, 8)
    got = torch.from_numpy(frag.transpose(0, 4, 1, 3, 5, 2).reshape(cout, cin, nt).copy())  # [cb, i, chunk, h, j, t]
    tail = blob[nw + ncb * 32:]
    wsinv = tail[3].item()
    s = -int(round(np.log2(wsinv)))
    assert wsinv == 2.0 ** -s
    top = w.abs().max().item() * 2.0 ** s
    assert 2 ** 13 <= top < 2 ** 14, top
    want = (w.reshape(cout, cin, nt) * 2.0 ** s).to(torch.float16)  # fp32 -> fp16: round to nearest even, subnormals kept
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert (want == 0).any() or (want.float().abs() < 2.0 ** -14).any()  # the weights reach down into fp16's subnormals
    assert torch.equal(blob[nw:nw + cout], b)
    assert tail.tolist() == [2.0 ** -(s + 2), 4.0, 0.0, 2.0 ** -s]  # oscale, xscale, amax, wsinv
    # the first piece of the fp16x2 blob of the same weights is this piece
    blob2 = torch.zeros(n2)
    assert lib.nnd_conv2d_pack_ex(_p(w), _p(b), cout, cin, kh, kw, 2, _p(blob2)) == 0
    frag2 = blob2[:2 * nw].numpy().view(np.float16).reshape(ncb, nch, nt, 2, 2, 32, 8)
    assert np.array_equal(frag2[:, :, :, 0].view(np.int16), frag.view(np.int16))
    assert blob2[2 * nw + ncb * 32:].tolist() == tail.tolist()


def test_update_block_and_encoder_blobs_shrink_by_the_second_pieces():
    """The engines' blobs under arithmetic 1: the same layers take the 16-bit kernels as under 2, each with half the fragment floats;
    what falls back to exact fp32 inside the blob (Cin % 16 != 0) has the same size under both."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_pack_pins", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                  "scripts", "make_pack_pins.py"))
    pins = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pins)
    pins.ARITH["fp16"] = 1
    for args in pins.UPDATE_BLOCKS:
        r1, r2, r0 = (pins.update_block(*args, a) for a in ("fp16", "fp16x2", "fp32"))
        assert [o >= 0 for o in r1["scale_slots"]] == [o >= 0 for o in r2["scale_slots"]]
        assert r1["workspace_floats"] == r2["workspace_floats"]
        assert r0["packed_floats"] // 2 < r1["packed_floats"] < r2["packed_floats"]
        assert r1["sha256"] != r2["sha256"]
    r1, r2 = (pins.encoder(1, 192, a) for a in ("fp16", "fp16x2"))
    assert r1["packed_floats"] < r2["packed_floats"] and r1["workspace_floats"] == r2["workspace_floats"]


def _parent_pins():
    import test_pack_pins_cpu as T
    return T


@pytest.mark.parametrize("case_id", [
    "conv2d-192-256-3-3-fp32", "conv2d-192-256-3-3-fp16x2", "conv2d-192-256-3-3-bf16x3", "conv2d-576-256-1-1-fp16x2",
    "conv2d-256-36-1-1-fp16x2", "update_block-sep_conv-128-64-36-1-576-fp16x2", "update_block-sep_conv-128-128-576-1-144-fp16x2",
    "update_block-conv_gru-128-128-36-2-576-bf16x3", "update_block-sep_conv-128-64-36-1-576-fp32", "update_block-sep_conv-128-64-36-1-576-fp16x2-546",
    "encoder-1-192-fp16x2", "encoder-1-192-bf16x3", "encoder-0-0-fp32", "conv3d-16-16-16-1-fp16x2", "conv3d-32-16-0-2-fp16x2"])
def test_blobs_of_the_other_arithmetics_equal_the_parents(case_id):
    T = _parent_pins()
    assert T.pins.run_case(case_id) == T.PINS[case_id]
