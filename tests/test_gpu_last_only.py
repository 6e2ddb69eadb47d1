"""GPU: the last-upsample-only mode of the refinement loops (NND_FLAG_LAST_UPSAMPLE_ONLY; `last_only=True` on the engine,
`outputs="last"` on the models) computes the mask head and the convex upsample on the last iteration only, and its final up_disp,
low-res state and hidden state are those of the all-outputs mode bit for bit: in the three arithmetics, on both flow-head paths
(folded into the upsample launch at most 256 tiles of 4x8 pixels, separate above) and in all four loops."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _raft(raft_sd, iters, arithmetic="fp16x2", outputs="all", fused=True):
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    m = BaseRAFTStereo(iters=iters, context_dim=64, arithmetic=arithmetic, outputs=outputs, fused_loop=fused)
    m.load_state_dict(raft_sd, strict=True)
    return m.to(DEV).eval()


def _frames(seed, B, H, W):
    from nndepth_amd import weightgen
    return [x.to(DEV) for x in weightgen.synthetic_frames(seed, B, H, W)]


def _loop_inputs(m, f1, f2):
    from nndepth_amd import ops
    from nndepth_amd.cost_volume import CorrBlock1D
    fmap1, fmap2, cnet = m.forward_fnet(f1, f2)
    net, inp = ops.split_tanh_relu(cnet.float(), m.hidden_dim)
    return CorrBlock1D(fmap1.float(), fmap2.float(), 4, 4)._pyr, net, inp


def _freeze(m, name, *args):
    """The test doubles' encoder side is PyTorch-ROCm, whose convolutions need not repeat their bits from call to call: computed
    once, so that both modes refine the same features (the HIP path behind it is what is compared)."""
    with torch.no_grad():
        out = getattr(m, name)(*args)
    setattr(m, name, lambda *a: out)


def _last_vs_all(m, *args):
    m.outputs = "all"
    full = m(*args)
    m.outputs = "last"
    last = m(*args)
    m.outputs = "all"
    return full, last


@pytest.mark.parametrize("arithmetic", ["fp32", "bf16x3", "fp16x2"])
@pytest.mark.parametrize("B,H,W", [(1, 96, 160), (2, 384, 768)])  # at 1/8: 9 tiles (folded flow head) | 2 x 144 tiles (separate)
def test_raft_last_equals_all(raft_sd, arithmetic, B, H, W):
    m = _raft(raft_sd, 5, arithmetic)
    full, last = _last_vs_all(m, *_frames(B, B, H, W))
    assert len(full) == 5 and len(last) == 1
    assert torch.equal(last[0]["up_disp"], full[-1]["up_disp"])


def test_raft_seam_by_seam_last_equals_all(raft_sd):
    m = _raft(raft_sd, 3, fused=False)
    full, last = _last_vs_all(m, *_frames(7, 1, 96, 160))
    assert len(last) == 1 and torch.equal(last[0]["up_disp"], full[-1]["up_disp"])


@pytest.mark.parametrize("arithmetic", ["fp32", "bf16x3", "fp16x2"])
@pytest.mark.parametrize("B,H,W", [(1, 96, 160), (2, 384, 768)])
def test_engine_refine_last_only(raft_sd, arithmetic, B, H, W):
    m = _raft(raft_sd, 2, arithmetic)
    f1, f2 = _frames(11, B, H, W)
    m(f1, f2)  # calibrates (fp16x2)
    eng = m.update_block.sync_engine(DEV)
    pyr, net, inp = _loop_inputs(m, f1, f2)
    init = torch.rand(net.shape[0], 1, *net.shape[2:], device=DEV) * 4
    for disp_init in (None, init):
        up_a, low_a, net_a = eng.refine(pyr, 4, 4, net, inp, 8, 6, disp_init=disp_init, keep_all=True)
        up_l, low_l, net_l = eng.refine(pyr, 4, 4, net, inp, 8, 6, disp_init=disp_init, last_only=True)
        assert up_l.shape[0] == 1
        assert torch.equal(up_l[0], up_a[-1]) and torch.equal(low_l, low_a) and torch.equal(net_l, net_a)
    assert eng.desc.flags == 0


def test_igev_last_equals_all():
    from igev_double import make_igev
    from nndepth_amd import weightgen
    from nndepth_amd.igev_stereo import CostVolumeFilterNetwork, IGEVStereoBase
    m = make_igev(IGEVStereoBase, CostVolumeFilterNetwork, iters=4, hidden_dim=64, context_dim=64)
    weightgen.fill_module_(m, "igev.")
    m = m.to(DEV).eval()
    m.outputs = "all"
    f1, f2 = _frames(6, 1, 128, 192)
    _freeze(m, "forward_fnet", f1, f2)
    full = m(f1, f2)
    low_full = m.last_low_coords.clone()
    m.outputs = "last"
    last = m(f1, f2)
    assert len(full) == 4 and len(last) == 1
    assert torch.equal(last[0]["up_disp"], full[-1]["up_disp"]) and torch.equal(m.last_low_coords, low_full)


def test_cre_last_and_test_mode_equal_all(cre_sd):
    from nndepth_amd.cre_stereo import CREStereoBase
    m = CREStereoBase(iters=4)
    m.load_state_dict(cre_sd, strict=True)
    m = m.to(DEV).eval()
    f1, f2 = _frames(3, 1, 128, 192)
    full, last = _last_vs_all(m, f1, f2)
    assert len(full) == 8 and len(last) == 1
    assert torch.equal(last[0]["up_disp"], full[-1]["up_disp"])
    m.test_mode = True
    assert torch.equal(m(f1, f2), full[-1]["up_disp"])
    m.test_mode = False
    init = full[-1]["up_disp"][:, :, ::4, ::4].contiguous()  # the flow_init hand-over: one stage of `iters` iterations
    full, last = _last_vs_all(m, f1, f2, init)
    assert len(full) == 4 and len(last) == 1 and torch.equal(last[0]["up_disp"], full[-1]["up_disp"])


def test_coarse2fine_last_equals_all():
    from c2f_double import make_c2f
    from nndepth_amd import weightgen
    from nndepth_amd.raft_stereo import Coarse2FineRAFTStereoBase
    m = make_c2f(Coarse2FineRAFTStereoBase, iters=3, corr_levels=1)
    weightgen.fill_module_(m, "c2f.")
    m = m.to(DEV).eval()
    f1, f2 = _frames(5, 1, 384, 512)
    _freeze(m, "forward_features", f1, f2)
    full, last = _last_vs_all(m, f1, f2)
    assert len(full) == 9 and len(last) == 1
    assert tuple(last[0]["up_disp"].shape[-2:]) == (384, 512)
    assert torch.equal(last[0]["up_disp"], full[-1]["up_disp"])


def test_calibration_is_that_of_the_all_outputs_schedule(raft_sd):
    f1, f2 = _frames(2, 1, 96, 160)
    a = _raft(raft_sd, 4, "fp16x2", "all")
    b = _raft(raft_sd, 4, "fp16x2", "last")
    out_a, out_b = a(f1, f2), b(f1, f2)  # each calibrates on this pair first
    ra, rb = a.activation_ranges(), b.activation_ranges()
    assert ra and ra == rb
    assert "flow_head.conv1+mask.0" in ra and "mask.2" in ra
    assert torch.equal(out_b[0]["up_disp"], out_a[-1]["up_disp"])


def test_last_only_launch_count(raft_sd, monkeypatch, capfd):
    iters = 4
    m = _raft(raft_sd, 2)
    f1, f2 = _frames(9, 1, 96, 160)
    m(f1, f2)
    eng = m.update_block.sync_engine(DEV)
    pyr, net, inp = _loop_inputs(m, f1, f2)
    torch.cuda.synchronize()
    capfd.readouterr()
    monkeypatch.setenv("NND_DEBUG_SYNC", "1")
    eng.refine(pyr, 4, 4, net, inp, 8, iters, last_only=True)
    torch.cuda.synchronize()
    names = re.findall(r"\[nnd\] (.*?) \.\.\. ok", capfd.readouterr().err)
    assert names.count("flow_head.conv1") == iters - 1, names
    assert names.count("flow_head.conv1+mask.0") == 1, names
    assert sum("upsample" in n for n in names) == 1, names


def test_graphed_last_only_forward_equals_direct(raft_sd):
    from nndepth_amd.graph import GraphedForward
    m = _raft(raft_sd, 6, outputs="last")
    fwd = GraphedForward(m)
    for seed in (0, 1):
        f1, f2 = _frames(seed, 1, 96, 160)
        direct = m(f1, f2)[0]["up_disp"].clone()
        replay = fwd(f1, f2)
        assert len(replay) == 1 and torch.equal(direct, replay[0]["up_disp"])
