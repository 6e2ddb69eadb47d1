"""Coarse2FineGroupRepViTRAFTStereo drop-in class and its encoder side, without a GPU: state_dict layout against the reference's
(tests/golden/c2f_repvit.npz, scripts/make_golden_c2f_repvit.py), the containers' PyTorch forward and the host fold
(ops.RepViTEngine.fold) against the reference's encoder-side maps, and the refusals of the C-ABI / Python side."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from nndepth_amd import weightgen

GOLD = os.path.join(os.path.dirname(__file__), "golden", "c2f_repvit.npz")
CONFIGS = {
    "default": dict(corr_levels=1),
    "alt": dict(corr_levels=1, context_dim=64, hidden_dim=64, num_blocks_per_stage=[1, 2, 1, 1],
                token_mixer_types=["repmixer", "attention", "repmixer", "attention"], use_ffn_per_stage=[True, True, False, True]),
}
MAPS = ["fnet0", "fnet1", "fnet2", "fnet3", "fnet4", "fused1", "fused2", "cnet0", "cnet1", "cnet2"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def build(cfg, **kw):
    from nndepth_amd.raft_stereo import Coarse2FineGroupRepViTRAFTStereo
    m = Coarse2FineGroupRepViTRAFTStereo(iters=4, **CONFIGS[cfg], **kw)
    weightgen.fill_module_(m, "c2frv.")
    return m.eval()


def sampled(gold, key, t):
    a = t.detach().reshape(-1).cpu().double().numpy()
    return a[weightgen.sample_index(key, a.size, 4096)]


def check_maps(gold, cfg, maps, rel, what):
    for name in MAPS:
        ref = gold[f"{cfg}_{name}"].astype(np.float64)
        got = sampled(gold, f"{cfg}_{name}", maps[name])
        err = np.abs(got - ref).max()
        bar = rel * float(gold[f"{cfg}_{name}_maxabs"])
        print(f"{what} [{cfg}] {name}: max-abs err {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (cfg, name, err, bar)


def frames():
    return weightgen.synthetic_frames(3, 1, 128, 192)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_state_dict_matches_reference_key_for_key(gold, cfg):
    m = build(cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == list(gold[cfg + "_keys"])
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == list(gold[cfg + "_shapes"])
    # a reference-shaped checkpoint (the same keys / shapes, in the reference's order) loads strictly
    ref_sd = {k: weightgen.make_tensor("ckpt." + k, tuple(int(x) for x in s.split(",") if x), sd[k].dtype)
              for k, s in zip(gold[cfg + "_keys"], gold[cfg + "_shapes"])}
    m.load_state_dict(ref_sd, strict=True)


def test_registered_and_config_fields():
    from nndepth_amd.raft_stereo import STEREO_MODELS, BaseRAFTStereo, Coarse2FineGroupRepViTRAFTStereo
    assert STEREO_MODELS["coarse2fine"] is Coarse2FineGroupRepViTRAFTStereo
    assert STEREO_MODELS["base-raft-stereo"] is BaseRAFTStereo
    # every field of the reference's RepViTRAFTStereoModelConfig (configs.py:11-47), corr_levels=1 as its assert requires
    cfg = dict(iters=12, fnet_dim=256, hidden_dim=128, context_dim=64, corr_levels=1, corr_radius=4, tracing=False,
               include_preprocessing=False, weights=None, strict_load=True, num_groups=4, downsample_ratios=[(2, 2)] * 4,
               ffn_exp_ratios=[1.0, 3.0, 3.0, 4.0], num_blocks_per_stage=[4, 4, 6, 2], patch_size=7,
               stem_strides=[(2, 2), (2, 2), (1, 1)], token_mixer_types=["repmixer", "repmixer", "repmixer", "attention"])
    m = Coarse2FineGroupRepViTRAFTStereo(**cfg)
    assert m.cnet_proj[0].out_channels == 128 and m.hip_encoder


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_containers_forward_matches_reference(gold, cfg):
    from nndepth_amd.raft_stereo import Coarse2FineRAFTStereoBase
    m = build(cfg, hip_encoder=False)
    f1, f2 = frames()
    with torch.no_grad():
        fnet = m.fnet(torch.cat([f1, f2], 0))
        feats, cnets = Coarse2FineRAFTStereoBase.forward_features(m, f1, f2)
    maps = {f"fnet{i}": t for i, t in enumerate(fnet)}
    maps.update(fused1=feats[1], fused2=feats[2], cnet0=cnets[0], cnet1=cnets[1], cnet2=cnets[2])
    assert torch.equal(feats[0], fnet[4])
    check_maps(gold, cfg, maps, 1e-6, "containers")


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_host_fold_reproduces_reference(gold, cfg):
    from nndepth_amd.ops import RepViTEngine
    m = build(cfg)
    desc = RepViTEngine.descriptor(m.fnet, m.cnet_proj, m.fusion_blocks)
    layers = RepViTEngine.fold(m.fnet, m.cnet_proj, m.fusion_blocks)
    assert 3 * len(layers) == RepViTEngine.__init__.__globals__["lib"].nnd_repvit_num_tensors(C.byref(desc))
    f1, f2 = frames()
    with torch.no_grad():
        feats, cnets, fnet = RepViTEngine.fold_forward(layers, desc, f1, f2)
    maps = {f"fnet{i}": t for i, t in enumerate(fnet)}
    maps.update(fused1=feats[1], fused2=feats[2], cnet0=cnets[0], cnet1=cnets[1], cnet2=cnets[2])
    check_maps(gold, cfg, maps, 1e-5, "host fold")


def test_cabi_refuses_bad_descriptors_before_any_launch():
    from nndepth_amd._lib import RepViTDesc, lib
    from nndepth_amd.ops import RepViTEngine
    m = build("default")
    d = RepViTEngine.descriptor(m.fnet, m.cnet_proj, m.fusion_blocks)
    assert lib.nnd_repvit_num_tensors(C.byref(d)) > 0 and lib.nnd_repvit_packed_floats(C.byref(d)) > 0
    assert lib.nnd_repvit_workspace_floats(C.byref(d), 2, 64, 96) > 0
    bad = RepViTDesc.from_buffer_copy(d)
    bad.struct_size = 8
    assert lib.nnd_repvit_num_tensors(C.byref(bad)) < 0
    assert b"struct_size" in lib.nnd_last_error()
    bad = RepViTDesc.from_buffer_copy(d)
    bad.down_strides[1] = 3
    assert lib.nnd_repvit_packed_floats(C.byref(bad)) < 0
    assert b"stride" in lib.nnd_last_error()
    bad = RepViTDesc.from_buffer_copy(d)
    bad.patch_size = 6
    assert lib.nnd_repvit_workspace_floats(C.byref(bad), 2, 64, 96) < 0
    assert b"patch_size" in lib.nnd_last_error()
    # forward refuses the descriptor before touching any pointer (all NULL here)
    bad = RepViTDesc.from_buffer_copy(d)
    bad.stem_strides[0] = 4
    assert lib.nnd_repvit_forward(C.byref(bad), None, None, None, 1, None, None, None, None, None, None, None, 2, 64, 96, None) < 0


# (num_tensors, packed_floats, SHA-256 of the packed blob) per configuration, as the commit before the encoder sides moved onto one
# layer plan (csrc/enc_plan.h) produced them (weightgen 'c2frv.')
PLAN_PINS = {
    "default": (180, 2360064, "5524dfda1bc9454f95abfafd7806332c17af8588a129952aae48f0959997c3d2"),
    "alt": (102, 952576, "b456ea84952f89ebbe8ed2f47309f2b183643224035132c738c4d2158f3dbc87"),
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_repvit_plan_and_pack_unchanged(cfg):
    """nnd_repvit_* build their plan and pack through the code they share with nnd_mbv3_* and nnd_midas_* (csrc/enc_plan.h).  Sizes
    and the SHA-256 of the packed blob are the values of the commit before that refactor (PLAN_PINS; the workspace and the
    single-layer sizes are the same for both configurations)."""
    from nndepth_amd._lib import lib
    from nndepth_amd.ops import RepViTEngine
    m = build(cfg)
    d = RepViTEngine.descriptor(m.fnet, m.cnet_proj, m.fusion_blocks)
    n, floats, sha = PLAN_PINS[cfg]
    assert lib.nnd_repvit_num_tensors(C.byref(d)) == n
    assert lib.nnd_repvit_packed_floats(C.byref(d)) == floats
    assert lib.nnd_repvit_workspace_floats(C.byref(d), 2, 64, 96) == 215296
    assert lib.nnd_repvit_workspace_floats(C.byref(d), 2, 512, 960) == 17218560
    assert lib.nnd_repvit_pointwise_packed_floats(192, 64, 1) == 12672
    assert lib.nnd_repvit_pointwise_packed_floats(16, 16, 2) == 576
    eng = RepViTEngine(d, RepViTEngine.fold(m.fnet, m.cnet_proj, m.fusion_blocks), "cpu")
    assert hashlib.sha256(eng.packed.numpy().tobytes()).hexdigest() == sha


def test_python_side_names_what_it_refuses():
    from nndepth_amd._lib import NndError
    from nndepth_amd.ops import RepViTEngine
    from nndepth_amd.raft_stereo import patch_coarse2fine
    m = build("default")
    assert RepViTEngine.blocker(m, m.fnet, m.cnet_proj, m.fusion_blocks) is None
    # a reparameterised token mixer
    tm = m.fnet.stage_0[1][0].token_mixer
    tm.reparam_conv = torch.nn.Conv2d(32, 32, 3, padding=1, groups=32)
    why = RepViTEngine.blocker(m, m.fnet, m.cnet_proj, m.fusion_blocks)
    assert "reparam_conv" in why and "stage_0.1.0.token_mixer" in why
    del tm.reparam_conv
    # strides other than (1, 1) / (2, 2), even patch sizes, training mode
    m2 = build("default", stem_strides=[(2, 2), (2, 1), (1, 1)])
    assert "(2, 1)" in RepViTEngine.blocker(m2, m2.fnet, m2.cnet_proj, m2.fusion_blocks)
    m3 = build("default", patch_size=6)
    assert "patch_size 6" in RepViTEngine.blocker(m3, m3.fnet, m3.cnet_proj, m3.fusion_blocks)
    m.train()
    assert "training" in RepViTEngine.blocker(m, m.fnet, m.cnet_proj, m.fusion_blocks)
    with pytest.raises(NndError, match="inference-only"):
        m(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
    # the HIP path refuses a CPU run through the engine's device check, never falls back
    m.eval()
    with pytest.raises(NndError):
        m(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))
    import inspect
    assert inspect.signature(patch_coarse2fine).parameters["hip_encoder"].default is False
