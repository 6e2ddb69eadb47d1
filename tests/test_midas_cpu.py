"""MobileNetV3DepthModel drop-in class without a GPU: state_dict layout against the reference class (tests/golden/midas_mbnet.npz,
scripts/make_golden_midas.py), the `weights=` round trip, DEPTH_MODELS, the host fold (ops.MidasEngine.fold) in float64, the
explicit PyTorch path against the fixture, the refusals of the C-ABI / Python side, and the unchanged nnd_mbv3_* plan."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from nndepth_amd import weightgen

GOLD = os.path.join(os.path.dirname(__file__), "golden", "midas_mbnet.npz")
MAPS = ["tap0", "tap1", "tap2", "tap3", "decoder", "pre_relu", "depth"]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def build(**kw):
    from nndepth_amd.midas import MobileNetV3DepthModel
    m = MobileNetV3DepthModel(**kw)
    weightgen.fill_module_(m, "midas.")
    return m.eval()


def test_state_dict_matches_reference_key_for_key(gold):
    sd = build().state_dict()
    assert list(sd.keys()) == gold["keys"].tolist()
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == gold["shapes"].tolist()
    keys = list(sd.keys())
    assert keys[0] == "encoder.backbone.conv_stem.weight" and keys[-1] == "last_conv.4.bias"
    assert "decoder.skip_layers.3.0.weight" in sd and "decoder.upsampler_layers.3.conv1.weight" in sd
    assert "decoder.upsampler_layers.0.bn2.running_var" in sd and tuple(sd["last_conv.4.weight"].shape) == (1, 64, 1, 1)


def test_registered_and_constructor():
    from nndepth_amd.midas import DEPTH_MODELS, MobileNetV3DepthModel
    assert DEPTH_MODELS == {"mbnet_v3": MobileNetV3DepthModel}
    m = MobileNetV3DepthModel(feature_channels=32, weights=None, strict_load=True)
    assert m.hip and tuple(m.state_dict()["decoder.skip_layers.2.0.weight"].shape) == (32, 112, 3, 3)


def test_weights_load_through_constructor(tmp_path):
    from nndepth_amd.midas import MobileNetV3DepthModel
    src = build()
    path = str(tmp_path / "midas.pth")
    torch.save(src.state_dict(), path)
    m = MobileNetV3DepthModel(weights=path, strict_load=True)
    for (k, a), b in zip(m.state_dict().items(), src.state_dict().values()):
        assert torch.equal(a, b), k
    sd = src.state_dict()
    del sd["last_conv.4.bias"]
    torch.save(sd, path)
    with pytest.raises(RuntimeError, match="last_conv.4.bias"):
        MobileNetV3DepthModel(weights=path)
    MobileNetV3DepthModel(weights=path, strict_load=False)
    with pytest.raises(ValueError, match="Unsupported weight format"):
        MobileNetV3DepthModel(weights=str(tmp_path / "midas.ckpt"))


def test_host_fold_reproduces_module_forward_in_float64():
    from nndepth_amd.ops import MidasEngine
    m = build().double()
    x = weightgen.synthetic_frames(3, 2, 64, 96)[0].double()
    with torch.no_grad():
        ref = m.forward_torch(x)
        layers = MidasEngine.fold(m)
        got = MidasEngine.fold_forward(layers, x)
    # 15 blocks' layers + stem, 4 skip convs, 3 + 3 + 3 + 2 block convs (block 3 has no conv1), 3 of last_conv
    assert [l["kind"] for l in layers[-18:]] == ["skip"] * 4 + ["up_conv1", "up_conv2", "up_out"] * 3 + ["up_conv2", "up_out", "last0",
                                                                                                     "last2", "last4"]
    for name in MAPS:
        err, mx = (got[name] - ref[name]).abs().max().item(), ref[name].abs().max().item()
        assert err <= 1e-13 * max(mx, 1.0), (name, err)


def test_hip_false_matches_reference_fixture(gold):
    x = weightgen.synthetic_frames(7, 1, 128, 192)[0]
    for shift in (False, True):
        m = build(hip=False)
        if shift:
            with torch.no_grad():
                m.last_conv[4].bias.fill_(float(gold["shift_bias"]))
        with torch.no_grad():
            r = m.forward_torch(x)
            assert torch.equal(m(x), r["depth"])
        for name in MAPS:
            key = name + "_shift" if shift and name in ("pre_relu", "depth") else name
            a = r[name].reshape(-1).double().numpy()
            err = np.abs(a[weightgen.sample_index(key, a.size, 4096)] - gold[key]).max()
            bar = 4.0 * float(gold[key + "_err64"]) + 1e-7 * float(gold[key + "_maxabs"])  # CPU fp32 drift across machines
            assert err <= bar, (key, err, bar)
    assert (gold["depth_shift"] == 0).mean() <= 0.01 and (gold["depth"] == 0).mean() > 0.5


def test_cabi_refuses_bad_descriptors_before_any_launch():
    from nndepth_amd._lib import MidasDesc, lib
    d = MidasDesc(feature_channels=64, flags=0)
    n = lib.nnd_midas_num_tensors(C.byref(d))
    assert n == 2 * (63 - 2 + 4 + 11 + 3) and lib.nnd_midas_packed_floats(C.byref(d)) > 0  # nnd_mbv3's 63 layers hold two projections
    assert lib.nnd_midas_workspace_floats(C.byref(d), 1, 64, 96) > 0
    bad = MidasDesc.from_buffer_copy(d)
    bad.struct_size = 8
    assert lib.nnd_midas_num_tensors(C.byref(bad)) < 0
    assert b"struct_size" in lib.nnd_last_error()
    bad = MidasDesc.from_buffer_copy(d)
    bad.flags = 2
    assert lib.nnd_midas_packed_floats(C.byref(bad)) < 0 and b"flags" in lib.nnd_last_error()
    for c in (0, 24, 256):
        bad = MidasDesc.from_buffer_copy(d)
        bad.feature_channels = c
        assert lib.nnd_midas_forward(C.byref(bad), None, None, None, None, 1, 64, 96, None) < 0
        assert b"feature_channels" in lib.nnd_last_error() and str(c).encode() in lib.nnd_last_error()
    for hw in ((72, 96), (64, 100)):
        assert lib.nnd_midas_workspace_floats(C.byref(d), 1, *hw) < 0
        assert b"multiples of 32" in lib.nnd_last_error()
        # non-null pointers that are never dereferenced: the size is refused before any launch
        buf = torch.zeros(8)
        p = C.c_void_p(buf.data_ptr())
        assert lib.nnd_midas_forward(C.byref(d), p, p, p, p, 1, *hw, None) < 0
        assert b"multiples of 32" in lib.nnd_last_error()
    assert lib.nnd_midas_forward(C.byref(d), None, None, None, None, 1, 64, 96, None) < 0
    assert b"null" in lib.nnd_last_error()
    assert lib.nnd_midas_head_packed_floats(24) < 0 and b"24" in lib.nnd_last_error()
    assert lib.nnd_midas_up2x_pw_packed_floats(64, 200) < 0
    assert lib.nnd_midas_head(64, None, None, None, None, 1, 8, 8, None) < 0
    assert lib.nnd_midas_conv_add(64, 64, 5, None, None, None, None, 1, 8, 8, None) < 0


def test_python_side_names_what_it_refuses():
    from nndepth_amd._lib import NndError
    from nndepth_amd.ops import MidasEngine
    m = build()
    assert MidasEngine.descriptor(m).feature_channels == 64
    with pytest.raises(NndError, match="multiples of 32"):
        m(torch.zeros(1, 3, 72, 96))
    with pytest.raises(NndError, match="HIP device only"):  # the HIP path refuses a CPU run, never falls back
        m(torch.zeros(1, 3, 64, 96))
    m.train()
    with pytest.raises(NndError, match="inference-only"):
        m(torch.zeros(1, 3, 64, 96))
    m.eval()
    with pytest.raises(NndError, match="feature_channels"):
        MidasEngine.descriptor(build(feature_channels=24))
    m.last_conv[1] = torch.nn.Identity()
    with pytest.raises(NndError, match="last_conv"):
        MidasEngine.descriptor(m)
    m2 = build()
    m2.encoder.feature_hooks = [1, 2, 3, 4, 5]
    with pytest.raises(NndError, match="feature_hooks"):
        MidasEngine.descriptor(m2)


def test_mbv3_plan_and_pack_unchanged():
    """nnd_mbv3_* share their backbone code with nnd_midas_* now.  Sizes and the SHA-256 of the packed blob as the commit before the
    MiDaS model produced them (IGEVStereoMBNet defaults, weightgen 'igevmb.')."""
    from nndepth_amd._lib import MobileNetV3Desc, lib
    from nndepth_amd.igev_stereo import IGEVStereoMBNet
    from nndepth_amd.ops import MobileNetV3Engine
    d = MobileNetV3Desc(fnet_dim=256, cnet_dim=256, flags=0)
    assert lib.nnd_mbv3_num_tensors(C.byref(d)) == 126
    assert lib.nnd_mbv3_packed_floats(C.byref(d)) == 3032576
    assert lib.nnd_mbv3_workspace_floats(C.byref(d), 1, 64, 96) == 371520
    assert lib.nnd_mbv3_workspace_floats(C.byref(d), 2, 544, 960) == 62692224
    assert lib.nnd_mbv3_pointwise_packed_floats(64, 24, 3) == 18560
    assert lib.nnd_mbv3_pointwise_packed_floats(160, 960, 1) == 153920
    m = IGEVStereoMBNet(iters=4)
    weightgen.fill_module_(m, "igevmb.")
    m.eval()
    eng = MobileNetV3Engine(d, MobileNetV3Engine.fold(m.fnet, m.fnet_proj, m.cnet_proj), "cpu")
    assert hashlib.sha256(eng.packed.numpy().tobytes()).hexdigest() == "085ceb81451f949d1efa6a84d83b2279d41495ed25603b26befbdc4f019811aa"


def test_midas_plan_and_pack_unchanged():
    """nnd_midas_* build their plan, pack and size their workspace through the code they share with nnd_repvit_* and nnd_mbv3_*
    (csrc/enc_plan.h, mbv3.hip's one backbone walk).  Sizes, offsets and the SHA-256 of the packed blob as the commit before that
    refactor produced them (the model of build(), weightgen 'midas.')."""
    from nndepth_amd._lib import lib
    from nndepth_amd.ops import MidasEngine
    m = build()
    d = MidasEngine.descriptor(m)
    assert lib.nnd_midas_num_tensors(C.byref(d)) == 158
    assert lib.nnd_midas_packed_floats(C.byref(d)) == 3483584
    assert lib.nnd_midas_workspace_floats(C.byref(d), 1, 64, 96) == 511488
    assert lib.nnd_midas_workspace_floats(C.byref(d), 2, 544, 960) == 86486784
    assert [lib.nnd_midas_workspace_offset(C.byref(d), i, 1, 64, 96) for i in range(6)] == [0, 9216, 13056, 15744, 130752, 327360]
    assert lib.nnd_midas_up2x_pw_packed_floats(64, 64) == 4160
    assert lib.nnd_midas_head_packed_floats(64) == 36993
    eng = MidasEngine(d, MidasEngine.fold(m), "cpu")
    assert hashlib.sha256(eng.packed.numpy().tobytes()).hexdigest() == "34c3c9fed865fa83cd8a0bfa5912a9d8dadb1ae6b5484611aea9482cc273ab1a"
