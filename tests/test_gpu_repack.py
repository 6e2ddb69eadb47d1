"""GPU: a model repacks what it cached when a parameter is edited in place — the next forward equals, bit for bit, that of a freshly
constructed model holding the edited parameters — for every cached group of the five model classes; a repacked fp16x2 engine is
uncalibrated until the next forward; and a call inside `ops.calibration()` leaves the engine's own descriptor untouched."""
import pytest
import torch

from nndepth_amd import weightgen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _raft(**kw):
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    return BaseRAFTStereo(iters=2, context_dim=64, **kw), "raft."


def _cre(**kw):
    from nndepth_amd.cre_stereo import CREStereoBase
    return CREStereoBase(iters=2, **kw), "cre."


def _igev(**kw):
    from nndepth_amd.igev_stereo import IGEVStereoMBNet
    return IGEVStereoMBNet(iters=2, **kw), "igevmb."


def _c2f(**kw):
    from nndepth_amd.raft_stereo import Coarse2FineGroupRepViTRAFTStereo
    return Coarse2FineGroupRepViTRAFTStereo(iters=2, corr_levels=1, **kw), "c2frv."


def _midas(**kw):
    from nndepth_amd.midas import MobileNetV3DepthModel
    return MobileNetV3DepthModel(feature_channels=64), "midas."


def _first_conv(module):
    return next(p for p in module.parameters() if p.dim() == 4)


UB = "update_block.encoder.convc1.weight"
# model -> (constructor, frame size: the smallest its own GPU tests use, one parameter of every cached group)
CASES = {
    "BaseRAFTStereo": (_raft, (96, 160), lambda m: [_first_conv(m.fnet), m.get_parameter(UB)]),
    "CREStereoBase": (_cre, (128, 192), lambda m: [_first_conv(m.fnet), m.get_parameter(UB), m.conv_offset_8.weight,
                                                   m.self_att_fn.layers[0].q_proj.weight]),
    "IGEVStereoMBNet": (_igev, (128, 192), lambda m: [_first_conv(m.fnet), m.get_parameter(UB), m.cv_regularizer.conv1[0].conv.weight,
                                                      m.cv_squeezer.weight]),
    "Coarse2FineGroupRepViTRAFTStereo": (_c2f, (128, 192), lambda m: [_first_conv(m.fnet), m.get_parameter(UB)]),
    "MobileNetV3DepthModel": (_midas, (128, 192), lambda m: [_first_conv(m.encoder), m.last_conv[2].weight]),
}


def _build(make, state=None, **kw):
    m, prefix = make(**kw)
    if state is None:
        weightgen.fill_module_(m, prefix)
    else:
        m.load_state_dict(state, strict=True)
    return m.to(DEV).eval()


def _run(m, frames):
    """Every tensor a forward returns (IGEV: and the loop's low-resolution state)."""
    out = m(*frames)
    maps = [out] if torch.is_tensor(out) else [o["up_disp"] for o in out]
    if hasattr(m, "last_low_coords"):
        maps.append(m.last_low_coords)
    return [t.clone() for t in maps]


def _edit(params):
    with torch.no_grad():
        for p in params:
            p.view(-1)[::2].mul_(0.5)  # every other element: no norm layer behind the conv can undo it


def _frames(name, hw):
    f = [x.to(DEV) for x in weightgen.synthetic_frames(5, 1, *hw)]
    return f[:1] if name == "MobileNetV3DepthModel" else f


@pytest.mark.parametrize("name", list(CASES))
def test_in_place_edit_is_repacked(name):
    make, hw, groups = CASES[name]
    frames = _frames(name, hw)
    kw = {} if name == "MobileNetV3DepthModel" else {"arithmetic": "fp32"}
    m = _build(make, **kw)
    first = _run(m, frames)
    assert all(torch.isfinite(t).all() for t in first)
    # one group at a time, so that a group that is not repacked cannot hide behind another that is
    for p in groups(m):
        _edit([p])
        second = _run(m, frames)
        assert any(not torch.equal(a, b) for a, b in zip(first, second)), name
        first = second
    fresh = _run(_build(make, state={k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, **kw), frames)
    assert len(fresh) == len(second) and all(torch.equal(a, b) for a, b in zip(fresh, second)), name


def test_repacked_fp16x2_engines_are_uncalibrated_until_the_next_forward():
    make, hw, groups = CASES["BaseRAFTStereo"]
    frames = _frames("BaseRAFTStereo", hw)
    m = _build(make, arithmetic="fp16x2")
    first = _run(m, frames)  # calibrates on its own input
    assert m.update_block.engine.calibrated and m._encoder_engine(DEV).calibrated
    _edit(groups(m))
    assert m.update_block.sync_engine(DEV).calibrated is False and m._encoder_engine(DEV).calibrated is False
    second = _run(m, frames)
    assert m.update_block.engine.calibrated is True and m._encoder_engine(DEV).calibrated is True
    assert not torch.equal(first[-1], second[-1])
    fresh = _run(_build(make, state={k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, arithmetic="fp16x2"), frames)
    assert all(torch.equal(a, b) for a, b in zip(fresh, second))


def test_calibrating_call_leaves_the_engine_descriptor_alone():
    from nndepth_amd import ops
    from test_engine_layer_cpu import _fp16x2_engines
    ub, enc, c3 = _fp16x2_engines(DEV)
    z = lambda *s: torch.from_numpy(weightgen.uniform01(f"repack{s}", int(torch.Size(s).numel()))).reshape(s).to(DEV) - 0.5  # noqa: E731
    calls = [(ub, lambda: ub.forward(z(1, 128, 8, 16), z(1, 64, 8, 16).relu(), z(1, 36, 8, 16), z(1, 1, 8, 16))),
             (enc, lambda: enc.forward(z(1, 3, 32, 64))),
             (c3, lambda: c3(ops.volume_to_depth_major(z(1, 8, 8, 8, 16))))]
    for eng, call in calls:
        assert not eng.calibrated
        with ops.calibration() as c:
            call()
            assert eng.desc.flags == 0  # the flag rode on this call's copy
        assert eng.desc.flags == 0 and eng.calibrated is True
        assert (c.status & 1) == 0
