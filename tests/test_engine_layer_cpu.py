"""CPU: the Python layer over the engines where no GPU is needed — the one repack-on-change cache (ops.ParamCache), the update
block's repack through it, and the per-call descriptors (ops._call_desc): an engine's own `desc` is never written by a call."""
import contextlib
import glob
import os
import re
import threading

import torch
import torch.nn as nn


def _module():
    from nndepth_amd import weightgen
    m = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Sequential(nn.Conv2d(4, 4, 1)))
    return weightgen.fill_module_(m, "cache.").eval()


def test_param_cache_rebuilds_on_each_trigger_and_not_otherwise():
    from nndepth_amd import ops
    m, cache, built = _module(), ops.ParamCache(), []

    def get(device="cuda:0", extra=(), track=False):
        return cache.get((m,), device, lambda: built.append(len(built)) or len(built), extra, track)

    assert get() == 1 and get() == 1 and built == [0]
    m.train().eval()  # neither a parameter nor a buffer
    assert get() == 1 and get(torch.device("cuda:0")) == 1
    with torch.no_grad():
        m[0].weight.mul_(2)  # in-place parameter edit: _version
    assert get() == 2 and get() == 2
    m[0].bias.data = m[0].bias.data.clone()  # .data replacement: data_ptr
    assert get() == 3 and get() == 3
    m[1].running_mean.add_(1)  # a buffer edit
    assert get() == 4 and get() == 4
    assert get("cuda:1") == 5 and get("cuda:1") == 5  # device string
    assert get("cuda:1", extra=("bf16x3",)) == 6 and get("cuda:1", extra=("bf16x3",)) == 6  # extra
    # a replaced submodule that holds the same parameters: seen only with track_modules
    assert get(track=True) == 7 and get(track=True) == 7
    old, new = m[2][0], nn.Conv2d(4, 4, 1)
    new.weight, new.bias = old.weight, old.bias
    m[2][0] = new
    assert get(track=True) == 8 and get(track=True) == 8
    assert get() == 9  # (track_modules itself is part of the key)
    m[2][0] = old
    assert get() == 9 and len(built) == 9


def test_param_cache_keeps_its_state_when_build_raises():
    from nndepth_amd import ops
    m, cache = _module(), ops.ParamCache()
    assert cache.get((m,), "cpu", lambda: "first") == "first"
    with torch.no_grad():
        m[0].weight.add_(1)

    def fails():
        raise RuntimeError("blocked")
    for _ in range(2):  # asked again on every call until a build succeeds
        try:
            cache.get((m,), "cpu", fails)
            raise AssertionError("build() was not called")
        except RuntimeError:
            pass
    assert cache.get((m,), "cpu", lambda: "second") == "second"


def test_update_block_repacks_when_a_parameter_changes():
    from nndepth_amd import weightgen
    from nndepth_amd.blocks import BasicUpdateBlock
    ub = BasicUpdateBlock(hidden_dim=128, cor_planes=36, context_dim=64, flow_channel=1, spatial_scale=8, arithmetic="fp16x2")
    weightgen.fill_module_(ub, "u.")
    eng = ub.sync_engine("cpu")
    blob = eng.packed
    assert eng is ub.engine and ub.sync_engine("cpu").packed is blob
    eng.calibrated = True
    with torch.no_grad():
        next(ub.parameters()).mul_(2)
    eng = ub.sync_engine("cpu")
    assert eng is ub.engine and eng.packed is not blob and not torch.equal(eng.packed, blob)
    assert eng.calibrated is False  # a fresh blob carries the default activation scales
    assert ub.sync_engine("cpu").packed is eng.packed


def _fp16x2_engines(device="cpu"):
    """An fp16x2 UpdateBlockEngine, EncoderEngine and Conv3dNorm on seeded weightgen parameters."""
    from nndepth_amd import ops, weightgen
    from nndepth_amd.encoder import BasicEncoder
    from oracle import torch_ref as R
    ub = ops.UpdateBlockEngine(128, 64, 36, 1, 576, "sep_conv", "fp16x2")
    ub.load(weightgen.fill_state_dict(R.update_block_spec("u", 128, 36, 64, 1, 8)), "u.", device=device)
    fnet = weightgen.fill_module_(BasicEncoder(output_dim=256), "fnet.")
    enc = ops.EncoderEngine(256, "batch", 0, "fp16x2").load(fnet.state_dict(), device=device)
    bn = tuple(weightgen.make_tensor(f"c3.bn.{k}", (16,)) for k in ("weight", "bias", "running_mean", "running_var"))
    c3 = ops.Conv3dNorm(weightgen.make_tensor("c3.conv.weight", (16, 8, 3, 3, 3)), None, 1, bn, device=device, arithmetic="fp16x2")
    return ub, enc, c3


def test_call_descriptor_carries_the_flags_the_engine_descriptor_never(monkeypatch):
    from nndepth_amd import _lib, ops
    # leaving `ops.calibration()` fixes the scales on the device (`_calibration_finish` under torch.cuda.device): these engines
    # are loaded on the CPU, so in this test only both are replaced by no-ops
    monkeypatch.setattr(ops.torch.cuda, "device", lambda d: contextlib.nullcontext())
    for eng in _fp16x2_engines():
        eng._calibration_finish = lambda status: None
        assert eng.desc.flags == 0 and ops._call_desc(eng).flags == 0
        other = {}
        with ops.calibration():
            d = ops._call_desc(eng)
            t = threading.Thread(target=lambda: other.update(flags=ops._call_desc(eng).flags))  # another thread, the same moment
            t.start()
            t.join()
            assert d.flags & _lib.NND_FLAG_CALIBRATE == 1 and eng.desc.flags == 0
            assert other["flags"] == 0
            assert type(d) is type(eng.desc) and d is not eng.desc and d.struct_size == eng.desc.struct_size
        assert eng.desc.flags == 0 and eng.calibrated is True
        assert ops._call_desc(eng).flags == 0
        assert ops._call_desc(eng, _lib.NND_FLAG_LAST_UPSAMPLE_ONLY).flags == 2 and eng.desc.flags == 0


def test_no_code_assigns_desc_flags():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nndepth_amd")
    files = sorted(glob.glob(os.path.join(root, "*.py")))
    assert len(files) > 10
    pat = re.compile(r"\.desc\.flags\s*=(?!=)")
    hits = [f"{os.path.basename(f)}:{i}" for f in files for i, line in enumerate(open(f), 1) if pat.search(line)]
    assert hits == []
