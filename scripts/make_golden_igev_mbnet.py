"""Fixture of IGEVStereoMBNet (tests/golden/igev_mbnet.npz, REPORT_igev_mbnet.txt).

Runs only where the reference checkout is importable (like oracle/make_golden*.py; it installs the stand-ins of
oracle/make_golden.py and changes nothing under oracle/).  timm is not available, so the stand-in of
timm.models.mobilenetv3.tf_mobilenetv3_large_100 returns nndepth_amd.mobilenetv3.MobileNetV3Features: the reference's own
IGEVStereoMBNet, MobilenetV3LargeEncoder (conv_stem -> bn1 -> act1 -> every stage, hooks 1..5), forward_fnet, volume, regulariser
and loop run around it.  Weights: nndepth_amd.weightgen.fill_module_(model, "igevmb.") — not stored, the tests regenerate them.
Frames: weightgen.synthetic_frames(7, 1, 128, 192).  Stored:
  keys / shapes                 the reference class' state_dict key list (in order) with shapes
  <map>                         fmap1, fmap2, cnet1, guide0..2 (forward_fnet's outputs), fp32 on the CPU; maps larger than SAMPLE
                                elements are stored at weightgen.sample_index(<map>, numel, SAMPLE) only
  <map>_maxabs / _err64         max |map| and max |fp32 - float64| of the same reference forward_fnet run in float64
  stage<i>_maxabs               max |x| of backbone stage i's output (both frames), i = 0..6
  up0..up3 (+ _maxabs)          the reference's full forward with iters=4, sampled the same way

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_igev_mbnet.py [path of the reference checkout; default: oracle's]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
SAMPLE = 4096
H, W = 128, 192
MAPS = ["fmap1", "fmap2", "cnet1", "guide0", "guide1", "guide2"]


def main(ref_path: str):
    from nndepth_amd import weightgen
    from nndepth_amd.mobilenetv3 import MobileNetV3Features
    import oracle.make_golden as mg
    if ref_path:
        mg.REF = ref_path
    mg._install_standins()

    def tf_mobilenetv3_large_100(pretrained=False, features_only=False, **kw):
        assert features_only and not kw, kw
        return MobileNetV3Features()  # pretrained: the generated weights below replace whatever it would load

    sys.modules["timm.models.mobilenetv3"].tf_mobilenetv3_large_100 = tf_mobilenetv3_large_100
    from nndepth.models.igev_stereo import STEREO_MODELS
    from nndepth.models.igev_stereo.model import IGEVStereoMBNet
    assert STEREO_MODELS["igev_stereo_mbnet"] is IGEVStereoMBNet

    f1, f2 = weightgen.synthetic_frames(7, 1, H, W)
    out = {}
    rep = ["IGEVStereoMBNet, the reference class on the nndepth_amd.mobilenetv3 containers (scripts/make_golden_igev_mbnet.py)",
           f"weights weightgen.fill_module_(model, 'igevmb.'), frames synthetic_frames(7, 1, {H}, {W}), default kwargs + iters=4; "
           f"maps > {SAMPLE} elements stored at weightgen.sample_index only"]

    def put(key, t):
        a = t.detach().reshape(-1).numpy().astype(np.float32)
        out[key] = a[weightgen.sample_index(key, a.size, SAMPLE)]

    torch.manual_seed(0)
    model = IGEVStereoMBNet(iters=4)
    weightgen.fill_module_(model, "igevmb.")
    model.eval()
    sd = model.state_dict()
    out["keys"] = np.array(list(sd.keys()))
    out["shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    n_bb = sum(1 for k in sd if k.startswith("fnet."))
    rep.append(f"{len(sd)} state_dict keys, {n_bb} in fnet.backbone "
               f"({sum(v.numel() for k, v in model.named_parameters() if k.startswith('fnet.')) / 1e6:.2f} M parameters)")

    stages = {}

    def hook(i):
        def fn(mod, inp, outp):
            stages[i] = max(stages.get(i, 0.0), outp.detach().abs().max().item())
        return fn

    handles = [blk.register_forward_hook(hook(i)) for i, blk in enumerate(model.fnet.backbone.blocks)]
    with torch.no_grad():
        maps = dict(zip(MAPS[:3], model.forward_fnet(f1, f2)[:3]))
        maps.update(zip(MAPS[3:], model.forward_fnet(f1, f2)[3]))
    for h in handles:
        h.remove()
    stem = model.fnet.backbone.act1(model.fnet.backbone.bn1(model.fnet.backbone.conv_stem(torch.cat([f1, f2])))).abs().max().item()
    rep.append(f"  max |x| through the backbone: stem {stem:.3f}, " + ", ".join(f"stage {i} {stages[i]:.3f}" for i in sorted(stages)))
    for i in sorted(stages):
        out[f"stage{i}_maxabs"] = np.float64(stages[i])
    with torch.no_grad():
        m64 = model.double()
        r = m64.forward_fnet(f1.double(), f2.double())
        maps64 = dict(zip(MAPS[:3], r[:3]))
        maps64.update(zip(MAPS[3:], r[3]))
    model.float()
    for name, t in maps.items():
        err = (t.double() - maps64[name]).abs().max().item()
        mx = t.abs().max().item()
        put(name, t)
        out[f"{name}_maxabs"] = np.float64(mx)
        out[f"{name}_err64"] = np.float64(err)
        rep.append(f"  {name:7s} {tuple(t.shape)!s:18s} max-abs {mx:9.4f}   fp32-CPU vs float64 {err:.3e} ({err / mx:.1e} rel)")
    with torch.no_grad():
        ups = [o["up_disp"] for o in model(f1, f2)]
    assert len(ups) == 4
    for i, u in enumerate(ups):
        put(f"up{i}", u)
        out[f"up{i}_maxabs"] = np.float64(u.abs().max().item())
    rep.append(f"  forward iters=4: {len(ups)} up_disp {tuple(ups[-1].shape)}, final max-abs {ups[-1].abs().max():.3f}, "
               f"range [{ups[-1].min():.3f}, {ups[-1].max():.3f}]")
    np.savez_compressed(os.path.join(GOLD, "igev_mbnet.npz"), **out)
    with open(os.path.join(GOLD, "REPORT_igev_mbnet.txt"), "w") as f:
        f.write("\n".join(rep) + "\n")
    print("\n".join(rep))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
