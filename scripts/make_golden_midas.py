"""Fixture of MobileNetV3DepthModel (tests/golden/midas_mbnet.npz, REPORT_midas.txt).

Runs only where the reference checkout is importable (like scripts/make_golden_igev_mbnet.py; it installs the stand-ins of
oracle/make_golden.py and changes nothing under oracle/).  timm is not available, so the stand-in of
timm.models.mobilenetv3.tf_mobilenetv3_large_100 returns nndepth_amd.mobilenetv3.MobileNetV3Features: the reference's own
MobileNetV3DepthModel, MobilenetV3LargeEncoder (hooks 1, 2, 4, 5), BaseDecoder, UpsamplerBlock and last_conv run around it.
Weights: nndepth_amd.weightgen.fill_module_(model, "midas.") — not stored, the tests regenerate them.
Frame: weightgen.synthetic_frames(7, 1, 128, 192)[0].  Stored (fp32 on the CPU, each map at weightgen.sample_index(<map>, numel,
SAMPLE), with <map>_maxabs and <map>_err64 = max |fp32 - float64| of the same reference forward run in float64):
  keys / shapes                 the reference class' state_dict key list (in order) with shapes
  tap0..tap3, decoder           the encoder's four maps and the decoder's output — they do not depend on last_conv.4.bias
  pre_relu, depth               the map before the final ReLU and the output with the GENERATED last_conv.4.bias (-0.045: most of
                                the output is clamped to zero, so `depth` alone would pass on almost anything)
  pre_relu_shift, depth_shift   the same with last_conv.4.bias = SHIFT_BIAS: no element is clamped (asserted here: at most 1 % zeros)

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_midas.py [path of the reference checkout; default: oracle's]
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
SHIFT_BIAS = 0.0107


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
    from nndepth.models.midas.models.mobilenet_v3 import MobileNetV3DepthModel

    x = weightgen.synthetic_frames(7, 1, H, W)[0]
    out = {}
    rep = ["MobileNetV3DepthModel, the reference class on the nndepth_amd.mobilenetv3 containers (scripts/make_golden_midas.py)",
           f"weights weightgen.fill_module_(model, 'midas.'), frame synthetic_frames(7, 1, {H}, {W})[0], default kwargs; every map stored "
           f"at weightgen.sample_index ({SAMPLE} elements)"]

    torch.manual_seed(0)
    model = MobileNetV3DepthModel()
    weightgen.fill_module_(model, "midas.")
    model.eval()
    sd = model.state_dict()
    out["keys"] = np.array(list(sd.keys()))
    out["shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    rep.append(f"{len(sd)} state_dict keys ({sum(p.numel() for p in model.parameters()) / 1e6:.2f} M parameters), "
               f"generated last_conv.4.bias {model.last_conv[4].bias.item():+.4f}")

    def run(m, inp):
        with torch.no_grad():
            taps = m.forward_encoder(inp)
            dec = m.forward_decoder(taps)
            pre = m.last_conv[:5](dec)
            depth = m.last_conv(dec)
        assert torch.equal(depth, m(inp))
        r = {f"tap{i}": t for i, t in enumerate(taps)}
        r.update(decoder=dec, pre_relu=pre, depth=depth)
        return r

    def put(key, t, t64):
        a = t.detach().reshape(-1).numpy().astype(np.float32)
        out[key] = a[weightgen.sample_index(key, a.size, SAMPLE)]
        err, mx = (t.double() - t64).abs().max().item(), t.abs().max().item()
        out[f"{key}_maxabs"] = np.float64(mx)
        out[f"{key}_err64"] = np.float64(err)
        zeros = (t == 0).double().mean().item()
        rep.append(f"  {key:15s} {tuple(t.shape)!s:18s} range [{t.min():+.4f}, {t.max():+.4f}]   fp32-CPU vs float64 {err:.3e} "
                   f"({err / mx:.1e} rel)   exact zeros {100 * zeros:.1f} %")
        return zeros

    r32 = run(model, x)
    r64 = run(model.double(), x.double())
    model.float()
    for k in r32:
        put(k, r32[k], r64[k])
    with torch.no_grad():
        model.last_conv[4].bias.fill_(SHIFT_BIAS)
    s32 = run(model, x)
    s64 = run(model.double(), x.double())
    rep.append(f"last_conv.4.bias = {SHIFT_BIAS:+.4f}:")
    for k in ("pre_relu", "depth"):
        zeros = put(k + "_shift", s32[k], s64[k])
        assert zeros <= 0.01, (k, zeros)
    out["shift_bias"] = np.float64(SHIFT_BIAS)
    path = os.path.join(GOLD, "midas_mbnet.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    with open(os.path.join(GOLD, "REPORT_midas.txt"), "w") as f:
        f.write("\n".join(rep) + "\n")
    print("\n".join(rep))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
