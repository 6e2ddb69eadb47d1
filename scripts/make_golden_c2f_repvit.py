"""Fixture of the Coarse2FineGroupRepViTRAFTStereo encoder side (tests/golden/c2f_repvit.npz, REPORT_c2f_repvit.txt).

Runs only where the reference checkout is importable (like oracle/make_golden*.py; it imports the timm / loguru stand-ins of
oracle/make_golden.py and changes nothing under oracle/).  Weights: nndepth_amd.weightgen.fill_module_(model, "c2frv.") — not
stored, the tests regenerate them.  Frames: weightgen.synthetic_frames(3, 1, 128, 192) (stage 3 is then 2x3: W = 3 exercises the
per-row softmax of LinearSelfAttention).  For the default config and one non-default config:
  <cfg>_keys / <cfg>_shapes    the reference's state_dict key list (in order) with shapes
  <cfg>_<map>                  fnet0..fnet4 (RepViT outputs), fused1, fused2 (FeatureFusionBlocks), cnet0..cnet2 (cnet_proj on the
                               left frame), fp32 on the CPU; maps larger than SAMPLE elements are stored at
                               weightgen.sample_index(<cfg>_<map>, numel, SAMPLE) only
  <cfg>_<map>_maxabs / _err64  max |map| and max |fp32 - float64| of the same reference forward run in float64
and for the default config the reference's full forward with iters=4: up0..up11 (sampled the same way).

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_c2f_repvit.py [path of the reference checkout; default: oracle's]
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
# "default": the class defaults (context_dim = hidden_dim = 128: cnet_proj[0] is 256 -> 256 and has a skip BatchNorm);
# "alt": RepViTRAFTStereoModelConfig's context_dim = 64 with a non-default backbone
CONFIGS = {
    "default": dict(corr_levels=1),
    "alt": dict(corr_levels=1, context_dim=64, hidden_dim=64, num_blocks_per_stage=[1, 2, 1, 1],
                token_mixer_types=["repmixer", "attention", "repmixer", "attention"], use_ffn_per_stage=[True, True, False, True]),
}


def encoder_side(model, f1, f2):
    """The reference forward's encoder side (model.py:275-288), spelled out: RepViT outputs, fused maps, cnets."""
    B = f1.shape[0]
    fnet = model.fnet(torch.cat([f1, f2], 0))
    feats = fnet[::2][::-1]
    fused, cnets, prev = [], [], None
    for idx, feat in enumerate(feats):
        if prev is not None:
            feat = model.fusion_blocks[idx - 1]([prev, feat])
            fused.append(feat)
        cnets.append(model.cnet_proj[idx](feat[:B].clone()))
        prev = feat
    return dict([(f"fnet{i}", t) for i, t in enumerate(fnet)] + [(f"fused{i + 1}", t) for i, t in enumerate(fused)]
                + [(f"cnet{i}", t) for i, t in enumerate(cnets)])


def main(ref_path: str):
    from nndepth_amd import weightgen
    import oracle.make_golden as mg
    if ref_path:
        mg.REF = ref_path
    mg._install_standins()
    from nndepth.models.raft_stereo.model import Coarse2FineGroupRepViTRAFTStereo

    f1, f2 = weightgen.synthetic_frames(3, 1, H, W)
    out, rep = {}, ["Coarse2FineGroupRepViTRAFTStereo encoder side (scripts/make_golden_c2f_repvit.py)",
                    f"weights weightgen.fill_module_(model, 'c2frv.'), frames synthetic_frames(3, 1, {H}, {W}); "
                    f"maps > {SAMPLE} elements stored at weightgen.sample_index only"]

    def put(key, t):
        a = t.detach().reshape(-1).numpy().astype(np.float32)
        out[key] = a[weightgen.sample_index(key, a.size, SAMPLE)]

    for cfg, kw in CONFIGS.items():
        torch.manual_seed(0)
        model = Coarse2FineGroupRepViTRAFTStereo(iters=4, **kw)
        weightgen.fill_module_(model, "c2frv.")
        model.eval()
        sd = model.state_dict()
        out[cfg + "_keys"] = np.array(list(sd.keys()))
        out[cfg + "_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
        n_enc = sum(1 for k in sd if not k.startswith("update_block."))
        n_par = sum(v.numel() for k, v in model.named_parameters() if not k.startswith("update_block."))
        ls = torch.cat([v.reshape(-1) for k, v in sd.items() if "layer_scale" in k])
        rep.append(f"[{cfg}] {kw or 'defaults'}: {len(sd)} state_dict keys, {n_enc} on the encoder side ({n_par / 1e6:.2f} M parameters); "
                   f"layer_scale |x| in [{ls.abs().min():.3f}, {ls.abs().max():.3f}] (O(1): the residual branches are visible)")
        with torch.no_grad():
            maps = encoder_side(model, f1, f2)
            maps64 = encoder_side(model.double(), f1.double(), f2.double())
        model.float()
        for name, t in maps.items():
            err = (t.double() - maps64[name]).abs().max().item()
            mx = t.abs().max().item()
            put(f"{cfg}_{name}", t)
            out[f"{cfg}_{name}_maxabs"] = np.float64(mx)
            out[f"{cfg}_{name}_err64"] = np.float64(err)
            rep.append(f"  {name:7s} {tuple(t.shape)!s:18s} max-abs {mx:9.4f}   fp32-CPU vs float64 {err:.3e} ({err / mx:.1e} rel)")
        if cfg == "default":
            with torch.no_grad():
                ups = [o["up_disp"] for o in model(f1, f2)]
            assert len(ups) == 12
            for i, u in enumerate(ups):
                put(f"up{i}", u)
                out[f"up{i}_maxabs"] = np.float64(u.abs().max().item())
            rep.append(f"  forward iters=4: {len(ups)} up_disp {tuple(ups[-1].shape)}, final max-abs {ups[-1].abs().max():.3f}")
    np.savez_compressed(os.path.join(GOLD, "c2f_repvit.npz"), **out)
    with open(os.path.join(GOLD, "REPORT_c2f_repvit.txt"), "w") as f:
        f.write("\n".join(rep) + "\n")
    print("\n".join(rep))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
