"""Fixture of the one-piece fp16 arithmetic's model test (tests/golden/fp16_raft.npz with the 64x128 arrays, fp16_raft_96x160.npz with
the others: one file would pass the size limit of a committed file; the first section of REPORT_fp16.txt).

Runs only where the reference checkout is importable (like scripts/make_golden_*.py: it imports the stand-ins of
oracle/make_golden.py and changes nothing under oracle/).  The reference's BaseRAFTStereo(context_dim=64) with
weightgen.fill_state_dict(oracle.torch_ref.raft_stereo_spec()) — the weights of every RAFT-Stereo golden, not stored — on the
TartanAir pair of tests/golden resized to 64x128 (12 iterations) and 96x160 (8 iterations; W / 8 >= 16 for the four correlation
levels), on the CPU:
  frames_<HxW>    the two resized, normalised frames (2, 3, H, W)
  fp32_<HxW>      up_disp of every iteration of the fp32 forward (iters, H, W)
  bf16_<HxW>      the same under torch.autocast("cpu", dtype=torch.bfloat16): the arithmetic every trainer of the reference validates
                  with (raft_trainer.py:242,352)
  dev_<HxW>       mean |bf16 - fp32| per iteration: what the GPU test gates against

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_fp16.py [path of the reference checkout; default: oracle's]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")
SIZES = {(64, 128): 12, (96, 160): 8}
MARK = "== fixture (scripts/make_golden_fp16.py)\n"


def frames_at(hw):
    from PIL import Image
    out = []
    for side in ("left", "right"):
        img = np.asarray(Image.open(os.path.join(GOLD, f"tartanair_000000_{side}.png")).convert("RGB"))
        t = torch.from_numpy(img.copy()).permute(2, 0, 1).float().unsqueeze(0)
        t = torch.nn.functional.interpolate(t, hw, mode="bilinear")
        out.append((t - 127.5) / 127.5)
    return out


def main(ref_path):
    from nndepth_amd import weightgen
    from oracle import torch_ref as R
    import oracle.make_golden as mg
    if ref_path:
        mg.REF = ref_path
    mg._install_standins()
    from nndepth.models.raft_stereo.model import BaseRAFTStereo

    sd = weightgen.fill_state_dict(R.raft_stereo_spec())
    rep = []
    for (h, w), iters in SIZES.items():
        model = BaseRAFTStereo(iters=iters, context_dim=64).eval()
        model.load_state_dict(sd, strict=True)
        f1, f2 = frames_at((h, w))
        with torch.no_grad():
            fp32 = torch.stack([o["up_disp"][0, 0].float() for o in model(f1, f2)])
            with torch.autocast("cpu", dtype=torch.bfloat16):
                bf16 = torch.stack([o["up_disp"][0, 0].float() for o in model(f1, f2)])
        assert fp32.shape == bf16.shape == (iters, h, w)
        dev = (bf16 - fp32).abs().mean(dim=(1, 2))
        key, out = f"{h}x{w}", {}
        out["frames_" + key] = torch.cat([f1, f2]).numpy()
        out["fp32_" + key] = fp32.numpy()
        out["bf16_" + key] = bf16.numpy()
        out["dev_" + key] = dev.double().numpy()
        rep.append(f"{key}, {iters} iterations: |up_disp| max {fp32[-1].abs().max():.2f} px; mean |bf16 autocast - fp32| per iteration: "
                   + " ".join(f"{d:.2e}" for d in dev.tolist()) + "\n")
        name = os.path.join(GOLD, "fp16_raft.npz" if (h, w) == (64, 128) else f"fp16_raft_{key}.npz")
        np.savez_compressed(name, **out)
        assert os.path.getsize(name) < (1 << 20), (name, os.path.getsize(name))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from fp16_report import report_section  # the one writer of REPORT_fp16.txt
    report_section(MARK, rep)
    print("".join(rep), end="")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
