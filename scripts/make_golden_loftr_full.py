"""Fixture of the LoFTR full (softmax) attention (tests/golden/loftr_full.npz, REPORT_loftr_full.txt).

Runs only where the reference checkout is importable (like scripts/make_golden_midas_loss.py; it installs the stand-ins of
oracle/make_golden.py and changes nothing under oracle/), on the CPU in fp32.  The inputs of every case are a pure function of
the case's name (tests/loftr_full_cases.py: make_case), so no input array is stored, only:

  names            JSON list of the case names
  d_ref            (ncases,) float64: max |reference fp32 - float64 contract|; the reference is the imported FullAttention
                   (att/ cases, on the (N, L, H, D) tokens) or LoFTREncoderLayer(256, 8, "full") (layer/ cases)
  fmax             (ncases,) float64: max |contract|
  ref_out/<name>   the reference's fp32 output as an (N, C, H, W) map, for the two cases of loftr_full_cases.STORED

A case with d_ref > 7.5e-6 * max(1, fmax) is refused: an ill-conditioned case would only loosen the bar the tests derive from d_ref.
The cases of loftr_full_cases.REFUSED are known to be: they are measured, reported and left out of the fixture, and the script stops
if one of them has come inside the cap (the list is stale) or any other case is outside it.
An existing REPORT keeps its measured GPU section (everything from the line "GPU:" on; tests/test_gpu_loftr_full.py writes it).

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_loftr_full.py [path of the reference checkout; default: oracle's]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")


def main(ref_path):
    import oracle.make_golden as mg
    if ref_path:
        mg.REF = ref_path
    mg._install_standins()
    from nndepth.blocks.attn_block import FullAttention
    from nndepth.blocks.transformer import LoFTREncoderLayer
    import loftr_full_cases as lc

    torch.set_grad_enabled(False)
    sd = lc.state_dict()
    rep = ["LoFTR full attention: the reference's FullAttention / LoFTREncoderLayer(256, 8, 'full') on the CPU in fp32 against the "
           f"float64 contract (tests/loftr_full_cases.py); scripts/make_golden_loftr_full.py, torch {torch.__version__.split('+')[0]}, "
           f"numpy {np.__version__}",
           f"refused above d_ref = {lc.CAP:g} * max(1, fmax); per case: fmax, d_ref, d_ref / fmax"]
    d_ref, fmax, stored = [], [], {}
    for name in lc.CASES + lc.REFUSED:
        want = lc.contract(name)
        if name.startswith("att/"):
            q, k, v, nhead = lc.make_case(name)
            tok = lambda t: t.reshape(t.shape[0], nhead, lc.HEAD, t.shape[2]).permute(0, 3, 1, 2).contiguous()  # (N, L, H, D)
            got = FullAttention()(tok(q), tok(k), tok(v)).permute(0, 2, 3, 1).reshape(q.shape)
        else:
            prefix, x, source = lc.make_case(name)
            layer = LoFTREncoderLayer(lc.D_MODEL, lc.NHEAD, "full").eval()
            layer.load_state_dict({k[len(prefix):]: t for k, t in sd.items() if k.startswith(prefix)}, strict=True)
            n, c, h, w = x.shape
            tok = lambda t: t.permute(0, 2, 3, 1).reshape(n, h * w, c)
            got = layer(tok(x), tok(source)).reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()
            if name in lc.STORED:
                stored["ref_out/" + name] = got.numpy().copy()
        assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        d, f = float(np.abs(got.numpy().astype(np.float64) - want).max()), float(np.abs(want).max())
        if name in lc.REFUSED:
            if d <= lc.CAP * max(1.0, f):
                raise SystemExit(f"case {name}: listed as refused, but d_ref = {d:.3e} with fmax = {f:.3e} is inside the cap")
            rep.append(f"REFUSED {name:33s} fmax = {f:<12.6g} d_ref = {d:.3e}  d_ref / fmax = {d / f:.2e}  (above the cap: in no fixture, no test)")
            continue
        if d > lc.CAP * max(1.0, f):
            raise SystemExit(f"case {name}: d_ref = {d:.3e} with fmax = {f:.3e} is above the cap; the case is ill-conditioned")
        rep.append(f"case {name:36s} fmax = {f:<12.6g} d_ref = {d:.3e}  d_ref / fmax = {d / f:.2e}")
        d_ref.append(d), fmax.append(f)
    path = os.path.join(GOLD, "loftr_full.npz")
    np.savez_compressed(path, names=np.array(json.dumps(list(lc.CASES))), d_ref=np.array(d_ref), fmax=np.array(fmax), **stored)
    rep.append(f"worst d_ref / max(1, fmax) = {max(d / max(1.0, f) for d, f in zip(d_ref, fmax)):.3e}")
    rep.append(f"loftr_full.npz: {os.path.getsize(path)} bytes")
    report = os.path.join(GOLD, "REPORT_loftr_full.txt")
    gpu = []
    if os.path.exists(report):
        old = open(report).read().split("\n")
        if "GPU:" in old:
            gpu = old[old.index("GPU:"):]
    with open(report, "w") as fh:
        fh.write("\n".join(rep + [g for g in gpu if g]) + "\n")
    print("\n".join(rep))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
