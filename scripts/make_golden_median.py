"""Fixture of the median-filter tests (tests/golden/median.npz).

Dev-time only, like the other make_golden_* scripts; runs on the CPU.  The expected results come from the loops of THIS file,
one pixel and one tap at a time in plain Python (the ok taps of the clipped window in a list, sorted by their integer key, a
running integer sum until twice it reaches the total), NOT from the vectorised numpy oracle of tests/median_cases.py, which
tests/test_median_cpu.py then checks against these loops and against this file.  Only the float steps of the guide distance use
numpy scalars (np.float32 arithmetic).  Nothing here comes from the reference, which has no such operation.

Stored, for the cases of `cases()` (inputs from tests/median_cases.py at median_cases.GOLDEN_SHAPE: a (2,1,9,40) map, a 3-channel
guide and a mask):

  <case>_{filtered,mask_out,changed}   the three outputs
  numpy                                the version that evaluated all of it

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_median.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
KEYS = ("filtered", "mask_out", "changed")


def _bits(v) -> int:
    return int(np.array(v, dtype=F32).view(np.uint32))


def _key(v) -> int:
    b = _bits(v)
    return b ^ (0xFFFFFFFF if b & 0x80000000 else 0x80000000)


def _weight(guide, b, y, x, qy, qx, inv_step, weights) -> int:
    with np.errstate(all="ignore"):
        dist = None
        for c in range(guide.shape[1]):
            a = abs(F32(guide[b, c, y, x]) - F32(guide[b, c, qy, qx]))
            dist = a if dist is None else F32(dist + a)
        s = F32(F32(dist) * F32(inv_step))
    return int(weights[int(s) if s < F32(255.0) else 255])


def median_loops(d, radius=1, mask=None, mask_is_valid=True, guide=None, inv_step=None, weights=None, min_count=1, fill_invalid=False,
                 fill=0.0):
    B, _, H, W = d.shape
    ok = np.zeros(d.shape, bool)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                valid = True if mask is None else (bool(np.asarray(mask).reshape(d.shape)[b, 0, y, x]) == bool(mask_is_valid))
                ok[b, 0, y, x] = valid and math.isfinite(d[b, 0, y, x])
    out = np.zeros(d.shape, F32)
    mask_out = np.zeros(d.shape, np.uint8)
    changed = np.zeros(d.shape, np.uint8)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                taps = []  # (key, weight, value) of the ok taps of the clipped window
                for qy in range(max(0, y - radius), min(H, y + radius + 1)):
                    for qx in range(max(0, x - radius), min(W, x + radius + 1)):
                        if ok[b, 0, qy, qx]:
                            w = 1 if guide is None else _weight(guide, b, y, x, qy, qx, inv_step, weights)
                            taps.append((_key(d[b, 0, qy, qx]), w, d[b, 0, qy, qx]))
                n, T = len(taps), sum(t[1] for t in taps)
                produced = (ok[b, 0, y, x] or fill_invalid) and n >= min_count and T > 0
                if produced:
                    taps.sort(key=lambda t: t[0])
                    S, i = 0, 0
                    while True:  # all the taps of one key at a time: S(v) counts every tap with key <= key(v)
                        j = i
                        while j < n and taps[j][0] == taps[i][0]:
                            S += taps[j][1]
                            j += 1
                        if 2 * S >= T:
                            break
                        i = j
                    value = taps[i][2]
                else:
                    value = d[b, 0, y, x] if ok[b, 0, y, x] else F32(fill)
                out[b, 0, y, x] = value
                mask_out[b, 0, y, x] = int((ok[b, 0, y, x] or produced) == bool(mask_is_valid))
                changed[b, 0, y, x] = int(_bits(out[b, 0, y, x]) != _bits(d[b, 0, y, x]) or (not ok[b, 0, y, x] and produced))
    return out, mask_out, changed


def cases():
    """name -> kwargs of median_loops / median_cases.median_filter: a handful of parameter sets on the golden inputs."""
    import median_cases as Mc
    shape = Mc.GOLDEN_SHAPE
    d, mask = Mc.scene(shape, 3)
    _, _, guide = Mc.edge_guide(shape, 3, 3)
    de, me, ge = Mc.edge_guide(shape, 3, 4, nan=True)
    T = Mc.tables()
    return {
        "r1": dict(d=d, radius=1, mask=mask),
        "r2_fill_invalid": dict(d=d, radius=2, mask=mask, fill_invalid=True, min_count=5, fill=-1.0),
        "r3_occlusion_negative": dict(d=-d, radius=3, mask=~mask, mask_is_valid=False, min_count=49, fill_invalid=True, fill=2.5),
        "r2_guided_exp": dict(d=d, radius=2, mask=mask, guide=guide, weights=T["exp"][0], inv_step=T["exp"][1], fill_invalid=True),
        "r3_guided_edge_nan": dict(d=de, radius=3, mask=me, guide=ge, weights=T["gauss"][0], inv_step=T["gauss"][1]),
        "r7_guided_cut": dict(d=de, radius=7, mask=me, guide=ge[:, :1], weights=T["zeros_after_5"][0], inv_step=T["zeros_after_5"][1],
                              fill_invalid=True, min_count=3),
        "r1_few_values_no_mask": dict(d=Mc.few_values(shape, 5)[0], radius=1),
        "r7_special": dict(d=Mc.special(shape, 6)[0], radius=7, fill=9.0, fill_invalid=True),
    }


def main():
    out = {"numpy": np.array(np.__version__)}
    for name, kw in cases().items():
        for key, a in zip(KEYS, median_loops(**kw)):
            out[f"{name}_{key}"] = a
        print(name, "changed", int(out[f"{name}_changed"].sum()), "of", out[f"{name}_changed"].size)
    np.savez_compressed(os.path.join(GOLD, "median.npz"), **out)


if __name__ == "__main__":
    main()
