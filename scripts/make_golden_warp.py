"""Fixture of the view-warp / hole-filling tests (tests/golden/warp_fill.npz).

Dev-time only, like the other make_golden_* scripts; runs on the CPU.  The expected results come from the loops of THIS file,
one pixel at a time in plain Python (ascending x with a strict `>` for the winner of a target, a walk to the left and to the right
for the neighbours of a hole), NOT from the vectorised numpy oracle of tests/warp_cases.py, which tests/test_warp_cpu.py then
checks against these loops and against this file.  Only the float steps use numpy scalars (np.float32 arithmetic, np.rint).

Stored, for the cases of `cases()` (inputs from tests/warp_cases.py at warp_cases.GOLDEN_SHAPE and smaller):

  warp_<case>_{disp,valid,occluded,source[,features]}   the five outputs of the warp
  fill_<case>_{filled,was_filled,mask_out}              the three outputs of the fill
  numpy                                                 the version that evaluated all of it

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_warp.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32


def _valid(mask, mask_is_valid, b, y, x):
    return True if mask is None else (bool(mask[b, 0, y, x]) == bool(mask_is_valid))


def warp_loops(d, disp_sign="negative", to_view="right", threshold=1.0, mask=None, features=None, fill=0.0, mask_is_valid=True):
    B, _, H, W = d.shape
    disp = np.full(d.shape, F32(fill), F32)
    won = np.zeros(d.shape, bool)
    occluded = np.ones(d.shape, np.uint8)
    source = np.full(d.shape, -1, np.int32)
    feats = None if features is None else np.zeros(features.shape, F32)
    thr = F32(threshold)
    with np.errstate(all="ignore"):
        for b in range(B):
            for y in range(H):
                best = [None] * W  # per target: (m, x) of the winner so far
                landed = [None] * W  # per source: (m, t)
                for x in range(W):  # ascending x, strict >: among equal m the smallest x stays
                    m = (-d[b, 0, y, x] if disp_sign == "negative" else d[b, 0, y, x]) + F32(0)
                    if not (_valid(mask, mask_is_valid, b, y, x) and math.isfinite(m) and m >= 0):
                        continue
                    t = np.rint(F32(x) - m if to_view == "right" else F32(x) + m)
                    if not (t >= 0 and t <= W - 1):
                        continue
                    t = int(t)
                    landed[x] = (m, t)
                    if best[t] is None or m > best[t][0]:
                        best[t] = (m, x)
                for t in range(W):
                    if best[t] is not None:
                        m, x = best[t]
                        disp[b, 0, y, t] = -m if disp_sign == "negative" else m
                        won[b, 0, y, t] = True
                        source[b, 0, y, t] = x
                        if feats is not None:
                            feats[b, :, y, t] = features[b, :, y, x]
                for x in range(W):
                    if landed[x] is not None:
                        m, t = landed[x]
                        occluded[b, 0, y, x] = 0 if F32(best[t][0] - m) <= thr else 1
    return disp, (won == bool(mask_is_valid)).astype(np.uint8), occluded, source, feats


def _pick(rule, va, vb, da, db):
    """the first of two neighbours?"""
    if rule == "min_abs":
        return abs(va) <= abs(vb)
    if rule == "max_abs":
        return abs(va) >= abs(vb)
    return da <= db


def fill_loops(d, mask=None, mask_is_valid=True, rule="min_abs", vertical=True, fill=0.0):
    B, _, H, W = d.shape
    out = np.full(d.shape, F32(fill), F32)
    was = np.zeros(d.shape, np.uint8)
    has = np.zeros(d.shape, bool)
    for b in range(B):
        ok = [[_valid(mask, mask_is_valid, b, y, x) and math.isfinite(d[b, 0, y, x]) for x in range(W)] for y in range(H)]
        nonempty = [any(r) for r in ok]
        for y in range(H):
            if not nonempty[y]:
                continue
            for x in range(W):
                has[b, 0, y, x] = True
                if ok[y][x]:
                    out[b, 0, y, x] = d[b, 0, y, x]
                    continue
                L = x - 1
                while L >= 0 and not ok[y][L]:
                    L -= 1
                R = x + 1
                while R < W and not ok[y][R]:
                    R += 1
                if L >= 0 and R < W:
                    src = L if _pick(rule, d[b, 0, y, L], d[b, 0, y, R], x - L, R - x) else R
                else:
                    src = L if L >= 0 else R
                out[b, 0, y, x] = d[b, 0, y, src]
                was[b, 0, y, x] = 1
        if not vertical:
            continue
        rows = out[b, 0].copy()  # the row-pass result
        for y in range(H):
            if nonempty[y]:
                continue
            U = y - 1
            while U >= 0 and not nonempty[U]:
                U -= 1
            D = y + 1
            while D < H and not nonempty[D]:
                D += 1
            if U < 0 and D >= H:
                continue
            for x in range(W):
                if U >= 0 and D < H:
                    src = U if _pick(rule, rows[U, x], rows[D, x], y - U, D - y) else D
                else:
                    src = U if U >= 0 else D
                out[b, 0, y, x] = rows[src, x]
                was[b, 0, y, x] = 1
                has[b, 0, y, x] = True
    return out, was, (has == bool(mask_is_valid)).astype(np.uint8)


def cases():
    """name -> ("warp" | "fill", arguments of warp_loops / fill_loops); small, so that the loops take a second."""
    import warp_cases as Wc
    shape = Wc.GOLDEN_SHAPE
    g = Wc.S.rng(11)
    out = {}
    for sign in ("negative", "positive"):
        for view in ("right", "left"):
            d, mask = Wc.scene(shape, 77, sign)
            out[f"scene_{sign}_{view}"] = ("warp", dict(d=d, disp_sign=sign, to_view=view, threshold=1.0, mask=mask,
                                                         features=g.random((shape[0], 3) + shape[2:]).astype(F32), fill=-7.0))
    out["ties_left"] = ("warp", dict(d=Wc.half_integer((1, 1, 2, 9)), disp_sign="positive", to_view="left"))
    out["ties_right"] = ("warp", dict(d=Wc.half_integer((1, 1, 2, 9), 1.5), disp_sign="positive", to_view="right"))
    out["special"] = ("warp", dict(d=Wc.special(), disp_sign="positive", to_view="right", threshold=float("inf")))
    out["bar"] = ("warp", dict(d=Wc.bar(), disp_sign="positive", threshold=Wc.BAR_THRESHOLD))
    out["bar_ulp"] = ("warp", dict(d=Wc.bar(ulp=True), disp_sign="positive", threshold=Wc.BAR_THRESHOLD))
    for rule in Wc.RULES:
        d, mask = Wc.holes(shape, 5)
        out[f"holes_{rule}"] = ("fill", dict(d=d, mask=mask, rule=rule, fill=-1.0))
        d, mask = Wc.fill_pattern(8)
        out[f"pattern_{rule}"] = ("fill", dict(d=d, mask=mask, rule=rule, fill=-1.0))
        out[f"pattern_{rule}_rows_only"] = ("fill", dict(d=d, mask=~mask, mask_is_valid=False, rule=rule, vertical=False, fill=3.0))
    return out


WARP_KEYS = ("disp", "valid", "occluded", "source", "features")
FILL_KEYS = ("filled", "was_filled", "mask_out")


def main():
    out = {}
    for name, (kind, kw) in cases().items():
        res = warp_loops(**kw) if kind == "warp" else fill_loops(**kw)
        for key, a in zip(WARP_KEYS if kind == "warp" else FILL_KEYS, res):
            if a is not None:
                out[f"{kind}_{name}_{key}"] = a
        if kind == "warp":
            print(f"warp {name}: {int((res[3] < 0).sum())} holes, {int(res[2].sum())} occluded of {res[2].size}")
        else:
            print(f"fill {name}: {int(res[1].sum())} filled, {int((res[2] == 0).sum())} still invalid of {res[1].size}")
    out["numpy"] = np.array(np.__version__)
    path = os.path.join(GOLD, "warp_fill.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print(f"warp_fill.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
