"""Fixture of the view-synthesis and photometric-error tests (tests/golden/photometric.npz).

Dev-time only, like the other make_golden_* scripts; runs on the CPU.  The expected results come from the loops of THIS file,
one pixel, one channel and one tap at a time in plain Python with np.float32 scalars (every arithmetic step wrapped in F32, so it
is one rounded fp32 operation), NOT from the vectorised numpy oracle of tests/photometric_cases.py, which
tests/test_photometric_cpu.py then checks against these loops and against this file.  Nothing here comes from the reference,
which has no such operation.

Stored, for the cases of `cases()` (inputs from tests/photometric_cases.py at photometric_cases.GOLDEN_SHAPE, (2,3,7,24)):

  <case>_{error,valid,l1,dssim}            the outputs of photometric_error
  <case>_{recon,in}                        the outputs of synthesize_view, for the cases of RECON_CASES
  numpy                                    the version that evaluated all of it

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_photometric.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
KEYS = ("recon", "in", "error", "valid", "l1", "dssim")
RECON_CASES = ("scene", "right", "edges")


def stored(name):
    """The keys of KEYS that the file holds for case `name`."""
    return KEYS if name in RECON_CASES else KEYS[2:]


def _reflect(i, n):
    return -i if i < 0 else 2 * n - 2 - i if i >= n else i


def _clamp01(v):
    return F32(0.0) if v < 0 else F32(1.0) if v > 1 else v  # a NaN fails both tests and stays


def sample_loops(other, d, mask, mask_is_valid, disp_sign, target_view):
    """rec (B,C,H,W) float32 (0 where not in) and in (B,H,W) bool, pixel by pixel."""
    B, C, H, W = other.shape
    rec = np.zeros((B, C, H, W), F32)
    inn = np.zeros((B, H, W), bool)
    mk = None if mask is None else np.asarray(mask).reshape(B, H, W)
    with np.errstate(all="ignore"):
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    v = F32(d[b, 0, y, x])
                    m = F32((-v if disp_sign == "negative" else v) + F32(0.0))
                    mask_ok = True if mk is None else (bool(mk[b, y, x]) == bool(mask_is_valid))
                    if not (mask_ok and math.isfinite(m) and m >= 0):
                        continue
                    xr = F32(F32(x) - m) if target_view == "left" else F32(F32(x) + m)
                    if not (xr >= 0 and xr <= F32(W - 1)):
                        continue
                    fl = F32(math.floor(xr))
                    i0 = int(fl)
                    i1 = min(i0 + 1, W - 1)
                    f = F32(xr - fl)
                    inn[b, y, x] = True
                    for c in range(C):
                        a = F32(F32(other[b, c, y, i0]) * F32(F32(1.0) - f))
                        e = F32(F32(other[b, c, y, i1]) * f)
                        rec[b, c, y, x] = F32(a + e)
    return rec, inn


def _boxsum(get, y, x, H, W):
    """(r(y-1) + r(y)) + r(y+1) with r(y') = (v(y',x-1) + v(y',x)) + v(y',x+1) over the reflected taps; get(yy, xx) -> F32."""
    rows = []
    for dy in (-1, 0, 1):
        yy = _reflect(y + dy, H)
        v = [get(yy, _reflect(x + dx, W)) for dx in (-1, 0, 1)]
        rows.append(F32(F32(v[0] + v[1]) + v[2]))
    return F32(F32(rows[0] + rows[1]) + rows[2])


def photometric_loops(target, other, d, mask=None, mask_is_valid=True, disp_sign="negative", target_view="left", ssim_weight=0.85,
                      data_range=2.0, fill=0.0):
    """(recon, in, error, valid, l1, dssim) as KEYS: recon with `fill`, `in` and `valid` uint8 in the polarity of the mask."""
    B, C, H, W = target.shape
    r = float(data_range)
    c1, c2, inv_range = F32((0.01 * r) ** 2), F32((0.03 * r) ** 2), F32(1.0 / r)
    w, fl = F32(ssim_weight), F32(fill)
    inv9, invC = F32(1.0 / 9.0), F32(F32(1.0) / F32(C))
    rec, inn = sample_loops(other, d, mask, mask_is_valid, disp_sign, target_view)
    error, l1o, dso = (np.full((B, 1, H, W), fl, F32) for _ in range(3))
    valid = np.zeros((B, 1, H, W), np.uint8)
    with np.errstate(all="ignore"):
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    if w > 0:
                        taps_in = all(inn[b, _reflect(y + dy, H), _reflect(x + dx, W)] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
                    else:
                        taps_in = bool(inn[b, y, x])
                    ok = False
                    if taps_in:
                        l1 = ds = None
                        for c in range(C):
                            t, q = target[b, c], rec[b, c]
                            l1c = F32(abs(F32(t[y, x] - q[y, x])) * inv_range)
                            l1 = l1c if l1 is None else F32(l1 + l1c)
                            if w > 0:
                                mx = F32(_boxsum(lambda yy, xx: t[yy, xx], y, x, H, W) * inv9)
                                my = F32(_boxsum(lambda yy, xx: q[yy, xx], y, x, H, W) * inv9)
                                sx = F32(F32(_boxsum(lambda yy, xx: F32(t[yy, xx] * t[yy, xx]), y, x, H, W) * inv9) - F32(mx * mx))
                                sy = F32(F32(_boxsum(lambda yy, xx: F32(q[yy, xx] * q[yy, xx]), y, x, H, W) * inv9) - F32(my * my))
                                sxy = F32(F32(_boxsum(lambda yy, xx: F32(t[yy, xx] * q[yy, xx]), y, x, H, W) * inv9) - F32(mx * my))
                                n = F32(F32(F32(F32(F32(2.0) * mx) * my) + c1) * F32(F32(F32(2.0) * sxy) + c2))
                                dn = F32(F32(F32(F32(mx * mx) + F32(my * my)) + c1) * F32(F32(sx + sy) + c2))
                                dsc = _clamp01(F32(F32(F32(1.0) - F32(n / dn)) * F32(0.5)))
                                ds = dsc if ds is None else F32(ds + dsc)
                        l1 = F32(l1 * invC)
                        if w > 0:
                            ds = F32(ds * invC)
                            e = F32(F32(w * ds) + F32(F32(F32(1.0) - w) * l1))
                        else:
                            e = l1
                        ok = math.isfinite(e)
                        if ok:
                            error[b, 0, y, x], l1o[b, 0, y, x] = e, l1
                            if w > 0:
                                dso[b, 0, y, x] = ds
                    valid[b, 0, y, x] = int(ok == bool(mask_is_valid))
    recon = np.where(inn[:, None], rec, fl).astype(F32)
    return recon, (inn == bool(mask_is_valid)).astype(np.uint8)[:, None], error, valid, l1o, dso


def cases():
    """name -> kwargs of photometric_loops: a handful of parameter sets on the golden inputs."""
    import photometric_cases as Pc
    B = Pc.builders(Pc.GOLDEN_SHAPE, seed=3)
    one = Pc.builders((2, 1) + Pc.GOLDEN_SHAPE[2:], seed=4)
    return {
        "scene": dict(B["scene"]),
        "scene_l1_only": dict(B["scene"], ssim_weight=0.0, fill=-7.0),
        "positive_occlusion": dict(B["scene_positive_occlusion"], fill=-7.0),
        "right": dict(B["scene_right"], data_range=1.0),
        "integer_half_c1": dict(one["integer_half"]),
        "edges": dict(B["edges"]),
        "special_disp_ssim_only": dict(B["special_disp"], fill=2.5, ssim_weight=1.0),
        "special_pictures": dict(B["special_pictures"]),
    }


def main():
    out = {"numpy": np.array(np.__version__)}
    for name, kw in cases().items():
        res = photometric_loops(**kw)
        for key, a in zip(KEYS, res):
            if key in stored(name):
                out[f"{name}_{key}"] = a
        ok = res[3] == int(kw.get("mask_is_valid", True))
        print(name, "valid", int(ok.sum()), "of", ok.size)
    np.savez_compressed(os.path.join(GOLD, "photometric.npz"), **out)


if __name__ == "__main__":
    main()
