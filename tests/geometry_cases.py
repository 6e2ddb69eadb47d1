"""Oracles and inputs of the stereo-geometry tests (csrc/geometry.hip, nndepth_amd/geometry.py), numpy only.

Every contract is a closed form, so the oracles are the contracts themselves: the double-precision ones (to_depth, points) are
evaluated in numpy float64 and rounded once to fp32; the fp32 ones (to_disparity, lr_consistency) are evaluated with numpy
float32 arrays, where every ufunc is one rounded operation.  `lr` takes the dtype as an argument: on the dyadic scenes below every
step is exact in fp32, so the float32 and float64 evaluations agree bit for bit, which the tests assert rather than assume."""
import numpy as np

F32, F64 = np.float32, np.float64
TARTANAIR_FX, TARTANAIR_BASELINE = 320, 0.25  # nndepth/data/datasets/tartanair_dataset.py:28,30
LR_THRESHOLD = 1.0 + 2.0 ** -7                # err is a multiple of 1/64 on the dyadic scenes: |err - threshold| >= 2^-7
SUBNORMAL = float(np.float32(1e-41))


def cam_of(K: np.ndarray, B: int) -> np.ndarray:
    """(B,4) float64 {fx, fy, cx, cy} of a (3,3) or (B,3,3) intrinsic, through fp32 as the device array holds them."""
    K = np.asarray(K, F32).reshape(-1, 3, 3)
    par = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1).astype(F64)
    return np.broadcast_to(par, (B, 4)) if par.shape[0] == 1 else par


def to_depth(d, fx, baseline, sign="negative", min_disp=0.0, max_depth=None, mask=None):
    """d (B,1,H,W) fp32, fx (B,) -> (depth fp32, valid uint8): the numpy float64 formula rounded once."""
    d = np.asarray(d, F32)
    m = -d if sign == "negative" else d
    fx = np.asarray(fx, F32).astype(F64).reshape(-1, 1, 1, 1)
    with np.errstate(all="ignore"):
        z = (fx * F64(baseline) / m.astype(F64)).astype(F32)
        ok = np.isfinite(m) & (m > F32(min_disp))
        if max_depth is not None:
            ok &= z <= F32(max_depth)
    if mask is not None:
        ok &= np.asarray(mask).reshape(d.shape) != 0
    return np.where(ok, z, F32(0)), ok.astype(np.uint8)


def to_disparity(z, fx, baseline, sign="negative", eps=1e-8):
    """The reference's TartanAir expression -BASELINE * FX / (depth + 1e-8) on an fp32 array: the scalar rounded to fp32, the sum
    and the quotient in fp32."""
    z = np.asarray(z, F32)
    c = (-F64(baseline) * np.asarray(fx, F32).astype(F64)).astype(F32).reshape(-1, 1, 1, 1)
    with np.errstate(all="ignore"):
        d = c / (z + F32(eps))
    assert d.dtype == F32
    return d if sign == "negative" else -d


def points_map(z, cam, mask=None):
    """z (B,1,H,W) fp32, cam (B,4) -> (B,3,H,W) fp32; ((u - cx) * Z) / fx in float64, rounded once; 0 where mask == 0."""
    z = np.asarray(z, F32)
    B, _, H, W = z.shape
    v, u = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    fx, fy, cx, cy = (cam[:, i].reshape(B, 1, 1) for i in range(4))
    Z = z[:, 0].astype(F64)
    with np.errstate(all="ignore"):
        X = ((u - cx) * Z / fx).astype(F32)
        Y = ((v - cy) * Z / fy).astype(F32)
    out = np.stack([X, Y, z[:, 0]], 1)
    if mask is not None:
        out = np.where(np.asarray(mask).reshape(B, 1, H, W) != 0, out, F32(0))
    return out


def compact(z, cam, mask=None, features=None):
    """(points (n,3), feats (n,C) or None, offsets (B+1,) int64): the valid pixels of each sample in row-major order."""
    z = np.asarray(z, F32)
    B, _, H, W = z.shape
    ok = np.ones((B, H * W), bool) if mask is None else np.asarray(mask).reshape(B, H * W) != 0
    pm = points_map(z, cam).reshape(B, 3, H * W)
    offsets = np.concatenate([[0], np.cumsum(ok.sum(1))]).astype(np.int64)
    pts = np.concatenate([pm[b][:, ok[b]].T for b in range(B)], 0)
    feats = None
    if features is not None:
        f = np.asarray(features, F32).reshape(B, -1, H * W)
        feats = np.concatenate([f[b][:, ok[b]].T for b in range(B)], 0)
    return pts, feats, offsets


def lr(dl, dr, threshold, left_sign="negative", right_sign="negative", right_flipped=False, dtype=F32):
    """(occluded uint8, err) of (B,1,H,W) maps, every step one operation in `dtype`; err = +inf where an earlier test decided."""
    dl, dr = np.asarray(dl, F32).astype(dtype), np.asarray(dr, F32).astype(dtype)
    if right_flipped:
        dr = dr[..., ::-1]
    B, _, H, W = dl.shape
    mL = -dl if left_sign == "negative" else dl
    mR = -dr if right_sign == "negative" else dr
    x = np.broadcast_to(np.arange(W, dtype=dtype), dl.shape)
    with np.errstate(all="ignore"):
        go = np.isfinite(mL) & ~(mL < 0)
        xr = np.where(go, x - mL, dtype(0))
        go &= ~(xr < 0) & ~(xr > dtype(W - 1))
        xr = np.where(go, xr, dtype(0))
        fl = np.floor(xr)
        i0 = fl.astype(np.int64)
        i1 = np.minimum(i0 + 1, W - 1)
        f = xr - fl
        s = np.take_along_axis(mR, i0, 3) * (dtype(1) - f) + np.take_along_axis(mR, i1, 3) * f
        err = np.where(go, np.abs(mL - s), dtype(np.inf))
        occ = ~(err <= dtype(threshold))
    return occ.astype(np.uint8), err


def special_disparity(B, H, W, seed, sign="negative"):
    """Magnitudes in (0, 64) with every special value the contract names placed at fixed pixels of sample 0, stored with `sign`."""
    g = np.random.default_rng(seed)
    m = (g.random((B, 1, H, W)) * 64 + 0.01).astype(F32)
    flat = m[0, 0].reshape(-1)
    special = [0.0, -0.0, SUBNORMAL, -SUBNORMAL, -3.5, -1e-3, np.inf, -np.inf, np.nan, 4.0, float(np.nextafter(F32(4), F32(0))),
               float(np.nextafter(F32(4), F32(8))), 0.5, float(np.nextafter(F32(0.5), F32(0)))]
    idx = g.permutation(flat.size)[:len(special)]
    flat[idx] = np.asarray(special, F32)
    return (-m if sign == "negative" else m), idx


def lr_scene(H, W, seed=0, bg=2.0, fg=5.0, ramp=True):
    """Left and right disparity MAGNITUDES (1,1,H,W), every value a multiple of 1/8: a fronto-parallel background at `bg`, a
    foreground box at `fg` in the upper rows shifted consistently into the right view (what it hides there and what the left view
    cannot see of the background are the occlusions), and in the lower third a column ramp (right: bg + xr/8; left: the
    consistent (8 bg + x) / 9 rounded to 1/8) so that the interpolation weights matter."""
    L = np.full((H, W), bg, F64)
    R = np.full((H, W), bg, F64)
    y0, y1 = 1, max(2, (2 * H) // 3)
    x0, x1 = W // 2, min(W - 1, W // 2 + max(2, W // 4))
    L[y0:y1, x0:x1] = fg
    a, b = int(x0 - fg), int(x1 - fg)
    R[y0:y1, max(a, 0):max(b, 0)] = fg
    if ramp:
        r0 = y1 + 1
        xs = np.arange(W, dtype=F64)
        R[r0:] = bg + xs / 8
        L[r0:] = np.round((8 * bg + xs) / 9 * 8) / 8
    assert np.array_equal(L * 8, np.round(L * 8)) and np.array_equal(R * 8, np.round(R * 8))
    return L[None, None].astype(F32), R[None, None].astype(F32)


def lr_cases():
    """name -> (mL, mR) magnitudes (B,1,H,W): two-plane scenes with a ramp at 12x40 and 7x33, W = 5, and a 2-sample batch with
    NaN / inf / wrong-sign pixels in the left map, a NaN in the right one and a disparity larger than the frame is wide."""
    cases = {"12x40": lr_scene(12, 40), "7x33": lr_scene(7, 33, bg=1.5, fg=4.25), "3x5": lr_scene(3, 5, bg=0.5, fg=1.0, ramp=False)}
    l0, r0 = lr_scene(9, 70, bg=3.0, fg=9.5)
    l1, r1 = lr_scene(9, 70, bg=0.0, fg=2.125)
    l1[0, 0, 0, 3], l1[0, 0, 0, 9], l1[0, 0, 1, 2], l1[0, 0, 2, 5] = np.nan, np.inf, -1.0, 80.0
    l1[0, 0, 0, 69] = -0.0
    r1[0, 0, 4, 20] = np.nan
    cases["2x9x70"] = (np.concatenate([l0, l1]), np.concatenate([r0, r1]))
    return cases


def stored(m, sign):
    """The map a model with `sign` would store for the magnitudes m."""
    return -m if sign == "negative" else m.copy()
