"""View synthesis and the photometric error (csrc/photometric.hip): a vectorised numpy oracle of the numbered contract in
include/nndepth_amd.h, and the inputs of tests/test_photometric_cpu.py, tests/test_gpu_photometric.py and
scripts/make_golden_photometric.py.

Every numpy operation on float32 arrays is one rounded fp32 operation, and the oracle performs the contract's steps one at a time
in the contract's order; with dtype=np.float64 the same steps run in double (the comparison with the Monodepth composition in
tests/test_photometric_cpu.py).  The loops of scripts/make_golden_photometric.py say the same pixel by pixel, and
test_photometric_cpu.py holds the two against each other.

Random inputs come from numpy's PCG64, seeded per case (speckle_cases.rng)."""
import math

import numpy as np

import speckle_cases as S

F32 = np.float32
bits = S.bits
GOLDEN_SHAPE = (2, 3, 7, 24)
SCENE_SHAPES = [(2, 3, 19, 131), (2, 1, 11, 131), (1, 4, 35, 259)]
SMALL_SHAPES = [(2, 3, 2, 2), (1, 1, 3, 5), (2, 3, 5, 7)]  # + the shapes around the tile, from the library
INVALIDITY = ("special_disp", "special_pictures", "edges", "edges_right")  # the builders whose purpose is what is NOT valid
MIN_VALID_SHARE, MIN_SHARE_WIDTH = 0.25, 40  # narrower frames: the margin x < m, which no picture covers, dominates


def constants(data_range=2.0):
    """(c1, c2, inv_range) as geometry.photometric_error forms them: float32, once."""
    r = float(data_range)
    return F32((0.01 * r) ** 2), F32((0.03 * r) ** 2), F32(1.0 / r)


def valid_of(shape, mask=None, mask_is_valid=True) -> np.ndarray:
    if mask is None:
        return np.ones(shape, bool)
    m = np.asarray(mask).reshape(shape) != 0
    return m if mask_is_valid else ~m


def _box(v):
    """Step 4: the 3 x 3 sum of the (B,H,W) array with reflected borders, row sums first."""
    H, W = v.shape[1:]
    p = np.pad(v, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    r = (p[:, :, 0:W] + p[:, :, 1:W + 1]) + p[:, :, 2:W + 2]
    return (r[:, 0:H] + r[:, 1:H + 1]) + r[:, 2:H + 2]


def _clamp01(v):
    return np.where(v < 0, v.dtype.type(0), np.where(v > 1, v.dtype.type(1), v))  # a NaN stays a NaN


def sample(other, d, mask=None, mask_is_valid=True, disp_sign="negative", target_view="left", dtype=F32):
    """Steps 1 - 3: (rec (B,C,H,W), 0 where not in; in (B,H,W) bool)."""
    F = dtype
    other, d = np.asarray(other), np.asarray(d)
    assert other.dtype == F32 and d.dtype == F32 and d.ndim == 4 and d.shape[1] == 1 and other.ndim == 4
    B, C, H, W = other.shape
    assert d.shape == (B, 1, H, W) and H >= 2 and W >= 2
    with np.errstate(all="ignore"):
        dd = d[:, 0].astype(F)
        m = (-dd if disp_sign == "negative" else dd) + F(0.0)
        src_ok = valid_of((B, H, W), mask, mask_is_valid) & np.isfinite(m) & (m >= 0)
        x = np.broadcast_to(np.arange(W, dtype=F), (B, H, W))
        xr = x - m if target_view == "left" else x + m
        inn = src_ok & (xr >= 0) & (xr <= F(W - 1))
        xs = np.where(inn, xr, F(0.0))
        fl = np.floor(xs)
        i0 = fl.astype(np.int64)
        i1 = np.minimum(i0 + 1, W - 1)
        f = xs - fl
        rec = np.empty((B, C, H, W), F)
        for c in range(C):
            o = other[:, c].astype(F)
            a = np.take_along_axis(o, i0, 2) * (F(1.0) - f)
            b = np.take_along_axis(o, i1, 2) * f
            rec[:, c] = np.where(inn, a + b, F(0.0))
        assert m.dtype == F and xr.dtype == F and f.dtype == F
    return rec, inn


def synthesize_view(other, d, mask=None, mask_is_valid=True, disp_sign="negative", target_view="left", fill=0.0):
    """(recon fp32 (B,C,H,W), valid uint8 (B,1,H,W) in the polarity of the mask)."""
    rec, inn = sample(other, d, mask, mask_is_valid, disp_sign, target_view)
    recon = np.where(inn[:, None], rec, F32(fill)).astype(F32)
    return recon, (inn == bool(mask_is_valid)).astype(np.uint8)[:, None]


def photometric_error(target, other, d, mask=None, mask_is_valid=True, disp_sign="negative", target_view="left", ssim_weight=0.85,
                      data_range=2.0, fill=0.0, dtype=F32):
    """(error, valid uint8 in the polarity of the mask, l1, dssim), each (B,1,H,W), and `ok` (B,1,H,W) bool = valid whatever
    the polarity.  dtype=np.float64: the same steps in double, on the same float32 inputs and constants."""
    F = dtype
    target = np.asarray(target)
    assert target.dtype == F32 and target.shape == np.asarray(other).shape
    B, C, H, W = target.shape
    c1, c2, inv_range = (F(v) for v in constants(data_range))
    w = F(F32(ssim_weight))
    rec, inn = sample(other, d, mask, mask_is_valid, disp_sign, target_view, F)
    inv9, invC = F(1.0 / 9.0), F(1.0) / F(C)
    with np.errstate(all="ignore"):
        ds = l1 = None
        for c in range(C):
            t, r = target[:, c].astype(F), rec[:, c]
            l1c = np.abs(t - r) * inv_range
            l1 = l1c if l1 is None else l1 + l1c
            if w > 0:
                mx, my = _box(t) * inv9, _box(r) * inv9
                sx = _box(t * t) * inv9 - mx * mx
                sy = _box(r * r) * inv9 - my * my
                sxy = _box(t * r) * inv9 - mx * my
                n = ((F(2.0) * mx) * my + c1) * (F(2.0) * sxy + c2)
                dn = ((mx * mx + my * my) + c1) * ((sx + sy) + c2)
                dsc = _clamp01((F(1.0) - n / dn) * F(0.5))
                ds = dsc if ds is None else ds + dsc
        l1 = l1 * invC
        if w > 0:
            ds = ds * invC
            a = w * ds
            b = (F(1.0) - w) * l1
            e = a + b
            in9 = _box(inn.astype(np.int64)) == 9
        else:
            ds = np.zeros_like(l1)
            e = l1
            in9 = inn
        assert e.dtype == F and l1.dtype == F and ds.dtype == F
        ok = in9 & np.isfinite(e)
    fl = F(fill)
    error, l1o = np.where(ok, e, fl), np.where(ok, l1, fl)
    dso = np.where(ok, ds, fl) if w > 0 else np.full_like(l1, fl)
    return error[:, None], (ok == bool(mask_is_valid)).astype(np.uint8)[:, None], l1o[:, None], dso[:, None], ok[:, None]


def stats_of(error, l1, dssim, ok, ssim_weight=0.85):
    """(B,4) float64 {count, sum e, sum l1, sum ds} with math.fsum over the valid values: the exact sums, rounded once."""
    out = np.zeros((ok.shape[0], 4), np.float64)
    for b in range(ok.shape[0]):
        v = ok[b]
        out[b] = [int(v.sum()), math.fsum(error[b][v].astype(np.float64)), math.fsum(l1[b][v].astype(np.float64)),
                  math.fsum(dssim[b][v].astype(np.float64)) if ssim_weight > 0 else 0.0]
    return out


# ----------------------------------------------------------------------------------------------------------------- the inputs
def texture(c, y, x, b=0):
    """A smooth picture in [-0.95, 0.95] as a function of real-valued columns: what both views sample."""
    return 0.55 * np.sin(0.35 * x + 0.9 * c + 0.23 * y + 0.5 * b) + 0.4 * np.cos(0.083 * x - 0.31 * y + 1.7 * c)


def magnitude(shape, seed):
    """|disparity| (B,1,H,W) float64: a slanted plane, a nearer box in its middle, 0.2 px of noise; scaled down for narrow frames."""
    g = S.rng(seed)
    B, _, H, W = shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    m = np.broadcast_to(2.0 + 0.03 * x + 0.05 * y, (B, 1, H, W)).copy()
    m[:, :, H // 4:H // 4 + H // 2, W // 3:W // 3 + W // 3] += 4.0
    return (m + g.normal(0.0, 0.2, m.shape)) * min(1.0, W / 64.0)


def holes(shape, seed):
    """A valid mask (B,1,H,W) with rectangular holes (about 8 % of the frame)."""
    g = S.rng(seed)
    B, _, H, W = shape
    mask = np.ones((B, 1, H, W), bool)
    for b in range(B):
        for _ in range(4):
            h, w = max(1, H // 6), max(1, W // 9)
            y0, x0 = int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1))
            mask[b, 0, y0:y0 + h, x0:x0 + w] = False
    return mask


def pair(shape, m, seed, target_view="left", noise=0.02):
    """(target, other) fp32: `other` is the texture, `target` the texture seen through the true magnitude m, plus a little noise."""
    g = S.rng(seed)
    B, C, H, W = shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    other = np.stack([np.stack([texture(c, y, x, b) for c in range(C)]) for b in range(B)])
    xs = x[None] - m[:, 0] if target_view == "left" else x[None] + m[:, 0]
    target = np.stack([np.stack([texture(c, y, xs[b], b) for c in range(C)]) for b in range(B)])
    return (target + g.normal(0.0, noise, target.shape)).astype(F32), other.astype(F32)


def scene(shape, seed, disp_sign="negative", target_view="left"):
    """(target, other, d, valid mask): the pair of `pair` with a map that is the true magnitude + 0.2 px of noise, and `holes`."""
    B, C, H, W = shape
    m = magnitude((B, 1, H, W), seed)
    target, other = pair(shape, m, seed + 1, target_view)
    noisy = (m + S.rng(seed + 2).normal(0.0, 0.2, m.shape)).astype(F32)
    return target, other, (-noisy if disp_sign == "negative" else noisy), holes(shape, seed + 3)


def consistent(shape, k, seed):
    """(target, other, d): other[x] = target[x + k] and m = k everywhere (left view, negative sign): rec == target where in."""
    g = S.rng(seed)
    B, C, H, W = shape
    target = g.uniform(-1.0, 1.0, shape).astype(F32)
    other = g.uniform(-1.0, 1.0, shape).astype(F32)
    if k < W:
        other[..., :W - k] = target[..., k:]
    return target, other, np.full((B, 1, H, W), -float(k), F32)


def builders(shape, seed=0):
    """name -> kwargs of `photometric_error` / `synthesize_view` (target, other, d, mask, mask_is_valid, disp_sign, target_view)."""
    B, C, H, W = shape
    g = S.rng(100 + seed)
    out = {}
    t, o, d, m = scene(shape, 11 + seed)
    out["scene"] = dict(target=t, other=o, d=d, mask=m)
    out["scene_no_mask"] = dict(target=t, other=o, d=d)
    t, o, d, m = scene(shape, 12 + seed, "positive")
    out["scene_positive_occlusion"] = dict(target=t, other=o, d=d, mask=~m, mask_is_valid=False, disp_sign="positive")
    t, o, d, m = scene(shape, 13 + seed, "negative", "right")
    out["scene_right"] = dict(target=t, other=o, d=d, mask=m, target_view="right")
    # one magnitude per sample, 0, 0.5, 1: the smallest frames keep valid pixels
    mag = np.empty((B, 1, H, W))
    for b in range(B):
        mag[b] = (0.0, 0.5, 1.0)[b % 3]
    t, o = pair(shape, mag, 14 + seed)
    out["small_m"] = dict(target=t, other=o, d=(-mag).astype(F32))
    # integer and half-integer magnitudes per pixel
    mag = g.integers(0, 7, (B, 1, H, W)) * 0.5 * min(1.0, W / 16.0)
    mag = np.round(mag * 2) / 2
    t, o = pair(shape, mag, 15 + seed)
    out["integer_half"] = dict(target=t, other=o, d=(-mag).astype(F32))
    # the upper rows (y <= H // 2): xr exactly 0 (m = x) in the even ones, m = 0 in the odd ones (xr = W-1 in the last column); right
    # view: xr exactly W-1 (m = W-1-x) and m = 0 (xr = 0 in the first column).  The lower rows: half a pixel outside the frame.
    x = np.broadcast_to(np.arange(W, dtype=np.float64), (B, 1, H, W))
    y = np.arange(H)[:, None]
    t, o = pair(shape, np.zeros((B, 1, H, W)), 16 + seed)
    mag = np.where(y > H // 2, x + 0.5, np.where(y % 2 == 0, x, 0.0))
    out["edges"] = dict(target=t, other=o, d=(-mag).astype(F32))
    mag = np.where(y > H // 2, W - 0.5 - x, np.where(y % 2 == 0, W - 1 - x, 0.0))
    out["edges_right"] = dict(target=t, other=o, d=mag.astype(F32), disp_sign="positive", target_view="right")
    # -0.0, NaN, +-inf and the wrong sign in the map
    t, o, d, m = scene(shape, 17 + seed)
    pool = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 1.5, -1.5, -0.5, 3e38, -3e38], dtype=F32)
    pick = g.random(d.shape) < 0.15
    d = d.copy()
    d[pick] = pool[g.integers(0, pool.size, int(pick.sum()))]
    out["special_disp"] = dict(target=t, other=o, d=d, mask=m)
    # NaN and inf in either picture, a few isolated pixels
    t, o, d, m = scene(shape, 18 + seed)
    t, o = t.copy(), o.copy()
    for arr, vals in ((t, (np.nan, np.inf)), (o, (np.nan, -np.inf))):
        n = max(2, arr.size // 150)
        idx = g.choice(arr.size, n, replace=False)
        arr.reshape(-1)[idx] = np.array(vals, F32)[g.integers(0, 2, n)]
    out["special_pictures"] = dict(target=t, other=o, d=d, mask=m)
    return out

