"""The masked median and the guided weighted median (csrc/median.hip): a vectorised numpy oracle of the closed form in
include/nndepth_amd.h, and the inputs of tests/test_median_cpu.py, tests/test_gpu_median.py and scripts/make_golden_median.py.

The oracle gathers the (2r+1)^2 taps of every pixel from a map of keys padded with the "not ok" sentinel, sorts them by key (a
stable argsort of the keys as int64), takes the integer cumulative sums of the weights in that order and picks the first tap at
which twice the sum reaches the total; taps of equal key are neighbours in the sorted order and copy the same bits, so the first
of a run that reaches the total is the tap of smallest key that does.  The guide distance is float32 throughout: every numpy
operation on float32 arrays is one rounded fp32 operation.  The loops of scripts/make_golden_median.py say the same pixel by
pixel, and test_median_cpu.py holds the two against each other.

Random inputs come from numpy's PCG64, seeded per case (speckle_cases.rng)."""
import numpy as np

import speckle_cases as S

F32 = np.float32
bits = S.bits
BAD = np.int64(0xFFFFFFFF)
GOLDEN_SHAPE = (2, 1, 9, 40)
SHAPES = [(1, 1, 1, 1), (1, 1, 1, 2), (2, 1, 3, 5), (3, 1, 6, 9), (2, 1, 9, 40)]  # + (2, 1, tileH + 3, 2 * tileW + 3), from the library
SMALL = (2, 1, 5, 7)  # smaller than the window of radius 7 in both directions


def keys_of(d) -> np.ndarray:
    """key(v) = bits(v) ^ (sign ? 0xFFFFFFFF : 0x80000000) as int64."""
    b = bits(d).astype(np.int64)
    return b ^ np.where(b & 0x80000000 != 0, np.int64(0xFFFFFFFF), np.int64(0x80000000))


def valid_of(shape, mask=None, mask_is_valid=True) -> np.ndarray:
    if mask is None:
        return np.ones(shape, bool)
    m = np.asarray(mask).reshape(shape) != 0
    return m if mask_is_valid else ~m


def range_weights(sigma, step=None, kind="exp"):
    """What nndepth_amd.geometry.range_weights states, written again: (uint16[256], float32 inv_step)."""
    step = sigma / 32 if step is None else step
    d = np.arange(256, dtype=np.float64) * step
    f = {"exp": lambda: np.exp(-d / sigma), "gauss": lambda: np.exp(-d * d / (2.0 * sigma * sigma)),
         "box": lambda: (d <= sigma).astype(np.float64)}[kind]()
    return np.floor(65535.0 * f + 0.5).astype(np.uint16), F32(1.0 / step)


def _taps(a, r, pad):
    """(B,H,W,(2r+1)^2): the window of every pixel of the (B,H,W) array, row-major, `pad` outside the frame."""
    B, H, W = a.shape
    p = np.full((B, H + 2 * r, W + 2 * r), pad, a.dtype)
    p[:, r:r + H, r:r + W] = a
    return np.stack([p[:, dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)], axis=-1)


def tap_weights(guide, r, inv_step, weights):
    """(B,H,W,(2r+1)^2) int64: weights[b] of every tap, whether ok or not."""
    guide = np.asarray(guide)
    assert guide.dtype == F32 and guide.ndim == 4 and 1 <= guide.shape[1] <= 4
    weights = np.asarray(weights)
    assert weights.dtype == np.uint16 and weights.shape == (256,)
    with np.errstate(all="ignore"):
        dist = None
        for c in range(guide.shape[1]):
            g = guide[:, c]
            a = np.abs(g[..., None] - _taps(g, r, F32(0)))
            dist = a if dist is None else dist + a
        assert dist.dtype == F32
        s = dist * F32(inv_step)
        assert s.dtype == F32
        b = np.where(s < F32(255.0), s, F32(255.0)).astype(np.int64)  # a NaN is not < 255
    return weights.astype(np.int64)[b]


def median_filter(d, radius=1, mask=None, mask_is_valid=True, guide=None, inv_step=None, weights=None, min_count=1, fill_invalid=False,
                  fill=0.0):
    """(filtered fp32, mask_out uint8 in the polarity of the mask, changed uint8)."""
    d = np.asarray(d)
    assert d.dtype == F32 and d.ndim == 4 and d.shape[1] == 1 and radius >= 1 and 1 <= min_count <= (2 * radius + 1) ** 2
    ok = valid_of(d.shape, mask, mask_is_valid) & np.isfinite(d)
    key = np.where(ok, keys_of(d), BAD)[:, 0]
    kt = _taps(key, radius, BAD)
    okt = kt != BAD
    w = okt.astype(np.int64) if guide is None else np.where(okt, tap_weights(guide, radius, inv_step, weights), 0)
    order = np.argsort(kt, axis=-1, kind="stable")
    ks, ws = np.take_along_axis(kt, order, -1), np.take_along_axis(w, order, -1)
    n, T = okt.sum(-1), w.sum(-1)
    first = np.argmax(2 * np.cumsum(ws, axis=-1) >= T[..., None], axis=-1)
    kstar = np.take_along_axis(ks, first[..., None], -1)[..., 0]
    vstar = (kstar ^ np.where(kstar & 0x80000000 != 0, np.int64(0x80000000), np.int64(0xFFFFFFFF))).astype(np.uint32).view(F32)
    produced = ((ok[:, 0] | bool(fill_invalid)) & (n >= min_count) & (T > 0))[:, None]
    out = np.where(produced, vstar[:, None], np.where(ok, d, F32(fill))).astype(F32)
    changed = (bits(out) != bits(d)) | (~ok & produced)
    return out, ((ok | produced) == bool(mask_is_valid)).astype(np.uint8), changed.astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------------- the inputs
def scene(shape, seed, disp_sign="positive"):
    """(d, valid mask): speckle_cases.scene (two slanted planes, a foreground box, salt, blobs) with about 20 % holes in runs."""
    d, mask, _ = S.scene(shape, seed)
    g = S.rng(seed + 1000)
    run = g.random(shape) < 0.04
    mask = mask & ~(run | np.roll(run, 1, 3) | np.roll(run, 2, 3))
    return (-d if disp_sign == "negative" else d), mask


def few_values(shape, seed):
    """(d, mask): 0.5 * U{-2..3}: many ties, and -0.0 among the zeros; 85 % valid."""
    g = S.rng(seed)
    d = (g.integers(-2, 4, shape) * 0.5).astype(F32)
    d[(d == 0) & (g.random(shape) < 0.5)] = -0.0
    return d, g.random(shape) < 0.85


def special(shape, seed):
    """(d, None): +-0.0, denormals, +-3e38 and, as invalid pixels, NaN and +-inf among ordinary values of both signs."""
    g = S.rng(seed)
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 3e38, -3e38, 1.5, -1.5, np.nan, np.inf, -np.inf, 2.0, -7.25, 1.1754944e-38],
                    dtype=F32)
    return pool[g.integers(0, pool.size, shape)], None


def masks(shape):
    """name -> valid mask: all invalid, a checkerboard, a single ok pixel."""
    _, _, H, W = shape
    y, x = np.mgrid[0:H, 0:W]
    single = np.zeros(shape, bool)
    single[-1, 0, H // 2, W // 2] = True
    return {"all_invalid": np.zeros(shape, bool), "checkerboard": np.broadcast_to(((x + y) % 2 == 0)[None, None], shape).copy(),
            "single": single}


def edge_guide(shape, C=3, seed=0, offset=1, nan=False):
    """(d, mask, guide): a disparity step at column W//2 and a guide (C channels, a little noise) whose step lies `offset`
    columns further right: the weighted median moves the disparity edge onto the guide's.  nan: NaNs and an inf in the guide."""
    B, _, H, W = shape
    g = S.rng(seed + 7 * C)
    x = np.arange(W)
    d = np.where(x < W // 2, 10.0, 30.0).astype(F32) + g.uniform(-0.25, 0.25, shape).astype(F32)
    guide = np.where(x < W // 2 + offset, 0.2, 0.8).astype(F32) + g.uniform(-0.02, 0.02, (B, C, H, W)).astype(F32)
    guide = guide.astype(F32)
    if nan:
        guide[g.random(guide.shape) < 0.05] = np.nan
        guide[0, 0, 0, 0] = np.inf
    return d, g.random(shape) < 0.9, guide


def tables():
    """name -> (uint16[256], inv_step): the three kinds, zeros after entry k, a constant table."""
    t = {k: range_weights(0.2, None, k) for k in ("exp", "gauss", "box")}
    cut = np.zeros(256, np.uint16)
    cut[:6] = [65535, 40000, 20000, 3, 2, 1]
    t["zeros_after_5"] = (cut, F32(16.0))
    t["constant"] = (np.full(256, 9, np.uint16), F32(50.0))
    return t


def builders(shape, seed=0):
    """name -> kwargs of `median_filter` without radius: every input above at `shape`."""
    T = tables()
    out = {}
    d, m = scene(shape, 11 + seed)
    out["scene"] = dict(d=d, mask=m)
    out["scene_negative_occlusion"] = dict(d=-d, mask=~m, mask_is_valid=False, fill=-2.0)
    d, m = few_values(shape, 12 + seed)
    out["few_values"] = dict(d=d, mask=m)
    out["special"] = dict(d=special(shape, 13 + seed)[0])
    for name, m in masks(shape).items():
        out[name] = dict(d=scene(shape, 14 + seed)[0], mask=m, fill_invalid=True, fill=5.0)
    for C in (1, 3):
        d, m, g = edge_guide(shape, C, seed)
        out[f"edge_c{C}"] = dict(d=d, mask=m, guide=g, weights=T["exp"][0], inv_step=T["exp"][1], fill_invalid=True)
    d, m, g = edge_guide(shape, 3, seed + 1, nan=True)
    out["guide_nan"] = dict(d=d, mask=m, guide=g, weights=T["gauss"][0], inv_step=T["gauss"][1])
    d, m, g = edge_guide(shape, 2, seed + 2)
    out["zeros_after_5"] = dict(d=few_values(shape, 15 + seed)[0], mask=m, guide=g, weights=T["zeros_after_5"][0], inv_step=T["zeros_after_5"][1],
                                fill_invalid=True, fill=-1.0)
    out["constant_table"] = dict(d=d, mask=m, guide=g, weights=T["constant"][0], inv_step=T["constant"][1])
    out["box_c4"] = dict(d=d, mask=m, guide=edge_guide(shape, 4, seed + 3)[2], weights=T["box"][0], inv_step=T["box"][1])
    return out
